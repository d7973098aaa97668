"""The fp16 + fp6 forward (hoig_amd/csrc/conv_f6.hip, the arithmetic of an eval forward) against a float64 emulation of its own arithmetic:
one table (conv_f6_reference.ROWS), one test body (docs/conv_f6_parity.md).

Per row: the entry point returns HOIG_OK, the route record names the launcher the row was shaped for, y agrees with
conv_f6_reference.conv_f6_ref under TOL_F6 (fp32 accumulation order is all that separates them) and with the float64 convolution under
1.5 x the emulation's own error + TOL_F6, which keeps a row honest should emulator and kernel ever be wrong in the same way.  Then the
weight records bit for bit, records and planes after the weights moved, and the shapes the launcher refuses."""
import ctypes

import pytest
import torch

import conv_f6_reference as F6
import conv_reference as R
from test_ops_gpu import PREC_BOUNDS

pytestmark = pytest.mark.gpu

TOL_F6 = F6.TOL_F6
# tanh and sigmoid rows: the forward tolerance tests/test_conv_routes_gpu.py gives its activation rows (the device's own tanh / exp), added
ACT_TOL = {'tanh': PREC_BOUNDS['bf16x3'][0], 'sigmoid': PREC_BOUNDS['bf16x3'][0]}
STATS_TOL = 1e-5            # the channel sums against float64 sums of the stored y (tests/test_conv_m16_gpu.py's bound)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _act(L, name):
    return {'none': L.ACT_NONE, 'relu': L.ACT_RELU, 'lrelu': L.ACT_LRELU, 'tanh': L.ACT_TANH, 'sigmoid': L.ACT_SIGMOID}[name]


def _cuda(t):
    return None if t is None else t.cuda()


def f6_entry(L, ops, wd, x, x2=None, bias=None, act='none', slope=0.2, in_scale=None, in_shift=None, in_relu_c0=0, y=None, stats=None,
             stride=1, k=3):
    """hoig_conv2d_fwd_f6_ex on CUDA tensors (wd: packed weight) -> (return code, y)."""
    B, H, W, C1 = x.shape
    Cg = C1 + (x2.shape[-1] if x2 is not None else 0)
    Co = wd.shape[0]
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    d = L.ConvDesc(B, H, W, Cg, Ho, Wo, Co, k, k, stride, k // 2, 0, _act(L, act), slope, L.PREC_F16F6)
    hi, _ = ops._packed_planes(wd, False, False)
    qh, ql = ops._f6_planes(wd)
    if y is None:
        y = torch.full((B, Ho, Wo, Co), float('nan'), device='cuda')
    rc = L.lib.hoig_conv2d_fwd_f6_ex(ctypes.byref(d), _p(x), C1 if x2 is not None else 0, _p(x2), _p(hi), _p(qh), _p(ql), _p(bias), _p(in_scale),
                                     _p(in_shift), in_relu_c0, _p(y), _p(stats), _st())
    return rc, y


def check_row(rid, report=None):
    """The one test body.  report: a dict that receives what was measured (tools/conv_f6_parity.py fills docs/conv_f6_parity.md with it)."""
    from hoig_amd import _lib as L, ops
    r, o = F6.ROW[rid], F6.operands(rid)
    report = {} if report is None else report
    ref, truth = F6.emulated(rid), F6.truth(rid)
    report['emu_vs_f64'] = F6.rel_err64(ref, truth)
    ops.set_precision('f16f6')
    old = ops.set_f6_min_tiles(1)
    try:
        x, wd, bias = o['x'].cuda(), ops.pack_weight(o['w'].cuda()), _cuda(o['bias'])
        x1, x2 = (x[..., :r.c1].contiguous(), x[..., r.c1:].contiguous()) if r.c1 else (x, None)
        stats = prefill = None
        if rid == 'stats':          # a known, different value per accumulator: the kernel must ADD to it, per image
            prefill = torch.arange(r.B * 2 * r.Co, dtype=torch.float64).reshape(r.B, 2, r.Co) * 0.25 - 7.0
            stats = prefill.cuda()
        with torch.no_grad():
            if r.via == 'conv2d':
                y = ops.conv2d(x, wd, bias, 1, 1, _act(L, r.act), 0.2)
            elif r.via == 'cat2':
                y = ops.conv2d_cat2(x1, x2, wd)
            else:
                rc, y = f6_entry(L, ops, wd, x1, x2, bias, r.act, 0.2, _cuda(o['in_scale']), _cuda(o['in_shift']), r.relu_c0, stats=stats)
                assert rc == L.OK, 'the launcher refused the row: %d' % rc
        report['route'] = L.last_route(L.ROUTE_FWD)
        torch.cuda.synchronize()
        assert report['route'] == r.route, '%s ran on %r, the row was shaped for %r' % (rid, report['route'], r.route)
        extra = ACT_TOL.get(r.act, 0.0)
        report['vs_emu'], report['vs_f64'] = F6.rel_err64(y, ref), F6.rel_err64(y, truth)
        report['bound_emu'], report['bound_f64'] = TOL_F6 + extra, 1.5 * report['emu_vs_f64'] + TOL_F6 + extra
        print('%s: %s, kernel vs emulation %.2e (bound %.1e), kernel vs float64 %.2e (bound %.2e), emulation vs float64 %.2e' % (
            rid, report['route'], report['vs_emu'], report['bound_emu'], report['vs_f64'], report['bound_f64'], report['emu_vs_f64']))
        assert TOL_F6 < report['emu_vs_f64'], 'TOL_F6 does not tell this row from float64'
        assert report['vs_emu'] < report['bound_emu'], (rid, report['vs_emu'], report['bound_emu'])
        assert report['vs_f64'] < report['bound_f64'], (rid, report['vs_f64'], report['bound_f64'])
        if stats is not None:
            added = stats.cpu() - prefill
            yd = y.double().cpu()
            report['stats'] = (F6.rel_err64(added[:, 0], yd.sum((1, 2))), F6.rel_err64(added[:, 1], (yd * yd).sum((1, 2))))
            print('stats: sum %.2e, sum of squares %.2e' % report['stats'])
            assert max(report['stats']) < STATS_TOL, report['stats']
        return report
    finally:
        ops.set_f6_min_tiles(old)
        ops.set_precision('f32')


@pytest.mark.parametrize('rid', [r.id for r in F6.ROWS])
def test_conv_f6_row(rid):
    check_row(rid)


def test_every_f6_route_has_a_row():
    from hoig_amd import _lib as L
    ids = {n for n in L.route_names() if n.startswith('fwd_f6_')}
    assert ids == {'fwd_f6_64', 'fwd_f6_128', 'fwd_f6_64_normin', 'fwd_f6_128_normin'}
    assert ids == {r.route for r in F6.ROWS}


# ---------------------------------------------------------------------------------------------------- the weight records
def _device_records(L, wd):
    co, ci = wd.shape[0], wd.shape[1]
    n = L.lib.hoig_f6_plane_bytes(co, 9, ci)
    assert n == 9 * (ci // 64) * co * F6.REC
    qh, ql = torch.zeros(n, dtype=torch.uint8, device='cuda'), torch.zeros(n, dtype=torch.uint8, device='cuda')
    assert L.lib.hoig_pack_conv_weight_f6(_p(wd), co, 9, ci, _p(qh), _p(ql), _st()) == L.OK
    torch.cuda.synchronize()
    return qh, ql


def _assert_records(got, w, what):
    """Codes and scale bytes equal conv_f6_reference.weight_records(w), -0 codes (0x20) included; pad bytes ignored."""
    for g, want, name in zip(got, F6.weight_records(w), ('hi', 'lo')):
        bad = F6.records_differ(g, want)
        assert bad == 0, '%s: %d of %d %s records differ from the emulation (%d with 0x20 read as 0x00)' % (
            what, bad, want.shape[0] * want.shape[1], name, F6.records_differ(g, want, allow_signed_zero=True))


@pytest.mark.parametrize('rid', ['one_tile', 'blocks3_tiles4', 'spread', 'dead_block', 'saturate', 'tiny', 'tiny_activations'])
def test_weight_records_bit_for_bit(rid):
    """tiny_activations: the activations of the `tiny` row passed through the packer as a weight (one output channel per pixel, / 256):
    the same split32 as the halo loader's, on values whose lo is an fp16 subnormal."""
    from hoig_amd import _lib as L, ops
    if rid == 'tiny_activations':
        w = (F6.operands('tiny')['x'].reshape(256, 64, 1, 1) / 256.0).repeat(1, 1, 3, 3).contiguous()
    else:
        w = F6.operands(rid)['w']
    _assert_records(_device_records(L, ops.pack_weight(w.cuda())), w, rid)


def _tree(seed=0):
    """A ParamTree that holds two eligible 3x3 weights of different shapes, with a bias and an ineligible weight between them."""
    import collections
    from hoig_amd import nn as hnn
    shapes = collections.OrderedDict([('a.weight', (64, 128, 3, 3)), ('a.bias', (64,)), ('thin.weight', (64, 32, 3, 3)),
                                      ('five.weight', (64, 64, 5, 5)), ('b.weight', (128, 64, 3, 3))])
    tree = hnn.ParamTree(shapes, 'cuda')
    g = torch.Generator().manual_seed(31 + seed)
    sd = collections.OrderedDict((k, torch.randn(s, generator=g) * (0.05 if len(s) == 4 else 1.0)) for k, s in shapes.items())
    tree.load_state_dict(sd)
    return tree, sd


def _tree_records_match(tree):
    torch.cuda.synchronize()
    for name, p in tree.P.items():
        planes = tree.packed_f6(p)
        assert (planes is not None) == (name in ('a.weight', 'b.weight')), name
        if planes is not None:
            _assert_records(planes, p.detach().cpu(), name)


def test_param_tree_records_bit_for_bit():
    """hoig_pack_conv_weights_f6_all: every eligible weight of the tree in one launch, each at its own byte offset."""
    from hoig_amd import ops
    tree, sd = _tree()
    ops.set_precision('f16f6')
    try:
        _tree_records_match(tree)
        assert torch.equal(tree.P['a.weight'].detach().cpu(), sd['a.weight'])
    finally:
        ops.set_precision('f32')


@pytest.mark.parametrize('how', ['adam_step', 'adam_step_unfused', 'load_state_dict'])
def test_records_and_planes_follow_the_weights(how):
    """A fresh fp16 plane over stale fp6 records (or the reverse) is a 1e-4-class error that no other test sees: after the weights moved
    -- FusedAdam.step, which re-packs the fp16 planes in its own launch (and, unfused, leaves them to the next forward), or
    load_state_dict -- the records equal weight_records of the NEW weights, and a convolution on them agrees with the emulation."""
    from hoig_amd import _lib as L, nn as hnn, ops
    tree, _ = _tree(1)
    o = F6.operands('cat_64_64')                    # (2, 8, 32, 128): an input for a.weight
    x = o['x'].cuda()
    ops.set_precision('f16f6')
    old = ops.set_f6_min_tiles(1)
    try:
        w = tree.P['a.weight']
        with torch.no_grad():
            y0 = ops.conv2d(x, w, None, 1, 1)       # (planes and records of the old weights exist from here on)
        assert L.last_route(L.ROUTE_FWD) == 'fwd_f6_64'
        assert F6.rel_err64(y0, F6.conv_f6_ref(o['x'], w.detach().cpu())) < TOL_F6
        before = w.detach().cpu().clone()
        if how == 'load_state_dict':
            tree.load_state_dict(_tree(2)[1])
        else:
            opt = hnn.FusedAdam(tree, lr=3e-3)
            opt.fuse_planes = how == 'adam_step'
            tree.flat_grad.copy_(torch.randn(tree.flat.numel(), generator=torch.Generator().manual_seed(8)))
            opt.step()
        after = w.detach().cpu().clone()
        assert (after - before).abs().max().item() > 1e-3, 'the weights did not move'
        _tree_records_match(tree)
        with torch.no_grad():
            y1 = ops.conv2d(x, w, None, 1, 1)
        assert L.last_route(L.ROUTE_FWD) == 'fwd_f6_64'
        e_new, e_old = F6.rel_err64(y1, F6.conv_f6_ref(o['x'], after)), F6.rel_err64(y1, F6.conv_f6_ref(o['x'], before))
        print('%s: against the new weights %.2e, against the old ones %.2e' % (how, e_new, e_old))
        assert e_new < TOL_F6 and e_old > 1e-2
    finally:
        ops.set_f6_min_tiles(old)
        ops.set_precision('f32')


@pytest.mark.parametrize('captured_in', ['f32', 'bf16x3:f16x2', 'f16f6'])
def test_records_follow_weights_that_a_replayed_graph_moved(captured_in):
    """An eval forward in the f16f6 arithmetic between replays of the captured training step.  The replay moves the weights on the
    device, and the host only hears of it through FusedAdam.replayed(): whatever the graph did not re-pack itself must be re-made for
    the next eval forward -- the fp6 records (no graph but an f16f6 one packs them) and, after an f32 capture, the fp16 planes too,
    which the first eval forward allocates.  Records bit for bit, and ops.conv2d against the emulation on the NEW weights, which
    needs the plane and the records both.  (replayed() left the tree's version alone: the records of the first eval stayed
    "current" for good -- under fresh fp16 planes the whole hi * lo term was wrong, 2e-4 per layer.)"""
    from common import product_trainer
    from hoig_amd import _lib as L, ops
    from hoig_amd.models import trainer as T
    old = ops.set_f6_min_tiles(1)
    try:
        ops.set_precision(captured_in)
        m = product_trainer('generator_spade_attn', 2, 64, hip_graph=True)
        for _ in range(T._GRAPH_WARMUP + 1):
            m.optimize_parameters()
        assert [k for k, g in m._graphs.items() if g['graphs'] is not None], 'the step was not captured'
        G = m._G
        name, w = next((k, v) for k, v in G.P.items() if v.dim() == 4 and v.shape[0] == 64 and v.shape[1] % 64 == 0
                       and tuple(v.shape[2:]) == (3, 3) and not getattr(v, '_hoig_transposed', False))
        x = torch.randn(1, 8, 32, w.shape[1], generator=torch.Generator().manual_seed(6))

        def eval_forward(what):
            ops.set_precision('f16f6')
            try:
                torch.cuda.synchronize()
                now = w.detach().cpu().clone()
                _assert_records(G.packed_f6(w), now, '%s, %s' % (name, what))
                with torch.no_grad():
                    y = ops.conv2d(x.cuda(), w, None, 1, 1)
                assert L.last_route(L.ROUTE_FWD) == 'fwd_f6_64'
                err = F6.rel_err64(y, F6.conv_f6_ref(x, now))
                print('%s, %s: ops.conv2d against the emulation on the current weights %.2e' % (captured_in, what, err))
                assert err < TOL_F6, (what, err)
                return now
            finally:
                ops.set_precision(captured_in)

        before = eval_forward('after the capture')
        for rnd in range(2):                        # (twice: the planes the first eval forward made must not pass for current either)
            m.optimize_parameters()                 # a replay
            m.optimize_parameters()
            assert len([k for k, g in m._graphs.items() if g['graphs'] is not None]) == 1
            now = eval_forward('after replays, round %d' % rnd)
            assert not torch.equal(now, before)
            before = now
    finally:
        ops.set_f6_min_tiles(old)
        ops.set_precision('f32')


# ---------------------------------------------------------------------------------------------------- refusals
# what, shape changes against the base (B 2, 64 -> 64, 8 x 32, 3x3 stride 1), return code, the three-term route ops.conv2d lands on
# (maps this small are below every halo kernel's launch size: the 16x16x32 implicit GEMM takes them).  None for the two refusals that
# no operator can provoke: conv2d_cat2 takes the two-tensor kernel only with C1 % 64 == 0 (and concatenates otherwise, which is an
# ordinary conv2d), conv2d_after_norm returns None unless C1 % 32 == 0 and passes in_relu_c0 = C1.
REFUSALS = [
    ('H=12', dict(H=12), 'EUNSUPPORTED', 'fwd_igemm_m16_64x64'),
    ('W=48', dict(W=48), 'EUNSUPPORTED', 'fwd_igemm_m16_64x64'),
    ('Ci=96', dict(Ci=96), 'EUNSUPPORTED', 'fwd_igemm_m16_64x64'),
    ('Co=96', dict(Co=96), 'EUNSUPPORTED', 'fwd_igemm_m16_64x128'),
    ('stride=2', dict(stride=2), 'EUNSUPPORTED', 'fwd_igemm_m16_64x64'),
    ('5x5', dict(k=5), 'EUNSUPPORTED', 'fwd_igemm_m16_64x64'),
    ('C1=16', dict(c1=16), 'EINVAL', None),
    ('in_relu_c0=16', dict(relu_c0=16), 'EUNSUPPORTED', None),
    ('default_min_tiles', dict(min_tiles=None), 'EUNSUPPORTED', 'fwd_igemm_m16_64x64'),
]


@pytest.mark.parametrize('what,change,code,x3_route', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_shapes_touch_nothing_and_run_on_three_terms(what, change, code, x3_route):
    """launch_f6 refuses every shape outside its tiling BEFORE it launches or records anything: the return code, a prefilled output left
    as it was, the forward route record unchanged.  Through ops.conv2d the same layer then runs on a three-term launcher, by id, at the
    three-term error."""
    from hoig_amd import _lib as L, ops
    s = dict(B=2, Ci=64, Co=64, H=8, W=32, stride=1, k=3, c1=0, relu_c0=0, min_tiles=1)
    s.update(change)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(s['B'], s['H'], s['W'], s['Ci'], generator=g)
    w = torch.randn(s['Co'], s['Ci'], s['k'], s['k'], generator=g) * 0.05
    ops.set_precision('f16f6')
    old = ops.set_f6_min_tiles(1)
    try:
        assert old == 192, 'the default threshold is 192 workgroups'
        # a launch the kernel takes, so that the record holds a known id
        ok = F6.operands('one_tile')
        rc, _ = f6_entry(L, ops, ops.pack_weight(ok['w'].cuda()), ok['x'].cuda())
        assert rc == L.OK and L.last_route(L.ROUTE_FWD) == 'fwd_f6_64'
        before = tuple(L.last_route(i) for i in range(3))
        ops.set_f6_min_tiles(s['min_tiles'] or old)
        # the refused call: dummy planes and records large enough for any of these shapes (nothing may read them)
        xd = x.cuda()
        x1, x2 = (xd[..., :s['c1']].contiguous(), xd[..., s['c1']:].contiguous()) if s['c1'] else (xd, None)
        Ho, Wo = (s['H'] - 1) // s['stride'] + 1, (s['W'] - 1) // s['stride'] + 1
        d = L.ConvDesc(s['B'], s['H'], s['W'], s['Ci'], Ho, Wo, s['Co'], s['k'], s['k'], s['stride'], s['k'] // 2, 0, L.ACT_NONE, 0.0, L.PREC_F16F6)
        planes = [torch.zeros(1 << 20, dtype=torch.uint8, device='cuda') for _ in range(3)]
        fold = torch.ones(2, s['B'], s['Ci'], device='cuda') if s['relu_c0'] else None
        y = torch.full((s['B'], Ho, Wo, s['Co']), 3.5, device='cuda')
        rc = L.lib.hoig_conv2d_fwd_f6_ex(ctypes.byref(d), _p(x1), s['c1'], _p(x2), _p(planes[0]), _p(planes[1]), _p(planes[2]), None,
                                         _p(fold[0]) if fold is not None else None, _p(fold[1]) if fold is not None else None, s['relu_c0'],
                                         _p(y), None, _st())
        torch.cuda.synchronize()
        assert rc == getattr(L, code), (what, rc)
        assert (y == 3.5).all().item(), 'a refused launch wrote its output'
        assert tuple(L.last_route(i) for i in range(3)) == before, 'a refused launch changed the route record'
        if x3_route is None:
            return
        with torch.no_grad():
            y = ops.conv2d(xd, ops.pack_weight(w.cuda()), None, s['stride'], s['k'] // 2)
        route = L.last_route(L.ROUTE_FWD)
        err = F6.rel_err64(y, R.conv_ref(x, w, None, s['stride'], s['k'] // 2))
        print('%s: ops.conv2d ran on %s, %.2e against float64' % (what, route, err))
        assert route == x3_route, (what, route)
        assert err < 5e-6, 'not the three-term arithmetic (tests/test_ops_gpu.py::test_conv_f16f6_forward draws the same line)'
    finally:
        ops.set_f6_min_tiles(old)
        ops.set_precision('f32')
