"""The composite convolution autograd functions -- ops.conv_heads, ops.conv2d_padded_in, ops.conv2d_pair, the norm -> convolution
hand-off of split planes, a live bias under a frozen weight -- forward and every gradient against the float64 reference of
tests/conv_reference.py, with the routes their backward took (docs/conv_backward_parity.md)."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import conv_reference as R
import gpu_util
from test_conv_routes_gpu import MIXED, MODES16, _EXACT
from test_ops_gpu import PREC_BOUNDS, TOL as TOL32

pytestmark = pytest.mark.gpu


def _bounds(mode, emu=None, routes=None):
    """{'y', 'dx', 'dw'} -> bound: PREC_BOUNDS of the mode's forward / backward arithmetic, the three-term bound for a pass that ran on
    an exact-fp32 launcher, 4 x the reference's rounding emulation where that is larger."""
    parts = mode.split(':')
    fm, bm = parts[0], parts[-1]
    out = {'y': PREC_BOUNDS[fm][0], 'dx': PREC_BOUNDS[bm][1], 'dw': PREC_BOUNDS[bm][2]}
    for k, idx in (('y', 0), ('dx', 1), ('dw', 2)):
        if routes and (routes.get(k) or '').startswith(_EXACT):
            out[k] = PREC_BOUNDS['bf16x3'][idx]
        elif emu is not None:
            out[k] = max(out[k], 4.0 * emu[k])
    return out


def _tree(shapes, seed, scale=0.05):
    from hoig_amd import nn as hnn
    tree = hnn.ParamTree(shapes, torch.device('cuda'), {}, {})
    with torch.no_grad():
        tree.flat.copy_((torch.randn(tree.flat.shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda())
    tree.version += 1
    return tree


def _route_hook(x, seen):
    """The record is per host thread and the autograd engine runs a backward on its device thread: read it there, when dx arrives."""
    from hoig_amd import _lib as L
    x.register_hook(lambda g: seen.update(dx=L.last_route(L.ROUTE_DGRAD), dw=L.last_route(L.ROUTE_WGRAD)))


MEASURED = []          # (test id, tensor, error, bound): what docs/conv_backward_parity.md quotes


def _lt(a, ref, bound, what):
    e = gpu_util.rel_err(a, ref)
    MEASURED.append((os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0], what, e, bound))
    assert e < bound, (what, e, bound)
    return e


# ------------------------------------------------------------------------------------------------------------------ conv_heads
_HEAD_ACTS = {'tanh': torch.tanh, 'sigmoid': torch.sigmoid, 'none': lambda t: t}


@functools.lru_cache(maxsize=None)
def _heads_reference(shape, acts, drop_last):
    B, H, W, Ci = shape
    g = torch.Generator().manual_seed(40 + H)
    x = torch.randn(B, H, W, Ci, generator=g)
    w = torch.randn(5, Ci, 7, 7, generator=g) * (49 * Ci) ** -0.5
    gys = [torch.randn(B, H, W, n, generator=g) for n in (3, 1, 1)]
    pre = R.conv_ref(x, w, None, 1, 3).requires_grad_(True)
    outs, off = [], 0
    for n, a in zip((3, 1, 1), acts):
        outs.append(_HEAD_ACTS[a](pre[..., off:off + n]))
        off += n
    used = list(zip(outs, gys))[:2 if drop_last else 3]
    gpre, = torch.autograd.grad([o for o, _ in used], [pre], [gy.double() for _, gy in used])
    dx, dw, _ = R.conv_grads_ref(x, w, None, gpre, 1, 3)
    return dict(x=x, w=w, gys=gys, outs=[o.detach() for o in outs], dx=dx, dw=dw, gpre=gpre)


@pytest.mark.parametrize('mode', MODES16)
@pytest.mark.parametrize('acts,drop_last', [(('tanh', 'sigmoid', 'none'), False), (('tanh', 'none', 'none'), False),
                                            (('tanh', 'sigmoid', 'none'), True)])
@pytest.mark.parametrize('shape', [(2, 16, 32, 64), (1, 10, 24, 64)])
def test_conv_heads_backward(shape, acts, drop_last, mode):
    """One fused 7x7 convolution, a per-head activation; (2, 16, 32, 64) is on the 4 x 32 tiles of the thin-channel MFMA kernels,
    (1, 10, 24, 64) is not and takes the fp32 fallbacks (5 outputs: neither the <= 4-channel direct kernel nor the 16-bit one).
    drop_last: the third head's output is unused, its gradient arrives as None."""
    from hoig_amd import _lib as L, ops
    ref = _heads_reference(shape, acts, drop_last)
    code = {'tanh': L.ACT_TANH, 'sigmoid': L.ACT_SIGMOID, 'none': L.ACT_NONE}
    ops.set_precision(mode)
    try:
        gpu_util.poison_free_memory()
        xd = ref['x'].cuda().requires_grad_(True)
        wd = ops.pack_weight(ref['w'].cuda()).requires_grad_(True)
        seen = {}
        _route_hook(xd, seen)
        outs = ops.conv_heads(xd, wd, (3, 1, 1), [code[a] for a in acts])
        assert L.last_route(L.ROUTE_FWD) == 'fwd_head7'
        used = list(zip(outs, ref['gys']))[:2 if drop_last else 3]
        torch.autograd.backward([o for o, _ in used], [gy.cuda() for _, gy in used])
        torch.cuda.synchronize()
        tiled = shape[1] % 4 == 0 and shape[2] % 32 == 0
        assert seen == ({'dx': 'dgrad_thin', 'dw': 'wgrad_thin_out_direct'} if tiled else
                        {'dx': 'dgrad_igemm_f32_64x64', 'dw': 'wgrad_f32_32x128'}), seen
        emu = R.rounded_operand_error((ref['x'], ref['w'], None, ref['gpre'].float(), 1, 3, False), mode)
        b = _bounds(mode, emu, seen)
        for o, want in zip(outs, ref['outs']):
            _lt(o, want, b['y'], 'head')
        _lt(xd.grad, ref['dx'], b['dx'], 'dx')
        _lt(wd.grad, ref['dw'], b['dw'], 'dw')
    finally:
        ops.set_precision('f32')


# ------------------------------------------------------------------------------------------------------------------ conv2d_padded_in
@functools.lru_cache(maxsize=None)
def _padded_in_reference(Ci, H, W):
    """Operands whose float64 pre-activations all keep a distance from zero that the three-term forward cannot cross (LeakyReLU's
    derivative jumps there: a flipped mask would be the reference's conditioning, not the kernel's error): the first seed from 60
    upwards with min |pre| > 4 x the emulated forward error, decided from the reference alone."""
    for seed in range(60, 140):
        c = R.Case(2, Ci, 64, H, W, 4, 2, 1, False, True, 'lrelu', 0.2, seed)
        x, w, b, gy = R.make_case(c)
        pre = R.conv_ref(x, w, b, 2, 1)
        fwd_err = R.rounded_operand_error((x, w, None, gy, 2, 1, False), 'bf16x3')['y'] * pre.abs().max().item()
        if pre.abs().min().item() > 4.0 * fwd_err:
            break
    else:
        raise AssertionError('no well-conditioned seed')
    y = R.conv_ref(x, w, b, 2, 1, False, 'lrelu', 0.2)
    dx, dw, db = R.conv_grads_ref(x, w, b, gy, 2, 1, False, 'lrelu', 0.2)
    return dict(x=x, w=w, b=b, gy=gy, y=y, dx=dx, dw=dw, db=db)


@pytest.mark.parametrize('mode', MODES16)
@pytest.mark.parametrize('H,W', [(16, 24), (9, 9)])
@pytest.mark.parametrize('Ci', [19, 24])
def test_conv2d_padded_in(Ci, H, W, mode):
    """The discriminator's first layer: 19 / 24 input channels zero-padded to 32 for the 16-bit kernels.  x.grad has Ci channels, the flat
    gradients of weight and bias are the unpadded reference's -- and twice that after a second backward into the same buffers."""
    from hoig_amd import _lib as L, ops
    ref = _padded_in_reference(Ci, H, W)
    ops.set_precision(mode)
    try:
        gpu_util.poison_free_memory()
        tree = _tree({'c.weight': (64, Ci, 4, 4), 'c.bias': (64,)}, 1)
        w, b = tree.P['c.weight'], tree.P['c.bias']
        with torch.no_grad():
            w.copy_(ref['w'].cuda())
            b.copy_(ref['b'].cuda())
        tree.version += 1
        emu = R.rounded_operand_error((ref['x'], ref['w'], None, ref['gy'], 2, 1, False), mode)
        bd = _bounds(mode, emu)
        for n in (1, 2):
            xd = ref['x'].cuda().requires_grad_(True)
            seen = {}
            _route_hook(xd, seen)
            y = ops.conv2d_padded_in(xd, w, b, 2, 1, L.ACT_LRELU, 0.2)
            y.backward(ref['gy'].cuda())
            ops.join_wgrad_streams()
            torch.cuda.synchronize()
            assert seen['dw'] == 'wgrad_bf16_64', seen
            assert xd.grad.shape == ref['x'].shape
            _lt(y, ref['y'], bd['y'], 'y')
            _lt(xd.grad, ref['dx'], bd['dx'], 'dx')
            _lt(w.grad, n * ref['dw'], bd['dw'], 'dw after %d backward(s)' % n)
            _lt(b.grad, n * ref['db'], bd['dw'], 'db after %d backward(s)' % n)
    finally:
        ops.set_precision('f32')


# ------------------------------------------------------------------------------------------------------------------ conv2d_pair
@functools.lru_cache(maxsize=None)
def _pair_reference(Ci, fork):
    """Two problems of one descriptor (6 x 32 x 64, Ci -> 128, 3x3): the smallest shape pair_ok accepts."""
    out = []
    for k in (0, 1):
        c = R.Case(6, Ci, 128, 32, 64, 3, 1, 1, False, True, 'none', 0.0, 80 + k)
        x, w, b, gy = R.make_case(c)
        gx = torch.randn(x.shape, generator=torch.Generator().manual_seed(90 + k))
        dx, dw, db = R.conv_grads_ref(x, w, b, gy, 1, 1)
        out.append(dict(x=x, w=w, b=b, gy=gy, gx=gx, y=R.conv_ref(x, w, b, 1, 1), y_nobias=R.conv_ref(x, w, None, 1, 1), dx=dx, dw=dw, db=db))
    return out


_PAIR_ROUTES = {'y': 'fwd_halo3_m16_128_pair', 'dx': 'dgrad_halo3_m16_128_split_pair', 'dw': 'wgrad_dma_pair'}


@pytest.mark.parametrize('variant', ['dead_bias', 'live_bias', 'fork_both', 'fork_first_only', 'ci32_fallback', 'frozen_weight',
                                     'frozen_weight_live_bias'])
def test_conv2d_pair(variant):
    """Grouped launches against float64 (until now only against two single launches).  pair_ok asks for a two-term backward, so the mode
    is bf16x3:f16x2; under plain bf16x3 it declines, which is asserted."""
    from hoig_amd import _lib as L, ops
    Ci = 32 if variant == 'ci32_fallback' else 128
    fork = variant.startswith('fork')
    live = variant in ('live_bias', 'frozen_weight_live_bias')
    frozen = variant.startswith('frozen')
    ra, rb = _pair_reference(Ci, fork)
    prev = L.set_tuning('pair', 1)
    ops.set_precision(MIXED)
    try:
        gpu_util.poison_free_memory()
        tree = _tree({'a.weight': (128, Ci, 3, 3), 'a.bias': (128,), 'b.weight': (128, Ci, 3, 3), 'b.bias': (128,)}, 2)
        P = tree.P
        with torch.no_grad():
            for k, r in (('a', ra), ('b', rb)):
                P[k + '.weight'].copy_(r['w'].cuda())
                P[k + '.bias'].copy_(r['b'].cuda())
        tree.version += 1
        if frozen:
            P['b.weight'].requires_grad_(False)
        xa, xb = ra['x'].cuda().requires_grad_(True), rb['x'].cuda().requires_grad_(True)
        ops.set_precision('bf16x3')
        assert not ops.pair_ok(xa, xb, P['a.weight'], P['b.weight'])
        ops.set_precision(MIXED)
        assert ops.pair_ok(xa, xb, P['a.weight'], P['b.weight'])
        seen = {}
        _route_hook(xa, seen)
        ba, bb = (P['a.bias'], P['b.bias']) if live else (None, None)
        out = ops.conv2d_pair(xa, xb, P['a.weight'], P['b.weight'], ba, bb, dead_bias=not live, fork=fork)
        seen['y'] = L.last_route(L.ROUTE_FWD)
        outs, grads = [out[0], out[1]], [ra['gy'].cuda(), rb['gy'].cuda()]
        if fork:
            outs.append(out[2]); grads.append(ra['gx'].cuda())
            if variant == 'fork_both':
                outs.append(out[3]); grads.append(rb['gx'].cuda())
        torch.autograd.backward(outs, grads)
        ops.join_wgrad_streams()
        ops.check_split_grads_consumed()
        torch.cuda.synchronize()
        want = dict(_PAIR_ROUTES)
        if variant == 'ci32_fallback':
            want['dx'] = 'dgrad_igemm_f32_128x32'             # (32 gathered outputs: no packed-plane kernel, grouped or single)
        if frozen:
            want['dw'] = 'wgrad_dma'                          # one problem: the single launch
        assert seen == want, seen
        b = _bounds(MIXED, routes=seen)
        for r, y, x, k in ((ra, out[0], xa, 'a'), (rb, out[1], xb, 'b')):
            _lt(y, r['y'] if live else r['y_nobias'], b['y'], 'y' + k)
            dx = r['dx']
            if fork and (k == 'a' or variant == 'fork_both'):
                dx = dx + r['gx'].double()
            _lt(x.grad, dx, b['dx'], 'dx' + k)
            if frozen and k == 'b':
                assert float(P['b.weight'].grad.abs().max()) == 0.0
            else:
                _lt(P[k + '.weight'].grad, r['dw'], b['dw'], 'dw' + k)
            if live:
                _lt(P[k + '.bias'].grad, r['db'], b['dw'], 'db' + k)
            else:
                assert float(P[k + '.bias'].grad.abs().max()) == 0.0
    finally:
        ops.set_precision('f32')
        L.set_tuning('pair', prev)


# ------------------------------------------------------------------------------------------------------------------ norm -> convolution
@pytest.mark.parametrize('kind', ['in_affine_residual', 'spade'])
def test_norm_hands_the_convolution_split_planes_against_float64(kind):
    """conv3x3 (flat weight, dead bias, 32 -> 128, 2 x 8 x 32) -> instance norm with affine + residual, or the fused SPADE norm, no
    activation: the norm's backward writes its dx as bf16 hi | lo planes and the convolution's backward takes them (the weight gradient
    runs on the LDS-DMA kernel, no offer is left over) -- against float64 convolution + instance norm."""
    from hoig_amd import _lib as L, ops
    B, H, W, Ci, Co = 2, 8, 32, 32, 128
    g = torch.Generator().manual_seed(70)
    x = torch.randn(B, H, W, Ci, generator=g)
    w = torch.randn(Co, Ci, 3, 3, generator=g) * (9 * Ci) ** -0.5
    nw, nb = torch.randn(Co, generator=g), torch.randn(Co, generator=g)
    res = torch.randn(B, H, W, Co, generator=g)
    gb = torch.randn(B, H, W, 2 * Co, generator=g) * 0.3
    gout = torch.randn(B, H, W, Co, generator=g)
    # float64: the convolution through the reference, the norm through torch's instance norm on doubles
    yc = R.conv_ref(x, w, None, 1, 1).requires_grad_(True)
    ycn = yc.permute(0, 3, 1, 2)
    nwd, nbd, gbd = nw.double().requires_grad_(True), nb.double().requires_grad_(True), gb.double().requires_grad_(True)
    if kind == 'in_affine_residual':
        z = res.double() + F.instance_norm(ycn, weight=nwd, bias=nbd, eps=1e-5).permute(0, 2, 3, 1)
    else:
        z = F.instance_norm(ycn, eps=1e-5).permute(0, 2, 3, 1) * (1 + gbd[..., :Co]) + gbd[..., Co:]
    gyc, gnw, gnb, ggb = torch.autograd.grad(z, [yc, nwd, nbd, gbd], gout.double(), allow_unused=True)
    dx_ref, dw_ref, _ = R.conv_grads_ref(x, w, None, gyc, 1, 1)
    ops.set_precision(MIXED)
    try:
        assert L.lib.hoig_set_tuning(b'split_grads', -1) == 1
        gpu_util.poison_free_memory()
        tree = _tree({'c.weight': (Co, Ci, 3, 3), 'n.weight': (Co,), 'n.bias': (Co,)}, 3)
        P = tree.P
        with torch.no_grad():
            P['c.weight'].copy_(w.cuda()); P['n.weight'].copy_(nw.cuda()); P['n.bias'].copy_(nb.cuda())
        tree.version += 1
        xd = x.cuda().requires_grad_(True)
        gbd_d = gb.cuda().requires_grad_(True)
        seen = {}
        _route_hook(xd, seen)
        y = ops.conv2d(xd, P['c.weight'], None, 1, 1, dead_bias=True)
        assert getattr(y, '_hoig_split_grad', None) is not None
        if kind == 'in_affine_residual':
            zd = ops.instance_norm(y, P['n.weight'], P['n.bias'], residual=res.cuda())
        else:
            zd = ops.spade_norm_fused(y, gbd_d)
        zd.backward(gout.cuda())
        ops.join_wgrad_streams()
        ops.check_split_grads_consumed()
        torch.cuda.synchronize()
        assert seen['dw'] == 'wgrad_dma', seen
        b = _bounds(MIXED, routes=seen)
        _lt(zd, z.detach(), PREC_BOUNDS['bf16x3'][0], 'z')
        _lt(xd.grad, dx_ref, b['dx'], 'dx')
        _lt(P['c.weight'].grad, dw_ref, b['dw'], 'dw')
        if kind == 'in_affine_residual':
            _lt(P['n.weight'].grad, gnw, PREC_BOUNDS['bf16x3'][1], 'dgamma')
            _lt(P['n.bias'].grad, gnb, PREC_BOUNDS['bf16x3'][1], 'dbeta')
        else:
            _lt(gbd_d.grad, ggb, PREC_BOUNDS['bf16x3'][1], 'd[gamma|beta]')
    finally:
        ops.set_precision('f32')


# ------------------------------------------------------------------------------------------------------------------ frozen weight, live bias
@pytest.mark.parametrize('mode', MODES16 + ('f32',))
@pytest.mark.parametrize('flat', [False, True])
@pytest.mark.parametrize('act', ['none', 'tanh'])
def test_bias_gradient_under_a_frozen_weight(act, flat, mode):
    """w.requires_grad = False, b.requires_grad = True: no weight-gradient launch follows, the bias gradient is the column sum of the
    (activation-backward) gradient on its own -- hoig_colsum_accum / hoig_act_bwd_colsum.  (It used to come out as zero.)"""
    from hoig_amd import _lib as L, ops
    c = R.Case(2, 64, 128, 9, 9, 4, 1, 1, False, True, act, 0.2, 21)
    x, w, b, gy = R.make_case(c)
    y_ref = R.conv_ref(x, w, b, 1, 1, False, act)
    dx_ref, _, db_ref = R.conv_grads_ref(x, w, b, gy, 1, 1, False, act)
    code = {'none': L.ACT_NONE, 'tanh': L.ACT_TANH}[act]
    ops.set_precision(mode)
    try:
        gpu_util.poison_free_memory()
        if flat:
            tree = _tree({'c.weight': (128, 64, 4, 4), 'c.bias': (128,)}, 4)
            wd, bd = tree.P['c.weight'], tree.P['c.bias']
            with torch.no_grad():
                wd.copy_(w.cuda()); bd.copy_(b.cuda())
            tree.version += 1
            wd.requires_grad_(False)
        else:
            wd, bd = ops.pack_weight(w.cuda()), b.cuda().requires_grad_(True)
        bound = TOL32 if mode == 'f32' else PREC_BOUNDS['bf16x3'][2]          # (a column sum in fp32, whatever the mode)
        bdx = TOL32 if mode == 'f32' else _bounds(mode)['dx']
        for n in (1, 2):
            xd = x.cuda().requires_grad_(True)
            y = ops.conv2d(xd, wd, bd, 1, 1, code, 0.2)
            y.backward(gy.cuda())
            ops.join_wgrad_streams()
            torch.cuda.synchronize()
            _lt(xd.grad, dx_ref, bdx, 'dx')
            if flat:
                _lt(bd.grad, n * db_ref, bound, 'db after %d backward(s)' % n)
                assert float(wd.grad.abs().max()) == 0.0
            else:
                _lt(bd.grad, n * db_ref, bound, 'db after %d backward(s)' % n)      # (autograd sums the returned gradients)
    finally:
        ops.set_precision('f32')
