"""The Adam kernels against float64 (tests/adam_reference.py, docs/optimizer_parity.md): every entry point on raw buffers, one step at a
time from shared inputs, measured in units of what fp32 arithmetic itself costs on the row (the reference's fp32 twin); slices that start
off a 16-byte boundary; FusedAdam over a tree whose layout exercises the table builder, on its routes (fused, two launches, slices)."""
import ctypes

import numpy as np
import pytest
import torch

import adam_reference as A

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025]
BIG = 2097152 + 3 * 1024 + 3           # hoig_stream_grid stops at 2048 workgroups of 256 float4s: a second pass for some, and a tail
BETAS = (0.5, 0.999)
SENT = -7.25                           # fills the margins around every buffer
MARGIN = 8                             # elements


def _L():
    from hoig_amd import _lib
    return _lib


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buf(object):
    """n floats on the device between two margins of SENT, starting `off` elements past a 256-byte boundary."""

    def __init__(self, a, off=0):
        self.n, self.lo = len(a), MARGIN + off
        self.t = torch.full((self.n + 2 * MARGIN + 4,), SENT, dtype=torch.float32, device='cuda')
        assert self.t.data_ptr() % 256 == 0
        self.t[self.lo:self.lo + self.n] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        self.ptr = self.t.data_ptr() + 4 * self.lo

    def get(self):
        x = self.t.cpu().numpy()
        assert (x[:self.lo] == SENT).all() and (x[self.lo + self.n:] == SENT).all(), 'a store outside the slice'
        return x[self.lo:self.lo + self.n].copy()


def _state(step_before, betas=BETAS):
    return torch.tensor([A.LR, betas[0], betas[1], A.EPS, float(step_before)], dtype=torch.float64, device='cuda')


def _check_tick(state, derived, step, betas=BETAS):
    """state[4] is exact; each of the six floats is within one fp32 ulp of derived64."""
    st, dv = state.cpu().numpy(), derived.cpu().numpy()
    assert st[4] == float(step) and st[:4].tolist() == [A.LR, betas[0], betas[1], A.EPS]
    for got, want in zip(dv[:6], A.derived64(A.LR, betas[0], betas[1], A.EPS, step)):
        assert abs(float(got) - want) <= float(np.spacing(np.float32(want))), (step, got, want)
    assert not dv[6:].any()


def _tick(step, gd, betas=BETAS, skip=0.0):
    """The tick of step number `step` (guarded when gd is not None) -> (state, derived, guard)."""
    L = _L()
    state, derived = _state(step - 1, betas), torch.zeros(8, dtype=torch.float32, device='cuda')
    guard = None
    if gd is None:
        L.call('hoig_adam_tick', state.data_ptr(), derived.data_ptr(), _st())
    else:
        guard = torch.tensor([gd, skip], dtype=torch.float32, device='cuda')
        L.call('hoig_adam_tick_guarded', state.data_ptr(), derived.data_ptr(), guard.data_ptr(), _st())
    return state, derived, guard


def run_slice(entry, case, gs, gd, offs=(0, 0, 0, 0), betas=BETAS):
    """One step of `case` through a slice entry point: 'step' (hoig_adam_step), 'dev' (tick + hoig_adam_step_dev; the guarded pair when
    gd is not None) -> p, m, v."""
    L = _L()
    n, step = len(case['p']), case['step']
    p, g, m, v = (Buf(case[k], o) for k, o in zip('pgmv', offs))
    if entry == 'step':
        L.call('hoig_adam_step', p.ptr, g.ptr, m.ptr, v.ptr, n, A.LR, betas[0], betas[1], A.EPS, step, gs, _st())
    else:
        state, derived, guard = _tick(step, gd, betas)
        if gd is None:
            L.call('hoig_adam_step_dev', p.ptr, g.ptr, m.ptr, v.ptr, n, derived.data_ptr(), gs, _st())
        else:
            L.call('hoig_adam_step_dev_guarded', p.ptr, g.ptr, m.ptr, v.ptr, n, derived.data_ptr(), gs, guard.data_ptr(), _st())
        _check_tick(state, derived, step, betas)
    torch.cuda.synchronize()
    assert np.array_equal(g.get(), case['g'])
    return p.get(), m.get(), v.get()


# ---- the fused entry points want a table: one packed weight (64, 1, 32) with both kinds of planes at offset 0, the rest plain
W_ELEMS, W_ROW = 2048, [0, 64, 1, 32, 3, 0]


def pack_tables(n_plain):
    """(segs, ntiles, plain chunks, nplain, buffer length) for a buffer of one packed weight and n_plain plain elements: the plain part is
    padded to a multiple of 4 (chunks are counted in float4s), in chunks of at most 1024."""
    n4 = (n_plain + 3) // 4 * 4
    chunks, at = [], W_ELEMS
    while at < W_ELEMS + n4:
        c = min(1024, W_ELEMS + n4 - at)
        chunks.append([at, c])
        at += c
    return (torch.tensor([W_ROW], dtype=torch.int64, device='cuda'), 2,
            torch.tensor(chunks if chunks else [[0, 0]], dtype=torch.int64, device='cuda'), len(chunks), W_ELEMS + n4)


def run_pack(case, gs, gd, betas=BETAS, skip=0.0, planes=None, tick=None):
    """One step of a row of W_ELEMS + n elements through hoig_adam_pack_step (gd None) or its guarded form -> p, m, v, the four planes
    (tensors of the padded length, prefilled with 0x5A5A unless given)."""
    L = _L()
    n = len(case['p'])
    segs, ntiles, plain, nplain, total = pack_tables(n - W_ELEMS)
    pad = np.zeros(total - n, dtype=np.float32)
    p, g, m, v = (Buf(np.concatenate([case[k], pad])) for k in 'pgmv')
    if planes is None:
        planes = [torch.full((total,), 0x5A5A, dtype=torch.int16, device='cuda') for _ in range(4)]
    state, derived, guard = tick if tick is not None else _tick(case['step'], gd, betas, skip)
    args = [p.ptr, g.ptr, m.ptr, v.ptr, derived.data_ptr(), gs, segs.data_ptr(), 1, ntiles, plain.data_ptr(), nplain] + \
           [b.data_ptr() for b in planes]
    if gd is None:
        L.call('hoig_adam_pack_step', *(args + [_st()]))
    else:
        L.call('hoig_adam_pack_step_guarded', *(args + [guard.data_ptr(), _st()]))
    torch.cuda.synchronize()
    if not skip:
        _check_tick(state, derived, case['step'], betas)
    out = []
    for b in (p, m, v):
        x = b.get()
        assert not x[n:].any(), 'the padding of the plain part moved'
        out.append(x[:n])
    return out[0], out[1], out[2], planes


RATIOS = {}


def _note(family, r):
    for k, x in r.items():
        RATIOS[(family, k)] = max(RATIOS.get((family, k), 0.0), x)


def _family(n):
    return 'n<=8' if n <= 8 else ('n~1024' if n < BIG else 'n=2.1M')


CASES = [(n, kind, gs, gd) for n in SIZES for kind in ('zero', 'randn') for gs, gd in ((1.0, None), (0.5, None), (1.0, 1.0), (0.5, 0.37))]
CASES += [(BIG, 'zero', 0.5, None), (BIG, 'zero', 0.5, 0.37), (BIG, 'randn', 1.0, None), (BIG, 'randn', 1.0, 1.0)]


@pytest.mark.parametrize('n,kind,gs,gd', CASES)
def test_slice_entry_points_against_float64(n, kind, gs, gd):
    """hoig_adam_step and tick + hoig_adam_step_dev (gd None), or the guarded tick + hoig_adam_step_dev_guarded with guard = {gd, 0}: the
    step counts 1, 2, 3, 10, 1000 and 100000, each from the twin's moments of the one before."""
    worst = {}
    for case in A.row_steps(n, kind, gs, gd):
        for entry in (('step', 'dev') if gd is None else ('dev',)):
            p, m, v = run_slice(entry, case, gs, gd)
            r = A.check_step(case, p, m, v, '%s n=%d' % (entry + ('_guarded' if gd is not None else ''), n))
            _note(_family(n), r)
            for k, x in r.items():
                worst[k] = max(worst.get(k, 0.0), x)
    print('adam slices n=%d %s gs=%g guard=%s: kernel / twin worst relative error %s' % (n, kind, gs, gd, {k: round(x, 3) for k, x in worst.items()}))


PACK_CASES = [(n, kind, gs, gd) for n in (1, 5, 8, 1023, 1024, 1025) for kind, gs, gd in (('zero', 0.5, None), ('zero', 0.5, 0.37), ('randn', 1.0, 1.0))]
PACK_CASES += [(n, 'zero', 1.0, None) for n in (2, 3, 4, 7)] + [(BIG, 'zero', 0.5, 0.37), (BIG, 'randn', 1.0, None)]


@pytest.mark.parametrize('n,kind,gs,gd', PACK_CASES)
def test_fused_entry_points_against_float64(n, kind, gs, gd):
    """hoig_adam_pack_step (gd None) and hoig_adam_pack_step_guarded over a buffer of one packed weight and n plain elements: the same
    bounds (what the planes must hold is tests/test_pack_planes_gpu.py's business)."""
    worst = {}
    for case in A.row_steps(W_ELEMS + n, kind, gs, gd):
        p, m, v, _ = run_pack(case, gs, gd)
        r = A.check_step(case, p, m, v, 'pack%s n=%d' % ('_guarded' if gd is not None else '', n))
        _note('fused ' + _family(n), r)
        for k, x in r.items():
            worst[k] = max(worst.get(k, 0.0), x)
    print('adam fused n=%d+%d %s gs=%g guard=%s: kernel / twin %s' % (W_ELEMS, n, kind, gs, gd, {k: round(x, 3) for k, x in worst.items()}))


@pytest.mark.parametrize('n', [5, 1025])
@pytest.mark.parametrize('gd', [None, 0.37])
def test_a_first_moment_decay_other_than_one_half(n, gd):
    """betas = (0.9, 0.999): 1 - beta1 is not beta1, and the first moment's product rounds."""
    betas = (0.9, 0.999)
    for case in A.row_steps(n, 'zero', 0.5, gd, betas):
        for entry in (('step', 'dev') if gd is None else ('dev',)):
            p, m, v = run_slice(entry, case, 0.5, gd, betas=betas)
            _note('beta1=0.9', A.check_step(case, p, m, v, '%s n=%d beta1=0.9' % (entry, n)))
    for case in A.row_steps(W_ELEMS + n, 'zero', 0.5, gd, betas):
        p, m, v, _ = run_pack(case, 0.5, gd, betas=betas)
        _note('beta1=0.9', A.check_step(case, p, m, v, 'pack n=%d beta1=0.9' % n))


@pytest.mark.parametrize('entry', ['dev', 'pack'])
def test_a_skipped_step_touches_nothing_and_the_next_one_does_not_count_it(entry):
    """guard = {anything, 1}: p, m, v, the planes, `state` and `derived` keep their bits; the taken step after it is number step0 + 1."""
    L = _L()
    n = 1025 + (W_ELEMS if entry == 'pack' else 0)
    case = [c for c in A.row_steps(n, 'randn', 0.5, 0.37)][3]              # step 10: nonzero moments
    step = case['step']
    state = _state(step - 1)
    derived = torch.tensor([3.0, 1.0, 4.0, 1.0, 5.0, 9.0, 0.0, 0.0], dtype=torch.float32, device='cuda')
    guard = torch.tensor([123.0, 1.0], dtype=torch.float32, device='cuda')
    before = (state.clone(), derived.clone())
    L.call('hoig_adam_tick_guarded', state.data_ptr(), derived.data_ptr(), guard.data_ptr(), _st())
    if entry == 'dev':
        p, g, m, v = (Buf(case[k]) for k in 'pgmv')
        L.call('hoig_adam_step_dev_guarded', p.ptr, g.ptr, m.ptr, v.ptr, n, derived.data_ptr(), 0.5, guard.data_ptr(), _st())
        torch.cuda.synchronize()
        got = (p.get(), m.get(), v.get())
    else:
        p_, m_, v_, planes = run_pack(case, 0.5, 123.0, skip=1.0, tick=(state, derived, guard))
        got = (p_, m_, v_)
        assert all(bool((b == 0x5A5A).all()) for b in planes)
    for x, k in zip(got, 'pmv'):
        assert x.tobytes() == case[k].tobytes(), k
    assert torch.equal(state, before[0]) and torch.equal(derived, before[1])
    # the next step is taken, from the un-advanced count
    guard.copy_(torch.tensor([0.37, 0.0]))
    L.call('hoig_adam_tick_guarded', state.data_ptr(), derived.data_ptr(), guard.data_ptr(), _st())
    _check_tick(state, derived, step)
    if entry == 'dev':
        L.call('hoig_adam_step_dev_guarded', p.ptr, g.ptr, m.ptr, v.ptr, n, derived.data_ptr(), 0.5, guard.data_ptr(), _st())
        torch.cuda.synchronize()
        got = (p.get(), m.get(), v.get())
    else:
        got = run_pack(case, 0.5, 0.37, tick=(state, derived, guard))[:3]
    A.check_step(case, got[0], got[1], got[2], '%s after a skipped step' % entry)


# ------------------------------------------------------------------------------------------------ slices off a 16-byte boundary
OFFS = [(1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (0, 0, 1, 0), (0, 2, 0, 0), (3, 0, 0, 0), (0, 0, 0, 1)]


@pytest.mark.parametrize('offs', OFFS, ids=['%d%d%d%d' % o for o in OFFS])
@pytest.mark.parametrize('n', [1, 5, 1025])
def test_slices_off_a_16_byte_boundary(n, offs):
    """Views that start 1, 2 and 3 elements past a 16-byte boundary (all four, or just one of p, g, m, v): the scalar loop takes all n,
    and the results meet the same bounds; nothing is written outside the slice (Buf.get)."""
    for gs, gd in ((0.5, None), (0.5, 0.37)):
        for case in A.row_steps(n, 'zero', gs, gd):
            for entry in (('step', 'dev') if gd is None else ('dev',)):
                p, m, v = run_slice(entry, case, gs, gd, offs)
                _note('misaligned', A.check_step(case, p, m, v, '%s n=%d offs=%s' % (entry, n, offs)))
                if case['step'] == 10:          # (what docs/optimizer_parity.md reports: the scalar loop's bits are the float4 loop's)
                    pa, ma, va = run_slice(entry, case, gs, gd)
                    same = pa.tobytes() == p.tobytes() and ma.tobytes() == m.tobytes() and va.tobytes() == v.tobytes()
                    RATIOS[('misaligned', 'bits equal the aligned launch')] = min(RATIOS.get(('misaligned', 'bits equal the aligned launch'), 1.0), float(same))


# ------------------------------------------------------------------------------------------------ FusedAdam over a tree
TREE_SHAPES = A.TREE_SHAPES
TREE_STEPS = 5


def _tree_data():
    """Weights randn * 0.05; gradients sign * 10^u, u uniform in [-6, 1], the sign of an element the same at every step (row_steps)."""
    rng = np.random.RandomState(11)
    ref = {k: (rng.standard_normal(s) * 0.05).astype(np.float32) for k, s in TREE_SHAPES}
    sign = {k: rng.choice([-1.0, 1.0], s) for k, s in TREE_SHAPES}
    grads = [{k: (sign[k] * 10.0 ** rng.uniform(-6.0, 1.0, s)).astype(np.float32) for k, s in TREE_SHAPES} for _ in range(TREE_STEPS)]
    return ref, grads


_tree_truth = {}


def _truth():
    """Per parameter: adam64 and the twin over the five steps, each carrying its own state (computed once)."""
    if not _tree_truth:
        ref, grads = _tree_data()
        for k, _ in TREE_SHAPES:
            args = (ref[k].ravel(), [g[k].ravel() for g in grads], np.zeros(ref[k].size), np.zeros(ref[k].size), 0, A.LR, BETAS, A.EPS, 0.5)
            _tree_truth[k] = (A.adam64(*args), A.adam32_twin(*args))
    return _tree_truth


def _make_tree(ref):
    from hoig_amd.nn import ParamTree, FusedAdam
    tree = ParamTree(TREE_SHAPES, torch.device('cuda'), transposed_names=('up.weight',))
    tree.load_state_dict({k: torch.from_numpy(v) for k, v in ref.items()})
    tree._ensure_plane_bufs()
    for b in tree._plane_bufs:
        b.zero_()
    tree._refresh_planes()
    assert tree.fused_step_tables() is not None
    assert sorted(tree._plane_flags.values()) == [1, 2, 3, 3, 3] and 's.mlp_gb.weight' in tree.F
    return tree, FusedAdam(tree, lr=A.LR, betas=BETAS)


def _cuts(n, aligned):
    a, b = n // 5, n // 2 + 1
    if aligned:
        return [(0, a // 4 * 4), (a // 4 * 4, b // 4 * 4), (b // 4 * 4, n)]
    a, b = a // 4 * 4 + 1, b // 4 * 4 + 2           # (1 and 2 past a multiple of 4: the second slice is off by 1, the third by 2)
    return [(0, a), (a, b), (b, n)]


def _run_tree(route):
    ref, grads = _tree_data()
    tree, opt = _make_tree(ref)
    n = tree.flat.numel()
    for gs in grads:
        with torch.no_grad():
            for k, p_ in tree.P.items():
                p_.grad.copy_(torch.from_numpy(gs[k]).cuda())
        opt.fuse_planes = route == 'fused'
        ready = iter(_cuts(n, route == 'aligned')) if route in ('aligned', 'misaligned') else None
        opt.step(grad_scale=0.5, ready=ready)
    torch.cuda.synchronize()
    return tree, opt


def _check_tree(tree, opt, what):
    sd, osd = tree.state_dict(), opt.state_dict()
    names = [k for k, _ in TREE_SHAPES]
    assert tree.ref_names() == names and sorted(osd['state']) == list(range(len(names)))
    for i, k in enumerate(names):
        (pr, mr, vr, ur, sr), (pt, mt, vt, ut, _) = _truth()[k]
        st = osd['state'][i]
        assert float(st['step']) == float(sr) == TREE_STEPS
        p, m, v = (t.cpu().numpy().ravel() for t in (sd[k], st['exp_avg'], st['exp_avg_sq']))
        for name, got, t_, r_ in (('m', m, mt, mr), ('v', v, vt, vr)):
            e, lim = A.worst_rel(got, r_), 4.0 * A.worst_rel(t_, r_)
            _note('tree', {name: e / (lim / 4.0) if lim > 0 else 0.0})
            assert e <= lim, '%s %s: %s off by %.3e relative, the limit (4 x twin) is %.3e' % (what, k, name, e, lim)
        # five roundings of p (an update stays under 2 lr, so |p| < |p_ref| + 2e-3 throughout) and the twin's update errors, step by step
        lim = TREE_STEPS * 2.0 ** -24 * (np.abs(pr) + 2e-3) + 4.0 * sum(float(np.max(np.abs(a.astype(np.float64) - b))) for a, b in zip(ut, ur))
        assert (np.abs(p - pr) <= lim).all(), (what, k, float(np.max(np.abs(p - pr))))
    # the alignment gaps never move
    covered = torch.zeros(tree.flat.numel(), dtype=torch.bool)
    for k, off in tree._offsets.items():
        covered[off:off + int(np.prod(tree._internal[k][0]))] = True
    assert int((~covered).sum()) == 1 + 3 + 2 + 1
    for buf in (tree.flat, opt.exp_avg, opt.exp_avg_sq):
        assert not bool(buf.cpu()[~covered].any()), '%s: an alignment gap moved' % what


@pytest.mark.parametrize('route', ['fused', 'two', 'aligned', 'misaligned'])
def test_fused_adam_over_a_tree_against_float64(route):
    """Five steps on one route: the update and the planes in one launch, two launches, slices cut at multiples of 4, slices cut 1 and 2
    elements past a multiple of 4 (FusedAdam.step(ready=...) at any element: include/hoig_kernels.h)."""
    tree, opt = _run_tree(route)
    _check_tree(tree, opt, route)
    if route == 'misaligned':                   # against one launch over the whole buffer: the bits, for docs/optimizer_parity.md
        t2, o2 = _run_tree('two')
        same = torch.equal(tree.flat, t2.flat) and torch.equal(opt.exp_avg, o2.exp_avg) and torch.equal(opt.exp_avg_sq, o2.exp_avg_sq)
        RATIOS[('tree', 'misaligned slices: bits equal one launch')] = float(same)
        print('misaligned slices against one launch: bits %s' % ('equal' if same else 'differ'))


def test_fused_adam_state_dict_round_trip():
    from hoig_amd.nn import FusedAdam
    tree, opt = _run_tree('fused')
    sd, osd = tree.state_dict(), opt.state_dict()
    t2, _ = _make_tree({k: np.zeros(s, dtype=np.float32) for k, s in TREE_SHAPES})
    o2 = FusedAdam(t2, lr=1.0, betas=(0.1, 0.2))
    t2.load_state_dict(sd)
    o2.load_state_dict(osd)
    assert torch.equal(t2.flat, tree.flat) and torch.equal(o2.exp_avg, opt.exp_avg) and torch.equal(o2.exp_avg_sq, opt.exp_avg_sq)
    assert o2.step_count == TREE_STEPS and o2.param_groups[0]['lr'] == A.LR and tuple(o2.param_groups[0]['betas']) == BETAS
    sd2, osd2 = t2.state_dict(), o2.state_dict()
    for k in sd:
        assert torch.equal(sd[k], sd2[k])
    for i in osd['state']:
        for key in ('exp_avg', 'exp_avg_sq', 'step'):
            assert torch.equal(osd['state'][i][key], osd2['state'][i][key])


def test_zz_report_the_ratios():
    """Prints the worst kernel / twin ratio per row family (docs/optimizer_parity.md holds a run's figures); every one was asserted <= 4
    where it was measured."""
    for k in sorted(RATIOS):
        print('ratio %-40s %-45s %.3f' % (k[0], k[1], RATIOS[k]))
    assert all(x <= 4.0 for (fam, k), x in RATIOS.items() if k in ('m', 'v', 'update'))
