"""The operand-plane packers against tests/pack_reference.py, bit for bit (docs/optimizer_parity.md): the per-weight packer in both modes,
the one-launch packer over a table, and the planes the fused Adam step leaves -- each over buffers prefilled with 0x5A5A, which must
survive everywhere outside a flagged weight's own span."""
import ctypes

import numpy as np
import pytest
import torch

import pack_reference as P

pytestmark = pytest.mark.gpu
MARGIN = 64


def _L():
    from hoig_amd import _lib
    return _lib


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_weights = {}


def _weight(i):
    """(w, planted places, {for_dgrad: (hi, lo)}) of shape i, made once."""
    if i not in _weights:
        w, at = P.weight(P.SHAPES[i], 100 + i)
        _weights[i] = (w, at, {d: P.planes(w, d) for d in (False, True)})
    return _weights[i]


def _bits(t):
    return t.cpu().numpy().view(np.uint16)


def _explain(got, want, name):
    """What differs, for the failure message: how many elements, and whether they are all fp16 subnormals or zeros of the reference."""
    bad = np.flatnonzero(got != want)
    if len(bad) == 0:
        return ''
    sub = (want[bad] & 0x7C00) == 0
    return '%s: %d of %d elements differ (%d of them where the reference is an fp16 subnormal or zero); first: got %#06x want %#06x at %d' % (
        name, len(bad), len(want), int(sub.sum()), got[bad[0]], want[bad[0]], bad[0])


@pytest.mark.parametrize('with_lo', [True, False], ids=['lo', 'lo_null'])
@pytest.mark.parametrize('for_dgrad', [False, True], ids=['forward', 'dgrad'])
@pytest.mark.parametrize('i', range(len(P.SHAPES)), ids=['%dx%dx%d' % s for s in P.SHAPES])
def test_per_weight_packer(i, for_dgrad, with_lo):
    """hoig_pack_conv_weight_bf16: (128, 25, 192) has more elements than one pass of its capped grid covers."""
    L = _L()
    Co, RS, Ci = P.SHAPES[i]
    w, _, ref = _weight(i)
    n = w.size
    wd = torch.from_numpy(w).cuda()
    hi = torch.full((n + 2 * MARGIN,), P.SENTINEL, dtype=torch.int16, device='cuda')
    lo = torch.full((n + 2 * MARGIN,), P.SENTINEL, dtype=torch.int16, device='cuda')
    L.call('hoig_pack_conv_weight_bf16', wd.data_ptr(), Co, RS, Ci, 1 if for_dgrad else 0, hi.data_ptr() + 2 * MARGIN,
           lo.data_ptr() + 2 * MARGIN if with_lo else None, _st())
    torch.cuda.synchronize()
    h, l = _bits(hi), _bits(lo)
    for x in (h, l):
        assert (x[:MARGIN] == P.SENTINEL).all() and (x[MARGIN + n:] == P.SENTINEL).all()
    assert np.array_equal(h[MARGIN:MARGIN + n], ref[for_dgrad][0]), _explain(h[MARGIN:MARGIN + n], ref[for_dgrad][0], 'hi')
    if with_lo:
        assert np.array_equal(l[MARGIN:MARGIN + n], ref[for_dgrad][1]), _explain(l[MARGIN:MARGIN + n], ref[for_dgrad][1], 'lo')
    else:
        assert (l == P.SENTINEL).all()
    assert np.array_equal(wd.cpu().numpy(), w)


# ---- a flat buffer of all seven weights with plain parameters in between
FLAGS = [3, 1, 2, 3, 1, 2, 3]
GAPS = [4, 1028, 8, 1024, 12, 2052, 4]          # plain elements behind each weight (multiples of 4: a parameter starts 16-byte aligned)


def _layout():
    """-> (rows of the table, [(offset, count)] of the plain runs, total elements, tile count)"""
    rows, plain, at, tile = [], [], 0, 0
    for (Co, RS, Ci), fl, gap in zip(P.SHAPES, FLAGS, GAPS):
        rows.append([at, Co, RS, Ci, fl, tile])
        tile += (Co // 32) * (Ci // 32)
        at += Co * RS * Ci
        plain.append((at, gap))
        at += gap
    return rows, plain, at, tile


def _flat():
    rows, plain, total, _ = _layout()
    flat = np.zeros(total, dtype=np.float32)
    for i, r in enumerate(rows):
        w = _weight(i)[0]
        flat[r[0]:r[0] + w.size] = w.ravel()
    rng = np.random.RandomState(7)
    for a, c in plain:
        flat[a:a + c] = rng.standard_normal(c).astype(np.float32)
    return flat


def _expected(flat):
    """The four plane buffers (forward hi, lo; data-gradient hi, lo) a launch over the table must leave of `flat`, from 0x5A5A."""
    rows, _, total, _ = _layout()
    out = [np.full(total, P.SENTINEL, dtype=np.uint16) for _ in range(4)]
    for off, Co, RS, Ci, fl, _ in rows:
        w = flat[off:off + Co * RS * Ci].reshape(Co, RS, Ci)
        if fl & 1:
            out[0][off:off + w.size], out[1][off:off + w.size] = P.planes(w, False)
        if fl & 2:
            out[2][off:off + w.size], out[3][off:off + w.size] = P.planes(w, True)
    return out


def _compare(bufs, want):
    for name, b, x in zip(('forward hi', 'forward lo', 'dgrad hi', 'dgrad lo'), bufs, want):
        got = _bits(b)
        assert (got[:MARGIN] == P.SENTINEL).all() and (got[MARGIN + len(x):] == P.SENTINEL).all(), name
        assert np.array_equal(got[MARGIN:MARGIN + len(x)], x), _explain(got[MARGIN:MARGIN + len(x)], x, name)


def _plane_bufs(total):
    bufs = [torch.full((total + 2 * MARGIN,), P.SENTINEL, dtype=torch.int16, device='cuda') for _ in range(4)]
    return bufs, [b.data_ptr() + 2 * MARGIN for b in bufs]


def test_one_launch_packer_over_a_table():
    """hoig_pack_conv_weights_bf16_all with flags 1, 2 and 3: a flagged weight's span holds the reference's planes; the spans of the kinds
    a weight is not flagged for, the plain parameters between the weights and the margins still hold 0x5A5A."""
    L = _L()
    rows, _, total, ntiles = _layout()
    flat = _flat()
    fd = torch.from_numpy(flat).cuda()
    table = torch.tensor(rows, dtype=torch.int64, device='cuda')
    bufs, ptrs = _plane_bufs(total)
    L.call('hoig_pack_conv_weights_bf16_all', fd.data_ptr(), table.data_ptr(), len(rows), ntiles, ptrs[0], ptrs[1], ptrs[2], ptrs[3], _st())
    torch.cuda.synchronize()
    _compare(bufs, _expected(flat))
    assert np.array_equal(fd.cpu().numpy(), flat)


@pytest.mark.parametrize('guarded', [False, True], ids=['plain', 'guarded'])
def test_planes_left_by_the_fused_adam_step(guarded):
    """hoig_adam_pack_step / _guarded: the planes are those of the fp32 weights the SAME launch wrote, read back from `flat`.  The planted
    values get a zero gradient (and zero moments), so they stay what they are and reach the split."""
    import adam_reference as A
    L = _L()
    rows, plain, total, ntiles = _layout()
    flat = _flat()
    g = A.gradients(total, 77)
    g[np.abs(g) < 1e-3] *= np.float32(1e6)              # (most elements move by about lr: a launch that packed the OLD weights shows)
    for i, r in enumerate(rows):
        g[r[0] + _weight(i)[1]] = 0.0
    chunks = []
    for a, c in plain:
        while c > 0:
            chunks.append([a, min(c, 1024)])
            a, c = a + min(c, 1024), c - min(c, 1024)
    fd, gd, md, vd = (torch.from_numpy(x).cuda() for x in (flat, g, np.zeros_like(flat), np.zeros_like(flat)))
    table = torch.tensor(rows, dtype=torch.int64, device='cuda')
    pl = torch.tensor(chunks, dtype=torch.int64, device='cuda')
    state = torch.tensor([A.LR, 0.5, 0.999, A.EPS, 0.0], dtype=torch.float64, device='cuda')
    derived = torch.zeros(8, dtype=torch.float32, device='cuda')
    guard = torch.tensor([0.37, 0.0], dtype=torch.float32, device='cuda')
    bufs, ptrs = _plane_bufs(total)
    args = [fd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), derived.data_ptr(), 0.5, table.data_ptr(), len(rows), ntiles,
            pl.data_ptr(), len(chunks)] + ptrs
    if guarded:
        L.call('hoig_adam_tick_guarded', state.data_ptr(), derived.data_ptr(), guard.data_ptr(), _st())
        L.call('hoig_adam_pack_step_guarded', *(args + [guard.data_ptr(), _st()]))
    else:
        L.call('hoig_adam_tick', state.data_ptr(), derived.data_ptr(), _st())
        L.call('hoig_adam_pack_step', *(args + [_st()]))
    torch.cuda.synchronize()
    new = fd.cpu().numpy()
    moved = new != flat
    assert moved[g != 0].mean() > 0.9 and not moved[g == 0].any()
    for i, r in enumerate(rows):
        at = r[0] + _weight(i)[1]
        assert new[at].tobytes() == flat[at].tobytes()
    _compare(bufs, _expected(new))
