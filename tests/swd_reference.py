"""Truths, limits and the checks themselves for the sliced Wasserstein distance (hoig_amd/metrics/swd.py, hoig_amd/csrc/swd.*):
tests/test_swd_cpu.py runs every check through the CPU twins (device 'cpu'), tests/test_swd_gpu.py through the kernels (device
'cuda') -- the same truths and the same limits.

The truth is float64 numpy: scipy.ndimage.convolve(mode='mirror') with the 5 x 5 outer product for the pyramid, np.sort for the
sort, a pure-Python Philox4x32-10 for the positions, np.random.default_rng for the directions.  Nothing of the product is used.

Where the limits come from (docs/swd.md has the derivations; U32 = 2^-24, U64 = 2^-53):
  * Every pyramid value is below 256 in magnitude, so one fp32 rounding moves it by at most E = 2^-17.  The Gaussian levels 1 and 2
    of a byte image are EXACT: every weight is a multiple of 1/16, so level l holds multiples of 2^-8l below 256 -- 16 and 24
    significant bits -- and so are all partial sums.  Exactness ends at the horizontal pass of level 3 (multiples of 2^-28).  From
    there a pass is 5 products and 4 sums, each within E, and the weights of a pass sum to 1: g_err(l) = 18 E max(0, l - 2).
  * lap[l] = g[l] - up(g[l+1]).  The step up of level 1 (multiples of 2^-8, weights multiples of 1/8: 2^-14) is exact, so lap[0] is
    exact.  Above it a pass is at most 3 products and 3 sums: lap_err(l) = g_err(l) + g_err(l+1) + 12 E + E (the difference).  The
    last level is g itself.  The float64 reference's own error (at most 60 roundings of 2^-53 * 256) is REF = 2^-38.
  * fp64 sums of E terms in any order: |d sum| <= E U64 sum |x|.  mean: (E + 1) U64 max |x|; the deviation: that of the mean plus
    (E / 2 + 3) U64 sd (first order; the derivation is in the docs).
  * the projection: the operand fl32((x - mean) / sd) is within U32 |z| (+ 4 U64 |z| of its fp64 arithmetic), a chain of 147 fmaf
    within 147 U32 sum |z_k w_k|: |d p| <= 149 U32 sum |z_k w_k|.
  * end to end: a pyramid error eps moves the mean by <= eps and the deviation by <= eps, so z by <= eps (2 + |z|) / (sd - eps); a
    projection by <= sum_k |dz_k| |w_k| + 149 U32 sum |z_k w_k|; sorting is 1-Lipschitz in the sup norm, so the mean |a - b| of the
    sorted projections moves by at most the sum of the two sets' largest projection errors.
"""
import ctypes

import numpy as np
import torch

U32, U64 = 2.0 ** -24, 2.0 ** -53
E32 = 2.0 ** -17
REF = 2.0 ** -38
K = 147
LD = np.longdouble


def to(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def back(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ Philox and the positions
def philox4x32_10(ctr, key):
    """Salmon et al. 2011 in Python integers."""
    c, k = [int(v) & 0xFFFFFFFF for v in ctr], [int(v) & 0xFFFFFFFF for v in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def levels_of(H, W, levels=None):
    n = int(np.floor(np.log2(min(H, W) / 16.0))) + 1
    return n if levels is None else min(n, levels)


def ref_positions(n, H, W, nl, patches, seed, set_id, first=0):
    pos = np.zeros((n, nl, patches, 2), np.int32)
    for i in range(n):
        for lv in range(nl):
            for p in range(patches):
                w = philox4x32_10((set_id, lv, first + i, p), (seed & 0xFFFFFFFF, seed >> 32))
                pos[i, lv, p] = ((w[0] * ((H >> lv) - 6)) >> 32, (w[1] * ((W >> lv) - 6)) >> 32)
    return pos


# ------------------------------------------------------------------------------------------------ the pyramid
F5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
F55 = np.outer(F5, F5)


def ref_pyramid(img, nl):
    """img uint8 [H,W,3] -> the Laplacian levels, float64 [Hl,Wl,3], finest first."""
    from scipy.ndimage import convolve
    g = [img.astype(np.float64)]
    for _ in range(1, nl):
        f = np.stack([convolve(g[-1][:, :, c], F55, mode='mirror') for c in range(3)], -1)
        g.append(f[::2, ::2])
    lap = []
    for lv in range(nl - 1):
        z = np.zeros_like(g[lv])
        z[::2, ::2] = g[lv + 1]
        lap.append(g[lv] - np.stack([convolve(z[:, :, c], 4.0 * F55, mode='mirror') for c in range(3)], -1))
    lap.append(g[-1])
    return lap


def ref_descriptors(u8, nl, pos):
    """-> a list of nl float64 [n * patches, 147]"""
    n, patches = u8.shape[0], pos.shape[2]
    out = [np.zeros((n * patches, K)) for _ in range(nl)]
    for i in range(n):
        lap = ref_pyramid(u8[i], nl)
        for lv in range(nl):
            for p in range(patches):
                y0, x0 = pos[i, lv, p]
                out[lv][i * patches + p] = lap[lv][y0:y0 + 7, x0:x0 + 7].transpose(2, 0, 1).reshape(K)
    return out


def g_err(lv):
    return 18.0 * E32 * max(0, lv - 2)


def lap_err(lv, nl):
    if lv == nl - 1:
        return g_err(lv)
    return 0.0 if lv == 0 else g_err(lv) + g_err(lv + 1) + 13.0 * E32


def images(n, H, W, seed):
    """Smooth gradients plus noise: every level has something to see."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([np.sin(xx / 5.0 + g.uniform(0, 6, (n, 1, 1))), np.cos(yy / 7.0 + g.uniform(0, 6, (n, 1, 1))),
                     np.sin((xx + yy) / 9.0 + g.uniform(0, 6, (n, 1, 1)))], -1) * 0.5 + 0.5
    return np.clip(base * 200.0 + g.uniform(0, 56, base.shape), 0, 255).astype(np.uint8)


# (H, W, levels argument, n): two levels three ways, a capped chain, and the five-level chain of one 256 x 256 image
PYRAMID_CASES = [(32, 32, None, 3), (64, 32, None, 3), (48, 80, None, 3), (64, 64, 3, 3), (256, 256, None, 1)]
PATCHES = 5


def corner_positions(n, H, W, nl):
    pos = np.zeros((n, nl, 4, 2), np.int32)
    for lv in range(nl):
        h, w = (H >> lv) - 7, (W >> lv) - 7
        pos[:, lv] = [(0, 0), (0, w), (h, 0), (h, w)]
    return pos


def check_descriptors(dev, case, seed=5, set_id=1):
    """-> the rows (numpy, per level) for the twin / device comparison"""
    from hoig_amd.metrics import swd as S
    H, W, levels, n = case
    nl = levels_of(H, W, levels)
    assert S.pyramid_levels(H, W, levels) == nl == (5 if H == 256 else (3 if levels else 2))
    u8 = images(n, H, W, 100 + H + W)
    want_pos = ref_positions(n, H, W, nl, PATCHES, seed, set_id)
    got_pos = back(S.patch_positions(n, H, W, levels, PATCHES, seed, set_id, 0, dev))
    assert got_pos.dtype == np.int32 and np.array_equal(got_pos, want_pos)
    # the drawn patches, then one at every corner of every level: the mirror boundary is read on all four sides
    pos = np.concatenate([want_pos, corner_positions(n, H, W, nl)], 2)
    got = [back(t) for t in S.laplacian_descriptors_u8(to(dev, u8), levels, positions=pos)]
    want = ref_descriptors(u8, nl, pos)
    assert len(got) == nl
    for lv in range(nl):
        err = np.abs(got[lv].astype(np.float64) - want[lv]).max()
        print('pyramid %dx%d level %d: error %.3g, limit %.3g' % (H, W, lv, err, lap_err(lv, nl) + REF))
        assert got[lv].shape == (n * (PATCHES + 4), K) and err <= lap_err(lv, nl) + REF
    drawn = [back(t) for t in S.laplacian_descriptors_u8(to(dev, u8), levels, PATCHES, seed, set_id)]
    for lv in range(nl):
        assert np.array_equal(drawn[lv].reshape(n, PATCHES, K), got[lv].reshape(n, PATCHES + 4, K)[:, :PATCHES])
    return got


def check_split(dev):
    """The same images in calls of 1 + 2 and of 3: the same rows, because the image index is the running count."""
    from hoig_amd.metrics import swd as S
    u8 = to(dev, images(3, 32, 32, 77))
    whole = S.SWDBank(1, PATCHES, None, 9, dev).append(u8)
    parts = S.SWDBank(1, PATCHES, None, 9, dev).append(u8[:1]).append(u8[1:])
    assert whole.n == parts.n == 3 and whole.num_levels() == 2
    for lv in range(2):
        assert np.array_equal(back(whole.rows(lv)), back(parts.rows(lv)))
    assert np.array_equal(back(S.patch_positions(2, 32, 32, None, PATCHES, 9, 1, 1, dev)), ref_positions(3, 32, 32, 2, PATCHES, 9, 1)[1:])
    other = S.SWDBank(0, PATCHES, None, 9, dev).append(u8)
    assert not np.array_equal(back(other.rows(0)), back(whole.rows(0)))        # the set id is in the counter
    copy = whole.copy().append(u8[:1])
    assert copy.n == 4 and whole.n == 3 and back(whole.rows(0)).shape[0] == 3 * PATCHES


# ------------------------------------------------------------------------------------------------ statistics
STAT_ROWS = (1, 15, 43, 700)        # 49 R elements per channel: one chunk, and several with a ragged last one


def check_stats(dev, rows):
    from hoig_amd.metrics import swd as S
    g = np.random.default_rng(rows)
    x = (g.standard_normal((rows, K)) * g.uniform(1, 60, (1, K)) + np.repeat([100.0, -3.0, 0.5], 49)).astype(np.float32)
    stats, status = S.channel_stats(to(dev, x))
    stats = back(stats)
    assert back(status).tolist() == [0] and stats.shape == (3, 2) and stats.dtype == np.float64
    for c in range(3):
        v = x[:, 49 * c:49 * c + 49].astype(LD).ravel()
        n = v.size
        mean, sd = v.mean(), np.sqrt(((v - v.mean()) ** 2).mean())
        lim_mean = (n + 1) * U64 * float(np.abs(v).max())
        lim_sd = lim_mean + (n / 2.0 + 3) * U64 * float(sd)
        print('stats rows %d channel %d: mean error %.3g (limit %.3g), deviation error %.3g (limit %.3g)' %
              (rows, c, abs(stats[c, 0] - mean), lim_mean, abs(stats[c, 1] - sd), lim_sd))
        assert abs(stats[c, 0] - mean) <= lim_mean and abs(stats[c, 1] - sd) <= lim_sd
    return stats


def check_degenerate(dev):
    from hoig_amd import _lib as L
    from hoig_amd.metrics import swd as S
    flat = np.full((3, 32, 32, 3), 128, np.uint8)
    flat[:, :, :, 1] = images(3, 32, 32, 1)[:, :, :, 1]                    # channel 1 lives, 0 and 2 are constant
    bank = S.SWDBank(0, PATCHES, None, 0, dev).append(to(dev, flat))
    stats, status = S.channel_stats(bank.rows(0))
    assert back(status).tolist() == [5] and 5 & L.SWD_DEGENERATE == 5 and np.isfinite(back(stats)).all()
    assert back(stats)[0, 1] == 0.0 and back(stats)[1, 1] > 0.0
    good = S.SWDBank(1, PATCHES, None, 0, dev).append(to(dev, images(3, 32, 32, 2)))
    try:
        S.swd_from_banks(bank, good, 2, 8, 0)
    except ValueError as e:
        assert 'generated' in str(e) and 'level 0' in str(e) and '0, 2' in str(e)
    else:
        raise AssertionError('a constant channel must be a ValueError')


# ------------------------------------------------------------------------------------------------ projection
PROJ_ROWS = (1, 63, 64, 65, 127, 129)             # the 64-row tile of the kernel: one below, at, one above; two tiles +- 1
PROJ_DIRS = (1, 5, 128)
IDENTITY = np.array([[0.0, 1.0]] * 3)


def check_project_exact(dev, rows, dirs):
    """Small integers and the identity normalisation: every product and sum is exact, so any lane of the tile that reads the wrong
    operand or stores to the wrong place shows."""
    from hoig_amd.metrics import swd as S
    g = np.random.default_rng(rows * 131 + dirs)
    x = g.integers(-8, 9, (rows, K)).astype(np.float32)
    w = g.integers(-4, 5, (K, dirs)).astype(np.float32)
    got = back(S.project(to(dev, x), to(dev, IDENTITY), to(dev, w)))
    assert got.shape == (dirs, rows) and np.array_equal(got, (x.astype(np.float64) @ w.astype(np.float64)).T)
    return got


def check_project(dev, rows, dirs):
    from hoig_amd.metrics import swd as S
    g = np.random.default_rng(rows * 17 + dirs)
    x = (g.standard_normal((rows, K)) * 40.0 + 3.0).astype(np.float32)
    stats = np.array([[2.5, 37.0], [-1.0, 41.5], [4.0, 44.25]])
    w = ref_directions(1, dirs, rows)[0]
    got = back(S.project(to(dev, x), to(dev, stats), to(dev, w)))
    z = (x.astype(np.float64) - np.repeat(stats[:, 0], 49)) / np.repeat(stats[:, 1], 49)
    want = (z @ w.astype(np.float64)).T
    limit = 149.0 * U32 * (np.abs(z) @ np.abs(w.astype(np.float64))).T
    print('projection %d x %d: error %.3g of limit %.3g' % (rows, dirs, np.abs(got - want).max(), limit.max()))
    assert (np.abs(got - want) <= limit).all()
    return got


# ------------------------------------------------------------------------------------------------ the sort
SORT_KINDS = ('normal', 'equal', 'sorted', 'reversed', 'dups', 'mix', 'highbytes')


def sort_sizes():
    from hoig_amd import _lib as L
    lds, tile = L.SORT_LDS_MAX, L.SORT_TILE
    assert lds + 1 < tile - 1                        # (the sizes around the tile take the multi-pass route)
    return [1, 2, 63, 64, 65, lds - 1, lds, lds + 1, tile - 1, tile, tile + 1, 3 * tile + 17]


# (S, n, kind) beyond the crossing of sort_sizes() with the kinds: many segments, and a long ragged segment near 2^18
SORT_LARGE = [(128, 8197, 'normal'), (128, 64, 'dups'), (128, 2048, 'mix'), (3, 262021, 'normal'), (1, 262021, 'highbytes'),
              (3, 262021, 'dups')]


def sort_keys(S, n, kind, seed=0):
    g = np.random.default_rng(seed + 1000 * S + n)
    if kind == 'normal':
        k = g.standard_normal((S, n))
    elif kind == 'equal':
        k = np.full((S, n), -2.5)
    elif kind == 'sorted':
        k = np.sort(g.standard_normal((S, n)), 1)
    elif kind == 'reversed':
        k = np.sort(g.standard_normal((S, n)), 1)[:, ::-1]
    elif kind == 'dups':
        k = g.standard_normal(16)[g.integers(0, 16, (S, n))]
    elif kind == 'mix':
        pool = np.array([0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.0, -1.0, 3e38, -3e38], np.float32)
        k = np.where(g.random((S, n)) < 0.5, pool[g.integers(0, pool.size, (S, n))], g.standard_normal((S, n)).astype(np.float32))
    else:
        # every key shares its two high bytes: the passes over them see a single occupied bucket
        return (np.uint32(0x3F800000) | g.integers(0, 1 << 16, (S, n)).astype(np.uint32)).view(np.float32)
    return np.ascontiguousarray(k.astype(np.float32))


def encode(keys):
    """The order-preserving map float -> uint32, restated."""
    b = keys.view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000))


def assert_sorted(got, keys):
    """np.sort exactly; and, because np.sort leaves the order of -0 and +0 open, the bits against np.sort of the integer keys."""
    assert got.dtype == np.float32 and got.shape == keys.shape
    assert np.array_equal(got, np.sort(keys, axis=1))
    assert np.array_equal(encode(got), np.sort(encode(keys), axis=1))


def check_sort(dev, S, n, kind):
    from hoig_amd.metrics import swd as Sw
    keys = sort_keys(S, n, kind)
    t = to(dev, keys)
    assert back(Sw.sort_segments(t)).tolist() == [0]
    assert_sorted(back(t), keys)


def check_sort_nan(dev, n):
    from hoig_amd import _lib as L
    from hoig_amd.metrics import swd as Sw
    keys = sort_keys(3, n, 'normal', 5)
    keys[1, n // 2] = np.nan
    t = to(dev, keys)
    assert back(Sw.sort_segments(t)).tolist() == [L.SORT_NAN]
    got = back(t)
    assert_sorted(got[[0, 2]], keys[[0, 2]])
    assert np.isnan(got[1]).sum() == 1
    clean = to(dev, sort_keys(3, n, 'normal', 6))
    assert back(Sw.sort_segments(clean)).tolist() == [0]          # the status is cleared by every call


def check_sort_unaligned(dev, n):
    from hoig_amd.metrics import swd as Sw
    keys = sort_keys(3, n, 'normal', 7)
    buf = torch.zeros(3 * n + 1, dtype=torch.float32, device=dev)
    view = buf[1:].view(3, n)
    view.copy_(to(dev, keys))
    assert view.data_ptr() % 16 == 4 or view.data_ptr() % 8 == 4
    assert back(Sw.sort_segments(view)).tolist() == [0]
    assert_sorted(back(view), keys)
    assert float(buf[0]) == 0.0


# ------------------------------------------------------------------------------------------------ sorted L1
L1_SIZES = (1, 63, 2049, 5000, 300001)


def check_l1_exact(dev, N):
    from hoig_amd.metrics import swd as S
    g = np.random.default_rng(N)
    a, b = g.integers(-1000, 1000, N).astype(np.float32), g.integers(-1000, 1000, N).astype(np.float32)
    got = back(S.sorted_l1(to(dev, a), to(dev, b)))
    assert got.dtype == np.float64 and got.tolist() == [float(np.abs(a.astype(np.int64) - b.astype(np.int64)).sum())]


def check_l1(dev, N):
    from hoig_amd.metrics import swd as S
    g = np.random.default_rng(N + 1)
    a, b = g.standard_normal(N).astype(np.float32), g.standard_normal(N).astype(np.float32)
    got = back(S.sorted_l1(to(dev, a), to(dev, b)))
    want = np.abs(a.astype(LD) - b.astype(LD)).sum()
    assert abs(got[0] - want) <= (N + 1) * U64 * float(want)
    return got


# ------------------------------------------------------------------------------------------------ end to end
E2E = dict(patches=5, dirs=8, repeats=2, seed=0)


def ref_directions(repeats, dirs, seed):
    d = np.random.default_rng(seed).standard_normal((repeats, K, dirs))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def ref_swd(gen, real, patches, repeats, dirs, seed, levels=None, ids=(0, 1)):
    """-> (per-level values, per-level limits) in float64 numpy."""
    n, H, W = gen.shape[:3]
    nl = levels_of(H, W, levels)
    w = ref_directions(repeats, dirs, seed).astype(np.float64)        # (fp32 values: the directions are an input of both sides)
    desc = [ref_descriptors(u8, nl, ref_positions(n, H, W, nl, patches, seed, sid)) for u8, sid in ((gen, ids[0]), (real, ids[1]))]
    values, limits = [], []
    for lv in range(nl):
        eps = lap_err(lv, nl) + REF
        z, dz = [], []
        for d in desc:
            x = d[lv].reshape(-1, 3, 49)
            mean, sd = x.mean((0, 2), keepdims=True), x.std((0, 2), keepdims=True)
            zz = ((x - mean) / sd).reshape(-1, K)
            z.append(zz)
            dz.append(eps * (2.0 + np.abs(zz)) / np.repeat((sd - eps).ravel(), 49))
        reps, lim = [], []
        for r in range(repeats):
            pa, pb = np.sort(z[0] @ w[r], axis=0), np.sort(z[1] @ w[r], axis=0)
            reps.append(np.abs(pa - pb).mean())
            lim.append(sum((e @ np.abs(w[r]) + 149.0 * U32 * (np.abs(q) @ np.abs(w[r]))).max() for q, e in zip(z, dz)))
        values.append(float(np.mean(reps)) * 1000.0)
        limits.append(max(lim) * 1000.0 * (1.0 + 1e-6))
    return values, limits


def e2e_sets():
    g = np.random.default_rng(2024)
    return g.integers(0, 256, (3, 32, 32, 3), dtype=np.uint8), g.integers(0, 256, (3, 32, 32, 3), dtype=np.uint8)


def bank(dev, u8, set_id, opts=E2E):
    from hoig_amd.metrics import swd as S
    return S.SWDBank(set_id, opts['patches'], None, opts['seed'], dev).append(to(dev, u8))


def check_end_to_end(dev):
    from hoig_amd.metrics import swd as S
    gen, real = e2e_sets()
    want, limit = ref_swd(gen, real, **E2E)
    d = S.directions(E2E['repeats'], E2E['dirs'], E2E['seed'])
    assert d.dtype == np.float32 and np.abs(d.astype(np.float64) - ref_directions(E2E['repeats'], E2E['dirs'], E2E['seed'])).max() <= U32
    got = S.swd_from_banks(bank(dev, gen, 0), bank(dev, real, 1), E2E['repeats'], E2E['dirs'], E2E['seed'])
    assert sorted(got) == ['swd', 'swd_levels', 'swd_sizes'] and got['swd_sizes'] == [(32, 32), (16, 16)]
    for lv in range(2):
        print('end to end level %d: %.9g against %.9g, error %.3g, limit %.3g' %
              (lv, got['swd_levels'][lv], want[lv], abs(got['swd_levels'][lv] - want[lv]), limit[lv]))
        assert abs(got['swd_levels'][lv] - want[lv]) <= limit[lv]
    assert got['swd'] == sum(got['swd_levels']) / 2.0 and got['swd'] > 1.0
    # identical sets: exactly 0 with one set id, and not with two (the sets draw their patches independently)
    same = S.swd_from_banks(bank(dev, gen, 0), bank(dev, gen, 0), E2E['repeats'], E2E['dirs'], E2E['seed'])
    assert same['swd'] == 0.0 and same['swd_levels'] == [0.0, 0.0]
    assert S.swd_from_banks(bank(dev, gen, 0), bank(dev, gen, 1), E2E['repeats'], E2E['dirs'], E2E['seed'])['swd'] > 0.0
    # symmetric in the two sets when each keeps its set id
    assert S.swd_from_banks(bank(dev, real, 1), bank(dev, gen, 0), E2E['repeats'], E2E['dirs'], E2E['seed']) == got
    return got


def check_argument_errors(dev):
    import pytest
    from hoig_amd.metrics import swd as S
    for shape in ((2, 40, 32, 3), (2, 15, 32, 3), (2, 32, 12, 3)):          # 40 = 8 * 5 is fine for two levels; 15 and 12 are below 16
        u8 = to(dev, np.zeros(shape, np.uint8))
        if shape[1] == 40:
            S.laplacian_descriptors_u8(u8, patches=2)
            continue
        with pytest.raises(ValueError, match='at least 16'):
            S.laplacian_descriptors_u8(u8, patches=2)
    with pytest.raises(ValueError, match='divisible by 2'):
        S.laplacian_descriptors_u8(to(dev, np.zeros((1, 33, 32, 3), np.uint8)), patches=2)
    with pytest.raises(ValueError, match='divisible by 4'):
        S.laplacian_descriptors_u8(to(dev, np.zeros((1, 64, 66, 3), np.uint8)), patches=2)
    S.laplacian_descriptors_u8(to(dev, np.zeros((1, 64, 66, 3), np.uint8)), levels=2, patches=2)
    gen, real = e2e_sets()
    with pytest.raises(ValueError, match='3 of .* and 2 of'):
        S.swd_from_banks(bank(dev, gen, 0), bank(dev, real[:2], 1), 2, 8, 0)
    with pytest.raises(ValueError, match=r'\(32, 32\) and 3 of \(64, 32\)'):
        S.swd_from_banks(bank(dev, gen, 0), bank(dev, images(3, 64, 32, 3), 1), 2, 8, 0)
    with pytest.raises(ValueError):
        S.laplacian_descriptors_u8(to(dev, gen), positions=np.full((3, 2, 1, 2), 26, np.int32))      # 26 > 32 - 7
    with pytest.raises(ValueError):
        S.swd_options(dict(patch=3))
    with pytest.raises(ValueError):
        S.swd_options(7)
