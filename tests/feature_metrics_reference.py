"""Truths, limits and the checks themselves for the feature-space metrics (hoig_amd/metrics/feature_metrics.py,
hoig_amd/csrc/feature_metrics.*): tests/test_feature_metrics_cpu.py runs every check through the CPU twins (device 'cpu'),
tests/test_feature_metrics_gpu.py through the kernels (device 'cuda') -- the same truths and the same limits.

The truths are np.longdouble restatements of the published estimators (Binkowski et al. 2018; Kynkaanniemi et al. 2019; Naeem et al.
2020): Gram matrices by longdouble products, distances as direct sums of (x - y)^2, radii by np.sort.  Nothing of the product is used.

Where the limits come from (U = 2^-53; first order; docs/feature_metrics.md has the derivation):
  * a dot product of D terms made in any order, on operands that carry up to one rounding each (the pivot subtraction):
    |d dot| <= (D + 2) U A with A = sum |x_k y_k| -- the rule of tests/fid_device_reference.py's check_gemm.
  * b = gamma dot + coef0 (a product and a sum): |db| <= |gamma| (D + 2) U A + 2 U B with B = |gamma| A + |coef0| >= |b|.
  * p = b^degree by degree - 1 products: |dp| <= degree B^(degree - 1) |db| + (degree - 1) U B^degree.
  * a sum of N such terms in any order: |dS| <= sum |dp| + N U sum B^degree.
  * mmd^2 = Sxx / (m (m - 1)) + Syy / (m (m - 1)) - 2 Sxy / m^2: the sums' limits through the same formula, plus 4 U of the formula
    on the magnitudes (three quotients, one product by 2, two sums).
  * the mean over S subsets: the mean of the limits plus (S + 1) U of the mean magnitude; the population standard deviation is
    1-Lipschitz in the largest perturbation of a sample (std(v) = |v - mean v|_2 / sqrt S and v -> v - mean v is a projection):
    the largest per-subset limit, plus (S + 8) U of twice the largest magnitude for its own arithmetic.
  * d^2 = (|a|^2 + |b|^2) - 2 a.b on a = fl(x - pivot): each of the three products within (D + 2) U of its magnitude, two sums and
    the product by 2: |d d^2| <= (D + 4) U (|a|^2 + |b|^2 + 2 sum |a_k b_k|).  The clamp at 0 moves a value towards the truth.
    The k-th smallest of a list is 1-Lipschitz in the largest perturbation of an entry: a radius is held to the largest limit of its row.
"""
import ctypes

import numpy as np
import torch

U = 2.0 ** -53
LD = np.longdouble


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def to(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def back(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ KID
KID_DIMS = (1, 5, 37, 64)
KID_SIZES = (2, 15, 16, 17, 63, 64, 65, 130)     # one below, at and one above the MFMA tile and the workgroup tile; three tiles a side
# (D, m, S, degree): every D with every m; S in {1, 3} and degree 1 .. 4 walk along; and the long-K case
KID_CASES = [(D, m, (1, 3)[(a + b) % 2], 1 + (a + b) % 4) for a, m in enumerate(KID_SIZES) for b, D in enumerate(KID_DIMS)] + \
            [(2048, 100, 2, 3)]


def kid_id(case):
    return 'D%d-m%d-S%d-deg%d' % case


def kid_inputs(case, seed=0):
    """Non-negative fp32 features (as ReLU and an average pool give), nx != ny, and subsets that share rows: the pools are only a
    few rows larger than a subset."""
    D, m, S, _ = case
    g = np.random.default_rng(seed + 7 * D + m)
    x = (np.abs(g.standard_normal((m + 7, D))) + 0.1).astype(np.float32)
    y = (np.abs(g.standard_normal((m + 3, D)) * 1.2 + 0.3) + 0.1).astype(np.float32)
    ix = np.stack([g.permutation(m + 7)[:m] for _ in range(S)]).astype(np.int32)
    iy = np.stack([g.permutation(m + 3)[:m] for _ in range(S)]).astype(np.int32)
    return x, y, ix, iy


def kid_truth(x, y, ix, iy, degree, gamma, coef0):
    """-> (truth [S, 4] longdouble, limit [S, 4] fp64, magnitude of mmd^2 [S] fp64)"""
    D = x.shape[1]
    S, m = ix.shape
    truth, limit, mags = np.zeros((S, 4), LD), np.zeros((S, 4)), np.zeros(S)
    off = ~np.eye(m, dtype=bool)
    for s in range(S):
        xs, ys = x[ix[s]].astype(LD), y[iy[s]].astype(LD)
        sums, lims, tops = [], [], []
        for a, b, mask in ((xs, xs, off), (ys, ys, off), (xs, ys, np.ones((m, m), bool))):
            k = (LD(gamma) * (a @ b.T) + LD(coef0)) ** degree
            A = (np.abs(a) @ np.abs(b).T).astype(np.float64)
            B = abs(gamma) * A + abs(coef0)
            db = abs(gamma) * (D + 2) * U * A + 2 * U * B
            dp = degree * B ** (degree - 1) * db + (degree - 1) * U * B ** degree
            n = int(mask.sum())
            sums.append(k[mask].sum())
            tops.append(float((B ** degree)[mask].sum()))
            lims.append(float(dp[mask].sum()) + n * U * tops[-1])
        pairs, both = LD(m) * LD(m - 1), LD(m) * LD(m)
        truth[s] = sums + [sums[0] / pairs + sums[1] / pairs - 2 * sums[2] / both]
        mags[s] = tops[0] / float(pairs) + tops[1] / float(pairs) + 2 * tops[2] / float(both)
        limit[s] = lims + [lims[0] / float(pairs) + lims[1] / float(pairs) + 2 * lims[2] / float(both) + 4 * U * mags[s]]
    return truth, limit, mags


def check_kid(dev, case):
    """The per-subset sums and mmd^2 of kid_sums, and the mean and the standard deviation over the subsets, within the limits."""
    from hoig_amd.metrics import feature_metrics as F
    D, m, S, degree = case
    gamma, coef0 = 1.0 / D, 1.0
    x, y, ix, iy = kid_inputs(case)
    truth, limit, mags = kid_truth(x, y, ix, iy, degree, gamma, coef0)
    out, status = F.kid_sums(to(dev, x), to(dev, y), ix, iy, degree, None, coef0)
    assert back(status).tolist() == [0]
    got = back(out)
    err = np.abs(got.astype(LD) - truth).astype(np.float64)
    print('kid', dev, kid_id(case), 'max err / limit %.3g' % float((err / limit).max()))
    assert (err <= limit).all()
    mean, std = float(np.mean(got[:, 3])), float(np.std(got[:, 3]))
    t = truth[:, 3]
    t_mean = t.sum() / LD(S)
    t_std = np.sqrt(((t - t_mean) ** 2).sum() / LD(S))
    lim_mean = float(limit[:, 3].mean()) + (S + 1) * U * float(mags.mean())
    lim_std = float(limit[:, 3].max()) + (S + 8) * U * 2 * float(mags.max())
    e_mean, e_std = float(abs(LD(mean) - t_mean)), float(abs(LD(std) - t_std))
    print('kid', dev, kid_id(case), 'mean err / limit %.3g std err / limit %.3g' % (e_mean / lim_mean, e_std / lim_std))
    assert e_mean <= lim_mean and e_std <= lim_std
    return got


def kid_exact_sums(x, y, ix, iy):
    """Integer features, gamma = 1/8, coef0 = 1, degree 3: k = (dot + 8)^3 / 512 with every product, power and sum exact in fp64.
    -> [S, 3] sums by integer arithmetic."""
    S, m = ix.shape
    out = np.zeros((S, 3))
    for s in range(S):
        xs, ys = x[ix[s]].astype(np.int64), y[iy[s]].astype(np.int64)
        kxx, kyy, kxy = ((a @ b.T + 8) ** 3 for a, b in ((xs, xs), (ys, ys), (xs, ys)))
        total = [int(kxx.sum() - np.trace(kxx)), int(kyy.sum() - np.trace(kyy)), int(kxy.sum())]
        assert max(total) < 2 ** 53
        out[s] = [t / 512.0 for t in total]
    return out


def check_kid_exact(dev, onehot):
    """The lane maps on exact integers: m = 150 (three tiles a side, the last ragged), S = 2, a gather in a permuted order.  The three
    sums must EQUAL the integer arithmetic.  onehot: row r is a_r e_r, so that only the position pairs that meet in one row have a
    kernel value other than 1 -- the excluded diagonal of xx and yy, and a scattered set for xy: a swapped row / column map or a
    wrongly counted mirror tile gives another VALUE."""
    from hoig_amd.metrics import feature_metrics as F
    g = np.random.default_rng(5 + onehot)
    m, S = 150, 2
    if onehot:
        D = nx = ny = m
        x = (np.eye(m) * g.integers(1, 4, m)[:, None]).astype(np.float32)
        y = (np.eye(m) * g.integers(1, 4, m)[:, None]).astype(np.float32)
    else:
        D, nx, ny = 37, 170, 163
        x, y = g.integers(-3, 4, (nx, D)).astype(np.float32), g.integers(-3, 4, (ny, D)).astype(np.float32)
    ix = np.stack([g.permutation(nx)[:m] for _ in range(S)]).astype(np.int32)
    iy = np.stack([g.permutation(ny)[:m] for _ in range(S)]).astype(np.int32)
    want = kid_exact_sums(x, y, ix, iy)
    out, status = F.kid_sums(to(dev, x), to(dev, y), ix, iy, 3, 0.125, 1.0)
    got = back(out)
    assert back(status).tolist() == [0]
    assert np.array_equal(got[:, :3], want), (got[:, :3], want)
    pairs, both = float(m * (m - 1)), float(m * m)
    assert np.array_equal(got[:, 3], (want[:, 0] / pairs + want[:, 1] / pairs) - (2.0 * want[:, 2]) / both)
    return got


FINISH_S, FINISH_M = 3, 577              # ten tiles a side: 100 slots per term, more than one round of the 64 lanes


def finish_partials():
    nt = (FINISH_M + 63) // 64
    return np.random.default_rng(11).standard_normal((FINISH_S, 3, nt * nt)) * 1e3


def check_finish(dev):
    """hoig_kid_finish_f64 on given partials: the sums within N U sum |p| of the longdouble sums of the slots that run; -> out for the
    bit-for-bit comparison of device and twin."""
    from hoig_amd import _lib as L
    part = finish_partials()
    nt = (FINISH_M + 63) // 64
    runs = np.array([[term == 2 or e % nt >= e // nt for e in range(nt * nt)] for term in range(3)])
    tp = to(dev, part)
    out = torch.zeros((FINISH_S, 4), dtype=torch.float64, device=dev)
    if dev == 'cpu':
        L.call('hoig_kid_finish_f64_host', _p(tp), FINISH_S, FINISH_M, None, _p(out))
    else:
        L.call('hoig_kid_finish_f64', _p(tp), FINISH_S, FINISH_M, None, _p(out), torch.cuda.current_stream().cuda_stream)
    got = back(out)
    for s in range(FINISH_S):
        for term in range(3):
            p = part[s, term][runs[term]]
            assert abs(LD(got[s, term]) - p.astype(LD).sum()) <= p.size * U * np.abs(p).sum()
    return got


# ------------------------------------------------------------------------------------------------ radii
RADII_CASES = [(2, 5, 1), (16, 5, 3), (40, 37, 3), (65, 37, 5), (130, 64, 8)]       # (n, D, k)


def gaussians(n, D, seed, shift=0.0, scale=1.0):
    """Seeded Gaussians cast to fp32, plus a common offset of +3 per column, so that the pivot matters."""
    g = np.random.default_rng(seed)
    return (g.standard_normal((n, D)) * scale + shift + 3.0).astype(np.float32)


def dist2_truth(x, y):
    """Direct sums of (x - y)^2 in longdouble, [nx, ny]."""
    xl, yl = x.astype(LD), y.astype(LD)
    return np.stack([((xi[None, :] - yl) ** 2).sum(1) for xi in xl])


def radii_truth(x, k):
    d = dist2_truth(x, x)
    n = x.shape[0]
    return np.array([np.sort(d[i][np.arange(n) != i])[k - 1] for i in range(n)], LD)


def dist2_limit(x, y, pivot):
    """(D + 4) U (|a|^2 + |b|^2 + 2 |a|.|b|) on the pivoted operands, [nx, ny]."""
    a, b = np.abs(x.astype(np.float64) - pivot), np.abs(y.astype(np.float64) - pivot)
    return (x.shape[1] + 4) * U * ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] + 2 * (a @ b.T))


def check_radii(dev, case, duplicate=False):
    from hoig_amd.metrics import feature_metrics as F
    n, D, k = case
    x = gaussians(n, D, 100 + n)
    if duplicate:
        x[n - 1] = x[1]
    pivot = x.astype(np.float64).mean(0)
    truth = radii_truth(x, k)
    lim = dist2_limit(x, x, pivot)
    np.fill_diagonal(lim, 0.0)
    limit = lim.max(1)
    radius, status = F.knn_radii(to(dev, x), k, to(dev, pivot))
    got = back(radius)
    assert back(status).tolist() == [0]
    assert np.isfinite(got).all() and (got >= 0.0).all()
    err = np.abs(got.astype(LD) - truth).astype(np.float64)
    print('radii', dev, case, 'dup' if duplicate else '', 'max err / limit %.3g' % float((err / limit).max()))
    assert (err <= limit).all()
    if duplicate and k == 1:
        assert truth[1] == 0 and truth[n - 1] == 0
    # without the pivot the same limit holds on the unpivoted magnitudes (which are larger): the operands are then exact
    radius0, _ = F.knn_radii(to(dev, x), k, None)
    lim0 = dist2_limit(x, x, np.zeros(D))
    np.fill_diagonal(lim0, 0.0)
    assert (np.abs(back(radius0).astype(LD) - truth).astype(np.float64) <= lim0.max(1)).all()
    return got


# ------------------------------------------------------------------------------------------------ hits, precision, recall, density
# ((n_real, n_fake, D), shift, scale, seed) with k = 3; the fake set is N(shift, scale^2) around the real set's N(0, 1)
PRC_K = 3
PRC_CASES = [((40, 33, 37), 0.3, 1.2, 0), ((65, 17, 37), 0.4, 1.0, 1), ((130, 100, 64), 0.5, 0.9, 0), ((16, 16, 5), 0.6, 0.8, 1)]
PRC_GAP = 1e-9


def prc_id(case):
    return '%dx%dx%d' % case[0]


def prc_inputs(case):
    (n_real, n_fake, D), shift, scale, seed = case
    return gaussians(n_real, D, 1000 + seed), gaussians(n_fake, D, 2000 + seed, shift, scale)


_PRC_TRUTH = {}


def prc_truth(case):
    """-> dict(in_real: hits of the fake rows in the real balls, in_fake: the other way, precision, recall, density, gap), computed
    once per case.  Asserts that no d^2 / r - 1 lies within PRC_GAP of 0: the counts do not hang on a rounding."""
    if case not in _PRC_TRUTH:
        real, fake = prc_inputs(case)
        r_real, r_fake = radii_truth(real, PRC_K), radii_truth(fake, PRC_K)
        d = dist2_truth(real, fake)                                     # [n_real, n_fake]
        gap = min(np.abs(d / r_real[:, None] - 1).min(), np.abs(d.T / r_fake[:, None] - 1).min())
        assert gap > PRC_GAP, gap
        in_real = (d <= r_real[:, None]).sum(0).astype(np.int32)
        in_fake = (d.T <= r_fake[:, None]).sum(0).astype(np.int32)
        _PRC_TRUTH[case] = dict(in_real=in_real, in_fake=in_fake, precision=float(np.mean(in_real > 0)),
                                recall=float(np.mean(in_fake > 0)), density=float(in_real.sum()) / (PRC_K * in_real.shape[0]),
                                gap=float(gap))
    return _PRC_TRUTH[case]


def prc_reference_is_informative():
    """Precision and recall are neither all 0 nor all 1 in at least three of the four cases."""
    inside = [0.0 < prc_truth(c)['precision'] < 1.0 and 0.0 < prc_truth(c)['recall'] < 1.0 for c in PRC_CASES]
    return sum(inside) >= 3


def check_prc(dev, case):
    """The counts must be EQUAL to the reference's, and so precision, recall and density."""
    from hoig_amd.metrics import feature_metrics as F
    real, fake = prc_inputs(case)
    want = prc_truth(case)
    in_real, in_fake = F.manifold_counts(to(dev, real), to(dev, fake), PRC_K)
    print('prc', dev, prc_id(case), 'precision %.3f recall %.3f density %.3f smallest gap %.3g' %
          (want['precision'], want['recall'], want['density'], want['gap']))
    assert in_real.dtype == np.int32 and np.array_equal(in_real, want['in_real']) and np.array_equal(in_fake, want['in_fake'])
    got = F.precision_recall_from_features(to(dev, real), to(dev, fake), PRC_K)
    assert got == {'precision': want['precision'], 'recall': want['recall'], 'density': want['density']}
    return got
