"""Truths, limits and the checks themselves for the fp64 FID statistics (hoig_amd/metrics/fid_device.py, hoig_amd/csrc/fid_stats.*):
tests/test_fid_device_cpu.py runs every check through the CPU twins (device 'cpu'), tests/test_fid_device_gpu.py through the kernels
(device 'cuda') -- the same truths and the same limits.

Where the limits come from (u = 2^-53, the unit roundoff of fp64):
  * a dot product of K terms made in any order carries at most K roundings per term (the product, then at most K - 1 additions), so
    |error| <= K u |a|^T |b| to first order; the fp32 mode adds the two pivot subtractions: (K + 2) u |A|^T |B|, element by element.
    An accumulated call continues the same sum, so two calls over K1 and K2 rows are held to the limit of one call over K1 + K2.
  * the moments: the same with A = B = X - p for C; s = sum(x - p) carries at most N roundings per term, |ds| <= (N + 1) u a with
    a = sum |x - p|.  sigma = (C - s s^T / n) / (n - 1) adds a product, two divisions, a subtraction and the symmetrising mean: with
    A = |X - p|^T |X - p|, |d sigma| <= (2 N + 16) u (A + a a^T / n) / (n - 1), and |d mu| <= (N + 4) u (a / n + |p|).  A merged
    state was rebased (C' = C_o + s_o d^T + d s_o^T + n_o d d^T, d = p_o - p): its magnitudes A and a are those of the terms that
    were actually added, taken around the pivot each part was summed at.
  * eigenvalues: 8 n 2^-52 max|lambda|, absolute.
  * the Frechet trace: the recorded errors below (measured through the CPU twins, docs/fid_device.md), times 8, at least 1e-13.
"""
import ctypes
import hashlib
import json
import os

import numpy as np
import torch

U = 2.0 ** -53
LD = np.longdouble

# ---- relative error of Tr sqrtm(S1 S2) through the CPU twins against the 60-digit truth, per class, and scipy's on the same inputs
# (printed by check_trace / check_closed_form on device 'cpu'; docs/fid_device.md has the table)
RECORDED_FULL_RANK = 3.63e-16          # (200, 200); scipy 2.49e-9
RECORDED_RANK_DEFICIENT = 5.47e-9      # the largest of the five rank-deficient cases, (3, 200)
RECORDED_CLOSED_2048 = 1.25e-16        # scipy 2.13e-15
SCIPY_RANK_DEFICIENT = 5.69e-8         # scipy's largest on the same five, (2, 2)
TRACE_CASES = [(40, 40), (40, 25), (25, 40), (200, 200), (2, 2), (3, 200)]
TRACE_RANKS = {(40, 40): (39, 39), (40, 25): (39, 24), (25, 40): (24, 39), (200, 200): (64, 64), (2, 2): (1, 1), (3, 200): (2, 64)}


def trace_limit(case):
    recorded = RECORDED_FULL_RANK if case == (200, 200) else RECORDED_RANK_DEFICIENT
    return max(8 * recorded, 1e-13)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def to(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def back(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ GEMM
GEMM_SHAPES = [(5, 64, 64), (50, 192, 192), (130, 39, 24), (1, 1, 1)]
# (shape, fp32 + pivot, accumulate, symmetric): every mode on every shape that admits it (the symmetric mode needs M == N)
GEMM_CASES = [(s, f32, acc, sym) for s in GEMM_SHAPES for f32 in (False, True) for acc in (False, True) for sym in (False, True)
              if not sym or s[1] == s[2]]


def gemm_id(v):
    return '%dx%dx%d' % v if isinstance(v, tuple) else str(int(v))


def gemm_operands(shape, f32, seed=0):
    K, M, N = shape
    g = np.random.default_rng(seed + 1000 * K + M)
    a, b = g.standard_normal((K, M)), g.standard_normal((K, N))
    pivot = None
    if f32:
        a, b = (np.abs(a) + 0.25).astype(np.float32), (np.abs(b) + 0.25).astype(np.float32)
        pivot = g.uniform(0.2, 1.0, max(M, N))
    return a, b, pivot


def gemm_truth(a, b, pivot):
    """(A^T B in longdouble, |A|^T |B| in fp64) of the operands as the kernel sees them."""
    al, bl = a.astype(LD), b.astype(LD)
    if pivot is not None:
        al, bl = al - pivot.astype(LD)[:a.shape[1]], bl - pivot.astype(LD)[:b.shape[1]]
    return al.T @ bl, (np.abs(al).T @ np.abs(bl)).astype(np.float64)


def check_gemm(dev, shape, f32, accumulate, symmetric):
    from hoig_amd import _lib as L
    from hoig_amd.metrics import fid_device as F
    K, M, N = shape
    a, b, pivot = gemm_operands(shape, f32)
    if symmetric:
        assert M == N
        b = a
    truth, mag = gemm_truth(a, b, pivot)
    limit = (K + 2) * U * mag
    flags = (L.GEMM_F32 if f32 else 0) | (L.GEMM_SYMMETRIC if symmetric else 0)
    ta = to(dev, a)
    tb = ta if symmetric else to(dev, b)
    tp = to(dev, pivot) if pivot is not None else None
    # C sits inside a wider block of sentinels: the leading dimension is explicit and nothing outside C is written
    wide = torch.full((M, N + 3), -7.0, dtype=torch.float64, device=dev)
    c = wide[:, :N]
    if accumulate:
        k1 = K // 2            # (K = 1: an empty first call, then all of it on top)
        F.gemm_tn(ta[:k1], tb[:k1] if not symmetric else ta[:k1], c, flags, tp)
        F.gemm_tn(ta[k1:], tb[k1:] if not symmetric else ta[k1:], c, flags | L.GEMM_ACCUMULATE, tp)
    else:
        F.gemm_tn(ta, tb, c, flags, tp)
    got = back(wide)
    assert (got[:, N:] == -7.0).all()
    err = np.abs(got[:, :N].astype(LD) - truth).astype(np.float64)
    print('gemm', dev, shape, 'f32' if f32 else 'f64', 'acc' if accumulate else '', 'sym' if symmetric else '',
          'max err / limit %.3g' % float((err / limit).max()))
    assert (err <= limit).all()
    if symmetric:
        assert np.array_equal(got[:, :N], got[:, :N].T)


# ------------------------------------------------------------------------------------------------ moments
def features(n, dims=64, seed=0):
    """Seeded non-negative fp32 features (ReLU + average pool gives such) with per-column scales from 1e-6 to 1."""
    g = np.random.default_rng(seed)
    scale = 10.0 ** np.linspace(-6, 0, dims)
    mix = g.standard_normal((dims, dims)) / np.sqrt(dims) + np.eye(dims)
    # (the product in longdouble: numpy's own loop, the same bits on every machine, which the recorded truths below rely on)
    x = np.abs((g.standard_normal((n, dims)).astype(LD) @ mix.astype(LD)).astype(np.float64) + 0.5) * scale
    return x.astype(np.float32)


def _magnitudes(parts, pivots, base):
    """A and a of the limit: every part around the pivot it was summed at, the rebase terms of the parts merged into `base`."""
    D = parts[0].shape[1]
    A, a = np.zeros((D, D)), np.zeros(D)
    for x, p in zip(parts, pivots):
        y = np.abs(x.astype(np.float64) - p)
        Ao, ao = y.T @ y, y.sum(0)
        d = np.abs(p - base)
        A += Ao + np.outer(ao, d) + np.outer(d, ao) + x.shape[0] * np.outer(d, d)
        a += ao + x.shape[0] * d
    return A, a


def check_moments(dev):
    from hoig_amd.metrics.fid_device import Moments
    x = features(61, 64, 3)
    cuts = [(0, 7), (7, 8), (8, 30)], [(30, 41), (41, 61)]          # uneven batches, two states
    states = []
    for group in cuts:
        m = Moments(64, dev)
        for lo, hi in group:
            m.update(to(dev, x[lo:hi]))
        states.append(m)
    first, second = states
    pivots = [back(first.pivot), back(second.pivot)]
    assert np.allclose(pivots[0], x[:7].astype(np.float64).mean(0), rtol=1e-14, atol=0)      # the first batch's mean
    saved = second.state_dict()
    first.merge(second)
    assert first.n == 61 and second.n == 31
    n = 61
    mu, sigma = (back(t) for t in first.statistics())
    xl = x.astype(LD)
    want_mu, want_sigma = np.mean(xl, axis=0), np.cov(xl, rowvar=False)
    A, a = _magnitudes([x[:30], x[30:]], pivots, pivots[0])
    lim_sigma = (2 * n + 16) * U * (A + np.outer(a, a) / n) / (n - 1)
    lim_mu = (n + 4) * U * (a / n + np.abs(pivots[0]))
    e_mu, e_sigma = np.abs(mu.astype(LD) - want_mu).astype(np.float64), np.abs(sigma.astype(LD) - want_sigma).astype(np.float64)
    print('moments', dev, 'mu err / limit %.3g' % float((e_mu / lim_mu).max()), 'sigma err / limit %.3g' % float((e_sigma / lim_sigma).max()))
    assert (e_mu <= lim_mu).all() and (e_sigma <= lim_sigma).all()
    assert np.array_equal(sigma, sigma.T)
    # a state round-trips through its dict, and the host statistics are the device's
    again = Moments(64, dev).load_state_dict(saved)
    assert again.n == 31 and torch.equal(again.C, second.C) and torch.equal(again.s, second.s)
    hm, hs = first.statistics_host()
    assert np.array_equal(hm, mu) and np.array_equal(hs, sigma)
    return lim_mu, lim_sigma


def moments_limits(x, pivot):
    """The limits for ONE state fed the rows x around `pivot` (numpy, fp64)."""
    n = x.shape[0]
    A, a = _magnitudes([x], [pivot], pivot)
    return (n + 4) * U * (a / n + np.abs(pivot)), (2 * n + 16) * U * (A + np.outer(a, a) / n) / (n - 1)


# ------------------------------------------------------------------------------------------------ covariances of the trace cases
_cov = {}


def covariance(n, seed, dims=64):
    if (n, seed, dims) not in _cov:
        x = features(n, dims, seed).astype(LD)             # (longdouble, rounded once: no BLAS, so the same bits everywhere)
        _cov[(n, seed, dims)] = (np.mean(x, axis=0).astype(np.float64), np.cov(x, rowvar=False).astype(np.float64))
    return _cov[(n, seed, dims)]


def case_statistics(case):
    (m1, s1), (m2, s2) = covariance(case[0], 11), covariance(case[1], 12)
    return m1, s1, m2, s2


# ------------------------------------------------------------------------------------------------ pivoted Cholesky
def check_pchol(dev):
    from hoig_amd.metrics.fid_device import pivoted_cholesky
    out = {}
    for n, rank in ((40, 39), (2, 1), (200, 64), (0, 0)):
        s = np.zeros((64, 64)) if n == 0 else covariance(n, 11)[1]
        fac, piv, info = pivoted_cholesky(to(dev, s))
        fac, piv, info = back(fac), back(piv), back(info)
        assert info.tolist() == [rank, 0], (n, info)
        assert (fac[:, rank:] == 0).all() and sorted(set(piv[:rank].tolist())) == sorted(piv[:rank].tolist())
        # the stop rule leaves a remaining diagonal of at most D 2^-52 d0, and a semi-definite remainder is bounded by its diagonal
        d0 = s.diagonal().max() if n else 0.0
        resid = np.abs(fac @ fac.T - s)
        assert resid.max() <= 64 * 2.0 ** -52 * d0 * 4, (n, resid.max(), d0)
        out[n] = (fac, piv, info)
    fac, piv, info = pivoted_cholesky(to(dev, np.eye(64)))
    assert back(info).tolist() == [64, 0] and back(piv).tolist() == list(range(64)) and np.array_equal(back(fac), np.eye(64))
    return out


# ------------------------------------------------------------------------------------------------ eigenvalues
def eig_matrices():
    g = np.random.default_rng(5)
    out = {}
    for n in (1, 2, 24, 39, 64, 192):
        a = g.standard_normal((n + 3, n))
        out['gram%d' % n] = a.T @ a
    out['identity'] = np.eye(24)
    q, _ = np.linalg.qr(g.standard_normal((40, 40)))
    w = np.concatenate([np.full(12, 3.0), np.full(12, 3.0 + 1e-13), g.uniform(0.1, 5.0, 16)])
    c = (q * w) @ q.T
    out['cluster'] = 0.5 * (c + c.T)
    out['zero'] = np.zeros((24, 24))
    return out


def check_eigvals(dev, name, a):
    from hoig_amd.metrics.fid_device import sym_eigvals
    n = a.shape[0]
    lam, info = sym_eigvals(to(dev, a))
    lam, want = back(lam), np.linalg.eigvalsh(a)
    limit = 8 * n * 2.0 ** -52 * np.abs(want).max()
    err = np.abs(lam - want).max()
    print('eigvals', dev, name, 'err %.3g limit %.3g' % (err, limit))
    assert back(info).tolist() == [0]
    assert (np.diff(lam) >= 0).all() and err <= limit
    return lam


# ------------------------------------------------------------------------------------------------ the trace: truth at 60 digits
_truth = {}


def mp_trace_truth(s1, s2):
    """Tr sqrtm(S1 S2) of the two fp64 matrices as they stand, at 60 digits: the sum of the principal square roots of the product's
    eigenvalues, real part (the matrices are symmetric only up to their own rounding, and a rank-deficient one is indefinite by it)."""
    import mpmath as mp
    with mp.workdps(60):
        prod = mp.matrix(s1.tolist()) * mp.matrix(s2.tolist())
        ev = mp.eig(prod, left=False, right=False)
        return float(mp.re(mp.fsum(mp.sqrt(mp.mpc(v)) for v in ev)))


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fid_device_truth.json')


def _digest(s1, s2):
    return hashlib.sha256(s1.tobytes() + s2.tobytes()).hexdigest()


def trace_truth(case):
    """The 60-digit truth of a case: recorded in tests/golden/fid_device_truth.json next to a digest of the two matrices it belongs to
    (about 20 s of mpmath per case); computed afresh where the matrices at hand are not those bits.
    ``python tests/fid_device_reference.py`` writes the file."""
    if case not in _truth:
        _, s1, _, s2 = case_statistics(case)
        recorded = {}
        if os.path.exists(GOLDEN):
            with open(GOLDEN) as f:
                recorded = json.load(f)
        entry = recorded.get('%d-%d' % case)
        _truth[case] = float(entry['truth']) if entry and entry['sha256'] == _digest(s1, s2) else mp_trace_truth(s1, s2)
    return _truth[case]


def scipy_trace(s1, s2):
    from scipy import linalg
    covmean, _ = linalg.sqrtm(s1.dot(s2), disp=False)
    return np.trace(covmean).real if np.isfinite(covmean).all() else float('nan')


def check_trace(dev, case):
    from hoig_amd.metrics.fid_device import sqrt_trace
    _, s1, _, s2 = case_statistics(case)
    truth = trace_truth(case)
    got, ranks = sqrt_trace(to(dev, s1), to(dev, s2))
    got = float(got)
    err = abs(got - truth) / truth
    sp = scipy_trace(s1, s2)
    sp_err = abs(sp - truth) / truth
    print('trace', dev, case, 'ranks', ranks, 'truth %.17g got %.17g rel err %.3g scipy %.3g limit %.3g' % (truth, got, err, sp_err,
                                                                                                         trace_limit(case)))
    assert tuple(ranks) == TRACE_RANKS[case]
    assert err <= trace_limit(case)
    if np.isfinite(sp_err):
        assert err <= 4 * sp_err
    return err, sp_err


# ------------------------------------------------------------------------------------------------ closed form at 2048 dims
_closed = {}


def closed_form(dims=2048):
    """S1 = Q diag(a) Q^T, S2 = Q diag(b) Q^T with Q = I - 2 u u^T a Householder reflector: Tr sqrtm(S1 S2) = sum sqrt(a b)."""
    if dims not in _closed:
        g = np.random.default_rng(9)
        u = g.standard_normal(dims)
        u /= np.linalg.norm(u)
        q = np.eye(dims) - 2.0 * np.outer(u, u)
        a, b = g.uniform(1e-3, 1.0, dims), g.uniform(1e-3, 1.0, dims)
        s1, s2 = (q * a) @ q.T, (q * b) @ q.T
        s1, s2 = 0.5 * (s1 + s1.T), 0.5 * (s2 + s2.T)
        truth = float(np.sum(np.sqrt(a.astype(LD) * b.astype(LD))))
        _closed[dims] = (s1, s2, truth)
    return _closed[dims]


def check_closed_form(dev):
    from hoig_amd.metrics.fid_device import sqrt_trace
    s1, s2, truth = closed_form()
    got, ranks = sqrt_trace(to(dev, s1), to(dev, s2))
    err = abs(float(got) - truth) / truth
    limit = max(8 * RECORDED_CLOSED_2048, 1e-13)
    print('closed form 2048', dev, 'ranks', ranks, 'rel err %.3g limit %.3g' % (err, limit))
    assert tuple(ranks) == (2048, 2048)
    assert err <= limit
    return err


if __name__ == '__main__':
    out = {}
    for case in TRACE_CASES:
        _, s1, _, s2 = case_statistics(case)
        out['%d-%d' % case] = {'sha256': _digest(s1, s2), 'truth': repr(mp_trace_truth(s1, s2))}
        print(case, out['%d-%d' % case])
    with open(GOLDEN, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
