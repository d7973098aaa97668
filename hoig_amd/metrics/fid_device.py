"""FID's statistics and distance without the host (opt-in; docs/fid_device.md): streaming fp64 moments of the Inception features and
the Frechet distance through a pivoted Cholesky and a symmetric eigenvalue kernel instead of scipy's sqrtm.

``Moments`` keeps, per image set, the count n, a pivot p (the mean of the first batch's rows, fixed afterwards), s = sum(x - p) and
C = sum (x - p)(x - p)^T; mu = p + s / n and sigma = (C - s s^T / n) / (n - 1) -- np.mean / np.cov in the shifted form
docs/norm_conditioning.md argues for.  Nothing of size N is kept, and two states merge.

``frechet_distance_device``: Tr sqrtm(S1 S2) is the nuclear norm of L2^T L1 for any factors Si = Li Li^T; the factors come from
hoig_pchol_f64, the singular values as the square roots of the eigenvalues of the smaller Gram matrix (hoig_gemm_tn_f64 twice,
hoig_sym_eigvals_f64).  Where scipy's sqrtm is non-finite, fid.calculate_frechet_distance adds 1e-6 to both diagonals; this function
returns the value of the formula itself.

Every function here runs on the tensors' own device: CUDA tensors go to the kernels, CPU tensors to their host twins
(``frechet_distance_host_twin``, ``Moments(dims, 'cpu')``), which walk the same code.
"""
import os

import numpy as np
import torch

from .. import _lib as L
from .._twin import ptr as _p, run as _run


def fid_device_option(value):
    """The fid_device / device_stats argument: None takes HOIG_DEVICE_FID=1 (off otherwise)."""
    return os.environ.get('HOIG_DEVICE_FID', '') == '1' if value is None else bool(value)


def _ld(t):
    """Leading dimension of a 2-D tensor whose rows are contiguous (a column slice of a larger matrix included)."""
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError('a matrix with contiguous rows expected, got shape %s strides %s' % (tuple(t.shape), t.stride()))
    return t.stride(0) if t.shape[0] > 1 and t.stride(0) >= t.shape[1] else t.shape[1]


def gemm_tn(a, b, c, flags=0, pivot=None):
    """c [M, N] (+)= a^T b for a [K, M], b [K, N] (hoig_gemm_tn_f64): fp64, or fp32 with GEMM_F32 (then minus `pivot` per column)."""
    want = torch.float32 if flags & L.GEMM_F32 else torch.float64
    if a.dtype != want or b.dtype != want or c.dtype != torch.float64 or a.shape[0] != b.shape[0] or \
            c.shape != (a.shape[1], b.shape[1]) or not (a.device == b.device == c.device):
        raise ValueError('gemm_tn: %s %s x %s %s -> %s %s' % (a.dtype, tuple(a.shape), b.dtype, tuple(b.shape), c.dtype, tuple(c.shape)))
    _run('hoig_gemm_tn_f64', c, (_p(a), _ld(a), _p(b), _ld(b), _p(pivot), _p(c), _ld(c), a.shape[1], b.shape[1], a.shape[0], flags))
    return c


def pivoted_cholesky(sigma):
    """-> (L [D, D] with zeros right of the rank, piv [D] int32, info [2] int32 = rank, status) on sigma's device; no sync."""
    D = sigma.shape[0]
    if sigma.dim() != 2 or sigma.shape[1] != D or sigma.dtype != torch.float64:
        raise ValueError('a square fp64 matrix expected, got %s %s' % (sigma.dtype, tuple(sigma.shape)))
    dev = sigma.device
    fac = torch.zeros((D, D), dtype=torch.float64, device=dev)
    piv = torch.full((D,), -1, dtype=torch.int32, device=dev)
    info = torch.zeros((2,), dtype=torch.int32, device=dev)
    tail = ()
    if sigma.is_cuda:
        nbytes = L.lib.hoig_pchol_f64_workspace_bytes(D)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        tail = (_p(ws), nbytes)
    try:
        _run('hoig_pchol_f64', sigma, (_p(sigma), _ld(sigma), D, _p(fac), D, _p(piv), _p(info)), tail=tail)
    except L.HoigKernelError:
        if sigma.is_cuda or int(info[1]) == 0:
            raise                         # (the twin also returns the status it writes)
    return fac, piv, info


def sym_eigvals(a):
    """-> (eigenvalues ascending [n], NaN where the kernel refused its input; info [1] int32 = status) on a's device; no sync."""
    n = a.shape[0]
    if a.dim() != 2 or a.shape[1] != n or a.dtype != torch.float64:
        raise ValueError('a square fp64 matrix expected, got %s %s' % (a.dtype, tuple(a.shape)))
    lam = torch.full((n,), float('nan'), dtype=torch.float64, device=a.device)
    info = torch.zeros((1,), dtype=torch.int32, device=a.device)
    tail = ()
    if a.is_cuda:
        nbytes = L.lib.hoig_sym_eigvals_f64_workspace_bytes(n)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=a.device)
        tail = (_p(ws), nbytes)
    try:
        _run('hoig_sym_eigvals_f64', a, (_p(a), _ld(a), n, _p(lam), _p(info)), tail=tail)
    except L.HoigKernelError:
        if a.is_cuda or int(info[0]) == 0:
            raise
    return lam, info


class Moments(object):
    """Streaming mean and covariance of feature rows in fp64 on `device` ('cpu': through the host twins)."""

    def __init__(self, dims, device=None):
        self.dims, self.device = int(dims), torch.device(device if device is not None else 'cuda')
        self.n = 0                        # (known from the shapes alone, so a Python int: reading it never waits for the device)
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=self.device)
        self.pivot, self.s, self.C = z(self.dims), z(self.dims), z(self.dims, self.dims)

    def update(self, feats):
        """fp32 [B, dims] on this state's device (what InceptionFeatures.features_u8 returns); fp32 -> fp64 is exact."""
        if feats.dtype != torch.float32 or feats.dim() != 2 or feats.shape[1] != self.dims or feats.device.type != self.device.type:
            raise ValueError('fp32 [B, %d] on %s expected, got %s %s on %s' % (self.dims, self.device, feats.dtype, tuple(feats.shape),
                                                                              feats.device))
        if feats.shape[0] == 0:
            return self
        feats = feats.contiguous()
        x = feats.double()
        if self.n == 0:
            self.pivot = x.mean(0)
        self.s += (x - self.pivot).sum(0)
        gemm_tn(feats, feats, self.C, L.GEMM_F32 | L.GEMM_SYMMETRIC | L.GEMM_ACCUMULATE, self.pivot)
        self.n += feats.shape[0]
        return self

    def copy(self):
        m = Moments.__new__(Moments)
        m.dims, m.device, m.n = self.dims, self.device, self.n
        m.pivot, m.s, m.C = self.pivot.clone(), self.s.clone(), self.C.clone()
        return m

    def merge(self, other):
        """Adds `other`'s rows: its sums are rebased to this pivot (d = p_other - p: s' = s_o + n_o d,
        C' = C_o + s_o d^T + d s_o^T + n_o d d^T)."""
        if other.dims != self.dims:
            raise ValueError('merge: %d and %d dims' % (self.dims, other.dims))
        if other.n == 0:
            return self
        op, os_, oc = (t.to(self.device) for t in (other.pivot, other.s, other.C))
        if self.n == 0:
            self.pivot, self.s, self.C, self.n = op.clone(), os_.clone(), oc.clone(), other.n
            return self
        d = op - self.pivot
        self.s += os_ + other.n * d
        self.C += oc + (torch.outer(os_, d) + torch.outer(d, os_)) + other.n * torch.outer(d, d)
        self.n += other.n
        return self

    def statistics(self):
        """(mu [dims], sigma [dims, dims]) in fp64 on the device: np.mean(act, 0), np.cov(act, rowvar=False)."""
        if self.n == 0:
            raise ValueError('no images were given')
        mu = self.pivot + self.s / self.n
        sigma = (self.C - torch.outer(self.s, self.s) / self.n) / (self.n - 1)
        return mu, 0.5 * (sigma + sigma.t())

    def statistics_host(self):
        mu, sigma = self.statistics()
        return mu.cpu().numpy(), sigma.cpu().numpy()

    def state_dict(self):
        return {'n': torch.tensor(self.n, dtype=torch.int64), 'pivot': self.pivot.clone(), 's': self.s.clone(), 'C': self.C.clone()}

    def load_state_dict(self, state):
        if tuple(state['C'].shape) != (self.dims, self.dims):
            raise ValueError('load_state_dict: C %s for %d dims' % (tuple(state['C'].shape), self.dims))
        self.n = int(state['n'])
        self.pivot, self.s, self.C = (state[k].to(self.device, torch.float64).clone() for k in ('pivot', 's', 'C'))
        return self


def _tensor(x, device):
    if isinstance(x, torch.Tensor):
        return x.detach().to(device, torch.float64)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64))).to(device)


def sqrt_trace(sigma1, sigma2):
    """Tr sqrtm(sigma1 sigma2) as a 0-d tensor on the inputs' device, and the two ranks.  Synchronises once, to read the ranks."""
    f1, _, info1 = pivoted_cholesky(sigma1)
    f2, _, info2 = pivoted_cholesky(sigma2)
    (r1, st1), (r2, st2) = torch.stack([info1, info2]).tolist()
    if st1 != 0 or st2 != 0:
        raise ValueError('frechet distance: a covariance has a non-finite entry')
    if min(r1, r2) == 0:
        return torch.zeros((), dtype=torch.float64, device=sigma1.device), (r1, r2)
    # h = (larger factor)^T (smaller factor); the Gram matrix of its columns, the smaller side, has no structurally zero eigenvalue
    big, small = (f1[:, :r1], f2[:, :r2]) if r2 <= r1 else (f2[:, :r2], f1[:, :r1])
    h = gemm_tn(big, small, torch.empty((big.shape[1], small.shape[1]), dtype=torch.float64, device=sigma1.device))
    gram = gemm_tn(h, h, torch.empty((h.shape[1], h.shape[1]), dtype=torch.float64, device=sigma1.device), L.GEMM_SYMMETRIC)
    lam, _ = sym_eigvals(gram)
    return lam.clamp_min(0.0).sqrt().sum(), (r1, r2)


def _frechet(mu1, sigma1, mu2, sigma2, device):
    mu1, sigma1, mu2, sigma2 = (_tensor(x, device) for x in (mu1, sigma1, mu2, sigma2))
    mu1, mu2 = mu1.reshape(-1), mu2.reshape(-1)
    if mu1.shape != mu2.shape:
        raise ValueError('Training and test mean vectors have different lengths')
    if sigma1.shape != sigma2.shape or sigma1.shape != (mu1.shape[0], mu1.shape[0]):
        raise ValueError('Training and test covariances have different dimensions')
    tr, _ = sqrt_trace(sigma1.contiguous(), sigma2.contiguous())
    diff = mu1 - mu2
    value = (diff.dot(diff) + torch.trace(sigma1) + torch.trace(sigma2) - 2.0 * tr).item()
    if not np.isfinite(value):
        raise ValueError('frechet distance: non-finite statistics')
    return value


def frechet_distance_device(mu1, sigma1, mu2, sigma2, device=None):
    """||mu1 - mu2||^2 + Tr S1 + Tr S2 - 2 Tr sqrtm(S1 S2) on the device; numpy arrays (an .npz reference) or tensors."""
    if device is None:
        on = [x.device for x in (mu1, sigma1, mu2, sigma2) if isinstance(x, torch.Tensor) and x.is_cuda]
        device = on[0] if on else 'cuda'
    return _frechet(mu1, sigma1, mu2, sigma2, torch.device(device))


def frechet_distance_host_twin(mu1, sigma1, mu2, sigma2):
    """The same through the CPU twins of the kernels."""
    return _frechet(mu1, sigma1, mu2, sigma2, torch.device('cpu'))
