"""KID and improved precision / recall (with density) on Inception features that stay on the device (docs/feature_metrics.md).

``kid_from_features``: the Kernel Inception Distance of Binkowski et al. 2018 -- the unbiased MMD^2 estimate under the polynomial
kernel (gamma x.y + coef0)^degree on `subsets` random subsets of `subset_size` rows, its mean and its standard deviation over the
subsets.  ``precision_recall_from_features``: Kynkaanniemi et al. 2019 -- every row of a set carries a ball whose radius is the
distance to its k-th nearest neighbour in that set; precision is the share of generated rows inside some real ball, recall the share
of real rows inside some generated ball -- and the density of Naeem et al. 2020, the mean number of real balls a generated row lies
in, over k.  ``FeatureBank`` keeps the fp32 blocks InceptionFeatures.features_u8 returns.

Every product is made by the fp64 kernels of hoig_amd/csrc/feature_metrics.hip; nothing of size m x m or n x n is stored.  CUDA
tensors go to the kernels, CPU tensors to their host twins, which walk the same code.
"""
import numpy as np
import torch

from .. import _lib as L
from .._twin import ptr as _p, run as _run


def _features(x, name):
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError('%s: fp32 [N, dims] expected, got %s %s' % (name, x.dtype, tuple(x.shape)))
    return x.detach().contiguous()


def _status_error(what, status):
    parts = [text for bit, text in ((L.FM_NONFINITE, 'a non-finite feature'), (L.FM_CLAMPED, 'an index outside its set')) if status & bit]
    return ValueError('%s: %s' % (what, ' and '.join(parts) or 'status %d' % status))


# ------------------------------------------------------------------------------------------------ KID
def draw_subsets(nx, ny, subsets, m, seed):
    """The gather tables ix, iy [subsets, m] (int32, numpy).  The draw order is part of the value: ONE
    np.random.RandomState(seed) per call, and for subset 0, 1, .. in turn choice(nx, m, replace=False), then
    choice(ny, m, replace=False)."""
    rng = np.random.RandomState(seed)
    ix, iy = np.empty((subsets, m), np.int32), np.empty((subsets, m), np.int32)
    for s in range(subsets):
        ix[s] = rng.choice(nx, m, replace=False)
        iy[s] = rng.choice(ny, m, replace=False)
    return ix, iy


def _check_table(name, idx, subsets, m, n):
    idx = np.ascontiguousarray(np.asarray(idx))
    if idx.shape != (subsets, m) or idx.dtype.kind not in 'iu':
        raise ValueError('%s: an integer [%d, %d] table expected, got %s %s' % (name, subsets, m, idx.dtype, idx.shape))
    if idx.size and (idx.min() < 0 or idx.max() >= n):
        raise ValueError('%s: an index outside [0, %d)' % (name, n))
    return idx.astype(np.int32)


def kid_sums(x, y, ix, iy, degree=3, gamma=None, coef0=1.0):
    """-> (out [S, 4] fp64 = per subset {sum_xx, sum_yy, sum_xy, mmd^2}, status [1] int32) on x's device; no sync.  ix, iy:
    [S, m] integer tables (numpy or lists), checked here on the host -- an index outside its set is a ValueError -- and uploaded."""
    x, y = _features(x, 'x'), _features(y, 'y')
    if y.shape[1] != x.shape[1] or y.device != x.device:
        raise ValueError('x %s on %s and y %s on %s' % (tuple(x.shape), x.device, tuple(y.shape), y.device))
    ix = np.asarray(ix)
    if ix.ndim != 2 or ix.shape[0] < 1 or ix.shape[1] < 2:
        raise ValueError('ix: [S >= 1, m >= 2] expected, got %s' % (ix.shape,))
    S, m = ix.shape
    ix, iy = _check_table('ix', ix, S, m, x.shape[0]), _check_table('iy', iy, S, m, y.shape[0])
    if int(degree) != degree or not 1 <= degree <= 4:
        raise ValueError('degree %r: 1 .. 4' % (degree,))
    gamma = 1.0 / x.shape[1] if gamma is None else float(gamma)
    tix, tiy = torch.from_numpy(ix).to(x.device), torch.from_numpy(iy).to(x.device)
    out = torch.empty((S, 4), dtype=torch.float64, device=x.device)
    status = torch.zeros((1,), dtype=torch.int32, device=x.device)
    _run('hoig_kid_poly_f64', x, (_p(x), x.shape[0], _p(y), y.shape[0], x.shape[1], _p(tix), _p(tiy), S, m, gamma, float(coef0),
                                  int(degree), _p(out), _p(status)), L.lib.hoig_kid_workspace_bytes(S, m) if x.is_cuda else None)
    return out, status


def kid_from_features(x, y, subsets=100, subset_size=1000, seed=0, degree=3, gamma=None, coef0=1.0):
    """(mean, std) of the per-subset unbiased MMD^2 between the feature sets x [nx, dims] and y [ny, dims] (fp32, on one device).
    gamma None: 1 / dims.  m = min(subset_size, nx, ny); the subsets are those of draw_subsets(nx, ny, subsets, m, seed).  The mean and
    the population standard deviation over the subsets are taken in fp64."""
    x, y = _features(x, 'x'), _features(y, 'y')
    m = min(int(subset_size), x.shape[0], y.shape[0])
    if m < 2:
        raise ValueError('KID needs subsets of at least 2 rows, got min(%d, %d, %d)' % (subset_size, x.shape[0], y.shape[0]))
    if subsets < 1:
        raise ValueError('subsets must be >= 1')
    ix, iy = draw_subsets(x.shape[0], y.shape[0], int(subsets), m, seed)
    out, status = kid_sums(x, y, ix, iy, degree, gamma, coef0)
    st = int(status.item())
    if st != 0:
        raise _status_error('KID', st)
    mmd = out[:, 3].cpu().numpy()
    if not np.isfinite(mmd).all():
        raise ValueError('KID: a non-finite value')
    return float(np.mean(mmd)), float(np.std(mmd))


# ------------------------------------------------------------------------------------------------ precision / recall / density
def _pivot(x, pivot):
    if pivot is None:
        return None
    if pivot.dtype != torch.float64 or tuple(pivot.shape) != (x.shape[1],) or pivot.device != x.device:
        raise ValueError('pivot: fp64 [%d] on %s expected' % (x.shape[1], x.device))
    return pivot.contiguous()


def knn_radii(x, k=3, pivot=None):
    """-> (radius [n] fp64: the k-th smallest SQUARED distance of every row of x to the other rows, status [1] int32); no sync."""
    x = _features(x, 'x')
    n = x.shape[0]
    if int(k) != k or not 1 <= k <= min(8, n - 1):
        raise ValueError('k %r: 1 .. min(8, n - 1) with n = %d' % (k, n))
    pivot = _pivot(x, pivot)
    radius = torch.empty((n,), dtype=torch.float64, device=x.device)
    status = torch.zeros((1,), dtype=torch.int32, device=x.device)
    _run('hoig_knn_radius_f64', x, (_p(x), n, x.shape[1], _p(pivot), int(k), _p(radius), _p(status)),
         L.lib.hoig_knn_workspace_bytes(n) if x.is_cuda else None)
    return radius, status


def manifold_hits(x, radius, y, pivot=None):
    """-> (hits [ny] int32: the number of rows i of x with d^2(x_i, y_j) <= radius[i], status [1] int32); no sync."""
    x, y = _features(x, 'x'), _features(y, 'y')
    if y.shape[1] != x.shape[1] or y.device != x.device:
        raise ValueError('x %s on %s and y %s on %s' % (tuple(x.shape), x.device, tuple(y.shape), y.device))
    if radius.dtype != torch.float64 or tuple(radius.shape) != (x.shape[0],) or radius.device != x.device:
        raise ValueError('radius: fp64 [%d] on %s expected' % (x.shape[0], x.device))
    pivot = _pivot(x, pivot)
    hits = torch.empty((y.shape[0],), dtype=torch.int32, device=x.device)
    status = torch.zeros((1,), dtype=torch.int32, device=x.device)
    _run('hoig_manifold_hits_f64', x, (_p(x), x.shape[0], _p(radius.contiguous()), _p(y), y.shape[0], x.shape[1], _p(pivot), _p(hits),
                                       _p(status)), L.lib.hoig_manifold_hits_workspace_bytes(x.shape[0], y.shape[0]) if x.is_cuda else None)
    return hits, status


def manifold_counts(real, fake, k=3):
    """-> (hits of the generated rows in the real set's balls, hits of the real rows in the generated set's balls), int32 numpy.
    The pivot of every distance is the column mean of `real`."""
    real, fake = _features(real, 'real'), _features(fake, 'fake')
    if real.shape[1] != fake.shape[1] or real.device != fake.device:
        raise ValueError('real %s on %s and fake %s on %s' % (tuple(real.shape), real.device, tuple(fake.shape), fake.device))
    pivot = real.double().mean(0)
    r_real, s1 = knn_radii(real, k, pivot)
    r_fake, s2 = knn_radii(fake, k, pivot)
    in_real, s3 = manifold_hits(real, r_real, fake, pivot)
    in_fake, s4 = manifold_hits(fake, r_fake, real, pivot)
    st = int(torch.stack([s1, s2, s3, s4]).max().item())
    if st != 0:
        raise _status_error('precision / recall', st)
    return in_real.cpu().numpy(), in_fake.cpu().numpy()


def precision_recall_from_features(real, fake, k=3):
    """{'precision', 'recall', 'density'} of the generated features `fake` against the real features `real` (fp32 [n, dims])."""
    in_real, in_fake = manifold_counts(real, fake, k)
    return {'precision': float(np.mean(in_real > 0)), 'recall': float(np.mean(in_fake > 0)),
            'density': float(in_real.astype(np.int64).sum()) / (float(k) * in_real.shape[0])}


# ------------------------------------------------------------------------------------------------ the features of a stream
class FeatureBank(object):
    """The fp32 feature rows of one image set, kept on `device`: append() takes [B, dims] blocks, rows() is one [N, dims] tensor.
    Unlike fid_device.Moments this grows with N: 4 * dims bytes per image, 400 MB per set at N = 50 000 and 2048 dims."""

    def __init__(self, dims, device=None):
        self.dims, self.device = int(dims), torch.device(device if device is not None else 'cuda')
        self.blocks, self.n = [], 0

    def append(self, feats):
        if feats.dtype != torch.float32 or feats.dim() != 2 or feats.shape[1] != self.dims or feats.device.type != self.device.type:
            raise ValueError('fp32 [B, %d] on %s expected, got %s %s on %s' % (self.dims, self.device, feats.dtype, tuple(feats.shape),
                                                                              feats.device))
        if feats.shape[0]:
            self.blocks.append(feats.detach().clone())            # (a copy: the network may reuse its output buffer)
            self.n += feats.shape[0]
        return self

    def copy(self):
        b = FeatureBank(self.dims, self.device)
        b.blocks, b.n = list(self.blocks), self.n
        return b

    def rows(self):
        if self.n == 0:
            raise ValueError('no images were given')
        return torch.cat(self.blocks)


def _options(value, name):
    """A kid= / prc= argument: None or False (off), True (the defaults) or a dict of keyword arguments."""
    if value is None or value is False:
        return None
    if value is True:
        return {}
    if isinstance(value, dict):
        return dict(value)
    raise ValueError('%s: True or a dict of keyword arguments, got %r' % (name, value))


# ------------------------------------------------------------------------------------------------ directories
def _path_features(paths, batch_size, device, dims, weights, precision, device_png_decode):
    """The fp32 features of two image directories, in get_activations' batches, on the network's device."""
    import os
    from . import images as I
    from .fid import InceptionFeatures
    for p in paths:
        if not os.path.exists(p):
            raise RuntimeError('Invalid path: %s' % p)
    model = InceptionFeatures(weights, dims, precision, device)
    out = []
    for p in paths:
        files = I.list_images(p)
        size = batch_size
        if size > len(files):
            print('Warning: batch size is bigger than the data size. Setting batch size to data size')
            size = len(files)
        bank = FeatureBank(dims, model.device)
        for u8 in I.DeviceBatches(I.batches_of(list(files), size), model.device, device_png_decode=device_png_decode):
            bank.append(model.features_u8(u8))
        out.append(bank.rows())
    return out


def calculate_kid_given_paths(paths, batch_size, device, dims, weights=None, precision=None, device_png_decode=None, **kid):
    """(mean, std) of the KID between two image directories: kid_from_features(features of paths[0], features of paths[1], **kid)."""
    x, y = _path_features(paths, batch_size, device, dims, weights, precision, device_png_decode)
    return kid_from_features(x, y, **kid)


def calculate_prc_given_paths(paths, batch_size, device, dims, weights=None, precision=None, device_png_decode=None, **prc):
    """{'precision', 'recall', 'density'} of the generated images in paths[0] against the real images in paths[1]."""
    fake, real = _path_features(paths, batch_size, device, dims, weights, precision, device_png_decode)
    return precision_recall_from_features(real, fake, **prc)
