"""The Laplacian-pyramid sliced Wasserstein distance (SWD) of Karras et al. 2018 ("Progressive Growing of GANs",
sliced_wasserstein.py) between two sets of uint8 images, on the device (docs/swd.md).  It needs no trained network.

Per image and pyramid level `patches` 7 x 7 x 3 patches of the Laplacian level are taken at Philox-drawn positions; per set, level and
channel they are normalised to zero mean and unit deviation; both sets are projected on `repeats` x `dirs` random unit directions, every
direction's projections are sorted, and the level's value is 1000 times the mean |a_sorted - b_sorted|.  One value per level, finest
first, and their mean.

Every stage is a kernel of hoig_amd/csrc/swd.hip; CUDA tensors go to the kernels, CPU tensors to their host twins, which run the same
code in the same order and give the same bits.
"""
import os

import numpy as np
import torch

from .. import _lib as L
from .._twin import ptr as _p, run as _run
from .feature_metrics import _options  # noqa: F401  (the Scorer's swd= argument is read like kid= and prc=)

K = L.SWD_K
DEFAULTS = dict(patches=128, repeats=4, dirs=128, levels=None, seed=0)
SET_GEN, SET_REAL = 0, 1


# ------------------------------------------------------------------------------------------------ the pyramid and its patches
def pyramid_levels(H, W, levels=None):
    """floor(log2(min(H, W) / 16)) + 1, at most `levels`; ValueError below 16 or when H or W is not divisible by 2^(L-1)."""
    if min(H, W) < 16:
        raise ValueError('SWD needs images of at least 16 x 16, got %d x %d' % (H, W))
    n = L.lib.hoig_swd_levels(int(H), int(W))
    if levels is not None:
        if int(levels) != levels or levels < 1:
            raise ValueError('levels %r: an integer >= 1' % (levels,))
        n = min(n, int(levels))
    if H % (1 << (n - 1)) or W % (1 << (n - 1)):
        raise ValueError('SWD over %d levels needs H and W divisible by %d, got %d x %d' % (n, 1 << (n - 1), H, W))
    return n


def _images(u8):
    if not isinstance(u8, torch.Tensor):
        u8 = torch.from_numpy(np.ascontiguousarray(u8))
    if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[-1] != 3 or u8.shape[0] < 1:
        raise ValueError('uint8 [N,H,W,3] expected, got %s %s' % (u8.dtype, tuple(u8.shape)))
    return u8.detach().contiguous()


def patch_positions(n, H, W, levels=None, patches=128, seed=0, set_id=0, first_index=0, device='cpu'):
    """int32 [n, L, patches, 2] = (y0, x0) of every patch of images first_index .. first_index + n - 1 of set `set_id`
    (docs/swd.md has the counter layout)."""
    nl = pyramid_levels(H, W, levels)
    if n < 1 or patches < 1 or first_index < 0 or seed < 0:
        raise ValueError('n %d, patches %d, first_index %d, seed %d' % (n, patches, first_index, seed))
    pos = torch.empty((n, nl, patches, 2), dtype=torch.int32, device=device)
    _run('hoig_swd_positions', pos, (int(seed), int(set_id), int(first_index), n, H, W, nl, patches, _p(pos)))
    return pos


def laplacian_descriptors_u8(u8, levels=None, patches=128, seed=0, set_id=0, first_index=0, positions=None):
    """-> a list of L tensors fp32 [n * patches, 147], finest level first: the patches of the Laplacian pyramid of u8 [n,H,W,3].
    positions: int32 [n, L, patches, 2] to use in place of the drawn ones (a corner outside its level is a ValueError)."""
    u8 = _images(u8)
    n, H, W = u8.shape[0], u8.shape[1], u8.shape[2]
    nl = pyramid_levels(H, W, levels)
    if positions is None:
        pos = patch_positions(n, H, W, levels, patches, seed, set_id, first_index, u8.device)
    else:
        host = np.ascontiguousarray(positions.cpu().numpy() if isinstance(positions, torch.Tensor) else np.asarray(positions))
        if host.ndim != 4 or host.shape[0] != n or host.shape[1] != nl or host.shape[3] != 2 or host.dtype.kind not in 'iu':
            raise ValueError('positions: an integer [%d, %d, patches, 2] expected, got %s %s' % (n, nl, host.dtype, host.shape))
        patches = host.shape[2]
        for lv in range(nl):
            top = np.array([(H >> lv) - 7, (W >> lv) - 7])
            if (host[:, lv] < 0).any() or (host[:, lv] > top).any():
                raise ValueError('positions: a corner outside [0, %d] x [0, %d] at level %d' % (top[0], top[1], lv))
        pos = torch.from_numpy(host.astype(np.int32)).to(u8.device)
    out = torch.empty((nl, n * patches, K), dtype=torch.float32, device=u8.device)
    _run('hoig_swd_descriptors_u8', u8, (_p(u8), n, H, W, nl, patches, _p(pos), _p(out)),
         L.lib.hoig_swd_descriptors_workspace_bytes(n, H, W, nl) if u8.is_cuda else None)
    return [out[lv] for lv in range(nl)]


# ------------------------------------------------------------------------------------------------ the stages of a level
def _rows(x, name='rows'):
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != K or x.shape[0] < 1:
        raise ValueError('%s: fp32 [R, %d] expected, got %s %s' % (name, K, x.dtype, tuple(x.shape)))
    return x.detach().contiguous()


def channel_stats(rows):
    """-> (stats [3, 2] fp64 = {mean, population standard deviation} per channel, status [1] int32: bit c for a zero deviation)."""
    rows = _rows(rows)
    stats = torch.empty((3, 2), dtype=torch.float64, device=rows.device)
    status = torch.zeros((1,), dtype=torch.int32, device=rows.device)
    _run('hoig_swd_channel_stats_f64', rows, (_p(rows), rows.shape[0], _p(stats), _p(status)),
         L.lib.hoig_swd_channel_stats_workspace_bytes(rows.shape[0]) if rows.is_cuda else None)
    return stats, status


def directions(repeats=4, dirs=128, seed=0):
    """fp32 [repeats, 147, dirs] (numpy): np.random.default_rng(seed).standard_normal, every column scaled to unit length in float64."""
    if repeats < 1 or dirs < 1:
        raise ValueError('repeats %d, dirs %d' % (repeats, dirs))
    d = np.random.default_rng(seed).standard_normal((repeats, K, dirs))
    d /= np.sqrt(np.sum(np.square(d), axis=1, keepdims=True))
    return d.astype(np.float32)


def project(rows, stats, dirs):
    """-> fp32 [D, R], direction-major: the normalised rows [R, 147] times dirs [147, D]."""
    rows = _rows(rows)
    if stats.dtype != torch.float64 or tuple(stats.shape) != (3, 2) or stats.device != rows.device:
        raise ValueError('stats: fp64 [3, 2] on %s expected' % rows.device)
    if dirs.dtype != torch.float32 or dirs.dim() != 2 or dirs.shape[0] != K or dirs.shape[1] < 1 or dirs.device != rows.device:
        raise ValueError('dirs: fp32 [%d, D] on %s expected, got %s %s' % (K, rows.device, dirs.dtype, tuple(dirs.shape)))
    stats, dirs = stats.contiguous(), dirs.contiguous()
    out = torch.empty((dirs.shape[1], rows.shape[0]), dtype=torch.float32, device=rows.device)
    _run('hoig_swd_project_f32', rows, (_p(rows), rows.shape[0], _p(stats), _p(dirs), dirs.shape[1], _p(out)))
    return out


def sort_segments(keys):
    """Sorts every row of keys (fp32 [S, n], contiguous; any 4-byte aligned base) ascending, in place.  -> status [1] int32
    (L.SORT_NAN: a NaN key was read)."""
    if keys.dtype != torch.float32 or keys.dim() != 2 or not keys.is_contiguous() or keys.shape[0] < 1 or keys.shape[1] < 1:
        raise ValueError('keys: contiguous fp32 [S, n] expected, got %s %s' % (keys.dtype, tuple(keys.shape)))
    S, n = keys.shape
    status = torch.zeros((1,), dtype=torch.int32, device=keys.device)
    if not keys.is_cuda:
        L.call('hoig_sort_segments_f32_host', _p(keys), S, n, _p(status))
        return status
    nbytes = L.lib.hoig_sort_segments_workspace_bytes(S, n)
    if nbytes < 0:
        raise ValueError('sort_segments: no workspace for [%d, %d]' % (S, n))
    with torch.cuda.device(keys.device):
        _sort_call(keys, torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=keys.device), status)
    return status


def _sort_call(keys, ws, status):
    """sort_segments with a workspace the caller keeps (device only)."""
    L.call('hoig_sort_segments_f32', _p(keys), keys.shape[0], keys.shape[1], _p(ws), _p(status), torch.cuda.current_stream().cuda_stream)


def sorted_l1(a, b):
    """-> fp64 [1]: sum |a - b| over two fp32 tensors of one shape."""
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.shape != b.shape or a.device != b.device or a.numel() < 1:
        raise ValueError('two fp32 tensors of one shape on one device expected')
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty((1,), dtype=torch.float64, device=a.device)
    _run('hoig_swd_sorted_l1_f64', a, (_p(a), _p(b), a.numel(), _p(out)),
         L.lib.hoig_swd_sorted_l1_workspace_bytes(a.numel()) if a.is_cuda else None)
    return out


# ------------------------------------------------------------------------------------------------ the descriptors of a stream
class SWDBank(object):
    """The descriptors of one image set, kept on `device`: append() takes uint8 [B,H,W,3] images, rows(level) is one
    [N * patches, 147] tensor.  4 * 147 * patches * L bytes per image: 376 KB at 256 x 256 with the defaults.  The image index that
    goes into a patch's Philox counter is the running count, so the rows do not depend on how the images are split into calls."""

    def __init__(self, set_id, patches=128, levels=None, seed=0, device=None):
        self.set_id, self.patches, self.levels, self.seed = int(set_id), int(patches), levels, int(seed)
        self.device = torch.device(device if device is not None else 'cuda')
        self.blocks, self.n, self.size = [], 0, None

    def append(self, u8):
        u8 = _images(u8)
        if u8.device.type != self.device.type:
            raise ValueError('images on %s expected, got %s' % (self.device, u8.device))
        size = (u8.shape[1], u8.shape[2])
        if self.size is not None and size != self.size:
            raise ValueError('images of one set differ in size: %dx%d after %dx%d' % (size + self.size))
        self.blocks.append(laplacian_descriptors_u8(u8, self.levels, self.patches, self.seed, self.set_id, self.n))
        self.n, self.size = self.n + u8.shape[0], size
        return self

    def copy(self):
        b = SWDBank(self.set_id, self.patches, self.levels, self.seed, self.device)
        b.blocks, b.n, b.size = list(self.blocks), self.n, self.size
        return b

    def num_levels(self):
        if self.n == 0:
            raise ValueError('no images were given')
        return len(self.blocks[0])

    def rows(self, level):
        if self.n == 0:
            raise ValueError('no images were given')
        return torch.cat([blk[level] for blk in self.blocks])


def _stats_checked(bank, name, level):
    stats, status = channel_stats(bank.rows(level))
    st = int(status.item())
    if st:
        raise ValueError('SWD: the %s set has a constant channel %s at level %d: its deviation is zero' %
                         (name, ', '.join(str(c) for c in range(3) if st >> c & 1), level))
    return stats


def swd_from_banks(gen, real, repeats=4, dirs=128, seed=0):
    """{'swd', 'swd_levels', 'swd_sizes'} of two SWDBanks with the same number of images of one size.  One repeat at a time: the two
    projection buffers hold 2 * dirs * rows * 4 bytes."""
    if gen.n == 0 or real.n == 0:
        raise ValueError('no images were given')
    if gen.n != real.n or gen.size != real.size:
        raise ValueError('SWD needs two sets of as many images of one size: %d of %s and %d of %s' % (gen.n, gen.size, real.n, real.size))
    if gen.patches != real.patches or gen.num_levels() != real.num_levels():
        raise ValueError('the two banks differ in patches or levels')
    dev = gen.rows(0).device
    D = torch.from_numpy(directions(repeats, dirs, seed)).to(dev)
    values = []
    ws = sort_status = None
    for level in range(gen.num_levels()):
        a, b = gen.rows(level), real.rows(level)
        sa, sb = _stats_checked(gen, 'generated', level), _stats_checked(real, 'real', level)
        if a.is_cuda and ws is None:
            ws = torch.empty(L.lib.hoig_sort_segments_workspace_bytes(dirs, a.shape[0]) // 8 + 1, dtype=torch.float64, device=dev)
            sort_status = torch.zeros((1,), dtype=torch.int32, device=dev)
        sums = []
        for r in range(repeats):
            pa, pb = project(a, sa, D[r]), project(b, sb, D[r])
            for proj in (pa, pb):
                if proj.is_cuda:
                    with torch.cuda.device(dev):
                        _sort_call(proj, ws, sort_status)
                    st = sort_status
                else:
                    st = sort_segments(proj)
                if int(st.item()):
                    raise ValueError('SWD: a NaN projection at level %d' % level)
            sums.append(float(sorted_l1(pa, pb).item()) / float(pa.numel()))
        values.append(sum(sums) / float(repeats) * 1000.0)
    H, W = gen.size
    return {'swd': sum(values) / float(len(values)), 'swd_levels': values, 'swd_sizes': [(H >> lv, W >> lv) for lv in range(len(values))]}


def swd_options(value):
    """A Scorer's swd= argument: None / False (off), True (the defaults) or a dict of patches, repeats, dirs, levels, seed."""
    opts = _options(value, 'swd')
    if opts is None:
        return None
    unknown = sorted(set(opts) - set(DEFAULTS))
    if unknown:
        raise ValueError('swd: unknown options %s (patches, repeats, dirs, levels, seed)' % unknown)
    return dict(DEFAULTS, **opts)


def banks_for(opts, device):
    """(generated, real) SWDBanks of a set of options: set ids 0 and 1, so that the two sets draw their patches independently."""
    return tuple(SWDBank(s, opts['patches'], opts['levels'], opts['seed'], device) for s in (SET_GEN, SET_REAL))


def calculate_swd_given_paths(paths, batch_size, device, device_png_decode=None, **swd):
    """{'swd', 'swd_levels', 'swd_sizes'} of the images in paths[0] (generated) against those in paths[1] (real)."""
    from . import images as I
    opts = swd_options(swd or True)
    for p in paths:
        if not os.path.exists(p):
            raise RuntimeError('Invalid path: %s' % p)
    dev = torch.device(device if device is not None else 'cuda')
    banks = banks_for(opts, dev)
    for p, bank in zip(paths, banks):
        files = I.list_images(p)
        size = min(batch_size, len(files))
        if size == 0:
            raise ValueError('no images in %s' % p)
        for u8 in I.DeviceBatches(I.batches_of(list(files), size), dev, device_png_decode=device_png_decode):
            bank.append(u8)
    return swd_from_banks(banks[0], banks[1], opts['repeats'], opts['dirs'], opts['seed'])
