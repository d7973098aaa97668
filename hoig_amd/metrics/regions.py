"""Scores on the hand and the object region of a frame (docs/region_metrics.md): masked PSNR / MAE from integer sums, and LPIPS, SSIM,
FID and KID on square crops around each region, taken from the ground truth's label map and resized as Pillow would.

A label map is uint8 [N,H,W]: 0 background, 1 hand, 2 object.  Every stage is a kernel of hoig_amd/csrc/region_metrics.hip; CUDA
tensors go to the kernels, CPU tensors to their host twins, which run the same inline code.  All of it is integers and bytes: the two
agree in every bit, and no value depends on how a stream is cut into update() calls.

Left out: soft masks (a label is one value per pixel), precision / recall and SWD per region, and a fid_reference for a region.
"""
import ctypes
import os

import numpy as np
import torch

from .. import _lib as L
from .._twin import ptr as _p, run as _run
from .feature_metrics import FeatureBank, _options, kid_from_features

NAMES = ('hand', 'object')
DEFAULTS = dict(size=128, min_pixels=64, batch=50)
SSIM_WINDOW = 11


def region_options(value):
    """A Scorer's regions= argument: None / False (off), True (the defaults) or a dict of size, min_pixels, batch."""
    opts = _options(value, 'regions')
    if opts is None:
        return None
    unknown = sorted(set(opts) - set(DEFAULTS))
    if unknown:
        raise ValueError('regions: unknown options %s (size, min_pixels, batch)' % unknown)
    opts = dict(DEFAULTS, **opts)
    if not 4 <= int(opts['size']) <= 512 or int(opts['min_pixels']) < 0 or int(opts['batch']) < 1:
        raise ValueError('regions: size in 4 .. 512, min_pixels >= 0, batch >= 1, got %r' % (opts,))
    return {k: int(v) for k, v in opts.items()}


def labels_from_masks(bg_mask, hand_mask):
    """uint8 labels of two masks of one shape: 1 where hand_mask < 0.5 (that mask is 1 OUTSIDE the hand), else 2 where bg_mask < 0.5,
    else 0."""
    is_hand = hand_mask < 0.5
    return (is_hand.to(torch.uint8) + (~is_hand & (bg_mask < 0.5)).to(torch.uint8) * 2).contiguous()


# ------------------------------------------------------------------------------------------------ the three stages
def _images(u8, name):
    if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[-1] != 3 or u8.shape[0] < 1:
        raise ValueError('%s: uint8 [N,H,W,3] expected, got %s %s' % (name, u8.dtype, tuple(u8.shape)))
    return u8.detach().contiguous()


def region_stats(gen_u8, gt_u8, labels_u8, regions=len(NAMES)):
    """-> (stats int64 [N, regions + 1, 8], status int32 [1]).  Row = [count, sum |d|, sum d^2, x0, y0, x1, y1, 0] of d = gen - gt over
    the three channels; row 0 every pixel, row r the pixels labelled r.  status: L.REGION_BAD_LABEL when a label above `regions` was
    read (the largest such label in bits 8 .. 15); that pixel counts in row 0 only."""
    gen_u8, gt_u8 = _images(gen_u8, 'generated'), _images(gt_u8, 'ground truth')
    N, H, W = gen_u8.shape[:3]
    if gt_u8.shape != gen_u8.shape or gt_u8.device != gen_u8.device:
        raise ValueError('generated %s and ground truth %s differ' % (tuple(gen_u8.shape), tuple(gt_u8.shape)))
    if labels_u8.dtype != torch.uint8 or tuple(labels_u8.shape) != (N, H, W) or labels_u8.device != gen_u8.device:
        raise ValueError('labels: uint8 [%d, %d, %d] on %s expected, got %s %s on %s' % (N, H, W, gen_u8.device, labels_u8.dtype,
                                                                                     tuple(labels_u8.shape), labels_u8.device))
    labels_u8 = labels_u8.detach().contiguous()
    stats = torch.empty((N, regions + 1, 8), dtype=torch.int64, device=gen_u8.device)
    status = torch.empty((1,), dtype=torch.int32, device=gen_u8.device)
    _run('hoig_region_stats_u8', gen_u8, (_p(gen_u8), _p(gt_u8), _p(labels_u8), N, H, W, regions, _p(stats), _p(status)))
    return stats, status


def region_boxes(stats, H, W, min_pixels=64):
    """-> int32 [N, regions, 4] = [left, top, side, valid] from region_stats' rows (the rule: docs/region_metrics.md)."""
    if stats.dtype != torch.int64 or stats.dim() != 3 or stats.shape[2] != 8 or stats.shape[1] < 2 or stats.shape[0] < 1:
        raise ValueError('stats: int64 [N, regions + 1, 8] expected, got %s %s' % (stats.dtype, tuple(stats.shape)))
    stats = stats.contiguous()
    N, R = stats.shape[0], stats.shape[1] - 1
    boxes = torch.empty((N, R, 4), dtype=torch.int32, device=stats.device)
    _run('hoig_region_boxes', stats, (_p(stats), N, int(H), int(W), R, int(min_pixels), _p(boxes)))
    return boxes


_tables = {}   # (max_side, size, device) -> int32 buffer on the device


def tables_host(max_side, size):
    """hoig_region_tables: the taps of every source side 1 .. max_side to `size` in one int32 numpy buffer."""
    nbytes = L.lib.hoig_region_tables_bytes(int(max_side), int(size))
    L.check(min(nbytes, 0), 'hoig_region_tables_bytes')
    out = np.zeros(nbytes // 4, np.int32)
    L.call('hoig_region_tables', int(max_side), int(size), ctypes.c_void_p(out.ctypes.data))
    return out


def _tables_on(max_side, size, device):
    key = (max_side, size, torch.device(device))
    if key not in _tables:
        _tables[key] = torch.from_numpy(tables_host(max_side, size)).to(device)
    return _tables[key]


def region_crops(u8, boxes, size=128):
    """-> uint8 [regions, N, size, size, 3]: Image.crop((left, top, left + side, top + side)).resize((size, size), Image.BILINEAR) of
    every box of `boxes` [N, regions, 4] in its image of u8 [N,H,W,3], equal in every byte; zeros for an invalid box."""
    u8 = _images(u8, 'images')
    N, H, W = u8.shape[:3]
    if boxes.dtype != torch.int32 or boxes.dim() != 3 or boxes.shape[0] != N or boxes.shape[2] != 4 or boxes.device != u8.device:
        raise ValueError('boxes: int32 [%d, regions, 4] on %s expected, got %s %s' % (N, u8.device, boxes.dtype, tuple(boxes.shape)))
    boxes = boxes.contiguous()
    R, size = boxes.shape[1], int(size)
    out = torch.empty((R, N, size, size, 3), dtype=torch.uint8, device=u8.device)
    if not u8.is_cuda:
        L.call('hoig_region_crop_resize_u8_host', _p(u8), N, H, W, _p(boxes), R, size, _p(out))
        return out
    nbytes = L.lib.hoig_region_crop_workspace_bytes(N, H, W, R, size)
    L.check(min(nbytes, 0), 'hoig_region_crop_workspace_bytes')
    work = torch.empty(nbytes, dtype=torch.uint8, device=u8.device)
    tables = _tables_on(min(H, W), size, u8.device)
    _run('hoig_region_crop_resize_u8', u8, (_p(u8), N, H, W, _p(boxes), R, size, _p(tables), _p(out), _p(work)))
    return out


# ------------------------------------------------------------------------------------------------ the scalar formulas
def psnr_mae(rows):
    """(psnr, mae) per row of int64 [M, 8] numpy: 10 log10(255^2 * 3 count / sum d^2) (inf where the sum is 0) and
    sum |d| / (3 count), in fp64."""
    cnt, ad, sq = (rows[:, i].astype(np.float64) for i in range(3))
    with np.errstate(divide='ignore'):
        psnr = 10.0 * np.log10(255.0 ** 2 * 3.0 * cnt / sq)
    return psnr, ad / (3.0 * cnt)


# ------------------------------------------------------------------------------------------------ a stream
class RegionScores(object):
    """The region half of a Scorer: update(gen_u8, gt_u8, labels_u8) runs stats -> boxes -> crops of both streams and sends every full
    batch of `batch` crops of a region to the networks it was given; nothing is copied to the host and nothing waits for the device
    before result().  fid: InceptionFeatures or None, lpips: LPIPS or None, ssim: bool, kid: None or kid_from_features' keyword
    arguments (needs fid), fid_device: the Frechet distance from fid_device.Moments on the device."""

    def __init__(self, options=True, fid=None, lpips=None, ssim=True, kid=None, fid_device=False, names=NAMES):
        self.opts = region_options(options if options is not None else True)
        self.names, self.fid, self.lpips, self.ssim, self.kid, self.fid_device = tuple(names), fid, lpips, bool(ssim), kid, bool(fid_device)
        if not 1 <= len(self.names) <= L.REGION_MAX:
            raise ValueError('1 .. %d region names expected' % L.REGION_MAX)
        if self.ssim and self.opts['size'] < SSIM_WINDOW:
            raise ValueError('regions: SSIM\'s %d-tap window needs crops of at least %d pixels, got size=%d'
                             % (SSIM_WINDOW, SSIM_WINDOW, self.opts['size']))
        if kid is not None and fid is None:
            raise ValueError('kid per region needs the FID network')
        R = len(self.names)
        self.n = 0
        self._stats, self._valid, self._status = [], [], None
        from .stream import _Batches            # (stream imports this module: the name is taken here, not at import time)
        self._queues = [(_Batches(self.opts['batch']), _Batches(self.opts['batch'])) for _ in range(R)]
        self._lpips = [[] for _ in range(R)]
        self._ssim = [[] for _ in range(R)]
        self._banks = None
        if fid is not None:
            self._banks = [(FeatureBank(fid.dims, fid.device), FeatureBank(fid.dims, fid.device)) for _ in range(R)]

    # ---- one batch of one region's crops
    def _batch(self, r, gen, gt, lpips_into, ssim_into, banks):
        from . import kernels as K
        from .ssim import ssim_nhwc
        if self.lpips is not None or self.ssim:
            pair = torch.cat([gen, gt]).contiguous()
            if self.lpips is not None:
                lpips_into.append(self.lpips.distance_u8(pair))
            if self.ssim:
                ssim_into.append(ssim_nhwc(K.stage_images_u8(pair, None, ()), data_range=1.0).mean(1))
        if self.fid is not None:
            banks[0].append(self.fid.features_u8(gen.contiguous()))
            banks[1].append(self.fid.features_u8(gt.contiguous()))

    def update(self, gen_u8, gt_u8, labels_u8):
        if gen_u8.shape[0] == 0:
            return
        R = len(self.names)
        H, W = gen_u8.shape[1:3]
        stats, status = region_stats(gen_u8, gt_u8, labels_u8, R)
        boxes = region_boxes(stats, H, W, self.opts['min_pixels'])
        crops = region_crops(gen_u8, boxes, self.opts['size']), region_crops(gt_u8, boxes, self.opts['size'])
        self._stats.append(stats)
        self._valid.append(boxes[:, :, 3].ne(0))
        self._status = status if self._status is None else torch.maximum(self._status, status)
        self.n += gen_u8.shape[0]
        for r in range(R):
            qg, qt = self._queues[r]
            for gen, gt in zip(qg.push(crops[0][r]), qt.push(crops[1][r])):
                self._batch(r, gen, gt, self._lpips[r], self._ssim[r], self._banks[r] if self._banks else None)

    # ---- the totals (the state is left as it is, so update() may go on)
    def _frechet(self, gen, gt):
        from .fid import calculate_frechet_distance
        if self.fid_device:
            from .fid_device import Moments, frechet_distance_device
            a, b = Moments(self.fid.dims, gen.device).update(gen), Moments(self.fid.dims, gt.device).update(gt)
            return frechet_distance_device(*(a.statistics() + b.statistics()))
        gen, gt = gen.double().cpu().numpy(), gt.double().cpu().numpy()
        return calculate_frechet_distance(np.mean(gen, axis=0), np.cov(gen, rowvar=False), np.mean(gt, axis=0), np.cov(gt, rowvar=False))

    def result(self):
        if self.n == 0:
            raise ValueError('no images were given')
        status = int(self._status.item())
        if status & L.REGION_BAD_LABEL:
            raise ValueError('regions: label %d in a label map of %d regions (0 background, %s)'
                             % (status >> 8 & 255, len(self.names), ', '.join('%d %s' % (i + 1, n) for i, n in enumerate(self.names))))
        stats = torch.cat(self._stats).cpu().numpy()
        valid_dev = torch.cat(self._valid)
        valid = valid_dev.cpu().numpy()
        out = {}
        psnr, mae = psnr_mae(stats[:, 0])
        out['psnr'], out['mae'] = float(np.mean(psnr)), float(np.mean(mae))
        for r, name in enumerate(self.names):
            keep = valid[:, r]
            count = int(keep.sum())
            if count == 0:
                raise ValueError('regions: no image has a valid %s region (at least %d pixels)' % (name, max(self.opts['min_pixels'], 1)))
            out['n_' + name] = count
            psnr, mae = psnr_mae(stats[keep, r + 1])
            out['psnr_' + name], out['mae_' + name] = float(np.mean(psnr)), float(np.mean(mae))
            lp, ss = list(self._lpips[r]), list(self._ssim[r])
            banks = tuple(b.copy() for b in self._banks[r]) if self._banks else None
            qg, qt = self._queues[r]
            if qg.rest is not None:
                self._batch(r, qg.rest, qt.rest, lp, ss, banks)
            if self.lpips is not None:
                out['lpips_' + name] = torch.cat(lp)[valid_dev[:, r]].double().mean().item()
            if self.ssim:
                out['ssim_' + name] = torch.cat(ss)[valid_dev[:, r]].double().mean().item()
            if self.fid is not None:
                if count < 2:
                    raise ValueError('regions: FID / KID of the %s region need at least 2 valid images, got %d' % (name, count))
                gen, gt = banks[0].rows()[valid_dev[:, r]].contiguous(), banks[1].rows()[valid_dev[:, r]].contiguous()
                out['fid_' + name] = self._frechet(gen, gt)
                if self.kid is not None:
                    out['kid_' + name], out['kid_std_' + name] = kid_from_features(gen, gt, **self.kid)
        return out


# ------------------------------------------------------------------------------------------------ directories
def _read_labels(files):
    from PIL import Image
    maps = []
    for f in files:
        with Image.open(f) as im:
            if im.mode not in ('L', 'P'):
                raise ValueError('%s: an 8-bit greyscale label map expected, got mode %s' % (f, im.mode))
            maps.append(np.asarray(im, dtype=np.uint8))
    return torch.from_numpy(np.stack(maps))


def calculate_region_metrics_given_paths(paths, labels_dir, size=128, min_pixels=64, batch_size=50, fid=None, lpips=None, ssim=True,
                                         kid=None, device=None, fid_device=False):
    """The region scores of the images in paths[0] (generated) against those in paths[1] (ground truth) with the label maps of
    `labels_dir` (8-bit greyscale files holding the label values), all three paired by sorted position: {'n', 'psnr', 'mae'} and per
    region 'n_<r>', 'psnr_<r>', 'mae_<r>' and, for what was given, 'lpips_<r>', 'ssim_<r>', 'fid_<r>', 'kid_<r>', 'kid_std_<r>' --
    the values of Scorer(regions=dict(size=size, min_pixels=min_pixels, batch=batch_size)) on the same images.  fid: an
    InceptionFeatures, lpips: an LPIPS (the caller builds them: weights.py), kid: True or kid_from_features' keyword arguments."""
    from . import images as I
    for p in list(paths) + [labels_dir]:
        if not os.path.exists(p):
            raise RuntimeError('Invalid path: %s' % p)
    files = [I.list_images(p) for p in list(paths) + [labels_dir]]
    if not files[0] or len({len(f) for f in files}) != 1:
        raise ValueError('%s, %s and %s hold %d, %d and %d images' % (paths[0], paths[1], labels_dir, len(files[0]), len(files[1]),
                                                                    len(files[2])))
    dev = torch.device(device if device is not None else 'cuda')
    scores = RegionScores(dict(size=size, min_pixels=min_pixels, batch=batch_size), fid, lpips, ssim, _options(kid, 'kid'), fid_device)
    groups = [I.batches_of(list(f), batch_size) for f in files]
    for gen, gt, names in zip(I.DeviceBatches(groups[0], dev), I.DeviceBatches(groups[1], dev), groups[2]):
        scores.update(gen, gt, _read_labels(names).to(dev))
    out = {'n': scores.n}
    out.update(scores.result())
    return out
