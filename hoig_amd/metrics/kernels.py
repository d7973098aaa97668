"""Device side of the metrics: thin wrappers over the forward-only kernels of hoig_amd/csrc/metrics.hip and over hoig_conv2d_fwd.

Activations are fp32 NHWC CUDA tensors.  Nothing here records autograd state: the metric networks have no backward.
"""
import ctypes
import itertools

import torch

from .. import _lib as L
from .. import ops as O
from .._lib import ConvDesc

# Three-term 16-bit forward (HOIG_PREC_BF16X3: products to ~2^-21, fp32 accumulation) meets the metric tolerances of
# tests/test_metrics_gpu.py; 'f32' (exact fp32 products) is the parity mode.
DEFAULT_PRECISION = 'bf16x3'

# ImageNet normalisation of get_eval_loader (data/default_dataset.py) and LPIPS's own input scaling (metrics/lpips.py)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
LPIPS_MU, LPIPS_SIGMA = (-0.03, -0.088, -0.188), (0.458, 0.448, 0.450)

mac_counter = None   # [int]: when set, every Conv call adds its multiply-adds (tools/bench_metrics.py)


def precision_code(precision):
    name = precision or DEFAULT_PRECISION
    if name not in O._PREC or name == 'f16f6':
        raise ValueError('precision %r: one of %s' % (name, sorted(k for k in O._PREC if k != 'f16f6')))
    return O._PREC[name]


_owner_ids = itertools.count(1)


class _WeightOwner(object):
    """Gives the packed-weight cache of hoig_amd.ops a version of this network's own: weights are fixed after loading, so their
    16-bit planes are made once (and a later network whose weights reuse the same addresses does not see stale planes)."""

    def __init__(self):
        self.version = next(_owner_ids)

    def packed_planes(self, w, for_dgrad):
        return None


class Conv(object):
    """conv2d(x, w) + b, then ReLU, with (pad_h, pad_w) padding: a square padding goes to the kernel, an asymmetric one through
    hoig_pad2d first.  w: (Co, Ci, R, S) fp32 on the host."""

    def __init__(self, w, b, stride=1, pad=(0, 0), relu=True, device=None, owner=None):
        self.co, self.ci, self.r, self.s = w.shape
        self.w = O.pack_weight(w.float().to(device))
        self.b = b.float().to(device).contiguous()
        if owner is not None:
            self.w._hoig_owner = owner
        self.stride, self.pad = stride, tuple(pad)
        self.act = L.ACT_RELU if relu else L.ACT_NONE

    def __call__(self, x, prec):
        ph, pw = self.pad
        pad = ph
        if ph != pw:
            x, pad = pad2d(x, ph, pw), 0
        B, H, W, Ci = x.shape
        assert Ci == self.ci, (Ci, self.ci)
        Ho, Wo = (H + 2 * pad - self.r) // self.stride + 1, (W + 2 * pad - self.s) // self.stride + 1
        y = torch.empty((B, Ho, Wo, self.co), dtype=torch.float32, device=x.device)
        d = ConvDesc(B, H, W, Ci, Ho, Wo, self.co, self.r, self.s, self.stride, pad, 0, self.act, 0.0, prec)
        O._conv_fwd_raw(d, x, self.w, self.b, y)
        if mac_counter is not None:
            mac_counter[0] += B * Ho * Wo * self.co * Ci * self.r * self.s
        return y


def pool2d(x, k, stride, pad_h=0, pad_w=0, mode=L.POOL_MAX, count_include_pad=True):
    B, H, W, C = x.shape
    Ho, Wo = (H + 2 * pad_h - k) // stride + 1, (W + 2 * pad_w - k) // stride + 1
    y = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=x.device)
    L.call('hoig_pool2d_fwd', O._p(x), O._p(y), B, H, W, C, k, stride, pad_h, pad_w, mode, 1 if count_include_pad else 0, O._st())
    return y


def pad2d(x, pad_h, pad_w):
    B, H, W, C = x.shape
    y = torch.empty((B, H + 2 * pad_h, W + 2 * pad_w, C), dtype=torch.float32, device=x.device)
    L.call('hoig_pad2d', O._p(x), O._p(y), B, H, W, C, pad_h, pad_w, O._st())
    return y


def global_avgpool(x):
    B, H, W, C = x.shape
    y = torch.empty((B, C), dtype=torch.float32, device=x.device)
    L.call('hoig_global_avgpool', O._p(x), O._p(y), B, H * W, C, O._st())
    return y


def cat_channels(parts):
    """torch.cat(parts, channel axis) of NHWC tensors, one channel-slice copy per part."""
    C = sum(p.shape[-1] for p in parts)
    y = torch.empty(parts[0].shape[:-1] + (C,), dtype=torch.float32, device=parts[0].device)
    npix = y.numel() // C
    off = 0
    for p in parts:
        L.call('hoig_copy_channels', O._p(p), O._p(y), npix, p.shape[-1], 0, C, off, p.shape[-1], 0, O._st())
        off += p.shape[-1]
    return y


def stage_images_u8(u8, size=None, steps=()):
    """uint8 [B,H,W,C] on the device -> fp32 NHWC: /255 (ToTensor), bilinear resize to `size` (align_corners=False) when it differs,
    then each (sub, div) step of `steps` per channel, in order."""
    assert u8.dtype == torch.uint8 and u8.is_cuda and u8.is_contiguous() and u8.dim() == 4
    B, H, W, C = u8.shape
    Ho, Wo = size if size is not None else (H, W)
    flat = [v for sub, div in steps for v in (list(sub) + list(div))]
    aff = (ctypes.c_float * max(len(flat), 1))(*flat)
    y = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=u8.device)
    L.call('hoig_stage_images_u8', O._p(u8), O._p(y), B, H, W, C, Ho, Wo, len(steps), ctypes.cast(aff, ctypes.c_void_p), O._st())
    return y


_pil_tables = {}   # (in, out, device) -> int32 [out, 2 + ksize] on the device


def pil_table_host(n_in, n_out):
    """hoig_pil_bilinear_table: the taps of one axis of Pillow's 8-bit BILINEAR resize, int32 numpy [n_out, 2 + ksize] with rows
    [xmin, n, k[0..ksize)]."""
    import numpy as np
    ksize = L.lib.hoig_pil_bilinear_ksize(n_in, n_out)
    L.check(min(ksize, 0), 'hoig_pil_bilinear_ksize')
    table = np.zeros((n_out, 2 + ksize), np.int32)
    L.call('hoig_pil_bilinear_table', n_in, n_out, ctypes.c_void_p(table.ctypes.data))
    return table


def _pil_table(n_in, n_out, device):
    key = (n_in, n_out, torch.device(device))
    if key not in _pil_tables:
        _pil_tables[key] = torch.from_numpy(pil_table_host(n_in, n_out)).to(device)
    return _pil_tables[key]


def pil_resize_u8(u8, size):
    """uint8 [B,H,W,3] on the device -> uint8 [B,Ho,Wo,3], size = (Ho, Wo): PIL's Image.resize((Wo, Ho), Image.BILINEAR) of every
    image, equal in every byte.  One launch per axis that changes; the tap tables are made once per (in, out, device)."""
    assert u8.dtype == torch.uint8 and u8.is_cuda and u8.is_contiguous() and u8.dim() == 4
    B, H, W, C = u8.shape
    Ho, Wo = size
    nbytes = L.lib.hoig_resize_pil_bilinear_u8_workspace_bytes(B, H, W, C, Ho, Wo)
    L.check(min(nbytes, 0), 'hoig_resize_pil_bilinear_u8_workspace_bytes')
    y = torch.empty((B, Ho, Wo, C), dtype=torch.uint8, device=u8.device)
    tw = _pil_table(W, Wo, u8.device) if W != Wo else None
    th = _pil_table(H, Ho, u8.device) if H != Ho else None
    work = torch.empty(nbytes, dtype=torch.uint8, device=u8.device) if nbytes else None
    L.call('hoig_resize_pil_bilinear_u8', O._p(u8), B, H, W, C, O._p(y), Ho, Wo, *[O._p(t) if t is not None else None
                                                                                for t in (tw, th, work)], O._st())
    return y


def pil_resize_chain_u8(u8, img_size, side=299):
    """images.resize_chain for a device batch: PIL BILINEAR to img_size x img_size, then to side x side."""
    mid = u8 if tuple(u8.shape[1:3]) == (img_size, img_size) else pil_resize_u8(u8, (img_size, img_size))   # (a copy otherwise)
    return pil_resize_u8(mid, (side, side))


def nchw_to_nhwc(x):
    O._chk(x)
    return O.nchw_to_nhwc(x)
