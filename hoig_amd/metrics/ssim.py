"""SSIM and MS-SSIM on the HIP path, with pytorch_msssim 0.2.1's semantics (the package metrics/ssim.py calls).

Each level is one fused hoig_ssim launch (separable Gaussian window, the five filtered moments, the ssim and cs maps and their
per-(image, channel) means); MS-SSIM's downsampling is hoig_pool2d_fwd (average 2 x 2, padding (H % 2, W % 2), padded zeros
counted).  Only the (levels, N, C) means reach the combination on the host side of the stream.
"""
import torch

from .. import _lib as L
from .. import ops as O
from . import images as I
from . import kernels as KR

MS_WEIGHTS = [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]


def _level(xy, data_range, win_size, win_sigma, K_):
    """xy: [2N, H, W, C] (X then Y) -> ssim, cs: (N, C) fp32."""
    B2, H, W, C = xy.shape
    n = B2 // 2
    s = torch.empty((n, C), dtype=torch.float32, device=xy.device)
    cs = torch.empty_like(s)
    nbytes = L.lib.hoig_ssim_workspace_bytes(n, H, W, C, win_size)
    if nbytes < 0:
        raise ValueError('image %dx%d is smaller than the %d-tap window' % (H, W, win_size))
    work = torch.zeros(nbytes, dtype=torch.uint8, device=xy.device)
    L.call('hoig_ssim', O._p(xy), O._p(xy[n:]), O._p(s), O._p(cs), n, H, W, C, float(data_range), float(K_[0]), float(K_[1]), win_size,
           float(win_sigma), O._p(work), O._st())
    return s, cs


def _check(X, Y, win_size):
    if X.dim() != 4:
        raise ValueError('Input images should be 4-d tensors.')
    if X.type() != Y.type():
        raise ValueError('Input images should have the same dtype.')
    if X.shape != Y.shape:
        raise ValueError('Input images should have the same shape.')
    if win_size % 2 != 1:
        raise ValueError('Window size should be odd.')


def _nhwc_pair(X, Y):
    return KR.nchw_to_nhwc(torch.cat([X, Y]).float())


def ssim_nhwc(xy, data_range=255, win_size=11, win_sigma=1.5, K=(0.01, 0.03), nonnegative_ssim=False):
    """Per-(image, channel) SSIM (N, C) of xy = [X | Y] in NHWC."""
    s, _ = _level(xy, data_range, win_size, win_sigma, K)
    return torch.relu(s) if nonnegative_ssim else s


def ms_ssim_nhwc(xy, data_range=255, win_size=11, win_sigma=1.5, weights=None, K=(0.01, 0.03)):
    """Per-(image, channel) MS-SSIM (N, C) of xy = [X | Y] in NHWC."""
    smaller = min(xy.shape[1:3])
    assert smaller > (win_size - 1) * 2 ** 4, \
        'Image size should be larger than %d due to the 4 downsamplings in ms-ssim' % ((win_size - 1) * 2 ** 4)
    w = torch.tensor(weights if weights is not None else MS_WEIGHTS, dtype=torch.float32, device=xy.device)
    mcs = []
    for i in range(w.shape[0]):
        s, cs = _level(xy, data_range, win_size, win_sigma, K)
        if i < w.shape[0] - 1:
            mcs.append(torch.relu(cs))
            H, W = xy.shape[1:3]
            xy = _pool2x2(xy, H % 2, W % 2)
    vals = torch.stack(mcs + [torch.relu(s)], dim=0)
    return torch.prod(vals ** w.view(-1, 1, 1), dim=0)


def _pool2x2(xy, ph, pw):
    return KR.pool2d(xy, 2, 2, ph, pw, L.POOL_AVG, True)


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, K=(0.01, 0.03), nonnegative_ssim=False):
    """pytorch_msssim.ssim on (N, C, H, W) tensors: the mean over channels per image (N,), or over everything (size_average)."""
    _check(X, Y, win_size)
    with torch.no_grad():
        v = ssim_nhwc(_nhwc_pair(X, Y), data_range, win_size, win_sigma, K, nonnegative_ssim)
    return v.mean() if size_average else v.mean(1)


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, K=(0.01, 0.03), weights=None):
    """pytorch_msssim.ms_ssim on (N, C, H, W) tensors: relu(cs) of the first four levels, relu(ssim) of the last, the product of
    the levels raised to `weights`, then the mean over channels (N,) or over everything (size_average)."""
    _check(X, Y, win_size)
    with torch.no_grad():
        v = ms_ssim_nhwc(_nhwc_pair(X, Y), data_range, win_size, win_sigma, weights, K)
    return v.mean() if size_average else v.mean(1)


def ssim_pairs_u8(u8):
    """Per-image (SSIM, MS-SSIM), each (N,), of uint8 [2N, 299, 299, 3] (X then Y, already through the resize chain) with
    calculate_ssim_given_paths' inputs: ToTensor, ImageNet Normalize, data_range=255."""
    xy = KR.stage_images_u8(u8, None, [(KR.IMAGENET_MEAN, KR.IMAGENET_STD)])
    return ssim_nhwc(xy, 255).mean(1), ms_ssim_nhwc(xy, 255).mean(1)


def calculate_ssim_given_paths(paths, img_size=256, batch_size=1, device=None, device_resize=False, device_png_decode=None):
    """(SSIM, MS-SSIM) means over two directories of images paired by sorted position, with the reference's inputs exactly
    (metrics/ssim.py): get_eval_loader's transform (PIL resize to img_size, then to 299 x 299, ImageNet Normalize) and
    data_range=255 on those normalised tensors.  Their range is about 5, not 255, so C1 and C2 dominate and both values sit close to
    1: that is the reference's setting, reproduced, not corrected.  device_resize: the workers only decode and the two PIL resizes run
    on the device (kernels.pil_resize_chain_u8: the same bytes, so the same values).  device_png_decode (HOIG_DEVICE_PNG_DECODE=1): the
    supported PNG files are decoded on the device too (images.DeviceBatches); it implies device_resize."""
    from .lpips import paired_batches
    device_png_decode = I.png_decode_option(device_png_decode)
    device_resize = device_resize or device_png_decode
    print('Calculating SSIM given paths %s and %s...' % (paths[0], paths[1]))
    dev = torch.device(device if device is not None else 'cuda')
    s_all, m_all = [], []
    for u8 in I.DeviceBatches(paired_batches(paths, batch_size), dev, None if device_resize else img_size,
                              device_png_decode=device_png_decode):
        s, m = ssim_pairs_u8(KR.pil_resize_chain_u8(u8, img_size) if device_resize else u8)
        s_all.append(s)
        m_all.append(m)
    return torch.cat(s_all).double().mean().item(), torch.cat(m_all).double().mean().item()
