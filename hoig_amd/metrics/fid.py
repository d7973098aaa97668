"""FID on the HIP path: pytorch_fid's "FID Inception" network (metrics/pytorch_fid/inception.py) and fid_score.py's functions, with
the reference's names and signatures (weight arguments added at the end).

Convolutions run on hoig_conv2d_fwd with BatchNorm (eps 1e-3) folded into their weights and biases at load time, ReLU in the
epilogue; the default arithmetic is the three-term 16-bit forward (``precision='bf16x3'``, about fp32-accurate), ``precision='f32'``
gives exact fp32 products.  Statistics, the covariance and sqrtm stay on the host in fp64, as in the reference; ``device_stats=True``
(HOIG_DEVICE_FID=1, off by default) keeps them on the device instead (fid_device.py, docs/fid_device.md).
"""
import os

import numpy as np
import torch
from scipy import linalg

from .. import _lib as L
from . import images as I
from . import kernels as K
from .weights import INCEPTION_FILE, hub_path, resolve, take

IMAGE_EXTENSIONS = I.IMAGE_EXTENSIONS
BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}
BN_EPS = 1e-3


def _conv(name, ci, co, k, stride=1, pad=(0, 0)):
    k = (k, k) if isinstance(k, int) else k
    return (name, ci, co, k, stride, pad)


def _block_a(n, ci, pf):
    return [_conv(n + '.branch1x1', ci, 64, 1), _conv(n + '.branch5x5_1', ci, 48, 1), _conv(n + '.branch5x5_2', 48, 64, 5, 1, (2, 2)),
            _conv(n + '.branch3x3dbl_1', ci, 64, 1), _conv(n + '.branch3x3dbl_2', 64, 96, 3, 1, (1, 1)),
            _conv(n + '.branch3x3dbl_3', 96, 96, 3, 1, (1, 1)), _conv(n + '.branch_pool', ci, pf, 1)]


def _block_c(n, c7):
    return [_conv(n + '.branch1x1', 768, 192, 1), _conv(n + '.branch7x7_1', 768, c7, 1),
            _conv(n + '.branch7x7_2', c7, c7, (1, 7), 1, (0, 3)), _conv(n + '.branch7x7_3', c7, 192, (7, 1), 1, (3, 0)),
            _conv(n + '.branch7x7dbl_1', 768, c7, 1), _conv(n + '.branch7x7dbl_2', c7, c7, (7, 1), 1, (3, 0)),
            _conv(n + '.branch7x7dbl_3', c7, c7, (1, 7), 1, (0, 3)), _conv(n + '.branch7x7dbl_4', c7, c7, (7, 1), 1, (3, 0)),
            _conv(n + '.branch7x7dbl_5', c7, 192, (1, 7), 1, (0, 3)), _conv(n + '.branch_pool', 768, 192, 1)]


def _block_e(n, ci):
    return [_conv(n + '.branch1x1', ci, 320, 1), _conv(n + '.branch3x3_1', ci, 384, 1),
            _conv(n + '.branch3x3_2a', 384, 384, (1, 3), 1, (0, 1)), _conv(n + '.branch3x3_2b', 384, 384, (3, 1), 1, (1, 0)),
            _conv(n + '.branch3x3dbl_1', ci, 448, 1), _conv(n + '.branch3x3dbl_2', 448, 384, 3, 1, (1, 1)),
            _conv(n + '.branch3x3dbl_3a', 384, 384, (1, 3), 1, (0, 1)), _conv(n + '.branch3x3dbl_3b', 384, 384, (3, 1), 1, (1, 0)),
            _conv(n + '.branch_pool', ci, 192, 1)]


# the BasicConv2d layers of each output block: (name, Ci, Co, (R, S), stride, (pad_h, pad_w))
BLOCK_LAYERS = [
    [_conv('Conv2d_1a_3x3', 3, 32, 3, 2), _conv('Conv2d_2a_3x3', 32, 32, 3), _conv('Conv2d_2b_3x3', 32, 64, 3, 1, (1, 1))],
    [_conv('Conv2d_3b_1x1', 64, 80, 1), _conv('Conv2d_4a_3x3', 80, 192, 3)],
    _block_a('Mixed_5b', 192, 32) + _block_a('Mixed_5c', 256, 64) + _block_a('Mixed_5d', 288, 64)
    + [_conv('Mixed_6a.branch3x3', 288, 384, 3, 2), _conv('Mixed_6a.branch3x3dbl_1', 288, 64, 1),
       _conv('Mixed_6a.branch3x3dbl_2', 64, 96, 3, 1, (1, 1)), _conv('Mixed_6a.branch3x3dbl_3', 96, 96, 3, 2)]
    + _block_c('Mixed_6b', 128) + _block_c('Mixed_6c', 160) + _block_c('Mixed_6d', 160) + _block_c('Mixed_6e', 192),
    [_conv('Mixed_7a.branch3x3_1', 768, 192, 1), _conv('Mixed_7a.branch3x3_2', 192, 320, 3, 2),
     _conv('Mixed_7a.branch7x7x3_1', 768, 192, 1), _conv('Mixed_7a.branch7x7x3_2', 192, 192, (1, 7), 1, (0, 3)),
     _conv('Mixed_7a.branch7x7x3_3', 192, 192, (7, 1), 1, (3, 0)), _conv('Mixed_7a.branch7x7x3_4', 192, 192, 3, 2)]
    + _block_e('Mixed_7b', 1280) + _block_e('Mixed_7c', 2048),
]


def fold_bn(w, gamma, beta, mean, var, eps=BN_EPS):
    """conv (no bias) -> BatchNorm(eval) as one conv: (w * s, beta - mean * s) with s = gamma / sqrt(var + eps), in fp64."""
    s = gamma / torch.sqrt(var + eps)
    return w * s.view(-1, 1, 1, 1), beta - mean * s


def load_inception(weights, dims):
    """{layer name: (w, b)} (fp64, BN folded) of the layers up to the block `dims` selects."""
    sd, src = resolve(weights, [hub_path(INCEPTION_FILE)], 'FID Inception')
    out = {}
    for layers in BLOCK_LAYERS[:BLOCK_INDEX_BY_DIM[dims] + 1]:
        for name, ci, co, (r, s), _, _ in layers:
            w = take(sd, src, name + '.conv.weight', (co, ci, r, s))
            bn = [take(sd, src, '%s.bn.%s' % (name, k), (co,)) for k in ('weight', 'bias', 'running_mean', 'running_var')]
            out[name] = fold_bn(w, *bn)
    return out


class InceptionFeatures(object):
    """pytorch_fid's InceptionV3([BLOCK_INDEX_BY_DIM[dims]]) with the FID weights, up to that block, followed by the global
    average.  __call__(x) takes the staged images (fp32 NHWC on the device, [-1, 1], 299 x 299) and returns (B, dims) fp32."""

    def __init__(self, weights=None, dims=2048, precision=None, device=None):
        if dims not in BLOCK_INDEX_BY_DIM:
            raise ValueError('dims %r: one of %s' % (dims, sorted(BLOCK_INDEX_BY_DIM)))
        self.dims, self.prec = dims, K.precision_code(precision)
        self.device = torch.device(device if device is not None else 'cuda')
        owner = K._WeightOwner()
        self.c = {}
        folded = load_inception(weights, dims)
        for layers in BLOCK_LAYERS[:BLOCK_INDEX_BY_DIM[dims] + 1]:
            for name, _, _, _, stride, pad in layers:
                w, b = folded[name]
                self.c[name] = K.Conv(w, b, stride, pad, True, self.device, owner)

    def _f(self, name, x):
        return self.c[name](x, self.prec)

    def _a(self, n, x):
        f = lambda k, t: self._f(n + '.' + k, t)
        b5 = f('branch5x5_2', f('branch5x5_1', x))
        b3 = f('branch3x3dbl_3', f('branch3x3dbl_2', f('branch3x3dbl_1', x)))
        bp = f('branch_pool', K.pool2d(x, 3, 1, 1, 1, L.POOL_AVG, False))
        return K.cat_channels([f('branch1x1', x), b5, b3, bp])

    def _c(self, n, x):
        f = lambda k, t: self._f(n + '.' + k, t)
        b7 = f('branch7x7_3', f('branch7x7_2', f('branch7x7_1', x)))
        bd = x
        for i in range(1, 6):
            bd = f('branch7x7dbl_%d' % i, bd)
        bp = f('branch_pool', K.pool2d(x, 3, 1, 1, 1, L.POOL_AVG, False))
        return K.cat_channels([f('branch1x1', x), b7, bd, bp])

    def _e(self, n, x, pool_mode):
        f = lambda k, t: self._f(n + '.' + k, t)
        t = f('branch3x3_1', x)
        u = f('branch3x3dbl_2', f('branch3x3dbl_1', x))
        if pool_mode == L.POOL_AVG:
            p = K.pool2d(x, 3, 1, 1, 1, L.POOL_AVG, False)
        else:
            p = K.pool2d(x, 3, 1, 1, 1, L.POOL_MAX)
        return K.cat_channels([f('branch1x1', x), f('branch3x3_2a', t), f('branch3x3_2b', t), f('branch3x3dbl_3a', u),
                               f('branch3x3dbl_3b', u), f('branch_pool', p)])

    def blocks(self, x):
        """The feature map that ends the selected block (NHWC)."""
        f = self._f
        x = f('Conv2d_2b_3x3', f('Conv2d_2a_3x3', f('Conv2d_1a_3x3', x)))
        x = K.pool2d(x, 3, 2)
        if self.dims == 64:
            return x
        x = K.pool2d(f('Conv2d_4a_3x3', f('Conv2d_3b_1x1', x)), 3, 2)
        if self.dims == 192:
            return x
        for n in ('Mixed_5b', 'Mixed_5c', 'Mixed_5d'):
            x = self._a(n, x)
        bd = f('Mixed_6a.branch3x3dbl_3', f('Mixed_6a.branch3x3dbl_2', f('Mixed_6a.branch3x3dbl_1', x)))
        x = K.cat_channels([f('Mixed_6a.branch3x3', x), bd, K.pool2d(x, 3, 2)])
        for n in ('Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e'):
            x = self._c(n, x)
        if self.dims == 768:
            return x
        b3 = f('Mixed_7a.branch3x3_2', f('Mixed_7a.branch3x3_1', x))
        b7 = x
        for i in range(1, 5):
            b7 = f('Mixed_7a.branch7x7x3_%d' % i, b7)
        x = K.cat_channels([b3, b7, K.pool2d(x, 3, 2)])
        x = self._e('Mixed_7b', x, L.POOL_AVG)
        return self._e('Mixed_7c', x, L.POOL_MAX)

    def __call__(self, x):
        with torch.no_grad():
            return K.global_avgpool(self.blocks(x))

    def features_u8(self, u8):
        """uint8 [B,H,W,3] on the device -> (B, dims): ToTensor, bilinear to 299 (align_corners=False), 2x - 1 (inception.py)."""
        return self(K.stage_images_u8(u8, (299, 299), [((0.5,) * 3, (0.5,) * 3)]))


def _model(model, dims, device, weights, precision):
    if model is None or isinstance(model, int):
        return InceptionFeatures(weights, dims, precision, device)
    return model


def get_activations(files, model, batch_size=50, dims=2048, device=None, weights=None, precision=None, device_png_decode=None):
    """fid_score.py get_activations: (len(files), dims) fp64 activations, batch_size clipped to the number of files.
    device_png_decode (HOIG_DEVICE_PNG_DECODE=1): the supported PNG files are decoded on the device (images.DeviceBatches)."""
    model = _model(model, dims, device, weights, precision)
    if batch_size > len(files):
        print('Warning: batch size is bigger than the data size. Setting batch size to data size')
        batch_size = len(files)
    pred = np.empty((len(files), dims))
    start = 0
    for u8 in I.DeviceBatches(I.batches_of(list(files), batch_size), model.device, device_png_decode=device_png_decode):
        f = model.features_u8(u8).double().cpu().numpy()
        pred[start:start + f.shape[0]] = f
        start += f.shape[0]
    return pred


def calculate_activation_statistics(files, model, batch_size=50, dims=2048, device=None, weights=None, precision=None,
                                    device_png_decode=None, device_stats=None):
    """device_stats (HOIG_DEVICE_FID=1): the same batches go into streaming fp64 moments on the device (fid_device.Moments) and only
    mu and sigma come back; close to the default's values, not equal."""
    from .fid_device import Moments, fid_device_option
    if fid_device_option(device_stats):
        model = _model(model, dims, device, weights, precision)
        files = list(files)
        if batch_size > len(files):
            print('Warning: batch size is bigger than the data size. Setting batch size to data size')
            batch_size = len(files)
        moments = Moments(dims, model.device)
        for u8 in I.DeviceBatches(I.batches_of(files, batch_size), model.device, device_png_decode=device_png_decode):
            moments.update(model.features_u8(u8))
        return moments.statistics_host()
    act = get_activations(files, model, batch_size, dims, device, weights, precision, device_png_decode)
    return np.mean(act, axis=0), np.cov(act, rowvar=False)


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """||mu1 - mu2||^2 + Tr(S1 + S2 - 2 sqrtm(S1 S2)), scipy sqrtm; eps on the diagonals when the product is singular; a small
    imaginary part is dropped, a large one raises ValueError (fid_score.py)."""
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    assert mu1.shape == mu2.shape, 'Training and test mean vectors have different lengths'
    assert sigma1.shape == sigma2.shape, 'Training and test covariances have different dimensions'
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        print('fid calculation produces singular product; adding %s to diagonal of cov estimates' % eps)
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError('Imaginary component {}'.format(np.max(np.abs(covmean.imag))))
        covmean = covmean.real
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean)


def compute_statistics_of_path(path, model, batch_size, dims, device=None, weights=None, precision=None, device_png_decode=None,
                               device_stats=None):
    if str(path).endswith('.npz'):
        with np.load(path) as f:
            return f['mu'][:], f['sigma'][:]
    return calculate_activation_statistics(I.list_images(path), model, batch_size, dims, device, weights, precision, device_png_decode,
                                           device_stats)


def calculate_fid_given_paths(paths, batch_size, device, dims, weights=None, precision=None, device_png_decode=None, device_stats=None):
    """device_stats (HOIG_DEVICE_FID=1): moments and the distance on the device (fid_device.frechet_distance_device)."""
    from .fid_device import fid_device_option, frechet_distance_device
    device_stats = fid_device_option(device_stats)
    for p in paths:
        if not os.path.exists(p):
            raise RuntimeError('Invalid path: %s' % p)
    model = InceptionFeatures(weights, dims, precision, device)
    m1, s1 = compute_statistics_of_path(paths[0], model, batch_size, dims, device, device_png_decode=device_png_decode,
                                        device_stats=device_stats)
    m2, s2 = compute_statistics_of_path(paths[1], model, batch_size, dims, device, device_png_decode=device_png_decode,
                                        device_stats=device_stats)
    if device_stats:
        return frechet_distance_device(m1, s1, m2, s2, model.device)
    return calculate_frechet_distance(m1, s1, m2, s2)
