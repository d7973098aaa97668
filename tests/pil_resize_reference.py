"""numpy restatement of Pillow's 8-bit ``Image.resize(size, Image.BILINEAR)`` (TEST INFRASTRUCTURE for hoig_amd/csrc/pil_resize.h).

A fixed-point, separable convolution: per axis the taps are computed in double, normalised, rounded to 22 fractional bits; the
horizontal pass runs first and is rounded to bytes, the vertical pass reads that; a pass that keeps its size is skipped.
tests/test_pil_resize_cpu.py pins THIS to Pillow in every byte, so that "equal to the restatement" means "equal to Pillow" for the
tables, which Pillow does not expose.
"""
import math

import numpy as np
from PIL import Image

PRECISION_BITS = 22

# (H, W) -> (Ho, Wo)
CASES = [((256, 256), (299, 299)),      # the metric shape
         ((64, 64), (299, 299)),
         ((300, 300), (256, 256)),
         ((37, 53), (299, 299)),
         ((512, 384), (256, 256)),
         ((299, 299), (64, 80)),
         ((5, 7), (3, 2)),              # taps clipped at both edges
         ((1, 1), (4, 4)),
         ((256, 200), (256, 299)),      # horizontal pass only
         ((200, 256), (299, 256)),      # vertical pass only
         ((256, 256), (256, 256))]      # copy
CHAIN = ((200, 180), 256, 299)          # (H, W) -> img_size -> side, as images.resize_chain


def axis_pairs():
    """Every (in, out) of one axis that CASES and CHAIN resample."""
    pairs = set()
    for (h, w), (ho, wo) in CASES:
        pairs |= {(h, ho), (w, wo)}
    (h, w), a, b = CHAIN
    pairs |= {(h, a), (w, a), (a, b)}
    return sorted(p for p in pairs if p[0] != p[1])


def ksize(n_in, n_out):
    return 2 * int(math.ceil(max(n_in / n_out, 1.0))) + 1


def coefficients(n_in, n_out):
    """-> xmin [n_out], n [n_out], k [n_out, ksize] (int32; unused taps zero)."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support, ss = fs, 1.0 / fs
    xmin, cnt, k = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32), np.zeros((n_out, ksize(n_in, n_out)), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)          # int(): truncation towards zero, as C's (int)
        hi = min(int(center + support + 0.5), n_in)
        w = np.array([max(0.0, 1.0 - abs((x + lo - center + 0.5) * ss)) for x in range(hi - lo)], np.float64)
        total = 0.0
        for v in w:                                        # summed in tap order
            total += v
        w = w / total
        xmin[xx], cnt[xx] = lo, hi - lo
        k[xx, :hi - lo] = [int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
    return xmin, cnt, k


def resample_axis(a, n_out, axis):
    """One pass of `a` (uint8) along `axis`."""
    n_in = a.shape[axis]
    xmin, cnt, k = coefficients(n_in, n_out)
    src = np.moveaxis(a, axis, 0).astype(np.int32)
    out = np.empty((n_out,) + src.shape[1:], np.int32)
    for xx in range(n_out):
        taps = k[xx, :cnt[xx]].reshape((-1,) + (1,) * (src.ndim - 1))
        out[xx] = ((1 << (PRECISION_BITS - 1)) + (src[xmin[xx]:xmin[xx] + cnt[xx]] * taps).sum(0, dtype=np.int32)) >> PRECISION_BITS
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


def resize(a, size):
    """a: uint8 [..., H, W, C]; size = (Ho, Wo)."""
    ho, wo = size
    if a.shape[-2] != wo:
        a = resample_axis(a, wo, a.ndim - 2)
    if a.shape[-3] != ho:
        a = resample_axis(a, ho, a.ndim - 3)
    return np.ascontiguousarray(a)


def pillow(a, size):
    """Pillow itself on each image of a: uint8 [B, H, W, 3]."""
    return np.stack([np.asarray(Image.fromarray(im).resize((size[1], size[0]), Image.BILINEAR)) for im in a])


def content(b, h, w, seed, binary=False):
    rng = np.random.RandomState(seed)
    if binary:
        return (rng.randint(0, 2, size=(b, h, w, 3)) * 255).astype(np.uint8)
    return rng.randint(0, 256, size=(b, h, w, 3)).astype(np.uint8)
