"""What a 16-bit operand plane of a convolution weight must contain (pack_weight_kernel, pack_all_kernel and the plane-writing half of
adam_pack_kernel in hoig_amd/csrc/weight_planes.hip; docs/optimizer_parity.md), in numpy, written from the layout's description and
importing none of the project's code.

A weight is stored [Co][RS][Ci], fp32.  A plane has N rows of K reduction indices:
  forward planes        n = co, k = rs * Ci + ci, K = RS * Ci;   hi = fp16(256 w), lo = fp16(256 w - hi)   (round to nearest even, with
                                                                 gradual underflow, as numpy's float16 rounds)
  data-gradient planes  n = ci, k = rs * Co + co, K = RS * Co;   hi = bf16(w),     lo = bf16(w - hi)       (round to nearest even)
Element (n, k) lives at plane_index(n, k, K): 32 x 32 blocks of 1024 elements, block (n / 32, k / 32) at ((n / 32)(K / 32) + k / 32) * 1024;
inside a block row n % 32 holds its four 8-element groups at position ((k % 32) / 8) XOR ((n / 4) % 4).
"""
import numpy as np

SENTINEL = 0x5A5A
SHAPES = [(32, 1, 32), (64, 9, 32), (32, 9, 64), (64, 16, 96), (96, 25, 160), (160, 49, 64), (128, 25, 192)]      # (Co, RS, Ci)


def plane_index(n, k, K):
    n, k = np.asarray(n, dtype=np.int64), np.asarray(k, dtype=np.int64)
    block = (n // 32) * (K // 32) + k // 32
    group = ((k % 32) // 8) ^ ((n // 4) % 4)
    return block * 1024 + (n % 32) * 32 + group * 8 + k % 8


def bf16_rne(x):
    """float32 (finite) -> the bits of the nearest bfloat16, ties to the even mantissa: the upper half of the word, plus one when the
    lower half is above 0x8000, or is 0x8000 and the upper half is odd."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    upper, lower = u >> 16, u & 0xFFFF
    up = (lower > 0x8000) | ((lower == 0x8000) & ((upper & 1) == 1))
    return (upper + up).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, dtype=np.uint32) << 16).view(np.float32)


def split_bf16(w):
    """-> (hi, lo) bits: hi = bf16(w), lo = bf16(w - hi); the difference is taken in fp32 (it is exact there)."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    hi = bf16_rne(w)
    return hi, bf16_rne(w - bf16_value(hi))


def split_fp16(w):
    """-> (hi, lo) bits: hi = fp16(256 w), lo = fp16(256 w - hi), the product and the difference in fp32 (both exact)."""
    xs = np.ascontiguousarray(w, dtype=np.float32) * np.float32(256.0)
    with np.errstate(under='ignore'):
        hi = xs.astype(np.float16)
        lo = (xs - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def rows_and_columns(Co, RS, Ci, for_dgrad):
    """(n, k, K) of every element of a [Co][RS][Ci] weight, in storage order."""
    co, rs, ci = np.meshgrid(np.arange(Co), np.arange(RS), np.arange(Ci), indexing='ij')
    if for_dgrad:
        return ci.ravel(), (rs * Co + co).ravel(), RS * Co
    return co.ravel(), (rs * Ci + ci).ravel(), RS * Ci


def planes(w, for_dgrad):
    """w: float32 [Co][RS][Ci] -> (hi plane, lo plane), uint16 [Co * RS * Ci]."""
    Co, RS, Ci = w.shape
    n, k, K = rows_and_columns(Co, RS, Ci, for_dgrad)
    idx = plane_index(n, k, K)
    h, l = split_bf16(w.ravel()) if for_dgrad else split_fp16(w.ravel())
    hi, lo = np.empty(w.size, dtype=np.uint16), np.empty(w.size, dtype=np.uint16)
    hi[idx], lo[idx] = h, l
    return hi, lo


def planted():
    """The values a split can get wrong, float32:
      - words whose lower half is 0x7FFF, 0x8000, 0x8001 under an even and an odd upper half (bf16 ties and near-ties), both signs,
        at three magnitudes
      - 256 w exactly halfway between two fp16 neighbours, below an even and an odd fp16 mantissa, normal and subnormal
      - +0 and -0
      - |w| in (2^-33, 2^-22): 256 w is an fp16 subnormal or rounds to 0 (2^-33: the tie between 0 and the smallest subnormal)
      - magnitudes up to 200 (256 w stays inside fp16's range)"""
    out = []
    for upper in (0x3D4C, 0x3D4D, 0x3F80, 0x3F81, 0x3A02, 0x3A03, 0x4300, 0x42FF):
        for lower in (0x7FFF, 0x8000, 0x8001):
            for sign in (0, 0x80000000):
                out.append(np.array([(upper << 16) | lower | sign], dtype=np.uint32).view(np.float32)[0])
    for hb in (0x3554, 0x3555, 0x4A00, 0x4A01, 0x2C00, 0x2FFF, 0x0012, 0x0013, 0x03FF, 0x0400, 0x0000):
        a, b = (np.array([hb, hb + 1], dtype=np.uint16).view(np.float16)).astype(np.float32)
        mid = np.float32((a + b) / np.float32(2.0))
        for sign in (1.0, -1.0):
            out.append(np.float32(sign * mid / np.float32(256.0)))
    out += [np.float32(0.0), np.float32(-0.0)]
    for e in np.linspace(-33.0, -22.0, 45)[1:-1]:
        out += [np.float32(2.0 ** e), np.float32(-(2.0 ** e) * 1.37)]
    out += [np.float32(2.0 ** -33 * (1 + 2.0 ** -20)), np.float32(2.0 ** -32), np.float32(1.5 * 2.0 ** -32), np.float32(-2.5 * 2.0 ** -32)]
    out += [np.float32(x) for x in (200.0, -200.0, 199.99, -157.3, 100.3, -64.0, 31.999, 255.0 / 256.0 * 200)]
    out = np.array(out, dtype=np.float32)
    assert np.isfinite(out).all() and np.abs(out).max() <= 200.0
    return out


def weight(shape, seed):
    """randn * 0.05 with the planted values at seeded places -> (w [Co][RS][Ci] float32, the planted places in the flattened weight)."""
    rng = np.random.RandomState(seed)
    w = (rng.standard_normal(shape) * 0.05).astype(np.float32)
    pl = planted()
    at = rng.choice(w.size, len(pl), replace=False)
    w.ravel()[at] = pl
    return w, at
