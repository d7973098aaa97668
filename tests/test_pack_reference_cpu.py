"""tests/pack_reference.py itself, without a GPU (docs/optimizer_parity.md)."""
import numpy as np
import pytest
import torch

import pack_reference as P


@pytest.mark.parametrize('Co,RS,Ci', P.SHAPES)
@pytest.mark.parametrize('for_dgrad', [False, True])
def test_plane_index_is_a_bijection(Co, RS, Ci, for_dgrad):
    n, k, K = P.rows_and_columns(Co, RS, Ci, for_dgrad)
    N = Ci if for_dgrad else Co
    assert K == RS * (Co if for_dgrad else Ci) and n.max() == N - 1 and k.max() == K - 1
    idx = P.plane_index(n, k, K)
    assert idx.min() == 0 and idx.max() == N * K - 1 and len(np.unique(idx)) == N * K
    # a 32 x 32 block stays a block, a row of a block a row, an 8-element group a group
    assert np.array_equal(idx // 1024, (n // 32) * (K // 32) + k // 32)
    assert np.array_equal(idx % 1024 // 32, n % 32) and np.array_equal(idx % 8, k % 8)


def test_plane_index_swizzles_the_groups_of_a_row():
    assert P.plane_index(0, 0, 64) == 0 and P.plane_index(0, 9, 64) == 9
    assert P.plane_index(4, 0, 64) == 4 * 32 + 8 and P.plane_index(4, 8, 64) == 4 * 32          # rows 4..7: groups 0 <-> 1
    assert P.plane_index(13, 31, 64) == 13 * 32 + (3 ^ 3) * 8 + 7                                # rows 12..15: XOR 3
    assert P.plane_index(16, 8, 64) == 16 * 32 + 8                                               # (n / 4) % 4 wraps at 16
    assert P.plane_index(33, 40, 64) == (1 * 2 + 1) * 1024 + 32 + 8


def test_bf16_rounding_is_torch_bfloat16():
    rng = np.random.RandomState(1)
    x = np.concatenate([P.planted(), (rng.standard_normal(4096) * 10.0 ** rng.uniform(-12, 2, 4096)).astype(np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(P.bf16_rne(x), want)
    tie_even = np.array([0x3D4C8000, 0x3D4D8000, 0x3D4C7FFF, 0x3D4C8001], dtype=np.uint32).view(np.float32)
    assert P.bf16_rne(tie_even).tolist() == [0x3D4C, 0x3D4E, 0x3D4C, 0x3D4D]


def test_the_splits_on_the_planted_values():
    w = P.planted()
    hi, lo = P.split_bf16(w)
    back = P.bf16_value(hi).astype(np.float64) + P.bf16_value(lo).astype(np.float64)
    assert np.all(np.abs(back - w) <= 2.0 ** -16 * np.abs(w))            # two 8-bit mantissas
    h, l = P.split_fp16(w)
    xs = w.astype(np.float64) * 256
    back = h.view(np.float16).astype(np.float64) + l.view(np.float16).astype(np.float64)
    assert np.all(np.abs(back - xs) <= 2.0 ** -21 * np.abs(xs) + 2.0 ** -25)      # two 11-bit mantissas; half the smallest subnormal
    # halfway between fp16 neighbours goes to the even one; 2^-33 * 256 ties to 0, anything above it to the smallest subnormal
    assert P.split_fp16(np.float32(2.0 ** -33))[0] == 0 and P.split_fp16(np.float32(2.0 ** -33 * (1 + 2.0 ** -20)))[0] == 1
    mid = np.float32((np.float32(np.float16(1.0)) + np.float32(np.nextafter(np.float16(1.0), np.float16(2.0)))) / 2) / np.float32(256)
    assert P.split_fp16(mid)[0] == np.float16(1.0).view(np.uint16)
    assert P.split_fp16(np.float32(-0.0))[0] == 0x8000 and P.split_bf16(np.float32(-0.0)) == (0x8000, 0)


def test_planes_put_every_element_where_the_layout_says():
    w, at = P.weight((64, 9, 32), 3)
    for for_dgrad in (False, True):
        hi, lo = P.planes(w, for_dgrad)
        h, l = (P.split_bf16 if for_dgrad else P.split_fp16)(w.ravel())
        for co, rs, ci in ((0, 0, 0), (5, 2, 9), (63, 8, 31), (37, 4, 16)):
            n, k, K = (ci, rs * 64 + co, 9 * 64) if for_dgrad else (co, rs * 32 + ci, 9 * 32)
            i = (co * 9 + rs) * 32 + ci
            assert hi[P.plane_index(n, k, K)] == h[i] and lo[P.plane_index(n, k, K)] == l[i]
