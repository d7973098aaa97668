"""tests/conv_f6_reference.py held by itself: the e2m3 quantiser exhaustively, split32 and the record layout on hand-made blocks, the
emulation inside a window that a degenerate emulator misses, and the TEETH condition -- each switch of DEFECTS moves the emulated output
by at least 4 x TOL_F6, so the bound of tests/test_conv_f6_gpu.py sees a kernel broken that way (docs/conv_f6_parity.md)."""
import pytest
import torch

import conv_f6_reference as F6
import conv_reference as R

GAUSSIAN = [r.id for r in F6.ROWS if r.gaussian]
# the rows whose GPU bound is TOL_F6 as it stands (tanh and sigmoid rows add the activation's own tolerance)
TEETH_ROWS = [rid for rid in GAUSSIAN if F6.ROW[rid].act not in ('tanh', 'sigmoid')]


# ---------------------------------------------------------------------------------------------------- the quantiser
def test_e2m3_codes_decode_and_encode_to_themselves():
    codes = torch.arange(64, dtype=torch.uint8)
    v = F6.e2m3_decode(codes)
    pos = v[:32]
    assert pos[0] == 0 and pos[31] == 7.5 and (pos[1:] > pos[:-1]).all()
    steps = pos[1:] - pos[:-1]
    assert (steps[pos[1:] <= 2] == 0.125).all() and (steps[(pos[1:] > 2) & (pos[1:] <= 4)] == 0.25).all()
    assert (steps[pos[1:] > 4] == 0.5).all()
    assert torch.equal(v[32:], -pos) and torch.signbit(v[32]), 'code 0x20 is -0.0'
    assert torch.equal(F6.e2m3_encode(v), codes)


def test_e2m3_midpoints_round_to_the_even_code_and_the_neighbourhood_to_the_nearer():
    pos = F6.E2M3_POS
    mid = (pos[:-1] + pos[1:]) / 2
    lower = torch.arange(31)
    even = torch.where(lower % 2 == 0, lower, lower + 1)
    assert torch.equal(F6.e2m3_encode(mid).long(), even)
    assert torch.equal(F6.e2m3_encode(-mid).long(), even + 32)
    eps = 2.0 ** -30
    assert torch.equal(F6.e2m3_encode(mid - eps).long(), lower) and torch.equal(F6.e2m3_encode(mid + eps).long(), lower + 1)


def test_e2m3_saturates_and_keeps_the_sign_of_zero():
    """7.75 is the midpoint of 7.5 (odd mantissa) and the 8.0 the format does not have: it rounds away, to saturation, like everything
    above.  +-0: the sign bit of the code is the sign bit of the value, also where the magnitude rounds to zero -- -0.0 and every value
    in [-0.0625, -0) encode as 0x20, which decodes to -0.0 and multiplies like +0.  The device's conversion does the same (measured:
    no record of tests/test_conv_f6_gpu.py differs, docs/conv_f6_parity.md), so that test compares the codes as they are and allows
    no +-0 difference; records_differ(..., allow_signed_zero=True) exists to tell such a difference from a real one should it appear."""
    big = torch.tensor([7.5, 7.625, 7.75, 8.0, 100.0, 65504.0, float('inf')], dtype=torch.float64)
    assert (F6.e2m3_encode(big) == 31).all() and (F6.e2m3_encode(-big) == 63).all()
    assert F6.e2m3_encode(torch.tensor([7.25 - 2.0 ** -30])).item() == 30
    z = F6.e2m3_encode(torch.tensor([0.0, -0.0, 0.0625, -0.0625, -0.01, 0.0625 + 2.0 ** -30], dtype=torch.float64))
    assert z.tolist() == [0, 32, 0, 32, 32, 1]


# ---------------------------------------------------------------------------------------------------- split32 and the records
def test_split32_scales_on_hand_made_blocks():
    t = torch.zeros(4, 32)
    t[0, 3] = 5.0                     # amax 5 = 1.25 * 2^2: e = 2, eh = 0, el = -11
    t[0, 4] = 1.0 + 2.0 ** -12        # hi = 1, lo = 2^-12 = 0.5 * 2^-11: lo code 0.5 -> 0b000100
    t[1, 0] = -(2.0 ** -30)           # e = -30: eh = -32, el = -43; fp16(x) and fp16(x - -0) underflow to -0: both codes 0x20
    t[3, 7] = 2.0 ** -140             # an fp32 subnormal: exponent field 0 -> e = -127, eh clamps to -100, el to -111
    s = F6.split32(t, 1.0)
    assert s.scale_hi[:, 0].tolist() == [127, 127 - 32, 127 - 22, 27] and s.scale_lo[:, 0].tolist() == [116, 127 - 43, 127 - 33, 16]
    assert s.code_hi[0, 3].item() == 0b011010 and s.code_hi[0, 4].item() == 0b001000 and s.code_lo[0, 4].item() == 0b000100
    assert s.q_hi[0, 3].item() == 5.0 and s.q_lo[0, 4].item() == 2.0 ** -12
    assert s.code_hi[1, 0].item() == 0x20 and s.code_lo[1, 0].item() == 0x20 and s.code_hi[1, 1:].sum().item() == 0
    assert s.code_hi[2].sum().item() == 0 and s.code_lo[2].sum().item() == 0          # the all-zero block: scale 2^-22 from e = -20
    # pre = 256: the scale follows the scaled value
    assert F6.split32(t, 256.0).scale_hi[0, 0].item() == 127 + 8


def test_split32_takes_the_block_maximum_from_the_fp32_values():
    """4 - 2^-12 is below 4 in fp32 (e = 1, scale 2^-1) and rounds to 4.0 in fp16: hi / scale = 8, which saturates at 7.5.  A split that
    took the maximum from the fp16 values would pick e = 2 and represent 4.0 exactly."""
    t = torch.zeros(1, 32)
    t[0, 0] = 4.0 - 2.0 ** -12
    s = F6.split32(t, 1.0)
    assert s.hi[0, 0].item() == 4.0 and s.scale_hi[0, 0].item() == 126 and s.code_hi[0, 0].item() == 31 and s.q_hi[0, 0].item() == 3.75


def test_split32_dequantised_values_are_within_half_a_step():
    g = torch.Generator().manual_seed(3)
    t = torch.randn(50, 64, generator=g) * torch.exp(torch.randn(50, 64, generator=g))
    s = F6.split32(t, 1.0)
    sh = torch.pow(2.0, s.scale_hi.double() - 127).repeat_interleave(32, -1)
    sl = torch.pow(2.0, s.scale_lo.double() - 127).repeat_interleave(32, -1)
    saturated = (s.code_hi & 31) == 31
    assert ((s.hi - s.q_hi).abs() <= torch.where(saturated, 0.5, 0.25) * sh).all()    # half of the largest step, 0.5; 8.0 -> 7.5 loses 0.5
    assert ((s.lo - s.q_lo).abs() <= 0.125 * sl).all() and (s.lo.abs() <= 4.0 * sl).all()      # |lo| <= 2^(e-11) = 4 scales: steps <= 0.25


def test_weight_records_layout():
    """Record (tap * (Ci / 64) + cb64, co): block 0 in bytes 0..23, block 1 in 24..47, element j in bits [6j, 6j + 6) little-endian,
    scale bytes at 48 / 49, pads zero; decoding the bytes again gives split32's codes."""
    Co, Ci = 3, 128
    w = torch.zeros(Co, Ci, 3, 3)
    w[2, 64 + 32 + 5, 1, 2] = 1.5 / 256                       # co 2, tap 5, cb64 1, block 1, element 5: 256 w = 1.5 -> e = 0, eh = -2: 6.0
    qh, ql = F6.weight_records(w)
    assert qh.shape == ql.shape == (9 * 2, Co, F6.REC) and qh.dtype == torch.uint8
    rec = qh[5 * 2 + 1, 2]
    assert rec[48].item() == 127 - 22 and rec[49].item() == 127 - 2 and rec[50:].sum().item() == 0
    bits = int.from_bytes(bytes(rec[24:48].tolist()), 'little')
    assert bits == 0b011100 << (6 * 5) and rec[:24].sum().item() == 0
    other = qh.clone()
    other[5 * 2 + 1, 2] = 0
    assert other[..., :48].sum().item() == 0
    # random weights: the bytes decode to split32's codes and scales, in the layout's order
    g = torch.Generator().manual_seed(9)
    w = torch.randn(Co, Ci, 3, 3, generator=g) * 0.05
    s = F6.split32(w.permute(0, 2, 3, 1).reshape(Co, 9, Ci), 256.0)
    for rec, codes, scale in zip(F6.weight_records(w), (s.code_hi, s.code_lo), (s.scale_hi, s.scale_lo)):
        got = F6.unpack6(rec[..., :48].reshape(9, 2, Co, 2, 24))                       # [tap][cb64][co][half][32]
        assert torch.equal(got.permute(2, 0, 1, 3, 4).reshape(Co, 9, Ci), codes)
        assert torch.equal(rec[..., 48:50].reshape(9, 2, Co, 2).permute(2, 0, 1, 3).reshape(Co, 9, 4), scale)
    assert F6.records_differ(*F6.weight_records(w)) > 0 and F6.records_differ(qh, qh) == 0
    flipped = qh.clone()
    flipped[0, 0, 0] = 0x20                                    # element 0 of an all-zero block: -0 instead of +0
    assert F6.records_differ(flipped, qh) == 1 and F6.records_differ(flipped, qh, allow_signed_zero=True) == 0


# ---------------------------------------------------------------------------------------------------- the emulation
@pytest.mark.parametrize('rid', GAUSSIAN)
def test_emulation_sits_between_three_exact_terms_and_two(rid):
    """conv_f6_ref against float64: above the rounding error of three exact fp16 terms (pure float64, or cross terms kept exact, would
    sit at or below it) and below the error of two terms (no cross term lo(w): an emulator without its cross terms would sit there)."""
    r, o = F6.ROW[rid], F6.operands(rid)
    case = (o['x'], o['w'], None, None, 1, 1, False)
    e3 = R.rounded_operand_error(case, 'bf16x3', passes=('y',))['y']
    e2 = R.rounded_operand_error(case, 'f16x2', passes=('y',))['y']
    x, w = o['x'], o['w']
    e6 = F6.rel_err64(F6.conv_f6_ref(x, w), R.conv_ref(x, w, None, 1, 1))
    print('%s: three terms %.2e < fp16 + fp6 %.2e < two terms %.2e' % (rid, e3, e6, e2))
    assert 0.0 < e3 < e6 < e2, (e3, e6, e2)
    assert 10 * e3 < e6 and 2 * e6 < e2, 'the window has no room: %r' % ((e3, e6, e2),)


def test_every_defect_moves_a_gaussian_row_by_four_tolerances():
    """The teeth of tests/test_conv_f6_gpu.py: a kernel with one of DEFECTS differs from the intact emulation by the margin printed
    here on the row named, and the test's bound is TOL_F6 -- at most a quarter of the smallest margin.  (Measured, per defect the best
    row: docs/conv_f6_parity.md.)"""
    best = {}
    for d in F6.DEFECTS:
        per_row = {rid: F6.rel_err64(F6.emulated(rid, d), F6.emulated(rid)) for rid in TEETH_ROWS}
        rid = max(per_row, key=per_row.get)
        best[d] = (per_row[rid], rid)
        print('%-26s %.2e on %-16s (%.1f x TOL_F6); smallest %.2e' % (d, per_row[rid], rid, per_row[rid] / F6.TOL_F6, min(per_row.values())))
    for d, (margin, rid) in best.items():
        assert margin >= 4.0 * F6.TOL_F6, (d, margin, rid)
    assert F6.TOL_F6 <= 0.25 * min(m for m, _ in best.values())


def test_tolerance_is_below_every_rows_own_quantisation_error():
    """TOL_F6 < emulation-vs-float64 on every row: a kernel inside TOL_F6 of the emulation is told apart from float64."""
    for r in F6.ROWS:
        e = F6.rel_err64(F6.emulated(r.id), F6.truth(r.id))
        assert F6.TOL_F6 < e, (r.id, e)


def test_normalised_input_keeps_the_frame_zero_and_relus_by_channel():
    o = F6.operands('normin_relu_c1')
    g = F6.gathered_input(o['x'][..., :32], o['x'][..., 32:], o['in_scale'], o['in_shift'], 32)
    want = torch.addcmul(o['in_shift'].double().reshape(2, 1, 1, -1), o['x'].double(), o['in_scale'].double().reshape(2, 1, 1, -1))
    assert torch.equal(g[..., :32], want[..., :32].float()) and (g[..., :32] < 0).any()            # scaled and shifted, no ReLU below c0
    assert torch.equal(g[..., 32:], want[..., 32:].clamp_min(0).float()) and (g[..., 32:] == 0).any()
    assert not torch.equal(o['in_scale'][0], o['in_scale'][1]) and (o['in_scale'][:, :32] != 1).all()      # per image, also on x1's channels
    # shifts of order 1: a frame that were normalised instead of left zero would move the border by order 1e-1
    y = F6.emulated('normin_relu0')
    o = F6.operands('normin_relu0')
    padded = torch.nn.functional.pad(o['x'], (0, 0, 1, 1, 1, 1))
    wrong = F6.conv_f6_ref(F6.gathered_input(padded, None, o['in_scale'], o['in_shift'], 0), o['w'])[:, 1:-1, 1:-1]
    assert F6.rel_err64(wrong, y) > 1e-1 and torch.equal(wrong[:, 1:-1, 1:-1], y[:, 1:-1, 1:-1])
