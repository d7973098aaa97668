"""float64 CPU emulation of the fp16 + fp6 forward arithmetic of hoig_amd/csrc/conv_f6.hip (HOIG_PREC_F16F6), written from that file
(split32, pack_f6_kernel, its header comment) -- the yardstick of tests/test_conv_f6_gpu.py, itself held by
tests/test_conv_f6_reference_cpu.py (docs/conv_f6_parity.md).

A product a * w is computed as  hi(a) * hi(w') + q(lo(a)) * q(hi(w')) + q(hi(a)) * q(lo(w')),  w' = 256 w, a = hi + lo and w' = hi + lo the
fp16 split, q() the block-scaled e2m3 quantiser: one E8M0 scale per 32 channels, taken from the exponent of the block's largest |fp32
value|, elements rounded to nearest even and saturating at 7.5.  Every product and sum below is exact in float64 (16-bit factors, at
most 9 * Ci terms); what a kernel adds to this is its fp32 accumulation order alone.

Layouts as in tests/conv_reference.py: activations NHWC, weights logical (Co, Ci, 3, 3) over any strides, results float64."""
import collections
import functools

import numpy as np
import torch

import conv_reference as R

# Bound of kernel-minus-emulation in rel_err64: fp32 accumulation over 9 * Ci products in MFMA order.  MEASURED, not derived
# (docs/conv_f6_parity.md): 4 x the largest error of the three-term kernel against three_term_ref() over the rows below.
TOL_F6 = 4e-6

REC = 56                    # bytes of a weight record: 24 B block 0 | 24 B block 1 | scale bytes at 48, 49 | 6 pad bytes (never written)
REC_USED = 50
W_SCALE = 256.0

# ---- e2m3: 1 sign bit, 2 exponent bits (bias 1), 3 mantissa bits; code = sign << 5 | exponent << 3 | mantissa
E2M3_POS = torch.tensor([m * 0.125 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 1) for e in range(4) for m in range(8)], dtype=torch.float64)
_MID = (E2M3_POS[:-1] + E2M3_POS[1:]) / 2


def e2m3_decode(codes):
    """uint8 codes (6 bits) -> float64 values; code 0x20 is -0.0."""
    c = torch.as_tensor(codes).to(torch.int64)
    v = E2M3_POS[c & 31]
    return torch.where((c & 32) != 0, -v, v)


def e2m3_encode(v):
    """float64 values -> uint8 codes: round to nearest, ties to the even mantissa, saturating at +-7.5.  The sign bit is the value's own
    sign bit, also where the magnitude rounds to zero and for -0.0 (so -0.0 and every value in [-0.0625, -0] encode as 0x20, which decodes
    to -0.0: the product it enters is the same zero)."""
    v = torch.as_tensor(v, dtype=torch.float64)
    a = v.abs()
    idx = torch.searchsorted(_MID, a.contiguous(), right=False)          # number of midpoints strictly below |v|
    tie = (idx < 31) & (a == _MID[idx.clamp(max=30)])
    idx = idx + (tie & (idx % 2 == 1)).to(idx.dtype)                      # a tie goes to the even code of (idx, idx + 1)
    return (idx + 32 * torch.signbit(v).to(idx.dtype)).to(torch.uint8)


Split = collections.namedtuple('Split', 'hi code_hi code_lo scale_hi scale_lo q_hi q_lo lo')


def split32(t, pre=1.0):
    """split32 of conv_f6.hip over the last axis of fp32 tensor `t`, in blocks of 32 (the axis must be a multiple of 32).
    -> Split: hi = fp16(x) as float64, x = fp32(t * pre); code_hi / code_lo the e2m3 codes (uint8, t's shape) of hi / 2^eh and of
    lo / 2^el, lo = fp16(x - hi); scale_hi / scale_lo the E8M0 bytes eh + 127 / el + 127 (uint8, one per block: shape[:-1] + (n / 32,));
    q_hi / q_lo the dequantised values code * 2^eh / code * 2^el (float64); lo itself (float64, IEEE: fp16 subnormals kept)."""
    assert t.dtype == torch.float32 and t.shape[-1] % 32 == 0
    x = (t * torch.tensor(pre, dtype=torch.float32)).contiguous()
    hi16 = x.to(torch.float16)
    lo16 = (x - hi16.float()).to(torch.float16)
    blk = x.reshape(x.shape[:-1] + (x.shape[-1] // 32, 32))
    amax = blk.abs().amax(-1)                                              # over the fp32 values, not the fp16 ones
    e = ((amax.view(torch.int32) >> 23) & 0xFF) - 127
    e = torch.where(amax > 0, e, torch.full_like(e, -20))
    eh = (e - 2).clamp(-100, 100)
    el = (eh - 11).clamp(min=-120)
    sh, sl = torch.pow(2.0, eh.double()).unsqueeze(-1), torch.pow(2.0, el.double()).unsqueeze(-1)
    hi, lo = hi16.double(), lo16.double()
    ch = e2m3_encode(hi.reshape(blk.shape) / sh)
    cl = e2m3_encode(lo.reshape(blk.shape) / sl)
    qh = (e2m3_decode(ch) * sh).reshape(x.shape)
    ql = (e2m3_decode(cl) * sl).reshape(x.shape)
    return Split(hi, ch.reshape(x.shape), cl.reshape(x.shape), (eh + 127).to(torch.uint8), (el + 127).to(torch.uint8), qh, ql, lo)


def _pack6(codes):
    """(..., 32) uint8 codes -> (..., 24) bytes: element j in bits [6j, 6j + 6), little-endian."""
    bits = np.unpackbits(codes.numpy()[..., None], axis=-1, bitorder='little')[..., :6]
    return torch.from_numpy(np.packbits(bits.reshape(bits.shape[:-2] + (192,)), axis=-1, bitorder='little'))


def unpack6(frag):
    """The inverse of the packing: (..., 24) bytes -> (..., 32) codes."""
    bits = np.unpackbits(torch.as_tensor(frag).numpy(), axis=-1, bitorder='little')
    bits = bits.reshape(bits.shape[:-1] + (32, 6))
    return torch.from_numpy(np.packbits(np.concatenate([bits, np.zeros_like(bits[..., :2])], -1), axis=-1, bitorder='little')[..., 0])


def weight_records(w):
    """-> (q_hi, q_lo): the two byte arrays hoig_pack_conv_weight_f6 makes of conv weight `w` (Co, Ci, R, S), Ci % 64 == 0, each
    uint8 [R * S * Ci / 64][Co][56]: record (tap * (Ci / 64) + cb64, co) holds 32-channel block 2 cb64 in bytes 0..23, block 2 cb64 + 1 in
    bytes 24..47, their scale bytes at 48 and 49; the six pad bytes are zero here and never compared."""
    Co, Ci, Rr, S = w.shape
    assert Ci % 64 == 0
    s = split32(w.detach().cpu().float().permute(0, 2, 3, 1).reshape(Co, Rr * S, Ci), W_SCALE)
    out = []
    for codes, scale in ((s.code_hi, s.scale_hi), (s.code_lo, s.scale_lo)):
        frag = _pack6(codes.reshape(Co, Rr * S, Ci // 64, 2, 32))           # [co][tap][cb64][half][24]
        rec = torch.zeros(Rr * S, Ci // 64, Co, REC, dtype=torch.uint8)
        rec[..., :48] = frag.permute(1, 2, 0, 3, 4).reshape(Rr * S, Ci // 64, Co, 48)
        rec[..., 48:50] = scale.reshape(Co, Rr * S, Ci // 64, 2).permute(1, 2, 0, 3)
        out.append(rec.reshape(Rr * S * (Ci // 64), Co, REC))
    return out[0], out[1]


def records_differ(got, want, allow_signed_zero=False):
    """Number of records whose codes or scale bytes differ (pad bytes ignored).  allow_signed_zero: codes 0x00 and 0x20 count as equal."""
    got = torch.as_tensor(got).cpu().reshape(-1, REC)
    want = torch.as_tensor(want).cpu().reshape(-1, REC)
    assert got.shape == want.shape
    if not allow_signed_zero:
        return int((got[:, :REC_USED] != want[:, :REC_USED]).any(1).sum())
    cg, cw = unpack6(got[:, :48].reshape(-1, 2, 24)), unpack6(want[:, :48].reshape(-1, 2, 24))
    cg, cw = torch.where(cg == 32, torch.zeros_like(cg), cg), torch.where(cw == 32, torch.zeros_like(cw), cw)
    return int(((cg != cw).reshape(got.shape[0], -1).any(1) | (got[:, 48:50] != want[:, 48:50]).any(1)).sum())


# ---- switches that break the emulation in the ways a kernel could be broken; tests/test_conv_f6_reference_cpu.py proves with them that
# the bound of tests/test_conv_f6_gpu.py would notice (nothing else uses them)
DEFECT_TAP = (1, 2)         # the tap (r, s) the two tap defects drop
DEFECT_BLOCK = (0, 4, 0)    # (output channel, tap index r * 3 + s, 32-channel block) of the scale defect
DEFECTS = (
    'hi_lo_tap_dropped',            # one tap of q(hi(a)) * q(lo(w)) missing
    'lo_hi_tap_dropped',            # one tap of q(lo(a)) * q(hi(w)) missing
    'weight_scale_off_by_one',      # the E8M0 byte of one 32-channel block of the weight's hi records one too large
    'weight_records_swapped',       # the hi and the lo record array of the weight exchanged
)


def gathered_input(x, x2=None, in_scale=None, in_shift=None, in_relu_c0=0):
    """The fp32 tensor the halo loader splits: [x | x2] along channels; with in_scale / in_shift (B, Cg) fp32(fma(x, scale, shift)) per
    (image, channel), ReLU on channels >= in_relu_c0.  (The fma is taken as the float64 sum of the exact product, rounded to fp32: a
    double rounding, which differs from the fused one on about one value in 2^29.)"""
    g = x if x2 is None else torch.cat([x, x2], -1)
    g = g.detach().cpu().float()
    if in_scale is not None:
        B, Cg = g.shape[0], g.shape[-1]
        v = g.double() * in_scale.detach().cpu().double().reshape(B, 1, 1, Cg) + in_shift.detach().cpu().double().reshape(B, 1, 1, Cg)
        g = v.float()
        g[..., in_relu_c0:] = g[..., in_relu_c0:].clamp_min(0.0)
    return g


def conv_f6_ref(x, w, bias=None, act='none', slope=0.2, x2=None, in_scale=None, in_shift=None, in_relu_c0=0, defect=None):
    """-> y (NHWC float64) = act((sum hi_a hi_w + sum q(lo_a) q(hi_w) + sum q(hi_a) q(lo_w)) / 256 + bias) of the 3x3 stride-1 pad-1
    convolution; the zero frame is padding of the gathered (normalised) tensor and stays zero.  defect: one of DEFECTS, or None."""
    assert defect is None or defect in DEFECTS
    a = split32(gathered_input(x, x2, in_scale, in_shift, in_relu_c0), 1.0)
    Co, Ci = w.shape[0], w.shape[1]
    ws = split32(w.detach().cpu().float().permute(0, 2, 3, 1).contiguous(), W_SCALE)           # [Co][R][S][Ci]
    logical = lambda t: t.permute(0, 3, 1, 2)
    w_hh, w_qh, w_ql = logical(ws.hi), logical(ws.q_hi).clone(), logical(ws.q_lo).clone()
    if defect == 'weight_records_swapped':
        w_qh, w_ql = w_ql, w_qh
    elif defect == 'weight_scale_off_by_one':
        co, tap, kb = DEFECT_BLOCK
        w_qh[co, kb * 32:kb * 32 + 32, tap // 3, tap % 3] *= 2.0
    elif defect == 'hi_lo_tap_dropped':
        w_ql[:, :, DEFECT_TAP[0], DEFECT_TAP[1]] = 0.0
    elif defect == 'lo_hi_tap_dropped':
        w_qh[:, :, DEFECT_TAP[0], DEFECT_TAP[1]] = 0.0
    y = R.conv_ref(a.hi, w_hh, None, 1, 1) + R.conv_ref(a.q_lo, w_qh, None, 1, 1) + R.conv_ref(a.q_hi, w_ql, None, 1, 1)
    y = y / W_SCALE
    if bias is not None:
        y = y + bias.detach().cpu().double().reshape(1, 1, 1, -1)
    return R.ACTS[act](y, slope)


def three_term_ref(x, w, bias=None, act='none', slope=0.2):
    """The same layer on three fp16 terms with exact accumulation (HOIG_PREC_BF16X3's forward: both operands hi + lo, lo * lo dropped;
    conv_reference._terms) -- what the three-term kernel is held against when TOL_F6 is measured."""
    (xh, xl), (wh, wl) = R._terms(x.detach().cpu(), 2, torch.float16), R._terms(w.detach().cpu(), 2, torch.float16, W_SCALE)
    y = R.conv_ref(xh + xl, wh + wl, None, 1, 1) - R.conv_ref(xl, wl, None, 1, 1)
    if bias is not None:
        y = y + bias.detach().cpu().double().reshape(1, 1, 1, -1)
    return R.ACTS[act](y, slope)


def rel_err64(a, ref):
    """max |a - ref| / max |ref| in float64 (gpu_util.rel_err goes through fp32, which is this file's own error level)."""
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return ((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


# ---- the rows of tests/test_conv_f6_gpu.py (the CPU test runs the emulation on the Gaussian ones)
Row = collections.namedtuple('Row', 'id B Ci Co H W route kind c1 bias act normin relu_c0 gaussian via')


def _row(id, B, Ci, Co, H, W, route='fwd_f6_64', kind='gauss', c1=0, bias=False, act='none', normin=False, relu_c0=0, via='entry'):
    """via: 'entry' (hoig_conv2d_fwd_f6_ex itself), or the operator of hoig_amd.ops the row goes through"""
    return Row(id, B, Ci, Co, H, W, route, kind, c1, bias, act, normin, relu_c0, kind == 'gauss' and not normin, via)


ROWS = [
    _row('one_tile', 1, 64, 64, 8, 32),                                   # every pixel touches the zero frame; one 64-channel block
    _row('blocks3_tiles4', 1, 192, 64, 16, 64),                           # three blocks: the halo restaged twice; tile seams in x and y
    _row('co192', 1, 64, 192, 8, 64),                                     # N & 127 != 0: three 64-channel tiles (the n0 offsets)
    _row('n128', 3, 64, 256, 32, 256, 'fwd_f6_128'),                      # 96 pixel tiles x 2 = 192 workgroups: the smallest 128-channel launch
    _row('n64_by_count', 2, 64, 256, 32, 256),                            # one image short: 128 < 192, four 64-channel tiles
    _row('cat_32_96', 2, 128, 64, 8, 32, c1=32),                          # a 64-channel block that straddles the two tensors
    _row('cat_96_32', 2, 128, 64, 8, 32, c1=96),
    _row('cat_64_64', 2, 128, 64, 8, 32, c1=64),
] + [_row('bias_' + a, 1, 64, 64, 8, 32, bias=True, act=a) for a in ('none', 'relu', 'lrelu', 'tanh', 'sigmoid')] + [
    _row('normin_relu0', 2, 128, 64, 8, 32, 'fwd_f6_64_normin', normin=True, relu_c0=0),
    _row('normin_relu_c1', 2, 128, 64, 8, 32, 'fwd_f6_64_normin', c1=32, normin=True, relu_c0=32),
    _row('normin_norelu', 2, 128, 64, 8, 32, 'fwd_f6_64_normin', normin=True, relu_c0=128),
    _row('normin_n128', 3, 64, 256, 32, 256, 'fwd_f6_128_normin', normin=True, relu_c0=0),
    _row('stats', 2, 64, 64, 16, 32),
    _row('spread', 1, 64, 64, 8, 32, kind='spread'),                      # magnitudes 2^-8 .. 2^8 inside one block: small elements quantise to 0
    _row('dead_block', 1, 128, 64, 8, 32, kind='dead_block'),             # an all-zero block of x (scale 2^-20), an all-zero output channel of w
    _row('saturate', 1, 64, 64, 8, 32, kind='saturate'),                  # block maxima in [7.75, 8) x scale: hi saturates at 7.5
    _row('tiny', 1, 64, 64, 8, 32, kind='tiny'),                          # activations of order 2^-10: lo is an fp16 subnormal
    # through hoig_amd.ops: the planes, records and descriptor the operators make themselves
    _row('ops_conv2d', 1, 128, 64, 8, 64, bias=True, act='lrelu', via='conv2d'),
    _row('ops_cat2', 3, 128, 64, 32, 256, c1=64, via='cat2'),            # (the smallest map conv2d_cat2 keeps off cat_channels: 192 4-row tiles)
]
ROW = {r.id: r for r in ROWS}
assert len(ROW) == len(ROWS)


def _magnitudes(n, g):
    """per-channel magnitudes in [0.05, 3], log-uniform"""
    return torch.exp(torch.rand(n, generator=g) * (np.log(3.0) - np.log(0.05)) + np.log(0.05))


def _plant_maxima(t, top, g):
    """In every 32-block of the last axis: the other elements clamped to 0.85 top, one element set to +-[7.75, 8) / 8 * top."""
    t = t.clamp(-0.85 * top, 0.85 * top)
    blk = t.reshape(t.shape[:-1] + (t.shape[-1] // 32, 32)).clone()
    pos = torch.randint(0, 32, blk.shape[:-1] + (1,), generator=g)
    val = (7.75 + 0.25 * torch.rand(pos.shape, generator=g)) / 8.0 * top
    val = val * (torch.randint(0, 2, pos.shape, generator=g) * 2 - 1)
    blk.scatter_(-1, pos, val.float())
    return blk.reshape(t.shape)


@functools.lru_cache(maxsize=None)
def operands(rid):
    """Seeded operands of row `rid`, fp32 on the CPU, made once and never written to: dict x (NHWC, all gathered channels), w (logical),
    bias or None, in_scale / in_shift (B, Ci) or None.  Gaussian as conv_reference.make_case, times a per-channel magnitude in
    [0.05, 3] (x per channel, w per input channel), unless the row's kind says otherwise."""
    r = ROW[rid]
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(rid)) % 9973
    x, w, b, _ = R.make_case(R.Case(r.B, r.Ci, r.Co, r.H, r.W, 3, 1, 1, False, r.bias, 'none', 0.2, seed))
    g = torch.Generator().manual_seed(77 + seed)
    if r.kind == 'spread':
        m = 2.0 ** (torch.arange(32, dtype=torch.float32) * (16.0 / 31.0) - 8.0)
        x = x * m[torch.randperm(32, generator=g)].repeat(r.Ci // 32)
        w = w * m[torch.randperm(32, generator=g)].repeat(r.Ci // 32).reshape(1, -1, 1, 1)
    else:
        x = x * _magnitudes(r.Ci, g)
        w = w * _magnitudes(r.Ci, g).reshape(1, -1, 1, 1)
    if r.kind == 'dead_block':
        x[..., 32:64] = 0.0
        w[5] = 0.0
    elif r.kind == 'saturate':
        x = _plant_maxima(x, 4.0, g)
        w = _plant_maxima(w.permute(0, 2, 3, 1).contiguous(), 2.0 ** -4, g).permute(0, 3, 1, 2).contiguous()
    elif r.kind == 'tiny':
        x = x * 2.0 ** -10
    out = dict(x=x.contiguous(), w=w.contiguous(), bias=b, in_scale=None, in_shift=None)
    if r.normin:          # given directly, different per image and channel, also on the first tensor of a concatenation (ops passes 1 and
        # 0 there; other values pin the loader's indexing across the straddling block); shifts of order 1: a normalised frame shows at 1e-1
        out['in_scale'] = torch.rand(r.B, r.Ci, generator=g) + 0.5
        out['in_shift'] = torch.randn(r.B, r.Ci, generator=g)
    return out


def row_args(rid):
    """Keyword arguments of conv_f6_ref for row `rid` (x split into x | x2 where the row concatenates)."""
    r, o = ROW[rid], operands(rid)
    x, x2 = (o['x'][..., :r.c1].contiguous(), o['x'][..., r.c1:].contiguous()) if r.c1 else (o['x'], None)
    return dict(x=x, w=o['w'], bias=o['bias'], act=r.act, slope=0.2, x2=x2, in_scale=o['in_scale'], in_shift=o['in_shift'],
                in_relu_c0=r.relu_c0)


@functools.lru_cache(maxsize=None)
def emulated(rid, defect=None):
    return conv_f6_ref(defect=defect, **row_args(rid))


@functools.lru_cache(maxsize=None)
def truth(rid):
    """float64 convolution of the row's unrounded operands (the normalisation in float64 as well)."""
    r, o = ROW[rid], operands(rid)
    g = o['x'].double()
    if r.normin:
        g = g * o['in_scale'].double().reshape(r.B, 1, 1, -1) + o['in_shift'].double().reshape(r.B, 1, 1, -1)
        g[..., r.relu_c0:] = g[..., r.relu_c0:].clamp_min(0.0)
    return R.conv_ref(g, o['w'], o['bias'], 1, 1, False, r.act, 0.2)
