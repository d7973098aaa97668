"""Every convolution backward route against float64: one table, one test body (docs/conv_backward_parity.md).

A row names the launcher it was shaped for; the library's route record (hoig_conv_last_route, hoig_amd/csrc/conv_route.h) says which one
ran, and a row that does not reach its route FAILS.  Per row and arithmetic mode: y, dx, dw, db against tests/conv_reference.py in
gpu_util.rel_err, then the entry point the autograd layer calls once more into PREFILLED dw / db buffers -- a route that stores
where it must add fails there.  Bounds: PREC_BOUNDS of tests/test_ops_gpu.py (TOL in exact fp32), or, where the reference's own emulation
of the mode's operand rounding says the shape cannot meet them, 4 x that emulation (conv_reference.rounded_operand_error)."""
import collections
import ctypes
import functools

import pytest
import torch

import conv_reference as R
import gpu_util
from test_ops_gpu import PREC_BOUNDS, TOL

pytestmark = pytest.mark.gpu

MIXED = 'bf16x3:f16x2'
MODES16 = ('bf16x3', MIXED)
ALL3 = MODES16 + ('f32',)
# rows above this many multiply-adds take PREC_BOUNDS as they are (never wider): their float64 emulation would cost more than the test
EMU_MAX_FLOP = 1e9

Row = collections.namedtuple('Row', 'id case wgrad dgrad fwd tuning kind modes')


def row(id, case, wgrad=None, dgrad=None, fwd=None, tuning=None, kind='conv', modes=MODES16):
    return Row(id, R.Case(*case), wgrad, dgrad, fwd, tuning or {}, kind, modes)


def C(B, Ci, Co, H, W, k, stride, pad, transposed=False, bias=False, act='none'):
    return (B, Ci, Co, H, W, k, stride, pad, transposed, bias, act, 0.2, B * 7 + Ci + 3 * Co + H + k)


T, Bs = True, True          # (readable flags in the table: transposed, bias)
F32_128x32 = 'dgrad_igemm_f32_128x32'

# kind: 'conv' (ops.conv2d / ops.conv_transpose2d, accumulate through hoig_conv2d_bwd_weight), 'fwd' (forward only: the activation
# epilogues), 'fork' (ops.conv2d_fork: the second reader's gradient enters the data gradient), 'cat' (dw through
# hoig_conv2d_cat_bwd_weight), 'split' / 'split_w' (dw -- and dx -- from pre-split dy), 'split_pair' / 'split_pair_w' (the grouped
# forms), 'noscratch' (the thin weight gradient on a stream without a registered scratch block), 'fwd_pair' (forward only: y of both
# problems from hoig_conv2d_fwd_packed_pair, `fwd` being the route of that grouped launch).
# wgrad / dgrad / fwd: the route asserted (a dict where it depends on the mode; None: not asserted for this row).
ROWS = [
    # ---------------------------------------------------------------- weight gradient: launch_wgrad_halo by variant
    row('halo_cm1', C(2, 32, 64, 6, 64, 3, 1, 1, bias=Bs), 'wgrad_halo_cm1', F32_128x32),
    row('halo_cm1_3tiles', C(3, 96, 192, 4, 96, 3, 1, 1, bias=Bs), 'wgrad_halo_cm1', 'dgrad_igemm_bf16_64x128'),
    row('halo_cm2_th2', C(2, 32, 128, 6, 64, 3, 1, 1, bias=Bs), 'wgrad_halo_cm2', F32_128x32),
    row('halo_th4', C(2, 512, 512, 32, 64, 3, 1, 1, bias=Bs), {'bf16x3': 'wgrad_halo_cm2', MIXED: 'wgrad_halo_th4'}),
    row('halo_s2_cm1', C(2, 32, 64, 8, 64, 3, 2, 1, bias=Bs), 'wgrad_halo_s2_cm1', F32_128x32, fwd='fwd_s2g_m16p4_64'),
    row('halo_s2_cm2', C(2, 32, 128, 12, 64, 3, 2, 1, bias=Bs), 'wgrad_halo_s2_cm2', F32_128x32),
    row('halo_tout', C(2, 128, 64, 6, 64, 3, 2, 1, T), 'wgrad_halo_tout', 'dgrad_igemm_bf16_64x128'),
    row('halo_tout_small', C(2, 128, 32, 4, 32, 3, 2, 1, T), 'wgrad_halo_tout', 'dgrad_s2g_m16p4_128'),
    row('halo_5x5', C(2, 32, 64, 8, 36, 5, 1, 0, bias=Bs), 'wgrad_halo_5x5', F32_128x32, tuning={'wflat5': 0}),
    row('flat5', C(2, 32, 64, 9, 20, 5, 1, 0, bias=Bs), 'wgrad_flat5', F32_128x32),
    row('flat5_fused_bias', C(2, 32, 64, 8, 36, 5, 1, 0, bias=Bs), 'wgrad_flat5', F32_128x32, tuning={'wflat5': 2}),
    row('tile5', C(2, 32, 64, 12, 72, 5, 1, 0, bias=Bs), 'wgrad_tile5', F32_128x32),
    row('tile5_fused_bias', C(2, 32, 64, 8, 100, 5, 1, 0, bias=Bs), 'wgrad_tile5', F32_128x32),
    # ---------------------------------------------------------------- the generic 16-bit weight gradient
    row('bf16_4x4s2_64', C(2, 32, 64, 8, 8, 4, 2, 1, bias=Bs), 'wgrad_bf16_64', F32_128x32),
    row('bf16_4x4s2_128', C(2, 64, 128, 10, 6, 4, 2, 1, bias=Bs), 'wgrad_bf16_128', 'dgrad_igemm_bf16_64x64'),
    row('bf16_4x4s1', C(2, 64, 128, 9, 9, 4, 1, 1, bias=Bs), 'wgrad_bf16_128', 'dgrad_igemm_bf16_64x64'),
    row('bf16_1x1', C(2, 64, 96, 5, 7, 1, 1, 0, bias=Bs), 'wgrad_bf16_128', 'dgrad_igemm_bf16_64x64'),
    row('bf16_3x3_w9', C(2, 36, 40, 7, 9, 3, 1, 1, bias=Bs), 'wgrad_bf16_64'),
    row('bf16_convT_off_halo', C(2, 128, 64, 5, 7, 3, 2, 1, T), 'wgrad_bf16_64', 'dgrad_igemm_bf16_64x128'),
    # ---------------------------------------------------------------- the fp32 weight gradient, also as the fallback of a 16-bit run
    row('f32_attn_128_25', C(2, 128, 25, 8, 8, 1, 1, 0, bias=Bs), 'wgrad_f32_32x128', modes=ALL3),
    row('f32_d_first_19', C(2, 19, 64, 16, 16, 4, 2, 1, bias=Bs), 'wgrad_f32_64x128', F32_128x32, fwd={'f32': 'fwd_igemm_f32_64x64'},
        modes=ALL3),
    row('f32_32x64', C(2, 4, 16, 6, 6, 3, 1, 1, bias=Bs), 'wgrad_f32_32x64', F32_128x32, modes=ALL3),
    row('f32_128x64', C(2, 3, 128, 10, 10, 3, 1, 1, bias=Bs), 'wgrad_f32_128x64', F32_128x32, fwd={'f32': 'fwd_igemm_f32_64x128'},
        modes=ALL3),
    row('f32_128x128', C(2, 16, 96, 6, 6, 3, 1, 1, bias=Bs), 'wgrad_f32_128x128', F32_128x32, modes=('f32',)),
    row('f32_32x128', C(2, 16, 24, 6, 6, 3, 1, 1, bias=Bs), 'wgrad_f32_32x128', F32_128x32, fwd='fwd_igemm_f32_128x32', modes=('f32',)),
    row('f32_64x128', C(2, 16, 48, 6, 6, 3, 1, 1, bias=Bs), 'wgrad_f32_64x128', F32_128x32, modes=('f32',)),
    row('small_7x7_head', C(2, 64, 3, 8, 40, 7, 1, 3), 'wgrad_small', 'dgrad_small',
        fwd={'f32': 'fwd_small', 'bf16x3': 'fwd_head7', MIXED: 'fwd_head7'}, modes=ALL3),
    # ---------------------------------------------------------------- pre-split dy, the concatenated input
    row('dma', C(2, 32, 128, 8, 32, 3, 1, 1), 'wgrad_dma', kind='split_w', modes=(MIXED,)),
    row('dma_dgrad_128', C(5, 128, 128, 32, 160, 3, 1, 1), 'wgrad_dma', 'dgrad_halo3_m16_128_split', kind='split', modes=(MIXED,)),
    row('dma_dgrad_64', C(4, 64, 128, 64, 256, 3, 1, 1), 'wgrad_dma', 'dgrad_halo3_m16_64_split', kind='split', modes=(MIXED,)),
    row('dma_pair', C(2, 32, 128, 8, 32, 3, 1, 1), 'wgrad_dma_pair', kind='split_pair_w', modes=(MIXED,)),
    row('dma_pair_dgrad_128', C(3, 128, 128, 32, 160, 3, 1, 1), 'wgrad_dma_pair', 'dgrad_halo3_m16_128_split_pair', kind='split_pair',
        modes=(MIXED,)),
    row('dma_pair_dgrad_64', C(2, 64, 128, 64, 256, 3, 1, 1), 'wgrad_dma_pair', 'dgrad_halo3_m16_64_split_pair', kind='split_pair',
        modes=(MIXED,)),
    row('cat_64_64', C(2, 128, 64, 4, 64, 3, 1, 1, bias=Bs), 'wgrad_halo_cm1', kind='cat'),
    # ---------------------------------------------------------------- data gradient: the packed-plane dispatcher (run())
    row('k128', C(2, 1024, 128, 8, 8, 1, 1, 0), 'wgrad_bf16_128', 'dgrad_k128'),
    row('halo1_64', C(5, 64, 32, 32, 128, 1, 1, 0), None, 'dgrad_halo1_64'),
    row('halo1_128w', C(5, 128, 32, 32, 128, 1, 1, 0), None, 'dgrad_halo1_128w'),
    row('halo1_128', C(3, 128, 32, 64, 256, 1, 1, 0), None, 'dgrad_halo1_128'),
    row('same5_64', C(5, 64, 32, 32, 128, 5, 1, 2), None, 'dgrad_same5_64'),
    row('same5_128w', C(5, 128, 32, 32, 128, 5, 1, 2), None, 'dgrad_same5_128w'),
    row('same5_128', C(3, 128, 32, 64, 256, 5, 1, 2), None, 'dgrad_same5_128'),
    row('halo3_64', C(5, 64, 32, 32, 128, 3, 1, 1), None, 'dgrad_halo3_64'),
    row('halo3_128w', C(5, 128, 32, 32, 128, 3, 1, 1), None, 'dgrad_halo3_128w'),
    row('halo3_128', C(4, 256, 32, 12, 512, 3, 1, 1), None, 'dgrad_halo3_128'),
    row('halo3_m16_64', C(4, 64, 32, 64, 256, 3, 1, 1), None, 'dgrad_halo3_m16_64'),
    row('halo3_m16_128', C(5, 128, 32, 32, 160, 3, 1, 1), None, 'dgrad_halo3_m16_128'),
    row('flat_k3', C(2, 128, 32, 8, 8, 3, 1, 1), None, 'dgrad_flat_m16_k3'),
    row('flat_k3_off', C(2, 128, 32, 8, 8, 3, 1, 1), None, 'dgrad_igemm_bf16_64x128', tuning={'flat5': 1}),
    row('flat_k5', C(2, 128, 32, 12, 12, 5, 1, 0), None, 'dgrad_flat_m16_k5'),
    row('flat_k5_off', C(2, 128, 32, 12, 12, 5, 1, 0), None, 'dgrad_igemm_bf16_64x128', tuning={'flat5': 0}),
    row('halo5_ksplit', C(2, 128, 32, 8, 72, 5, 1, 0), None, 'dgrad_halo5_m16_ksplit'),
    row('halo5_nosplit', C(2, 128, 32, 8, 72, 5, 1, 0), None, 'dgrad_halo5_m16', tuning={'halo5': 2}),
    row('halo5_off', C(2, 128, 32, 8, 72, 5, 1, 0), None, 'dgrad_igemm_bf16_64x128', tuning={'halo5': 0}),
    # stride-2 3x3: Conv2d's data gradient scatters, ConvTranspose2d's gathers
    row('s2s_p4_64', C(2, 64, 32, 8, 64, 3, 2, 1), None, {'bf16x3': 'dgrad_s2s_64', MIXED: 'dgrad_s2s_m16p4_64'}),
    row('s2s_p4_128', C(2, 128, 32, 8, 64, 3, 2, 1), None, 'dgrad_s2s_m16p4_128'),
    row('s2s_p8_128', C(4, 128, 32, 64, 256, 3, 2, 1), None, 'dgrad_s2s_m16p8_128'),
    row('s2s_m16_128', C(3, 128, 32, 64, 256, 3, 2, 1), None, 'dgrad_s2s_m16_128'),
    row('s2s_m16_64', C(3, 64, 32, 64, 256, 3, 2, 1), None, {'bf16x3': 'dgrad_s2s_64', MIXED: 'dgrad_s2s_m16_64'}),
    row('s2s_m16_128_nopipe', C(2, 128, 32, 8, 64, 3, 2, 1), None, 'dgrad_s2s_m16_128', tuning={'s2_pipe': 0}),
    row('s2s_128_k32', C(2, 128, 32, 8, 64, 3, 2, 1), None, 'dgrad_s2s_128', tuning={'s2_16': 0}),
    row('s2g_p4_64', C(2, 64, 32, 4, 32, 3, 2, 1, T), 'wgrad_f32_32x128', 'dgrad_s2g_m16p4_64'),
    row('s2g_p8_128', C(4, 128, 32, 64, 256, 3, 2, 1, T), 'wgrad_halo_tout', 'dgrad_s2g_m16p8_128'),
    row('s2g_m16_128', C(3, 128, 32, 32, 512, 3, 2, 1, T), 'wgrad_halo_tout', 'dgrad_s2g_m16_128'),
    row('s2g_m16_64_nopipe', C(2, 64, 32, 4, 32, 3, 2, 1, T), None, 'dgrad_s2g_m16_64', tuning={'s2_pipe': 0}),
    row('s2g_64_k32', C(2, 64, 32, 4, 32, 3, 2, 1, T), None, 'dgrad_s2g_64', tuning={'s2_16': 0}),
    row('s2g_128_k32', C(2, 128, 32, 4, 32, 3, 2, 1, T), None, 'dgrad_s2g_128', tuning={'s2_16': 0}),
    # the generic implicit GEMM: 32x32x16 (data gradients by default), 16x16x32 under igemm16 = 2
    row('ig_64x64', C(2, 64, 32, 8, 8, 4, 2, 1), None, 'dgrad_igemm_bf16_64x64'),
    row('ig_128x64', C(2, 64, 32, 128, 258, 1, 1, 0), None, 'dgrad_igemm_bf16_128x64'),
    row('ig_128x128', C(2, 256, 32, 128, 129, 1, 1, 0), None, 'dgrad_igemm_bf16_128x128'),
    row('ig_128x128w', C(2, 128, 32, 64, 130, 1, 1, 0), None, 'dgrad_igemm_bf16_128x128w'),
    row('ig_64x128', C(2, 128, 32, 5, 7, 1, 1, 0), None, 'dgrad_igemm_bf16_64x128'),
    row('ig_64x128_ksplit', C(2, 128, 64, 8, 8, 4, 2, 1), None, 'dgrad_igemm_bf16_64x128'),
    row('m16_64x64', C(2, 64, 32, 8, 8, 4, 2, 1), None, 'dgrad_igemm_m16_64x64', tuning={'igemm16': 2}),
    row('m16_128x64', C(2, 64, 32, 128, 258, 1, 1, 0), None, 'dgrad_igemm_m16_128x64', tuning={'igemm16': 2}),
    row('m16_128x128', C(2, 256, 32, 128, 129, 1, 1, 0), None, 'dgrad_igemm_m16_128x128', tuning={'igemm16': 2}),
    row('m16_128x128w', C(2, 128, 32, 64, 130, 1, 1, 0), None, 'dgrad_igemm_m16_128x128w', tuning={'igemm16': 2}),
    row('m16_64x128', C(2, 128, 32, 5, 7, 1, 1, 0), None, 'dgrad_igemm_m16_64x128', tuning={'igemm16': 2}),
    row('m16_64x128_ksplit', C(2, 128, 64, 8, 8, 4, 2, 1), None, 'dgrad_igemm_m16_64x128', tuning={'igemm16': 2}),
    # exact fp32
    row('f32_ig_64x64', C(2, 64, 32, 6, 6, 3, 1, 1), None, 'dgrad_igemm_f32_64x64', modes=('f32',)),
    row('f32_ig_128x64', C(2, 64, 32, 128, 256, 1, 1, 0), None, 'dgrad_igemm_f32_128x64', modes=('f32',)),
    row('f32_ig_128x128', C(2, 256, 32, 128, 128, 1, 1, 0), None, 'dgrad_igemm_f32_128x128', modes=('f32',)),
    row('f32_ig_64x128', C(2, 96, 32, 6, 6, 3, 1, 1), None, 'dgrad_igemm_f32_64x128', modes=('f32',)),
    # the second reader's gradient: in the halo kernel's epilogue, and by hoig_add behind a kernel that has none
    row('fork_halo_epilogue', C(5, 64, 32, 32, 128, 3, 1, 1), None, 'dgrad_halo3_64', kind='fork'),
    row('fork_separate_add', C(2, 64, 32, 8, 8, 4, 2, 1), None, 'dgrad_igemm_bf16_64x64', kind='fork'),
    # ---------------------------------------------------------------- forward only: the activation epilogues
    row('act_halo3_lrelu', C(5, 32, 64, 32, 128, 3, 1, 1, bias=Bs, act='lrelu'), fwd='fwd_halo3_64', kind='fwd'),
    row('act_igemm_relu', C(2, 64, 64, 8, 8, 4, 2, 1, bias=Bs, act='relu'), fwd='fwd_igemm_m16_64x64', kind='fwd'),
    row('act_thin_tanh', C(2, 3, 64, 8, 64, 7, 1, 3, bias=Bs, act='tanh'), fwd='fwd_thin', kind='fwd'),
    row('act_head7_tanh', C(2, 64, 3, 8, 64, 7, 1, 3, bias=Bs, act='tanh'), fwd='fwd_head7', kind='fwd'),
    row('act_f32_sigmoid', C(2, 16, 24, 6, 6, 3, 1, 1, bias=Bs, act='sigmoid'), fwd='fwd_igemm_f32_128x32', kind='fwd', modes=('f32',)),
    # activation + live bias: hoig_act_bwd_colsum makes db (a smooth activation: no mask to flip in the max norm)
    row('act_bwd_colsum_tanh', C(2, 64, 128, 9, 9, 4, 1, 1, bias=Bs, act='tanh'), 'wgrad_bf16_128', 'dgrad_igemm_bf16_64x64'),
    row('act_bwd_colsum_halo', C(2, 32, 64, 6, 64, 3, 1, 1, bias=Bs, act='sigmoid'), 'wgrad_halo_cm1', F32_128x32),
]

# ---- the forward through the launchers it shares with the data gradient (run() in conv_igemm_bf16.hip, launchers in conv_halo32.hip: the same conditions with
# N = Co, and always three fp16 terms): the rows above with Ci and Co swapped.  Full rows, so their backward is checked as well.
_FWD = [
    ('halo1_64', C(5, 32, 64, 32, 128, 1, 1, 0), 'fwd_halo1_64', None),
    ('halo1_128w', C(5, 32, 128, 32, 128, 1, 1, 0), 'fwd_halo1_128w', None),
    ('halo1_128', C(3, 32, 128, 64, 256, 1, 1, 0), 'fwd_halo1_128', None),
    ('same5_64', C(5, 32, 64, 32, 128, 5, 1, 2), 'fwd_same5_64', None),
    ('same5_128w', C(5, 32, 128, 32, 128, 5, 1, 2), 'fwd_same5_128w', None),
    ('same5_128', C(3, 32, 128, 64, 256, 5, 1, 2), 'fwd_same5_128', None),
    ('halo3_128w', C(5, 32, 128, 32, 128, 3, 1, 1), 'fwd_halo3_128w', None),
    ('halo3_128', C(4, 32, 256, 12, 512, 3, 1, 1), 'fwd_halo3_128', None),
    ('halo3_m16_64', C(4, 32, 64, 64, 256, 3, 1, 1), 'fwd_halo3_m16_64', None),
    ('halo3_m16_128', C(5, 32, 128, 32, 160, 3, 1, 1), 'fwd_halo3_m16_128', None),
    ('flat_k3', C(2, 32, 128, 8, 8, 3, 1, 1), 'fwd_flat_m16_k3', None),
    ('flat_k5', C(2, 32, 128, 12, 12, 5, 1, 0), 'fwd_flat_m16_k5', None),
    ('halo5_ksplit', C(2, 32, 128, 8, 72, 5, 1, 0), 'fwd_halo5_m16_ksplit', None),
    ('halo5_nosplit', C(2, 32, 128, 8, 72, 5, 1, 0), 'fwd_halo5_m16', {'halo5': 2}),
    ('s2g_p4_128', C(2, 32, 128, 8, 64, 3, 2, 1), 'fwd_s2g_m16p4_128', None),
    ('s2g_p8_128', C(4, 32, 128, 128, 512, 3, 2, 1), 'fwd_s2g_m16p8_128', None),
    ('s2g_m16_128', C(3, 32, 128, 128, 512, 3, 2, 1), 'fwd_s2g_m16_128', None),
    ('s2g_m16_64_nopipe', C(2, 32, 64, 8, 64, 3, 2, 1), 'fwd_s2g_m16_64', {'s2_pipe': 0}),
    ('s2g_64_k32', C(2, 32, 64, 8, 64, 3, 2, 1), 'fwd_s2g_64', {'s2_16': 0}),
    ('s2g_128_k32', C(2, 32, 128, 8, 64, 3, 2, 1), 'fwd_s2g_128', {'s2_16': 0}),
    ('s2s_64', C(2, 32, 64, 4, 32, 3, 2, 1, T), 'fwd_s2s_64', None),          # (three terms, 64-channel tiles: kept on the 32x32 kernel)
    ('s2s_p4_128', C(2, 32, 128, 4, 32, 3, 2, 1, T), 'fwd_s2s_m16p4_128', None),
    ('s2s_p8_128', C(4, 32, 128, 32, 128, 3, 2, 1, T), 'fwd_s2s_m16p8_128', None),
    ('s2s_m16_128', C(3, 32, 128, 32, 128, 3, 2, 1, T), 'fwd_s2s_m16_128', None),
    ('s2s_128_k32', C(2, 32, 128, 4, 32, 3, 2, 1, T), 'fwd_s2s_128', {'s2_16': 0}),
    ('m16_128x64', C(2, 32, 64, 128, 258, 1, 1, 0), 'fwd_igemm_m16_128x64', None),
    ('m16_128x128', C(2, 32, 256, 128, 129, 1, 1, 0), 'fwd_igemm_m16_128x128', None),
    ('m16_128x128w', C(2, 32, 128, 64, 130, 1, 1, 0), 'fwd_igemm_m16_128x128w', None),
    ('ig_64x64', C(2, 32, 64, 8, 8, 4, 2, 1), 'fwd_igemm_bf16_64x64', {'igemm16': 0}),
    ('ig_64x128', C(2, 32, 128, 5, 7, 1, 1, 0), 'fwd_igemm_bf16_64x128', {'igemm16': 0}),
    ('ig_128x64', C(2, 32, 64, 128, 258, 1, 1, 0), 'fwd_igemm_bf16_128x64', {'igemm16': 0}),
    ('ig_128x128', C(2, 32, 256, 128, 129, 1, 1, 0), 'fwd_igemm_bf16_128x128', {'igemm16': 0}),
    ('ig_128x128w', C(2, 32, 128, 64, 130, 1, 1, 0), 'fwd_igemm_bf16_128x128w', {'igemm16': 0}),
    ('dot_patchgan_head', C(2, 256, 1, 8, 8, 4, 1, 1, bias=Bs), 'fwd_dot', None),
]
for _id, _case, _route, _tune in _FWD:
    ROWS.append(row('fwd_' + _id, _case, fwd=_route, tuning=_tune))
ROWS += [
    row('fwd_f32_128x64', C(2, 32, 64, 128, 256, 1, 1, 0), fwd='fwd_igemm_f32_128x64', modes=('f32',)),
    row('fwd_f32_128x128', C(2, 32, 256, 128, 128, 1, 1, 0), fwd='fwd_igemm_f32_128x128', modes=('f32',)),
    row('fwd_f32_small_ci', C(2, 3, 64, 8, 64, 7, 1, 3, bias=Bs), fwd='fwd_small_ci', modes=('f32',)),
    # more activation epilogues, forward only
    row('act_halo1_relu', C(5, 32, 64, 32, 128, 1, 1, 0, bias=Bs, act='relu'), fwd='fwd_halo1_64', kind='fwd'),
    row('act_same5_lrelu', C(5, 32, 64, 32, 128, 5, 1, 2, bias=Bs, act='lrelu'), fwd='fwd_same5_64', kind='fwd'),
    row('act_halo3_m16_sigmoid', C(5, 32, 128, 32, 160, 3, 1, 1, bias=Bs, act='sigmoid'), fwd='fwd_halo3_m16_128', kind='fwd'),
    row('act_flat_k3_tanh', C(2, 32, 128, 8, 8, 3, 1, 1, bias=Bs, act='tanh'), fwd='fwd_flat_m16_k3', kind='fwd'),
    row('act_halo5_relu', C(2, 32, 128, 8, 72, 5, 1, 0, bias=Bs, act='relu'), fwd='fwd_halo5_m16', kind='fwd'),      # (an activation: no K split)
    row('act_s2g_relu', C(2, 32, 128, 8, 64, 3, 2, 1, bias=Bs, act='relu'), fwd='fwd_s2g_m16p4_128', kind='fwd'),
    row('act_s2g_p8_lrelu', C(4, 32, 128, 128, 512, 3, 2, 1, bias=Bs, act='lrelu'), fwd='fwd_s2g_m16p8_128', kind='fwd'),
    row('act_thin_out_tanh', C(2, 64, 3, 8, 64, 3, 1, 1, bias=Bs, act='tanh'), fwd='fwd_thin_out', kind='fwd'),
    # ConvTranspose2d onto 64-channel tiles: on three terms it stays on the 32x32 kernel (fwd_s2s_64 above, launch_halo_s2), so the
    # 16x16x32 forms are reached by a TWO-term forward only -- at most one workgroup per CU the 4-row form, above that (and N % 128 != 0,
    # which rules out the 8-row form) the kernel of conv_halo16.hip
    row('fwd_s2s_p4_64_f16x2', C(2, 32, 64, 4, 32, 3, 2, 1, T), fwd='fwd_s2s_m16p4_64', kind='fwd', modes=('f16x2',)),
    row('fwd_s2s_m16_64_f16x2', C(5, 32, 64, 32, 64, 3, 2, 1, T), fwd='fwd_s2s_m16_64', kind='fwd', modes=('f16x2',)),
    # the grouped forward on 64-channel tiles, through its entry point: ops.conv2d_pair never gets here (pair_ok asks for Co % 128 == 0);
    # Co = 64 needs 2 B (W / 32) (H / 4) >= 512 workgroups for the 8-row tiling
    row('fwd_pair_64', C(2, 32, 64, 64, 256, 3, 1, 1, bias=Bs), fwd='fwd_halo3_m16_64_pair', kind='fwd_pair', modes=(MIXED,)),
]

# ---- the thin-channel layers (conv_thin.hip): one row per fragment-count class of hoig_conv_thin_wgrad (nfr = ceil(R*S*F / 32): 1, 2,
# <= 4, <= 8, > 8), each with at most 8 tiles (fp32 atomics straight into dw) and with more (workspace + thin_reduce_kernel)
_THIN_IN = [(3, 3, 64, 1), (6, 3, 64, 2), (12, 3, 128, 4), (3, 7, 64, 5), (8, 7, 64, 13)]                     # Ci, k, Co, nfr
_THIN_OUT = [(2, 3, 64, 1), (1, 7, 64, 2), (8, 3, 128, 3), (3, 7, 64, 5), (5, 7, 64, 8), (8, 7, 64, 13)]      # Co, k, Ci, nfr
for _hw, _how in (((4, 64), 'direct'), ((8, 96), 'ws')):
    for _ci, _k, _co, _nfr in _THIN_IN:
        ROWS.append(row('thin_in_%dx%d_ci%d_nfr%d_%s' % (_k, _k, _ci, _nfr, _how), C(2, _ci, _co, _hw[0], _hw[1], _k, 1, _k // 2, bias=Bs),
                        'wgrad_thin_in_' + _how, 'dgrad_thin_out' if _k == 3 else F32_128x32, fwd='fwd_thin'))
    for _co, _k, _ci, _nfr in _THIN_OUT:
        ROWS.append(row('thin_out_%dx%d_co%d_nfr%d_%s' % (_k, _k, _co, _nfr, _how), C(2, _ci, _co, _hw[0], _hw[1], _k, 1, _k // 2, bias=Bs),
                        'wgrad_thin_out_' + _how, 'dgrad_thin'))
ROWS.append(row('thin_in_no_scratch', C(2, 8, 64, 8, 96, 7, 1, 3), 'wgrad_thin_in_direct', kind='noscratch'))
ROWS.append(row('thin_out_no_scratch', C(2, 64, 3, 8, 96, 7, 1, 3), 'wgrad_thin_out_direct', kind='noscratch'))

# Routes that no row of this file reaches, with the reason and the test that pins them.  The completeness test below caps it: no
# weight-gradient route, at most one data-gradient route in five.
NOT_PINNED_HERE = {}

# Forward routes that no row of this file reaches and another test asserts: route -> 'tests/<file>::<test>'.
ASSERTED_ELSEWHERE = {
    'fwd_f6_64': 'tests/test_conv_f6_gpu.py::test_every_f6_route_has_a_row',
    'fwd_f6_128': 'tests/test_conv_f6_gpu.py::test_every_f6_route_has_a_row',
    'fwd_f6_64_normin': 'tests/test_conv_f6_gpu.py::test_every_f6_route_has_a_row',
    'fwd_f6_128_normin': 'tests/test_conv_f6_gpu.py::test_every_f6_route_has_a_row',
    'fwd_igemm_m16_64x128': 'tests/test_conv_f6_gpu.py::test_refused_shapes_touch_nothing_and_run_on_three_terms',
    'fwd_halo3_m16_128_pair': 'tests/test_conv_composites_gpu.py::test_conv2d_pair',
    'fwd_halo3_m16_64_normin': 'tests/test_conv_m16_gpu.py::test_inference_norm_applied_by_the_consumers_loader',
    'fwd_halo3_m16_128_normin': 'tests/test_conv_m16_gpu.py::test_inference_norm_applied_by_the_consumers_loader',
}


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _flops(c):
    Ho, Wo = R.out_hw(c)
    return 2.0 * c.B * Ho * Wo * c.Co * c.Ci * c.k * c.k


@functools.lru_cache(maxsize=None)
def _reference(c):
    """Operands and float64 results of case `c`, computed once per session and never written to."""
    x, w, b, gy = R.make_case(c)
    y = R.conv_ref(x, w, b, c.stride, c.pad, c.transposed, c.act, c.slope)
    dx, dw, db = R.conv_grads_ref(x, w, b, gy, c.stride, c.pad, c.transposed, c.act, c.slope)
    return dict(x=x, w=w, b=b, gy=gy, y=y, dx=dx, dw=dw, db=db)


@functools.lru_cache(maxsize=None)
def _emulation(c, mode):
    return R.rounded_operand_error(c._replace(bias=False, act='none'), mode)


_EXACT = ('wgrad_f32_', 'wgrad_small', 'dgrad_igemm_f32_', 'dgrad_small', 'fwd_igemm_f32_', 'fwd_small', 'fwd_dot')


def _bounds(c, mode, routes):
    """{'y', 'dx', 'dw'} -> (bound, emulation or None).  A pass that ran on an exact-fp32 launcher inside a 16-bit run keeps the three-term
    bound; db takes dw's."""
    if mode == 'f32':
        return {k: (TOL, None) for k in ('y', 'dx', 'dw')}
    parts = mode.split(':')
    fm, bm = parts[0], parts[-1]
    base = {'y': PREC_BOUNDS[fm][0], 'dx': PREC_BOUNDS[bm][1], 'dw': PREC_BOUNDS[bm][2]}
    emu = _emulation(c, mode) if _flops(c) <= EMU_MAX_FLOP else None
    out = {}
    for k, idx in (('y', 0), ('dx', 1), ('dw', 2)):
        if (routes.get(k) or '').startswith(_EXACT):
            out[k] = (PREC_BOUNDS['bf16x3'][idx], None)
        elif emu is None:
            out[k] = (base[k], None)
        else:
            out[k] = (max(base[k], 4.0 * emu[k]), emu[k])
    return out


def _want(target, mode):
    return target.get(mode) if isinstance(target, dict) else target


def _desc(L, c, prec, act=None):
    Ho, Wo = R.out_hw(c)
    a = {'none': L.ACT_NONE, 'relu': L.ACT_RELU, 'lrelu': L.ACT_LRELU, 'tanh': L.ACT_TANH, 'sigmoid': L.ACT_SIGMOID}[act or c.act]
    return L.ConvDesc(c.B, c.H, c.W, c.Ci, Ho, Wo, c.Co, c.k, c.k, c.stride, c.pad, 1 if c.transposed else 0, a, c.slope, prec)


def _split(L, t):
    """fp32 NHWC [.., C] -> the bf16 hi | lo planes of hoig_split_planes_bf16"""
    out = torch.empty(t.shape[:-1] + (2, t.shape[-1]), dtype=torch.bfloat16, device=t.device)
    L.call('hoig_split_planes_bf16', _p(t), _p(out), t.numel() // t.shape[-1], t.shape[-1], torch.cuda.current_stream().cuda_stream)
    return out


def check_row(r, mode, report=None):
    """The one test body.  report: a dict that receives what was measured (the tool that fills docs/conv_backward_parity.md passes one)."""
    from hoig_amd import _lib as L, ops
    c = r.case
    report = {} if report is None else report
    prev_tuning = {k: L.set_tuning(k, v) for k, v in r.tuning.items()}
    ops.set_precision(mode)
    try:
        gpu_util.poison_free_memory()
        ref = _reference(c)
        act = {'none': L.ACT_NONE, 'relu': L.ACT_RELU, 'lrelu': L.ACT_LRELU, 'tanh': L.ACT_TANH, 'sigmoid': L.ACT_SIGMOID}[c.act]
        st = torch.cuda.current_stream().cuda_stream
        xd = ref['x'].cuda().requires_grad_(True)
        wd = ops.pack_weight(ref['w'].cuda(), c.transposed).requires_grad_(True)
        bd = ref['b'].cuda().requires_grad_(True) if c.bias else None
        gy = ref['gy'].cuda()
        seen = {}
        # the autograd engine runs the backward on its device thread and the record is per thread: read it there, when dx arrives
        xd.register_hook(lambda g: seen.update(dx=L.last_route(L.ROUTE_DGRAD), dw=L.last_route(L.ROUTE_WGRAD)))
        gx = None
        if c.transposed:
            y = ops.conv_transpose2d(xd, wd)
        elif r.kind == 'fork':
            y, x2 = ops.conv2d_fork(xd, wd, bd, c.stride, c.pad)
            gx = torch.randn(ref['x'].shape, generator=torch.Generator().manual_seed(5)).cuda()
        else:
            y = ops.conv2d(xd, wd, bd, c.stride, c.pad, act, c.slope)
        seen['y'] = L.last_route(L.ROUTE_FWD)
        if r.kind != 'fwd':
            if gx is not None:
                torch.autograd.backward([y, x2], [gy, gx])
            else:
                y.backward(gy)
        torch.cuda.synchronize()
        report['routes'] = dict(seen)
        bounds = _bounds(c, mode, seen)
        report['bounds'] = bounds

        # ---- the route
        for key, target in (('y', r.fwd), ('dx', r.dgrad), ('dw', r.wgrad)):
            want = _want(target, mode)
            if want is not None and r.kind in ('conv', 'fwd', 'fork') and not (key != 'y' and r.kind == 'fwd'):
                assert seen.get(key) == want, '%s: %s ran on %r, the row was shaped for %r' % (r.id, key, seen.get(key), want)

        # ---- values against float64
        err = report.setdefault('err', {})
        err['y'] = gpu_util.rel_err(y, ref['y'])
        assert err['y'] < bounds['y'][0], ('y', err['y'], bounds['y'])
        if r.kind == 'fwd':
            return report
        if r.kind == 'fwd_pair':
            # the second problem of the grouped launch: its own operands (another seed)
            ref2 = _reference(c._replace(seed=c.seed + 1))
            xb, wb, bb = ref2['x'].cuda(), ops.pack_weight(ref2['w'].cuda(), False), ref2['b'].cuda() if c.bias else None
            (ha, la), (hb, lb) = ops._packed_planes(wd.detach(), False, False), ops._packed_planes(wb, False, False)
            ya, yb = torch.empty_like(y), torch.empty_like(y)
            d = _desc(L, c, ops.precision)
            L.call('hoig_conv2d_fwd_packed_pair', ctypes.byref(d), _p(xd.detach()), _p(xb), _p(ha), _p(la), _p(hb), _p(lb),
                   _p(bd.detach()) if c.bias else None, _p(bb), _p(ya), _p(yb), st)
            torch.cuda.synchronize()
            report['routes_entry'] = {'y': L.last_route(L.ROUTE_FWD)}
            want = _want(r.fwd, mode)
            assert report['routes_entry']['y'] == want, '%s: y ran on %r, the row was shaped for %r' % (r.id, report['routes_entry']['y'], want)
            for key, got, truth in (('y_entry', ya, ref['y']), ('y_b_entry', yb, ref2['y'])):
                err[key] = gpu_util.rel_err(got, truth)
                assert err[key] < bounds['y'][0], (key, err[key], bounds['y'])
            return report
        dx_ref = ref['dx'] if gx is None else ref['dx'] + gx.cpu().double()
        err['dx'] = gpu_util.rel_err(xd.grad, dx_ref)
        err['dw'] = gpu_util.rel_err(wd.grad, ref['dw'])
        assert err['dx'] < bounds['dx'][0], ('dx', err['dx'], bounds['dx'])
        assert err['dw'] < bounds['dw'][0], ('dw', err['dw'], bounds['dw'])
        if c.bias:
            err['db'] = gpu_util.rel_err(bd.grad, ref['db'])
            assert err['db'] < bounds['dw'][0], ('db', err['db'], bounds['dw'])

        # ---- accumulation: the weight-gradient entry point once more, into prefilled buffers
        d = _desc(L, c, ops.precision)
        d_dg, d_wg = ops._bwd_descs(d)
        gen = torch.Generator().manual_seed(77)
        scale = ref['dw'].abs().max().item()
        fill_w = (torch.randn(ref['w'].shape, generator=gen) * scale)
        dw = ops.pack_weight(fill_w.cuda(), c.transposed)
        fill_b = db = None
        if c.bias:
            fill_b = torch.randn(c.Co, generator=gen) * ref['db'].abs().max().item()
            db = fill_b.cuda()
        x0, g = xd.detach(), gy
        if c.act != 'none':          # as _Conv.backward: activation backward and the bias gradient in one pass, then the weight gradient of g
            g = torch.empty_like(gy)
            L.call('hoig_act_bwd_colsum', _p(y.detach()), _p(gy), _p(g), _p(db), act, c.slope, gy.numel() // c.Co, c.Co, st)
        extra = {}
        if r.kind in ('conv', 'fork'):
            ops.wgrad_call('hoig_conv2d_bwd_weight', d_wg, _p(x0), _p(g), _p(dw), _p(db) if c.act == 'none' else None, st)
        elif r.kind == 'noscratch':
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                L.call('hoig_stream_scratch_set', s.cuda_stream, None, 0)
                L.call('hoig_conv2d_bwd_weight', ctypes.byref(d_wg), _p(x0), _p(g), _p(dw), None, s.cuda_stream)
            s.synchronize()
            ops._scratch.pop((x0.device, s.cuda_stream), None)
        elif r.kind == 'cat':
            c1 = c.Ci // 2
            x1, x2c = x0[..., :c1].contiguous(), x0[..., c1:].contiguous()
            L.call('hoig_conv2d_cat_bwd_weight', ctypes.byref(d_wg), _p(x1), c1, _p(x2c), _p(g), _p(dw), _p(db), st)
        elif r.kind in ('split', 'split_w'):
            gs = _split(L, g)
            L.call('hoig_conv2d_bwd_weight_split', ctypes.byref(d_wg), _p(x0), _p(gs), _p(dw), st)
            if r.kind == 'split':
                hi, lo = ops._packed_planes(wd.detach(), False, True)
                dx = torch.empty_like(x0)
                L.call('hoig_conv2d_bwd_data_packed_split', ctypes.byref(d_dg), _p(gs), _p(hi), _p(lo), None, _p(dx), st)
                extra['dx'] = (dx, ref['dx'])
        elif r.kind in ('split_pair', 'split_pair_w'):
            # the second problem of the grouped launch: its own operands (another seed), its own prefilled buffer
            ref2 = _reference(c._replace(seed=c.seed + 1))
            xb, gb = ref2['x'].cuda(), ref2['gy'].cuda()
            fill_w2 = torch.randn(ref['w'].shape, generator=gen) * scale
            dw2 = ops.pack_weight(fill_w2.cuda(), False)
            gs, gsb = _split(L, g), _split(L, gb)
            L.call('hoig_conv2d_bwd_weight_split_pair', ctypes.byref(d_wg), _p(x0), _p(xb), _p(gs), _p(gsb), _p(dw), _p(dw2), st)
            extra['dw_b'] = (dw2 - fill_w2.cuda(), ref2['dw'])
            if r.kind == 'split_pair':
                wb = ops.pack_weight(ref2['w'].cuda(), False)
                (ha, la), (hb, lb) = ops._packed_planes(wd.detach(), False, True), ops._packed_planes(wb, False, True)
                dxa, dxb = torch.empty_like(x0), torch.empty_like(xb)
                L.call('hoig_conv2d_bwd_data_packed_split_pair', ctypes.byref(d_dg), _p(gs), _p(gsb), _p(ha), _p(la), _p(hb), _p(lb),
                       None, None, _p(dxa), _p(dxb), st)
                extra['dx'] = (dxa, ref['dx'])
                extra['dx_b'] = (dxb, ref2['dx'])
        torch.cuda.synchronize()
        again = {'dw': L.last_route(L.ROUTE_WGRAD), 'dx': L.last_route(L.ROUTE_DGRAD)}
        report['routes_entry'] = again
        want_w, want_d = _want(r.wgrad, mode), _want(r.dgrad, mode)
        if r.kind in ('conv', 'fork'):
            assert again['dw'] == seen['dw'], 'the second call ran on %r, the backward on %r' % (again['dw'], seen['dw'])
        elif want_w is not None:
            assert again['dw'] == want_w, '%s: dw ran on %r, the row was shaped for %r' % (r.id, again['dw'], want_w)
        if 'dx' in extra and want_d is not None:
            assert again['dx'] == want_d, '%s: dx ran on %r, the row was shaped for %r' % (r.id, again['dx'], want_d)
        wb_bound = bounds['dw'][0] if not again['dw'].startswith(_EXACT) else PREC_BOUNDS['bf16x3'][2] if mode != 'f32' else TOL
        err['dw_accumulated'] = gpu_util.rel_err(dw - fill_w.cuda(), ref['dw'])
        assert err['dw_accumulated'] < wb_bound, ('dw += ', err['dw_accumulated'], wb_bound)
        if c.bias:
            err['db_accumulated'] = gpu_util.rel_err(db - fill_b.cuda(), ref['db'])
            assert err['db_accumulated'] < wb_bound, ('db +=', err['db_accumulated'], wb_bound)
        for key, (got, want) in extra.items():
            err[key + '_entry'] = gpu_util.rel_err(got, want)
            b = bounds['dx'][0] if key.startswith('dx') else wb_bound
            assert err[key + '_entry'] < b, (key, err[key + '_entry'], b)
        return report
    finally:
        ops.set_precision('f32')
        for k, v in prev_tuning.items():
            L.set_tuning(k, v)


def _params():
    return [pytest.param(r, m, id='%s-%s' % (r.id, m.replace(':', '_'))) for r in ROWS for m in r.modes]


@pytest.mark.parametrize('r,mode', _params())
def test_conv_route(r, mode):
    check_row(r, mode)


def _claimed(targets):
    out = set()
    for t in targets:
        out.update(t.values() if isinstance(t, dict) else ([t] if t else []))
    return out


def test_every_backward_route_has_a_row():
    """Every weight-gradient and data-gradient id of the library's route table is claimed by a row above or listed, with its reason,
    in NOT_PINNED_HERE: no weight-gradient route may be, and at most one data-gradient route in five."""
    from hoig_amd import _lib as L
    names = L.route_names()
    assert names[0] == 'none' and len(set(names)) == len(names)
    wgrad = {n for n in names if n.startswith('wgrad_')}
    dgrad = {n for n in names if n.startswith('dgrad_')}
    assert len(wgrad) >= 20 and len(dgrad) >= 40, 'the route table lost its ids'
    claimed_w, claimed_d = _claimed(r.wgrad for r in ROWS), _claimed(r.dgrad for r in ROWS)
    assert ROWS and len({r.id for r in ROWS}) == len(ROWS)
    assert claimed_w <= wgrad and claimed_d <= dgrad, 'a row names a route the library does not have: %r' % sorted(
        (claimed_w - wgrad) | (claimed_d - dgrad))
    assert all(isinstance(v, str) and v for v in NOT_PINNED_HERE.values())
    assert set(NOT_PINNED_HERE) <= wgrad | dgrad
    assert not set(NOT_PINNED_HERE) & (claimed_w | claimed_d), 'listed as not pinned, yet a row claims it'
    missing = (wgrad | dgrad) - claimed_w - claimed_d - set(NOT_PINNED_HERE)
    assert not missing, 'routes without a row and without a reason: %r' % sorted(missing)
    assert not set(NOT_PINNED_HERE) & wgrad, 'every weight-gradient route is pinned here'
    assert 5 * len(set(NOT_PINNED_HERE) & dgrad) <= len(dgrad)


def test_every_forward_route_has_a_row():
    """Every forward id of the library's route table is claimed by a row above, or asserted by the test ASSERTED_ELSEWHERE names (whose
    file must hold the route's name), or listed in NOT_PINNED_HERE with the dispatcher condition that shadows it: at most 3 of them."""
    import os
    import re
    from hoig_amd import _lib as L
    fwd = {n for n in L.route_names() if n.startswith('fwd_')}
    assert len(fwd) >= 58, 'the route table lost its ids'
    claimed = _claimed(r.fwd for r in ROWS)
    assert claimed <= fwd, 'a row names a route the library does not have: %r' % sorted(claimed - fwd)
    assert set(ASSERTED_ELSEWHERE) <= fwd
    assert not set(ASSERTED_ELSEWHERE) & claimed, 'listed as asserted elsewhere, yet a row claims it'
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for route, where in ASSERTED_ELSEWHERE.items():
        path, name = where.split('::')
        with open(os.path.join(root, path)) as f:
            text = f.read()
        assert re.search(r'^def %s\(' % re.escape(name), text, re.M), '%s has no %s' % (path, name)
        assert "'%s'" % route in text, '%s does not name %s' % (path, route)
    shadowed = set(NOT_PINNED_HERE) & fwd
    assert not shadowed & (claimed | set(ASSERTED_ELSEWHERE)), 'listed as not pinned, yet asserted'
    missing = fwd - claimed - set(ASSERTED_ELSEWHERE) - shadowed
    assert not missing, 'forward routes without a row and without a reason: %r' % sorted(missing)
    assert len(shadowed) <= 3
