"""The 2-D-tiled valid 5x5 kernels for the attention's wide maps (tuning key 'halo5'; forward and data gradient: hoig_amd/csrc/
conv_halo5.hip, weight gradient: wgrad_tile5_kernel in wgrad_flat.hip) against a float64 convolution and its autograd on the CPU, and
against the path the key replaces (key 0: the generic kernels) on the same inputs.

The weight-gradient kernel takes every such layer with Wi > 67, with the bias gradient where the caller passes one (Wo % 32 == 0 and an
even Ho) and without.
The forward / data-gradient kernel serves a launch whose output channels are a multiple of 128 (forward: Co; data gradient: Ci) on a map too wide for the
flattened-axis kernel (Wi > 52 or so); with few tiles and neither addend nor activation it splits K over blockIdx.y (atomic epilogue),
which key 2 turns off -- so every case runs under keys 0, 1 and 2, and between them the cases put both epilogues on partial tiles, image
boundaries and several channel blocks."""
import functools

import pytest
import torch
import torch.nn.functional as F

from gpu_util import nhwc_cuda, nchw_cpu
from test_ops_gpu import PREC_BOUNDS

pytestmark = pytest.mark.gpu

CASES = [
    # B, Ci, Co, Hi, Wi, bias, addend                 what the launches are
    (1, 64, 128, 21, 136, True, False),       # fwd 17 x 132: 2 x 9 partial tiles, two channel blocks
    (2, 32, 128, 20, 72, False, True),        # fwd 16 x 68 x two images, one channel block (never split)
    (1, 96, 128, 37, 68, True, True),         # fwd 33 x 64: three tile rows, three channel blocks
    (2, 64, 256, 24, 132, False, False),      # fwd 20 x 128, two channel tiles x two images
    (1, 128, 128, 9, 72, True, False),        # five tiles: fwd and dgrad (9 x 72 canvas, 5-row source) both take the split-K epilogue
    (2, 128, 64, 20, 136, False, True),       # dgrad with an addend over two images: 2 x 9 partial tiles, two channel blocks of dy
    (1, 256, 128, 21, 68, True, False),       # dgrad with two channel tiles, four channel blocks of dy
    (2, 64, 128, 12, 68, True, False),        # wgrad where the 2 x 32-pixel halo kernel could run (8 x 64 outputs): dbias from the tiled kernel
]


def _err(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max()).item()


@functools.lru_cache(maxsize=None)
def _reference(B, Ci, Co, Hi, Wi, bias, addend):
    """Inputs (fp32) and the float64 results; computed once per case, read-only."""
    g = torch.Generator().manual_seed(41)
    x = torch.randn(B, Ci, Hi, Wi, generator=g)
    w = torch.randn(Co, Ci, 5, 5, generator=g) * 0.03
    b = torch.randn(Co, generator=g) if bias else None
    gy = torch.randn(B, Co, Hi - 4, Wi - 4, generator=g)
    ad = torch.randn(B, Ci, Hi, Wi, generator=g) if addend else None
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if bias else None
    yr = F.conv2d(xr, wr, br)
    loss = (yr * gy.double()).sum()
    if addend:
        loss = loss + (xr * ad.double()).sum()
    loss.backward()
    return dict(x=x, w=w, b=b, gy=gy, ad=ad, y=yr.detach(), dx=xr.grad, dw=wr.grad, db=br.grad if bias else None)


def _run(L, ops, ref, mode, key):
    prec = {'bf16x3': L.PREC_BF16X3, 'f16x2': L.PREC_F16X2}[mode]
    prev = L.set_tuning('halo5', key)
    ops.set_precision(mode)
    try:
        xd = nhwc_cuda(ref['x']).requires_grad_(True)
        wd = ops.pack_weight(ref['w'].cuda()).requires_grad_(True)
        bd = ref['b'].cuda().requires_grad_(True) if ref['b'] is not None else None
        if ref['ad'] is not None:
            y, x2 = ops.conv2d_fork(xd, wd, bd, 1, 0, prec=prec)
            ((y * nhwc_cuda(ref['gy'])).sum() + (x2 * nhwc_cuda(ref['ad'])).sum()).backward()
        else:
            y = ops.conv2d(xd, wd, bd, 1, 0, prec=prec)
            y.backward(nhwc_cuda(ref['gy']))
        torch.cuda.synchronize()
    finally:
        ops.set_precision('f32')
        L.set_tuning('halo5', prev)
    return nchw_cpu(y), nchw_cpu(xd.grad), wd.grad.detach().cpu(), (bd.grad.detach().cpu() if bd is not None else None)


@pytest.mark.parametrize('mode', ['bf16x3', 'f16x2'])
@pytest.mark.parametrize('B,Ci,Co,Hi,Wi,bias,addend', CASES)
def test_halo5_against_float64_and_the_generic_path(B, Ci, Co, Hi, Wi, bias, addend, mode):
    """Forward, data gradient (zero border, with and without an addend), weight and bias gradient within PREC_BOUNDS of float64; and the
    error of the new path (key 1) at most 25 % above the error of the path it replaces (key 0).  Both sum the same products in fp32 and
    differ in the order only; the 25 % is slack for that.  Key 2 (no split over K) is held to PREC_BOUNDS alone: at these sizes key 0
    and key 1 add up to a dozen partial sums per output with atomics, and one unbroken fp32 chain of a three-term forward rounds up to
    four times coarser than that (9.0e-7 against 2.3e-7 at 21 x 136 x 64) -- the chain length, which at the step's own sizes (hundreds
    of tiles, no split) is the same on every path.

    The fp32 rounding of a three-term forward grows about linearly with the number of MFMAs chained into one accumulator (2.3e-7 /
    4.2e-7 / 9.0-10.9e-7 at 25 / 40 / 162 of them), so the relative bound holds where a launch of few tiles is split over K as finely
    here as on the generic path: launch_halo5_m16 keeps that kernel's minimum of 8 k-blocks per split and, at 64 tiles or fewer, lets
    the splits fill two rounds of workgroups to reach it (the forward of (2, 64, 256, 24, 132): 64 tiles, six splits of nine taps on
    both paths; with one round, four splits, it stood at 4.16e-7 against 2.66e-7, with six 2.70e-7 against 2.84e-7).  Measured ratios
    of the three-term forwards, key 1 / key 0: 0.40 .. 1.21; a split launch's own figure moves by some 6 % from run to run with the
    order of its atomics."""
    from hoig_amd import ops, _lib as L
    ref = _reference(B, Ci, Co, Hi, Wi, bias, addend)
    bf, bd, bw = PREC_BOUNDS[mode]
    errs = {}
    for key in (0, 1, 2):
        y, dx, dw, db = _run(L, ops, ref, mode, key)
        errs[key] = (_err(y, ref['y']), _err(dx, ref['dx']), _err(dw, ref['dw']))
        print('halo5=%d %s: fwd %.3e dgrad %.3e wgrad %.3e' % ((key, mode) + errs[key]))
        if bias:
            edb = _err(db, ref['db'])
            print('halo5=%d %s: dbias %.3e' % (key, mode, edb))
            assert edb < bw
    for key in (1, 2):
        ef, ed, ew = errs[key]
        assert ef < bf and ed < bd and ew < bw
    for e_new, e_old, what in zip(errs[1], errs[0], ('forward', 'data gradient', 'weight gradient')):
        assert e_new <= 1.25 * e_old, '%s: %.3e against %.3e on the generic path' % (what, e_new, e_old)


@pytest.mark.parametrize('B,Ci,Co,Hi,Wi,addend', [(2, 32, 128, 12, 40, False), (1, 128, 128, 12, 40, True)])
def test_halo5_key_leaves_the_narrow_layers_where_they_were(B, Ci, Co, Hi, Wi, addend):
    """40-wide maps stay on the flattened-axis kernel: key on and key 0 give the same bits.  (Launches without a split-K epilogue are
    compared -- the forward of one channel block, the data gradient with an addend: atomics of three or more partial sums are not
    ordered on either path.)"""
    from hoig_amd import ops, _lib as L
    ref = _reference(B, Ci, Co, Hi, Wi, False, addend)
    y0, dx0, _, _ = _run(L, ops, ref, 'bf16x3', 0)
    y1, dx1, _, _ = _run(L, ops, ref, 'bf16x3', 1)
    if addend:
        assert torch.equal(dx0, dx1)
    else:
        assert torch.equal(y0, y1)
