"""float64 CPU reference of the convolution layer (forward and the three gradients) and a CPU emulation of what each 16-bit
arithmetic mode rounds away -- the yardsticks of tests/test_conv_routes_gpu.py and tests/test_conv_composites_gpu.py.

Layouts are the product's: activations NHWC, weights in their LOGICAL shape -- (Co, Ci, R, S), or (Ci, Co, R, S) for a transposed
convolution -- over any strides (a packed weight's .cpu() is fine).  Everything returned is float64, activations NHWC.

The forward is written out here (im2col + one matrix product; a transposed convolution as the stride-1 convolution of the
zero-stuffed input with the flipped kernel) instead of calling F.conv2d, so that tests/test_conv_reference_cpu.py can hold it against
F.conv2d / F.conv_transpose2d; dx and db come from autograd through that forward, dw from torch.nn.grad.conv2d_weight."""
import collections

import torch
import torch.nn.functional as F

ACTS = {
    'none': lambda t, s: t,
    'relu': lambda t, s: torch.relu(t),
    'lrelu': lambda t, s: F.leaky_relu(t, s),
    'tanh': lambda t, s: torch.tanh(t),
    'sigmoid': lambda t, s: torch.sigmoid(t),
}

Case = collections.namedtuple('Case', 'B Ci Co H W k stride pad transposed bias act slope seed')
Case.__new__.__defaults__ = (False, False, 'none', 0.2, 0)


def out_hw(c):
    """Output height / width of case `c` (ConvTranspose2d: output_padding = stride - 1, the product's only use)."""
    if c.transposed:
        return ((c.H - 1) * c.stride - 2 * c.pad + c.k + c.stride - 1, (c.W - 1) * c.stride - 2 * c.pad + c.k + c.stride - 1)
    return ((c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1)


def make_case(c):
    """Seeded Gaussian operands of case `c`, float32 on the CPU: x and gy NHWC, w logical, b or None."""
    g = torch.Generator().manual_seed(1000 + c.seed)
    Ho, Wo = out_hw(c)
    x = torch.randn(c.B, c.H, c.W, c.Ci, generator=g)
    wshape = (c.Ci, c.Co, c.k, c.k) if c.transposed else (c.Co, c.Ci, c.k, c.k)
    w = torch.randn(wshape, generator=g) * (c.Ci * c.k * c.k) ** -0.5
    b = torch.randn(c.Co, generator=g) if c.bias else None
    gy = torch.randn(c.B, Ho, Wo, c.Co, generator=g)
    return x, w, b, gy


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _conv_nchw(x, w, stride, pad):
    """conv2d of NCHW x with (Co, Ci, R, S) w as im2col + matmul."""
    B, Ci, H, W = x.shape
    Co, _, R, S = w.shape
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    cols = F.unfold(x, (R, S), padding=pad, stride=stride)                     # [B, Ci*R*S, Ho*Wo]
    return (w.reshape(Co, -1) @ cols).reshape(B, Co, Ho, Wo)


def _forward(x, w, b, stride, pad, transposed, act, slope, hw):
    """NCHW doubles in, NCHW double out (differentiable)."""
    if not transposed:
        y = _conv_nchw(x, w, stride, pad)
    else:
        B, Ci, H, W = x.shape
        _, Co, R, S = w.shape
        Ho, Wo = hw
        z = x.new_zeros(B, Ci, (H - 1) * stride + 1, (W - 1) * stride + 1)
        z[:, :, ::stride, ::stride] = x
        lo_h, lo_w = R - 1 - pad, S - 1 - pad
        hi_h, hi_w = Ho - (z.shape[2] + lo_h - R + 1), Wo - (z.shape[3] + lo_w - S + 1)     # (output_padding lands here)
        z = F.pad(z, (lo_w, hi_w, lo_h, hi_h))
        y = _conv_nchw(z, w.flip(2, 3).transpose(0, 1), 1, 0)
    if b is not None:
        y = y + b.view(1, -1, 1, 1)
    return ACTS[act](y, slope)


def _hw(x, w, stride, pad, transposed, hw):
    if hw is not None or not transposed:
        return hw
    R, S = w.shape[2], w.shape[3]
    return ((x.shape[1] - 1) * stride - 2 * pad + R + stride - 1, (x.shape[2] - 1) * stride - 2 * pad + S + stride - 1)


def conv_ref(x, w, b=None, stride=1, pad=0, transposed=False, act='none', slope=0.2, hw=None):
    """-> y (NHWC float64).  hw: the output size of a transposed convolution (default: output_padding = stride - 1)."""
    with torch.no_grad():
        return _nhwc(_forward(_nchw(x.double()), w.double(), None if b is None else b.double(), stride, pad, transposed, act, slope,
                              _hw(x, w, stride, pad, transposed, hw)))


def conv_grads_ref(x, w, b, gy, stride=1, pad=0, transposed=False, act='none', slope=0.2, hw=None):
    """-> (dx NHWC, dw in w's logical shape, db or None), float64: the gradients of sum(y * gy)."""
    xd = _nchw(x.double()).contiguous().requires_grad_(True)
    wd = w.double().contiguous()
    bd = None if b is None else b.double().requires_grad_(True)
    pre = _forward(xd, wd, bd, stride, pad, transposed, 'none', slope, _hw(x, w, stride, pad, transposed, hw))
    y = ACTS[act](pre, slope)
    g = _nchw(gy.double())
    ins = [xd, pre] + ([bd] if bd is not None else [])
    grads = torch.autograd.grad(y, ins, g)
    dx, dpre = grads[0], grads[1].contiguous()
    db = grads[2] if bd is not None else None
    if not transposed:
        dw = torch.nn.grad.conv2d_weight(xd.detach(), wd.shape, dpre, stride=stride, padding=pad)
    else:           # conv_transpose2d is the adjoint of conv2d with the same (Ci, Co, R, S) weight: x and dy swap roles
        dw = torch.nn.grad.conv2d_weight(dpre, wd.shape, xd.detach(), stride=stride, padding=pad)
    return _nhwc(dx), dw, db


# ---- what an arithmetic mode rounds away (the comment on PREC_BOUNDS in tests/test_ops_gpu.py).
# A k-step multiplies 16-bit TERMS of the two operands -- fp16 in the forward (weights scaled by 2^8), bf16 in the backward:
#   bf16x3   both operands as hi + lo, the lo * lo product dropped
#   f16x2    the gathered operand (x forward, dy backward) as hi + lo, the other one as ONE term: the weight in the forward and in the
#            data gradient, x in the weight gradient
#   bf16     one term each
def _terms(t, n, dtype, scale=1.0):
    """(hi, lo) of t as the kernels split it; lo is zero with n == 1."""
    t = t.double() * scale
    hi = t.to(torch.float32).to(dtype).double()
    lo = (t - hi).to(torch.float32).to(dtype).double() if n == 2 else torch.zeros_like(hi)
    return hi / scale, lo / scale


_PASS_MODE = {'bf16x3': (2, 2), 'f16x2': (2, 1), 'bf16': (1, 1)}          # terms of (gathered operand, other operand)


def _mode_of_pass(mode, which):
    parts = mode.split(':')
    fwd, dg = parts[0], parts[1] if len(parts) > 1 else parts[0]
    return {'y': fwd, 'dx': dg, 'dw': parts[2] if len(parts) > 2 else dg}[which]


def _relerr(a, ref):
    return ((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def rounded_operand_error(case, mode, passes=('y', 'dx', 'dw')):
    """{'y', 'dx', 'dw'} -> the max-norm relative error that `mode`'s operand rounding alone leaves in each pass of `case` (a Case, or
    the (x, w, b, gy, stride, pad, transposed) operands themselves), against the unrounded float64 reference.  Exact accumulation:
    this is the arithmetic's own error, computed from the reference alone -- a kernel's error is compared WITH it, never used for it.
    passes=('y',): the forward alone (the gradients' float64 references are the expensive part; gy may then be None)."""
    if isinstance(case, Case):
        x, w, b, gy = make_case(case)
        stride, pad, transposed = case.stride, case.pad, case.transposed
    else:
        x, w, b, gy, stride, pad, transposed = case
    y0 = conv_ref(x, w, None, stride, pad, transposed)
    hw = tuple(y0.shape[1:3])
    out = {}
    # forward: x gathered, w the other operand; fp16 terms, weight planes hold fp16(2^8 w)
    ng, no = _PASS_MODE[_mode_of_pass(mode, 'y')]
    (xh, xl), (wh, wl) = _terms(x, ng, torch.float16), _terms(w, no, torch.float16, 256.0)
    y = conv_ref(xh + xl, wh + wl, None, stride, pad, transposed, hw=hw)
    if ng == 2 and no == 2:
        y = y - conv_ref(xl, wl, None, stride, pad, transposed, hw=hw)
    out['y'] = _relerr(y, y0)
    if 'dx' not in passes and 'dw' not in passes:          # (a forward-only caller: gy may be None)
        return out
    dx0, dw0, _ = conv_grads_ref(x, w, None, gy, stride, pad, transposed)
    # data gradient: dy gathered, w the other operand; bf16 terms
    ng, no = _PASS_MODE[_mode_of_pass(mode, 'dx')]
    (gh, gl), (wh, wl) = _terms(gy, ng, torch.bfloat16), _terms(w, no, torch.bfloat16)
    dx = conv_grads_ref(x, wh + wl, None, gh + gl, stride, pad, transposed, hw=hw)[0]
    if ng == 2 and no == 2:
        dx = dx - conv_grads_ref(x, wl, None, gl, stride, pad, transposed, hw=hw)[0]
    out['dx'] = _relerr(dx, dx0)
    # weight gradient: dy gathered, x the other operand; bf16 terms
    ng, no = _PASS_MODE[_mode_of_pass(mode, 'dw')]
    (gh, gl), (xh, xl) = _terms(gy, ng, torch.bfloat16), _terms(x, no, torch.bfloat16)
    dw = conv_grads_ref(xh + xl, w, None, gh + gl, stride, pad, transposed, hw=hw)[1]
    if ng == 2 and no == 2:
        dw = dw - conv_grads_ref(xl, w, None, gl, stride, pad, transposed, hw=hw)[1]
    out['dw'] = _relerr(dw, dw0)
    return out
