"""tests/conv_reference.py against torch's own convolutions in float64, and its rounding emulation against the project's bounds."""
import pytest
import torch
import torch.nn.functional as F

import conv_reference as R
from test_ops_gpu import PREC_BOUNDS

# one case per kind: stride 1, stride 2, transposed, valid 5x5, 4x4 pad 1, 1x1
CASES = {
    'stride1': R.Case(2, 12, 20, 6, 9, 3, 1, 1, False, True, seed=1),
    'stride2': R.Case(2, 8, 16, 8, 10, 3, 2, 1, False, True, seed=2),
    'transposed': R.Case(2, 16, 8, 4, 5, 3, 2, 1, True, False, seed=3),
    'valid5x5': R.Case(2, 8, 16, 9, 11, 5, 1, 0, False, True, seed=4),
    '4x4pad1': R.Case(2, 6, 16, 9, 9, 4, 1, 1, False, True, seed=5),
    '4x4s2': R.Case(2, 6, 16, 10, 8, 4, 2, 1, False, True, seed=6),
    '1x1': R.Case(2, 24, 10, 5, 7, 1, 1, 0, False, True, seed=7),
}


def _torch_autograd(c, x, w, b, gy, act='none'):
    xr = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if b is not None else None
    if c.transposed:
        y = F.conv_transpose2d(xr, wr, br, stride=c.stride, padding=c.pad, output_padding=c.stride - 1)
    else:
        y = F.conv2d(xr, wr, br, stride=c.stride, padding=c.pad)
    y = R.ACTS[act](y, c.slope)
    y.backward(gy.double().permute(0, 3, 1, 2))
    return (y.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1), wr.grad, br.grad if br is not None else None)


def _close(a, b):
    return (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item())


@pytest.mark.parametrize('name', sorted(CASES))
@pytest.mark.parametrize('act', ['none', 'tanh', 'lrelu'])
def test_reference_agrees_with_torch_autograd_in_float64(name, act):
    c = CASES[name]
    x, w, b, gy = R.make_case(c)
    assert tuple(gy.shape[1:3]) == R.out_hw(c)
    y, dx, dw, db = _torch_autograd(c, x, w, b, gy, act)
    assert _close(R.conv_ref(x, w, b, c.stride, c.pad, c.transposed, act, c.slope), y)
    rdx, rdw, rdb = R.conv_grads_ref(x, w, b, gy, c.stride, c.pad, c.transposed, act, c.slope)
    assert rdx.dtype == rdw.dtype == torch.float64
    assert _close(rdx, dx) and _close(rdw, dw)
    assert (rdb is None) == (db is None)
    if db is not None:
        assert _close(rdb, db)


def test_reference_takes_a_packed_weight():
    """A weight laid over packed [Co][R][S][Ci] storage (ops.pack_weight's strides) is read by its logical shape."""
    c = CASES['stride1']
    x, w, b, gy = R.make_case(c)
    packed = torch.empty_strided(tuple(w.shape), (c.k * c.k * c.Ci, 1, c.k * c.Ci, c.Ci))
    packed.copy_(w)
    assert torch.equal(R.conv_ref(x, packed, b, 1, 1), R.conv_ref(x, w, b, 1, 1))


@pytest.mark.parametrize('name', sorted(CASES))
def test_rounded_operand_error_is_nonzero_and_inside_the_two_term_bounds(name):
    c = CASES[name]
    e2 = R.rounded_operand_error(c, 'f16x2')
    e3 = R.rounded_operand_error(c, 'bf16x3')
    e1 = R.rounded_operand_error(c, 'bf16')
    mixed = R.rounded_operand_error(c, 'bf16x3:f16x2')
    for key, bound in zip(('y', 'dx', 'dw'), PREC_BOUNDS['f16x2']):
        assert 0.0 < e2[key] < bound, (key, e2[key], bound)
        assert 0.0 < e3[key] < e2[key] < e1[key], (key, e3[key], e2[key], e1[key])      # more terms, less error
    for key, bound in zip(('y', 'dx', 'dw'), PREC_BOUNDS['bf16x3']):
        assert e3[key] < bound
    assert mixed['y'] == e3['y'] and mixed['dx'] == e2['dx'] and mixed['dw'] == e2['dw']


def test_rounded_operand_error_is_a_function_of_the_reference_alone():
    c = CASES['4x4s2']
    assert R.rounded_operand_error(c, 'f16x2') == R.rounded_operand_error(c, 'f16x2')
    x, w, b, gy = R.make_case(c)
    assert R.rounded_operand_error((x, w, b, gy, c.stride, c.pad, c.transposed), 'f16x2') == R.rounded_operand_error(c, 'f16x2')
