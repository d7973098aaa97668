"""tests/adam_reference.py itself, without a GPU: adam64 against torch.optim.Adam on float64 tensors, the guard's skip, and the fp32 twin
against adam64 on the rows that tests/test_adam_gpu.py runs (docs/optimizer_parity.md)."""
import math

import numpy as np
import pytest
import torch

import adam_reference as A

SIZES = [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025]
BIG = 2097152 + 3 * 1024 + 3


@pytest.mark.parametrize('betas', [(0.5, 0.999), (0.9, 0.999)])
@pytest.mark.parametrize('grad_scale', [1.0, 0.5])
def test_adam64_is_torch_adam_in_float64(betas, grad_scale):
    """Five steps; grad_scale is folded into the gradients torch sees.  1e-12 relative, element by element."""
    n = 257
    rng = np.random.RandomState(3)
    p0 = rng.standard_normal(n)
    gs = [A.gradients(n, 40 + k) for k in range(5)]
    tp = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([tp], lr=A.LR, betas=betas, eps=A.EPS)
    p, m, v, step = p0, np.zeros(n), np.zeros(n), 0
    for k, g in enumerate(gs):
        tp.grad = torch.tensor(g.astype(np.float64) * grad_scale)
        before = tp.detach().numpy().copy()
        opt.step()
        p, m, v, upd, step = A.adam64(p, [g], m, v, step, A.LR, betas, A.EPS, grad_scale)
        st = opt.state[tp]
        assert step == k + 1 == int(st['step'])
        for got, want in ((p, tp.detach().numpy()), (m, st['exp_avg'].numpy()), (v, st['exp_avg_sq'].numpy()),
                          (upd[0], before - tp.detach().numpy())):
            if got is upd[0]:       # (torch's update is only known through p: a difference of two O(1) numbers)
                assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want) + 4e-16)
            else:
                assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))
    # ... and the five steps in one call are the five calls
    p5, m5, v5, u5, s5 = A.adam64(p0, gs, np.zeros(n), np.zeros(n), 0, A.LR, betas, A.EPS, grad_scale)
    assert s5 == 5 and np.array_equal(p5, p) and np.array_equal(m5, m) and np.array_equal(v5, v) and len(u5) == 5


@pytest.mark.parametrize('fn', [A.adam64, A.adam32_twin], ids=['adam64', 'twin'])
def test_a_skipped_step_changes_nothing_and_does_not_count(fn):
    n = 37
    rng = np.random.RandomState(5)
    p0, m0, v0 = rng.standard_normal(n), rng.standard_normal(n) * 1e-2, rng.uniform(1e-6, 1e-2, n)
    p0, m0, v0 = (a.astype(np.float32) for a in (p0, m0, v0))
    g = A.gradients(n, 8)
    p, m, v, upd, step = fn(p0, [g], m0, v0, 7, A.LR, (0.5, 0.999), A.EPS, 0.5, guard=(123.0, 1.0))
    assert step == 7 and not upd[0].any()
    for got, want in ((p, p0), (m, m0), (v, v0)):
        assert np.array_equal(got, want.astype(got.dtype))
    # skipped, then taken: the taken step is number 8, with the guard's scale on the gradient
    a = fn(p0, [g, g], m0, v0, 7, A.LR, (0.5, 0.999), A.EPS, 0.5, guard=[(123.0, 1.0), (np.float32(0.37), 0.0)])
    b = fn(p0, [g * np.float32(0.37)], m0, v0, 7, A.LR, (0.5, 0.999), A.EPS, 0.5)
    assert a[4] == b[4] == 8
    for x, y in zip(a[:3], b[:3]):
        assert np.allclose(x, y, rtol=1e-6, atol=0)


def test_derived64():
    d = A.derived64(2e-4, 0.5, 0.999, 1e-8, 3)
    assert d == (2e-4 / (1 - 0.125), 0.5, 0.999, 1.0 - 0.999, 1e-8, math.sqrt(1.0 - 0.999 ** 3))
    big = A.derived64(2e-4, 0.5, 0.999, 1e-8, 100000)
    assert big[0] == 2e-4 and big[5] == 1.0


def test_the_input_check_refuses_subnormal_intermediates():
    g = np.array([1e-21], dtype=np.float32)            # g^2 = 1e-42: a float32 subnormal
    with pytest.raises(AssertionError, match='subnormal'):
        A.adam32_twin(np.zeros(1), [g], np.zeros(1), np.zeros(1), 0, A.LR, (0.5, 0.999), A.EPS)
    A.adam32_twin(np.zeros(1), [g], np.zeros(1), np.zeros(1), 0, A.LR, (0.5, 0.999), A.EPS, check=False)


def _rows():
    out = [(n, kind, gs, gd, betas) for n in SIZES for kind in ('zero', 'randn') for gs, gd in ((1.0, None), (0.5, 0.37))
           for betas in ((0.5, 0.999), (0.9, 0.999))]
    return out + [(BIG, 'zero', 0.5, None, (0.5, 0.999))]


@pytest.mark.parametrize('n,kind,gs,gd,betas', _rows())
def test_the_twin_stays_close_to_adam64(n, kind, gs, gd, betas):
    """1e-5 relative on m, v and the update: a dozen fp32 roundings of at most 6e-8 each come to under 1e-6, and the rows have no
    cancellation (steady signs), so 1e-5 only says that the twin computes Adam.  The rows pass the input check (row_steps runs it), have
    their block of zeros -- m, v and the update exactly 0 there at every step -- and their block where eps dominates."""
    for case in A.row_steps(n, kind, gs, gd, betas):
        (pr, mr, vr, ur), (pt, mt, vt, ut) = case['ref'], case['twin']
        for name, t, r in (('m', mt, mr), ('v', vt, vr), ('update', ut, ur)):
            assert A.zeros_agree(t, r) and A.zeros_agree(r, t)
            assert A.worst_rel(t, r) <= 1e-5, (name, case['step'], A.worst_rel(t, r))
        assert np.all(np.abs(pt - pr) <= 2.0 ** -24 * np.abs(pr) + np.max(np.abs(ut - ur)))
        if n >= 8:
            z = case['g'] == 0
            assert z.sum() >= 2 and not mr[z].any() and not vr[z].any() and not ur[z].any()
            tiny = (np.abs(case['g']) > 0) & (np.abs(case['g']) < 2.1e-9)
            assert tiny.sum() >= 2
            if case['step'] == 1:           # sqrt(v) / sqrt(bc2) = |g'| there: below eps
                assert np.all(np.abs(case['g'][tiny].astype(np.float64)) * gs * (gd or 1.0) < A.EPS)
