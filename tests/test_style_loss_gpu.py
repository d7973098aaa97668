"""The opt-in style (Gram-matrix) term of G on the device (docs/style_loss.md): the kernels against the CPU twin, bit for bit
(tests/test_style_loss_cpu.py pins the twin against float64); the autograd function against torch autograd in float64; the Trainer's
opt.lambda_style in the eager and the captured step; and the defaults, which are the parent's."""
import gc
import os

import numpy as np
import pytest
import torch

import style_loss_reference as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GEN, BATCH, SIDE = 'generator_spade_attn', 2, 64
_ids = lambda v: 'x'.join(str(s) for s in v)


# ------------------------------------------------------------------------------------------------ kernels against the twin
@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'raw'])
@pytest.mark.parametrize('shape', R.SHAPES, ids=_ids)
def test_kernels_equal_the_twin_bit_for_bit(shape, relu):
    """The fp64 Gram matrices (so the chunk partials' sums), S, both slots and dFx.  This rests on the fp32 MFMA being a k-ordered fma
    chain from the accumulator it is given."""
    x, y = R.case(shape, relu=relu)
    dev, cpu = R.run(DEV, x, y, init=0.5), R.run('cpu', x, y, init=0.5)
    diff = np.abs(dev['gram'] - cpu['gram'])
    print('style_loss gram %s %s: %d of %d entries differ, by at most %.3e' % (_ids(shape), 'relu' if relu else 'raw',
                                                                             int((diff != 0).sum()), diff.size, float(diff.max())))
    assert dev['gram'].tobytes() == cpu['gram'].tobytes()
    assert R.same_bits(dev, cpu)
    assert R.dfeat(DEV, x, cpu['S']).tobytes() == R.dfeat('cpu', x, cpu['S']).tobytes()
    none = R.run(DEV, x, y, scale=2.5, term=False, report=False, gram=False)
    assert R.same_bits(none, R.run('cpu', x, y, scale=2.5, term=False, report=False, gram=False))


def test_identical_inputs_and_a_nan_on_the_device():
    x, y = R.case((3, 7, 11, R.T + 16))
    got = R.run(DEV, x, x.copy())
    assert got['term'][0] == 0.0 and got['report'][0] == 0.0 and got['S'].tobytes() == bytes(got['S'].nbytes)
    x[1, 2, 3, 7] = np.nan                   # (a NaN's payload is not pinned)
    dev, cpu = R.run(DEV, x, y), R.run('cpu', x, y)
    assert np.isnan(dev['term'][0]) and np.isnan(dev['report'][0]) and dev['S'].tobytes() == cpu['S'].tobytes()
    assert np.isfinite(dev['S']).all() and not dev['S'][1, 7].any() and dev['S'][1].any()


def test_entry_points_refuse_and_write_nothing():
    from hoig_amd import _lib as L
    N, P, C = 2, 9, 32
    fx, fy = torch.ones(N, P, C, device=DEV), torch.zeros(N, P, C, device=DEV)
    S, d = torch.full((N, C, C), 7.0, device=DEV), torch.full((N, P, C), 7.0, device=DEV)
    slot = torch.full((4,), 7.0, device=DEV)
    need = L.lib.hoig_style_workspace_bytes(N, P, C)
    ws = torch.zeros(need // 8 + 2, dtype=torch.float64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    good = [fx.data_ptr(), fy.data_ptr(), N, P, C, 1.0, S.data_ptr(), slot.data_ptr(), slot.data_ptr() + 4, None, ws.data_ptr(), need, st]
    for i, v, rc in ((0, None, L.EINVAL), (6, None, L.EINVAL), (6, S.data_ptr() + 8, L.EINVAL), (6, fx.data_ptr(), L.EINVAL),
                     (5, float('nan'), L.EINVAL), (2, 0, L.EINVAL), (10, None, L.EINVAL), (10, ws.data_ptr() + 8, L.EINVAL),
                     (11, need - 8, L.EINVAL), (2, 4097, L.EUNSUPPORTED), (3, 2 ** 22 + 1, L.EUNSUPPORTED), (4, 24, L.EUNSUPPORTED),
                     (4, 528, L.EUNSUPPORTED)):
        bad = list(good)
        bad[i] = v
        assert L.lib.hoig_style_gram(*bad) == rc, (i, v)
    good_d = [fx.data_ptr(), S.data_ptr(), N, P, C, d.data_ptr(), st]
    for i, v, rc in ((0, None, L.EINVAL), (5, None, L.EINVAL), (5, fx.data_ptr(), L.EINVAL), (5, d.data_ptr() + 4, L.EINVAL),
                     (2, 0, L.EINVAL), (4, 40, L.EUNSUPPORTED), (3, 2 ** 22 + 1, L.EUNSUPPORTED)):
        bad = list(good_d)
        bad[i] = v
        assert L.lib.hoig_style_dfeat(*bad) == rc, (i, v)
    torch.cuda.synchronize()
    assert bool((S == 7.0).all()) and bool((slot == 7.0).all()) and bool((d == 7.0).all())
    assert L.lib.hoig_style_gram(*good) == L.OK and L.lib.hoig_style_dfeat(*good_d) == L.OK
    torch.cuda.synchronize()
    c = R.coeff((N, 1, P, C), 1.0)
    row = np.float32(0.0)
    for _ in range(C):                       # (the chain of one element: fma(1, c, acc), C times)
        row = np.float32(row + c)
    assert slot.tolist() == [7.0 + 1.0 / C, 7.0 + 1.0 / C, 7.0, 7.0] and bool((S == float(c)).all()) and bool((d == float(row)).all())


# ------------------------------------------------------------------------------------------------ the autograd function
def _torch_term(fx, fy, scale):
    """Section 1 in torch float64 -> scale L"""
    N, H, W, C = fx.shape
    gram = lambda f: torch.matmul(f.reshape(N, H * W, C).transpose(1, 2), f.reshape(N, H * W, C)) / (C * H * W)
    return scale * (gram(fx) - gram(fy)).abs().sum() / (N * C * C)


def test_the_autograd_function_against_torch_autograd_in_float64():
    from hoig_amd import ops
    from hoig_amd import style_loss as SL
    shape = (3, 7, 11, R.T + 16)
    x, y = R.case(shape, seed=5)
    want = R.reference(x, y)
    slots = ops.LossSlots(['g_tsf', 'g_style'], DEV, extra=['raw'])
    tx, ty = torch.from_numpy(x).to(DEV).requires_grad_(True), torch.from_numpy(y).to(DEV)
    slots.begin()
    a = SL.style_loss(tx, ty, R.SCALE, slots.term('g_style'), slots.term('raw'))
    b = SL.style_loss(tx, ty, R.SCALE, slots.term('g_style'))
    slots.total(a, b).backward()
    torch.cuda.synchronize()
    x64 = tx.detach().double().requires_grad_(True)
    (2 * _torch_term(x64, ty.double(), R.SCALE)).backward()
    auto = x64.grad.cpu().numpy()
    S_ref = (want['sign'] * float(want['c'])).astype(np.float32)
    # torch's gradient is the reference's up to float64 rounding and c's one fp32 rounding, outside the entries whose sign is not
    # settled (torch takes its own there)
    assert (np.abs(auto - 2 * R.grad_reference(x, want)) <= 2 * R.grad_bound(x, S_ref, want['amb'])).all()
    # each call's gradient is within the bound of its own; autograd adds the two in one more fp32 add
    got = tx.grad.cpu().numpy().astype(np.float64)
    assert (np.abs(got - auto) <= 2 * R.grad_bound(x, S_ref, want['amb']) + R.u * np.abs(auto)).all()
    once = R.run('cpu', x, y)
    assert float(slots.value('g_style')) == float(once['term'][0] + once['term'][0]) and float(slots.value('raw')) == float(once['report'][0])
    assert float(slots.value('g_tsf')) == 0.0
    # no gradient wanted: no gradient launch
    called = []
    real = SL.dfeat
    SL.dfeat = lambda *a: (called.append(1), real(*a))[1]
    try:
        w = torch.ones((), device=DEV, requires_grad=True)
        (SL.style_loss(tx.detach(), ty, R.SCALE, slots.term('g_style')) * w).backward()
    finally:
        SL.dfeat = real
    assert not called


# ------------------------------------------------------------------------------------------------ Trainer
ON = dict(lambda_style=10)
_BUILT = []


def _trainer(**over):
    from common import product_trainer
    m = product_trainer(GEN, BATCH, SIDE, **over)
    _BUILT.append(m)
    return m


@pytest.fixture(autouse=True)
def _models_leave_with_their_test():
    """Every model built here is closed, and collected, when its test ends (as in tests/test_region_loss_gpu.py)."""
    yield
    while _BUILT:
        m = _BUILT.pop()
        torch.cuda.synchronize()
        m.close()
        del m
    gc.collect()


def _settle(m):
    m._wait_g()
    m._wait_d()
    torch.cuda.synchronize()


def _tap_style(monkeypatch):
    """Every call of style_loss leaves its features and scale, and (in an eager step) the gradient that the term hands back to autograd,
    in the list that is returned: the features go in through an alias of their own, so what arrives at the alias is this term's
    contribution alone -- the gradient entering the level with the option on minus off.  (Inside a capture the copies become part of the
    graph: every replay refreshes them.)"""
    from hoig_amd import style_loss as SL
    calls = []
    real = SL.style_loss

    def style_loss(fx, fy, scale, into, into_raw=None):
        alias, rec = fx.view_as(fx), dict(fx=fx.detach().clone(), fy=fy.detach().clone(), scale=scale)
        if alias.requires_grad and not torch.cuda.is_current_stream_capturing():
            alias.register_hook(lambda g: rec.__setitem__('grad', g.detach().clone()))
        calls.append(rec)
        return real(alias, fy, scale, into, into_raw)

    monkeypatch.setattr(SL, 'style_loss', style_loss)
    return calls


def _check_step(m, calls, grads):
    """The step's g_style against the float64 reference on the captured features of the last four calls, within the summed bound; with
    `grads`, every level's gradient against the reference's.  -> g_style"""
    sc, errs = m.get_current_scalars(), m.get_current_errors()
    assert list(sc) == ['lr_G', 'lr_D', 'g_style'] and all(np.isfinite(v) for v in sc.values())
    assert list(errs) == ['g_rec', 'g_tsf', 'g_adv', 'g_mask', 'g_mask_smooth', 'd_real', 'd_fake'] and all(np.isfinite(v) for v in errs.values())
    total, bound = 0.0, 0.0
    assert [tuple(c['fx'].shape[1:]) for c in calls[-4:]] == [(32, 32, 128), (16, 16, 256), (8, 8, 512), (4, 4, 512)]
    for c in calls[-4:]:
        x, y = c['fx'].cpu().numpy(), c['fy'].cpu().numpy()
        assert c['scale'] == 10.0 and c['fx'].shape[0] == BATCH
        want = R.reference(x, y, c['scale'])
        total += want['term']
        bound += c['scale'] * want['vbound'] + R.u * want['term']
        if grads:
            S_ref = (want['sign'] * float(want['c'])).astype(np.float32)
            g = c['grad'].cpu().numpy()
            assert np.isfinite(g).all() and g.any()
            assert (np.abs(g - R.grad_reference(x, want)) <= R.grad_bound(x, S_ref, want['amb'])).all()
    assert total > 0 and abs(sc['g_style'] - total) <= bound + 4 * R.u * total, (sc['g_style'], total, bound)
    return sc['g_style']


@pytest.mark.parametrize('how', ['eager', 'eager_d_late', 'unforked'])
def test_trainer_step_with_the_style_term(how, monkeypatch):
    """'eager': the D step beside G's backward ('d_early'); 'eager_d_late': behind it; 'unforked': every chain on the caller's stream
    (what HOIG_STREAMS=0 selects)."""
    from hoig_amd import _lib as L
    from hoig_amd import ops
    from hoig_amd.models.networks import generator as G
    if how == 'unforked':
        monkeypatch.setattr(G, '_FORK_STREAMS', False)
        monkeypatch.setattr(ops, '_WGRAD_SIDE', False)
    prev = L.set_tuning('d_early', 0 if how == 'eager_d_late' else 1)
    try:
        m = _trainer(**ON)
        assert m._style is not None and m._g_terms.names[-1] == 'g_style'
        calls = _tap_style(monkeypatch)
        pG = next(m._net(m._G).parameters()).detach().clone()
        pD = next(m._net(m._D).parameters()).detach().clone()
        m.optimize_parameters()
        _settle(m)
        for net, before in ((m._G, pG), (m._D, pD)):         # both networks moved, and nothing went non-finite
            after = next(m._net(net).parameters()).detach()
            assert bool(torch.isfinite(after).all()) and not torch.equal(after, before)
        assert len(calls) == 4
        _check_step(m, calls, grads=True)
    finally:
        L.set_tuning('d_early', prev)


def test_the_captured_step_follows_each_batchs_features(monkeypatch):
    from common import SEEDS
    from hoig_amd import synthetic
    m = _trainer(hip_graph=True, **ON)
    calls = _tap_style(monkeypatch)
    batches = [synthetic.make_inputs(BATCH, SIDE, seed=SEEDS['inputs']), synthetic.make_inputs(BATCH, SIDE, seed=77)]
    seen = []
    for k in (0, 0, 0, 1, 0, 1):                     # two eager steps, the capture and its replay, then replays on two batches in turn
        m.set_input(batches[k])
        m.optimize_parameters()
        _settle(m)
        seen.append((k, _check_step(m, calls, grads=False), len(calls)))
    assert any(g['graphs'] is not None for g in m._graphs.values()), 'the step was never captured'
    assert seen[-1][2] == seen[-3][2]                # (the replays call nothing: their copies are refreshed by the graph)
    a, b = seen[-2], seen[-1]
    assert a[0] != b[0] and a[1] != b[1]             # (each replay against its own batch's reference)
    assert bool(torch.isfinite(next(m._net(m._G).parameters())).all())


def test_trainer_with_the_defaults_is_the_parents(monkeypatch, tmp_path):
    from hoig_amd import _lib as L
    called = []
    real_call, real_attempt = L.call, L.attempt
    monkeypatch.setattr(L, 'call', lambda name, *a: (called.append(name), real_call(name, *a))[1])
    monkeypatch.setattr(L, 'attempt', lambda name, *a: (called.append(name), real_attempt(name, *a))[1])
    m = _trainer(checkpoints_dir=str(tmp_path))
    assert m._style is None and m._g_terms.names == ['g_adv', 'g_rec', 'g_tsf', 'g_mask', 'g_mask_smooth'] and m._g_terms.extra == []
    del called[:]
    m.optimize_parameters()
    _settle(m)
    default = list(called)
    m.save(1)
    assert default and not [n for n in called if n.startswith('hoig_style')]
    assert list(m.get_current_scalars()) == ['lr_G', 'lr_D']
    assert list(m.get_current_errors()) == ['g_rec', 'g_tsf', 'g_adv', 'g_mask', 'g_mask_smooth', 'd_real', 'd_fake']
    assert sorted(os.listdir(os.path.join(str(tmp_path), 't'))) == sorted(
        '%s_epoch_1_id_%s.pth' % (kind, tag) for kind in ('net', 'opt') for tag in 'GD')
    # ... and with the option on: four Gram calls and four gradient calls more, every loss launch as before, the same files
    # (the first model goes before the second comes, as in tests/test_region_loss_gpu.py)
    _BUILT.remove(m)
    m.close()
    del m
    gc.collect()
    h = _trainer(checkpoints_dir=str(tmp_path / 'on'), **ON)
    del called[:]
    h.optimize_parameters()
    _settle(h)
    on = list(called)
    assert on.count('hoig_style_gram') == 4 and on.count('hoig_style_dfeat') == 4
    for name in ('hoig_loss_accumulate', 'hoig_tv_accumulate', 'hoig_sum', 'hoig_sum_scaled', 'hoig_loss_fwd_bwd'):
        assert on.count(name) == default.count(name), (name, on.count(name), default.count(name))
    h.save(1)
    assert sorted(os.listdir(os.path.join(str(tmp_path / 'on'), 't'))) == sorted(os.listdir(os.path.join(str(tmp_path), 't')))


def test_trainer_refuses_bad_options():
    from common import opt_namespace
    from hoig_amd.models import ModelsFactory
    with pytest.raises(ValueError, match='lambda_style'):
        ModelsFactory.get_by_name('trainer', opt_namespace(lambda_style=-1))
    with pytest.raises(ValueError, match='style_levels'):
        ModelsFactory.get_by_name('trainer', opt_namespace(lambda_style=1, style_levels='0'))
