"""The opt-in GAN objectives and the LeCam regulariser on the device (docs/gan_objectives.md): the kernels against the CPU twins -- bit
for bit outside the logistic objective, within the derived bound inside it (tests/test_gan_objectives_cpu.py pins the twins) --; the
Trainer's opt.gan_mode and opt.lecam in the eager and the captured step, the checkpoint file, the defaults, and the refusal under a
forced gradient exchange."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import gan_objectives_reference as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GEN, BATCH, SIDE = 'generator_spade_attn', 2, 64
MODES = sorted(R.MODES.items(), key=lambda kv: kv[1])
FORMS = sorted(R.FORMS.items(), key=lambda kv: kv[1])
S, LAM = 0.75, 0.3
_ids = lambda v: v[0] if isinstance(v[0], str) else '%dx%d' % v


def _ab(sizes, seed=0):
    return R.logits(sizes[0], 11 + seed), R.logits(sizes[1], 23 + seed)


def _add(x, y):
    return {k: (x[k] + y[k]) for k in x}


# ------------------------------------------------------------------------------------------------ kernels against twins
@pytest.mark.parametrize('sizes', R.SIZES, ids=_ids)
@pytest.mark.parametrize('mode', MODES[:2], ids=_ids)
def test_d_head_equals_the_twin_bit_for_bit(mode, sizes):
    a, b = _ab(sizes)
    assert R.same_bits(R.run_d(DEV, mode[1], a, b, S, init=0.5), R.run_d('cpu', mode[1], a, b, S, init=0.5))
    for form in FORMS:
        for count in (1, 2):                       # start 2: the regulariser without and with weight
            st = R.new_state(gamma=0.9, start=2, count=count, alpha_r=0.4375, alpha_f=-0.3)
            dev, cpu = R.run_d(DEV, mode[1], a, b, S, LAM, form[1], st), R.run_d('cpu', mode[1], a, b, S, LAM, form[1], st)
            assert R.same_bits(dev, cpu), (form, count)
            assert dev['state']['count'] == count + 1 and (dev['reg'] > 0) == (count == 2)
    st = R.new_state(gamma=0.9, start=2)           # the first tick, null gradients
    assert R.same_bits(R.run_d(DEV, mode[1], a, b, S, LAM, R.PAPER, st, grads=False), R.run_d('cpu', mode[1], a, b, S, LAM, R.PAPER, st, grads=False))


@pytest.mark.parametrize('sizes', R.SIZES, ids=_ids)
@pytest.mark.parametrize('mode', MODES[:2], ids=_ids)
def test_g_head_equals_the_twin_bit_for_bit(mode, sizes):
    b = R.logits(sizes[0], 5)
    assert R.same_bits(R.run_g(DEV, mode[1], b, S, init=0.25), R.run_g('cpu', mode[1], b, S, init=0.25))
    assert R.same_bits(R.run_g(DEV, mode[1], b, S, grads=False), R.run_g('cpu', mode[1], b, S, grads=False))


@pytest.mark.parametrize('sizes', R.SIZES, ids=_ids)
def test_logistic_is_within_the_bound_of_the_twin_and_of_float64(sizes):
    a, b = _ab(sizes, 1)
    for st in (None, R.new_state(gamma=0.9, start=2, count=2, alpha_r=0.4375, alpha_f=-0.3)):
        for form in FORMS if st is not None else FORMS[:1]:
            dev, cpu = R.run_d(DEV, R.LOGISTIC, a, b, S, LAM, form[1], st), R.run_d('cpu', R.LOGISTIC, a, b, S, LAM, form[1], st)
            want, bd = R.d_step(R.LOGISTIC, a, b, S, LAM, form[1], st, ulps=R.ULPS['device'])
            _, bh = R.d_step(R.LOGISTIC, a, b, S, LAM, form[1], st, ulps=R.ULPS['host'])
            R.check_d(dev, want, bd, ('float64', sizes, form))
            both = _add(bd, bh)                    # each side is within its own bound of the exact value
            R.check_d(dev, {k: np.asarray(cpu[k], np.float64) for k in both}, both, ('twin', sizes, form))
            # the means, and with them the state, hold no exp or log1p: the twin's bits
            assert dev['mean_a'] == cpu['mean_a'] and dev['mean_b'] == cpu['mean_b'] and dev['words'] == cpu['words']
    g, gc = R.run_g(DEV, R.LOGISTIC, b, S), R.run_g('cpu', R.LOGISTIC, b, S)
    want, bd = R.g_step(R.LOGISTIC, b, S, ulps=R.ULPS['device'])
    _, bh = R.g_step(R.LOGISTIC, b, S, ulps=R.ULPS['host'])
    assert abs(float(g['obj']) - want['obj']) <= bd['obj'] and abs(float(g['obj']) - float(gc['obj'])) <= bd['obj'] + bh['obj']
    assert (np.abs(g['db'] - want['db']) <= bd['db']).all() and (np.abs(g['db'].astype(np.float64) - gc['db']) <= bd['db'] + bh['db']).all()


def test_entry_points_refuse_and_write_nothing():
    from hoig_amd import _lib as L
    a, b = torch.zeros(600, device=DEV), torch.zeros(600, device=DEV)
    da, slot, ws = torch.full((600,), 7.0, device=DEV), torch.full((1,), 7.0, device=DEV), torch.zeros(64, dtype=torch.float64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    need = L.lib.hoig_gan_d_loss_workspace_bytes(600, 600)
    assert need == 4 * 48
    good = [R.HINGE, a.data_ptr(), 600, b.data_ptr(), 600, 1.0, 0.0, R.PAPER, None, da.data_ptr(), None, slot.data_ptr(), None, None, None,
            ws.data_ptr(), need, st]
    for i, v in ((0, 7), (2, 0), (9, b.data_ptr() + 64), (15, None), (15, ws.data_ptr() + 4), (16, need - 8)):
        bad = list(good)
        bad[i] = v
        assert L.lib.hoig_gan_d_loss(*bad) == L.EINVAL, (i, v)
    assert L.lib.hoig_gan_g_loss(R.HINGE, b.data_ptr(), 600, 1.0, None, slot.data_ptr(), ws.data_ptr(), 48, st) == L.EINVAL     # two chunks
    torch.cuda.synchronize()
    assert float(slot[0]) == 7.0 and bool((da == 7.0).all())
    assert L.lib.hoig_gan_d_loss(*good) == L.OK
    torch.cuda.synchronize()
    assert float(slot[0]) == 7.0 + 2.0 and bool((da == -1.0 / 600).all())


def test_the_autograd_functions_hand_back_the_stored_gradients():
    from hoig_amd import gan_loss as G
    from hoig_amd import ops
    a, b = _ab((130, 77), 2)
    slots = ops.LossSlots(['d', 'g_adv'], DEV, extra=['d_real', 'd_fake', 'd_reg'])
    lc = G.LeCam(DEV, LAM, decay=0.9, start=1)
    lc.load_state_dict(dict(count=1, alpha_real=0.25, alpha_fake=-0.5))
    ta, tb = torch.from_numpy(a).to(DEV).requires_grad_(True), torch.from_numpy(b).to(DEV).requires_grad_(True)
    slots.begin()
    d = G.gan_d_loss(ta, tb, R.HINGE, S, slots.term('d'), lecam=lc, into_real=slots.term('d_real'), into_fake=slots.term('d_fake'),
                     into_reg=slots.term('d_reg'))
    g = G.gan_g_loss(tb, R.HINGE, S, slots.term('g_adv'))
    slots.total(d, g).backward()
    torch.cuda.synchronize()
    st = R.new_state(gamma=0.9, start=1, count=1, alpha_r=0.25, alpha_f=-0.5)
    twin, twin_g = R.run_d('cpu', R.HINGE, a, b, S, LAM, R.PAPER, st), R.run_g('cpu', R.HINGE, b, S)
    assert ta.grad.cpu().numpy().tobytes() == twin['da'].tobytes()
    assert tb.grad.cpu().numpy().tobytes() == (twin['db'] + twin_g['db']).tobytes()
    assert [float(slots.value(k)) for k in ('d', 'd_real', 'd_fake', 'd_reg', 'g_adv')] == \
        [float(twin[k]) for k in ('obj', 'mean_a', 'mean_b', 'reg')] + [float(twin_g['obj'])]
    assert lc.state_dict()['count'] == 2 and lc.state.cpu().numpy().tobytes() == twin['words']


# ------------------------------------------------------------------------------------------------ Trainer
def _trainer(**over):
    from common import product_trainer
    return product_trainer(GEN, BATCH, SIDE, **over)


def _settle(m):
    m._wait_g()
    m._wait_d()
    torch.cuda.synchronize()


def _tap_d(m):
    """Every call of D's forward leaves (logits, the gradient that came back into them) in the list that is returned."""
    seen = []
    real = m._D.forward_nhwc

    def forward_nhwc(x):
        out = real(x)
        rec = [out.detach().clone(), None]
        if out.requires_grad:
            out.register_hook(lambda g: rec.__setitem__(1, g.detach().clone()))
        seen.append(rec)
        return out

    m._D.forward_nhwc = forward_nhwc
    return seen


def _torch_objective(mode, a, b, s):
    F = torch.nn.functional
    if mode == 'hinge':
        d = s * F.relu(1 - a).mean() + s * F.relu(1 + b).mean() if a is not None else None
        return d, -s * b.mean()
    sp = lambda z: torch.clamp(z, min=0) + torch.log1p(torch.exp(-z.abs()))      # (F.softplus turns linear above a threshold)
    d = s * sp(-a).mean() + s * sp(b).mean() if a is not None else None
    return d, s * sp(-b).mean()


@pytest.mark.parametrize('mode', ['hinge', 'logistic'])
def test_trainer_step_hands_d_the_objectives_gradient(mode):
    m = _trainer(gan_mode=mode, lambda_D_prob=0.5)
    assert m._gan is not None and m._lecam is None
    seen = _tap_d(m)
    pG = next(m._net(m._G).parameters()).detach().clone()
    pD = next(m._net(m._D).parameters()).detach().clone()
    m.optimize_parameters()
    _settle(m)
    assert sorted(r[0].shape[0] for r in seen) == [BATCH, 2 * BATCH] and all(r[1] is not None for r in seen)
    (g_logits, g_grad), (d_logits, d_grad) = sorted(seen, key=lambda r: r[0].shape[0])
    ulps = R.ULPS['device'] if mode == 'logistic' else R.ULPS['exact']
    s = 0.5
    # the D step: the gradient that entered D against torch autograd, in float64, on the same logits
    x = d_logits.double().requires_grad_(True)
    obj, _ = _torch_objective(mode, x[:BATCH], x[BATCH:], s)
    obj.backward()
    a, b = d_logits[:BATCH].cpu().numpy().ravel(), d_logits[BATCH:].cpu().numpy().ravel()
    want, bound = R.d_step(R.MODES[mode], a, b, s, ulps=ulps)
    got = d_grad.cpu().numpy().reshape(2, -1).astype(np.float64)
    auto = x.grad.cpu().numpy().reshape(2, -1)
    assert (np.abs(got[0] - auto[0]) <= bound['da']).all() and (np.abs(got[1] - auto[1]) <= bound['db']).all()
    assert np.abs(auto[0] - want['da']).max() <= 1e-15 and np.abs(auto[1] - want['db']).max() <= 1e-15     # (two float64 statements)
    errs = m.get_current_errors()
    assert abs(float(m._d_terms.value('d').detach()) - want['obj']) <= bound['obj'] and abs(float(obj.detach()) - want['obj']) <= 1e-12
    assert abs(errs['d_real'] - want['mean_a']) <= bound['mean_a'] and abs(errs['d_fake'] - want['mean_b']) <= bound['mean_b']
    # the G step
    y = g_logits.double().requires_grad_(True)
    _, gobj = _torch_objective(mode, None, y, s)
    gobj.backward()
    gb = g_logits.cpu().numpy().ravel()
    gwant, gbound = R.g_step(R.MODES[mode], gb, s, ulps=ulps)
    assert (np.abs(g_grad.cpu().numpy().ravel().astype(np.float64) - y.grad.cpu().numpy().ravel()) <= gbound['db']).all()
    assert abs(errs['g_adv'] - gwant['obj']) <= gbound['obj'] and abs(float(gobj.detach()) - gwant['obj']) <= 1e-12
    # both networks moved, and nothing went non-finite
    for net, before in ((m._G, pG), (m._D, pD)):
        after = next(m._net(net).parameters()).detach()
        assert bool(torch.isfinite(after).all()) and not torch.equal(after, before)
    assert all(np.isfinite(v) for v in errs.values())
    assert list(m.get_current_scalars()) == ['lr_G', 'lr_D']


@pytest.mark.parametrize('how,start', [('eager', 2), ('eager_d_late', 2), ('unforked', 2), ('captured', 2), ('captured', 4)],
                         ids=lambda v: str(v))
def test_lecam_through_the_trainer(how, start, monkeypatch):
    """'eager': the D step beside G's backward ('d_early'); 'eager_d_late': behind it; 'unforked': every chain on the caller's stream
    (what HOIG_STREAMS=0 selects); 'captured': the replayed hipGraph -- with start 4 the weight switches on inside the replays."""
    from hoig_amd import _lib as L
    from hoig_amd import ops
    from hoig_amd.models.networks import generator as G
    if how == 'unforked':
        monkeypatch.setattr(G, '_FORK_STREAMS', False)
        monkeypatch.setattr(ops, '_WGRAD_SIDE', False)
    prev = L.set_tuning('d_early', 0 if how == 'eager_d_late' else 1)
    try:
        _lecam_steps(how, start)
    finally:
        L.set_tuning('d_early', prev)


def _lecam_steps(how, start):
    m = _trainer(gan_mode='hinge', lecam=0.3, lecam_decay=0.9, lecam_start=start, hip_graph=(how == 'captured'))
    assert m._lecam is not None and m.get_current_scalars()['d_reg'] == 0.0
    ref = R.new_state(gamma=0.9, start=start)
    means = []
    steps = start + 3
    for k in range(1, steps + 1):
        m.optimize_parameters()
        _settle(m)
        errs, sc = m.get_current_errors(), m.get_current_scalars()
        assert list(sc) == ['lr_G', 'lr_D', 'lecam_real', 'lecam_fake', 'd_reg', 'lecam_bad']
        on = ref['count'] >= start                       # decided from the count as it stood before the step
        ref = R.tick(ref, errs['d_real'], errs['d_fake'])
        means += [errs['d_real'], errs['d_fake']]
        assert m._lecam.state_dict()['count'] == k and sc['lecam_bad'] == 0
        bound = R.anchor_bound(k, means, fed_fp32=True)
        assert abs(sc['lecam_real'] - ref['alpha_r']) <= bound and abs(sc['lecam_fake'] - ref['alpha_f']) <= bound, (k, sc, ref)
        assert (sc['d_reg'] > 0.0) == on and (on or sc['d_reg'] == 0.0), (k, sc['d_reg'])
        assert all(np.isfinite(v) for v in errs.values())
    assert ref['count'] == steps and on
    if how == 'captured':
        assert any(g['graphs'] is not None for g in m._graphs.values()), 'the step was never captured'
    # a step that does not train D runs no D head and takes no tick
    m.optimize_parameters(trainable=False)
    _settle(m)
    assert m._lecam.state_dict()['count'] == steps


def test_trainer_with_the_defaults_is_the_parents(monkeypatch, tmp_path):
    from hoig_amd import _lib as L
    called = []
    real_call, real_attempt = L.call, L.attempt
    monkeypatch.setattr(L, 'call', lambda name, *a: (called.append(name), real_call(name, *a))[1])
    monkeypatch.setattr(L, 'attempt', lambda name, *a: (called.append(name), real_attempt(name, *a))[1])
    m = _trainer(checkpoints_dir=str(tmp_path))
    assert m._gan is None and m._lecam is None and m._d_terms.extra == ['d_real', 'd_fake']
    m.optimize_parameters()
    m.optimize_parameters()
    m.save(1)
    assert called and not [n for n in called if n.startswith('hoig_gan_')]
    assert called.count('hoig_loss_accumulate') >= 6 and called.count('hoig_sum_scaled') == 4       # D's four launches, twice
    assert list(m.get_current_scalars()) == ['lr_G', 'lr_D']
    assert list(m.get_current_errors()) == ['g_rec', 'g_tsf', 'g_adv', 'g_mask', 'g_mask_smooth', 'd_real', 'd_fake']
    assert sorted(os.listdir(os.path.join(str(tmp_path), 't'))) == sorted(
        '%s_epoch_1_id_%s.pth' % (kind, tag) for kind in ('net', 'opt') for tag in 'GD')
    # ... and with an option on the heads are what is called
    del called[:]
    h = _trainer(gan_mode='hinge', lecam=0.1)
    h.optimize_parameters()
    assert called.count('hoig_gan_d_loss') == 1 and called.count('hoig_gan_g_loss') == 1 and 'hoig_sum_scaled' not in called


def test_save_and_load_restore_the_state_bit_for_bit(tmp_path, capsys):
    from common import opt_namespace
    from hoig_amd.models import ModelsFactory
    root = str(tmp_path)
    over = dict(gan_mode='logistic', lecam=0.2, lecam_decay=0.9, lecam_start=2, lecam_form='relu', checkpoints_dir=root)
    a = _trainer(**over)
    for _ in range(3):
        a.optimize_parameters()
    a.save(1)
    torch.cuda.synchronize()
    assert 'opt_epoch_1_id_D_lecam.pth' in os.listdir(os.path.join(root, 't'))
    sd = torch.load(os.path.join(root, 't', 'opt_epoch_1_id_D_lecam.pth'))
    assert sd['count'] == 3 and sd['bad'] == 0 and sd['form'] == 'relu' and sd['start'] == 2
    b = ModelsFactory.get_by_name('trainer', opt_namespace(load_epoch=1, **over))
    torch.cuda.synchronize()
    assert b._lecam.state.cpu().numpy().tobytes() == a._lecam.state.cpu().numpy().tobytes()
    assert 'loaded LeCam state' in capsys.readouterr().out
    os.remove(os.path.join(root, 't', 'opt_epoch_1_id_D_lecam.pth'))
    c = ModelsFactory.get_by_name('trainer', opt_namespace(load_epoch=1, **over))
    said = capsys.readouterr().out
    assert 'no LeCam checkpoint' in said and 'opt_epoch_1_id_D_lecam.pth' in said and c._lecam.state_dict()['count'] == 0


def test_trainer_refuses_bad_options():
    from common import opt_namespace
    from hoig_amd.models import ModelsFactory
    with pytest.raises(ValueError, match='gan_mode'):
        ModelsFactory.get_by_name('trainer', opt_namespace(gan_mode='wgan'))
    with pytest.raises(ValueError, match='lecam_decay'):
        ModelsFactory.get_by_name('trainer', opt_namespace(lecam=0.1, lecam_decay=1.5))


# ------------------------------------------------------------------------------------------------ under a forced exchange
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_exchange(port, q):
    """A `nccl` group of one rank with the exchange forced on (as tests/test_ddp_rccl_gpu.py forces it): LeCam is refused where the
    model is built; the hinge objective, which keeps no state, runs."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HOIG_DDP_FORCE='1',
                      HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    try:
        _trainer(use_ddp=True, gan_mode='hinge', lecam=0.1)
        refused = None
    except ValueError as ex:
        refused = str(ex)
    m = _trainer(use_ddp=True, gan_mode='hinge')
    active = m._G.sync.active
    m.optimize_parameters()
    _settle(m)
    q.put((refused, active, all(np.isfinite(v) for v in m.get_current_errors().values())))
    dist.barrier()
    dist.destroy_process_group()


def test_lecam_under_an_active_exchange_raises_and_hinge_runs():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_run_exchange, args=(_free_port(), q))
    p.start()
    refused, active, finite = q.get(timeout=600)
    p.join(timeout=120)
    assert p.exitcode == 0
    assert active and refused is not None and 'lecam' in refused and 'exchange' in refused and '0.1' in refused
    assert finite
