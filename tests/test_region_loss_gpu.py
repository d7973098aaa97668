"""The opt-in region reconstruction term of G on the device (docs/region_loss.md): the kernels against the CPU twin, bit for bit
(tests/test_region_loss_cpu.py pins the twin against float64); the autograd function against torch autograd in float64; the Trainer's
opt.lambda_rec_hand / opt.lambda_rec_obj in the eager and the captured step; and the defaults, which are the parent's."""
import gc
import os

import numpy as np
import pytest
import torch

import region_loss_reference as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GEN, BATCH, SIDE = 'generator_spade_attn', 2, 64
_ids = lambda v: 'x'.join(str(s) for s in v)


# ------------------------------------------------------------------------------------------------ kernels against the twin
@pytest.mark.parametrize('shape', R.SHAPES, ids=_ids)
def test_head_equals_the_twin_bit_for_bit(shape):
    pred, target, labels = R.case(shape)
    assert R.same_bits(R.run(DEV, pred, target, labels, init=0.5), R.run('cpu', pred, target, labels, init=0.5))
    for kw in (dict(grads=False), dict(split=False, min_pixels=1), dict(grads=False, reports=False, counts=False, split=False),
               dict(lam=(0.5, 0.0, 3.0), lam_all=0.0, min_pixels=10 ** 6)):
        assert R.same_bits(R.run(DEV, pred, target, labels, **kw), R.run('cpu', pred, target, labels, **kw)), kw


def test_head_equals_the_twin_on_the_edges_of_validity_bad_labels_and_a_nan():
    pred, target, labels = R.case((3, 16, 16, 3), seed=3)
    labels[labels == 1] = 0
    labels[1].reshape(-1)[5:14] = 1          # a hand of 9, and one of exactly 10
    labels[2].reshape(-1)[20:30] = 1
    for m in (9, 10, 11):
        dev, cpu = R.run(DEV, pred, target, labels, min_pixels=m), R.run('cpu', pred, target, labels, min_pixels=m)
        assert R.same_bits(dev, cpu), m
        R.check(dev, R.reference(pred, target, labels, min_pixels=m), m)
    labels[1, 3, 4], labels[0, 0, 9] = 7, 5
    dev = R.run(DEV, pred, target, labels)
    assert R.same_bits(dev, R.run('cpu', pred, target, labels)) and int(dev['status'][0]) == (R.BAD_LABEL | (7 << 8))
    lam7 = (0.0, 10.0, 2.5, 0.0, 0.0, 1.0, 0.0, 2.0)
    dev = R.run(DEV, pred, target, labels, lam=lam7, min_pixels=1)
    assert R.same_bits(dev, R.run('cpu', pred, target, labels, lam=lam7, min_pixels=1)) and int(dev['status'][0]) == 0
    pred[0, 2, 2, 1] = np.nan                # (a NaN's payload is not pinned: docs/region_loss.md)
    dev, cpu = R.run(DEV, pred, target, labels), R.run('cpu', pred, target, labels)
    assert R.same_bits(dev, cpu, nan_payload=False) and np.isnan(dev['term_all'][0]) and dev['dpred'][0, 2, 2, 1] == 0.0


def test_sign_of_zero_is_the_l1_kernels():
    """d = +0, -0, > 0, < 0 through hoig_loss_accumulate(HOIG_LOSS_L1) and through the head with a frame weight alone: the same gradients."""
    from hoig_amd import _lib as L
    pred = np.array([0.5, 0.25, -0.0, 0.0, -1.0, 2.0], np.float32).reshape(1, 1, 2, 3)
    target = np.array([0.5, 0.5, 0.0, -0.0, -1.0, 1.0], np.float32).reshape(1, 1, 2, 3)
    got = R.run(DEV, pred, target, np.zeros((1, 1, 2), np.uint8), lam=(0.0,), lam_all=6.0, min_pixels=1)
    p, t = torch.from_numpy(pred).to(DEV), torch.from_numpy(target).to(DEV)
    d, slot = torch.full_like(p, 7.0), torch.zeros(1, device=DEV)
    L.call('hoig_loss_accumulate', L.LOSS_L1, p.data_ptr(), t.data_ptr(), 0.0, 1.0, slot.data_ptr(), d.data_ptr(), 6,
           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert got['dpred'].reshape(-1).tolist() == d.cpu().reshape(-1).tolist() == [0.0, -1.0, 0.0, 0.0, 0.0, 1.0]


def test_entry_point_refuses_and_writes_nothing():
    import ctypes
    from hoig_amd import _lib as L
    p, t = torch.zeros(2, 4, 4, 3, device=DEV), torch.ones(2, 4, 4, 3, device=DEV)
    d, slot = torch.full((2, 4, 4, 3), 7.0, device=DEV), torch.full((1,), 7.0, device=DEV)
    lab, st = torch.zeros(2, 4, 4, dtype=torch.uint8, device=DEV), torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ws = torch.zeros(64, dtype=torch.float64, device=DEV)
    lam = (ctypes.c_double * 3)(0.0, 1.0, 1.0)
    need = L.lib.hoig_region_loss_workspace_bytes(2, 4, 4, 3, 2)
    assert 0 < need <= 64 * 8
    good = [p.data_ptr(), t.data_ptr(), lab.data_ptr(), 2, 4, 4, 3, 2, ctypes.cast(lam, ctypes.c_void_p), 96.0, 4, d.data_ptr(), slot.data_ptr(),
            None, None, None, st.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream]
    for i, v in ((3, 0), (7, R.MAX_R + 1), (10, 0), (11, p.data_ptr()), (17, None), (17, ws.data_ptr() + 8), (18, need - 8)):
        bad = list(good)
        bad[i] = v
        assert L.lib.hoig_region_loss(*bad) == L.EINVAL, (i, v)
    torch.cuda.synchronize()
    assert float(slot[0]) == 7.0 and bool((d == 7.0).all()) and int(st[0]) == -1
    assert L.lib.hoig_region_loss(*good) == L.OK
    torch.cuda.synchronize()
    assert float(slot[0]) == 7.0 + 96.0 and bool((d == -1.0).all()) and int(st[0]) == 0


# ------------------------------------------------------------------------------------------------ the autograd function
def _torch_terms(pred, target, labels, lam, lam_all, min_pixels):
    """Section 1 with torch.where on the labels, in float64 -> (sum_r lam_r L_r, lam_all L_all, [L_r])."""
    N, H, W, C = pred.shape
    ad = (pred - target).abs()
    Ls = []
    for r in range(len(lam)):
        m = labels == r
        n = m.reshape(N, -1).sum(1)
        valid = n >= min_pixels
        V = int(valid.sum())
        if V == 0:
            Ls.append(ad.sum() * 0.0)
            continue
        per = torch.where(m[..., None], ad, torch.zeros_like(ad)).reshape(N, -1).sum(1) / (C * n.clamp(min=1)).double()
        Ls.append(torch.where(valid, per, torch.zeros_like(per)).sum() / V)
    return sum(l * L for l, L in zip(lam, Ls)), lam_all * ad.mean(), Ls


def test_the_autograd_function_against_torch_autograd_in_float64():
    from hoig_amd import ops
    from hoig_amd import region_loss as RL
    pred, target, labels = R.case(R.SHAPES[3], seed=11)
    labels[0][labels[0] == 1] = 0                      # an image without a hand
    slots = ops.LossSlots(['g_rec', 'g_rec_region'], DEV, extra=['g_rec_bg', 'g_rec_hand', 'g_rec_obj'])
    tp = torch.from_numpy(pred).to(DEV).requires_grad_(True)
    tt, tl = torch.from_numpy(target).to(DEV), torch.from_numpy(labels).to(DEV)
    slots.begin()
    a = RL.region_l1_loss(tp, tt, tl, R.LAM, R.LAM_ALL, R.MIN_PIXELS, slots.term('g_rec_region'), into_regions=slots.term('g_rec_bg'),
                          into_all=slots.term('g_rec'))
    b = RL.region_l1_loss(tp, tt, tl, R.LAM, 0.0, R.MIN_PIXELS, slots.term('g_rec_region'), into_regions=slots.term('g_rec_bg'))
    slots.total(a, b).backward()
    torch.cuda.synchronize()
    x = tp.detach().double().requires_grad_(True)
    regions, frame, Ls = _torch_terms(x, tt.double(), tl, R.LAM, R.LAM_ALL, R.MIN_PIXELS)
    (2 * regions + frame).backward()
    want = R.reference(pred, target, labels)
    auto = x.grad.cpu().numpy()
    assert np.abs(auto - (want['grad'] + want['sign'] * want['B'][..., None])).max() <= 1e-15          # (two float64 statements)
    # each call's gradient is within the gradient bound of its own; autograd adds the two in one more fp32 add
    bound = 2 * R.grad_bound(want) + R.u * np.abs(auto)
    got = tp.grad.cpu().numpy().astype(np.float64)
    assert (np.abs(got - auto) <= bound).all() and (got[want['sign'] == 0] == 0).all()
    # calling twice into one slot adds
    once = R.run('cpu', pred, target, labels)
    twice = lambda v: float(np.float32(v) + np.float32(v))
    assert float(slots.value('g_rec')) == float(once['term_all'][0]) and float(slots.value('g_rec_region')) == twice(once['term'][0])
    assert [float(slots.value(k)) for k in ('g_rec_bg', 'g_rec_hand', 'g_rec_obj')] == [twice(v) for v in once['terms_r']]
    assert abs(float(slots.value('g_rec_region')) - 2 * float(regions.detach())) <= 2 * R.value_bound(want, float(regions.detach())) + R.u * 2 * float(regions.detach())


# ------------------------------------------------------------------------------------------------ Trainer
ON = dict(lambda_rec_hand=10, lambda_rec_obj=10, region_loss_min_pixels=4)


_BUILT = []


def _trainer(**over):
    from common import product_trainer
    m = product_trainer(GEN, BATCH, SIDE, **over)
    _BUILT.append(m)
    return m


@pytest.fixture(autouse=True)
def _models_leave_with_their_test():
    """A tapped model refers to itself (_tap_g), so it would live until some later collection and hand its streams back in the middle
    of another file's test: every model built here is closed, and collected, when its test ends."""
    yield
    while _BUILT:
        m = _BUILT.pop()
        m.__dict__.pop('_optimize_G', None)
        torch.cuda.synchronize()
        m.close()
        del m
    gc.collect()


def _settle(m):
    m._wait_g()
    m._wait_d()
    torch.cuda.synchronize()


def _tap_g(m):
    """Every call of the G loss leaves the two fake images, and the gradient that came back into the target view's, in the dict that is
    returned.  (Inside a capture the copies become part of the graph: every replay refreshes them.)"""
    seen = {}
    real = m._optimize_G

    def optimize_G(fake_src, fake_tsf, mbg, mh):
        seen['fake_src'], seen['fake_tsf'] = fake_src.detach().clone(), fake_tsf.detach().clone()
        if fake_tsf.requires_grad and not torch.cuda.is_current_stream_capturing():
            fake_tsf.register_hook(lambda g: seen.__setitem__('grad_tsf', g.detach().clone()))
        return real(fake_src, fake_tsf, mbg, mh)

    m._optimize_G = optimize_G
    return seen


def _nhwc(x):
    return np.ascontiguousarray(x.permute(0, 2, 3, 1).cpu().numpy())


def _check_report(m, seen, views='both'):
    """The step's scalars against the float64 reference on the captured images and the batch's labels -> the reference's L_hand."""
    B = BATCH
    n, o, g = m._n, m._opt, m._region
    labels = n['region_labels'].cpu().numpy()
    assert labels.shape == (2 * B, SIDE, SIDE) and set(np.unique(labels)) == {0, 1, 2}
    lam = (0.0, g['hand'], g['obj'])
    src = R.reference(_nhwc(seen['fake_src']), n['real_src'].cpu().numpy(), labels[:B], lam, o.lambda_rec, g['min_pixels'])
    tsf = R.reference(_nhwc(seen['fake_tsf']), n['real_tsf'].cpu().numpy(), labels[B:], lam, 0.0, g['min_pixels'])
    errs, sc = m.get_current_errors(), m.get_current_scalars()
    assert list(sc) == ['lr_G', 'lr_D', 'g_rec_region', 'g_rec_hand', 'g_rec_obj'] and all(np.isfinite(v) for v in sc.values())
    assert list(errs) == ['g_rec', 'g_tsf', 'g_adv', 'g_mask', 'g_mask_smooth', 'd_real', 'd_fake'] and all(np.isfinite(v) for v in errs.values())
    assert src['V'][1] > 0 and src['V'][2] > 0 and tsf['V'][1] > 0 and tsf['V'][2] > 0
    if views != 'tsf':        # (with the target view alone g_rec is ops.l1_loss's fp32 sum, as with the option off)
        assert abs(errs['g_rec'] - src['all']) <= R.value_bound(src, src['all']), (errs['g_rec'], src['all'])
    used = [w for w, name in ((src, 'src'), (tsf, 'tsf')) if views in ('both', name)]
    for key, r in (('g_rec_hand', 1), ('g_rec_obj', 2)):
        ref = sum(w['L'][r] for w in used)
        assert abs(sc[key] - ref) <= sum(R.value_bound(w, w['L'][r]) for w in used) + R.u * ref, (key, sc[key], ref)
    ref = sum(w['regions'] for w in used)
    assert abs(sc['g_rec_region'] - ref) <= sum(R.value_bound(w, w['regions']) for w in used) + R.u * ref
    return sum(w['L'][1] for w in used), tsf


def _tap_region(monkeypatch):
    """Every call of region_l1_loss leaves the gradient that the head hands back to autograd in the list that is returned: the image goes
    in through an alias of its own, so what arrives at the alias is this head's contribution alone."""
    from hoig_amd import region_loss as RL
    calls = []
    real = RL.region_l1_loss

    def region_l1_loss(pred, *a, **kw):
        alias, rec = pred.view_as(pred), {}
        if alias.requires_grad and not torch.cuda.is_current_stream_capturing():
            alias.register_hook(lambda g: rec.__setitem__('grad', g.detach().clone()))
        calls.append(rec)
        return real(alias, *a, **kw)

    monkeypatch.setattr(RL, 'region_l1_loss', region_l1_loss)
    return calls


@pytest.mark.parametrize('how', ['eager', 'eager_d_late', 'unforked'])
def test_trainer_step_with_the_region_terms(how, monkeypatch):
    """'eager': the D step beside G's backward ('d_early'); 'eager_d_late': behind it; 'unforked': every chain on the caller's stream
    (what HOIG_STREAMS=0 selects).  The gradient that enters G's output is a sum over its consumers, so what the region weights change
    in it is the head's own contribution: that is what is held to the labels here.  (Two models' forwards are not equal bit for bit --
    their fake images differed by 1e-6 relative when this test compared two of them --, so the weights-off gradient of a second model
    cannot serve.)"""
    from hoig_amd import _lib as L
    from hoig_amd import ops
    from hoig_amd.models.networks import generator as G
    if how == 'unforked':
        monkeypatch.setattr(G, '_FORK_STREAMS', False)
        monkeypatch.setattr(ops, '_WGRAD_SIDE', False)
    prev = L.set_tuning('d_early', 0 if how == 'eager_d_late' else 1)
    try:
        m = _trainer(**ON)
        assert m._region is not None
        seen, calls = _tap_g(m), _tap_region(monkeypatch)
        pG = next(m._net(m._G).parameters()).detach().clone()
        pD = next(m._net(m._D).parameters()).detach().clone()
        m.optimize_parameters()
        _settle(m)
        for net, before in ((m._G, pG), (m._D, pD)):         # both networks moved, and nothing went non-finite
            after = next(m._net(net).parameters()).detach()
            assert bool(torch.isfinite(after).all()) and not torch.equal(after, before)
        _, tsf = _check_report(m, seen)
        labels = m._n['region_labels'].cpu().numpy()[BATCH:]
        assert len(calls) == 2 and bool(torch.isfinite(seen['grad_tsf']).all())
        # the target view's head changes the gradient only on the hand's and the object's pixels of valid rows ...
        part = calls[1]['grad'].cpu().numpy()
        valid = tsf['counts'] >= ON['region_loss_min_pixels']
        inside = np.zeros(labels.shape, bool)
        for r in (1, 2):
            inside |= (labels == r) & valid[:, r][:, None, None]
        assert inside.any() and not part[~inside].any() and np.array_equal(part[inside] != 0, tsf['sign'][inside] != 0)
        # ... by the twin's bits on the captured image; the source view's head carries the frame part everywhere
        B = BATCH
        lam, real = (0.0, 10.0, 10.0), m._n['real_tsf'].cpu().numpy()
        assert part.tobytes() == R.run('cpu', _nhwc(seen['fake_tsf']), real, labels, lam, 0.0, 4)['dpred'].tobytes()
        src = R.run('cpu', _nhwc(seen['fake_src']), m._n['real_src'].cpu().numpy(), m._n['region_labels'].cpu().numpy()[:B], lam,
                    m._opt.lambda_rec, 4)
        assert calls[0]['grad'].cpu().numpy().tobytes() == src['dpred'].tobytes()
    finally:
        L.set_tuning('d_early', prev)


@pytest.mark.parametrize('views', ['src', 'tsf'])
def test_trainer_with_one_view(views):
    m = _trainer(region_loss_views=views, **ON)
    seen = _tap_g(m)
    m.optimize_parameters()
    _settle(m)
    _check_report(m, seen, views)


def test_the_captured_step_follows_each_batchs_masks():
    from common import SEEDS
    from hoig_amd import synthetic
    m = _trainer(hip_graph=True, **ON)
    seen = _tap_g(m)
    batches = [synthetic.make_inputs(BATCH, SIDE, seed=SEEDS['inputs']), synthetic.make_inputs(BATCH, SIDE, seed=77)]
    hands = []
    for k in (0, 0, 0, 1, 0, 1):                     # two eager steps, the capture and its replay, then replays on two batches in turn
        m.set_input(batches[k])
        m.optimize_parameters()
        _settle(m)
        hands.append((k, _check_report(m, seen)[0], m._n['region_labels'].cpu().numpy()))
    assert any(g['graphs'] is not None for g in m._graphs.values()), 'the step was never captured'
    a, b = hands[-2], hands[-1]
    assert a[0] != b[0] and not np.array_equal(a[2], b[2]) and a[1] != b[1]          # (each replay against its own batch's reference)


def test_trainer_with_the_defaults_is_the_parents(monkeypatch, tmp_path):
    from hoig_amd import _lib as L
    called = []
    real_call, real_attempt = L.call, L.attempt
    monkeypatch.setattr(L, 'call', lambda name, *a: (called.append(name), real_call(name, *a))[1])
    monkeypatch.setattr(L, 'attempt', lambda name, *a: (called.append(name), real_attempt(name, *a))[1])
    m = _trainer(checkpoints_dir=str(tmp_path))
    assert m._region is None and m._g_terms.names == ['g_adv', 'g_rec', 'g_tsf', 'g_mask', 'g_mask_smooth'] and m._g_terms.extra == []
    assert 'region_labels' not in m._n
    del called[:]
    m.optimize_parameters()
    _settle(m)
    default = list(called)
    m.save(1)
    assert default and not [n for n in called if n.startswith('hoig_region_loss')]
    assert list(m.get_current_scalars()) == ['lr_G', 'lr_D']
    assert list(m.get_current_errors()) == ['g_rec', 'g_tsf', 'g_adv', 'g_mask', 'g_mask_smooth', 'd_real', 'd_fake']
    assert sorted(os.listdir(os.path.join(str(tmp_path), 't'))) == sorted(
        '%s_epoch_1_id_%s.pth' % (kind, tag) for kind in ('net', 'opt') for tag in 'GD')
    # ... and with the option on the source view's L1 launch is the head's: one launch less of the one, two calls of the other, and
    # every other loss launch as before.  (Only the loss kernels are compared: what else a model's first step calls -- a bank of
    # streams when the process has none idle, their scratch -- depends on the models the process has built before.)
    # (the first model goes before the second comes: two at once would make the process create a second set of streams, which
    # later tests of the suite would then find in its banks)
    _BUILT.remove(m)
    m.close()
    del m
    gc.collect()
    h = _trainer(checkpoints_dir=str(tmp_path / 'on'), **ON)
    del called[:]
    h.optimize_parameters()
    _settle(h)
    on = list(called)
    assert on.count('hoig_region_loss') == 2 and on.count('hoig_loss_accumulate') == default.count('hoig_loss_accumulate') - 1
    for name in ('hoig_tv_accumulate', 'hoig_sum', 'hoig_sum_scaled', 'hoig_loss_fwd_bwd'):
        assert on.count(name) == default.count(name), (name, on.count(name), default.count(name))
    h.save(1)
    assert sorted(os.listdir(os.path.join(str(tmp_path / 'on'), 't'))) == sorted(os.listdir(os.path.join(str(tmp_path), 't')))


def test_trainer_refuses_bad_options():
    from common import opt_namespace
    from hoig_amd.models import ModelsFactory
    with pytest.raises(ValueError, match='lambda_rec_hand'):
        ModelsFactory.get_by_name('trainer', opt_namespace(lambda_rec_hand=-1))
    with pytest.raises(ValueError, match='region_loss_views'):
        ModelsFactory.get_by_name('trainer', opt_namespace(lambda_rec_obj=1, region_loss_views='all'))
