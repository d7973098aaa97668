"""The discriminator augmentation on the device (docs/d_augment.md): the kernels against the CPU twins bit for bit
(tests/test_d_augment_cpu.py pins the twins); the autograd operator; the Trainer's opt.d_augment in the eager step (with 'd_early' on
and off), the captured step, adaptive mode, the checkpoint file and under a forced gradient exchange."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import d_augment_reference as R

pytestmark = pytest.mark.gpu
GEN, BATCH, SIDE = 'generator_spade_attn', 2, 64
CASES = [(hw, B, k) for hw in R.SHAPES for B, k in ((1, 1), (3, 2), (1, 4), (3, 7), (3, 16))] + [((64, 64), 2, 16)]


def _call(name, *args):
    from hoig_amd import _lib as L
    return getattr(L.lib, name)(*args)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    """A device copy of a numpy array, 16-byte aligned (the caching allocator hands out 512-byte multiples)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    t = torch.from_numpy(a.copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _host_state(state_d):
    s = R.aligned(R.STATE_WORDS, np.uint64, 0)
    s[:] = state_d.cpu().numpy().view(np.uint64)
    return s


def _mixed_records(B, H, W, seed):
    """Records of every flag combination: drawn at p = 0.5 with every family, a different step per call."""
    return R.twin_draw(R.make_state(step=seed, p=0.5), 1, B, H, W)


def _data(B, H, W, k, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (B, H, W, 3)).astype(np.float32), rng.uniform(-1, 1, (B, H, W, k)).astype(np.float32),
            rng.uniform(-1, 1, (B, H, W, 3 + k)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize('hw', [(5, 7), (8, 8), (64, 64), (256, 256)], ids=lambda v: '%dx%d' % v)
def test_tick_and_draw_equal_the_twins(hw):
    H, W = hw
    B = 300                                                # (two workgroups of the draw)
    for step, p, policy, rank in ((0, 1.0, 7, 0), (2 ** 32 - 2, 0.3, 5, 3), (7, 0.0, 7, 1), (9, 0.6, 2, 0)):
        state_h = R.make_state(step=step, p=p, policy=policy, seed=5, rank=rank)
        state_d = _dev(state_h)
        for site in (0, 1, 2):
            assert _call('hoig_daug_tick', state_d.data_ptr(), _st()) == 0 and R.tick_host(state_h) == 0
            params_d = torch.full((B, 8), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
            assert _call('hoig_daug_draw', state_d.data_ptr(), site, B, H, W, params_d.data_ptr(), _st()) == 0
            torch.cuda.synchronize()
            assert _bits(params_d) == R.twin_draw(state_h, site, B, H, W).tobytes(), (step, site)
            assert _bits(state_d) == state_h.tobytes()
    assert int(state_h[R.STEP]) == 12


@pytest.mark.parametrize('n', [1, 37, 256, 1000, 4099])
def test_adapt_equals_the_twin(n):
    rng = np.random.default_rng(n)
    state_h = R.make_state(p=0.5, target=0.6, interval=3, increment=0.125)
    state_d = _dev(state_h)
    ps = []
    for j in range(10):
        v = rng.choice([-1.0, 0.0, 0.5, 2.0] if j < 5 else [-1.0, -0.5, 0.0, 1.0], size=n).astype(np.float32)
        v_h = R.aligned(n, np.float32, v)
        assert _call('hoig_daug_adapt', state_d.data_ptr(), _dev(v_h).data_ptr(), n, _st()) == 0
        assert R.adapt_host(state_h, v_h, n) == 0
        torch.cuda.synchronize()
        assert _bits(state_d) == state_h.tobytes(), j
        ps.append(R.state_p(state_h))
    assert int(state_h[R.ADJUSTS]) == 3 and int(state_h[R.STEPS]) == 1


@pytest.mark.parametrize('hw,B,k', CASES, ids=lambda v: '%dx%d' % v if isinstance(v, tuple) else str(v))
def test_forward_and_backward_equal_the_twins_bit_for_bit(hw, B, k):
    """Both launches of each direction (the reduction and the body), records of every flag combination; the inputs are never written."""
    H, W = hw
    img, cond, g = _data(B, H, W, k, 1000 * H + 10 * W + k)
    for params in (R.twin_draw(R.make_state(step=H + k, p=1.0), 0, B, H, W), _mixed_records(B, H, W, H * W + k)):
        img_d, cond_d, g_d, par_d = _dev(img), _dev(cond), _dev(g), _dev(params)
        out_d = torch.full((B, H, W, 3 + k), float('nan'), device='cuda')
        dimg_d = torch.full((B, H, W, 3), float('nan'), device='cuda')
        ws = torch.zeros(B * R.MAX_PARTS, device='cuda')
        assert _call('hoig_daug_fwd', img_d.data_ptr(), cond_d.data_ptr(), par_d.data_ptr(), out_d.data_ptr(), B, H, W, k, ws.data_ptr(), _st()) == 0
        assert _call('hoig_daug_bwd', g_d.data_ptr(), par_d.data_ptr(), dimg_d.data_ptr(), B, H, W, k, ws.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        assert _bits(out_d) == R.twin_fwd(img, cond, params).tobytes()
        assert _bits(dimg_d) == R.twin_bwd(g, params).tobytes()
        assert _bits(img_d) == img.tobytes() and _bits(cond_d) == cond.tobytes() and _bits(g_d) == g.tobytes()
        assert _bits(par_d) == params.tobytes()


def test_unaligned_output_takes_the_scalar_stores():
    """`out` and `dimg` four bytes past a 16-byte boundary, `img` likewise (the scalar loads of the image sum): the same bits."""
    B, H, W, k = 2, 6, 10, 2
    img, cond, g = _data(B, H, W, k, 3)
    params = R.twin_draw(R.make_state(step=1, p=1.0), 2, B, H, W)
    raw_i, raw_o, raw_d = torch.zeros(img.size + 1, device='cuda'), torch.zeros(B * H * W * (3 + k) + 1, device='cuda'), torch.zeros(img.size + 1, device='cuda')
    raw_i[1:].copy_(torch.from_numpy(img.ravel()))
    cond_d, g_d, par_d, ws = _dev(cond), _dev(g), _dev(params), torch.zeros(B * R.MAX_PARTS, device='cuda')
    assert _call('hoig_daug_fwd', raw_i.data_ptr() + 4, cond_d.data_ptr(), par_d.data_ptr(), raw_o.data_ptr() + 4, B, H, W, k, ws.data_ptr(), _st()) == 0
    assert _call('hoig_daug_bwd', g_d.data_ptr(), par_d.data_ptr(), raw_d.data_ptr() + 4, B, H, W, k, ws.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert _bits(raw_o[1:]) == R.twin_fwd(img, cond, params).tobytes() and _bits(raw_d[1:]) == R.twin_bwd(g, params).tobytes()
    assert raw_o[0].item() == 0.0 and raw_d[0].item() == 0.0


def test_each_half_of_a_stacked_tensor_leaves_the_other():
    B, H, W, k = 2, 9, 4, 7
    img, cond, _ = _data(B, H, W, k, 5)
    params = _mixed_records(B, H, W, 77)
    want = R.twin_fwd(img, cond, params).tobytes()
    img_d, cond_d, par_d, ws = _dev(img), _dev(cond), _dev(params), torch.zeros(B * R.MAX_PARTS, device='cuda')
    for half in (0, 1):
        both = torch.full((2 * B, H, W, 3 + k), 7.0, device='cuda')
        dst = both[half * B:(half + 1) * B]
        assert _call('hoig_daug_fwd', img_d.data_ptr(), cond_d.data_ptr(), par_d.data_ptr(), dst.data_ptr(), B, H, W, k, ws.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        assert _bits(dst) == want and bool((both[(1 - half) * B:(2 - half) * B] == 7.0).all())


def test_entry_points_refuse_and_write_nothing():
    from hoig_amd import _lib as L
    B, H, W, k = 2, 4, 4, 2
    state = _dev(R.make_state())
    s0 = _bits(state)
    params = torch.full((B + 1, 8), 7, dtype=torch.int32, device='cuda')
    img, cond = torch.full((B, H, W, 3), 1.0, device='cuda'), torch.full((B, H, W, k), 2.0, device='cuda')
    out, g = torch.full((B, H, W, 3 + k), 3.0, device='cuda'), torch.full((B, H, W, 3 + k), 4.0, device='cuda')
    dimg, ws = torch.full((B, H, W, 3), 5.0, device='cuda'), torch.full((B * R.MAX_PARTS,), 6.0, device='cuda')
    s, p, i, c, o, gg, d, w = (t.data_ptr() for t in (state, params, img, cond, out, g, dimg, ws))
    for args in [(None, 0, B, H, W, p), (s + 4, 0, B, H, W, p), (s, 0, B, H, W, None), (s, 0, B, H, W, p + 4), (s, -1, B, H, W, p), (s, 3, B, H, W, p),
                 (s, 0, 0, H, W, p), (s, 0, B, -1, W, p), (s, 0, B, H, 0, p)]:
        assert _call('hoig_daug_draw', *args, _st()) == L.EINVAL, args
    assert _call('hoig_daug_tick', None, _st()) == L.EINVAL and _call('hoig_daug_tick', s + 4, _st()) == L.EINVAL
    for args in [(None, gg, 4), (s, None, 4), (s, gg + 2, 4), (s, gg, 0), (s, gg, -5)]:
        assert _call('hoig_daug_adapt', *args, _st()) == L.EINVAL, args
    for args in [(None, c, p, o), (i, None, p, o), (i, c, None, o), (i, c, p, None), (i + 2, c, p, o), (i, c, p + 4, o), (i, c, p, o + 1), (i, c, p, i),
                 (i, c, p, c)]:
        assert _call('hoig_daug_fwd', *args, B, H, W, k, w, _st()) == L.EINVAL, args
    for dims in [(0, H, W, k), (B, 0, W, k), (B, H, -1, k), (B, H, W, 0)]:
        assert _call('hoig_daug_fwd', i, c, p, o, *dims, w, _st()) == L.EINVAL and _call('hoig_daug_bwd', gg, p, d, *dims, w, _st()) == L.EINVAL
    assert _call('hoig_daug_fwd', i, c, p, o, B, H, W, k, None, _st()) == L.EINVAL and _call('hoig_daug_fwd', i, c, p, o, B, H, W, k, o, _st()) == L.EINVAL
    for args in [(None, p, d), (gg, None, d), (gg, p, None), (gg, p + 4, d), (gg, p, d + 3), (gg, p, gg)]:
        assert _call('hoig_daug_bwd', *args, B, H, W, k, w, _st()) == L.EINVAL, args
    assert _call('hoig_daug_bwd', gg, p, d, B, H, W, k, None, _st()) == L.EINVAL and _call('hoig_daug_bwd', gg, p, d, B, H, W, k, gg, _st()) == L.EINVAL
    torch.cuda.synchronize()
    assert _bits(state) == s0 and bool((params == 7).all())
    for t, v in ((img, 1.0), (cond, 2.0), (out, 3.0), (g, 4.0), (dimg, 5.0), (ws, 6.0)):
        assert bool((t == v).all())


# ------------------------------------------------------------------------------------------------ the autograd operator
@pytest.mark.parametrize('hw,B,k', [((6, 10), 3, 7), ((16, 16), 2, 16)], ids=str)
def test_augment_cat_under_autograd_gives_the_twins_gradient(hw, B, k):
    from hoig_amd import ops
    H, W = hw
    img, cond, g = _data(B, H, W, k, 9)
    params = _mixed_records(B, H, W, 41)
    x = _dev(img).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # (the backward runs on the stream of the forward)
        y = ops.augment_cat(x, _dev(cond), _dev(params))
        loss = (y * _dev(g)).sum()
    loss.backward()
    side.synchronize()
    torch.cuda.synchronize()
    assert _bits(y) == R.twin_fwd(img, cond, params).tobytes()
    assert _bits(x.grad) == R.twin_bwd(g, params).tobytes()
    with pytest.raises(RuntimeError, match='no gradient'):
        ops.augment_cat(x, _dev(cond), _dev(params), out=torch.empty_like(y))
    out = torch.empty_like(y)
    assert ops.augment_cat(x.detach(), _dev(cond), _dev(params), out=out) is out
    torch.cuda.synchronize()
    assert _bits(out) == _bits(y)


def test_augment_cat_with_p_zero_is_cat_channels_both_ways():
    from hoig_amd import ops
    B, H, W, k = 3, 9, 4, 16
    img, cond, g = _data(B, H, W, k, 13)
    params = R.twin_draw(R.make_state(step=3, p=0.0), 0, B, H, W)
    assert (params[:, 7] == 0).all()
    xa, xb = _dev(img).requires_grad_(True), _dev(img).requires_grad_(True)
    ya, yb = ops.augment_cat(xa, _dev(cond), _dev(params)), ops.cat_channels([xb, _dev(cond)])
    (ya * _dev(g)).sum().backward()
    (yb * _dev(g)).sum().backward()
    torch.cuda.synchronize()
    assert _bits(ya) == _bits(yb) and _bits(xa.grad) == _bits(xb.grad)


# ------------------------------------------------------------------------------------------------ Trainer
def _trainer(**over):
    from common import product_trainer
    return product_trainer(GEN, BATCH, SIDE, **over)


def _finite(m):
    return all(np.isfinite(v) for v in m.get_current_errors().values())


def test_trainer_without_the_option_is_the_parents(monkeypatch, tmp_path):
    from hoig_amd import _lib as L
    called = []
    real_call, real_attempt = L.call, L.attempt
    monkeypatch.setattr(L, 'call', lambda name, *a: (called.append(name), real_call(name, *a))[1])
    monkeypatch.setattr(L, 'attempt', lambda name, *a: (called.append(name), real_attempt(name, *a))[1])
    m = _trainer(checkpoints_dir=str(tmp_path))
    assert m._daug is None and m._daug_options is None
    m.optimize_parameters()
    m.optimize_parameters()
    m.save(1)
    assert called and not [n for n in called if n.startswith('hoig_daug')]
    assert 'hoig_cat2_channels' in called
    assert list(m.get_current_scalars()) == ['lr_G', 'lr_D']
    assert sorted(os.listdir(os.path.join(str(tmp_path), 't'))) == sorted(
        '%s_epoch_1_id_%s.pth' % (kind, tag) for kind in ('net', 'opt') for tag in 'GD')


def _records_follow_the_twin(m, steps):
    """After every step the three sites' buffers hold the twin's draws at the device's step index; -> the step indices seen."""
    seen = []
    for _ in range(steps):
        m.optimize_parameters()
        m._wait_g()
        m._wait_d()
        torch.cuda.synchronize()
        state = _host_state(m._daug.state)
        seen.append(int(state[R.STEP]))
        for site in (0, 1, 2):
            assert _bits(m._daug.params(site, BATCH)) == R.twin_draw(state, site, BATCH, SIDE, SIDE).tobytes(), (seen, site)
        assert _finite(m)
    return seen


@pytest.mark.parametrize('mode', ['eager_d_early', 'eager_d_late', 'captured'])
def test_trainer_fixed_p_draws_advance_with_the_step(mode):
    from hoig_amd import _lib as L
    prev = L.set_tuning('d_early', 0 if mode == 'eager_d_late' else 1)
    try:
        m = _trainer(d_augment='color,translation,cutout', d_augment_p=0.7, d_augment_seed=3, hip_graph=(mode == 'captured'))
        assert m._daug.names() == ['color', 'translation', 'cutout'] and not m._daug.adaptive
        assert _records_follow_the_twin(m, 4) == [1, 2, 3, 4]
        if mode == 'captured':
            assert any(g['graphs'] is not None for g in m._graphs.values()), 'the step was never captured'
        flags = m._daug.params(0, BATCH)[:, 7].cpu().tolist() + m._daug.params(1, BATCH)[:, 7].cpu().tolist()
        assert all(0 <= f < 8 for f in flags)
        sc = m.get_current_scalars()
        assert list(sc) == ['lr_G', 'lr_D', 'd_aug_p'] and sc['d_aug_p'] == 0.7
    finally:
        L.set_tuning('d_early', prev)


def test_trainer_adaptive_p_follows_the_python_controller():
    """interval 2, kimg 0.01 (an increment of 0.4): after 2 * interval steps d_aug_p is the Python controller's over the sign counts of
    the d_real the device's own steps produced."""
    interval, kimg = 2, 0.01
    m = _trainer(d_augment='color,cutout', d_augment_p='adaptive', d_augment_interval=interval, d_augment_kimg=kimg, d_augment_target=0.6)
    assert m._daug.adaptive and m.get_current_scalars()['d_aug_p'] == 0.0
    fed = []
    real = m._daug.adapt
    m._daug.adapt = lambda d: (fed.append(d.detach().clone()), real(d))[1]
    ctl = R.PyController(0.0, 0.6, interval, BATCH * interval / (kimg * 1000.0))
    for _ in range(2 * interval):
        m.optimize_parameters()
    m._wait_g()
    m._wait_d()
    torch.cuda.synchronize()
    assert len(fed) == 2 * interval
    for d in fed:
        ctl.feed(int((d > 0).sum()), int((d < 0).sum()), d.numel())
    sc = m.get_current_scalars()
    assert list(sc) == ['lr_G', 'lr_D', 'd_aug_p', 'd_aug_rt']
    assert sc['d_aug_p'] == ctl.p and sc['d_aug_rt'] == ctl.rt
    state = _host_state(m._daug.state)
    assert int(state[R.ADJUSTS]) == 2 and int(state[R.STEPS]) == 0 and int(state[R.STEP]) == 2 * interval
    assert R._w2f(state[R.INCREMENT]) == ctl.increment
    assert _finite(m)


def test_checkpoint_round_trip_restores_the_step_and_p(tmp_path, capsys):
    from common import opt_namespace
    from hoig_amd.models import ModelsFactory
    root = str(tmp_path)
    over = dict(d_augment='translation', d_augment_p='adaptive', d_augment_interval=2, d_augment_kimg=0.01, checkpoints_dir=root)
    a = _trainer(**over)
    for _ in range(3):
        a.optimize_parameters()
    a.save(1)
    torch.cuda.synchronize()
    assert 'opt_epoch_1_id_D_aug.pth' in os.listdir(os.path.join(root, 't'))
    sd = torch.load(os.path.join(root, 't', 'opt_epoch_1_id_D_aug.pth'))
    assert sd['step'] == 3 and sd['steps'] == 1 and sd['adjusts'] == 1 and sd['policy'] == ['translation'] and sd['adaptive'] is True
    b = ModelsFactory.get_by_name('trainer', opt_namespace(load_epoch=1, **over))
    torch.cuda.synchronize()
    keep = [R.STEP, R.P, R.POS, R.NEG, R.TOTAL, R.STEPS, R.RT, R.ADJUSTS, R.SEED, R.RANK, R.TARGET, R.INTERVAL, R.POLICY]
    assert (_host_state(b._daug.state)[keep] == _host_state(a._daug.state)[keep]).all()
    assert b._daug.state_dict()['p'] == sd['p'] and 'loaded augmentation state' in capsys.readouterr().out
    os.remove(os.path.join(root, 't', 'opt_epoch_1_id_D_aug.pth'))
    c = ModelsFactory.get_by_name('trainer', opt_namespace(load_epoch=1, **dict(over, d_augment_p=0.25)))
    said = capsys.readouterr().out
    assert 'no augmentation checkpoint' in said and 'opt_epoch_1_id_D_aug.pth' in said
    assert c._daug.state_dict()['step'] == 0 and c._daug.state_dict()['p'] == 0.25


def test_trainer_refuses_bad_options():
    from common import opt_namespace
    from hoig_amd.models import ModelsFactory
    with pytest.raises(ValueError, match='d_augment'):
        ModelsFactory.get_by_name('trainer', opt_namespace(d_augment='color,flip'))
    with pytest.raises(ValueError, match='d_augment_p'):
        ModelsFactory.get_by_name('trainer', opt_namespace(d_augment='color', d_augment_p=1.5))


# ------------------------------------------------------------------------------------------------ under a forced exchange
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_exchange(port, q):
    """A `nccl` group of one rank with the exchange forced on (as tests/test_ddp_rccl_gpu.py forces it): adaptive p is refused where the
    model is built; a fixed p runs, and its records are the twin's under the rank's key."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HOIG_DDP_FORCE='1',
                      HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    try:
        _trainer(use_ddp=True, d_augment='color', d_augment_p='adaptive')
        refused = None
    except ValueError as ex:
        refused = str(ex)
    m = _trainer(use_ddp=True, d_augment='color,cutout', d_augment_p=0.5)
    active = m._G.sync.active
    seen = _records_follow_the_twin(m, 2)
    q.put((refused, active, seen, m._daug.rank))
    dist.barrier()
    dist.destroy_process_group()


def test_adaptive_under_an_active_exchange_raises_and_fixed_p_runs():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_run_exchange, args=(_free_port(), q))
    p.start()
    refused, active, seen, rank = q.get(timeout=600)
    p.join(timeout=120)
    assert p.exitcode == 0
    assert active and refused is not None and 'adaptive' in refused and 'exchange' in refused
    assert seen == [1, 2] and rank == 0
