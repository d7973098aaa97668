"""The weight EMA on the device (docs/ema.md): the kernels against the CPU twins bit for bit (tests/test_ema_cpu.py pins the twins);
behind FusedAdam's three routes and under a guard; the swap scope; the Trainer's opt.ema_decay / opt.eval_ema in the eager, the
captured and the exchanged step; the checkpoint pair."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import ema_reference as R
import test_grad_guard_gpu as G          # (the small ParamTrees and step routes of the guard's tests)

pytestmark = pytest.mark.gpu
SIZES = R.SIZES + (4096 * 3 + 7,)
GEN, BATCH, SIDE = 'generator_spade_attn', 2, 64
DECAY = 0.9


def _call(name, *args):
    from hoig_amd import _lib as L
    return getattr(L.lib, name)(*args)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev_f32(a):
    """A device copy of a numpy float32 array, 16-byte aligned (the caching allocator hands out 512-byte multiples)."""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize('n', SIZES)
def test_kernels_equal_the_twins_bit_for_bit(n):
    """Five chained ticks and updates on the device and through the twins; then a step under a guard with skip = 1; `param` is never
    written."""
    rng = np.random.default_rng(2000 + n)
    ema_h = R.aligned_f32(n, R.values(rng, n))
    ema_d = _dev_f32(ema_h)
    state_h = np.array([0.999, 1.0, 0.0], dtype=np.float64)
    derived_h = np.zeros(1, dtype=np.float32)
    state_d, derived_d = torch.from_numpy(state_h.copy()).cuda(), torch.zeros(1, device='cuda')
    go = torch.tensor([0.5, 0.0], device='cuda')
    skip = torch.tensor([1.0, 1.0], device='cuda')
    for k in range(5):
        param_h = R.aligned_f32(n, R.values(rng, n))
        param_d = _dev_f32(param_h)
        guard = go if k % 2 else None
        assert _call('hoig_ema_tick', state_d.data_ptr(), derived_d.data_ptr(), R._ptr(guard), _st()) == 0
        assert _call('hoig_ema_update', ema_d.data_ptr(), param_d.data_ptr(), n, derived_d.data_ptr(), R._ptr(guard), _st()) == 0
        assert R.tick_host(state_h, derived_h) == 0 and R.update_host(ema_h, param_h, n, derived_h) == 0
        torch.cuda.synchronize()
        assert _bits(ema_d) == ema_h.tobytes(), (n, k)
        assert _bits(state_d) == state_h.tobytes() and _bits(derived_d) == derived_h.tobytes()
        assert _bits(param_d) == param_h.tobytes()
    assert _call('hoig_ema_tick', state_d.data_ptr(), derived_d.data_ptr(), skip.data_ptr(), _st()) == 0
    assert _call('hoig_ema_update', ema_d.data_ptr(), param_d.data_ptr(), n, derived_d.data_ptr(), skip.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert _bits(ema_d) == ema_h.tobytes() and _bits(state_d) == state_h.tobytes() and _bits(derived_d) == derived_h.tobytes()
    assert _bits(param_d) == param_h.tobytes()


def test_entry_points_refuse_and_leave_the_outputs():
    from hoig_amd import _lib as L
    n = 8
    ema, param = torch.full((n,), 1.0, device='cuda'), torch.full((n,), 2.0, device='cuda')
    big = torch.full((n + 4,), 3.0, device='cuda')
    derived = torch.tensor([0.5], device='cuda')
    state = torch.tensor([0.9, 1.0, 4.0], dtype=torch.float64, device='cuda')
    e, p, b, d = ema.data_ptr(), param.data_ptr(), big.data_ptr(), derived.data_ptr()
    assert e % 16 == 0 and p % 16 == 0 and b % 16 == 0
    for args in [(None, p, n, d), (e, None, n, d), (e, p, n, None), (e, p, 0, d), (e, p, -3, d), (b + 4, p, n, d), (e, b + 4, n, d),
                 (e, e, n, d), (b, b + 16, n, d)]:
        assert _call('hoig_ema_update', *args, None, _st()) == L.EINVAL, args
    assert _call('hoig_ema_tick', None, d, None, _st()) == L.EINVAL
    assert _call('hoig_ema_tick', state.data_ptr(), None, None, _st()) == L.EINVAL
    for args in [(None, p, n), (e, None, n), (e, p, 0), (e, p, -1), (e, e, n), (b, b + 16, n), (b + 16, b, n), (b + 4, p, n), (e, b + 4, n)]:
        assert _call('hoig_swap_f32', *args, _st()) == L.EINVAL, args
    torch.cuda.synchronize()
    assert bool((ema == 1.0).all()) and bool((param == 2.0).all()) and bool((big == 3.0).all())
    assert derived.item() == 0.5 and state.tolist() == [0.9, 1.0, 4.0]


@pytest.mark.parametrize('n', [1, 5, 4099])
def test_swap_exchanges_and_a_second_swap_restores(n):
    rng = np.random.default_rng(n)
    a_h, b_h = R.values(rng, n), R.values(rng, n)
    a, b = _dev_f32(a_h), _dev_f32(b_h)
    assert _call('hoig_swap_f32', a.data_ptr(), b.data_ptr(), n, _st()) == 0
    torch.cuda.synchronize()
    assert _bits(a) == b_h.tobytes() and _bits(b) == a_h.tobytes()
    assert _call('hoig_swap_f32', a.data_ptr(), b.data_ptr(), n, _st()) == 0
    torch.cuda.synchronize()
    assert _bits(a) == a_h.tobytes() and _bits(b) == b_h.tobytes()


# ------------------------------------------------------------------------------------------------ behind FusedAdam
STEPS = 5


def _grads(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(v, generator=g) for v in shapes.values()] for _ in range(STEPS)]


def _adam_route(tree, opt, route, guard=None):
    kw = dict(guard=guard) if guard is not None else {}
    opt.fuse_planes = route == 'fused'
    opt.step(ready=iter(G._slices(tree.flat.numel())) if route == 'slices' else None, **kw)


@pytest.mark.parametrize('nan_step', [None, 2], ids=['clean', 'nan_in_step_3'])
@pytest.mark.parametrize('which,route', [('small', 'two'), ('small', 'slices'), ('planes', 'fused'), ('planes', 'two'), ('planes', 'slices')])
def test_average_behind_the_adam_routes_is_the_twins_replay(which, route, nan_step):
    """Five steps on random gradients, update() behind each: the average is the twins' over the weights as they stood after every
    step.  With a NaN in step 3 under a 'skip' guard the average and its count are those of the four steps that happened."""
    from hoig_amd.ema import EmaWeights
    from hoig_amd.guard import GradGuard
    shapes = G.R.SMALL_SHAPES if which == 'small' else G.R.ADAM_SHAPES
    ref, _ = G._data(shapes, 5, 0.05)
    grads = _grads(shapes, 77)
    tree, opt = G._tree(shapes, ref, which == 'planes')
    guard = GradGuard(tree, policy='skip') if nan_step is not None else None
    if nan_step is not None:
        grads[nan_step][1].view(-1)[1] = float('nan')
    ema = EmaWeights(tree, 0.999)
    torch.cuda.synchronize()
    ema0, clones = ema.ema.cpu(), []
    assert torch.equal(ema0, tree.flat.cpu())
    for gs in grads:
        G._set_grads(tree, gs)
        _adam_route(tree, opt, route, guard)
        ema.update(guard=guard)
        torch.cuda.synchronize()
        clones.append(tree.flat.cpu())
    skipped = () if nan_step is None else (nan_step,)
    want, count = R.replay(ema0, clones, 0.999, True, skipped=skipped)
    assert torch.equal(ema.ema.cpu(), want)
    assert ema.updates() == count == STEPS - len(skipped)
    if nan_step is not None:
        assert torch.equal(clones[nan_step], clones[nan_step - 1]) and guard.report()['skipped'] == 1
        four, _ = R.replay(ema0, [c for i, c in enumerate(clones) if i != nan_step], 0.999, True)
        assert torch.equal(want, four)
    assert not torch.equal(want, ema0) and bool(torch.isfinite(want).all())


# ------------------------------------------------------------------------------------------------ swapped()
def _planes_of(tree, name):
    hi, lo = tree.packed_planes(tree.P[name], False)
    torch.cuda.synchronize()
    return hi.clone(), lo.clone()


def test_swapped_scope(monkeypatch):
    from hoig_amd import ops
    from hoig_amd.ema import EmaWeights
    shapes = G.R.ADAM_SHAPES
    ref, _ = G._data(shapes, 3, 0.05)
    tree, opt = G._tree(shapes, ref, True)
    ema = EmaWeights(tree, 0.5, warmup=False)
    for gs in _grads(shapes, 11)[:2]:
        G._set_grads(tree, gs)
        opt.step()
        ema.update()
    torch.cuda.synchronize()
    weights, avg = tree.flat.clone(), ema.ema.clone()
    assert not torch.equal(weights, avg)
    planes_w = _planes_of(tree, 'a.weight')
    fresh, _ = G._tree(shapes, {k: v.cpu() for k, v in ema.state_dict().items()}, True)
    assert torch.equal(fresh.flat, avg)
    planes_avg = _planes_of(fresh, 'a.weight')
    assert not torch.equal(planes_w[0], planes_avg[0])

    def restored():
        torch.cuda.synchronize()
        got = _planes_of(tree, 'a.weight')
        return (torch.equal(tree.flat, weights) and torch.equal(ema.ema, avg) and not ema.active and torch.equal(got[0], planes_w[0])
                and torch.equal(got[1], planes_w[1]))

    version = tree.version
    with ema.swapped() as inside:
        assert inside is ema and ema.active and tree.version == version + 1
        torch.cuda.synchronize()
        assert torch.equal(tree.flat, avg) and torch.equal(ema.ema, weights)
        got = _planes_of(tree, 'a.weight')
        assert torch.equal(got[0], planes_avg[0]) and torch.equal(got[1], planes_avg[1])
        with pytest.raises(RuntimeError, match='already active'):
            with ema.swapped():
                pass
        with pytest.raises(RuntimeError, match='swapped'):
            ema.update()
        assert ema.active and torch.equal(tree.flat, avg)
    assert tree.version == version + 2 and restored()
    with pytest.raises(KeyError, match='from the body'):
        with ema.swapped():
            raise KeyError('from the body')
    assert restored()
    monkeypatch.setattr(ops, '_capture_depth', 1)          # (what ops.graph_capture() raises while a step is being captured)
    with pytest.raises(RuntimeError, match='captured'):
        with ema.swapped():
            pass
    monkeypatch.undo()
    assert restored()


# ------------------------------------------------------------------------------------------------ Trainer
def _snap(m):
    m._wait_g()
    torch.cuda.synchronize()
    return m._net(m._G).flat.cpu()


def _trainer(**over):
    """A seeded training Trainer whose average starts from the seeded weights (product_trainer loads them after construction)."""
    from common import product_trainer
    m = product_trainer(GEN, BATCH, SIDE, **over)
    if m._ema is not None:
        m._ema.reset()
    return m


def _steps_and_replay(m, steps):
    ema0 = m._ema.ema.cpu()
    snaps = []
    for _ in range(steps):
        m.optimize_parameters()
        snaps.append(_snap(m))
    want, count = R.replay(ema0, snaps, m._ema.decay, m._ema.warmup)
    assert not torch.equal(snaps[0], snaps[-1])
    return torch.equal(m._ema.ema.cpu(), want), count


def test_trainer_eager_average_is_the_twins_replay():
    m = _trainer(ema_decay=DECAY)
    g, d = m._net(m._G), m._net(m._D)
    assert m._ema.tree is g and m._ema.ema.numel() == g.flat.numel() != d.flat.numel()      # G only: D has no average
    same, count = _steps_and_replay(m, 3)
    assert same
    assert m._ema.updates() == count == 3
    assert list(m.get_current_scalars()) == ['lr_G', 'lr_D']


def test_trainer_without_the_option_is_the_parents(tmp_path):
    m = _trainer(checkpoints_dir=str(tmp_path))
    assert m._ema is None and m._ema_decay is None and m._eval_ema is False
    m.optimize_parameters()
    m.save(1)
    assert sorted(os.listdir(os.path.join(str(tmp_path), 't'))) == sorted(
        '%s_epoch_1_id_%s.pth' % (kind, tag) for kind in ('net', 'opt') for tag in 'GD')
    assert list(m.get_current_scalars()) == ['lr_G', 'lr_D']
    with pytest.raises(RuntimeError, match='ema_decay'):
        with m.ema_weights():
            pass


def test_trainer_refuses_bad_options():
    from common import opt_namespace
    from hoig_amd.models import ModelsFactory
    for bad in (1.0, -0.1, 'x'):
        with pytest.raises(ValueError, match='ema_decay'):
            ModelsFactory.get_by_name('trainer', opt_namespace(ema_decay=bad))
    with pytest.raises(ValueError, match='eval_ema'):
        ModelsFactory.get_by_name('trainer', opt_namespace(eval_ema=True))


def test_trainer_captured_step_advances_the_average_on_every_replay():
    """Two eager warm-up steps, the capture with its replay, one more replay: the average is the twins' over the four snapshots and the
    device's count is 4 -- no host call advances it."""
    m = _trainer(ema_decay=DECAY, hip_graph=True)
    same, count = _steps_and_replay(m, 4)
    assert any(g['graphs'] is not None for g in m._graphs.values()), 'the step was never captured'
    assert same
    assert m._ema.updates() == count == 4
    assert m._optimizer_G.step_count == 4


# ------------------------------------------------------------------------------------------------ checkpoints and the eval forward
# The control of test_eval_forward_runs_on_the_average: five eval forwards of the same loaded weights differ among themselves at this
# shape (the forward is not bit-reproducible from run to run), by at most this much in the measured runs (8.02e-06 and 9.24e-06: docs/ema.md;
# outputs lie in [-1, 1]).  The scope's forward may differ from the loaded model's by four times that.
CONTROL_MAX = 9.239e-06
_ckpt = {}


def _ckpt_run(root):
    """One run shared by the tests below: a training model with ema_decay and eval_ema takes two steps and saves; a fresh training
    model and a fresh eval-only model load the files; the forwards; then the models without the EMA pair."""
    if _ckpt:
        return _ckpt
    from common import SEEDS, opt_namespace
    from hoig_amd import synthetic
    from hoig_amd.models import ModelsFactory
    r = _ckpt
    a = _trainer(ema_decay=DECAY, eval_ema=True, checkpoints_dir=root)
    a.optimize_parameters()
    a.optimize_parameters()
    a.save(1)
    torch.cuda.synchronize()
    d = os.path.join(root, 't')
    r['files'] = sorted(os.listdir(d))
    avg = a._ema.ema.clone()
    sd_g, sd_e = torch.load(os.path.join(d, 'net_epoch_1_id_G.pth')), torch.load(os.path.join(d, 'net_epoch_1_id_G_ema.pth'))
    r['keys'] = (list(sd_g), list(sd_e))
    r['meta'] = torch.load(os.path.join(d, 'opt_epoch_1_id_G_ema.pth'))
    r['strict'] = a._net(a._G).import_dict(torch.empty_like(avg), sd_e, strict=True) is None
    r['label'] = 'net_epoch_1_id_G_ema.pth'.split('_')[2]
    inputs = synthetic.make_inputs(BATCH, SIDE, seed=SEEDS['inputs'])

    b = ModelsFactory.get_by_name('trainer', opt_namespace(checkpoints_dir=root, load_epoch=1, ema_decay=DECAY))
    torch.cuda.synchronize()
    r['resumed'] = (torch.equal(b._ema.ema, avg), b._ema.updates(), torch.equal(b._net(b._G).flat, a._net(a._G).flat))
    a.optimize_parameters()                               # one more step; b takes a's new weights and the same update
    a._wait_g()
    torch.cuda.synchronize()
    b._net(b._G).flat.copy_(a._net(a._G).flat)
    b._ema.update()
    torch.cuda.synchronize()
    r['continued'] = (torch.equal(b._ema.ema, a._ema.ema), b._ema.updates(), a._ema.updates())
    del b

    c = ModelsFactory.get_by_name('trainer', opt_namespace(checkpoints_dir=root, load_epoch=1, is_train=False, eval_ema=True))
    torch.cuda.synchronize()
    r['eval_only'] = (torch.equal(c._net(c._G).flat, avg), c._ema is None)
    c.set_input(inputs)
    c.set_eval()
    a.set_eval()
    with torch.no_grad():
        control = [c.forward()[3].clone() for _ in range(5)]
        before = (a._net(a._G).flat.clone(), a._ema.ema.clone())
        a._ema.load_state_dict(sd_e, r['meta']['updates'])        # (a has stepped since the save: give it the saved average back)
        in_scope = a.forward()[3].clone()
        torch.cuda.synchronize()
        r['scope_restores'] = torch.equal(a._net(a._G).flat, before[0]) and torch.equal(a._ema.ema, avg) and not a._ema.active
        a._eval_ema = False
        outside = a.forward()[3].clone()
        a._eval_ema = True
        with a.ema_weights():                                     # the explicit scope; forward() does not nest a second one
            explicit = a.forward()[3].clone()
    torch.cuda.synchronize()
    r['control'] = max(float((x - control[0]).abs().max()) for x in control[1:])
    r['forward'] = (float((in_scope - control[0]).abs().max()), float((in_scope - outside).abs().max()),
                    float((explicit - control[0]).abs().max()))
    print('eval forward: control %.3e; scope vs loaded %.3e, scope vs raw weights %.3e, explicit scope vs loaded %.3e'
          % ((r['control'],) + r['forward']))
    del c, a

    for f in ('net_epoch_1_id_G_ema.pth', 'opt_epoch_1_id_G_ema.pth'):
        os.remove(os.path.join(d, f))
    try:
        ModelsFactory.get_by_name('trainer', opt_namespace(checkpoints_dir=root, load_epoch=1, is_train=False, eval_ema=True))
        r['missing_eval'] = None
    except FileNotFoundError as ex:
        r['missing_eval'] = str(ex)
    import contextlib
    import io
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        e = ModelsFactory.get_by_name('trainer', opt_namespace(checkpoints_dir=root, load_epoch=1, ema_decay=DECAY))
    torch.cuda.synchronize()
    r['missing_train'] = (torch.equal(e._ema.ema, e._net(e._G).flat), e._ema.updates(), out.getvalue())
    return r


@pytest.fixture(scope='module')
def ckpt(tmp_path_factory):
    return _ckpt_run(str(tmp_path_factory.mktemp('ema_ckpt')))


def test_save_writes_the_ema_pair_in_the_reference_format(ckpt):
    assert ckpt['files'] == sorted(['%s_epoch_1_id_%s.pth' % (kind, tag) for kind in ('net', 'opt') for tag in ('G', 'D', 'G_ema')])
    assert ckpt['keys'][0] == ckpt['keys'][1] and ckpt['strict']
    assert ckpt['meta'] == dict(updates=2, decay=DECAY, warmup=True)
    assert ckpt['label'] == '1'


def test_a_resumed_run_continues_the_average(ckpt):
    assert ckpt['resumed'] == (True, 2, True)
    assert ckpt['continued'] == (True, 3, 3)


def test_an_eval_only_model_holds_the_saved_average_as_its_generator(ckpt):
    assert ckpt['eval_only'] == (True, True)


def test_a_missing_ema_file_is_an_error_in_eval_and_a_note_in_training(ckpt):
    assert ckpt['missing_eval'] is not None and 'net_epoch_1_id_G_ema.pth' in ckpt['missing_eval']
    same, updates, said = ckpt['missing_train']
    assert same and updates == 0 and 'no EMA checkpoint' in said and 'net_epoch_1_id_G_ema.pth' in said


def test_eval_forward_runs_on_the_average(ckpt):
    """Trainer.forward in eval mode with eval_ema against the eval-only model loaded from _G_ema.pth, same eval_precision.  Control:
    that loaded model's forward five times (code this change does not touch)."""
    vs_loaded, vs_raw, explicit = ckpt['forward']
    assert ckpt['scope_restores']
    assert vs_raw > 1e-2                                  # (the average is not the raw weights: warm-up decay 0.1, 0.18 at two updates)
    assert ckpt['control'] > 0.0, 'the control is bit-identical now: assert torch.equal instead of a tolerance'
    assert vs_loaded <= 4 * CONTROL_MAX and explicit <= 4 * CONTROL_MAX


# ------------------------------------------------------------------------------------------------ under a forced exchange
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_exchange(port, q):
    """A `nccl` group of one rank with the exchange forced on (as tests/test_ddp_rccl_gpu.py forces it): G's Adam runs slice by slice
    behind the all-reduce, and the update has to sit behind the LAST slice's."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HOIG_DDP_FORCE='1',
                      HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    m = _trainer(use_ddp=True, ema_decay=DECAY)
    active, slices = m._G.sync.active, len(m._G.sync.slices)
    same, count = _steps_and_replay(m, 2)
    q.put((active, slices, same, count, m._ema.updates()))
    dist.barrier()
    dist.destroy_process_group()


def test_average_under_a_forced_exchange_is_the_twins_replay():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_run_exchange, args=(_free_port(), q))
    p.start()
    active, slices, same, count, updates = q.get(timeout=600)
    p.join(timeout=120)
    assert p.exitcode == 0
    assert active and slices > 4
    assert same and count == updates == 2
