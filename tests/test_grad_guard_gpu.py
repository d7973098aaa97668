"""The gradient guard on the device (docs/grad_guard.md): the statistics and decision kernels through the cases, truths and limits of
tests/grad_guard_reference.py (tests/test_grad_guard_cpu.py runs the same ones on the CPU twins) and against the twins bit for bit;
the guarded Adam entry points over ParamTree + FusedAdam; the Trainer's opt.grad_guard."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import grad_guard_reference as R
from gpu_util import rel_err

pytestmark = pytest.mark.gpu
CASES = R.cases()


# ------------------------------------------------------------------------------------------------ statistics and decision
@pytest.mark.parametrize('nonfinite', [False, True], ids=['finite', 'nonfinite'])
@pytest.mark.parametrize('n,tname', [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_stats_kernels_against_fsum(n, tname, nonfinite):
    R.check_stats('cuda', n, tname, nonfinite)


@pytest.mark.parametrize('nonfinite', [False, True], ids=['finite', 'nonfinite'])
@pytest.mark.parametrize('n,tname', [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_stats_kernels_equal_the_twin_and_themselves(n, tname, nonfinite):
    R.check_device_equals_twin(n, tname, nonfinite)


def test_stats_kernels_do_not_depend_on_alignment():
    R.check_misaligned('cuda')


@pytest.mark.parametrize('name', sorted(R.REFUSED))
def test_stats_entry_point_refuses_and_leaves_the_outputs(name):
    R.check_refused('cuda', name)


def test_decide_kernel_is_the_twin_and_the_formula():
    R.check_decide('cuda')


# ------------------------------------------------------------------------------------------------ guarded Adam
LR, BETAS, STEPS = 2e-4, (0.5, 0.999), 3


def _data(shapes, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    ref = {k: torch.randn(v, generator=g) * scale for k, v in shapes.items()}
    grads = [[torch.randn(v, generator=g) for v in shapes.values()] for _ in range(STEPS)]
    return ref, grads


def _slices(n):
    """Three uneven (begin, end) ranges over n elements, cut at multiples of 4 (the parameters are 16-byte aligned)."""
    a, b = 4 * (n // 4 // 5), 4 * (n // 4 // 2 + 1)
    assert 0 < a < b < n
    return [(0, a), (a, b), (b, n)]


def _tree(shapes, ref, planes):
    from hoig_amd.nn import ParamTree, FusedAdam
    tree = ParamTree(shapes, torch.device('cuda'))
    tree.load_state_dict(ref)
    if planes:
        tree._ensure_plane_bufs()
        for b in tree._plane_bufs:          # (allocated uninitialised, and only the weights with planes are ever written)
            b.zero_()
        tree._refresh_planes()
        assert tree.fused_step_tables() is not None
    return tree, FusedAdam(tree, lr=LR, betas=BETAS)


def _set_grads(tree, gs):
    with torch.no_grad():
        for p_, gr in zip(tree.P.values(), gs):
            p_.grad.copy_(gr.cuda())


def _snapshot(tree, opt):
    """Everything a step may touch: parameters, both moments, the four operand planes, the device's step count."""
    torch.cuda.synchronize()
    planes = [b.clone() for b in tree._plane_bufs] if tree._plane_bufs else []
    return [tree.flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()] + planes + [opt._state.clone()]


def _same(a, b):
    """Bit for bit?  (prints which entries of the two snapshots differ)"""
    diff = [i for i, (x, y) in enumerate(zip(a, b)) if not torch.equal(x, y)]
    if diff or len(a) != len(b):
        print('snapshots differ at entries %s of %d / %d' % (diff, len(a), len(b)))
    return len(a) == len(b) and not diff


def _step(tree, opt, route, guard=None, grad_scale=1.0):
    """One step by route: 'fused' (update and planes in one launch), 'two' (update, then the planes), 'slices' (a ready iterator)."""
    kw = dict(guard=guard) if guard is not None else {}
    opt.fuse_planes = route == 'fused'
    opt.step(grad_scale=grad_scale, ready=iter(_slices(tree.flat.numel())) if route == 'slices' else None, **kw)
    if route == 'fused':
        assert tree._plane_version == tree.version
    tree._refresh_planes()


@pytest.mark.parametrize('which,route', [('small', 'two'), ('small', 'slices'), ('planes', 'fused'), ('planes', 'two'), ('planes', 'slices')])
def test_guarded_adam_on_clean_gradients_is_the_unguarded_step(which, route):
    """(a) guard = {1.0f, 0}: parameters, moments, planes and the step count of three guarded steps are the unguarded twin tree's bits."""
    from hoig_amd.guard import GradGuard
    shapes = R.SMALL_SHAPES if which == 'small' else R.ADAM_SHAPES
    ref, grads = _data(shapes, 17, 0.05)
    (t0, o0), (t1, o1) = _tree(shapes, ref, which == 'planes'), _tree(shapes, ref, which == 'planes')
    guard = GradGuard(t1, policy='skip', per_tensor=True)
    for gs in grads:
        _set_grads(t0, gs)
        _set_grads(t1, gs)
        _step(t0, o0, route, grad_scale=0.5)
        _step(t1, o1, route, guard=guard, grad_scale=0.5)
    assert _same(_snapshot(t0, o0), _snapshot(t1, o1))
    rep = guard.report()
    assert (rep['steps'], rep['skipped'], rep['clipped'], rep['nonfinite']) == (STEPS, 0, 0, 0)
    assert o1.step_count == STEPS == int(o1._state[4].item())
    want = 0.5 * float(torch.cat([g.double().flatten() for g in grads[-1]]).norm())
    assert abs(rep['norm'] - want) <= 1e-12 * want


def _adam64(ref, grads, max_norm=0.0):
    """float64 torch.optim.Adam (with clip_grad_norm_ when max_norm > 0) over `grads` -> (parameters, optimiser, steps that clipped)"""
    params = [v.double().clone().requires_grad_(True) for v in ref.values()]
    opt = torch.optim.Adam(params, lr=LR, betas=BETAS)
    fired = 0
    for gs in grads:
        for p, gr in zip(params, gs):
            p.grad = gr.double().clone()
        if max_norm > 0:
            fired += int(float(torch.nn.utils.clip_grad_norm_(params, max_norm)) > max_norm)
        opt.step()
    return params, opt, fired


def _against_adam64(tree, opt, shapes, params, opt_r):
    sd, osd, osr = tree.state_dict(), opt.state_dict(), opt_r.state_dict()
    for k, p in zip(shapes, params):
        assert rel_err(sd[k], p) < 1e-6
    for i in osr['state']:
        assert rel_err(osd['state'][i]['exp_avg'], osr['state'][i]['exp_avg']) < 1e-6
        assert rel_err(osd['state'][i]['exp_avg_sq'], osr['state'][i]['exp_avg_sq']) < 1e-6
        assert float(osd['state'][i]['step']) == float(osr['state'][i]['step'])


@pytest.mark.parametrize('which,route,name', [('small', 'two', 'b.weight'), ('small', 'slices', 'b.weight'), ('planes', 'fused', 'h.bias'),
                                              ('planes', 'two', 'h.bias')])
def test_guarded_adam_skips_a_nan_step(which, route, name):
    """(b) one NaN in a small tensor on step 2: that step touches nothing and does not count; the end state is float64 Adam's over the
    two clean gradients."""
    from hoig_amd.guard import GradGuard
    shapes = R.SMALL_SHAPES if which == 'small' else R.ADAM_SHAPES
    ref, grads = _data(shapes, 9)
    bad = [g.clone() for g in grads[1]]
    bad[list(shapes).index(name)].view(-1)[1] = float('nan')
    tree, opt = _tree(shapes, ref, which == 'planes')
    guard = GradGuard(tree, policy='skip', per_tensor=True)
    _set_grads(tree, grads[0])
    _step(tree, opt, route, guard=guard)
    before = _snapshot(tree, opt)
    _set_grads(tree, bad)
    _step(tree, opt, route, guard=guard)
    assert _same(before, _snapshot(tree, opt))
    rep = guard.report()
    assert rep['skipped'] == 1 and rep['steps'] == 2 and rep['nonfinite'] == 1
    assert int(opt._state[4].item()) == 1 and opt.step_count == 1
    assert all(float(s['step']) == 1.0 for s in opt.state_dict()['state'].values())
    rows = guard.per_tensor()
    assert [k for k, r in rows.items() if r[2]] == [name] and rows[name][2] == 1
    _set_grads(tree, grads[2])
    _step(tree, opt, route, guard=guard)
    params, opt_r, _ = _adam64(ref, [grads[0], grads[2]])
    _against_adam64(tree, opt, shapes, params, opt_r)
    assert guard.report()['skipped'] == 1 and opt.step_count == 2


@pytest.mark.parametrize('which,route', [('small', 'two'), ('small', 'slices'), ('planes', 'fused')])
def test_guarded_adam_clips_to_max_norm(which, route):
    """(c) max_norm between the smallest and the largest of the three gradient norms: float64 clip_grad_norm_ + Adam."""
    from hoig_amd.guard import GradGuard
    shapes = R.SMALL_SHAPES if which == 'small' else R.ADAM_SHAPES
    ref, grads = _data(shapes, 23)
    grads = [[g * s for g in gs] for gs, s in zip(grads, (0.5, 3.0, 1.0))]
    norms = sorted(float(torch.cat([g.double().flatten() for g in gs]).norm()) for gs in grads)
    max_norm = 0.5 * (norms[0] + norms[1])
    tree, opt = _tree(shapes, ref, which == 'planes')
    guard = GradGuard(tree, policy='watch', max_norm=max_norm)
    for gs in grads:
        _set_grads(tree, gs)
        _step(tree, opt, route, guard=guard)
    params, opt_r, fired = _adam64(ref, grads, max_norm)
    assert fired == 2
    _against_adam64(tree, opt, shapes, params, opt_r)
    rep = guard.report()
    assert rep['clipped'] == fired and rep['skipped'] == 0 and rep['steps'] == STEPS
    assert abs(rep['norm_peak'] - norms[2]) <= 1e-12 * norms[2]


def test_a_skipped_fused_step_does_not_mark_stale_planes_current():
    """A two-launch step leaves the planes stale; a fused guarded step that the device then SKIPS writes no plane, so it must not
    mark them current: the next refresh re-packs them from the weights.  After a fused step over current planes they stay current."""
    from hoig_amd.guard import GradGuard
    shapes = R.ADAM_SHAPES
    ref, grads = _data(shapes, 13)
    tree, opt = _tree(shapes, ref, True)
    guard = GradGuard(tree, policy='skip')
    _set_grads(tree, grads[0])
    opt.fuse_planes = False
    opt.step(guard=guard)                           # (two launches, no refresh: the planes are those of the old weights)
    assert tree._plane_version != tree.version
    bad = [g.clone() for g in grads[1]]
    bad[6].view(-1)[0] = float('nan')
    _set_grads(tree, bad)
    opt.fuse_planes = True
    opt.step(guard=guard)                           # (skipped on the device)
    assert tree._plane_version != tree.version
    tree._refresh_planes()
    got = [b.clone() for b in tree._plane_bufs]
    fresh, _ = _tree(shapes, {k: v.cpu() for k, v in tree.state_dict().items()}, True)
    torch.cuda.synchronize()
    assert torch.equal(fresh.flat, tree.flat) and _same(got, [b for b in fresh._plane_bufs])
    assert guard.report()['skipped'] == 1
    _set_grads(tree, grads[2])
    opt.step(guard=guard)                           # (taken, over current planes: the launch wrote the new ones)
    assert tree._plane_version == tree.version
    got = [b.clone() for b in tree._plane_bufs]
    tree._plane_version = -1
    tree._refresh_planes()
    torch.cuda.synchronize()
    assert _same(got, list(tree._plane_bufs))


def test_a_learning_rate_upload_keeps_the_device_step_count():
    """The host counts a guarded step as taken; the device skipped it.  A new learning rate must go up with the device's count."""
    from hoig_amd.guard import GradGuard
    shapes = R.SMALL_SHAPES
    ref, grads = _data(shapes, 31)
    tree, opt = _tree(shapes, ref, False)
    guard = GradGuard(tree, policy='skip')
    bad = [g.clone() for g in grads[1]]
    bad[0].view(-1)[0] = float('inf')
    for gs in (grads[0], bad):
        _set_grads(tree, gs)
        _step(tree, opt, 'two', guard=guard)
    assert opt.step_count == 2                      # (the host's assumption, until it is reconciled)
    opt.param_groups[0]['lr'] = 1e-4
    _set_grads(tree, grads[2])
    _step(tree, opt, 'two', guard=guard)
    torch.cuda.synchronize()
    assert opt._state.tolist()[0] == 1e-4 and int(opt._state[4].item()) == 2
    assert guard.report()['skipped'] == 1 and opt.step_count == 2


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_exchange(port, q):
    """A `nccl` group of one rank with the exchange forced on (as tests/test_ddp_rccl_gpu.py forces it): the guarded step behind
    GradSync.iter_all_reduce against the guarded step over the same slices without an exchange."""
    import torch.distributed as dist
    from hoig_amd.ddp import GradSync
    from hoig_amd.guard import GradGuard
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    shapes = R.ADAM_SHAPES
    ref, grads = _data(shapes, 41)
    grads[1][6].view(-1)[2] = float('nan')          # (h.bias, step 2: skipped on both sides)
    grads[2] = [g * 4.0 for g in grads[2]]          # (step 3 clips)
    max_norm = 1.5 * float(torch.cat([g.double().flatten() for g in grads[0]]).norm())
    (t0, o0), (t1, o1) = _tree(shapes, ref, True), _tree(shapes, ref, True)
    n = t0.flat.numel()
    sync = GradSync(t1.flat, t1.flat_grad, bucket_bytes=4 * 4 * (n // 4 // 3 + 1), force=True)
    assert sync.active and len(sync.slices) == 3
    g0 = GradGuard(t0, policy='skip', max_norm=max_norm, per_tensor=True)
    g1 = GradGuard(t1, policy='skip', max_norm=max_norm, per_tensor=True)
    for gs in grads:
        _set_grads(t0, gs)
        _set_grads(t1, gs)
        o0.step(grad_scale=1.0 / sync.world, ready=iter(sync.slices), guard=g0)
        o1.step(grad_scale=1.0 / sync.world, ready=sync.iter_all_reduce(), guard=g1)
    same = _same(_snapshot(t0, o0), _snapshot(t1, o1)) and torch.equal(g0.record, g1.record) and torch.equal(g0._seg_out, g1._seg_out)
    q.put((same, dict(g1.report()), o1.step_count))
    dist.barrier()
    dist.destroy_process_group()


def test_guarded_adam_under_a_forced_exchange_equals_the_plain_guarded_step():
    """(d) the exchange is drained, the reduced buffer observed, the slices updated: bit for bit the guarded step without an exchange."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_run_exchange, args=(_free_port(), q))
    p.start()
    same, rep, count = q.get(timeout=300)
    p.join(timeout=120)
    assert p.exitcode == 0
    assert same
    assert (rep['steps'], rep['skipped'], rep['clipped']) == (3, 1, 1) and count == 2


# ------------------------------------------------------------------------------------------------ Trainer
GEN, BATCH, SIDE = 'generator_spade_attn', 2, 64


def test_trainer_skips_a_non_finite_generator_step():
    from common import product_trainer
    m = product_trainer(GEN, BATCH, SIDE, grad_guard='skip')
    g, d, og = m._net(m._G), m._net(m._D), m._optimizer_G
    torch.cuda.synchronize()
    before = [g.flat.clone(), og.exp_avg.clone(), og.exp_avg_sq.clone()]
    d_before = d.flat.clone()
    keep = m._opt.lambda_rec
    m._opt.lambda_rec = float('inf')        # non-finite values arise as gradient VALUES only: no kernel derives an address from them
    m.optimize_parameters()
    torch.cuda.synchronize()
    assert _same(before, [g.flat, og.exp_avg, og.exp_avg_sq])
    sc = m.get_current_scalars()
    assert sc['skipped_G'] == 1 and sc['skipped_D'] == 0
    assert not torch.equal(d_before, d.flat) and bool(torch.isfinite(d.flat).all())
    m._opt.lambda_rec = keep
    m.optimize_parameters()
    torch.cuda.synchronize()
    assert not torch.equal(before[0], g.flat) and bool(torch.isfinite(g.flat).all())
    assert float(og.state_dict()['state'][0]['step']) == 1.0
    assert float(m._optimizer_D.state_dict()['state'][0]['step']) == 2.0
    sc = m.get_current_scalars()
    assert sc['skipped_G'] == 1 and np.isfinite(sc['grad_norm_G']) and sc['grad_norm_G'] > 0 and sc['grad_max_G'] > 0


def test_trainer_without_the_option_is_unchanged():
    from common import product_trainer
    m = product_trainer(GEN, BATCH, SIDE)
    assert list(m.get_current_scalars()) == ['lr_G', 'lr_D']
    assert m._guards == {}
    with pytest.raises(RuntimeError):
        m.grad_report()


def test_trainer_refuses_an_unknown_policy():
    from common import product_trainer
    with pytest.raises(ValueError, match='bogus'):
        product_trainer(GEN, BATCH, SIDE, grad_guard='bogus')
    with pytest.raises(ValueError, match='max_grad_norm'):
        product_trainer(GEN, BATCH, SIDE, max_grad_norm_G=1.0)


_captured = {}


def _captured_run():
    """hip_graph=True with the guard on and per-tensor rows, clean data: two eager steps plus two replays (run once, shared)."""
    if not _captured:
        from common import product_trainer
        m = product_trainer(GEN, BATCH, SIDE, hip_graph=True, grad_guard='skip', grad_stats_per_tensor=True)
        for _ in range(4):
            m.optimize_parameters()
        torch.cuda.synchronize()
        _captured.update(captured=any(g['graphs'] is not None for g in m._graphs.values()),
                         reports={k: v.report() for k, v in m._guards.items()},
                         steps=[float(o.state_dict()['state'][0]['step']) for o in (m._optimizer_G, m._optimizer_D)],
                         rows=m.grad_report(), names=m._net(m._G).ref_names(), scalars=m.get_current_scalars())
    return _captured


def test_trainer_guard_in_the_captured_step():
    r = _captured_run()
    assert r['captured'], 'the step was never captured'
    for tag in ('G', 'D'):
        assert r['reports'][tag]['steps'] == 4 and r['reports'][tag]['skipped'] == 0 and r['reports'][tag]['nonfinite'] == 0
    assert r['steps'] == [4.0, 4.0]
    assert set(r['scalars']) == {'lr_G', 'lr_D'} | {k + t for k in ('grad_norm_', 'grad_max_', 'skipped_', 'clipped_') for t in 'GD'}


def test_trainer_per_tensor_rows_add_up_to_the_global_norm():
    r = _captured_run()
    rows = r['rows']['G']
    assert list(rows) == r['names']
    total = float(np.sqrt(np.sum(np.array([v[0] for v in rows.values()], dtype=np.float64) ** 2)))
    want = r['reports']['G']['norm']
    assert want > 0 and abs(total - want) <= 1e-12 * want
    assert max(v[1] for v in rows.values()) == r['reports']['G']['max']
