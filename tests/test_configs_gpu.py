"""BASELINE.json's configurations at their REAL sizes on the GPU (configs[1], [3], [4]; configs[2] is [1] per rank under
RCCL: tests/test_ddp_rccl_gpu.py, tests/test_ddp_gpu.py).  The oracle is affordable on a slice of each (a CPU forward at
256x256 batch 2 or 512x512 batch 1 takes seconds); the full batch is then tied to that slice through properties that do not
depend on size: instance norm is per sample and every loss is a batch mean, so outputs of a sample do not depend on its batch
and the losses of a batch are the mean of the losses of its halves (models/trainer.py:436-474)."""
import numpy as np
import pytest
import torch

from common import oracle_trainer, product_trainer, SEEDS
from gpu_util import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-3                      # north_star: 1e-3 relative fp32 on the outputs


@pytest.fixture(autouse=True)
def _precision():
    from hoig_amd import ops
    ops.set_precision('bf16x3:f16x2')       # the benchmarked arithmetic (forward: three fp16 terms; backward: two bf16 terms)
    yield
    ops.set_precision('f32')


def _half(inputs, lo, hi):
    full = inputs['real_src'].shape[0]
    out = {}
    for k, v in inputs.items():
        if v.shape[0] == 2 * full:          # bg_mask / hand_mask: src then tsf
            out[k] = torch.cat([v[lo:hi], v[full + lo:full + hi]], 0).contiguous()
        else:
            out[k] = v[lo:hi].contiguous()
    return out


def _loss_tol(want):
    return 1e-3 * max(abs(want), 1e-2)


def test_config5_eval_forward_b32_hipgraph_replay():
    """configs[4]: eval.py's generator-only inference (eval.py:59-65: set_eval, forward under no_grad), 256x256, batch 32,
    captured in a hipGraph.  The replay must reproduce the eager forward (same kernels, same order; fp32 atomics in the
    instance-norm statistics and split-K epilogues make two runs agree to rounding, not bitwise; in the f16f6 arithmetic a
    last-bit difference of an activation can move an fp6 rounding of a cross term, so two runs differ by up to that arithmetic's
    own error against fp32 -- measured 3e-5 ... 2e-4 through the 45 conv + norm layers at 32 images, bound 5e-4; the parity
    statement is the oracle comparison below at TOL), must re-read its static
    input buffers (new inputs -> new outputs without re-capture), and its first sample must match the ORACLE's forward
    of that sample."""
    from hoig_amd import synthetic
    B, S = 32, 256
    first = synthetic.make_inputs(B, S, seed=SEEDS['inputs'])
    m = product_trainer('generator_spade_attn', B, S, inputs=first)
    m.set_eval()
    from hoig_amd import ops, _lib as L
    with torch.no_grad():
        with ops.inference_forward_precision(getattr(m._opt, 'eval_precision', 'f16f6')) as switched:
            assert switched and ops.precision == L.PREC_F16F6      # round 6: eval.py's forward runs on fp16 + fp6 cross terms by default
        assert ops.precision == L.PREC_BF16X3
        eager = [o.clone() for o in m.forward()]
        graph = torch.cuda.CUDAGraph()
        with ops.graph_capture(graph):
            outs = m.forward()
        graph.replay()
        torch.cuda.synchronize()
        r1 = [o.clone() for o in outs]
        graph.replay()
        torch.cuda.synchronize()
        r2 = [o.clone() for o in outs]
    for e, a, b in zip(eager, r1, r2):
        assert torch.isfinite(a).all()
        assert rel_err(a, e) < 5e-4 and rel_err(b, a) < 5e-4
    want = oracle_256_b1()[0]                                   # same per-sample seeds: sample 0 of the batch of 32
    for name, got, w in zip(['src_bg', 'tsf_bg', 'src_img', 'tsf_img'], r1[:4], want[:4]):
        assert rel_err(got[:1], w) < TOL, name
    assert rel_err(torch.cat([r1[4][:1], r1[4][B:B + 1]]), want[4]) < TOL        # masks: src then tsf along the batch
    assert rel_err(torch.cat([r1[5][:1], r1[5][B:B + 1]]), want[5]) < TOL
    # the graph reads the staged input buffers: overwrite them in place with another batch and replay
    # (another batch: the samples of this one rotated by one place along the batch -- every static buffer changes; generating 32 new
    # synthetic samples on the host took 10 s of this test)
    full = first['real_src'].shape[0]
    other = {k: (torch.cat([torch.roll(v[:full], 1, 0), torch.roll(v[full:], 1, 0)], 0) if torch.is_tensor(v) and v.shape[0] == 2 * full
                 else (torch.roll(v, 1, 0) if torch.is_tensor(v) else v)) for k, v in first.items()}
    with torch.no_grad():
        staged = dict(m._n)
        m.set_input(other)                       # allocates new buffers ...
        for k, v in m._n.items():                # ... copy their contents into the captured ones
            staged[k].copy_(v)
        m._n = staged
        graph.replay()
        torch.cuda.synchronize()
        assert rel_err(outs[3], r1[3]) > 1e-2                     # different inputs -> different images
        eager2 = m.forward()
        assert rel_err(outs[3], eager2[3]) < 2e-4


def test_config4_dexycb_512():
    """configs[3]: 512x512, DexYCB channels (bg 13, hand cond 9, D input 24, no arm mask).  Batch 1: forward against the
    oracle; batch 4 (the per-GPU batch): one full G+D step, finite, with losses equal to the mean over its two halves."""
    S = 512
    ot = oracle_trainer('generator_spade_attn', 1, S, dataset='dexycb')
    m = product_trainer('generator_spade_attn', 1, S, dataset='dexycb')
    with torch.no_grad():
        want, got = ot.forward(), m.forward()
    for a, b in zip(got, want):
        assert rel_err(a, b) < TOL
    del m, ot
    torch.cuda.empty_cache()
    _step_is_mean_of_halves(4, S, 'dexycb')


def _step_is_mean_of_halves(B, S, dataset):
    from hoig_amd import synthetic
    inputs = synthetic.make_inputs(B, S, seed=SEEDS['inputs'], dataset=dataset)
    losses = []
    for part in (inputs, _half(inputs, 0, B // 2), _half(inputs, B // 2, B)):
        m = product_trainer('generator_spade_attn', B, S, dataset=dataset, inputs=part)
        m.optimize_parameters()
        e = m.get_current_errors()
        assert all(np.isfinite(v) for v in e.values()), e
        assert torch.isfinite(m._G.flat).all() and torch.isfinite(m._D.flat).all()
        losses.append(e)
        del m
        torch.cuda.empty_cache()
    full, h0, h1 = losses
    for k in full:
        want = 0.5 * (h0[k] + h1[k])
        assert abs(full[k] - want) <= _loss_tol(want), (k, full[k], want)
    return full


_ORACLE_256 = {}


def oracle_256_b1():
    """(forward outputs, loss terms, gradients) of the ORACLE's step at 256 x 256 on sample 0 of the seeded batch: ~20 s of CPU, shared by
    the tests of this module."""
    if not _ORACLE_256:
        sys_path_tools()
        from precision_frontier import oracle_side
        _ORACLE_256['v'] = oracle_side(256, 1)
    return _ORACLE_256['v']


def test_config2_256_forward_and_step():
    """configs[1]: 256x256 HO3Dv3-shaped, batch 8, full G+D step.  The batch-8 forward against the oracle on its first sample (samples
    are seeded one by one: sample 0 of any batch is the oracle's batch of one; the oracle's losses and gradients at this size are
    compared in test_config2_gradients_256_against_oracle); batch 8: finite, and its losses are the mean of its halves' losses."""
    S, B = 256, 8
    want = oracle_256_b1()[0]
    from hoig_amd import ops
    ops.set_precision('bf16x3:f16x2')
    m = product_trainer('generator_spade_attn', B, S)
    with torch.no_grad():
        got = m.forward()
    for name, g, w in zip(['src_bg', 'tsf_bg', 'src_img', 'tsf_img'], got[:4], want[:4]):
        assert rel_err(g[:1], w) < TOL, name
    assert rel_err(torch.cat([got[4][:1], got[4][B:B + 1]]), want[4]) < TOL      # masks: src then tsf along the batch
    assert rel_err(torch.cat([got[5][:1], got[5][B:B + 1]]), want[5]) < TOL
    del m
    torch.cuda.empty_cache()
    _step_is_mean_of_halves(B, S, 'hov3')


def test_bench_line_contract():
    """bench.py's ONE JSON line (the driver's contract): the keys, the timed-step bookkeeping, the roofline object of the dominant
    kernel measured live, and the gen-fwd leg -- on a short --full run (2 timed steps, no CPU-baseline child)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--steps', '2', '--warmup', '1', '--full', '--no-cpu-baseline',
                        '--fwd-batch', '8', '--graph-steps', '2'], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['metric'].startswith('HOGAN train images/sec at 256') and d['unit'] == 'images/s'
    assert d['n_gpus'] == 1 and d['steps'] == 2 and d['warmup'] == 1 and d['higher_is_better'] is True
    assert d['scaling'] == 'weak' and d['vs_baseline'] is None and d['data'] == 'synthetic'
    assert abs(d['value'] - 8 / (d['ms_per_step'] * 1e-3)) < 0.02 * d['value']            # batch 8 pairs per step on one GPU
    assert 30 < d['value'] < 400
    assert 'workload' in d['config'] and 'model' not in d['config']
    rf = d['roofline']
    assert rf['bound'] == 'mfma' and rf['unit'] == 'TFLOP/s' and rf['peak'] == 2500.0
    assert abs(rf['frac'] - rf['achieved'] / rf['peak']) < 1e-3 and 0.05 < rf['frac'] < 0.334
    assert 'conv_halo3_m16_kernel' in rf['kernel']
    assert rf['traffic'] is None or rf['traffic_source']                                   # counters come from a committed pass
    assert d['hipgraph']['captured_step'] is True and d['hipgraph']['ms_per_step'] > 0 and d['step_form'].startswith('eager')
    assert d['gen_fwd']['finite'] and d['gen_fwd']['batch'] == 8 and d['losses_finite'] is True
    assert 'cpu_baseline' not in d or d['cpu_baseline'] is None or isinstance(d['cpu_baseline'], dict)


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain bench.py run (no --full) times its steps and prints the headline line only; --dump-outputs writes the last timed
    step's loss terms and G's and D's parameters as float32 / float64 .npy files, 64 MB at most."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--steps', '3', '--warmup', '1', '--dump-outputs',
                        str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['metric'].startswith('HOGAN train images/sec at 256') and d['unit'] == 'images/s' and d['higher_is_better'] is True
    assert d['steps'] == 3 and d['warmup'] == 1 and d['dtype'] and d['losses_finite'] is True
    assert abs(d['value'] - 8 / (d['ms_per_step'] * 1e-3)) < 0.02 * d['value']
    for k in ('roofline', 'hipgraph', 'gen_fwd', 'cpu_baseline', 'host_ms_per_step_idle_device'):
        assert k not in d, k
    files = sorted(os.listdir(str(tmp_path)))
    assert 'params_G.npy' in files and 'params_D.npy' in files and 'loss_g_rec.npy' in files and 'loss_d_fake.npy' in files
    total = 0
    for f in files:
        a = np.load(str(tmp_path / f))
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), f
        total += a.nbytes
    assert total <= 64 << 20
    assert np.abs(np.load(str(tmp_path / 'params_G.npy'))).max() > 0


def test_config2_gradients_256_against_oracle():
    """One G+D step at the bench resolution (256x256, batch 1: the oracle's step takes seconds): every gradient tensor of G and D
    against the CPU oracle, in the benchmarked arithmetic.  Measured (tools/grad_parity.py, profiles/r03_grad_parity_256.txt,
    4 runs): median 6.4e-3..6.6e-3, p95 8.5e-3..8.7e-3, worst 1.7e-2..2.2e-2 (an attention layer's 25-element bias); limits = the
    ones of the 128x128 test.  The opt-in 'f16f6' forward (fp6 cross terms on every eligible layer) is asserted on its OUTPUTS
    (1e-3) here and reported for its gradients: median 1.5e-2, p95 2.0e-2..2.4e-2, worst 2.7e-2..4.3e-2 -- beyond 3e-2, which is
    why it is not the default."""
    from hoig_amd import ops
    ofwd, oerr, ograd = oracle_256_b1()
    from conftest import want_gpu_slow
    modes = (('bf16x3:f16x2', (1e-2, 2e-2, 3e-2)),) + ((('f16f6', None),) if want_gpu_slow() else ())     # (the opt-in arithmetic's leg: opt-in)
    for mode, limits in modes:
        ops.set_precision(mode)
        old = ops.set_f6_min_tiles(1)
        try:
            m = product_trainer('generator_spade_attn', 1, 256)
            with torch.no_grad():
                fwd = m.forward()
            for a, b in zip(fwd, ofwd):
                assert rel_err(a, b) < TOL, mode
            m.optimize_parameters()
            e = m.get_current_errors()
            for k in oerr:
                assert abs(e[k] - oerr[k]) <= 1e-4 * max(abs(oerr[k]), 1e-2), (mode, k, e[k], oerr[k])
            vals = []
            for tag, net in (('G', m._G), ('D', m._D)):
                for k, v in net.export_dict(net.flat_grad).items():
                    if (tag, k) in ograd:
                        vals.append(float((v.detach().float().cpu() - ograd[(tag, k)]).norm() / ograd[(tag, k)].norm()))
            vals.sort()
            med, p95, worst = vals[len(vals) // 2], vals[int(0.95 * len(vals))], vals[-1]
            print('%s: gradient rel-L2 over %d tensors: median %.2e p95 %.2e worst %.2e' % (mode, len(vals), med, p95, worst))
            if limits is not None:
                assert med < limits[0] and p95 < limits[1] and worst < limits[2], (mode, med, p95, worst)
            else:
                assert med < 3e-2 and worst < 8e-2, (mode, med, worst)          # (sanity only: see the docstring)
            del m
            torch.cuda.empty_cache()
        finally:
            ops.set_f6_min_tiles(old)


def sys_path_tools():
    import os
    import sys
    p = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
    if p not in sys.path:
        sys.path.insert(0, p)


def test_eval_forward_with_and_without_the_loader_norm():
    """eval.py's forward (no_grad) with the single-reader IN -> ReLU -> conv3x3 chains fused into the consumer's loader (tuning key
    `norm_in`, default on; ops.conv2d_after_norm) against the same forward with every norm as a pass of its own: every output within
    1e-4 (a re-association of fp32 operations inside the 3-term arithmetic), and the fused forward launches fewer norm kernels."""
    from hoig_amd import _lib as L
    m = product_trainer('generator_spade_attn', 4, 256, eval_precision='same')      # (the loader norm sits in the three-term kernel)
    m.set_eval()
    outs = {}
    prev = L.set_tuning('norm_in', -1)
    try:
        for v in (0, 1):
            L.set_tuning('norm_in', v)
            with torch.no_grad():
                outs[v] = [o.clone() for o in m.forward()]
            torch.cuda.synchronize()
    finally:
        L.set_tuning('norm_in', prev)
    for a, b in zip(outs[1], outs[0]):
        assert torch.isfinite(a).all()
        assert rel_err(a, b) < 1e-4
