#!/usr/bin/env python
"""bench.py -- HOGAN G+D training-step throughput on synthetic 256x256 hand-object-pose tensors.

  python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]
      A plain run sets up, warms up, times the K steps and prints the headline line.  --full adds the other legs: the step in
      the other form (captured hipGraph / eager), host issue time, the dominant kernel's roofline, the generator-forward
      latency and the CPU baseline.  --dump-outputs DIR writes what the last timed step left its caller (loss terms, G's and
      D's parameters) as .npy files, so that two builds can be compared output for output; that step then starts from the
      seeded initial weights and optimiser state (restored outside the timed interval), so that it is the same in every run.
      N>1: one rank per GPU over RCCL.  Either the caller launches the ranks (`python -m torch.distributed.run
      --nproc-per-node N ... bench.py --gpus N ...`: RANK / LOCAL_RANK / WORLD_SIZE in the environment), or -- when
      WORLD_SIZE is not set -- this script starts that launcher itself as a CHILD process before touching the GPU and
      forwards rank 0's JSON line and the exit code.  Fewer than N visible GPUs is an error, never a silent 1-GPU run.

A "step" is one ``Trainer.optimize_parameters()`` (forward, G loss, backward, Adam(G), D loss, backward, Adam(D);
under DDP also the RCCL gradient exchange) on a per-GPU batch of 8 pairs (BASELINE.json configs[1]; weak scaling:
configs[2] is the same per-GPU batch on 8 GPUs).  Inputs are resident in HBM before the timed region.
Prints ONE JSON line on rank 0.
"""
import argparse
import contextlib
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)          # the product package only; tests/ + oracle/ are reachable from the cpu-baseline child alone

GFLOP_PER_PAIR_TRAIN_256 = 2555.2      # BASELINE.md §2 / SURVEY.md §8d (3*G + 3*VGG + 9*D), generator_spade_attn
PMC_FILES = ['r06_pmc_dominant_conv.json', 'r05_pmc_dominant_conv.json', 'r04_pmc_dominant_conv.json', 'r03_pmc_dominant_conv.json', 'r02_pmc_dominant_conv_f6.json', 'r02_pmc_dominant_conv.json', 'r01_pmc_dominant_conv.json']      # newest first (matched by kernel name below)
PEAK_F32, PEAK_16 = 157.3, 2500.0          # TFLOP/s dense MFMA (fp32 / fp16-bf16), MI355X_MICROARCH.md
DTYPE_NAMES = {'f16f6': 'fwd: fp16 hi*hi + the two cross terms of the hi/lo split on block-scaled fp6 MFMA (1.6 bf16-MFMA units per product; layers outside that kernel: three fp16 terms) / bwd: bf16x2 (dy split hi+lo, weights and x single bf16), f32 accumulate',
               'bf16x3:f16x2': 'f16x3 fwd (both operands split hi+lo on fp16, 3 MFMAs per product) / bf16x2 bwd (dy split hi+lo, weights and x single bf16, 2 MFMAs per product), f32 accumulate',
               'bf16x3': 'f16x3 fwd / bf16x3 bwd (both operands split hi+lo in 16-bit halves, 3 MFMAs per product, f32 accumulate)',
               'f16x2': 'f16x2 fwd / bf16x2 bwd (gathered operand split hi+lo, weights single 16-bit, 2 MFMAs per product, f32 accumulate)',
               'bf16': 'f16 fwd / bf16 bwd (single-pass 16-bit operands, f32 accumulate)', 'f32': 'f32 (v_mfma_f32_32x32x2_f32)'}
MFMA_TERMS = {'f16f6': 1.6, 'f32': 1, 'bf16x3': 3, 'f16x3': 3, 'f16x2': 2, 'bf16x2': 2, 'bf16': 1, 'f16': 1}      # issued MFMAs per algorithmic one


def _time_conv_launch(images, h, iters):
    """Average duration (ms) of ONE 3x3 stride-1 512->512 forward launch over `images` h x h maps: the kernel alone, HIP events on
    the launch stream, back-to-back launches on random data."""
    from hoig_amd import ops
    import types
    x = torch.randn(images, h, h, 512, device='cuda')
    w = ops.pack_weight(torch.randn(512, 512, 3, 3, device='cuda') * 0.02)
    # a weight outside a ParamTree has no version, so ops would re-split it on every call; give it a constant one so that
    # the timed loop launches the convolution kernel only (in the training step the split happens once per optimiser step)
    w._hoig_owner = types.SimpleNamespace(version=0, packed_planes=lambda w_, for_dgrad: None)
    for _ in range(10):
        ops.conv2d(x, w, None, 1, 1)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        ops.conv2d(x, w, None, 1, 1)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def dominant_kernel_roofline(batch, side, precision, iters=50):
    """The dominant kernel of the step is the 3x3 stride-1 512->512 convolution at side/8 (72 of ~260 conv calls of a
    forward, 44% of G's MACs).  The step launches it in TWO shapes (profiles/r04_conv_table.txt): 24 times
    over 2*batch images -- bg_model and obj_model process the src and the tsf batch STACKED -- and 30 times over batch images
    (src_model and tsf_model, separate weights, side by side on two streams, sized for half the chip each).  Both are timed
    here, alone; `achieved` is the kernel's average over the launches of a step (flops of the 24 + 30 launches / their time),
    so that the friendlier shape does not stand for the whole; each shape is listed under `launch_shapes`."""
    h = side // 8
    shapes = []
    for images, calls in ((2 * batch, 24), (batch, 30)):
        ms = _time_conv_launch(images, h, iters)
        flops = 2.0 * images * h * h * 512 * 512 * 9        # algorithmic: 2*M*N*K, M=images*h*h, N=512, K=9*512
        shapes.append(dict(images=images, calls_per_step=calls, avg_launch_ms=round(ms, 4), algorithmic_flop_per_launch=flops,
                           achieved=round(flops / (ms * 1e-3) / 1e12, 2)))
    batch2 = 2 * batch
    ms = shapes[0]['avg_launch_ms']
    flops_step = sum(sh['calls_per_step'] * sh['algorithmic_flop_per_launch'] for sh in shapes)
    ms_step = sum(sh['calls_per_step'] * sh['avg_launch_ms'] for sh in shapes)
    # HBM/fabric traffic of this kernel comes from separate rocprofv3 --pmc passes (FETCH_SIZE and WRITE_SIZE cannot
    # share a pass); the committed summary is attached when it was taken on the same kernel and shape
    traffic, traffic_source = None, None
    fwd_prec = precision.partition(':')[0]
    from hoig_amd import _lib
    m16 = True                                                   # the 8-row tilings run on v_mfma_f32_16x16x32 (conv_halo16.hip)
    halo = 'conv_halo3_m16_kernel'
    want = 'conv_halo3_f6_kernel' if fwd_prec == 'f16f6' else (halo if fwd_prec in ('bf16x3', 'f16x3') else None)
    for fn in PMC_FILES:
        try:
            pmc = json.load(open(os.path.join(ROOT, 'profiles', fn)))
        except Exception:
            continue
        if want and pmc.get('kernel_filter', 'conv_halo3_bf16_kernel') == want and batch2 == 16 and side == 256 and \
                'traffic_bytes_per_launch' in pmc:
            traffic = pmc['traffic_bytes_per_launch']
            traffic_source = ('profiles/%s: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this kernel on its %d-image '
                              'launch, committed; NOT measured in this run (counters cannot be read from inside the process)' % (fn, batch2))
            break
    achieved = flops_step / (ms_step * 1e-3) / 1e12
    fwd = precision.partition(':')[0]
    peak = PEAK_F32 if fwd == 'f32' else PEAK_16
    for sh in shapes:
        sh['frac'] = round(sh['achieved'] / peak, 4)
    nsx = {3: 2, 2: 3, 1: 1}[MFMA_TERMS[fwd]] if fwd not in ('f32', 'f16f6') else 0
    kname = ('igemm_f32_kernel' if fwd == 'f32' else 'conv_halo3_f6_kernel' if fwd == 'f16f6' else
             ('conv_halo3_m16_kernel<%d,4,2,128,true>' % nsx if m16 else 'conv_halo3_bf16_kernel<%d,4,2,128,2,true>' % nsx))
    return dict(bound='mfma', launch_mix='the EAGER step\'s: a captured step runs the 30 eight-image launches as 15 grouped launches over 16 images (tuning key pair = 2)',
                kernel='%s (conv3x3 s1 512->512 @%dx%d; per step 24 launches over %d images = src+tsf stacked and 30 over %d)'
                % (kname, h, h, batch2, batch),
                achieved=round(achieved, 2), peak=peak, unit='TFLOP/s', mfma_terms_per_product=MFMA_TERMS[fwd],
                frac=round(achieved / peak, 4), traffic=traffic, traffic_source=traffic_source,
                avg_launch_ms=round(ms_step / sum(sh['calls_per_step'] for sh in shapes), 4),
                algorithmic_flop_per_launch=flops_step / sum(sh['calls_per_step'] for sh in shapes), launch_shapes=shapes)


def gen_forward_latency(opt, batch, side, iters=10):
    """BASELINE.json's second headline: generator-only inference (`Trainer.forward` under no_grad in eval mode,
    eval.py:59-65), batch 32 at 256x256 (configs[4]); timed eagerly and as a captured hipGraph replay."""
    from hoig_amd import synthetic
    from hoig_amd.models import ModelsFactory
    opt.is_train = False
    opt.load_path = 'None'
    opt.load_epoch = -1
    from hoig_amd.models.trainer import Trainer
    model = Trainer.__new__(Trainer)          # eval.py would load a checkpoint; here: random-init weights (no files)
    from hoig_amd.models.base_model import BaseModel
    BaseModel.__init__(model, opt)
    model._name = 'Trainer'
    model.device = torch.device('cuda', torch.cuda.current_device())
    model._dexycb, model._world, model._side = False, 1, None
    with contextlib.redirect_stdout(sys.stderr):       # 'Network ... was created' banners: keep stdout to the JSON line
        model._init_create_networks(use_ddp=False)
    model._init_prefetch_inputs()
    model.set_eval()
    model.set_input(synthetic.make_inputs(batch, side, seed=8))
    out = {}
    with torch.no_grad():
        for _ in range(2):
            model.forward()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            model.forward()
        e.record()
        torch.cuda.synchronize()
        out['eager_ms_per_img'] = round(s.elapsed_time(e) / iters / batch, 4)
        try:
            from hoig_amd import ops
            graph = torch.cuda.CUDAGraph()
            with ops.graph_capture(graph):
                res = model.forward()
            graph.replay()
            torch.cuda.synchronize()
            s.record()
            for _ in range(iters):
                graph.replay()
            e.record()
            torch.cuda.synchronize()
            out['hipgraph_ms_per_img'] = round(s.elapsed_time(e) / iters / batch, 4)
            out['finite'] = bool(torch.isfinite(res[3]).all().item())
        except Exception as ex:          # report, do not hide
            out['hipgraph_error'] = repr(ex)[:200]
    out['batch'] = batch
    from hoig_amd import ops as _ops
    with torch.no_grad():
        with _ops.inference_forward_precision(getattr(opt, 'eval_precision', os.environ.get('HOIG_EVAL_PRECISION', 'f16f6'))) as switched:
            out['arithmetic'] = ('f16f6: 3x3 stride-1 layers on fp16 hi*hi + two block-scaled fp6 cross terms (1.6 MFMA units per product), the '
                                 'other layers on three fp16 terms; opt.eval_precision (no backward follows an eval.py forward)' if switched
                                 else 'the training forward\'s (%s)' % [k for k, v in _ops._PREC.items() if v == _ops.precision][0])
    out['gflop_per_img'] = 787.2 * (side / 256.0) ** 2
    best = out.get('hipgraph_ms_per_img', out['eager_ms_per_img'])
    out['tflops'] = round(out['gflop_per_img'] / best, 2)
    return out


DUMP_MAX_ELEMS = 6 << 20          # per parameter vector: 24 MB of float32; G and D together stay under 64 MB


def training_state(model):
    """(parameter tree, optimiser) of G and D: what a training step reads besides its batch and the frozen VGG."""
    return [(model._net(model._G), model._optimizer_G), (model._net(model._D), model._optimizer_D)]


def snapshot_state(model):
    return [tree.flat.clone() for tree, _ in training_state(model)]


def restore_state(model, snap):
    """Back to the state `snap` was taken in, before any optimiser step: the weights (their operand planes are re-made on the next
    step: version bump) and a fresh Adam (zero moments, step count 0, uploaded by the next step)."""
    for (tree, opt), flat in zip(training_state(model), snap):
        tree.flat.copy_(flat)
        tree.version += 1
        opt.exp_avg.zero_()
        opt.exp_avg_sq.zero_()
        opt.step_count = 0


def dump_outputs(out_dir, model, errors):
    """--dump-outputs: what the last timed step (`optimize_parameters`) hands its caller -- the loss terms of
    `get_current_errors()` (loss_<name>.npy, float64) and G's and D's parameters after their Adam updates (params_G.npy,
    params_D.npy, float32, the flat parameter buffers).  A buffer larger than DUMP_MAX_ELEMS is written as a fixed sample
    of its elements: DUMP_MAX_ELEMS positions drawn with a seeded generator (seed 0 for G, 1 for D), sorted."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    torch.cuda.synchronize()
    for k, v in errors.items():
        np.save(os.path.join(out_dir, 'loss_%s.npy' % k), np.array([v], dtype=np.float64))
    for seed, (tag, net) in enumerate((('G', model._G), ('D', model._D))):
        flat = model._net(net).flat.detach()
        if flat.numel() > DUMP_MAX_ELEMS:
            idx = torch.randint(flat.numel(), (DUMP_MAX_ELEMS,), generator=torch.Generator().manual_seed(seed))
            flat = flat[idx.sort().values.to(flat.device)]
        np.save(os.path.join(out_dir, 'params_%s.npy' % tag), flat.float().cpu().numpy())


def usable_cores():
    """Host cores this process may really use: scheduler affinity capped by the cgroup CPU quota (a thread pool
    sized from os.cpu_count() inside a quota-limited container oversubscribes badly)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        q, per = open('/sys/fs/cgroup/cpu.max').read().split()
        if q != 'max':
            n = min(n, max(1, int(int(q) / int(per))))
    except Exception:
        try:
            q = int(open('/sys/fs/cgroup/cpu/cpu.cfs_quota_us').read())
            per = int(open('/sys/fs/cgroup/cpu/cpu.cfs_period_us').read())
            if q > 0:
                n = min(n, max(1, q // per))
        except Exception:
            pass
    return max(1, n)


def cpu_baseline_worker(side, budget_s):
    """Child process (the only place tests/ and oracle/ are imported): the oracle = the reference's algorithm in fp32
    torch-CPU, on all usable host cores, per SURVEY.md §8(d): full G+D steps at `side`, batch 2 (>= 3 timed steps when the
    wall budget allows, never fewer than 1) after a 64x64 warm-up step, then the generator forward alone (eval, no_grad) at
    batch 4.  One JSON line per finished leg, so the parent can use whatever completed inside its timeout."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from common import oracle_trainer
    cores = usable_cores()
    torch.set_num_threads(cores)
    t_start = time.time()
    warm = oracle_trainer('generator_spade_attn', 1, 64)
    warm.optimize_parameters()
    del warm
    batch = 2
    ot = oracle_trainer('generator_spade_attn', batch, side)
    times = []
    while len(times) < 3:
        t0 = time.time()
        ot.optimize_parameters()
        times.append(time.time() - t0)
        print(json.dumps(dict(leg='train', seconds=times, cores=cores, side=side, batch=batch)), flush=True)
        if time.time() - t_start + 1.3 * max(times) > budget_s:
            break
    del ot
    if time.time() - t_start < budget_s:
        of = oracle_trainer('generator_spade_attn', 4, side)
        with torch.no_grad():
            t0 = time.time()
            of.forward()
            print(json.dumps(dict(leg='fwd', seconds=time.time() - t0, cores=cores, side=side, batch=4)), flush=True)


def cpu_baseline(side, budget_s=150):
    """The oracle (kind "port": pinned to the reference's own Python in the build container) timed on
    this box's host cores on a BOUNDED sample, in a child process under a hard timeout so the bench always finishes in
    minutes.  `value` = pairs per second of the full G+D step (median of the timed steps)."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), '--cpu-baseline-worker', str(side), '--cpu-budget', str(budget_s)]
    try:
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=budget_s + 120)
        lines = proc.stdout
    except subprocess.TimeoutExpired as ex:
        lines = ex.stdout.decode() if isinstance(ex.stdout, bytes) else (ex.stdout or '')
    train = fwd = None
    for ln in lines.strip().splitlines():
        try:
            r = json.loads(ln)
        except ValueError:
            continue
        if r.get('leg') == 'train':
            train = r
        elif r.get('leg') == 'fwd':
            fwd = r
    if train is None:
        return dict(value=None, unit='images/s', cores=usable_cores(), kind='port', sample='did not finish within the budget')
    ts = sorted(train['seconds'])
    med = ts[len(ts) // 2]
    out = dict(value=round(train['batch'] / med, 4), unit='images/s', cores=train['cores'], kind='port',
               sample='%d full G+D step(s) (optimize_parameters) of the oracle at %dx%d, batch %d, fp32 torch-CPU, after a '
                      '64x64 warm-up step: %s s per step (median used)' % (len(ts), side, side, train['batch'],
                                                                          ', '.join('%.1f' % t for t in train['seconds'])))
    if fwd is not None:
        out['gen_fwd_ms_per_img'] = round(fwd['seconds'] / fwd['batch'] * 1e3, 1)
        out['sample'] += '; generator forward (eval, no_grad) at batch %d: %.1f s' % (fwd['batch'], fwd['seconds'])
    return out


def _free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(args):
    """`python bench.py --gpus N` with N > 1 and no launcher around it: start `torch.distributed.run` as a child process
    (this parent has not initialised the GPU: device_count() does not), pass the arguments on, forward its output (rank 0
    prints the JSON line) and return its exit code."""
    import subprocess
    n_vis = torch.cuda.device_count()
    if n_vis < args.gpus and not args.dry_run_cpu:
        sys.stderr.write('bench.py: --gpus %d requested but only %d GPU(s) are visible; refusing to run a smaller job under '
                         'that label\n' % (args.gpus, n_vis))
        return 2
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(args.gpus),
           '--master-addr', '127.0.0.1', '--master-port', str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    return subprocess.call(cmd, env=env)


def dry_run_cpu(args, rank, world):
    """The N-rank protocol of the real run without a GPU (gloo): W untimed + K timed "steps" (rank r sleeps (r + 1) ms: the slowest
    rank must set the time), barriers on both sides, MAX over ranks, ONE JSON line on rank 0 -- labelled, with no throughput in it."""
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group(backend='gloo')
    step = lambda: time.sleep(1e-3 * (rank + 1))
    barrier = (lambda: dist.barrier()) if world > 1 else (lambda: None)
    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if rank == 0:
        print(json.dumps({'metric': 'DRY RUN (no GPU work): launcher / barrier / max-over-ranks protocol only', 'value': None,
                          'unit': None, 'dry_run': True, 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
                          'ms_per_step': round(dt / max(1, args.steps) * 1e3, 3), 'scaling': 'weak', 'data': 'none',
                          'config': {'workload': 'sleep((rank + 1) ms) per step', 'parallelism': 'dp%d' % world}}))
    if world > 1:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--batch', type=int, default=8, help='pairs per GPU')
    ap.add_argument('--side', type=int, default=256)
    ap.add_argument('--gen_name', default='generator_spade_attn')
    ap.add_argument('--dataset', default='hov3', choices=['hov3', 'dexycb'], help='channel configuration (config C4 = dexycb at --side 512 --batch 4)')
    ap.add_argument('--precision', default=os.environ.get('HOIG_PRECISION', 'bf16x3:f16x2'),
                    help="'<forward>[:<data gradient>[:<weight gradient>]]' of f32 | bf16x3 | f16x2 | bf16; f16f6 = forward on fp16 + block-scaled fp6 terms, backward f16x2: "
                         "faster, outputs inside 1e-3, but its worst gradient tensor exceeds 3e-2 at 256x256 (profiles/r03_grad_parity_256.txt), so it is opt-in (hoig_amd/ops.py set_precision)")
    ap.add_argument('--full', action='store_true',
                    help='after the headline: the comparison leg in the other step form, host issue time, the dominant kernel\'s roofline, '
                         'the generator-forward latency and the CPU baseline (the options below that name these legs apply to it)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write the loss terms and G\'s and D\'s parameters after the last timed step to DIR/<name>.npy (see dump_outputs)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--graph', action='store_true', help='time the step as a replayed hipGraph (default: issued kernel by kernel on its streams, which is faster on this ROCm: DESIGN.md section 3c)')
    ap.add_argument('--graph-steps', type=int, default=20, help='--full: steps of the comparison leg in the OTHER form (captured if the main run is eager, and vice versa); 0 = skip')
    ap.add_argument('--no-gen-fwd', action='store_true')
    ap.add_argument('--host-samples', type=int, default=5, help='--full: warmed samples of the host issue time per step (median reported); 0 = one plain step (profiling runs)')
    ap.add_argument('--fwd-batch', type=int, default=32, help='batch of the generator-forward latency leg')
    ap.add_argument('--cpu-baseline-worker', type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument('--cpu-budget', type=int, default=150, help='wall seconds the CPU-baseline child may use')
    ap.add_argument('--dry-run-cpu', action='store_true',
                    help='no GPU work: run the launcher / rank / barrier / max-over-ranks / rank-0-JSON protocol over gloo with a sleep '
                         'as the "step" (tests/test_host_cpu.py); the line it prints is labelled a dry run and carries no throughput')
    args = ap.parse_args()
    if args.cpu_baseline_worker:
        return cpu_baseline_worker(args.cpu_baseline_worker, args.cpu_budget)
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(self_launch(args))

    rank = int(os.environ.get('RANK', 0))
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    if world != args.gpus:
        sys.exit('bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks' % (args.gpus, world))
    if args.dry_run_cpu:
        return dry_run_cpu(args, rank, world)
    if torch.cuda.device_count() <= local_rank:
        sys.exit('bench.py: rank %d has no GPU (%d visible)' % (rank, torch.cuda.device_count()))
    ddp = world > 1
    torch.cuda.set_device(local_rank)
    if ddp:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group(backend='nccl', device_id=torch.device('cuda', local_rank))

    from hoig_amd import ops, synthetic
    from hoig_amd.models import ModelsFactory
    from hoig_amd.options import opt_namespace
    ops.set_precision(args.precision)

    opt = opt_namespace(gen_name=args.gen_name, local_rank=local_rank, image_size=args.side, dataset_mode=args.dataset,
                        hip_graph=bool(args.graph))
    torch.manual_seed(8)
    with contextlib.redirect_stdout(sys.stderr):       # the reference-style construction banners go to stderr
        model = ModelsFactory.get_by_name('trainer', opt, use_ddp=ddp)
    model.set_train()
    inputs = synthetic.make_inputs(args.batch, args.side, seed=8 + rank, dataset=args.dataset)
    model.set_input(inputs)
    initial = snapshot_state(model) if args.dump_outputs else None
    torch.cuda.synchronize()

    def barrier():
        if ddp:
            dist.barrier()
        torch.cuda.synchronize()

    # untimed and not counted as warm-up: the eager iterations the trainer runs before it captures the step, and the capture
    from hoig_amd.models import trainer as trainer_mod
    if args.graph:
        for _ in range(trainer_mod._GRAPH_WARMUP + 1):
            model.optimize_parameters()
    for _ in range(args.warmup):
        model.optimize_parameters()
    barrier()
    paused = 0.0
    t0 = time.perf_counter()
    for i in range(args.steps):
        if initial is not None and i == args.steps - 1:
            # --dump-outputs: the last timed step starts from the seeded initial weights and a fresh optimiser.  Every step sums
            # in fp32 atomics (norm statistics, split weight gradients, loss reductions), so runs differ by rounding per step,
            # and training on -- Adam normalises tiny gradients to full-size updates -- grows that far beyond rounding: only a
            # step from a fixed state computes the same outputs from the same inputs in every run.  (Not timed.)
            barrier()
            tp = time.perf_counter()
            restore_state(model, initial)
            barrier()
            paused += time.perf_counter() - tp
        model.optimize_parameters()
    barrier()
    dt = time.perf_counter() - t0 - paused
    if ddp:
        t = torch.tensor([dt], device='cuda', dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    errors = model.get_current_errors()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, model, errors)
    is_captured = lambda: bool(model._graphs) and all(g['graphs'] is not None for g in model._graphs.values())
    main_captured = is_captured()

    def host_issue_ms(samples=args.host_samples):
        """Host time to issue ONE step on an idle device: the median of `samples` warmed steps, each bracketed by a barrier (one
        un-warmed sample right after switching the step form read 148.9 ms in round 3's driver run: VERDICT r3)."""
        if samples <= 0:
            barrier()
            t = time.perf_counter()
            model.optimize_parameters()
            dt_ = (time.perf_counter() - t) * 1e3
            barrier()
            return dt_
        ts = []
        for i in range(samples + 2):
            barrier()
            t = time.perf_counter()
            model.optimize_parameters()
            ts.append((time.perf_counter() - t) * 1e3)
        barrier()
        ts = sorted(ts[2:])
        return ts[len(ts) // 2]

    other_ms, other_host_ms, main_host_ms = None, None, None
    if args.full:
        if args.graph_steps > 0:                       # the same step in the other form, same process, same weights
            model._use_graph = not args.graph
            model.set_input(inputs)                    # (a captured step reads its inputs from staging buffers made by set_input)
            for _ in range(trainer_mod._GRAPH_WARMUP + 2):
                model.optimize_parameters()
            barrier()
            t1 = time.perf_counter()
            for _ in range(args.graph_steps):
                model.optimize_parameters()
            barrier()
            other_ms = (time.perf_counter() - t1) / args.graph_steps * 1e3
            other_host_ms = host_issue_ms()
            other_captured = is_captured()
            model._use_graph = bool(args.graph)
            model.set_input(inputs)
            for _ in range(trainer_mod._GRAPH_WARMUP + 2):      # back in the main form, warmed again
                model.optimize_parameters()
            barrier()
        main_host_ms = host_issue_ms()

    if rank == 0:
        ms = dt / args.steps * 1e3
        value = world * args.batch * args.steps / dt
        out = {
            'metric': 'HOGAN train images/sec at %dx%d' % (args.side, args.side),
            'value': round(value, 3), 'unit': 'images/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': round(ms, 3), 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
            'dtype': DTYPE_NAMES.get(args.precision, args.precision),
            'data': 'synthetic',
            'config': {'workload': '%dx%d %s-shaped synthetic, batch %d per GPU, G+D full step (%s, VGG19 '
                                   'surrogate weights)' % (args.side, args.side, 'HO3Dv3' if args.dataset == 'hov3' else 'DexYCB',
                                                           args.batch, args.gen_name),
                       'global_batch': world * args.batch, 'parallelism': 'dp%d' % world},
            'step_tflops': round(GFLOP_PER_PAIR_TRAIN_256 * (args.side / 256.0) ** 2 * value / 1e3, 2),
            'step_form': 'captured hipGraph replay' if main_captured else 'eager: kernels issued on the step\'s HIP streams',
            'losses_finite': all(v == v and abs(v) != float('inf') for v in errors.values()),
        }
        if args.full:
            roof = None if os.environ.get('HOIG_BENCH_NO_ROOF') else dominant_kernel_roofline(args.batch, args.side, args.precision)
            out.update({
                'host_ms_per_step_idle_device': round(main_host_ms, 2),
                'hipgraph': None if other_ms is None else {
                    'form': 'eager' if args.graph else 'captured hipGraph replay',
                    'captured_step': bool(other_captured) if not args.graph else main_captured,
                    'ms_per_step': round(other_ms, 3), 'value': round(world * args.batch / (other_ms * 1e-3), 3),
                    'host_ms_per_step_idle_device': round(other_host_ms, 2)},
                'roofline': roof,
            })
            model = None
            torch.cuda.empty_cache()
            if world == 1 and not args.no_gen_fwd:
                out['gen_fwd'] = gen_forward_latency(opt, args.fwd_batch, args.side)
            if world == 1 and not args.no_cpu_baseline:
                out['cpu_baseline'] = cpu_baseline(args.side, args.cpu_budget)
        print(json.dumps(out))
    if ddp:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
