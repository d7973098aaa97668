"""The gradient guard's cost (docs/grad_guard.md): GradGuard.observe() -- hoig_grad_stats (two launches) + hoig_guard_decide -- timed alone
on the generator's and the discriminator's gradient buffers of the 256 x 256 batch-8 step, next to the byte floor (4 bytes per element
at the 4.7 TB/s the Adam kernel reaches), and the whole step with the guard off and on: bench.py runs
alternated in one call (the command of tools/ab_bench.sh; HOIG_GRAD_GUARD selects the option), with each side's run-to-run spread.

    python tools/bench_grad_guard.py --out profiles/grad_guard.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hoig_amd import ops, synthetic                       # noqa: E402
from hoig_amd.guard import GradGuard                      # noqa: E402
from hoig_amd.options import opt_namespace                # noqa: E402
from hoig_amd.models import ModelsFactory                 # noqa: E402

FLOOR_BYTES_PER_S = 4.7e12
CHILD_LIMIT_S = 300           # a bench.py child that runs longer is ended (subprocess.TimeoutExpired ends the tool)


def time_observe(guard, rounds, calls):
    """-> microseconds per observe(), one value per round (device events around `calls` back-to-back calls)."""
    for _ in range(5):
        guard.observe()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            guard.observe()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / calls)
    return out


def bench_step(env, steps, warmup):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup),
           '--no-cpu-baseline', '--graph-steps', '0', '--no-gen-fwd']
    res = subprocess.run(cmd, env=dict(os.environ, HOIG_BENCH_NO_ROOF='1', **env), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                         text=True, check=True, timeout=CHILD_LIMIT_S)
    return float(json.loads(res.stdout.strip().splitlines()[-1])['ms_per_step'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--ab-rounds', type=int, default=8)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ops.set_precision('bf16x3:f16x2')
    m = ModelsFactory.get_by_name('trainer', opt_namespace(gen_name='generator_spade_attn'), use_ddp=False)
    m.set_input(synthetic.make_inputs(8, 256, seed=1))
    m.optimize_parameters()                                  # (the buffers hold a real step's gradients)
    torch.cuda.synchronize()
    say('GradGuard.observe() alone: %d rounds of %d calls, microseconds per call (median, min .. max); floor = 4 B / element at 4.7 TB/s'
        % (a.rounds, a.calls))
    sums = {}
    for tag, net in (('G', m._G), ('D', m._D)):
        tree = m._net(net)
        for per_tensor in (False, True):
            guard = GradGuard(tree, policy='skip', max_norm=1.0, per_tensor=per_tensor)
            t = time_observe(guard, a.rounds, a.calls)
            n = tree.flat_grad.numel()
            floor = 4.0 * n / FLOOR_BYTES_PER_S * 1e6
            med = statistics.median(t)
            say('  %s  %6.1f M elements  rows %4d  median %7.1f  min %7.1f  max %7.1f  floor %6.1f  (%.2f x floor, %.2f TB/s)'
                % (tag, n / 1e6, guard.nseg, med, min(t), max(t), floor, med / floor, 4.0 * n / (med * 1e-6) / 1e12))
            sums[(tag, per_tensor)] = med
            rep = guard.report()
            say('     last record: norm %.6g  max %.6g  nonfinite %d' % (rep['norm'], rep['max'], rep['nonfinite']))
    del m
    torch.cuda.empty_cache()
    say('')
    say('the step, bench.py --steps %d --warmup %d --no-cpu-baseline --graph-steps 0 --no-gen-fwd, ms per step, alternated in this call'
        % (a.steps, a.warmup))
    off = dict(HOIG_GRAD_GUARD='off')
    on = dict(HOIG_GRAD_GUARD='skip')
    aa = [bench_step(off, a.steps, a.warmup), bench_step(off, a.steps, a.warmup)]
    say('  A/A pair (off, off): %.3f %.3f' % (aa[0], aa[1]))
    offs, ons = [], []
    for r in range(a.ab_rounds):
        offs.append(bench_step(off, a.steps, a.warmup))
        ons.append(bench_step(on, a.steps, a.warmup))
        say('  round %d: off %.3f   skip %.3f   difference %+.3f' % (r + 1, offs[-1], ons[-1], ons[-1] - offs[-1]))
    diffs = [b - c for b, c in zip(ons, offs)]
    alloff = aa + offs
    both = (sums[('G', False)] + sums[('D', False)]) / 1e3
    say('  off  (%d runs): median %.3f   min %.3f   max %.3f   (run-to-run spread %.3f ms)'
        % (len(alloff), statistics.median(alloff), min(alloff), max(alloff), max(alloff) - min(alloff)))
    say('  skip (%d runs): median %.3f   min %.3f   max %.3f   (run-to-run spread %.3f ms)'
        % (len(ons), statistics.median(ons), min(ons), max(ons), max(ons) - min(ons)))
    say('  per-round difference skip - off: median %+.3f   min %+.3f   max %+.3f ms;   observe() G + D alone: %.3f ms'
        % (statistics.median(diffs), min(diffs), max(diffs), both))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
