"""The weight EMA's cost (docs/ema.md): EmaWeights.update() -- hoig_ema_tick + hoig_ema_update -- and the swap timed alone on the
generator's and the discriminator's flat buffers, next to the byte floor (12 bytes per element for the update, 16 for the swap, at
the 4.7 TB/s the Adam kernel reaches), and the whole 256 x 256 batch-8 step with the average off and
on: bench.py runs alternated in one call (HOIG_EMA_DECAY selects the option; "off" is the step without this feature), with each
side's run-to-run spread.

    python tools/bench_ema.py --out profiles/ema.txt
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
from hoig_amd import _lib as L, ops, synthetic            # noqa: E402
from hoig_amd.ema import EmaWeights                       # noqa: E402
from hoig_amd.options import opt_namespace                # noqa: E402
from hoig_amd.models import ModelsFactory                 # noqa: E402

FLOOR_BYTES_PER_S = 4.7e12
CHILD_LIMIT_S = 300           # a bench.py child that runs longer is ended (subprocess.TimeoutExpired ends the tool)


def time_calls(fn, rounds, calls):
    """-> microseconds per fn(), one value per round (device events around `calls` back-to-back calls)."""
    for _ in range(6):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
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
    ap.add_argument('--decay', default='0.999')
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ops.set_precision('bf16x3:f16x2')
    m = ModelsFactory.get_by_name('trainer', opt_namespace(gen_name='generator_spade_attn'), use_ddp=False)
    m.set_input(synthetic.make_inputs(8, 256, seed=1))
    m.optimize_parameters()                                  # (the buffers hold a real step's weights)
    m._wait_g()
    m._wait_d()
    torch.cuda.synchronize()
    say('one run.  EmaWeights.update() and hoig_swap_f32 alone: %d rounds of %d calls, microseconds per call (median, min .. max); '
        'floor = 12 B (update) / 16 B (swap) per element at 4.7 TB/s' % (a.rounds, a.calls))
    alone = {}
    for tag, net in (('G', m._G), ('D', m._D)):
        tree = m._net(net)
        ema = EmaWeights(tree, float(a.decay))
        n = tree.flat.numel()
        st = torch.cuda.current_stream().cuda_stream
        for what, nbytes, fn in (('update', 12.0 * n, ema.update),
                                 ('swap  ', 16.0 * n, lambda: L.call('hoig_swap_f32', tree.flat.data_ptr(), ema.ema.data_ptr(), n, st))):
            t = time_calls(fn, a.rounds, a.calls)
            floor = nbytes / FLOOR_BYTES_PER_S * 1e6
            med = statistics.median(t)
            say('  %s %s  %6.1f M elements  median %7.1f  min %7.1f  max %7.1f  floor %6.1f  (%.2f x floor, %.2f TB/s)'
                % (tag, what, n / 1e6, med, min(t), max(t), floor, med / floor, nbytes / (med * 1e-6) / 1e12))
            alone[(tag, what.strip())] = med
        say('     updates counted on the device: %d' % ema.updates())
        del ema
    del m
    torch.cuda.empty_cache()
    say('')
    say('the step, bench.py --steps %d --warmup %d --no-cpu-baseline --graph-steps 0 --no-gen-fwd, ms per step, alternated in this call'
        % (a.steps, a.warmup))
    off = dict(HOIG_EMA_DECAY='0')
    on = dict(HOIG_EMA_DECAY=a.decay)
    aa = [bench_step(off, a.steps, a.warmup), bench_step(off, a.steps, a.warmup)]
    say('  A/A pair (off, off): %.3f %.3f' % (aa[0], aa[1]))
    offs, ons = [], []
    for r in range(a.ab_rounds):
        offs.append(bench_step(off, a.steps, a.warmup))
        ons.append(bench_step(on, a.steps, a.warmup))
        say('  round %d: off %.3f   ema %.3f   difference %+.3f' % (r + 1, offs[-1], ons[-1], ons[-1] - offs[-1]))
    diffs = [b - c for b, c in zip(ons, offs)]
    alloff = aa + offs
    say('  off (%d runs): median %.3f   min %.3f   max %.3f   (run-to-run spread %.3f ms)'
        % (len(alloff), statistics.median(alloff), min(alloff), max(alloff), max(alloff) - min(alloff)))
    say('  ema (%d runs): median %.3f   min %.3f   max %.3f   (run-to-run spread %.3f ms)'
        % (len(ons), statistics.median(ons), min(ons), max(ons), max(ons) - min(ons)))
    say('  per-round difference ema - off: median %+.3f   min %+.3f   max %+.3f ms;   update() on G alone: %.3f ms'
        % (statistics.median(diffs), min(diffs), max(diffs), alone[('G', 'update')] / 1e3))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
