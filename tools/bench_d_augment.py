"""The discriminator augmentation's cost (docs/d_augment.md): hoig_daug_fwd and hoig_daug_bwd (each with its reduction) timed alone at
batch 8, 256 x 256, 16 condition channels, next to the hoig_cat2_channels launch the forward replaces and the bytes each must move; and
the whole 256 x 256 batch-8 step with the option off and on: bench.py runs alternated in one call (HOIG_D_AUGMENT selects the option;
"off" is the step without this feature), with each side's run-to-run spread.

    python tools/bench_d_augment.py --out profiles/d_augment.txt
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
from hoig_amd import _lib as L                            # noqa: E402
from hoig_amd.d_augment import DAugment                   # noqa: E402

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


def finish(path, lines):
    if path:
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--ab-rounds', type=int, default=8)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--policy', default='color,translation,cutout')
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, S, k = 8, 256, 16
    C = 3 + k
    dev = torch.device('cuda', 0)
    g = torch.Generator(device='cpu').manual_seed(1)
    img = (torch.rand((B, S, S, 3), generator=g) * 2 - 1).to(dev)
    cond = (torch.rand((B, S, S, k), generator=g) * 2 - 1).to(dev)
    dy = (torch.rand((B, S, S, C), generator=g) * 2 - 1).to(dev)
    out, dimg = torch.empty((B, S, S, C), device=dev), torch.empty((B, S, S, 3), device=dev)
    ws = torch.empty(B * L.DAUG_MAX_PARTS, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    npix = B * S * S
    say('one run.  B = %d, %d x %d, k = %d; %d rounds of %d calls, microseconds per call (median, min .. max); bytes = what the call must '
        'read and write once' % (B, S, S, k, a.rounds, a.calls))
    alone = {}
    cases = [('cat2_channels      ', 8.0 * npix * C,
              lambda: L.call('hoig_cat2_channels', img.data_ptr(), 3, cond.data_ptr(), k, out.data_ptr(), npix, st))]
    for name, p in (('p = 1', 1.0), ('p = 0', 0.0)):
        aug = DAugment(dev, 7, p=p, seed=1)
        aug.tick()
        par = aug.draw(0, B, S, S)
        torch.cuda.synchronize()
        flags = par[:, 7].cpu().tolist()
        say('  records at %s: flags %s' % (name, flags))
        # forward: the image again for its sum when colour is on; backward: g's image channels again for G, then g's image channels and dimg
        fb = 8.0 * npix * C + (12.0 * npix if p else 0.0)
        bb = (4.0 * npix * C if p else 0.0) + 4.0 * npix * C + 12.0 * npix
        cases.append(('daug_fwd %s      ' % name, fb, lambda par=par: L.call(
            'hoig_daug_fwd', img.data_ptr(), cond.data_ptr(), par.data_ptr(), out.data_ptr(), B, S, S, k, ws.data_ptr(), st)))
        cases.append(('daug_bwd %s      ' % name, bb, lambda par=par: L.call(
            'hoig_daug_bwd', dy.data_ptr(), par.data_ptr(), dimg.data_ptr(), B, S, S, k, ws.data_ptr(), st)))
    aug = DAugment(dev, 7, p=1.0, seed=1)
    cases.append(('tick + draw        ', 0.0, lambda: (aug.tick(), aug.draw(1, B, S, S))))
    for what, nbytes, fn in cases:
        t = time_calls(fn, a.rounds, a.calls)
        med = statistics.median(t)
        rate = '  (%.2f TB/s over %.0f MB; g is read in 76-byte pixels of which 12 are used)' % (nbytes / (med * 1e-6) / 1e12, nbytes / 1e6) \
            if what.startswith('daug_bwd') else ('  (%.2f TB/s over %.0f MB)' % (nbytes / (med * 1e-6) / 1e12, nbytes / 1e6) if nbytes else '')
        say('  %s median %7.1f  min %7.1f  max %7.1f%s' % (what, med, min(t), max(t), rate))
        alone[what.strip()] = med
    del img, cond, dy, out, dimg
    torch.cuda.empty_cache()
    if a.ab_rounds <= 0:
        return finish(a.out, lines)
    say('')
    say('the step, bench.py --steps %d --warmup %d --no-cpu-baseline --graph-steps 0 --no-gen-fwd, ms per step, alternated in this call'
        % (a.steps, a.warmup))
    off = dict(HOIG_D_AUGMENT='off')
    on = dict(HOIG_D_AUGMENT=a.policy)
    aa = [bench_step(off, a.steps, a.warmup), bench_step(off, a.steps, a.warmup)]
    say('  A/A pair (off, off): %.3f %.3f' % (aa[0], aa[1]))
    offs, ons = [], []
    for r in range(a.ab_rounds):
        offs.append(bench_step(off, a.steps, a.warmup))
        ons.append(bench_step(on, a.steps, a.warmup))
        say('  round %d: off %.3f   aug %.3f   difference %+.3f' % (r + 1, offs[-1], ons[-1], ons[-1] - offs[-1]))
    diffs = [b - c for b, c in zip(ons, offs)]
    alloff = aa + offs
    say('  off (%d runs): median %.3f   min %.3f   max %.3f   (run-to-run spread %.3f ms)'
        % (len(alloff), statistics.median(alloff), min(alloff), max(alloff), max(alloff) - min(alloff)))
    say('  aug (%d runs): median %.3f   min %.3f   max %.3f   (run-to-run spread %.3f ms)'
        % (len(ons), statistics.median(ons), min(ons), max(ons), max(ons) - min(ons)))
    standalone = (3 * alone['daug_fwd p = 1'] + alone['daug_bwd p = 1'] - 2 * alone['cat2_channels'] + alone['tick + draw']) / 1e3
    say('  per-round difference aug - off: median %+.3f   min %+.3f   max %+.3f ms;   three forwards + one backward + the draws, less the '
        'two cat launches they replace, alone: %.3f ms' % (statistics.median(diffs), min(diffs), max(diffs), standalone))
    finish(a.out, lines)


if __name__ == '__main__':
    main()
