"""The cost of the opt-in GAN objectives (docs/gan_objectives.md): the fused D head (hoig_gan_d_loss: two launches) timed alone on
2 x 7 200 logits -- D's patch outputs at 256 x 256, batch 8 -- next to the four launches of the least-squares head it replaces (two
hoig_loss_accumulate, two hoig_sum_scaled), and the G head next to its one; and the whole 256 x 256 batch-8 step with the options off
and on: bench.py runs alternated in one call (HOIG_GAN_MODE / HOIG_LECAM select the options; "off" is the step without this feature),
with each side's run-to-run spread.

    python tools/bench_gan_objectives.py --out profiles/gan_objectives.txt
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
from hoig_amd import gan_loss as G                        # noqa: E402

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
    ap.add_argument('--mode', default='hinge')
    ap.add_argument('--lecam', default='0.3')
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n = 7200
    dev = torch.device('cuda', 0)
    g = torch.Generator(device='cpu').manual_seed(1)
    both = torch.randn((2 * n,), generator=g).to(dev)
    da, db = torch.empty(n, device=dev), torch.empty(n, device=dev)
    slots = torch.zeros(4, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    ws_bytes = L.lib.hoig_gan_d_loss_workspace_bytes(n, n)
    ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.float64, device=dev)
    lc = G.LeCam(dev, float(a.lecam), decay=0.99, start=1)
    pa, pb, s = both.data_ptr(), both.data_ptr() + 4 * n, 1.0
    p = [t.data_ptr() for t in (slots[0:1], slots[1:2], slots[2:3], slots[3:4])]
    say('one run.  2 x %d logits (D at 256 x 256, batch 8), %d workgroups; %d rounds of %d calls, microseconds per call (median, min .. max)'
        % (n, ws_bytes // 48, a.rounds, a.calls))

    def parent_d():
        L.call('hoig_loss_accumulate', L.LOSS_MSE, pa, None, 1.0, s / n, p[0], da.data_ptr(), n, st)
        L.call('hoig_loss_accumulate', L.LOSS_MSE, pb, None, -1.0, s / n, p[0], db.data_ptr(), n, st)
        L.call('hoig_sum_scaled', pa, 1.0 / n, p[1], n, st)
        L.call('hoig_sum_scaled', pb, 1.0 / n, p[2], n, st)

    def head(mode, state, weight):
        return lambda: L.call('hoig_gan_d_loss', mode, pa, n, pb, n, s, weight, L.LECAM_PAPER, state, da.data_ptr(), db.data_ptr(), p[0], p[1],
                              p[2], p[3] if state else None, ws.data_ptr(), ws_bytes, st)

    cases = [('least-squares head, 4 launches (off)   ', parent_d),
             ('hoig_gan_d_loss lsgan + LeCam, 2 launches', head(L.GAN_LSGAN, lc.state.data_ptr(), lc.weight)),
             ('hoig_gan_d_loss hinge, 2 launches        ', head(L.GAN_HINGE, None, 0.0)),
             ('hoig_gan_d_loss hinge + LeCam, 2 launches', head(L.GAN_HINGE, lc.state.data_ptr(), lc.weight)),
             ('hoig_gan_d_loss logistic + LeCam, 2 launches', head(L.GAN_LOGISTIC, lc.state.data_ptr(), lc.weight)),
             ('least-squares g_adv, 1 launch (off)    ',
              lambda: L.call('hoig_loss_accumulate', L.LOSS_MSE, pb, None, 0.0, s / n, p[0], db.data_ptr(), n, st)),
             ('hoig_gan_g_loss hinge, 2 launches        ',
              lambda: L.call('hoig_gan_g_loss', L.GAN_HINGE, pb, n, s, db.data_ptr(), p[0], ws.data_ptr(), ws_bytes, st))]
    for what, fn in cases:
        t = time_calls(fn, a.rounds, a.calls)
        say('  %s median %7.1f  min %7.1f  max %7.1f' % (what, statistics.median(t), min(t), max(t)))
    say('  (back-to-back launches on one stream: launch-bound either way; ticks taken by the state: %d)' % lc.state_dict()['count'])
    if a.ab_rounds <= 0:
        return finish(a.out, lines)
    say('')
    say('the step, bench.py --steps %d --warmup %d --no-cpu-baseline --graph-steps 0 --no-gen-fwd, ms per step, alternated in this call'
        % (a.steps, a.warmup))
    off = dict(HOIG_GAN_MODE='lsgan', HOIG_LECAM='0')
    on = dict(HOIG_GAN_MODE=a.mode, HOIG_LECAM=a.lecam)
    aa = [bench_step(off, a.steps, a.warmup), bench_step(off, a.steps, a.warmup)]
    say('  A/A pair (off, off): %.3f %.3f' % (aa[0], aa[1]))
    offs, ons = [], []
    for r in range(a.ab_rounds):
        offs.append(bench_step(off, a.steps, a.warmup))
        ons.append(bench_step(on, a.steps, a.warmup))
        say('  round %d: off %.3f   %s+lecam %.3f   difference %+.3f' % (r + 1, offs[-1], a.mode, ons[-1], ons[-1] - offs[-1]))
    diffs = [b - c for b, c in zip(ons, offs)]
    alloff = aa + offs
    say('  off (%d runs): median %.3f   min %.3f   max %.3f   (run-to-run spread %.3f ms)'
        % (len(alloff), statistics.median(alloff), min(alloff), max(alloff), max(alloff) - min(alloff)))
    say('  on  (%d runs): median %.3f   min %.3f   max %.3f   (run-to-run spread %.3f ms)'
        % (len(ons), statistics.median(ons), min(ons), max(ons), max(ons) - min(ons)))
    say('  per-round difference on - off: median %+.3f   min %+.3f   max %+.3f ms' % (statistics.median(diffs), min(diffs), max(diffs)))
    finish(a.out, lines)


if __name__ == '__main__':
    main()
