"""The cost of the opt-in region reconstruction term (docs/region_loss.md): the head (hoig_region_loss: one memset node, three launches)
timed alone on batch 8 at 256 x 256, C = 3, next to the one hoig_loss_accumulate L1 launch it replaces on the source view and to the
byte floor of its traffic; and the whole 256 x 256 batch-8 step with the option off and on: bench.py runs alternated in one call
(HOIG_LAMBDA_REC_HAND / HOIG_LAMBDA_REC_OBJ select the option; "off" is the step without this feature, launch for launch), with each
side's run-to-run spread.

    python tools/bench_region_loss.py --out profiles/region_loss.txt
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hoig_amd import _lib as L                            # noqa: E402

CHILD_LIMIT_S = 300           # a bench.py child that runs longer is ended (subprocess.TimeoutExpired ends the tool)
HBM_BYTES_PER_S = 8.0e12      # the MI355X's peak HBM bandwidth, for the byte floor


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
    ap.add_argument('--weight', default='10')
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    N, H, W, C, R = 8, 256, 256, 3, 2
    n = N * H * W * C
    dev = torch.device('cuda', 0)
    g = torch.Generator(device='cpu').manual_seed(1)
    pred, target = torch.rand((N, H, W, C), generator=g).to(dev), torch.rand((N, H, W, C), generator=g).to(dev)
    # a hand and an object disk per image, about 12 % of the frame together (docs/region_metrics.md)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    labels = torch.zeros((N, H, W), dtype=torch.uint8)
    for i in range(N):
        labels[i][(yy - 100 - 5 * i) ** 2 + (xx - 90) ** 2 <= 40 ** 2] = 1
        labels[i][(yy - 150) ** 2 + (xx - 160 + 3 * i) ** 2 <= 30 ** 2] = 2
    labels = labels.to(dev)
    dpred, slots = torch.empty_like(pred), torch.zeros(8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    ws_bytes = L.lib.hoig_region_loss_workspace_bytes(N, H, W, C, R)
    ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.float64, device=dev)
    lam = (ctypes.c_double * (R + 1))(0.0, float(a.weight), float(a.weight))
    lamp = ctypes.cast(lam, ctypes.c_void_p)
    p = [slots[k:k + 1].data_ptr() for k in range(8)]
    tiles = (H * W * C + L.RLOSS_TILE - 1) // L.RLOSS_TILE
    say('one run.  batch %d at %d x %d, C = %d: %d floats, %d + %d workgroups (counting, value and gradient); %d rounds of %d calls, '
        'microseconds per call (median, min .. max)' % (N, H, W, C, n, N * ((H * W + L.RLOSS_COUNT_TILE - 1) // L.RLOSS_COUNT_TILE),
                                                         N * tiles, a.rounds, a.calls))

    def head(grad):
        return lambda: L.call('hoig_region_loss', pred.data_ptr(), target.data_ptr(), labels.data_ptr(), N, H, W, C, R, lamp, 30.0, 64,
                              dpred.data_ptr() if grad else None, p[0], p[2], p[1], None, status.data_ptr(), ws.data_ptr(), ws_bytes, st)

    cases = [('hoig_loss_accumulate L1, 1 launch (off)          ',
              lambda: L.call('hoig_loss_accumulate', L.LOSS_L1, pred.data_ptr(), target.data_ptr(), 0.0, 30.0 / n, p[0], dpred.data_ptr(), n, st)),
             ('hoig_region_loss, memset + 3 launches            ', head(True)),
             ('hoig_region_loss without dpred, memset + 3 launches', head(False))]
    for what, fn in cases:
        t = time_calls(fn, a.rounds, a.calls)
        say('  %s median %7.1f  min %7.1f  max %7.1f' % (what, statistics.median(t), min(t), max(t)))
    nbytes = 3 * 4 * n + 2 * N * H * W
    say('  byte floor: 2 reads + 1 write of %.1f MB and the labels twice (%.1f MB) = %.1f MB, %.1f microseconds at %.1f TB/s'
        % (4 * n / 1e6, 2 * N * H * W / 1e6, nbytes / 1e6, nbytes / HBM_BYTES_PER_S * 1e6, HBM_BYTES_PER_S / 1e12))
    say('  (back-to-back calls on one stream, operands resident in the Infinity Cache; status word after the last call: %d)' % int(status[0]))
    if a.ab_rounds <= 0:
        return finish(a.out, lines)
    say('')
    say('the step, bench.py --steps %d --warmup %d --no-cpu-baseline --graph-steps 0 --no-gen-fwd, ms per step, alternated in this call'
        % (a.steps, a.warmup))
    off = dict(HOIG_LAMBDA_REC_HAND='', HOIG_LAMBDA_REC_OBJ='')
    on = dict(HOIG_LAMBDA_REC_HAND=a.weight, HOIG_LAMBDA_REC_OBJ=a.weight)
    aa = [bench_step(off, a.steps, a.warmup), bench_step(off, a.steps, a.warmup)]
    say('  A/A pair (off, off): %.3f %.3f' % (aa[0], aa[1]))
    offs, ons = [], []
    for r in range(a.ab_rounds):
        offs.append(bench_step(off, a.steps, a.warmup))
        ons.append(bench_step(on, a.steps, a.warmup))
        say('  round %d: off %.3f   on %.3f   difference %+.3f' % (r + 1, offs[-1], ons[-1], ons[-1] - offs[-1]))
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
