"""The cost of the opt-in style (Gram-matrix) term (docs/style_loss.md): per VGG level of a batch-8 step at 256 x 256, hoig_style_gram
(three launches) and hoig_style_dfeat (one) timed alone, next to the byte floor of their traffic, the issue floor of the fp32 MFMA and
torch.bmm on the same fp32 tensors; and the whole 256 x 256 batch-8 step with the option off and on: bench.py runs alternated in one
call (HOIG_LAMBDA_STYLE selects the option; "off" is the step without this feature, launch for launch), with each side's run-to-run
spread.

    python tools/bench_style_loss.py --out profiles/style_loss.txt
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

CHILD_LIMIT_S = 300           # a bench.py child that runs longer is ended (subprocess.TimeoutExpired ends the tool)
HBM_BYTES_PER_S = 8.0e12      # the MI355X's peak HBM bandwidth, for the byte floors
MFMA_F32_FLOPS = 157.3e12     # its peak on v_mfma_f32_32x32x2_f32, for the issue floor
LEVELS = [(256, 64), (128, 128), (64, 256), (32, 512), (16, 512)]          # (side, channels) of relu{k}_1 at 256 x 256


def time_calls(fn, rounds, calls):
    """-> microseconds per fn(), one value per round (device events around `calls` back-to-back calls)."""
    for _ in range(4):
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
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--ab-rounds', type=int, default=8)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--weight', default='10')
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    N = 8
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream().cuda_stream
    T, K = L.STYLE_TILE, L.STYLE_CHUNK
    say('one run.  batch %d, the five relu{k}_1 maps of a 256 x 256 step; %d rounds of %d calls, microseconds per call (median, min .. max)'
        % (N, a.rounds, a.calls))
    med = lambda t: '%8.1f  (%.1f .. %.1f)' % (statistics.median(t), min(t), max(t))
    for level, (side, C) in enumerate(LEVELS, 1):
        P = side * side
        g = torch.Generator(device='cpu').manual_seed(level)
        fx = torch.relu(torch.randn((N, P, C), generator=g)).to(dev)
        fy = torch.relu(torch.randn((N, P, C), generator=g)).to(dev)
        S, dfx, slot = torch.empty((N, C, C), device=dev), torch.empty_like(fx), torch.zeros(2, device=dev)
        ws_bytes = L.lib.hoig_style_workspace_bytes(N, P, C)
        ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.float64, device=dev)
        tiles = (C + T - 1) // T
        pairs, chunks = tiles * (tiles + 1) // 2, (P + K - 1) // K
        both = torch.cat([fx, fy])
        cases = [('hoig_style_gram, 3 launches', lambda: L.call('hoig_style_gram', fx.data_ptr(), fy.data_ptr(), N, P, C, 10.0, S.data_ptr(),
                                                               slot.data_ptr(), None, None, ws.data_ptr(), ws_bytes, st)),
                 ('torch.bmm F^T F, 2N images', lambda: torch.bmm(both.transpose(1, 2), both)),
                 ('hoig_style_dfeat, 1 launch ', lambda: L.call('hoig_style_dfeat', fx.data_ptr(), S.data_ptr(), N, P, C, dfx.data_ptr(), st)),
                 ('torch.bmm F S, N images    ', lambda: torch.bmm(fx, S))]
        say('level %d: %d x %d x %d, %d tile pairs x %d chunks x %d images = %d workgroups (Gram), workspace %.1f MB'
            % (level, side, side, C, pairs, chunks, 2 * N, pairs * chunks * 2 * N, ws_bytes / 1e6))
        for what, fn in cases:
            say('  %s %s' % (what, med(time_calls(fn, a.rounds, a.calls))))
        gram_bytes, gram_flops = 2 * N * P * C * 4, 2.0 * 2 * N * pairs * T * T * P
        d_bytes, d_flops = 2 * N * P * C * 4 + N * C * C * 4, 2.0 * N * P * C * tiles * T
        say('  floors: Gram %.1f MB read once = %.1f us at %.1f TB/s, %.2f GFLOP as issued = %.1f us at %.1f TF;  dfeat %.1f MB = %.1f us, '
            '%.2f GFLOP = %.1f us' % (gram_bytes / 1e6, gram_bytes / HBM_BYTES_PER_S * 1e6, HBM_BYTES_PER_S / 1e12, gram_flops / 1e9,
                                      gram_flops / MFMA_F32_FLOPS * 1e6, MFMA_F32_FLOPS / 1e12, d_bytes / 1e6,
                                      d_bytes / HBM_BYTES_PER_S * 1e6, d_flops / 1e9, d_flops / MFMA_F32_FLOPS * 1e6))
        del fx, fy, S, dfx, ws, both
    say('  (back-to-back calls on one stream, operands resident in the Infinity Cache where they fit)')
    if a.ab_rounds <= 0:
        return finish(a.out, lines)
    say('')
    say('the step, bench.py --steps %d --warmup %d --no-cpu-baseline --graph-steps 0 --no-gen-fwd, ms per step, alternated in this call; '
        'on: HOIG_LAMBDA_STYLE=%s, levels 2,3,4,5' % (a.steps, a.warmup, a.weight))
    off, on = dict(HOIG_LAMBDA_STYLE=''), dict(HOIG_LAMBDA_STYLE=a.weight)
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
