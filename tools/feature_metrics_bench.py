"""KID and precision / recall on the device (hoig_amd/metrics/feature_metrics.py), measured in one run on seeded features: the KID
kernels at 100 subsets of 1000 rows and precision / recall at k = 3, both on 5000 rows of 2048 dims per set, timed with device events
(median of the runs after a warm-up), the algorithmic rate beside hoig_gemm_tn_f64's on a Gram matrix of one subset, and the fp64
numpy restatement on this machine's threads; then Scorer.update pairs/s with and without kid / prc, alternated, on the seeded weights
of tools/bench_fid_device.py.  Nothing here is a real KID or precision / recall: there are no Inception weights and no dataset.
usage: python tools/feature_metrics_bench.py [--rows 5000] [--dims 2048] [--runs 5] [--pairs 200] [--out profiles/feature_metrics.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import metrics_reference as R                              # noqa: E402
from hoig_amd import _lib as L                             # noqa: E402
from hoig_amd.metrics import feature_metrics as F          # noqa: E402
from hoig_amd.metrics.fid import InceptionFeatures         # noqa: E402
from hoig_amd.metrics.fid_device import gemm_tn            # noqa: E402
from hoig_amd.metrics.stream import Scorer                 # noqa: E402


def device_seconds(fn, runs):
    """Median seconds of `runs` calls between device events, after one warm-up call; and the spread (max - min)."""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end) * 1e-3)
    return float(np.median(times)), max(times) - min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=5000)
    ap.add_argument('--dims', type=int, default=2048)
    ap.add_argument('--subsets', type=int, default=100)
    ap.add_argument('--subset-size', type=int, default=1000)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--pairs', type=int, default=200)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'feature_metrics_bench needs the GPU'
    assert a.runs >= 5
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n, D, S, m, k = a.rows, a.dims, a.subsets, min(a.subset_size, a.rows), 3
    say('KID and precision / recall on the device, %s, %d rows of %d dims per set, seeded features (no Inception weights, no dataset: '
        'no value below is a real KID or precision / recall); one run, device events, median of %d after a warm-up'
        % (torch.cuda.get_device_name(0), n, D, a.runs))
    g = np.random.default_rng(0)
    mix = (g.standard_normal((64, D)) / 8.0).astype(np.float32)
    real = np.abs(g.standard_normal((n, 64)).astype(np.float32) @ mix + 0.5).astype(np.float32)
    fake = np.abs((g.standard_normal((n, 64)).astype(np.float32) * 1.1 + 0.2) @ mix + 0.5).astype(np.float32)
    tr, tf = torch.from_numpy(real).cuda(), torch.from_numpy(fake).cuda()

    # ---- KID
    ix, iy = F.draw_subsets(n, n, S, m, 0)
    t_kid, spread = device_seconds(lambda: F.kid_sums(tf, tr, ix, iy), a.runs)
    flop = S * 3 * m * m * 2.0 * D                      # the symmetric halves counted once: what the kernels multiply is
    tiles = (m + 63) // 64                              # S * (2 * tiles (tiles + 1) / 2 + tiles^2) * 64^2 * 2 D
    done = S * (tiles * (tiles + 1) + tiles * tiles) * 64 * 64 * 2.0 * D
    mean, std = F.kid_from_features(tf, tr, S, m, 0)
    say('KID %d x %d: %.4f s (spread %.4f s, table upload included) = %.2f TF/s algorithmic (S 3 m^2 2 D = %.3g FLOP); the tiles that '
        'run multiply %.3g FLOP = %.2f TF/s; workspace %d bytes; value %.6g +- %.3g'
        % (S, m, t_kid, spread, flop / t_kid * 1e-12, flop, done, done / t_kid * 1e-12, L.lib.hoig_kid_workspace_bytes(S, m), mean, std))
    # hoig_gemm_tn_f64 on one subset's Gram matrix: the same product from K-major operands, result stored
    at = tf[torch.from_numpy(ix[0].astype(np.int64)).cuda()].t().contiguous()
    c = torch.empty((m, m), dtype=torch.float64, device='cuda')
    t_gemm, _ = device_seconds(lambda: gemm_tn(at, at, c, L.GEMM_F32), a.runs)
    say('  beside it: hoig_gemm_tn_f64 (fp32 operands, K-major, result stored), one %d x %d x %d Gram matrix: %.5f s = %.2f TF/s '
        '(profiles/fid_device.txt times stages, not this kernel alone)' % (m, m, D, t_gemm, 2.0 * m * m * D / t_gemm * 1e-12))
    t0 = time.perf_counter()
    x64, y64 = fake.astype(np.float64), real.astype(np.float64)
    vals = []
    for s in range(S):
        xs, ys = x64[ix[s]], y64[iy[s]]
        kxx, kyy, kxy = ((a_ @ b_.T / D + 1.0) ** 3 for a_, b_ in ((xs, xs), (ys, ys), (xs, ys)))
        vals.append((kxx.sum() - np.trace(kxx)) / (m * (m - 1)) + (kyy.sum() - np.trace(kyy)) / (m * (m - 1)) - 2 * kxy.sum() / (m * m))
    t_np = time.perf_counter() - t0
    say('  fp64 numpy restatement on %s threads: %.2f s (%.1f x the kernels); mean %.6g, difference %.3g'
        % (os.environ.get('OMP_NUM_THREADS', '?'), t_np, t_np / t_kid, float(np.mean(vals)), mean - float(np.mean(vals))))

    # ---- precision / recall
    out = {}

    def prc():
        out['v'] = F.manifold_counts(tr, tf, k)
    t_prc, spread = device_seconds(prc, a.runs)
    flop = 4 * 2.0 * n * n * D                           # two radius passes, two membership passes
    got = F.precision_recall_from_features(tr, tf, k)
    say('precision / recall k = %d: %.4f s (spread %.4f s, the read of the counts included) = %.2f TF/s over 4 n^2 2 D = %.3g FLOP; '
        'precision %.4f recall %.4f density %.4f' % (k, t_prc, spread, flop / t_prc * 1e-12, flop, got['precision'], got['recall'],
                                                     got['density']))
    t0 = time.perf_counter()

    def d2(p, q):
        return (p * p).sum(1)[:, None] + (q * q).sum(1)[None, :] - 2.0 * (p @ q.T)
    piv = y64.mean(0)
    rr, ff, rf = d2(y64 - piv, y64 - piv), d2(x64 - piv, x64 - piv), d2(y64 - piv, x64 - piv)
    np.fill_diagonal(rr, np.inf)
    np.fill_diagonal(ff, np.inf)
    r_real, r_fake = np.partition(rr, k - 1, 1)[:, k - 1], np.partition(ff, k - 1, 1)[:, k - 1]
    p_np, r_np = float(np.mean((rf <= r_real[:, None]).any(0))), float(np.mean((rf.T <= r_fake[:, None]).any(0)))
    t_np = time.perf_counter() - t0
    say('  fp64 numpy restatement: %.2f s (%.1f x the kernels); precision %.4f recall %.4f' % (t_np, t_np / t_prc, p_np, r_np))

    # ---- the scorer
    rng = np.random.RandomState(0)
    gen = torch.from_numpy(rng.randint(0, 256, size=(a.pairs, 256, 256, 3)).astype(np.uint8)).cuda()
    gt = torch.from_numpy(rng.randint(0, 256, size=(a.pairs, 256, 256, 3)).astype(np.uint8)).cuda()
    inc = InceptionFeatures(R.inception_state_dict(1), D, None, 'cuda')

    def run(on):
        s = Scorer(fid=inc, lpips=None, ssim=False, fid_batch=50, kid=on or None, prc=on or None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(0, a.pairs, 32):
            s.update(gen[i:i + 32], gt[i:i + 32])
        torch.cuda.synchronize()
        return a.pairs / (time.perf_counter() - t0)

    run(False), run(True)
    rates = {False: [], True: []}
    for _ in range(4):
        for on in (False, True):
            rates[on].append(run(on))
    for on in (False, True):
        say('Scorer.update kid / prc %-3s: %s pairs/s, median %.0f, spread %.0f' % ('on' if on else 'off', ' '.join('%.0f' % r for r in rates[on]),
                                                                                  np.median(rates[on]), max(rates[on]) - min(rates[on])))
    say('  difference of the medians: %.0f pairs/s (%d pairs of 256 x 256 in updates of 32, fid batch 50, dims %d, seeded weights)'
        % (np.median(rates[True]) - np.median(rates[False]), a.pairs, D))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
