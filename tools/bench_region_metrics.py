"""The region scores on the device (docs/region_metrics.md), in one run on seeded images with the target-view label maps of
hoig_amd.synthetic (no dataset, no weights: no value below is a score of real HOGAN output): (a) the time of the three stages of one
update() -- statistics, boxes, crops of both streams -- beside the bytes each moves, (b) Scorer.update pairs/s beside SSIM with the
option on against off in alternated rounds, (c) the same work in numpy + Pillow (tests/region_metrics_reference.py) on 16 threads.
usage: python tools/bench_region_metrics.py [--pairs 50] [--side 256] [--size 128] [--out profiles/region_metrics.txt]"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import region_metrics_reference as R                       # noqa: E402
from hoig_amd import synthetic                           # noqa: E402
from hoig_amd.metrics import regions as G                # noqa: E402
from hoig_amd.metrics.stream import Scorer               # noqa: E402
from bench_swd import seeded_images                        # noqa: E402

INNER = 200      # launches of a stage inside one timed window: a single one is tens of microseconds


def timed(fn, repeat=5):
    """median and spread (max - min) of the time of ONE call, from `repeat` synchronised windows of INNER calls after a warm-up"""
    fn()
    ts = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(INNER):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / INNER)
    return float(np.median(ts)), max(ts) - min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=50)
    ap.add_argument('--side', type=int, default=256)
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_region_metrics needs the GPU'
    torch.set_num_threads(16)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n, side, S = a.pairs, a.side, a.size
    opts = dict(G.DEFAULTS, size=S)
    say('Region scores on the device, %s, %d seeded pairs of %d x %d with the target-view labels of synthetic.make_inputs (no dataset: '
        'no value below is a score of real HOGAN output), crops of %d, min_pixels %d; one run, synchronised wall clock, a call\'s time '
        'from windows of %d calls, median of 5 windows after a warm-up'
        % (torch.cuda.get_device_name(0), n, side, side, S, opts['min_pixels'], INNER))
    inp = synthetic.make_inputs(n, side, seed=8)
    lab_host = R.labels_from_masks(inp['bg_mask'][n:, 0].numpy(), inp['hand_mask'][n:, 0].numpy())
    gen, gt, lab = seeded_images(n, side, 1), seeded_images(n, side, 2), torch.from_numpy(lab_host).cuda()
    stats, _ = G.region_stats(gen, gt, lab)
    boxes = G.region_boxes(stats, side, side, opts['min_pixels'])
    bx = boxes.cpu().numpy()
    sides = bx[:, :, 2][bx[:, :, 3] != 0]
    frac = float((lab_host != 0).mean())
    say('labels: hand + object cover %.1f %% of the frame; %d of %d boxes valid, sides %d .. %d (median %d)'
        % (100 * frac, sides.size, bx.shape[0] * bx.shape[1], sides.min(), sides.max(), int(np.median(sides))))

    # ---- (a) the three stages of one update()
    t, sp = timed(lambda: G.region_stats(gen, gt, lab))
    moved = n * side * side * 7
    say('(a) statistics of %d pairs:  %.6f s (spread %.6f s); reads 7 B per pixel = %.2f MB -> %.0f GB/s'
        % (n, t, sp, moved / 1e6, moved / t / 1e9))
    t_box, sp = timed(lambda: G.region_boxes(stats, side, side, opts['min_pixels']))
    say('    boxes:                   %.6f s (spread %.6f s); %d rows of 64 B in, %d boxes of 16 B out' % (t_box, sp, n * 2, n * 2))
    t_crop, sp = timed(lambda: (G.region_crops(gen, boxes, S), G.region_crops(gt, boxes, S)))
    read = 2 * int((sides.astype(np.int64) ** 2).sum()) * 3
    mid = 2 * int(sides.astype(np.int64).sum()) * S * 3
    wrote = 2 * 2 * n * S * S * 3
    say('    crops of both streams:   %.6f s (spread %.6f s); reads %.2f MB of windows (at most 2 R side^2 3 B per pair), writes and '
        'reads back %.2f MB between the passes, writes %.2f MB (2 R S^2 3 B per pair) -> %.0f GB/s over the three'
        % (t_crop, sp, read / 1e6, mid / 1e6, wrote / 1e6, (read + 2 * mid + wrote) / t_crop / 1e9))
    say('    the three together: %.6f s per update() of %d pairs = %.0f pairs/s' % (t + t_box + t_crop, n, n / (t + t_box + t_crop)))

    # ---- (b) Scorer.update with regions on against off, beside SSIM (which needs no weights)
    big = 8
    gens, gts, labs = gen.repeat(big, 1, 1, 1), gt.repeat(big, 1, 1, 1), lab.repeat(big, 1, 1)
    pairs = gens.shape[0]
    rates = {False: [], True: []}
    for rnd in range(5):                                   # (round 0 warms both up and is not kept)
        for on in (False, True):
            sc = Scorer(fid=None, lpips=None, ssim=True, regions=opts if on else None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(0, pairs, n):
                if on:
                    sc.update(gens[i:i + n], gts[i:i + n], labs[i:i + n])
                else:
                    sc.update(gens[i:i + n], gts[i:i + n])
            torch.cuda.synchronize()
            if rnd:
                rates[on].append(pairs / (time.perf_counter() - t0))
    for on in (False, True):
        say('(b) Scorer.update (ssim on) regions %-3s: %s pairs/s, median %.0f, spread %.0f'
            % ('on' if on else 'off', ' '.join('%.0f' % r for r in rates[on]), np.median(rates[on]), max(rates[on]) - min(rates[on])))
    say('    difference of the medians: %.0f pairs/s (%d pairs of %d x %d in updates of %d, alternated rounds; with the option on every '
        'batch of %d crops per region also goes through SSIM at %d x %d)'
        % (np.median(rates[True]) - np.median(rates[False]), pairs, side, side, n, opts['batch'], S, S))

    # ---- (c) the same work in numpy + Pillow on 16 threads
    g_host, t_host = gen.cpu().numpy(), gt.cpu().numpy()

    def one(i):
        st, _ = R.stats(g_host[i:i + 1], t_host[i:i + 1], lab_host[i:i + 1])
        b = R.boxes(st, side, side, opts['min_pixels'])
        return st, b, R.crops(g_host[i:i + 1], b, S), R.crops(t_host[i:i + 1], b, S)
    ts = []
    with ThreadPoolExecutor(16) as pool:
        for _ in range(4):
            t0 = time.perf_counter()
            per = list(pool.map(one, range(n)))
            ts.append(time.perf_counter() - t0)
    t_np = float(np.median(ts[1:]))
    same = (np.array_equal(np.concatenate([p[0] for p in per]), stats.cpu().numpy())
            and np.array_equal(np.concatenate([p[1] for p in per]), bx)
            and np.array_equal(np.concatenate([p[2] for p in per], 1), G.region_crops(gen, boxes, S).cpu().numpy())
            and np.array_equal(np.concatenate([p[3] for p in per], 1), G.region_crops(gt, boxes, S).cpu().numpy()))
    say('(c) the same statistics, boxes and crops in numpy int64 + Pillow on 16 threads: %.4f s per %d pairs (spread %.4f s) = %.0f '
        'pairs/s, %.0f x the device\'s three stages; every statistic, box and crop byte equal: %s'
        % (t_np, n, max(ts[1:]) - min(ts[1:]), n / t_np, t_np / (t + t_box + t_crop), same))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
