"""The sliced Wasserstein distance on the device (docs/swd.md), in one run on seeded images (no dataset, no weights: no value below is
the SWD of real HOGAN output): the time of an update() batch, of every stage of result(), Scorer.update pairs/s with swd on against
off in alternated rounds, the whole metric against the float64 numpy reference of tests/swd_reference.py on 16 threads (on a subset:
the reference takes a minute per few hundred images), and the segmented sort against torch.sort(dim=1) on the same tensor.
usage: python tools/bench_swd.py [--images 5000] [--side 256] [--batch 50] [--ref-images 100] [--out profiles/swd.txt]"""
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
import swd_reference as R                                  # noqa: E402
from hoig_amd.metrics import swd as S                    # noqa: E402
from hoig_amd.metrics.stream import Scorer               # noqa: E402


def seeded_images(n, side, seed):
    """uint8 [n, side, side, 3] on the device: a smooth pattern per image plus noise, from a seeded device generator."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(side, device='cuda'), torch.arange(side, device='cuda'), indexing='ij')
    out = torch.empty((n, side, side, 3), dtype=torch.uint8, device='cuda')
    for i in range(0, n, 250):
        m = min(250, n - i)
        ph = torch.rand((m, 1, 1, 3), generator=g, device='cuda') * 6.0
        fr = torch.rand((m, 1, 1, 3), generator=g, device='cuda') * 0.2 + 0.02
        base = torch.sin((xx + 2 * yy)[None, :, :, None] * fr + ph) * 0.5 + 0.5
        out[i:i + m] = (base * 200.0 + torch.rand((m, side, side, 3), generator=g, device='cuda') * 56.0).clamp(0, 255).to(torch.uint8)
    return out


def timed(fn, repeat=5):
    """median and spread (max - min) of `repeat` synchronised runs after one warm-up"""
    fn()
    ts = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), max(ts) - min(ts)


def numpy_swd(gen, real, opts, threads=16):
    """tests/swd_reference.py's float64 metric with the per-image pyramids on a thread pool."""
    n, H, W = gen.shape[:3]
    nl = R.levels_of(H, W)
    w = R.ref_directions(opts['repeats'], opts['dirs'], opts['seed']).astype(np.float64)
    desc = []
    with ThreadPoolExecutor(threads) as pool:
        for u8, sid in ((gen, 0), (real, 1)):
            pos = R.ref_positions(n, H, W, nl, opts['patches'], opts['seed'], sid)
            per = list(pool.map(lambda i: R.ref_descriptors(u8[i:i + 1], nl, pos[i:i + 1]), range(n)))
            desc.append([np.concatenate([p[lv] for p in per]) for lv in range(nl)])
    values = []
    for lv in range(nl):
        z = []
        for d in desc:
            x = d[lv].reshape(-1, 3, 49)
            z.append(((x - x.mean((0, 2), keepdims=True)) / x.std((0, 2), keepdims=True)).reshape(-1, 147))
        values.append(1000.0 * float(np.mean([np.abs(np.sort(z[0] @ w[r], axis=0) - np.sort(z[1] @ w[r], axis=0)).mean()
                                              for r in range(opts['repeats'])])))
    return values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--side', type=int, default=256)
    ap.add_argument('--batch', type=int, default=50)
    ap.add_argument('--ref-images', type=int, default=100)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_swd needs the GPU'
    torch.set_num_threads(16)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    opts = dict(S.DEFAULTS)
    say('Sliced Wasserstein distance on the device, %s, %d seeded images of %d x %d per set (no dataset: no value below is the SWD of '
        'real HOGAN output), defaults (patches %d, repeats %d, dirs %d); one run, synchronised wall clock, median of 5 after a warm-up'
        % (torch.cuda.get_device_name(0), a.images, a.side, a.side, opts['patches'], opts['repeats'], opts['dirs']))
    gen, real = seeded_images(a.images, a.side, 1), seeded_images(a.images, a.side, 2)

    # ---- update(): one batch into both banks
    def one_update():
        s = Scorer(fid=None, lpips=None, ssim=False, swd=True)
        s.update(gen[:a.batch], real[:a.batch])
    t, sp = timed(one_update)
    say('update() of %d pairs (pyramid, positions and gather of both streams): %.4f s (spread %.4f s) = %.0f pairs/s'
        % (a.batch, t, sp, a.batch / t))

    # ---- the whole stream, then result()
    s = Scorer(fid=None, lpips=None, ssim=False, swd=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(0, a.images, a.batch):
        s.update(gen[i:i + a.batch], real[i:i + a.batch])
    torch.cuda.synchronize()
    t_up = time.perf_counter() - t0
    t_res, sp = timed(s.result, 3)
    out = s.result()
    say('the stream: %d updates in %.3f s; result() %.3f s (spread %.3f s); swd %.6f, levels %s'
        % (a.images // a.batch, t_up, t_res, sp, out['swd'], ' '.join('%.6f' % v for v in out['swd_levels'])))

    # ---- the stages of result() on the finest level
    rows_a, rows_b = s._swd_gen.rows(0), s._swd_gt.rows(0)
    nrows = rows_a.shape[0]
    D = torch.from_numpy(S.directions(opts['repeats'], opts['dirs'], opts['seed'])).cuda()
    t, sp = timed(lambda: S.channel_stats(rows_a))
    say('stages on level 0 (%d rows of 147 per set):' % nrows)
    say('  channel statistics of one set:           %.5f s (spread %.5f s)' % (t, sp))
    stats = S.channel_stats(rows_a)[0]
    t, sp = timed(lambda: S.project(rows_a, stats, D[0]))
    say('  projection of one set on %d directions:  %.5f s (spread %.5f s) = %.2f TF/s over 2 * 147 * rows * dirs'
        % (opts['dirs'], t, sp, 2.0 * 147 * nrows * opts['dirs'] / t / 1e12))
    pa, pb = S.project(rows_a, stats, D[0]), S.project(rows_b, S.channel_stats(rows_b)[0], D[0])
    keep = pa.clone()
    ws = torch.empty(S.L.lib.hoig_sort_segments_workspace_bytes(pa.shape[0], pa.shape[1]) // 8 + 1, dtype=torch.float64, device='cuda')
    status = torch.zeros(1, dtype=torch.int32, device='cuda')

    def ours():
        pa.copy_(keep)
        S._sort_call(pa, ws, status)
    t_copy, _ = timed(lambda: pa.copy_(keep))
    t, sp = timed(ours)
    t_ours = t - t_copy
    say('  segmented sort of [%d, %d] keys:     %.5f s (spread %.5f s; the refill copy of %.5f s taken off) = %.3g keys/s'
        % (pa.shape[0], pa.shape[1], t_ours, sp, t_copy, pa.numel() / t_ours))
    t_torch, sp = timed(lambda: torch.sort(keep, dim=1))
    say('  torch.sort(dim=1) of the same tensor:    %.5f s (spread %.5f s) = %.3g keys/s; ours / torch = %.2f'
        % (t_torch, sp, keep.numel() / t_torch, t_ours / t_torch))
    ours()
    say('  the two agree: %s' % bool(torch.equal(pa, torch.sort(keep, dim=1).values)))
    S._sort_call(pb, ws, status)
    t, sp = timed(lambda: S.sorted_l1(pa, pb))
    say('  sorted L1 of two [%d, %d] buffers:   %.5f s (spread %.5f s)' % (pa.shape[0], pa.shape[1], t, sp))
    del pa, pb, keep, ws

    # ---- Scorer.update with swd on against off, beside SSIM (which needs no weights either)
    pairs = min(200, a.images)
    rates = {False: [], True: []}
    for rnd in range(5):                                   # (round 0 warms both up and is not kept)
        for on in (False, True):
            sc = Scorer(fid=None, lpips=None, ssim=True, swd=on)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(0, pairs, 32):
                sc.update(gen[i:i + 32], real[i:i + 32])
            torch.cuda.synchronize()
            if rnd:
                rates[on].append(pairs / (time.perf_counter() - t0))
    for on in (False, True):
        say('Scorer.update (ssim on) swd %-3s: %s pairs/s, median %.0f, spread %.0f'
            % ('on' if on else 'off', ' '.join('%.0f' % r for r in rates[on]), np.median(rates[on]), max(rates[on]) - min(rates[on])))
    say('  difference of the medians: %.0f pairs/s (%d pairs of %d x %d in updates of 32, alternated rounds)'
        % (np.median(rates[True]) - np.median(rates[False]), pairs, a.side, a.side))

    # ---- the whole metric against float64 numpy on 16 threads, on a subset
    m = min(a.ref_images, a.images)
    banks = S.banks_for(opts, 'cuda')

    def whole():
        b = [bk.copy() for bk in banks]
        b[0].append(gen[:m])
        b[1].append(real[:m])
        return S.swd_from_banks(b[0], b[1], opts['repeats'], opts['dirs'], opts['seed'])
    t_dev, sp = timed(whole, 3)
    got = whole()['swd_levels']
    g_host, r_host = gen[:m].cpu().numpy(), real[:m].cpu().numpy()
    t0 = time.perf_counter()
    want = numpy_swd(g_host, r_host, opts)
    t_np = time.perf_counter() - t0
    say('the whole metric on %d images per set: device %.3f s (spread %.3f s), float64 numpy / scipy on 16 threads %.1f s (%.0f x); '
        'largest difference of a level %.3g of values near %.1f'
        % (m, t_dev, sp, t_np, t_np / t_dev, max(abs(x - y) for x, y in zip(got, want)), max(want)))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
