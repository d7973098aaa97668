"""FID's statistics and distance on the device against the default (host) path, in one run on the seeded weights of
tools/bench_metrics.py: Scorer.update pairs/s and result() seconds with fid_device off and on, then the two stages of result() apart
on the same statistics -- the moments (np.mean / np.cov of the kept features against Moments.statistics) and the distance (scipy's
sqrtm against frechet_distance_device) -- and the difference of the two values.
usage: python tools/bench_fid_device.py [--pairs 200] [--batch 50] [--dims 2048] [--out profiles/fid_device.txt]"""
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
from hoig_amd.metrics.fid import InceptionFeatures, calculate_frechet_distance   # noqa: E402
from hoig_amd.metrics.fid_device import frechet_distance_device                  # noqa: E402
from hoig_amd.metrics.stream import Scorer               # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=200)
    ap.add_argument('--batch', type=int, default=50)
    ap.add_argument('--dims', type=int, default=2048)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_fid_device needs the GPU'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('FID statistics and distance, host against device (fid_device), %s, %d pairs of 256 x 256 in updates of 32, fid batch %d, dims %d, '
        'seeded weights; second of two passes' % (torch.cuda.get_device_name(0), a.pairs, a.batch, a.dims))
    rng = np.random.RandomState(0)
    gen = torch.from_numpy(rng.randint(0, 256, size=(a.pairs, 256, 256, 3)).astype(np.uint8)).cuda()
    gt = torch.from_numpy(rng.randint(0, 256, size=(a.pairs, 256, 256, 3)).astype(np.uint8)).cuda()
    inc = InceptionFeatures(R.inception_state_dict(1), a.dims, None, 'cuda')

    def run(fid_device):
        s = Scorer(fid=inc, lpips=None, ssim=False, fid_batch=a.batch, fid_device=fid_device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(0, a.pairs, 32):
            s.update(gen[i:i + 32], gt[i:i + 32])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = s.result()
        return s, t1 - t0, time.perf_counter() - t1, out['fid']

    values = {}
    for fid_device in (False, True):
        run(fid_device)
        s, t_up, t_res, values[fid_device] = run(fid_device)
        say('fid_device=%-5s Scorer.update: %d pairs in %.3f s = %.0f pairs/s; result() %.3f s; fid %.12g'
            % (fid_device, a.pairs, t_up, a.pairs / t_up, t_res, values[fid_device]))
        if not fid_device:
            t0 = time.perf_counter()
            stats = s.statistics() + s._statistics(s._feat_gt, s._fid_gt)
            t1 = time.perf_counter()
            calculate_frechet_distance(*stats)
            say('  host stages:   mean + np.cov of both sets %.3f s, scipy sqrtm distance %.3f s' % (t1 - t0, time.perf_counter() - t1))
        else:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dstats = s._moments(s._feat_gen, s._fid_gen).statistics() + s._moments(s._feat_gt, s._fid_gt).statistics()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            frechet_distance_device(*dstats)
            say('  device stages: last batch + moments of both sets %.3f s, Cholesky + Gram + eigenvalue distance %.3f s'
                % (t1 - t0, time.perf_counter() - t1))
    say('fid difference device - host: %.3g (relative %.3g)' % (values[True] - values[False],
                                                                 (values[True] - values[False]) / abs(values[False])))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
