"""Steady-state throughput of hoig_amd.metrics on seeded weights (the real weight files are not needed to time the networks):
FID Inception features (device-only from staged uint8 batches, and path-fed from PNG directories), LPIPS pairs, SSIM + MS-SSIM
pairs; achieved TF/s of the two networks from the multiply-adds their layer tables give (2 FLOP per multiply-add).  Then the pieces
of scoring from device memory, in the same run: the two launches of the PIL-exact resize alone, the path functions with that resize
on the device against on the host, and hoig_amd.metrics.stream.Scorer fed from device tensors.
usage: python tools/bench_metrics.py [--batch 50] [--iters 10] [--images 200] [--out FILE]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import metrics_reference as R                              # noqa: E402
from hoig_amd.metrics import images as I                   # noqa: E402
from hoig_amd.metrics import kernels as K                  # noqa: E402
from hoig_amd.metrics.fid import InceptionFeatures, get_activations   # noqa: E402
from hoig_amd.metrics.lpips import LPIPS, calculate_lpips_given_paths, paired_batches   # noqa: E402
from hoig_amd.metrics.ssim import ms_ssim_nhwc, ssim_nhwc, calculate_ssim_given_paths  # noqa: E402
from hoig_amd.metrics.stream import Scorer               # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters


def macs(fn):
    K.mac_counter = [0]
    try:
        fn()
        torch.cuda.synchronize()
        return K.mac_counter[0]
    finally:
        K.mac_counter = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=50)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--images', type=int, default=200)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_metrics needs the GPU'
    B, lines = a.batch, []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('hoig_amd.metrics throughput, %s, batch %d, %d timed iterations after one warm-up, seeded weights'
        % (torch.cuda.get_device_name(0), B, a.iters))
    rng = np.random.RandomState(0)
    u8 = torch.from_numpy(rng.randint(0, 256, size=(B, 256, 256, 3)).astype(np.uint8)).cuda()
    u8_299 = torch.from_numpy(rng.randint(0, 256, size=(2 * B, 299, 299, 3)).astype(np.uint8)).cuda()

    inc = InceptionFeatures(R.inception_state_dict(1), 2048, None, 'cuda')
    mac_i = macs(lambda: inc.features_u8(u8[:1]))
    t = timed(lambda: inc.features_u8(u8), a.iters)
    say('FID Inception (dims 2048, bf16x3): %.2f G multiply-adds per image; device-only %.1f ms per batch = %.0f images/s, %.1f TF/s'
        % (mac_i / 1e9, t * 1e3, B / t, 2 * mac_i * B / t / 1e12))
    lp = LPIPS(R.alexnet_state_dict(1), R.lpips_state_dict(2), None, 'cuda')
    stage = lambda: K.stage_images_u8(u8_299, None, [(K.IMAGENET_MEAN, K.IMAGENET_STD), (K.LPIPS_MU, K.LPIPS_SIGMA)])
    mac_a = macs(lambda: lp.features(stage()[:1]))
    t = timed(lambda: lp.distance_u8(u8_299), a.iters)
    say('LPIPS (AlexNet at 299, bf16x3): %.2f G multiply-adds per image, 2 images per pair; device-only %.1f ms per batch = %.0f pairs/s, '
        '%.1f TF/s' % (mac_a / 1e9, t * 1e3, B / t, 2 * mac_a * 2 * B / t / 1e12))
    xy = K.stage_images_u8(u8_299, None, [(K.IMAGENET_MEAN, K.IMAGENET_STD)])
    t = timed(lambda: (ssim_nhwc(xy, 255), ms_ssim_nhwc(xy, 255)), a.iters)
    say('SSIM + MS-SSIM at 299: device-only %.2f ms per batch = %.0f pairs/s' % (t * 1e3, B / t))

    pair = torch.cat([u8, u8.flip(0)])                                  # [2B,256,256,3]: one batch of B pairs
    wide = K.pil_resize_u8(pair, (256, 299))
    t_w = timed(lambda: K.pil_resize_u8(pair, (256, 299)), a.iters)
    t_h = timed(lambda: K.pil_resize_u8(wide, (299, 299)), a.iters)
    t = timed(lambda: K.pil_resize_chain_u8(pair, 256), a.iters)
    moved = (pair.numel() + 2 * wide.numel() + wide.numel() // 256 * 299) / 1e6
    say('PIL-exact resize 256 -> 299 of %d pairs: along W %.3f ms, along H %.3f ms (each launch alone), the chain %.3f ms per batch = '
        '%.0f pairs/s (%.1f MB read and written, %.0f GB/s)' % (B, t_w * 1e3, t_h * 1e3, t * 1e3, B / t, moved, moved / 1e3 / t))

    with tempfile.TemporaryDirectory() as root:
        da, db = os.path.join(root, 'a'), os.path.join(root, 'b')
        fa = R.write_pngs(da, a.images, 256, 1)
        R.write_pngs(db, a.images, 256, 2)
        groups = I.batches_of(fa, B)
        t0 = time.perf_counter()
        n = sum(x.shape[0] for x in I.DeviceBatches(groups, 'cuda'))
        torch.cuda.synchronize()
        dec = (time.perf_counter() - t0) / len(groups)
        say('host decode (%d workers, PNG 256x256): %.1f ms per batch of %d = %.0f images/s'
            % (I.decode_workers(), dec * 1e3, B, n / (dec * len(groups))))
        pg = paired_batches([da, db], B)
        t0 = time.perf_counter()
        n = sum(x.shape[0] for x in I.DeviceBatches(pg, 'cuda', 256)) // 2
        torch.cuda.synchronize()
        say('host decode + PIL resize chain to 299 (LPIPS/SSIM inputs): %.1f ms per batch of %d pairs = %.0f pairs/s'
            % ((time.perf_counter() - t0) / len(pg) * 1e3, B, n / (time.perf_counter() - t0)))
        get_activations(fa[:B], inc, B, 2048)
        t0 = time.perf_counter()
        get_activations(fa, inc, B, 2048)
        t = time.perf_counter() - t0
        say('FID features path-fed: %d images in %.2f s = %.0f images/s' % (len(fa), t, len(fa) / t))
        t0 = time.perf_counter()
        calculate_lpips_given_paths([da, db], 256, B, model=lp)
        t = time.perf_counter() - t0
        say('LPIPS path-fed: %d pairs in %.2f s = %.0f pairs/s' % (len(fa), t, len(fa) / t))
        t0 = time.perf_counter()
        calculate_ssim_given_paths([da, db], 256, B)
        t = time.perf_counter() - t0
        say('SSIM + MS-SSIM path-fed: %d pairs in %.2f s = %.0f pairs/s' % (len(fa), t, len(fa) / t))
        t0 = time.perf_counter()
        calculate_lpips_given_paths([da, db], 256, B, model=lp, device_resize=True)
        t = time.perf_counter() - t0
        say('LPIPS path-fed, device_resize=True: %d pairs in %.2f s = %.0f pairs/s' % (len(fa), t, len(fa) / t))
        t0 = time.perf_counter()
        calculate_ssim_given_paths([da, db], 256, B, device_resize=True)
        t = time.perf_counter() - t0
        say('SSIM + MS-SSIM path-fed, device_resize=True: %d pairs in %.2f s = %.0f pairs/s' % (len(fa), t, len(fa) / t))
        gen = torch.cat(list(I.DeviceBatches(I.batches_of(fa, B), 'cuda')))
        gt = torch.cat(list(I.DeviceBatches(I.batches_of(I.list_images(db), B), 'cuda')))

    # the same images from device memory, in updates of 32 (not the metrics' batch), after one warm-up pass; result() apart: with FID it
    # is the host's fp64 sqrtm of a dims x dims product (fid_score.py), which the path-fed feature rate above does not contain either
    def stream(**kw):
        def run():
            s = Scorer(fid=kw.get('fid'), lpips=kw.get('lpips'), ssim=kw.get('ssim', False), fid_batch=B, lpips_batch=B, ssim_batch=B)
            t0 = time.perf_counter()
            for i in range(0, gen.shape[0], 32):
                s.update(gen[i:i + 32], gt[i:i + 32])
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            s.result()
            return t1 - t0, time.perf_counter() - t1
        run()
        return run()

    n = gen.shape[0]
    for label, kw in (('FID features (both streams: 2 images per pair)', dict(fid=inc)), ('LPIPS', dict(lpips=lp)),
                      ('SSIM + MS-SSIM', dict(ssim=True)), ('FID + LPIPS + SSIM + MS-SSIM', dict(fid=inc, lpips=lp, ssim=True))):
        t, tr = stream(**kw)
        say('Scorer.update from device memory, %s: %d pairs in %.3f s = %.0f pairs/s; result() %.3f s' % (label, n, t, n / t, tr))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
