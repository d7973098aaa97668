"""What the device PNG decoder costs and whether it pays (docs/png_decode.md), from one run on the GPU:

  * device time per hoig_png_decode_u8 call (events around the call, inputs already on the device) and per kernel (torch.profiler's
    kernel records) for 100 images at 256 x 256 x 3, written by Pillow with its defaults and by the device encoder, on the
    'gradients + noise' (noise55) and 'smooth' contents of tests/png_reference.content; the compressed bytes that cross to the device
    against the raw pixels; the same call with the window in the workspace (tuning key png_window=1);
  * calculate_ssim_given_paths / calculate_lpips_given_paths pairs/s and get_activations images/s on seeded weights with
    device_png_decode off and on, alternated in this process for three rounds, at 16 decode workers and at 4.

usage: python tools/bench_png_decode.py [--images 100] [--iters 10] [--pairs 200] [--batch 50] [--out FILE]"""
import argparse
import io
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import metrics_reference as M                              # noqa: E402
import png_reference as R                                  # noqa: E402
from hoig_amd import _lib as L                             # noqa: E402
from hoig_amd import png, png_decode as D                  # noqa: E402
from hoig_amd.metrics import images as I                   # noqa: E402
from hoig_amd.metrics.fid import InceptionFeatures, get_activations   # noqa: E402
from hoig_amd.metrics.lpips import LPIPS, calculate_lpips_given_paths  # noqa: E402
from hoig_amd.metrics.ssim import calculate_ssim_given_paths           # noqa: E402


def pillow_file(img):
    b = io.BytesIO()
    Image.fromarray(img).save(b, 'PNG')
    return b.getvalue()


class Call(object):
    """One batch staged on the device; run() is the hoig_png_decode_u8 call alone."""

    def __init__(self, files):
        self.items = [D.parse(f)[0] for f in files]
        buf, self.plans, self.out_bytes, self.ws_bytes = D.pack(self.items)
        self.compressed = sum(len(p.stream) for p in self.items)
        self.buf = torch.from_numpy(buf).cuda()
        self.plans_dev = torch.from_numpy(np.frombuffer(bytes(self.plans), np.uint8).copy()).cuda()
        self.out = torch.empty(self.out_bytes, dtype=torch.uint8, device='cuda')
        self.status = torch.empty(len(files), dtype=torch.int32, device='cuda')
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device='cuda')

    def run(self):
        L.call('hoig_png_decode_u8', self.buf.data_ptr(), self.buf.numel(), self.plans, self.plans_dev.data_ptr(), len(self.items),
               self.out.data_ptr(), self.out_bytes, self.status.data_ptr(), self.ws.data_ptr(), self.ws_bytes, 0,
               torch.cuda.current_stream().cuda_stream)


def event_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), min(times), max(times)


def kernel_ms(fn, iters):
    """{kernel name fragment: mean ms per launch} from the profiler's kernel records; None where the profiler gives none"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            for frag in ('png_inflate_kernel', 'png_rows_kernel'):
                if frag in e.key:
                    total = getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0)
                    out[frag] = total / 1e3 / max(e.count, 1)
        return out or None
    except Exception as err:                               # the tool still reports the call's time
        print('profiler unavailable: %r' % (err,), flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=100)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--pairs', type=int, default=200)
    ap.add_argument('--batch', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_png_decode needs the GPU'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('hoig_png_decode_u8, %s: %d images of 256 x 256 x 3 per call, median (min .. max) of %d calls after one warm-up; inputs on the '
        'device' % (torch.cuda.get_device_name(0), a.images, a.iters))
    raw = a.images * 256 * 256 * 3
    for kind in ('noise55', 'smooth'):
        imgs = np.stack([R.content(kind, 256, 256, 3, seed=100 + i) for i in range(a.images)])
        writers = (('Pillow defaults', [pillow_file(im) for im in imgs]),
                   ('device encoder', png.encode_u8(torch.from_numpy(imgs).cuda())))
        for label, files in writers:
            call = Call(files)
            med, lo, hi = event_ms(call.run, a.iters)
            assert call.status.cpu().abs().sum().item() == 0
            got = call.out.view(a.images, 256, 256, 3).cpu().numpy()
            assert np.array_equal(got, imgs), 'decoded pixels differ from the input'
            per = kernel_ms(call.run, a.iters)
            L.set_tuning('png_window', 1)                  # the other window: the filtered stream in the workspace
            try:
                ws_med, ws_lo, ws_hi = event_ms(call.run, a.iters)
            finally:
                L.set_tuning('png_window', 0)
            assert np.array_equal(call.out.view(a.images, 256, 256, 3).cpu().numpy(), imgs)
            say('%-8s %-15s call %.3f ms (%.3f .. %.3f) = %.0f images/s; %s; %.2f MB compressed against %.2f MB raw (%.0f %%)'
                % (kind, label, med, lo, hi, a.images / med * 1e3,
                   'inflate %.3f ms, rows %.3f ms' % (per.get('png_inflate_kernel', float('nan')), per.get('png_rows_kernel', float('nan')))
                   if per else 'per-kernel times unavailable', call.compressed / 1e6, raw / 1e6, 100.0 * call.compressed / raw))
            say('%-8s %-15s the same call with png_window=1 (window in the workspace): %.3f ms (%.3f .. %.3f)' % (kind, label, ws_med, ws_lo, ws_hi))
        t0 = time.perf_counter()
        for f in writers[0][1]:
            np.asarray(Image.open(io.BytesIO(f)).convert('RGB'))
        t = time.perf_counter() - t0
        say('%-8s Pillow defaults: Image.open(...).convert(\'RGB\') on one host thread %.2f ms per image' % (kind, t / a.images * 1e3))

    inc = InceptionFeatures(M.inception_state_dict(1), 2048, None, 'cuda')
    lp = LPIPS(M.alexnet_state_dict(1), M.lpips_state_dict(2), None, 'cuda')
    B = a.batch
    with tempfile.TemporaryDirectory() as root:
        da, db = os.path.join(root, 'a'), os.path.join(root, 'b')
        fa = M.write_pngs(da, a.pairs, 256, 1)
        M.write_pngs(db, a.pairs, 256, 2)
        jobs = (('SSIM + MS-SSIM pairs/s', lambda on: calculate_ssim_given_paths([da, db], 256, B, device_png_decode=on)),
                ('LPIPS pairs/s', lambda on: calculate_lpips_given_paths([da, db], 256, B, model=lp, device_png_decode=on)),
                ('FID features images/s', lambda on: get_activations(fa, inc, B, 2048, device_png_decode=on)))
        real_workers = I.decode_workers
        say('directory functions, %d pairs of 256 x 256 PNGs (Pillow defaults, gradients + noise) in batches of %d, seeded weights; '
            'device_png_decode off / on alternated in one process, three rounds after a warm-up of each; this process may use %d CPUs'
            % (a.pairs, B, len(os.sched_getaffinity(0))))
        for workers in (16, 4):
            I.decode_workers = lambda w=workers: w
            for label, job in jobs:
                values = {False: job(False), True: job(True)}            # warm-up, and the values must be equal
                same = np.array_equal(values[False], values[True]) if isinstance(values[False], np.ndarray) else values[False] == values[True]
                assert same, 'device_png_decode changed the result of %s' % label
                rates = {False: [], True: []}
                for _ in range(3):
                    for on in (False, True):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        job(on)
                        torch.cuda.synchronize()
                        rates[on].append(a.pairs / (time.perf_counter() - t0))
                off, on = rates[False], rates[True]
                say('%2d workers  %-24s off %s (median %.0f)   on %s (median %.0f)   on / off %.2f'
                    % (workers, label, ' '.join('%.0f' % r for r in off), np.median(off), ' '.join('%.0f' % r for r in on),
                       np.median(on), np.median(on) / np.median(off)))
        I.decode_workers = real_workers
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
