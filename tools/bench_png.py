"""Measures the device PNG encoder against the Pillow path it can replace and writes profiles/png_encode.txt (docs/png_encode.md quotes it).

    python tools/bench_png.py [--out profiles/png_encode.txt] [--rounds 3] [--batches 8]

For batches of 12 images at 256 x 256 x 3 (eval.py's batch of 4 x 3 sets) of the gradients + noise class and of the no-noise class:
the encoder's time per call (events around hoig_png_encode_u8) and per kernel (the profiler's device times), the bytes that cross to
the host against the raw pixels, the file sizes against Pillow's, and EvalWriter.write_images pairs/s with device_png on and off at
workers = 4 and 16, the two settings interleaved in every round.  Nothing is asserted; both paths run in this one process."""
import argparse
import io
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import png_reference as R  # noqa: E402
from hoig_amd import _lib as L  # noqa: E402
from hoig_amd import eval_output as E  # noqa: E402
from hoig_amd import png  # noqa: E402

KINDS = (('noise55', 'gradients + noise 0..55'), ('smooth', 'gradients, no noise'))


def batch_of(kind, n=12):
    return np.stack([R.content(kind, 256, 256, 3, seed=s) for s in range(n)])


def call_ms(dev, reps=20):
    b, h, w, c = dev.shape
    stride = L.lib.hoig_png_encode_bound(h, w, c, 0)
    ws_bytes = L.lib.hoig_png_encode_workspace_bytes(b, h, w, c, 0)
    out = torch.empty(b * stride, dtype=torch.uint8, device=dev.device)
    sizes = torch.empty(b, dtype=torch.int32, device=dev.device)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev.device)

    def run():
        L.call('hoig_png_encode_u8', dev.data_ptr(), b, h, w, c, out.data_ptr(), stride, sizes.data_ptr(), ws.data_ptr(), ws_bytes, 0,
               torch.cuda.current_stream().cuda_stream)

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        run()
    t1.record()
    torch.cuda.synchronize()
    per_call = t0.elapsed_time(t1) / reps
    stages = {}
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                run()
            torch.cuda.synchronize()
        for ev in prof.key_averages():
            for name in ('png_filter_kernel', 'png_segment_kernel', 'png_assemble_kernel'):
                if name in ev.key:
                    total = getattr(ev, 'device_time_total', None) or getattr(ev, 'cuda_time_total', 0)
                    stages[name] = total / 1000.0 / max(ev.count, 1)
    except Exception as e:                                  # the per-kernel split is a nicety; the per-call time stands without it
        stages = {'profiler unavailable (%s)' % type(e).__name__: float('nan')}
    return per_call, stages, sizes.cpu().numpy()


def pairs_per_s(images, device_png, workers, batches):
    """EvalWriter.write_images on `batches` batches of 4 pairs x 3 sets, files on a temporary directory, closed before the clock stops."""
    out = tempfile.mkdtemp(prefix='bench_png_')
    try:
        w = E.EvalWriter(out, workers=workers, device_png=device_png)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for k in range(batches):
            names_a = ['v%d/%04d.jpg' % (k, i) for i in range(4)]
            names_b = ['v%d/%04d.jpg' % (k, i + 4) for i in range(4)]
            w.write_images(images, names_a, names_b)
        w.close()
        dt = time.perf_counter() - t
    finally:
        shutil.rmtree(out, ignore_errors=True)
    return 4 * batches / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'png_encode.txt'))
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batches', type=int, default=8)
    a = ap.parse_args()
    from PIL import Image
    import PIL
    lines = ['device PNG encoder, %s, torch %s, Pillow %s' % (torch.cuda.get_device_name(0), torch.__version__, PIL.__version__),
             'batches of 12 images 256 x 256 x 3, segment_bytes 8192', '']
    for kind, label in KINDS:
        host = batch_of(kind)
        dev = torch.from_numpy(host).to('cuda')
        per_call, stages, sizes = call_ms(dev)
        pil = []
        t = time.perf_counter()
        for img in host:
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, format='PNG')
            pil.append(buf.tell())
        pil_ms = (time.perf_counter() - t) * 1000 / len(host)
        lines.append('== %s (%s)' % (kind, label))
        lines.append('hoig_png_encode_u8: %.3f ms per call of 12 images (events, 20 calls)' % per_call)
        for name, ms in sorted(stages.items()):
            lines.append('  %-22s %.3f ms per launch (profiler device time)' % (name, ms))
        lines.append('bytes to the host: %d of %d raw (%.3f)' % (sizes.sum(), host.size, sizes.sum() / host.size))
        lines.append('file size: %d against Pillow %d per image on average (%.3f)' % (sizes.mean(), np.mean(pil), sizes.sum() / np.sum(pil)))
        lines.append('Pillow Image.save on this host, one thread: %.2f ms per image' % pil_ms)
        images = {k: dev[4 * i:4 * i + 4].contiguous() for i, k in enumerate(('source', 'imitators', 'gt'))}
        pairs_per_s(images, True, 4, 1)                    # warm both paths (pinned pool, thread pools, imports)
        pairs_per_s(images, False, 4, 1)
        for r in range(a.rounds):
            for workers in (4, 16):
                off = pairs_per_s(images, False, workers, a.batches)
                on = pairs_per_s(images, True, workers, a.batches)
                lines.append('round %d workers %2d: write_images %.1f pairs/s with Pillow, %.1f pairs/s with device_png (x%.2f)'
                             % (r + 1, workers, off, on, on / off))
        lines.append('')
    text = '\n'.join(lines)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
