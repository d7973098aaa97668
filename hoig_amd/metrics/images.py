"""Host side of the metrics: file lists, PIL decoding with the reference's resize chain, and batches staged to the device.

Decoding runs on a small thread pool one batch ahead of the device; a decoded batch goes through pinned memory and an asynchronous
host-to-device copy.  The pool is sized from the CPUs this process may run on (``os.sched_getaffinity``), at most 16.
"""
import os
import pathlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

# metrics/pytorch_fid/fid_score.py
IMAGE_EXTENSIONS = {'bmp', 'jpg', 'jpeg', 'pgm', 'png', 'ppm', 'tif', 'tiff', 'webp'}
EVAL_SIDE = 299   # get_eval_loader(imagenet_normalize=True): Resize([img_size, img_size]) then Resize([299, 299])


def list_images(path):
    """Image files directly under `path` with an IMAGE_EXTENSIONS suffix (case as written: pathlib's glob), sorted."""
    p = pathlib.Path(path)
    if not p.is_dir():
        raise RuntimeError('Invalid path: %s' % path)
    return [str(f) for f in sorted(f for ext in IMAGE_EXTENSIONS for f in p.glob('*.%s' % ext))]


def resize_chain(img, img_size, side=EVAL_SIDE):
    """torchvision's Resize([img_size, img_size]) then Resize([side, side]) on a PIL image: PIL BILINEAR both times."""
    return img.resize((img_size, img_size), Image.BILINEAR).resize((side, side), Image.BILINEAR)


def decode(path, img_size=None):
    """HWC uint8 RGB of `path`, through resize_chain when img_size is given."""
    with Image.open(path) as im:
        img = im.convert('RGB')
    if img_size is not None:
        img = resize_chain(img, img_size)
    return np.asarray(img, dtype=np.uint8)


def decode_workers():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _stack(arrays, names):
    shapes = {a.shape for a in arrays}
    if len(shapes) != 1:
        raise ValueError('images of one batch differ in size: %s' % ', '.join(
            '%s %dx%d' % (os.path.basename(n), a.shape[1], a.shape[0]) for n, a in zip(names, arrays)))
    return np.stack(arrays)


class DeviceBatches(object):
    """Iterates uint8 [B,H,W,3] CUDA tensors of `groups` (a list of file-name lists, one per batch), decoding batch i+1 on the thread
    pool while the caller's kernels for batch i run.  A batch whose images differ in size raises ValueError before it reaches the
    device."""

    def __init__(self, groups, device, img_size=None, workers=None):
        self.groups, self.device, self.img_size = groups, torch.device(device), img_size
        self.workers = workers or decode_workers()

    def __iter__(self):
        if not self.groups:
            return
        with ThreadPoolExecutor(self.workers) as pool, ThreadPoolExecutor(1) as ahead:
            def batch(names):
                return _stack(list(pool.map(lambda n: decode(n, self.img_size), names)), names)

            nxt = ahead.submit(batch, self.groups[0])
            for i in range(len(self.groups)):
                arr = nxt.result()
                if i + 1 < len(self.groups):
                    nxt = ahead.submit(batch, self.groups[i + 1])
                host = torch.from_numpy(arr)
                if self.device.type == 'cuda':
                    host = host.pin_memory()
                yield host.to(self.device, non_blocking=True)


def batches_of(items, batch_size):
    return [items[i:i + batch_size] for i in range(0, len(items), batch_size)]
