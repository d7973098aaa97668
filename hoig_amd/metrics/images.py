"""Host side of the metrics: file lists, PIL decoding with the reference's resize chain, and batches staged to the device.

Decoding runs on a small thread pool one batch ahead of the device; a decoded batch goes through pinned memory and an asynchronous
host-to-device copy.  The pool is sized from the CPUs this process may run on (``os.sched_getaffinity``), at most 16.

``device_png_decode`` (or ``HOIG_DEVICE_PNG_DECODE=1``; off by default): the workers only read the files and walk their chunks, and
the PNG files the device decoder supports go through one ``png_decode.decode_u8`` call per batch (docs/png_decode.md); every other file
is decoded by Pillow as before and copied into its batch position, and so is a file whose stream the device refuses (Pillow reads
some damaged files, and raises on the others as it does by default).  Both give Pillow's bytes.
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


def png_decode_option(value):
    """The device_png_decode argument: None takes HOIG_DEVICE_PNG_DECODE=1 (off otherwise)."""
    return os.environ.get('HOIG_DEVICE_PNG_DECODE', '') == '1' if value is None else bool(value)


def _stack(arrays, names):
    shapes = {a.shape for a in arrays}
    if len(shapes) != 1:
        raise ValueError('images of one batch differ in size: %s' % ', '.join(
            '%s %dx%d' % (os.path.basename(n), a.shape[1], a.shape[0]) for n, a in zip(names, arrays)))
    return np.stack(arrays)


class DeviceBatches(object):
    """Iterates uint8 [B,H,W,3] CUDA tensors of `groups` (a list of file-name lists, one per batch), decoding batch i+1 on the thread
    pool while the caller's kernels for batch i run.  A batch whose images differ in size raises ValueError before it reaches the
    device.  With device_png_decode the supported PNG files are decoded on the device, and img_size is applied there as well
    (kernels.pil_resize_chain_u8: the same bytes)."""

    def __init__(self, groups, device, img_size=None, workers=None, device_png_decode=None):
        self.groups, self.device, self.img_size = groups, torch.device(device), img_size
        self.workers = workers or decode_workers()
        self.device_png_decode = png_decode_option(device_png_decode)

    def __iter__(self):
        if not self.groups:
            return
        if self.device_png_decode:
            for u8 in self._iter_device_png():
                yield u8
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


    def _iter_device_png(self):
        from .. import png_decode as D
        from . import kernels as K

        def read(name):
            """(Plan, None) of a file for the device, (None, array) of one that Pillow decoded"""
            if name.lower().endswith('.png'):
                with open(name, 'rb') as f:
                    plan, _ = D.parse(f.read())
                if plan is not None:
                    return plan, None
            return None, decode(name)

        def shape(item):
            return (item[0].height, item[0].width, 3) if item[0] is not None else item[1].shape

        with ThreadPoolExecutor(self.workers) as pool, ThreadPoolExecutor(1) as ahead:
            def batch(names):
                items = list(pool.map(read, names))
                if len({shape(it) for it in items}) != 1:
                    raise ValueError('images of one batch differ in size: %s' % ', '.join(
                        '%s %dx%d' % (os.path.basename(n), shape(it)[1], shape(it)[0]) for n, it in zip(names, items)))
                return items

            nxt = ahead.submit(batch, self.groups[0])
            for i in range(len(self.groups)):
                items = nxt.result()
                if i + 1 < len(self.groups):
                    nxt = ahead.submit(batch, self.groups[i + 1])
                on_dev = [k for k, it in enumerate(items) if it[0] is not None]
                on_host = [k for k, it in enumerate(items) if it[0] is None]
                status = []
                u8 = D.decode_plans_u8([items[k][0] for k in on_dev], self.device, statuses=status) if on_dev else None
                for j, st in enumerate(status):
                    if st:                                       # a bad stream: this file is Pillow's to read, or to refuse
                        arr = decode(self.groups[i][on_dev[j]])
                        if arr.shape != tuple(u8.shape[1:]):
                            raise ValueError('%s: the image is not of the size its header states' % self.groups[i][on_dev[j]])
                        u8[j] = torch.from_numpy(arr).to(self.device)
                if on_host:
                    host = torch.from_numpy(np.stack([items[k][1] for k in on_host])).pin_memory().to(self.device, non_blocking=True)
                    if on_dev:
                        full = torch.empty((len(items),) + tuple(host.shape[1:]), dtype=torch.uint8, device=self.device)
                        full[torch.tensor(on_dev, device=self.device)] = u8
                        full[torch.tensor(on_host, device=self.device)] = host
                        u8 = full
                    else:
                        u8 = host
                yield K.pil_resize_chain_u8(u8, self.img_size) if self.img_size is not None else u8


def batches_of(items, batch_size):
    return [items[i:i + batch_size] for i in range(0, len(items), batch_size)]
