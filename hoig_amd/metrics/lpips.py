"""LPIPS-AlexNet on the HIP path (metrics/lpips.py), with the reference's names; weight arguments come after the existing ones.

AlexNet's five convolutions run on hoig_conv2d_fwd (bias + ReLU in the epilogue; default arithmetic the three-term 16-bit forward,
``precision='bf16x3'``, or ``'f32'``), its max pools on hoig_pool2d_fwd; each of the five layers' distances is one hoig_lpips_layer
launch.  x and y go through AlexNet together, as one batch of 2N.
"""
import os

import torch

from .. import _lib as L
from .. import ops as O
from . import images as I
from . import kernels as K
from .weights import ALEXNET_FILE, LPIPS_FILE, hub_path, resolve, take

# torchvision alexnet().features: (index, Ci, Co, k, stride, pad); LPIPS reads the ReLU after each
ALEXNET_CONVS = [(0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1)]


def load_alexnet(weights):
    """[(w, b)] fp64 of the five convolutions; keys `features.<i>.*` (torchvision) or `alexnet.layers.<i>.*` (the reference's LPIPS
    module)."""
    sd, src = resolve(weights, [hub_path(ALEXNET_FILE)], 'AlexNet')
    prefix = 'alexnet.layers.' if any(k.startswith('alexnet.layers.') for k in sd) else 'features.'
    return [(take(sd, src, '%s%d.weight' % (prefix, i), (co, ci, k, k)), take(sd, src, '%s%d.bias' % (prefix, i), (co,)))
            for i, ci, co, k, _, _ in ALEXNET_CONVS]


def load_lpips_heads(weights):
    """The five (C,) weights of `lpips_weights.<i>.main.1.weight` ((1, C, 1, 1) in the file)."""
    sd, src = resolve(weights, [os.path.join('metrics', LPIPS_FILE), hub_path(LPIPS_FILE)], 'LPIPS heads')
    return [take(sd, src, 'lpips_weights.%d.main.1.weight' % i, (1, co, 1, 1)).view(co) for i, (_, _, co, _, _, _) in
            enumerate(ALEXNET_CONVS)]


class LPIPS(object):
    """forward(x, y) -> per-image LPIPS (N,) of two (N, 3, H, W) batches in get_eval_loader's normalisation; the reference's value
    for a batch is their mean.  The weights are looked for at the given paths (or state dicts), else AlexNet in torch hub's
    checkpoints and the heads at metrics/lpips_weights.ckpt (relative to the working directory), then in torch hub's checkpoints;
    without them this raises RuntimeError."""

    def __init__(self, alexnet_weights=None, lpips_weights=None, precision=None, device=None):
        self.prec = K.precision_code(precision)
        alex, heads = load_alexnet(alexnet_weights), load_lpips_heads(lpips_weights)
        self.device = torch.device(device if device is not None else 'cuda')
        owner = K._WeightOwner()
        self.convs = [K.Conv(w, b, s, (p, p), True, self.device, owner) for (w, b), (_, _, _, _, s, p) in zip(alex, ALEXNET_CONVS)]
        self.heads = [h.float().to(self.device).contiguous() for h in heads]

    def features(self, x):
        """The five ReLU maps (NHWC) of AlexNet on x (NHWC, already scaled by (x - mu) / sigma)."""
        c = self.convs
        f1 = c[0](x, self.prec)
        f2 = c[1](K.pool2d(f1, 3, 2), self.prec)
        f3 = c[2](K.pool2d(f2, 3, 2), self.prec)
        f4 = c[3](f3, self.prec)
        return [f1, f2, f3, f4, c[4](f4, self.prec)]

    def distance(self, xy):
        """xy: [2N, H, W, 3] (x images then y images, scaled for AlexNet) -> (N,) fp32."""
        n = xy.shape[0] // 2
        out = torch.zeros(n, dtype=torch.float32, device=xy.device)
        with torch.no_grad():
            fmaps = self.features(xy)
            ws = max(L.lib.hoig_lpips_workspace_bytes(n, f.shape[1] * f.shape[2]) for f in fmaps)
            work = torch.zeros(ws, dtype=torch.uint8, device=xy.device)
            for f, w in zip(fmaps, self.heads):
                _, H, W, C = f.shape
                L.call('hoig_lpips_layer', O._p(f), O._p(f[n:]), O._p(w), O._p(out), n, H * W, C, O._p(work), O._st())
        return out

    def forward(self, x, y):
        with torch.no_grad():
            xy = K.nchw_to_nhwc(torch.cat([x, y]).float())
            mu = torch.tensor(K.LPIPS_MU, device=xy.device)
            sigma = torch.tensor(K.LPIPS_SIGMA, device=xy.device)
            return self.distance(((xy - mu) / sigma).contiguous())

    __call__ = forward

    def distance_u8(self, u8):
        """uint8 [2N, 299, 299, 3] (decoded and resized on the host) -> (N,): ToTensor, ImageNet Normalize, then (x - mu) / sigma."""
        return self.distance(K.stage_images_u8(u8, None, [(K.IMAGENET_MEAN, K.IMAGENET_STD), (K.LPIPS_MU, K.LPIPS_SIGMA)]))


def paired_batches(paths, batch_size):
    """File groups of [batch of paths[0] | same batch of paths[1]] (both directories sorted, equal counts)."""
    a, b = I.list_images(paths[0]), I.list_images(paths[1])
    if len(a) != len(b):
        raise ValueError('%s holds %d images, %s %d' % (paths[0], len(a), paths[1], len(b)))
    return [x + y for x, y in zip(I.batches_of(a, batch_size), I.batches_of(b, batch_size))]


def calculate_lpips_given_images(gen_images, gt_images, alexnet_weights=None, lpips_weights=None, precision=None, model=None):
    """Per-image LPIPS (N,) of two (N, 3, H, W) batches (lpips.py: one value per frame)."""
    model = model or LPIPS(alexnet_weights, lpips_weights, precision, gen_images.device)
    return model(gen_images, gt_images)


def calculate_lpips_given_paths(paths, img_size=256, batch_size=50, alexnet_weights=None, lpips_weights=None, precision=None,
                                device=None, model=None, device_resize=False, device_png_decode=None):
    """LPIPS between two directories of images (sorted, paired by position), in get_eval_loader's preprocessing (PIL resize to
    img_size, then to 299, ImageNet normalisation).  As in lpips.py, the result is the MEAN OF PER-BATCH MEANS: a short last batch
    counts as much as a full one (7 images in batches of 3 weigh the 7th image three times as much as each of the others).
    device_resize: the workers only decode and the two PIL resizes run on the device (kernels.pil_resize_chain_u8: the same bytes,
    so the same value).  device_png_decode (HOIG_DEVICE_PNG_DECODE=1): the supported PNG files are decoded on the device too
    (images.DeviceBatches); it implies device_resize."""
    device_png_decode = I.png_decode_option(device_png_decode)
    device_resize = device_resize or device_png_decode
    print('Calculating LPIPS given paths %s and %s...' % (paths[0], paths[1]))
    model = model or LPIPS(alexnet_weights, lpips_weights, precision, device)
    batches = I.DeviceBatches(paired_batches(paths, batch_size), model.device, None if device_resize else img_size,
                              device_png_decode=device_png_decode)
    if device_resize:
        batches = (K.pil_resize_chain_u8(u8, img_size) for u8 in batches)
    means = [model.distance_u8(u8).mean() for u8 in batches]
    return torch.stack(means).double().mean().item()
