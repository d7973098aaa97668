"""fp64 torch-CPU restatements of the reference's image-quality metrics (TEST INFRASTRUCTURE for hoig_amd.metrics).

  * the pytorch_fid "FID Inception" network (metrics/pytorch_fid/inception.py, FID variants of blocks A, C, E) with UNFOLDED
    BatchNorm (eps 1e-3), and fid_score.py's statistics;
  * LPIPS-AlexNet (metrics/lpips.py) and its path-level mean of batch means;
  * pytorch_msssim 0.2.1's ssim / ms_ssim;
  * get_eval_loader's preprocessing (PIL resizes, ToTensor, Normalize).

Also the seeded weight files with the real key names: He-scaled conv weights, BN running_var around 1, so activations stay O(1).
"""
import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

from quality_metrics import frechet_distance  # noqa: F401  (re-exported for the tests)

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
LPIPS_MU, LPIPS_SIGMA = (-0.03, -0.088, -0.188), (0.458, 0.448, 0.450)


# ----------------------------------------------------------------------------------------------------------- Inception
def _bc(name, ci, co, kh, kw=None, stride=1, ph=0, pw=None):
    return dict(name=name, ci=ci, co=co, k=(kh, kw if kw is not None else kh), stride=stride,
                pad=(ph, pw if pw is not None else ph))


def _a_layers(n, ci, pf):
    return [_bc(n + '.branch1x1', ci, 64, 1), _bc(n + '.branch5x5_1', ci, 48, 1), _bc(n + '.branch5x5_2', 48, 64, 5, ph=2),
            _bc(n + '.branch3x3dbl_1', ci, 64, 1), _bc(n + '.branch3x3dbl_2', 64, 96, 3, ph=1),
            _bc(n + '.branch3x3dbl_3', 96, 96, 3, ph=1), _bc(n + '.branch_pool', ci, pf, 1)]


def _c_layers(n, c7):
    L = [_bc(n + '.branch1x1', 768, 192, 1), _bc(n + '.branch7x7_1', 768, c7, 1), _bc(n + '.branch7x7_2', c7, c7, 1, 7, ph=0, pw=3),
         _bc(n + '.branch7x7_3', c7, 192, 7, 1, ph=3, pw=0), _bc(n + '.branch7x7dbl_1', 768, c7, 1)]
    for i, (kh, kw) in enumerate([(7, 1), (1, 7), (7, 1)], start=2):
        L.append(_bc(n + '.branch7x7dbl_%d' % i, c7, c7, kh, kw, ph=kh // 2, pw=kw // 2))
    return L + [_bc(n + '.branch7x7dbl_5', c7, 192, 1, 7, ph=0, pw=3), _bc(n + '.branch_pool', 768, 192, 1)]


def _e_layers(n, ci):
    return [_bc(n + '.branch1x1', ci, 320, 1), _bc(n + '.branch3x3_1', ci, 384, 1), _bc(n + '.branch3x3_2a', 384, 384, 1, 3, ph=0, pw=1),
            _bc(n + '.branch3x3_2b', 384, 384, 3, 1, ph=1, pw=0), _bc(n + '.branch3x3dbl_1', ci, 448, 1),
            _bc(n + '.branch3x3dbl_2', 448, 384, 3, ph=1), _bc(n + '.branch3x3dbl_3a', 384, 384, 1, 3, ph=0, pw=1),
            _bc(n + '.branch3x3dbl_3b', 384, 384, 3, 1, ph=1, pw=0), _bc(n + '.branch_pool', ci, 192, 1)]


def inception_layers():
    L = [_bc('Conv2d_1a_3x3', 3, 32, 3, stride=2), _bc('Conv2d_2a_3x3', 32, 32, 3), _bc('Conv2d_2b_3x3', 32, 64, 3, ph=1),
         _bc('Conv2d_3b_1x1', 64, 80, 1), _bc('Conv2d_4a_3x3', 80, 192, 3)]
    L += _a_layers('Mixed_5b', 192, 32) + _a_layers('Mixed_5c', 256, 64) + _a_layers('Mixed_5d', 288, 64)
    L += [_bc('Mixed_6a.branch3x3', 288, 384, 3, stride=2), _bc('Mixed_6a.branch3x3dbl_1', 288, 64, 1),
          _bc('Mixed_6a.branch3x3dbl_2', 64, 96, 3, ph=1), _bc('Mixed_6a.branch3x3dbl_3', 96, 96, 3, stride=2)]
    for n, c7 in (('Mixed_6b', 128), ('Mixed_6c', 160), ('Mixed_6d', 160), ('Mixed_6e', 192)):
        L += _c_layers(n, c7)
    L += [_bc('Mixed_7a.branch3x3_1', 768, 192, 1), _bc('Mixed_7a.branch3x3_2', 192, 320, 3, stride=2),
          _bc('Mixed_7a.branch7x7x3_1', 768, 192, 1), _bc('Mixed_7a.branch7x7x3_2', 192, 192, 1, 7, ph=0, pw=3),
          _bc('Mixed_7a.branch7x7x3_3', 192, 192, 7, 1, ph=3, pw=0), _bc('Mixed_7a.branch7x7x3_4', 192, 192, 3, stride=2)]
    return L + _e_layers('Mixed_7b', 1280) + _e_layers('Mixed_7c', 2048)


def inception_state_dict(seed=0, extras=True):
    """Seeded weights under pytorch_fid's key names (plus fc.*, AuxLogits.* and num_batches_tracked, which loaders ignore)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for l in inception_layers():
        co, ci, (kh, kw) = l['co'], l['ci'], l['k']
        sd[l['name'] + '.conv.weight'] = torch.randn(co, ci, kh, kw, generator=g) * (2.0 / (ci * kh * kw)) ** 0.5
        sd[l['name'] + '.bn.weight'] = 1.0 + 0.1 * torch.randn(co, generator=g)
        sd[l['name'] + '.bn.bias'] = 0.1 * torch.randn(co, generator=g)
        sd[l['name'] + '.bn.running_mean'] = 0.1 * torch.randn(co, generator=g)
        sd[l['name'] + '.bn.running_var'] = 1.0 + 0.2 * torch.rand(co, generator=g)
        if extras:
            sd[l['name'] + '.bn.num_batches_tracked'] = torch.tensor(0)
    if extras:
        sd['fc.weight'], sd['fc.bias'] = torch.randn(1008, 2048, generator=g) * 0.01, torch.zeros(1008)
        sd['AuxLogits.conv0.conv.weight'] = torch.randn(128, 768, 1, 1, generator=g)
    return sd


class InceptionRef(object):
    """fp64 NCHW forward of the FID Inception up to the block `dims` selects, then the global average (fid_score.py)."""

    def __init__(self, sd, dims=2048):
        self.sd = {k: v.double() for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()}
        self.meta = {l['name']: l for l in inception_layers()}
        self.dims = dims

    def conv(self, name, x):
        l, p = self.meta[name], self.sd
        y = F.conv2d(x, p[name + '.conv.weight'], None, l['stride'], l['pad'])
        y = F.batch_norm(y, p[name + '.bn.running_mean'], p[name + '.bn.running_var'], p[name + '.bn.weight'], p[name + '.bn.bias'],
                         False, 0.0, 1e-3)
        return F.relu(y)

    def seq(self, names, x):
        for n in names:
            x = self.conv(n, x)
        return x

    def block_a(self, n, x):
        c = lambda *k: self.seq([n + '.' + q for q in k], x)
        bp = self.conv(n + '.branch_pool', F.avg_pool2d(x, 3, 1, 1, count_include_pad=False))
        return torch.cat([c('branch1x1'), c('branch5x5_1', 'branch5x5_2'), c('branch3x3dbl_1', 'branch3x3dbl_2', 'branch3x3dbl_3'),
                          bp], 1)

    def block_c(self, n, x):
        c = lambda *k: self.seq([n + '.' + q for q in k], x)
        bp = self.conv(n + '.branch_pool', F.avg_pool2d(x, 3, 1, 1, count_include_pad=False))
        return torch.cat([c('branch1x1'), c('branch7x7_1', 'branch7x7_2', 'branch7x7_3'),
                          c(*['branch7x7dbl_%d' % i for i in range(1, 6)]), bp], 1)

    def block_e(self, n, x, maxpool):
        t = self.conv(n + '.branch3x3_1', x)
        u = self.seq([n + '.branch3x3dbl_1', n + '.branch3x3dbl_2'], x)
        p = F.max_pool2d(x, 3, 1, 1) if maxpool else F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)
        return torch.cat([self.conv(n + '.branch1x1', x),
                          torch.cat([self.conv(n + '.branch3x3_2a', t), self.conv(n + '.branch3x3_2b', t)], 1),
                          torch.cat([self.conv(n + '.branch3x3dbl_3a', u), self.conv(n + '.branch3x3dbl_3b', u)], 1),
                          self.conv(n + '.branch_pool', p)], 1)

    def blocks(self, x):
        """x: (N, 3, 299, 299) in [-1, 1] fp64 -> the selected block's map."""
        x = F.max_pool2d(self.seq(['Conv2d_1a_3x3', 'Conv2d_2a_3x3', 'Conv2d_2b_3x3'], x), 3, 2)
        if self.dims == 64:
            return x
        x = F.max_pool2d(self.seq(['Conv2d_3b_1x1', 'Conv2d_4a_3x3'], x), 3, 2)
        if self.dims == 192:
            return x
        for n in ('Mixed_5b', 'Mixed_5c', 'Mixed_5d'):
            x = self.block_a(n, x)
        x = torch.cat([self.conv('Mixed_6a.branch3x3', x),
                       self.seq(['Mixed_6a.branch3x3dbl_1', 'Mixed_6a.branch3x3dbl_2', 'Mixed_6a.branch3x3dbl_3'], x),
                       F.max_pool2d(x, 3, 2)], 1)
        for n in ('Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e'):
            x = self.block_c(n, x)
        if self.dims == 768:
            return x
        x = torch.cat([self.seq(['Mixed_7a.branch3x3_1', 'Mixed_7a.branch3x3_2'], x),
                       self.seq(['Mixed_7a.branch7x7x3_%d' % i for i in range(1, 5)], x), F.max_pool2d(x, 3, 2)], 1)
        return self.block_e('Mixed_7c', self.block_e('Mixed_7b', x, False), True)

    def features(self, images01):
        """(N, 3, H, W) in [0, 1] -> (N, dims): bilinear to 299 (align_corners=False), 2x - 1, blocks, global average."""
        x = F.interpolate(images01.double(), size=(299, 299), mode='bilinear', align_corners=False)
        return self.blocks(2 * x - 1).mean(dim=(2, 3))


# ----------------------------------------------------------------------------------------------------------- LPIPS
ALEX = [(0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1)]


def alexnet_state_dict(seed=1, prefix='features.'):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, ci, co, k, _, _ in ALEX:
        sd['%s%d.weight' % (prefix, i)] = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
        sd['%s%d.bias' % (prefix, i)] = 0.05 * torch.randn(co, generator=g)
    if prefix == 'features.':
        sd['classifier.1.weight'] = torch.randn(16, 16, generator=g)
    return sd


def lpips_state_dict(seed=2):
    g = torch.Generator().manual_seed(seed)
    return {'lpips_weights.%d.main.1.weight' % j: torch.rand(1, co, 1, 1, generator=g) / co * 8 for j, (_, _, co, _, _, _) in
            enumerate(ALEX)}


class LPIPSRef(object):
    def __init__(self, alex_sd, lpips_sd):
        self.alex = [(alex_sd['features.%d.weight' % i].double(), alex_sd['features.%d.bias' % i].double(), s, p)
                     for i, _, _, _, s, p in ALEX]
        self.heads = [lpips_sd['lpips_weights.%d.main.1.weight' % j].double() for j in range(5)]

    def fmaps(self, x):
        out = []
        for j, (w, b, s, p) in enumerate(self.alex):
            if j in (1, 2):
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, w, b, s, p))
            out.append(x)
        return out

    def per_image(self, x, y):
        """(N,) per-image LPIPS of two loader-normalised (N, 3, H, W) batches (lpips.py forward before its mean over N)."""
        mu, sigma = torch.tensor(LPIPS_MU).double().view(1, 3, 1, 1), torch.tensor(LPIPS_SIGMA).double().view(1, 3, 1, 1)
        fx, fy = self.fmaps((x.double() - mu) / sigma), self.fmaps((y.double() - mu) / sigma)
        val = 0
        for a, b, w in zip(fx, fy, self.heads):
            val = val + lpips_layer(a.flatten(2).transpose(1, 2), b.flatten(2).transpose(1, 2), w.view(-1))
        return val


def lpips_layer(fx, fy, w, dtype=torch.float64):
    """(B,) distance of one layer: [B, HW, C] maps, (C,) weight, fp64.  Both maps are scaled to unit channel norm per pixel
    (eps 1e-10 under the root), then mean over pixels of sum_c w_c (x_c - y_c)^2.  (dtype=torch.float32: the same statement in
    fp32, for the floor of the number format.)"""
    fx, fy, w = fx.to(dtype), fy.to(dtype), w.to(dtype).view(-1)
    nx = fx * torch.rsqrt((fx ** 2).sum(-1, keepdim=True) + 1e-10)
    ny = fy * torch.rsqrt((fy ** 2).sum(-1, keepdim=True) + 1e-10)
    return (w * (nx - ny) ** 2).sum(-1).mean(-1)


def lpips_given_batches(model, xs, ys, batch_size):
    """lpips.py calculate_lpips_given_paths: the mean of the per-batch means."""
    means = [model.per_image(xs[i:i + batch_size], ys[i:i + batch_size]).mean() for i in range(0, xs.shape[0], batch_size)]
    return torch.stack(means).mean().item()


# ----------------------------------------------------------------------------------------------------------- SSIM
def gauss_window(size=11, sigma=1.5):
    t = torch.arange(size, dtype=torch.float64) - size // 2
    g = torch.exp(-(t ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def _filter(x, g):
    C = x.shape[1]
    x = F.conv2d(x, g.view(1, 1, 1, -1).repeat(C, 1, 1, 1), groups=C)
    return F.conv2d(x, g.view(1, 1, -1, 1).repeat(C, 1, 1, 1), groups=C)


def ssim_pair(B, C, H, W, scale=1.0, seed=0):
    """(X, Y) fp32 (B, C, H, W) in [0, scale]: a smooth map (5x5 average of rand) and its mix with fresh noise, the map's share
    running from 0.2 to 0.9 across the batch, so that SSIM goes from far apart to close."""
    g = torch.Generator().manual_seed(seed)
    base = F.avg_pool2d(torch.rand(B, C, H, W, generator=g), 5, 1, 2)
    other = torch.rand(B, C, H, W, generator=g)
    mix = torch.linspace(0.2, 0.9, B).view(B, 1, 1, 1)
    return base * scale, (mix * base + (1 - mix) * other) * scale


def ssim_level(X, Y, data_range, win=11, sigma=1.5, K=(0.01, 0.03), dtype=torch.float64):
    """(ssim, cs) per (image, channel), fp64 (dtype=torch.float32: the same statement in fp32, whose distance to fp64 is the floor
    of the number format)."""
    g = gauss_window(win, sigma).to(dtype)
    X, Y = X.to(dtype), Y.to(dtype)
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    m1, m2 = _filter(X, g), _filter(Y, g)
    s11, s22, s12 = _filter(X * X, g) - m1 ** 2, _filter(Y * Y, g) - m2 ** 2, _filter(X * Y, g) - m1 * m2
    cs = (2 * s12 + C2) / (s11 + s22 + C2)
    s = (2 * m1 * m2 + C1) / (m1 ** 2 + m2 ** 2 + C1) * cs
    return s.flatten(2).mean(-1), cs.flatten(2).mean(-1)


MS_WEIGHTS = [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]


def ms_ssim_per_channel(X, Y, data_range, win=11, sigma=1.5, K=(0.01, 0.03)):
    X, Y = X.double(), Y.double()
    mcs = []
    for i in range(5):
        s, cs = ssim_level(X, Y, data_range, win, sigma, K)
        if i < 4:
            mcs.append(torch.relu(cs))
            pad = (X.shape[2] % 2, X.shape[3] % 2)
            X, Y = F.avg_pool2d(X, 2, padding=pad), F.avg_pool2d(Y, 2, padding=pad)
    v = torch.stack(mcs + [torch.relu(s)])
    return torch.prod(v ** torch.tensor(MS_WEIGHTS, dtype=torch.float64).view(-1, 1, 1), dim=0)


# ----------------------------------------------------------------------------------------------------------- loaders
def to_tensor(arr):
    """ToTensor of HWC uint8 -> (3, H, W) float32 in [0, 1]."""
    return torch.from_numpy(np.ascontiguousarray(arr)).permute(2, 0, 1).float().div(255)


def eval_loader_tensor(path, img_size=256):
    """get_eval_loader's transform on one file: Resize([img_size]*2), Resize([299]*2), ToTensor, ImageNet Normalize (fp32)."""
    img = Image.open(path).convert('RGB').resize((img_size, img_size), Image.BILINEAR).resize((299, 299), Image.BILINEAR)
    t = to_tensor(np.asarray(img))
    mean, std = torch.tensor(IMAGENET_MEAN).view(3, 1, 1), torch.tensor(IMAGENET_STD).view(3, 1, 1)
    return (t - mean) / std


def fid_tensor(path):
    """fid_score.py's dataset: ToTensor of the RGB image."""
    return to_tensor(np.asarray(Image.open(path).convert('RGB')))


def write_pngs(dirname, n, side, seed, prefix='img'):
    """n seeded RGB PNGs side x side (smooth gradients plus noise, so that SSIM's structure terms see something)."""
    import os
    rng = np.random.RandomState(seed)
    os.makedirs(dirname, exist_ok=True)
    yy, xx = np.mgrid[0:side, 0:side] / float(side)
    names = []
    for i in range(n):
        base = np.stack([np.sin(6.28 * (xx * rng.uniform(0.5, 3) + rng.uniform())) ,
                         np.cos(6.28 * (yy * rng.uniform(0.5, 3) + rng.uniform())),
                         xx * yy], -1) * 0.5 + 0.5
        img = np.clip(base * 200 + rng.uniform(0, 55, size=base.shape), 0, 255).astype(np.uint8)
        name = os.path.join(dirname, '%s_%03d.png' % (prefix, i))
        Image.fromarray(img).save(name)
        names.append(name)
    return names
