"""Shared by tests/test_d_augment_cpu.py and tests/test_d_augment_gpu.py (docs/d_augment.md): the CPU twins of the hoig_daug_* entry
points behind numpy arguments; an independent statement of the draws (Philox4x32-10 and the word table in Python integers) and of
the adaptive controller (Python doubles); DiffAugment's published functions (Zhao et al. 2020, DiffAugment_pytorch.py) in float64
torch with the random numbers taken from a record instead of torch.rand, composed as colour, translation, cutout; and the fp32 error
bounds that the tests derive from the operation counts."""
import itertools
import struct

import numpy as np
import torch

COLOR, TRANSLATION, CUTOUT = 1, 2, 4
STATE_WORDS, MAX_PARTS, THREADS = 16, 16, 256
STEP, P, POS, NEG, TOTAL, STEPS, SEED, RANK, TARGET, INTERVAL, INCREMENT, POLICY, RT, ADJUSTS = range(14)
POLICIES = tuple(sum(c) for r in range(1, 4) for c in itertools.combinations((COLOR, TRANSLATION, CUTOUT), r))      # every non-empty subset
SHAPES = ((5, 7), (8, 8), (6, 10), (9, 4), (16, 16))
KS = (1, 2, 4, 7, 16)
U = 2.0 ** -24                       # the unit roundoff of fp32


# ------------------------------------------------------------------------------------------------ buffers and twins
def aligned(n, dtype, fill=None):
    """An array of n elements whose first byte is 16-byte aligned."""
    item = np.dtype(dtype).itemsize
    raw = np.zeros(n + 16 // item, dtype=dtype)
    skip = (-raw.ctypes.data % 16) // item
    out = raw[skip:skip + n]
    assert out.ctypes.data % 16 == 0
    if fill is not None:
        out[:] = fill
    return out


def _f2w(x):
    return struct.unpack('<Q', struct.pack('<d', float(x)))[0]


def _w2f(w):
    return struct.unpack('<d', struct.pack('<Q', int(w)))[0]


def make_state(step=0, p=1.0, policy=7, seed=0, rank=0, target=0.6, interval=4, increment=0.0):
    s = aligned(STATE_WORDS, np.uint64, 0)
    s[STEP], s[P], s[SEED], s[RANK], s[TARGET], s[INTERVAL], s[INCREMENT], s[POLICY] = (
        step, _f2w(p), seed, rank, _f2w(target), interval, _f2w(increment), policy)
    return s


def state_p(s):
    return _w2f(s[P])


def _ptr(a):
    if a is None:
        return None
    return a.data_ptr() if torch.is_tensor(a) else a.ctypes.data


def _lib():
    from hoig_amd import _lib as L
    return L.lib


def tick_host(state):
    return _lib().hoig_daug_tick_host(_ptr(state))


def draw_host(state, site, B, H, W, params):
    return _lib().hoig_daug_draw_host(_ptr(state), site, B, H, W, _ptr(params))


def adapt_host(state, d_real, n):
    return _lib().hoig_daug_adapt_host(_ptr(state), _ptr(d_real), n)


def fwd_host(img, cond, params, out, B, H, W, k, ws):
    return _lib().hoig_daug_fwd_host(_ptr(img), _ptr(cond), _ptr(params), _ptr(out), B, H, W, k, _ptr(ws))


def bwd_host(g, params, dimg, B, H, W, k, ws):
    return _lib().hoig_daug_bwd_host(_ptr(g), _ptr(params), _ptr(dimg), B, H, W, k, _ptr(ws))


def twin_draw(state, site, B, H, W):
    params = aligned(B * 8, np.uint32, 0xDEADBEEF)
    assert draw_host(state, site, B, H, W, params) == 0
    return params.reshape(B, 8)


def twin_fwd(img, cond, params):
    """img [B,H,W,3], cond [B,H,W,k] float32, params [B,8] uint32 -> out [B,H,W,3+k] through the twin."""
    B, H, W, _ = img.shape
    k = cond.shape[-1]
    a, c = aligned(img.size, np.float32, img.ravel()), aligned(cond.size, np.float32, cond.ravel())
    pr = aligned(B * 8, np.uint32, params.ravel())
    out, ws = aligned(B * H * W * (3 + k), np.float32, np.nan), aligned(B * MAX_PARTS, np.float32, 0)
    assert fwd_host(a, c, pr, out, B, H, W, k, ws) == 0
    return out.reshape(B, H, W, 3 + k)


def twin_bwd(g, params):
    B, H, W, C = g.shape
    ga, pr = aligned(g.size, np.float32, g.ravel()), aligned(B * 8, np.uint32, params.ravel())
    dimg, ws = aligned(B * H * W * 3, np.float32, np.nan), aligned(B * MAX_PARTS, np.float32, 0)
    assert bwd_host(ga, pr, dimg, B, H, W, C - 3, ws) == 0
    return dimg.reshape(B, H, W, 3)


# ------------------------------------------------------------------------------------------------ the draws in Python integers
M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011): four counter words and two key words -> four output words."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def uniform(w):
    return np.float32(w >> 8) * np.float32(2.0 ** -24)


def shift_of(n):
    return int(n * 0.125 + 0.5)


def cut_of(n):
    return int(n * 0.5 + 0.5)


def f32_bits(f):
    return int(np.array([f], dtype=np.float32).view(np.uint32)[0])


def py_draw(step, site, B, H, W, p, policy, seed=0, rank=0):
    """The issue's statement of the records: uint32 [B, 8]."""
    out = np.zeros((B, 8), dtype=np.uint32)
    pf = np.float32(p)
    for i in range(B):
        w = []
        for j in range(3):
            w += philox4x32_10((step & M32, (step >> 32) & M32, site, 3 * i + j), (seed & M32, rank & M32))
        color = bool(policy & COLOR) and uniform(w[0]) < pf
        trans = bool(policy & TRANSLATION) and uniform(w[1]) < pf
        cut = bool(policy & CUTOUT) and uniform(w[2]) < pf
        b, s, k = np.float32(0), np.float32(1), np.float32(1)
        if color:
            b, s, k = uniform(w[3]) - np.float32(0.5), uniform(w[4]) * np.float32(2), uniform(w[5]) + np.float32(0.5)
        ty = tx = cy0 = cx0 = 0
        if trans:
            sy, sx = shift_of(H), shift_of(W)
            ty, tx = ((w[6] * (2 * sy + 1)) >> 32) - sy, ((w[7] * (2 * sx + 1)) >> 32) - sx
        if cut:
            zy, zx = cut_of(H), cut_of(W)
            cy0, cx0 = ((w[8] * (H + 1 - zy % 2)) >> 32) - zy // 2, ((w[9] * (W + 1 - zx % 2)) >> 32) - zx // 2
        out[i] = [f32_bits(b), f32_bits(s), f32_bits(k), ty & M32, tx & M32, cy0 & M32, cx0 & M32,
                  (COLOR if color else 0) | (TRANSLATION if trans else 0) | (CUTOUT if cut else 0)]
    return out


def record(b=0.0, s=1.0, k=1.0, ty=0, tx=0, cy0=0, cx0=0, flags=0):
    return np.array([f32_bits(b), f32_bits(s), f32_bits(k), ty & M32, tx & M32, cy0 & M32, cx0 & M32, flags], dtype=np.uint32)


def unpack(rec):
    f = rec[:3].copy().view(np.float32)
    i = rec[3:7].copy().view(np.int32)
    return float(f[0]), float(f[1]), float(f[2]), int(i[0]), int(i[1]), int(i[2]), int(i[3]), int(rec[7])


class PyController(object):
    """hoig_daug_adapt in Python doubles and integers."""

    def __init__(self, p, target, interval, increment):
        self.p, self.target, self.interval, self.increment = float(p), float(target), int(interval), float(increment)
        self.pos = self.neg = self.total = self.steps = 0
        self.rt = 0.0

    def feed(self, pos, neg, n):
        self.pos, self.neg, self.total, self.steps = self.pos + pos, self.neg + neg, self.total + n, self.steps + 1
        if self.steps < self.interval:
            return
        self.rt = (self.pos - self.neg) / self.total
        d = self.rt - self.target
        self.p = min(1.0, max(0.0, self.p + (self.increment if d > 0 else (-self.increment if d < 0 else 0.0))))
        self.pos = self.neg = self.total = self.steps = 0


# ------------------------------------------------------------------------------------------------ DiffAugment in float64
# DiffAugment_pytorch.py (NCHW), with each torch.rand / torch.randint replaced by the number the record holds.
def _rand_brightness(x, r):
    return x + (r - 0.5)


def _rand_saturation(x, r):
    x_mean = x.mean(dim=1, keepdim=True)
    return (x - x_mean) * (r * 2) + x_mean


def _rand_contrast(x, r):
    x_mean = x.mean(dim=[1, 2, 3], keepdim=True)
    return (x - x_mean) * (r + 0.5) + x_mean


def _rand_translation(x, translation_x, translation_y):
    grid_batch, grid_x, grid_y = torch.meshgrid(torch.arange(x.size(0), dtype=torch.long), torch.arange(x.size(2), dtype=torch.long),
                                                torch.arange(x.size(3), dtype=torch.long), indexing='ij')
    grid_x = torch.clamp(grid_x + translation_x + 1, 0, x.size(2) + 1)
    grid_y = torch.clamp(grid_y + translation_y + 1, 0, x.size(3) + 1)
    x_pad = torch.nn.functional.pad(x, [1, 1, 1, 1, 0, 0, 0, 0])
    return x_pad.permute(0, 2, 3, 1).contiguous()[grid_batch, grid_x, grid_y].permute(0, 3, 1, 2)


def _rand_cutout(x, offset_x, offset_y, ratio=0.5):
    cutout_size = int(x.size(2) * ratio + 0.5), int(x.size(3) * ratio + 0.5)
    grid_batch, grid_x, grid_y = torch.meshgrid(torch.arange(x.size(0), dtype=torch.long), torch.arange(cutout_size[0], dtype=torch.long),
                                                torch.arange(cutout_size[1], dtype=torch.long), indexing='ij')
    grid_x = torch.clamp(grid_x + offset_x - cutout_size[0] // 2, min=0, max=x.size(2) - 1)
    grid_y = torch.clamp(grid_y + offset_y - cutout_size[1] // 2, min=0, max=x.size(3) - 1)
    mask = torch.ones(x.size(0), x.size(2), x.size(3), dtype=x.dtype)
    mask[grid_batch, grid_x, grid_y] = 0
    return x * mask.unsqueeze(1)


def diffaugment_f64(img, cond, params, g=None):
    """img [B,H,W,3], cond [B,H,W,k] (numpy float32), params [B,8] -> the float64 output [B,H,W,3+k]; with g (the gradient of the
    output) also the float64 gradient with respect to img.  Sample by sample: colour on the image, then translation and cutout on
    image | cond.  A handcrafted box that lies wholly outside the map cuts nothing (no drawn centre gives one; see _cut_box)."""
    B, H, W, _ = img.shape
    outs, grads = [], []
    for i in range(B):
        b, s, k, ty, tx, cy0, cx0, flags = unpack(params[i])
        x = torch.from_numpy(img[i:i + 1].astype(np.float64)).permute(0, 3, 1, 2).requires_grad_(True)
        c = torch.from_numpy(cond[i:i + 1].astype(np.float64)).permute(0, 3, 1, 2)
        y = x
        if flags & COLOR:
            y = _rand_contrast(_rand_saturation(_rand_brightness(y, b + 0.5), s / 2), k - 0.5)
        y = torch.cat([y, c], dim=1)
        if flags & TRANSLATION:
            y = _rand_translation(y, torch.tensor([[[ty]]]), torch.tensor([[[tx]]]))
        if flags & CUTOUT:
            zy, zx = cut_of(H), cut_of(W)
            if cy0 + zy > 0 and cy0 < H and cx0 + zx > 0 and cx0 < W:
                y = _cut_box(y, cy0, cx0, zy, zx)
        y = y.permute(0, 2, 3, 1)
        outs.append(y.detach().numpy()[0])
        if g is not None:
            y.backward(torch.from_numpy(g[i:i + 1].astype(np.float64)))
            grads.append(x.grad.permute(0, 2, 3, 1).numpy()[0])
    return (np.stack(outs), np.stack(grads)) if g is not None else np.stack(outs)


def _cut_box(y, cy0, cx0, zy, zx):
    """rand_cutout with the centre that gives the box origin (cy0, cx0).  Its clamp maps the rows of a box that hangs over an edge onto
    the border row; the box of the record is clipped instead, so a box over an edge is cut here as the intersection (for a drawn centre
    both are the same set: the clamped rows are inside the box already whenever the box reaches the border)."""
    H, W = y.size(2), y.size(3)
    if cy0 + zy // 2 >= 0 and cx0 + zx // 2 >= 0 and cy0 + zy // 2 < H + 1 - zy % 2 and cx0 + zx // 2 < W + 1 - zx % 2:
        return _rand_cutout(y, torch.tensor([[[cy0 + zy // 2]]]), torch.tensor([[[cx0 + zx // 2]]]))
    mask = torch.ones(1, H, W, dtype=y.dtype)
    mask[:, max(cy0, 0):max(min(cy0 + zy, H), 0), max(cx0, 0):max(min(cx0 + zx, W), 0)] = 0
    return y * mask.unsqueeze(1)


# ------------------------------------------------------------------------------------------------ the fp32 bounds
def parts_of(units):
    return min(MAX_PARTS, max(1, -(-units // (4 * THREADS))))


def sum_depth(units, per_unit):
    """The most fp32 additions one term passes through in a reduction: its thread's run, eight tree levels, the partials."""
    parts = parts_of(units)
    chunk = -(-units // parts)
    return per_unit * -(-chunk // THREADS) + 8 + (parts - 1)


def fwd_bound(H, W):
    """See test_forward_twin_against_diffaugment_in_float64."""
    depth = sum_depth(-(-3 * H * W // 4), 4) + 1          # (+ the division by 3HW)
    e_mu = depth * U + 8 * U
    return 8 * U * 30.5 + 2.5 * e_mu


def bwd_bound(H, W):
    """See test_backward_twin_against_diffaugment_in_float64."""
    depth = sum_depth(H * W, 3) + 3                       # (+ 1 - k, the product, the division)
    return 8 * U * 10 + depth * U
