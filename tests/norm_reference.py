"""References, error measures and input makers of the instance-norm tests (tests/test_norm_cpu.py, tests/test_norm_gpu.py).

The reference of every check is torch.nn.functional.instance_norm + autograd in FLOAT64 on the CPU, fed the same fp32 values the
kernel reads.  The bound of a conditioning case is not a constant: torch's own fp32 CPU instance_norm -- the stable two-pass
algorithm, whose error grows like |mean|/sigma * 2^-24, the best an fp32 kernel can do on fp32 input -- is run on the same input,
e_ref is its error against float64, and a kernel has to stay inside max(8 * e_ref, 2e-6): a differently ordered but equally stable
summation (lanes, LDS tree, atomics) stays within 3 x e_ref; the floor covers ratio 0, where e_ref is 1e-7 and summation order alone
would fail.  fp32 emulations of the three formulas the kernels have used (two-pass, sums shifted by a pivot, plain sums) let
test_norm_cpu.py show, without a GPU, that the bound is reachable and that the inputs tell the formulas apart.

Tensors here are NHWC (the kernels' layout) unless a name says otherwise.
"""
import torch
import torch.nn.functional as F

EPS = 1e-5
TOL = 1e-4                 # the suite's operator bound on well-conditioned input (forward; 5 * TOL for gradients)
RATIOS = (0.0, 3.0, 10.0, 30.0, 100.0, 1000.0)
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2


def bound(e_ref):
    return max(8.0 * e_ref, 2e-6)


# ------------------------------------------------------------------------------------------------------------ error measures
def rel_err(a, b):
    """max |a-b| / max |b| over the tensor (tests/gpu_util.py:rel_err)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def chan_err(a, b):
    """max over channels (last dim) of  max |a-b| over the channel / max |b| over the channel: an error confined to one channel of a
    tensor is not hidden behind the tensor's largest element."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    C = b.shape[-1]
    d = (a - b).abs().reshape(-1, C).max(dim=0).values
    s = b.abs().reshape(-1, C).max(dim=0).values.clamp_min(1e-30)
    return (d / s).max().item()


def img_chan_err(a, b, scale_from=None):
    """The same per (image, channel) of a [B, ..., C] tensor -> [B, C] (the unit an instance norm works on).  scale_from: the tensor
    whose per-(image, channel) maximum is the scale, when that is not b itself -- the output BEFORE a (Leaky)ReLU: the activation is
    1-Lipschitz, so the error of act(u) is an error of u and is measured against the range of u; a channel whose large values are
    all negative would otherwise be judged against the few small ones that survive."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    B, C = b.shape[0], b.shape[-1]
    d = (a - b).abs().reshape(B, -1, C).max(dim=1).values
    s = (b if scale_from is None else scale_from.detach().double().cpu()).abs().reshape(B, -1, C).max(dim=1).values.clamp_min(1e-30)
    return d / s


def mean_err(mean, ref):
    """Error of a mean in units of the channel's scale |mean| + sigma -> [B, C] (relative to |mean| alone it is meaningless for
    a centred channel).  ref = stats64(x)."""
    m = mean.detach().double().cpu().reshape(ref['mean'].shape)
    return (m - ref['mean']).abs() / (ref['mean'].abs() + ref['sigma']).clamp_min(1e-30)


def rstd_err(rstd, ref):
    r = rstd.detach().double().cpu().reshape(ref['rstd'].shape)
    return (r - ref['rstd']).abs() / ref['rstd']


# ---------------------------------------------------------------------------------------------------------------- references
def stats64(x, eps=EPS):
    """float64 mean / sigma / rstd per (image, channel) of an NHWC fp32 tensor."""
    x64 = x.detach().double().cpu()
    B, C = x64.shape[0], x64.shape[-1]
    v = x64.reshape(B, -1, C)
    mean = v.mean(dim=1)
    var = ((v - mean[:, None]) ** 2).mean(dim=1)
    return dict(mean=mean, sigma=var.sqrt(), rstd=1.0 / (var + eps).sqrt())


def stats32_torch(x, eps=EPS):
    """What torch's fp32 CPU reductions make of the same values (the e_ref of mean / rstd)."""
    x = x.detach().float().cpu()
    B, C = x.shape[0], x.shape[-1]
    v = x.reshape(B, -1, C).transpose(1, 2).contiguous()          # [B, C, HW]: each channel contiguous, as in NCHW
    mean = v.mean(dim=2)
    var = v.var(dim=2, unbiased=False)
    return mean, 1.0 / (var + eps).sqrt()


def _act(t, act, slope):
    if act == ACT_RELU:
        return F.relu(t)
    if act == ACT_LRELU:
        return F.leaky_relu(t, slope)
    return t


def reference(x, mode=0, p0=None, p1=None, act=ACT_NONE, slope=0.0, residual=None, dy=None, addend=None, mask_from=None, dtype=torch.float64,
              eps=EPS):
    """instance norm + epilogue (+ backward when dy is given) on the CPU in `dtype`, from NHWC fp32 values.
    mode 0: plain; 1: affine p0 = weight[C], p1 = bias[C]; 2: SPADE p0 = gamma, p1 = beta (NHWC, same shape as x).
    mask_from: the kernel's own forward output -- the activation derivative of the backward is then taken from ITS sign (the
    backward's contract is 'given y'), so a pre-activation one rounding away from zero does not turn into an error of |dy|.
    -> dict(y, dx, dp0, dp1) in NHWC (dp0 / dp1: affine [C], SPADE NHWC)."""
    def prep(t, grad=False):
        if t is None:
            return None
        t = t.detach().cpu().to(dtype)
        if t.dim() == 4:
            t = t.permute(0, 3, 1, 2).contiguous()
        return t.requires_grad_(True) if grad else t
    back = dy is not None
    xr, q0, q1 = prep(x, back), prep(p0, back), prep(p1, back)
    if mode == 1:
        h = F.instance_norm(xr, weight=q0, bias=q1, eps=eps)
    else:
        h = F.instance_norm(xr, eps=eps)
        if mode == 2:
            h = h * (1 + q0) + q1
    if mask_from is not None and act != ACT_NONE:
        m = prep(mask_from)
        y = h * torch.where(m > 0, torch.ones_like(m), torch.full_like(m, slope if act == ACT_LRELU else 0.0))
    else:
        y = _act(h, act, slope)
    if residual is not None:
        y = y + prep(residual)
    out = dict(y=y.detach().permute(0, 2, 3, 1).contiguous())
    if back:
        y.backward(prep(dy))
        dx = xr.grad
        if addend is not None:
            dx = dx + prep(addend)
        out['dx'] = dx.permute(0, 2, 3, 1).contiguous()
        if mode == 1:
            out['dp0'], out['dp1'] = q0.grad, q1.grad
        elif mode == 2:
            out['dp0'], out['dp1'] = q0.grad.permute(0, 2, 3, 1).contiguous(), q1.grad.permute(0, 2, 3, 1).contiguous()
    return out


# ------------------------------------------------------------------------------------------------ fp32 emulations of the formulas
def _finish(x, mean, var, eps):
    rstd = 1.0 / torch.sqrt(var.clamp_min(0.0) + eps)
    return (x - mean[:, None, None, :]) * rstd[:, None, None, :], mean, rstd


def emu_two_pass(x, eps=EPS):
    """mean, then the centred values: their squares give the variance and their sum corrects what the first pass's rounding left in the
    mean (the tile kernel; the recomputation of the from-sums path)."""
    x = x.float()
    B, C = x.shape[0], x.shape[-1]
    v = x.reshape(B, -1, C)
    mean = v.sum(dim=1) / v.shape[1]
    d = v - mean[:, None]
    t1, t2 = d.sum(dim=1) / v.shape[1], (d * d).sum(dim=1) / v.shape[1]
    return _finish(x, mean + t1, t2 - t1 * t1, eps)


def pivot_pixels(HW):
    """The twelve pixels of hoig_amd/csrc/norm.hip:inorm_pivot -- three groups of four at the odd 24ths of the map."""
    return [[((2 * (4 * g + j) + 1) * HW) // 24 for j in range(4)] for g in range(3)]


def emu_pivot(x, pivot='median12', eps=EPS):
    """sums of (x - pivot), (x - pivot)^2 and var = E[d^2] - E[d]^2 (the streaming kernels).  pivot 'pixel0': the image's first pixel
    (what the kernel used before); 'median12': the median of three means of four spread pixels (what it uses now)."""
    x = x.float()
    B, C = x.shape[0], x.shape[-1]
    v = x.reshape(B, -1, C)
    if pivot == 'pixel0':
        p = v[:, 0]
    else:
        p = torch.stack([v[:, g].sum(dim=1) * 0.25 for g in pivot_pixels(v.shape[1])], 0).median(dim=0).values
    d = v - p[:, None]
    s1, s2 = d.sum(dim=1) / v.shape[1], (d * d).sum(dim=1) / v.shape[1]
    return _finish(x, p + s1, s2 - s1 * s1, eps)


def emu_plain(x, eps=EPS):
    """var = E[x^2] - E[x]^2 from plain sums (what hoig_inorm_stats_from_sums did with a convolution epilogue's sums)."""
    x = x.float()
    B, C = x.shape[0], x.shape[-1]
    v = x.reshape(B, -1, C)
    s1, s2 = v.sum(dim=1) / v.shape[1], (v * v).sum(dim=1) / v.shape[1]
    return _finish(x, s1, s2 - s1 * s1, eps)


def emu_sums_repaired(x, cond=8.0, eps=EPS):
    """plain sums where E[x^2] <= cond * var, otherwise centred on the plain sums' mean (hoig_inorm_stats_from_sums now)."""
    x = x.float()
    B, C = x.shape[0], x.shape[-1]
    v = x.reshape(B, -1, C)
    s1, s2 = v.sum(dim=1) / v.shape[1], (v * v).sum(dim=1) / v.shape[1]
    var = s2 - s1 * s1
    d = v - s1[:, None]
    t1, t2 = d.sum(dim=1) / v.shape[1], (d * d).sum(dim=1) / v.shape[1]
    redo = ~(s2 <= cond * var)
    return _finish(x, torch.where(redo, s1 + t1, s1), torch.where(redo, t2 - t1 * t1, var), eps)


# ---------------------------------------------------------------------------------------------------------------- input makers
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ratio_input(B, H, W, ratios=RATIOS, seed=0, sigma=1.0):
    """[B, H, W, C] fp32, C = len(ratios) rounded up to a multiple of 4 (cycling): channel c ~ sigma * (N(0, 1) + ratios[c])."""
    C = (len(ratios) + 3) // 4 * 4
    r = torch.tensor([ratios[c % len(ratios)] for c in range(C)], dtype=torch.float64)
    x = torch.randn(B, H, W, C, generator=_gen(seed), dtype=torch.float64)
    return ((x + r) * sigma).float(), r


def moved_pixels(x, k, block=1):
    """the corner block x block pixels of every (image, channel) moved by +k sigma of that channel (block 1: pixel 0, the pivot of the
    earlier streaming kernel and the zero-padded corner of a convolution's output)."""
    s = stats64(x)['sigma'].float()
    x = x.clone()
    x[:, :block, :block, :] += k * s[:, None, None, :]
    return x


def spike_input(B, H, W, C, seed=0, where=None):
    """every channel constant (a different level per channel, some negative, one zero) except for ONE pixel moved by 1."""
    g = _gen(seed)
    level = torch.linspace(-3.0, 5.0, C)
    level[C // 2] = 0.0
    x = level.expand(B, H, W, C).clone()
    for b in range(B):
        for c in range(C):
            i = int(torch.randint(0, H * W, (1,), generator=g)) if where is None else where
            x[b, i // W, i % W, c] += 1.0
    return x


def magnitude_input(B, H, W, C, seed=0):
    """N(0.5, 1) channels at magnitudes 1, 1e4 and 1e-4 side by side (1e-4: the variance is far below eps, the norm barely scales)."""
    x = torch.randn(B, H, W, C, generator=_gen(seed)) + 0.5
    scale = torch.ones(C)
    scale[1::3] = 1e4
    scale[2::3] = 1e-4
    return x * scale


def conditioning_inputs(H, W, B=1, seed=0):
    """name -> NHWC fp32 input: the conditioning cases of one map size.  One tensor per |mean|/sigma (eight channels, both signs), so
    that e_ref -- the worst channel of torch's fp32 kernel on that tensor -- belongs to that ratio and to no other."""
    out = {}
    for i, r in enumerate((0.0, 3.0, 10.0, 30.0, 100.0, 1000.0)):
        out['ratio%g' % r] = ratio_input(B, H, W, (r, -r) * 4, seed + i)[0]
    base0, base10 = ratio_input(B, H, W, (0.0,) * 8, seed + 11)[0], ratio_input(B, H, W, (10.0, -10.0) * 4, seed + 12)[0]
    for k in (10.0, 100.0, 1000.0):
        out['pixel0+%g' % k] = moved_pixels(base0, k, 1)
        out['corner3x3+%g' % k] = moved_pixels(base0, k, 3)
    out['ratio10,pixel0+1000'] = moved_pixels(base10, 1000.0, 1)
    out['ratio10,corner3x3-1000'] = moved_pixels(base10, -1000.0, 3)
    out['spike'] = spike_input(B, H, W, 8, seed + 2)
    out['spike@0'] = spike_input(B, H, W, 8, seed + 2, where=0)
    out['magnitudes'] = magnitude_input(B, H, W, 16, seed + 3)
    return out


# ------------------------------------------------------------------- convolutions whose OUTPUT has a wanted |mean| / sigma per channel
CONV_KINDS = {            # kind -> (kernel size, stride, transposed)
    's1': (3, 1, False), 's2': (3, 2, False), 'convT': (3, 2, True), 'stem7': (7, 1, False), 'f6': (3, 1, False)}


def conv_problem(kind, B, Ci, Co, Ho, Wo, ratio, seed=0, sigma_x=1.0, moved=0.0, row_scale=None, delta=None):
    """-> (x NCHW fp32, w fp32: [Co, Ci, k, k], or [Ci, Co, k, k] for 'convT') of a bias-free convolution (padding k // 2; stride 2:
    Conv2d halves, ConvTranspose2d with output_padding 1 doubles the map) whose output channel co is  level_co + noise  with
    level_co / sigma_co = +-ratio (sign alternating with co), exactly constant under the noise also along the zero-padded border:
    the input is a constant plane c plus N(0, sigma_x), and of each (output channel, tap) the weights sum to ZERO over the input
    channels, except for the taps of which every output pixel sees exactly one (the centre; ConvTranspose2d: the four taps {1,2}^2),
    whose weights carry an offset d_co.  moved: K added to input channel 0 at pixel (0, 0), which moves the corner block of every
    output channel by K * w[co, tap, 0].  row_scale: factor per output channel (magnitudes).  delta: d_co given, not solved (sigma_x 0)."""
    k, stride, transposed = CONV_KINDS[kind]
    g = _gen(seed)
    w = torch.randn(Co, Ci, k, k, generator=g, dtype=torch.float64) * 0.05
    w -= w.mean(dim=1, keepdim=True)
    live = [(1, 1), (1, 2), (2, 1), (2, 2)] if transposed else [(k // 2, k // 2)]
    f = 0.5 if transposed else 1.0                               # a ConvTranspose2d output pixel sees 9/4 taps on average
    c = max(8.0, 2.0 * ratio * sigma_x * (len(live) / Ci) ** 0.5)
    w0 = (w * w).sum(dim=(1, 2, 3))
    if delta is None:
        d = torch.sqrt(ratio ** 2 * f ** 2 * sigma_x ** 2 * w0 / (c ** 2 * Ci ** 2 - ratio ** 2 * f ** 2 * sigma_x ** 2 * len(live) * Ci))
    else:
        d = torch.full((Co,), float(delta), dtype=torch.float64)
    d = d * torch.tensor([1.0, -1.0], dtype=torch.float64).repeat(Co // 2 + 1)[:Co]
    for (r, s) in live:
        w[:, :, r, s] += d[:, None]
    if row_scale is not None:
        w *= row_scale.double()[:, None, None, None]
    Hi, Wi = (Ho * 2, Wo * 2) if (stride == 2 and not transposed) else (Ho // 2, Wo // 2) if transposed else (Ho, Wo)
    x = c + sigma_x * torch.randn(B, Ci, Hi, Wi, generator=g, dtype=torch.float64)
    x[:, 0, 0, 0] += moved
    if transposed:
        w = w.permute(1, 0, 2, 3).contiguous()
    return x.float(), w.float()


def conv_reference(kind, x, w, dtype=torch.float64):
    k, stride, transposed = CONV_KINDS[kind]
    x, w = x.to(dtype), w.to(dtype)
    if transposed:
        return F.conv_transpose2d(x, w, None, stride=2, padding=1, output_padding=1)
    return F.conv2d(x, w, None, stride=stride, padding=k // 2)


def achieved_ratio(h_nhwc):
    s = stats64(h_nhwc)
    return s['mean'].abs() / s['sigma'].clamp_min(1e-300)
