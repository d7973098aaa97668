"""The kernels of hoig_amd/csrc/metrics.hip on their own, at tile, channel and grid edges, against float64 on the CPU
(tests/metrics_reference.py).  docs/metrics_kernels_parity.md lists the cases, the bounds and the measured errors; every test prints
its figures before it asserts."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gpu_util
import metrics_reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GRID_CAP = 2048 * 256          # hoig_stream_grid: at most 2048 workgroups of 256 threads, then the grid-stride loop


@pytest.fixture(autouse=True)
def _poisoned_free_memory():
    gpu_util.poison_free_memory()          # an output element no kernel wrote reads as NaN


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().float().to(DEV)


def _nchw(y):
    return y.permute(0, 3, 1, 2).contiguous().cpu()


def _dev_zeros(nbytes):
    return torch.zeros(nbytes, dtype=torch.uint8, device=DEV)


# ============================================================================================================== SSIM, MS-SSIM
# (B, C, H, W, win), scale = data_range
SSIM_CASES = [
    ((2, 3, 11, 11, 11), 1.0),       # one output pixel
    ((2, 1, 90, 11, 11), 1.0),       # Wo = 1
    ((2, 1, 11, 90, 11), 1.0),       # Ho = 1
    ((2, 4, 26, 74, 11), 1.0),       # the valid map is exactly one 64 x 16 tile
    ((2, 3, 27, 75, 11), 1.0),       # four tiles, three of them one pixel wide or high
    ((1, 5, 17, 130, 5), 1.0),       # two full tiles in a row, C = 5
    ((3, 3, 40, 23, 3), 1.0),        # H > W, small window
    ((2, 2, 31, 79, 15), 1.0),       # the largest window, Ho = 17, Wo = 65
    ((2, 3, 20, 33, 1), 1.0),        # a one-tap window: cs is 1, only luminance is left
    ((2, 3, 40, 70, 11), 255.0),     # 0..255 inputs
    ((2, 3, 26, 74, 7), 255.0),      # 0..255 inputs, window of 7
]
SSIM_IDS = ['%dx%dx%dx%d-win%d-range%g' % (c + (s,)) for c, s in SSIM_CASES]
SSIM_TOL = 1e-5                      # absolute, on per-channel means of maps of at least 16 pixels
KK = (0.01, 0.03)


@functools.lru_cache(maxsize=None)
def ssim_case(case, scale):
    """X, Y, the fp64 (ssim, cs), and the distance of the same statement in fp32 on the CPU from it (the floor of the format)."""
    B, C, H, W, win = case
    X, Y = R.ssim_pair(B, C, H, W, scale, seed=H * W + C + win)
    want = R.ssim_level(X, Y, scale, win)
    f32 = R.ssim_level(X, Y, scale, win, dtype=torch.float32)
    floor = max((a.double() - b).abs().max().item() for a, b in zip(f32, want))
    return X, Y, want, floor


def _xy(X, Y):
    return _nhwc(torch.cat([X, Y]))


def _level(xy, dr, win):
    from hoig_amd.metrics import ssim as S
    return S._level(xy, dr, win, 1.5, KK)


@pytest.mark.parametrize('case,scale', SSIM_CASES, ids=SSIM_IDS)
def test_ssim_level_vs_fp64(case, scale):
    from hoig_amd.metrics import ssim as S
    B, C, H, W, win = case
    X, Y, (want_s, want_cs), floor = ssim_case(case, scale)
    npix = (H - win + 1) * (W - win + 1)
    # fewer than 16 pixels: no averaging of the cancellation in s11 = E[x^2] - E[x]^2 against C2; the bound is then four times the
    # error the fp32 statement itself makes on these very inputs
    tol = SSIM_TOL if npix >= 16 else 4 * floor
    assert want_s.max() - want_s.min() > 0.1 or B == 1, want_s               # far and close pairs, not one value
    assert want_s.min() > 0 and (win == 1 or want_s.min() < 0.1), want_s      # (B = 1 is the far pair alone)
    xy = _xy(X, Y)
    s, cs = _level(xy, scale, win)
    err_s = (s.double().cpu() - want_s).abs().max().item()
    err_cs = (cs.double().cpu() - want_cs).abs().max().item()
    print('ssim %s: ssim %.3f..%.3f  fp32-cpu %.2e  device ssim %.2e cs %.2e  bound %.2e'
          % (SSIM_IDS[SSIM_CASES.index((case, scale))], want_s.min(), want_s.max(), floor, err_s, err_cs, tol))
    assert s.shape == cs.shape == (B, C)
    assert err_s < tol and err_cs < tol
    if win == 1:
        assert (want_cs - 1).abs().max().item() < 1e-12
    assert torch.equal(S.ssim_nhwc(xy, scale, win_size=win), s)
    # the NCHW entries: mean over channels per image, or over everything
    per = S.ssim(X.to(DEV), Y.to(DEV), data_range=scale, size_average=False, win_size=win)
    assert per.shape == (B,) and (per.double().cpu() - want_s.mean(1)).abs().max().item() < tol
    allm = S.ssim(X.to(DEV), Y.to(DEV), data_range=scale, win_size=win)
    assert allm.dim() == 0 and abs(allm.item() - want_s.mean().item()) < tol


@pytest.mark.parametrize('case,scale', SSIM_CASES, ids=SSIM_IDS)
def test_ssim_of_equal_maps_is_exactly_one(case, scale):
    B, C, H, W, win = case
    X = ssim_case(case, scale)[0]
    one = torch.ones(B, C, device=DEV)
    for name, img in (('map', X), ('constant', torch.full_like(X, 0.7 * scale))):
        s, cs = _level(_xy(img, img), scale, win)
        print('ssim(x, x) %s %s: 1 - ssim %.3e, 1 - cs %.3e' % (SSIM_IDS[SSIM_CASES.index((case, scale))], name,
                                                               (1 - s.double()).abs().max().item(),
                                                               (1 - cs.double()).abs().max().item()))
        assert torch.equal(cs, one), name
        assert torch.equal(s, one), name


def test_ssim_negative_structure():
    from hoig_amd.metrics import ssim as S
    g = torch.Generator().manual_seed(12)
    X = torch.rand(2, 3, 161, 163, generator=g)
    Y = 1 - X
    want_s, want_cs = R.ssim_level(X, Y, 1.0)
    assert want_s.max() < -0.5 and want_cs.max() < -0.5, (want_s, want_cs)
    xy = _xy(X, Y)
    raw = S.ssim_nhwc(xy, 1.0)
    assert (raw.double().cpu() - want_s).abs().max().item() < SSIM_TOL
    assert (_level(xy, 1.0, 11)[1].double().cpu() - want_cs).abs().max().item() < SSIM_TOL
    assert torch.equal(S.ssim_nhwc(xy, 1.0, nonnegative_ssim=True), torch.zeros(2, 3, device=DEV))
    assert torch.equal(S.ssim(X.to(DEV), Y.to(DEV), data_range=1.0, size_average=False, nonnegative_ssim=True),
                       torch.zeros(2, device=DEV))
    assert R.ms_ssim_per_channel(X, Y, 1.0).abs().max().item() == 0
    assert torch.equal(S.ms_ssim_nhwc(xy, 1.0), torch.zeros(2, 3, device=DEV))
    assert torch.equal(S.ms_ssim(X.to(DEV), Y.to(DEV), data_range=1.0, size_average=False), torch.zeros(2, device=DEV))


def test_ssim_workspace_is_reusable():
    from hoig_amd import _lib as L
    from hoig_amd import ops as O
    B, C, H, W, win = 2, 3, 27, 75, 11
    pairs = [_xy(*R.ssim_pair(B, C, H, W, 1.0, seed)) for seed in (1, 2)]
    nbytes = L.lib.hoig_ssim_workspace_bytes(B, H, W, C, win)
    assert nbytes >= 256 + B * C * 4 * 2 * 4                            # four tiles

    def launch(xy, work):
        s, cs = torch.empty(B, C, device=DEV), torch.empty(B, C, device=DEV)
        L.call('hoig_ssim', O._p(xy), O._p(xy[B:]), O._p(s), O._p(cs), B, H, W, C, 1.0, KK[0], KK[1], win, 1.5, O._p(work), O._st())
        return s, cs

    work = _dev_zeros(nbytes)
    first = launch(pairs[0], work)
    second = launch(pairs[1], work)
    fresh = launch(pairs[1], _dev_zeros(nbytes))
    assert torch.equal(second[0], fresh[0]) and torch.equal(second[1], fresh[1])
    assert not torch.equal(first[0], second[0])
    assert work[:4 * B].count_nonzero().item() == 0                      # the arrival counters are back at 0
    assert (second[0].double().cpu() - R.ssim_level(*R.ssim_pair(B, C, H, W, 1.0, 2), 1.0)[0]).abs().max().item() < SSIM_TOL


MS_CASES = [(2, 3, 161, 163), (1, 3, 162, 200), (2, 2, 177, 161)]     # 161: the smallest legal side, its last level 11 x 11


@pytest.mark.parametrize('shape', MS_CASES, ids=['%dx%dx%dx%d' % s for s in MS_CASES])
def test_ms_ssim_at_the_smallest_sides(shape):
    from hoig_amd.metrics import ssim as S
    B, C, H, W = shape
    X, Y = R.ssim_pair(B, C, H, W, 1.0, seed=H + W)
    want = R.ms_ssim_per_channel(X, Y, 1.0)
    assert 0.05 < want.min() < 0.5 and want.max() < 0.99, want           # a wrong level moves the product
    got = S.ms_ssim_nhwc(_xy(X, Y), 1.0)
    err = (got.double().cpu() - want).abs().max().item()
    print('ms-ssim %s: reference %.3f..%.3f  device error %.2e  bound %.0e' % (shape, want.min(), want.max(), err, SSIM_TOL))
    assert got.shape == (B, C) and err < SSIM_TOL
    per = S.ms_ssim(X.to(DEV), Y.to(DEV), data_range=1.0, size_average=False)
    assert per.shape == (B,) and (per.double().cpu() - want.mean(1)).abs().max().item() < SSIM_TOL
    assert abs(S.ms_ssim(X.to(DEV), Y.to(DEV), data_range=1.0).item() - want.mean().item()) < SSIM_TOL


def test_ssim_refusals():
    from hoig_amd import _lib as L
    from hoig_amd.metrics import ssim as S
    x = torch.ones(1, 3, 160, 170, device=DEV)
    with pytest.raises(AssertionError, match='larger than 160'):
        S.ms_ssim(x, x, data_range=1.0)
    x = torch.ones(1, 3, 10, 40, device=DEV)
    with pytest.raises(ValueError, match='smaller than the 11-tap window'):
        S.ssim(x, x, data_range=1.0)
    xy = torch.ones(2, 20, 20, 3, device=DEV)
    with pytest.raises(L.HoigKernelError, match='unsupported'):
        S._level(xy, 1.0, 17, 1.5, KK)


# ============================================================================================================== LPIPS layer
LPIPS_CASES = [
    (2, 1, 4),         # one pixel, one channel quad
    (3, 15, 4),        # fewer pixels than lane groups
    (2, 16, 60),       # C4 = 15: one idle lane
    (2, 17, 64),       # C = 64 at a small HW
    (2, 255, 68),      # one pixel short of a tile
    (2, 256, 512),     # exactly one tile, the channel limit
    (3, 257, 508),     # one pixel into a second tile, a ragged last quad row
    (1, 513, 192),     # three tiles
]
LPIPS_TOL = 1e-5       # relative, per image


def lpips_maps(B, HW, C, seed):
    g = torch.Generator().manual_seed(seed)
    fx, fy = torch.relu(torch.randn(B, HW, C, generator=g)), torch.relu(torch.randn(B, HW, C, generator=g))
    w = torch.rand(C, generator=g) / C * 8                              # (the size of lpips_state_dict's heads)
    return fx, fy, w


def lpips_launch(fx, fy, w, out=None, work=None):
    """hoig_lpips_layer as LPIPS.distance calls it; fx, fy, w: device tensors.  out += the distance."""
    from hoig_amd import _lib as L
    from hoig_amd import ops as O
    B, HW, C = fx.shape
    out = torch.zeros(B, device=DEV) if out is None else out
    work = _dev_zeros(L.lib.hoig_lpips_workspace_bytes(B, HW)) if work is None else work
    L.call('hoig_lpips_layer', O._p(fx), O._p(fy), O._p(w), O._p(out), B, HW, C, O._p(work), O._st())
    return out


def _lpips_errors(fx, fy, w):
    """(relative device error, relative fp32-CPU error, fp64 values), the errors as the worst image's."""
    want = R.lpips_layer(fx, fy, w)
    got = lpips_launch(fx.to(DEV), fy.to(DEV), w.to(DEV))
    assert got.shape == want.shape
    f32 = R.lpips_layer(fx, fy, w, dtype=torch.float32)
    rel = lambda v: ((v.double().cpu() - want).abs() / want.abs()).max().item()
    return rel(got), rel(f32), want


@pytest.mark.parametrize('B,HW,C', LPIPS_CASES)
def test_lpips_layer_vs_fp64(B, HW, C):
    fx, fy, w = lpips_maps(B, HW, C, HW + C)
    err, floor, want = _lpips_errors(fx, fy, w)
    print('lpips (%d, %d, %d): value %.4f  fp32-cpu %.2e  device %.2e  bound %.0e' % (B, HW, C, want.mean(), floor, err, LPIPS_TOL))
    assert want.min() > 1e-3
    assert err < LPIPS_TOL


def _edge_maps(kind):
    fx, fy, w = lpips_maps(2, 300, 64, 300)
    g = torch.Generator().manual_seed(77)
    if kind == 'tiny':           # squared norms from 1e-13 to 1e-5, on both sides of the 1e-10 under the root
        fx = fx * 10 ** (torch.rand(2, 300, 1, generator=g) * 4 - 7)
        fy = fy * 10 ** (torch.rand(2, 300, 1, generator=g) * 4 - 7)
    elif kind == 'sparse':       # all-zero pixels in x only, in y only, in both, in neither
        fx = fx * (torch.rand(2, 300, 1, generator=g) < 0.5)
        fy = fy * (torch.rand(2, 300, 1, generator=g) < 0.5)
    elif kind == 'close':
        fy = fx * (1 + 1e-3 * torch.randn(2, 300, 64, generator=g))
    return fx, fy, w


# close maps: each normalised term carries a few ulp (2^-24 each from the norm, rsqrtf and the product), the difference of two terms
# 1e-3 apart amplifies that by 1e3, the square doubles it: a few 1e-4 relative
@pytest.mark.parametrize('kind,tol', [('tiny', LPIPS_TOL), ('sparse', LPIPS_TOL), ('close', 1e-3)])
def test_lpips_layer_edges(kind, tol):
    fx, fy, w = _edge_maps(kind)
    if kind == 'tiny':
        n2 = (fx.double() ** 2).sum(-1)
        assert (n2 < 1e-11).sum() > 50 and (n2 > 1e-9).sum() > 50
    if kind == 'sparse':
        zx, zy = (fx.abs().sum(-1) == 0), (fy.abs().sum(-1) == 0)
        assert min((zx & zy).sum(), (zx & ~zy).sum(), (~zx & zy).sum(), (~zx & ~zy).sum()) > 20
    err, floor, want = _lpips_errors(fx, fy, w)
    print('lpips %s (2, 300, 64): value %.3e  fp32-cpu %.2e  device %.2e  bound %.0e' % (kind, want.mean(), floor, err, tol))
    assert torch.isfinite(want).all() and want.min() > 0
    if kind == 'close':
        assert want.max() < 1e-6
    assert err < tol


def test_lpips_layer_exact_properties():
    fx, fy, w = [t.to(DEV) for t in lpips_maps(2, 300, 64, 300)]
    a = lpips_launch(fx, fy, w)
    assert a.min().item() > 1e-3
    assert torch.equal(lpips_launch(fx, fx, w), torch.zeros(2, device=DEV))
    assert torch.equal(lpips_launch(fx, fx.clone(), w), torch.zeros(2, device=DEV))
    assert torch.equal(lpips_launch(fy, fx, w), a)                      # swapped
    assert torch.equal(lpips_launch(fx, fy, w), a)                      # repeated
    for kind in ('tiny', 'sparse'):
        ex = _edge_maps(kind)[0].to(DEV)
        assert torch.equal(lpips_launch(ex, ex, w), torch.zeros(2, device=DEV)), kind


def test_lpips_layer_accumulates_and_reuses_its_workspace():
    from hoig_amd import _lib as L
    fx, fy, w = lpips_maps(2, 255, 68, 5)
    want = R.lpips_layer(fx, fy, w)
    out = torch.tensor([3.0, -1.5], device=DEV)
    lpips_launch(fx.to(DEV), fy.to(DEV), w.to(DEV), out=out)
    assert (out.double().cpu() - (torch.tensor([3.0, -1.5], dtype=torch.float64) + want)).abs().max().item() < 1e-6
    big = [t.to(DEV) for t in lpips_maps(2, 513, 64, 6)]
    small = [t.to(DEV) for t in lpips_maps(2, 17, 64, 7)]
    nbytes = L.lib.hoig_lpips_workspace_bytes(2, 513)
    assert nbytes >= L.lib.hoig_lpips_workspace_bytes(2, 17)
    work = _dev_zeros(nbytes)
    got_big = lpips_launch(*big, work=work)
    got_small = lpips_launch(*small, work=work)
    assert torch.equal(got_big, lpips_launch(*big)) and torch.equal(got_small, lpips_launch(*small))
    assert got_big.min().item() > 1e-3 and got_small.min().item() > 1e-3
    assert work[:8].count_nonzero().item() == 0


@pytest.mark.parametrize('C,w_offset', [(6, 0), (516, 0), (64, 4)])
def test_lpips_layer_refusals_write_nothing(C, w_offset):
    from hoig_amd import _lib as L
    from hoig_amd import ops as O
    B, HW = 2, 20
    fx, fy = torch.ones(B, HW, C, device=DEV), torch.ones(B, HW, C, device=DEV)
    wbuf = torch.ones(C + 4, device=DEV)
    out = torch.tensor([3.0, -1.5], device=DEV)
    work = _dev_zeros(L.lib.hoig_lpips_workspace_bytes(B, HW))
    assert wbuf.data_ptr() % 16 == 0
    with pytest.raises(L.HoigKernelError, match='unsupported'):
        L.call('hoig_lpips_layer', O._p(fx), O._p(fy), wbuf.data_ptr() + w_offset, O._p(out), B, HW, C, O._p(work), O._st())
    torch.cuda.synchronize()
    assert out.tolist() == [3.0, -1.5] and work.count_nonzero().item() == 0


# ============================================================================================================== pooling
@functools.lru_cache(maxsize=None)
def _big_pool_input():
    x = torch.randn(2, 64, 259, 259, generator=torch.Generator().manual_seed(259))
    return x, _nhwc(x)


def test_pool2d_max_second_pass_of_the_capped_grid():
    from hoig_amd.metrics import kernels as K
    x, xd = _big_pool_input()
    got = K.pool2d(xd, 3, 2)
    assert got.numel() // 4 == 532512 > GRID_CAP                        # float4 work items
    assert torch.equal(_nchw(got), F.max_pool2d(x, 3, 2))


def test_pool2d_avg_second_pass_of_the_capped_grid():
    from hoig_amd import _lib as L
    from hoig_amd.metrics import kernels as K
    x, xd = _big_pool_input()
    got = K.pool2d(xd, 2, 2, 1, 1, L.POOL_AVG, True)
    assert got.numel() // 4 == 540800 > GRID_CAP
    err = (_nchw(got).double() - F.avg_pool2d(x.double(), 2, padding=(1, 1))).abs().max().item()
    print('avg pool 2x2 pad 1 on (2, 259, 259, 64): %.2e' % err)
    assert err < 1e-6


@pytest.mark.parametrize('mode', ['max', 'avg', 'avg_valid'])
def test_pool2d_scalar_path_of_an_unaligned_pointer(mode):
    from hoig_amd import _lib as L
    from hoig_amd import ops as O
    from hoig_amd.metrics import kernels as K
    B, H, W, C = 2, 9, 11, 8
    x = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(3)).to(DEV)
    buf = torch.zeros(x.numel() + 4, device=DEV)
    buf[1:1 + x.numel()] = x.flatten()
    args = dict(max=(3, 2, 0, 0, L.POOL_MAX, 1), avg=(2, 2, 1, 1, L.POOL_AVG, 1), avg_valid=(3, 1, 1, 1, L.POOL_AVG, 0))[mode]
    k, s, ph, pw = args[:4]
    want = K.pool2d(x, k, s, ph, pw, args[4], bool(args[5]))           # float4 path (checked against torch elsewhere)
    got = torch.empty_like(want)
    assert x.data_ptr() % 16 == 0 and (buf.data_ptr() + 4) % 16 == 4 and C % 4 == 0
    L.call('hoig_pool2d_fwd', buf.data_ptr() + 4, O._p(got), B, H, W, C, *args, O._st())
    assert torch.isfinite(got).all() and torch.equal(got, want)
    xc = x.permute(0, 3, 1, 2).cpu()
    ref = dict(max=lambda: F.max_pool2d(xc, 3, 2), avg=lambda: F.avg_pool2d(xc.double(), 2, padding=1),
               avg_valid=lambda: F.avg_pool2d(xc.double(), 3, 1, 1, count_include_pad=False))[mode]()
    assert (_nchw(got).double() - ref.double()).abs().max().item() < 1e-6


def test_pool2d_small_shapes():
    from hoig_amd import _lib as L
    from hoig_amd.metrics import kernels as K
    g = torch.Generator().manual_seed(8)
    # the window is the image
    x = torch.randn(2, 5, 3, 3, generator=g)
    got = K.pool2d(_nhwc(x), 3, 1)
    assert got.shape == (2, 1, 1, 5) and torch.equal(_nchw(got), F.max_pool2d(x, 3, 1))
    got = K.pool2d(_nhwc(x), 3, 3, 0, 0, L.POOL_AVG, True)
    assert (_nchw(got).double() - F.avg_pool2d(x.double(), 3)).abs().max().item() < 1e-6
    # an image smaller than the window, padded
    x = torch.randn(2, 4, 2, 7, generator=g)
    got = K.pool2d(_nhwc(x), 3, 1, 1, 1)
    assert got.shape == (2, 2, 7, 4) and torch.equal(_nchw(got), F.max_pool2d(x, 3, 1, 1))
    got = K.pool2d(_nhwc(x), 3, 2, 1, 1)
    assert got.shape == (2, 1, 4, 4) and torch.equal(_nchw(got), F.max_pool2d(x, 3, 2, 1))
    # the in-image divisor at a 2 x 2 image: every 3 x 3 window holds the whole image, every 2 x 2 window one, two or four pixels
    x = torch.randn(1, 3, 2, 2, generator=g)
    for k in (3, 2):
        got = K.pool2d(_nhwc(x), k, 1, 1, 1, L.POOL_AVG, False)
        want = F.avg_pool2d(x.double(), k, 1, 1, count_include_pad=False)
        assert got.shape[1:3] == want.shape[2:] and (_nchw(got).double() - want).abs().max().item() < 1e-6
        got = K.pool2d(_nhwc(x), k, 1, 1, 1, L.POOL_AVG, True)
        assert (_nchw(got).double() - F.avg_pool2d(x.double(), k, 1, 1)).abs().max().item() < 1e-6


@pytest.mark.parametrize('C', [8, 3])
def test_pool2d_max_propagates_nan(C):
    from hoig_amd.metrics import kernels as K
    x = torch.randn(1, C, 9, 10, generator=torch.Generator().manual_seed(C))
    x[0, 1, 4, 5] = float('nan')
    x[0, C - 1, 0, 0] = float('nan')
    x[0, 0, 3, 3] = float('-inf')
    for k, s, p in ((3, 2, 0), (3, 1, 1)):
        want = F.max_pool2d(x, k, s, p)
        got = _nchw(K.pool2d(_nhwc(x), k, s, p, p))
        assert 0 < want.isnan().sum() < want[0, 1].numel()
        assert torch.equal(got.isnan(), want.isnan())
        assert torch.equal(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(want, nan=7.0))


# ============================================================================================================== staging
def _stage_reference(u8, size, steps):
    """fp32 torch on the CPU, as tests/test_metrics_gpu.py::test_stage_images_u8: ToTensor, F.interpolate, the affine steps."""
    t = torch.from_numpy(u8).permute(0, 3, 1, 2).float().div(255)
    if size is not None and tuple(size) != tuple(t.shape[2:]):
        t = F.interpolate(t, size=size, mode='bilinear', align_corners=False)
    for sub, div in steps:
        t = (t - torch.tensor(sub).view(1, -1, 1, 1)) / torch.tensor(div).view(1, -1, 1, 1)
    return t


def _stage_err(u8, size, steps):
    from hoig_amd.metrics import kernels as K
    got = K.stage_images_u8(torch.from_numpy(u8).to(DEV), size, steps)
    want = _stage_reference(u8, size, steps)
    assert tuple(got.shape) == (want.shape[0], want.shape[2], want.shape[3], want.shape[1])
    return (_nchw(got) - want).abs().max().item()


def test_stage_images_u8_second_pass_of_the_capped_grid():
    u8 = np.random.RandomState(1).randint(0, 256, size=(3, 100, 90, 3)).astype(np.uint8)
    assert 3 * 420 * 420 == 529200 > GRID_CAP                            # one work item per output pixel
    err = _stage_err(u8, (420, 420), [((0.5,) * 3, (0.5,) * 3)])
    print('stage (3, 100, 90, 3) -> 420 x 420: %.2e' % err)
    assert err < 1e-6


STEPS4 = [((0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)), ((-0.03, -0.088, -0.188, 0.1), (0.458, 0.448, 0.450, 0.5))]


@pytest.mark.parametrize('C', [1, 4])
@pytest.mark.parametrize('size', [None, (45, 31), (11, 29)], ids=['same', 'up', 'down'])
def test_stage_images_u8_channel_counts(C, size):
    u8 = np.random.RandomState(C).randint(0, 256, size=(2, 37, 53, C)).astype(np.uint8)      # (37, 53) -> (11, 29): no integer factor
    steps = {1: [((0.5,), (0.5,))], 4: STEPS4}[C]
    for st in ([], steps[:1], steps):
        # 1e-6 on the interpolated value in [0, 1] (the existing bound); a step divides by `div`, so whatever rounding the two
        # interpolations differ by grows by 1 / min(div) per step.  Without a resize both sides do the same three operations.
        tol = 1e-6 * (float(np.prod([1 / min(div) for _, div in st])) if size is not None else 1.0)
        err = _stage_err(u8, size, st)
        print('stage C=%d (37, 53) -> %s, %d steps: %.2e  bound %.1e' % (C, size, len(st), err, tol))
        assert err < tol


def test_stage_images_u8_one_pixel_and_refusal():
    from hoig_amd import _lib as L
    from hoig_amd.metrics import kernels as K
    u8 = np.array([[[[0, 255, 128, 7]]], [[[1, 2, 3, 4]]]], dtype=np.uint8)
    assert u8.shape == (2, 1, 1, 4)
    assert _stage_err(u8, None, []) == 0
    assert _stage_err(u8, (1, 1), STEPS4) < 1e-6                      # (the input's size: no resize)
    assert _stage_err(u8, (3, 2), []) < 1e-6                          # one source pixel, replicated
    bad = torch.zeros(1, 4, 4, 5, dtype=torch.uint8, device=DEV)
    with pytest.raises(L.HoigKernelError, match='invalid argument'):
        K.stage_images_u8(bad, None, [])


# ============================================================================================================== padding
def _pad_ref(x, ph, pw):
    return F.pad(x, (0, 0, pw, pw, ph, ph))                               # NHWC: zeros around H and W


def test_pad2d_second_pass_of_the_capped_grid():
    from hoig_amd.metrics import kernels as K
    x = torch.randn(2, 64, 64, 256, generator=torch.Generator().manual_seed(4))
    got = K.pad2d(x.to(DEV), 1, 3)
    assert got.numel() // 4 == 591360 > GRID_CAP
    assert torch.equal(got.cpu(), _pad_ref(x, 1, 3))


@pytest.mark.parametrize('shape,pad', [((1, 1, 1, 4), (2, 0)), ((3, 5, 7, 12), (0, 2)), ((2, 3, 4, 8), (0, 0))])
def test_pad2d_small(shape, pad):
    from hoig_amd.metrics import kernels as K
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(5)) + 3     # (no zero in the interior)
    got = K.pad2d(x.to(DEV), *pad)
    assert got.shape == (shape[0], shape[1] + 2 * pad[0], shape[2] + 2 * pad[1], shape[3])
    assert torch.equal(got.cpu(), _pad_ref(x, *pad))


def test_pad2d_refuses_channels_not_a_multiple_of_4():
    from hoig_amd import _lib as L
    from hoig_amd.metrics import kernels as K
    with pytest.raises(L.HoigKernelError, match='unsupported'):
        K.pad2d(torch.zeros(1, 3, 3, 6, device=DEV), 1, 1)


# ============================================================================================================== global average
@pytest.mark.parametrize('B,HW,C', [(3, 1, 7), (2, 3, 65), (2, 5, 64), (1, 64, 2048)])
def test_global_avgpool(B, HW, C):
    from hoig_amd.metrics import kernels as K
    x = torch.rand(B, HW, 1, C, generator=torch.Generator().manual_seed(HW + C)) + 0.5     # positive: a relative error per element
    xd = x.to(DEV)
    got = K.global_avgpool(xd)
    want = x.double().mean(dim=(1, 2))
    err = ((got.double().cpu() - want).abs() / want).max().item()
    print('global average (%d, %d, %d): %.2e' % (B, HW, C, err))
    assert got.shape == (B, C) and err < 1e-6
    assert torch.equal(got, K.global_avgpool(xd))
