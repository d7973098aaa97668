"""hoig_amd.metrics on the MI355X against the fp64 restatements of tests/metrics_reference.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metrics_reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().float().to(DEV)


def _nchw(y):
    return y.permute(0, 3, 1, 2).double().cpu()


def rel_err(a, b):
    return ((a.double().cpu() - b.double().cpu()).abs().max() / b.double().cpu().abs().max()).item()


@pytest.mark.parametrize('H,W', [(35, 35), (34, 36), (17, 18)])
@pytest.mark.parametrize('C', [3, 64])
def test_pooling(H, W, C):
    from hoig_amd import _lib as L
    from hoig_amd.metrics import kernels as K
    g = torch.Generator().manual_seed(H * W + C)
    x = torch.randn(2, C, H, W, generator=g)
    xd = _nhwc(x)
    assert torch.equal(_nchw(K.pool2d(xd, 3, 2)).float(), F.max_pool2d(x, 3, 2))
    assert torch.equal(_nchw(K.pool2d(xd, 3, 1, 1, 1)).float(), F.max_pool2d(x, 3, 1, 1))
    got = _nchw(K.pool2d(xd, 3, 1, 1, 1, L.POOL_AVG, False))
    assert (got - F.avg_pool2d(x.double(), 3, 1, 1, count_include_pad=False)).abs().max() < 1e-6
    pad = (H % 2, W % 2)
    got = _nchw(K.pool2d(xd, 2, 2, pad[0], pad[1], L.POOL_AVG, True))
    assert (got - F.avg_pool2d(x.double(), 2, padding=pad)).abs().max() < 1e-6


@pytest.mark.parametrize('size', [(299, 299), (256, 256), (64, 80)])
def test_stage_images_u8(size):
    from hoig_amd.metrics import kernels as K
    rng = np.random.RandomState(0)
    u8 = rng.randint(0, 256, size=(3, 256, 200, 3)).astype(np.uint8)
    t = torch.from_numpy(u8).permute(0, 3, 1, 2).float().div(255)
    want = 2 * F.interpolate(t, size=size, mode='bilinear', align_corners=False) - 1
    got = K.stage_images_u8(torch.from_numpy(u8).to(DEV), size, [((0.5,) * 3, (0.5,) * 3)])
    assert (_nchw(got).float() - want).abs().max().item() < 1e-6
    m, s = torch.tensor(K.IMAGENET_MEAN).view(1, 3, 1, 1), torch.tensor(K.IMAGENET_STD).view(1, 3, 1, 1)
    mu, sg = torch.tensor(K.LPIPS_MU).view(1, 3, 1, 1), torch.tensor(K.LPIPS_SIGMA).view(1, 3, 1, 1)
    want = (((t - m) / s) - mu) / sg
    got = K.stage_images_u8(torch.from_numpy(u8).to(DEV), None, [(K.IMAGENET_MEAN, K.IMAGENET_STD), (K.LPIPS_MU, K.LPIPS_SIGMA)])
    assert (_nchw(got).float() - want).abs().max().item() < 1e-6


@pytest.mark.parametrize('k,pad', [((1, 7), (0, 3)), ((7, 1), (3, 0)), ((1, 3), (0, 1)), ((3, 1), (1, 0))])
@pytest.mark.parametrize('prec,tol', [('f32', 1e-5), (None, 1e-4)])
def test_asymmetric_pad_conv(k, pad, prec, tol):
    from hoig_amd.metrics import kernels as K
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 160, 17, 17, generator=g, dtype=torch.float64)
    w = torch.randn(192, 160, k[0], k[1], generator=g, dtype=torch.float64) / (160 * k[0] * k[1]) ** 0.5
    b = torch.randn(192, generator=g, dtype=torch.float64) * 0.1
    conv = K.Conv(w, b, 1, pad, True, DEV, K._WeightOwner())
    got = _nchw(conv(_nhwc(x), K.precision_code(prec)))
    assert rel_err(got, F.relu(F.conv2d(x, w, b, padding=pad))) < tol


def _ssim_pairs(side, unit):
    g = torch.Generator().manual_seed(side)
    base = torch.rand(3, 3, side, side, generator=g)
    base = F.avg_pool2d(base, 5, 1, 2)                      # some structure
    other = torch.rand(3, 3, side, side, generator=g)
    mix = torch.tensor([0.2, 0.6, 0.9]).view(3, 1, 1, 1)
    y = mix * base + (1 - mix) * other                    # pairs far apart to close
    if unit:
        return base, y
    m, s = torch.tensor(R.IMAGENET_MEAN).view(1, 3, 1, 1), torch.tensor(R.IMAGENET_STD).view(1, 3, 1, 1)
    return (base - m) / s, (y - m) / s


@pytest.mark.parametrize('side', [299, 256])
@pytest.mark.parametrize('unit', [False, True])
def test_ssim_ms_ssim_per_channel(side, unit):
    from hoig_amd.metrics import ssim as S
    X, Y = _ssim_pairs(side, unit)
    dr, tol = (1.0, 1e-5) if unit else (255.0, 1e-6)
    xy = S.KR.nchw_to_nhwc(torch.cat([X, Y]).to(DEV))
    got = S.ssim_nhwc(xy, dr).double().cpu()
    want = R.ssim_level(X, Y, dr)[0]
    assert (got - want).abs().max().item() < tol
    if unit:
        assert want.min() < 0.5 and want.max() > 0.8, want           # the structure term is exercised
    got = S.ms_ssim_nhwc(xy, dr).double().cpu()
    assert (got - R.ms_ssim_per_channel(X, Y, dr)).abs().max().item() < tol
    v = S.ssim(X.to(DEV), Y.to(DEV), data_range=dr, size_average=False)
    assert torch.equal(v, S.ssim(X.to(DEV), Y.to(DEV), data_range=dr, size_average=False))


def _lpips(prec=None):
    from hoig_amd.metrics.lpips import LPIPS
    return LPIPS(R.alexnet_state_dict(1), R.lpips_state_dict(2), precision=prec, device=DEV)


def test_lpips_layers_and_values():
    from hoig_amd.metrics import kernels as K
    m, ref = _lpips(), R.LPIPSRef(R.alexnet_state_dict(1), R.lpips_state_dict(2))
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(3, 3, 299, 299, generator=g), torch.randn(3, 3, 299, 299, generator=g)
    mu, sg = torch.tensor(K.LPIPS_MU).view(1, 3, 1, 1), torch.tensor(K.LPIPS_SIGMA).view(1, 3, 1, 1)
    fm = m.features(_nhwc((x - mu) / sg))
    for a, b in zip(fm, ref.fmaps((x.double() - mu) / sg)):
        assert a.shape[1:3] == b.shape[2:]
        assert rel_err(_nchw(a), b) < 1e-4
    assert [f.shape[1] for f in fm] == [74, 36, 17, 17, 17]
    got = m(x.to(DEV), y.to(DEV)).double().cpu()
    want = ref.per_image(x, y)
    assert ((got - want).abs() / want.abs()).max().item() < 1e-4
    assert torch.equal(m(x.to(DEV), x.to(DEV)), torch.zeros(3, device=DEV))
    assert (m(y.to(DEV), x.to(DEV)).cpu() - got.float()).abs().max().item() < 1e-7 * max(1.0, got.abs().max().item()) + 1e-7
    assert torch.equal(m(x.to(DEV), y.to(DEV)), m(x.to(DEV), y.to(DEV)))


@pytest.mark.parametrize('dims', [64, 192, 768, 2048])
@pytest.mark.parametrize('prec,tol', [(None, 1e-4), ('f32', 1e-5)])
def test_inception_features(dims, prec, tol):
    from hoig_amd.metrics.fid import InceptionFeatures
    sd = R.inception_state_dict(4)
    m = InceptionFeatures(sd, dims, prec, DEV)
    rng = np.random.RandomState(dims)
    u8 = rng.randint(0, 256, size=(2, 256, 256, 3)).astype(np.uint8)
    got = m.features_u8(torch.from_numpy(u8).to(DEV))
    want = R.InceptionRef(sd, dims).features(torch.from_numpy(u8).permute(0, 3, 1, 2).double() / 255)
    assert got.shape == (2, dims)
    assert rel_err(got, want) < tol
    assert torch.equal(got, m.features_u8(torch.from_numpy(u8).to(DEV)))


def test_fid_end_to_end(tmp_path):
    from hoig_amd.metrics.fid import calculate_fid_given_paths
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    fa, fb = R.write_pngs(a, 128, 256, 10), R.write_pngs(b, 128, 256, 11)
    sd = R.inception_state_dict(5)
    got = calculate_fid_given_paths([a, b], 50, DEV, 64, weights=sd)
    ref = R.InceptionRef(sd, 64)
    stats = []
    for files in (fa, fb):
        feats = torch.cat([ref.features(torch.stack([R.fid_tensor(p) for p in files[i:i + 32]])) for i in range(0, 128, 32)])
        f = feats.numpy()
        stats += [f.mean(0), np.cov(f, rowvar=False)]
    want = R.frechet_distance(*stats)
    assert abs(got - want) / abs(want) < 1e-3, (got, want)
    assert got == calculate_fid_given_paths([a, b], 50, DEV, 64, weights=sd)


def test_path_level_lpips_and_ssim(tmp_path):
    from hoig_amd.metrics.lpips import calculate_lpips_given_paths
    from hoig_amd.metrics.ssim import calculate_ssim_given_paths
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    fa, fb = R.write_pngs(a, 12, 256, 20), R.write_pngs(b, 12, 256, 21)
    xs = torch.stack([R.eval_loader_tensor(p) for p in fa])
    ys = torch.stack([R.eval_loader_tensor(p) for p in fb])
    m = _lpips('f32')
    got = calculate_lpips_given_paths([a, b], 256, 5, model=m)
    want = R.lpips_given_batches(R.LPIPSRef(R.alexnet_state_dict(1), R.lpips_state_dict(2)), xs, ys, 5)
    assert abs(got - want) / abs(want) < 1e-5, (got, want)
    assert got == calculate_lpips_given_paths([a, b], 256, 5, model=m)
    s, ms = calculate_ssim_given_paths([a, b], 256, 4)
    ws = R.ssim_level(xs, ys, 255)[0].mean(1).mean().item()
    wms = R.ms_ssim_per_channel(xs, ys, 255).mean(1).mean().item()
    assert abs(s - ws) < 1e-5 and abs(ms - wms) < 1e-5, (s, ws, ms, wms)
    assert (s, ms) == calculate_ssim_given_paths([a, b], 256, 4)


def test_mixed_sizes_raise(tmp_path):
    from hoig_amd.metrics.fid import get_activations, InceptionFeatures
    names = R.write_pngs(str(tmp_path), 2, 64, 1) + R.write_pngs(str(tmp_path), 1, 80, 2, prefix='big')
    m = InceptionFeatures(R.inception_state_dict(6), 64, None, DEV)
    with pytest.raises(ValueError, match='differ in size'):
        get_activations(names, m, batch_size=3, dims=64)
