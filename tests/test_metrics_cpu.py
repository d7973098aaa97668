"""Host logic of hoig_amd.metrics (no GPU): BN folding, weight files, the Frechet distance, file lists, the LPIPS aggregation, the
PIL resize chain and the command line."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import metrics_reference as R
from quality_metrics import frechet_distance
from hoig_amd.metrics import fid, images, lpips, weights
from hoig_amd.metrics.__main__ import main as cli


def test_bn_fold_matches_conv_then_bn():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 8, 9, 11, generator=g, dtype=torch.float64)
    w = torch.randn(5, 8, 3, 1, generator=g, dtype=torch.float64)
    gamma, beta = torch.rand(5, generator=g, dtype=torch.float64) + 0.5, torch.randn(5, generator=g, dtype=torch.float64)
    mean, var = torch.randn(5, generator=g, dtype=torch.float64), torch.rand(5, generator=g, dtype=torch.float64) + 0.5
    want = F.batch_norm(F.conv2d(x, w, padding=(1, 0)), mean, var, gamma, beta, False, 0.0, 1e-3)
    wf, bf = fid.fold_bn(w, gamma, beta, mean, var)
    got = F.conv2d(x, wf, bf, padding=(1, 0))
    assert (got - want).abs().max().item() < 1e-12


def test_inception_layer_table_matches_restatement():
    mine = [(n, ci, co, k, s, p) for layers in fid.BLOCK_LAYERS for n, ci, co, k, s, p in layers]
    ref = [(l['name'], l['ci'], l['co'], l['k'], l['stride'], l['pad']) for l in R.inception_layers()]
    assert mine == ref and len(mine) == 94


def test_inception_weights_load_from_real_key_names(tmp_path):
    sd = R.inception_state_dict(3)
    path = str(tmp_path / weights.INCEPTION_FILE)
    torch.save(sd, path)
    for dims, n in ((64, 3), (192, 5), (768, 5 + 21 + 4 + 40), (2048, 94)):
        got = fid.load_inception(path, dims)
        assert len(got) == n
    w, b = fid.load_inception(path, 64)['Conv2d_2a_3x3']
    ref_w, ref_b = fid.fold_bn(sd['Conv2d_2a_3x3.conv.weight'].double(), *[sd['Conv2d_2a_3x3.bn.' + k].double() for k in
                                                                            ('weight', 'bias', 'running_mean', 'running_var')])
    assert torch.equal(w, ref_w) and torch.equal(b, ref_b)


def test_inception_weights_rejected_with_names(tmp_path):
    sd = R.inception_state_dict(3, extras=False)
    bad = dict(sd)
    del bad['Mixed_6e.branch7x7dbl_4.bn.running_var']
    path = str(tmp_path / 'missing.pth')
    torch.save(bad, path)
    fid.load_inception(path, 192)                         # the block of 192 does not need Mixed_6e
    with pytest.raises(RuntimeError, match=r'missing\.pth.*Mixed_6e\.branch7x7dbl_4\.bn\.running_var'):
        fid.load_inception(path, 768)
    bad = dict(sd)
    bad['Conv2d_1a_3x3.conv.weight'] = torch.zeros(32, 3, 5, 5)
    path = str(tmp_path / 'shape.pth')
    torch.save(bad, path)
    with pytest.raises(RuntimeError, match=r'shape\.pth.*Conv2d_1a_3x3\.conv\.weight.*\(32, 3, 3, 3\)'):
        fid.load_inception(path, 64)


def test_no_weights_no_metric(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.hub, 'get_dir', lambda: str(tmp_path))
    monkeypatch.chdir(tmp_path)
    with pytest.raises(RuntimeError, match='FID Inception weights not found'):
        fid.InceptionFeatures(dims=64)
    with pytest.raises(RuntimeError, match='AlexNet weights not found'):
        lpips.LPIPS()
    torch.save(R.alexnet_state_dict(), str(tmp_path / 'alex.pth'))
    with pytest.raises(RuntimeError, match=r'LPIPS heads weights not found.*metrics/lpips_weights\.ckpt'):
        lpips.LPIPS(alexnet_weights=str(tmp_path / 'alex.pth'))


def test_alexnet_and_head_key_forms(tmp_path, monkeypatch):
    a = lpips.load_alexnet(R.alexnet_state_dict(1))
    b = lpips.load_alexnet(R.alexnet_state_dict(1, prefix='alexnet.layers.'))
    assert all(torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]) for p, q in zip(a, b))
    heads = R.lpips_state_dict(2)
    os.makedirs(str(tmp_path / 'metrics'))
    torch.save({'module.' + k: v for k, v in heads.items()}, str(tmp_path / 'metrics' / 'lpips_weights.ckpt'))
    monkeypatch.chdir(tmp_path)
    got = lpips.load_lpips_heads(None)                   # found where the reference looks, 'module.' stripped
    assert [tuple(h.shape) for h in got] == [(64,), (192,), (384,), (256,), (256,)]
    assert torch.equal(got[2], heads['lpips_weights.2.main.1.weight'].double().view(-1))
    bad = dict(heads)
    bad['lpips_weights.3.main.1.weight'] = torch.zeros(1, 384, 1, 1)
    with pytest.raises(RuntimeError, match=r'lpips_weights\.3\.main\.1\.weight'):
        lpips.load_lpips_heads(bad)


def test_frechet_distance_matches_restatement(tmp_path):
    rng = np.random.RandomState(0)
    a, b = rng.randn(200, 16), rng.randn(180, 16) * 1.3 + 0.2
    m1, s1 = a.mean(0), np.cov(a, rowvar=False)
    m2, s2 = b.mean(0), np.cov(b, rowvar=False)
    assert abs(fid.calculate_frechet_distance(m1, s1, m2, s2) - frechet_distance(m1, s1, m2, s2)) < 1e-9
    # fewer samples than dimensions: singular covariances, the eps path
    a, b = rng.randn(6, 32), rng.randn(6, 32)
    m1, s1, m2, s2 = a.mean(0), np.cov(a, rowvar=False), b.mean(0), np.cov(b, rowvar=False)
    want = frechet_distance(m1, s1, m2, s2)
    assert np.isfinite(want) and abs(fid.calculate_frechet_distance(m1, s1, m2, s2) - want) < 1e-9 * max(1.0, abs(want))
    p = str(tmp_path / 'stats.npz')
    np.savez(p, mu=m1, sigma=s1)
    mu, sigma = fid.compute_statistics_of_path(p, None, 50, 2048)
    assert np.array_equal(mu, m1) and np.array_equal(sigma, s1)


def test_file_order_and_extension_filter(tmp_path):
    for n in ('b.png', 'a.jpg', 'c.PNG', 'd.txt', 'e.webp', '10.png', '9.png'):
        (tmp_path / n).write_bytes(b'')
    (tmp_path / 'sub.png').mkdir()                                      # directory is listed too)
    got = [os.path.basename(p) for p in images.list_images(str(tmp_path))]
    assert got == ['10.png', '9.png', 'a.jpg', 'b.png', 'e.webp', 'sub.png']    # (pathlib's glob, as fid_score.py: a matching
    with pytest.raises(RuntimeError, match='Invalid path'):
        images.list_images(str(tmp_path / 'nope'))


def test_resize_chain_is_pil_bilinear_twice(tmp_path):
    path = R.write_pngs(str(tmp_path), 1, 256, 5)[0]
    want = np.asarray(Image.open(path).convert('RGB').resize((128, 128), Image.BILINEAR).resize((299, 299), Image.BILINEAR))
    assert np.array_equal(images.decode(path, 128), want)
    assert np.array_equal(images.decode(path), np.asarray(Image.open(path).convert('RGB')))


def test_mixed_sizes_raise_before_the_device(tmp_path):
    names = R.write_pngs(str(tmp_path / 'a'), 2, 32, 1) + R.write_pngs(str(tmp_path / 'b'), 1, 40, 2)
    with pytest.raises(ValueError, match='differ in size'):
        list(images.DeviceBatches([names], 'cpu'))


class _FakeLPIPS(object):
    """distance_u8 = the mean pixel value of each x image: the aggregation alone is under test."""
    device = torch.device('cpu')

    def distance_u8(self, u8):
        n = u8.shape[0] // 2
        return u8[:n].double().mean(dim=(1, 2, 3))


def test_lpips_path_value_is_mean_of_batch_means(tmp_path):
    a = R.write_pngs(str(tmp_path / 'a'), 7, 24, 3)
    R.write_pngs(str(tmp_path / 'b'), 7, 24, 4)
    got = lpips.calculate_lpips_given_paths([str(tmp_path / 'a'), str(tmp_path / 'b')], img_size=24, batch_size=3,
                                            model=_FakeLPIPS())
    per = [float(images.decode(p, 24).astype(np.float64).mean()) for p in a]
    want = np.mean([np.mean(per[0:3]), np.mean(per[3:6]), np.mean(per[6:7])])
    assert abs(got - want) < 1e-9
    assert abs(got - np.mean(per)) > 1e-6            # (not the mean over images)


def test_ssim_level_equals_a_literal_loop_over_windows():
    X, Y = R.ssim_pair(1, 2, 13, 12, 1.0, 5)
    X, Y = X.double(), Y.double()
    win, C1, C2 = 3, 0.01 ** 2, 0.03 ** 2
    g = R.gauss_window(win, 1.5)
    g2 = g.view(-1, 1) * g.view(1, -1)
    s, cs = R.ssim_level(X, Y, 1.0, win)
    assert s.shape == (1, 2) and cs.shape == (1, 2)
    for c in range(2):
        sv, cv = [], []
        for i in range(13 - win + 1):
            for j in range(12 - win + 1):
                a, b = X[0, c, i:i + win, j:j + win], Y[0, c, i:i + win, j:j + win]
                ma, mb = (g2 * a).sum(), (g2 * b).sum()
                va, vb, vab = (g2 * a * a).sum() - ma * ma, (g2 * b * b).sum() - mb * mb, (g2 * a * b).sum() - ma * mb
                cv.append((2 * vab + C2) / (va + vb + C2))
                sv.append((2 * ma * mb + C1) / (ma * ma + mb * mb + C1) * cv[-1])
        assert len(sv) == 11 * 10
        assert abs(torch.stack(sv).mean().item() - s[0, c].item()) < 1e-12
        assert abs(torch.stack(cv).mean().item() - cs[0, c].item()) < 1e-12


def test_ssim_pair_spans_far_to_close():
    X, Y = R.ssim_pair(3, 2, 27, 75, 255.0, 1)
    assert X.dtype == torch.float32 and X.shape == Y.shape == (3, 2, 27, 75)
    assert 0 <= X.min() and X.max() <= 255 and 0 <= Y.min() and Y.max() <= 255 and X.max() > 100
    s = R.ssim_level(X, Y, 255.0)[0].mean(1)
    assert s[0] < s[1] < s[2] and s[0] < 0.1 and s[2] > 0.5, s


def test_lpips_layer_reference():
    g = torch.Generator().manual_seed(0)
    fx = torch.relu(torch.randn(3, 37, 20, generator=g, dtype=torch.float64))
    fy = torch.relu(torch.randn(3, 37, 20, generator=g, dtype=torch.float64))
    w = torch.rand(20, generator=g, dtype=torch.float64)
    v = R.lpips_layer(fx, fy, w)
    assert v.shape == (3,) and v.min() > 0
    assert torch.equal(v, R.lpips_layer(fy, fx, w))                     # symmetric
    assert torch.equal(R.lpips_layer(fx, fx, w), torch.zeros(3, dtype=torch.float64))
    # a literal loop over pixels and channels
    want = 0.0
    for p in range(37):
        nx, ny = (fx[1, p] ** 2).sum() + 1e-10, (fy[1, p] ** 2).sum() + 1e-10
        want += sum(w[c] * (fx[1, p, c] / nx.sqrt() - fy[1, p, c] / ny.sqrt()) ** 2 for c in range(20))
    assert abs(want.item() / 37 - v[1].item()) < 1e-12


def test_lpips_per_image_keeps_its_value():
    """per_image now goes through lpips_layer: the value it had as a 1x1 convolution of the squared difference of NCHW maps."""
    ref = R.LPIPSRef(R.alexnet_state_dict(1), R.lpips_state_dict(2))
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(2, 3, 67, 75, generator=g), torch.randn(2, 3, 67, 75, generator=g)
    mu, sigma = torch.tensor(R.LPIPS_MU).double().view(1, 3, 1, 1), torch.tensor(R.LPIPS_SIGMA).double().view(1, 3, 1, 1)
    old = 0
    for a, b, w in zip(ref.fmaps((x.double() - mu) / sigma), ref.fmaps((y.double() - mu) / sigma), ref.heads):
        na = a * torch.rsqrt((a ** 2).sum(1, keepdim=True) + 1e-10)
        nb = b * torch.rsqrt((b ** 2).sum(1, keepdim=True) + 1e-10)
        old = old + F.conv2d((na - nb) ** 2, w).mean(dim=(1, 2, 3))
    got = ref.per_image(x, y)
    assert old.min() > 0.01 and (got - old).abs().max().item() < 1e-12


def test_cli_validates_arguments(tmp_path):
    R.write_pngs(str(tmp_path / 'a'), 1, 16, 0)
    with pytest.raises(SystemExit):
        cli(['fid', str(tmp_path / 'a'), str(tmp_path / 'a'), '--dims', '100'])
    with pytest.raises(RuntimeError, match='Invalid path: .*missing'):
        cli(['lpips', str(tmp_path / 'a'), str(tmp_path / 'missing')])
    with pytest.raises(ValueError, match='dims'):
        fid.InceptionFeatures(dims=100)
