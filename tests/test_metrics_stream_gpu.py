"""Scoring from device memory (hoig_amd.metrics.stream, Trainer.eval_images_u8, EvalWriter.write_images) on the MI355X: EQUAL to
the path functions on directories of the same images, which tests/test_metrics_gpu.py pins to the fp64 restatements."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import metrics_reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
N, LPIPS_BATCH, SSIM_BATCH, FID_BATCH, DIMS = 12, 5, 4, 50, 64
CALLS = (5, 1, 6)                       # update() sizes: none of them a batch of any metric


def _read(names):
    return torch.from_numpy(np.stack([np.asarray(Image.open(n).convert('RGB')) for n in names])).to(DEV)


@pytest.fixture(scope='module')
def pairs(tmp_path_factory):
    """12 pairs of 256 x 256 PNGs, their bytes on the device, the three networks and the path functions' values."""
    from hoig_amd.metrics.fid import InceptionFeatures, calculate_fid_given_paths
    from hoig_amd.metrics.lpips import LPIPS, calculate_lpips_given_paths
    from hoig_amd.metrics.ssim import calculate_ssim_given_paths
    root = tmp_path_factory.mktemp('pairs')
    a, b = str(root / 'gen'), str(root / 'gt')
    gen, gt = _read(R.write_pngs(a, N, 256, 20)), _read(R.write_pngs(b, N, 256, 21))
    sd = R.inception_state_dict(5)
    lp = LPIPS(R.alexnet_state_dict(1), R.lpips_state_dict(2), precision='f32', device=DEV)
    want = dict(n=N, fid=calculate_fid_given_paths([a, b], FID_BATCH, DEV, DIMS, weights=sd),
                lpips=calculate_lpips_given_paths([a, b], 256, LPIPS_BATCH, model=lp))
    want['ssim'], want['ms_ssim'] = calculate_ssim_given_paths([a, b], 256, SSIM_BATCH)
    return dict(dirs=[a, b], gen=gen, gt=gt, lpips=lp, inception=InceptionFeatures(sd, DIMS, None, DEV), want=want, root=root)


def _scorer(p, **over):
    from hoig_amd.metrics.stream import Scorer
    kw = dict(fid=p['inception'], lpips=p['lpips'], ssim=True, img_size=256, fid_batch=FID_BATCH, lpips_batch=LPIPS_BATCH,
              ssim_batch=SSIM_BATCH)
    kw.update(over)
    return Scorer(**kw)


def _feed(s, gen, gt, calls=CALLS):
    at = 0
    for n in calls:
        s.update(gen[at:at + n], gt[at:at + n])
        at += n
    assert at == gen.shape[0]
    return s


def test_nhwc_tensor2im_gives_the_grids_crops():
    """B = 5 at nrow 2: a ragged 3 x 2 grid."""
    from hoig_amd import ops
    from hoig_amd.eval_output import crops_of
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(5, 16, 16, 3, generator=g) * 2.2 - 1.1).clamp(-1, 1).to(DEV)
    x[0, 0, 0] = torch.tensor([-1.0, 1.0, 0.0])
    for unnormalize in (True, False):
        xin = x if unnormalize else (x + 1) / 2
        got = ops.tensor2im_nhwc_u8(xin, unnormalize)
        assert got.shape == (5, 16, 16, 3) and got.dtype == torch.uint8 and got.is_cuda
        want = crops_of(ops.tensor2im_u8(xin, 2, unnormalize).cpu().numpy(), 5, 16)
        assert np.array_equal(got.cpu().numpy(), np.stack(want))
    assert got.cpu().numpy().max() == 255 and got.cpu().numpy().min() == 0


def test_the_scorer_equals_the_path_functions(pairs):
    got = _feed(_scorer(pairs), pairs['gen'], pairs['gt']).result()
    print(got, pairs['want'])
    assert got == pairs['want']


def test_the_path_functions_with_device_resize_give_the_same(pairs):
    from hoig_amd.metrics.lpips import calculate_lpips_given_paths
    from hoig_amd.metrics.ssim import calculate_ssim_given_paths
    want = pairs['want']
    got = calculate_lpips_given_paths(pairs['dirs'], 256, LPIPS_BATCH, model=pairs['lpips'], device_resize=True)
    print(got, want['lpips'])
    assert got == want['lpips']
    got = calculate_ssim_given_paths(pairs['dirs'], 256, SSIM_BATCH, device_resize=True)
    print(got, want['ssim'], want['ms_ssim'])
    assert got == (want['ssim'], want['ms_ssim'])


def test_the_grouping_of_updates_does_not_matter_and_result_keeps_the_state(pairs):
    s = _scorer(pairs, fid=None)
    _feed(s, pairs['gen'][:7], pairs['gt'][:7], (3, 4))
    part = s.result()
    assert part['n'] == 7 and 'fid' not in part
    _feed(s, pairs['gen'][7:], pairs['gt'][7:], (5,))
    got = s.result()
    assert {k: got[k] for k in ('n', 'lpips', 'ssim', 'ms_ssim')} == {k: pairs['want'][k] for k in ('n', 'lpips', 'ssim', 'ms_ssim')}
    only = _feed(_scorer(pairs, fid=None, lpips=None, ssim_batch=LPIPS_BATCH), pairs['gen'], pairs['gt'], (12,)).result()
    assert sorted(only) == ['ms_ssim', 'n', 'ssim']


def test_statistics_round_trip_and_fid_reference(pairs):
    from hoig_amd.metrics.fid import compute_statistics_of_path
    # the ground truth's statistics, saved by a scorer that is given it as its generated set
    s = _feed(_scorer(pairs, lpips=None, ssim=False), pairs['gt'], pairs['gen'])
    path = str(pairs['root'] / 'gt_stats.npz')
    s.save_statistics(path)
    mu, sigma = compute_statistics_of_path(path, None, FID_BATCH, DIMS)
    want_mu, want_sigma = s.statistics()
    assert mu.shape == (DIMS,) and sigma.shape == (DIMS, DIMS)
    assert np.array_equal(mu, want_mu) and np.array_equal(sigma, want_sigma)
    m2, s2 = compute_statistics_of_path(pairs['dirs'][1], pairs['inception'], FID_BATCH, DIMS)
    assert np.array_equal(mu, m2) and np.array_equal(sigma, s2)
    for ref in (path, (mu, sigma)):
        got = _feed(_scorer(pairs, lpips=None, ssim=False, fid_reference=ref), pairs['gen'], pairs['gt']).result()
        assert got == dict(n=N, fid=pairs['want']['fid'])


def test_trainer_eval_images_and_write_images(tmp_path):
    from common import product_trainer
    from hoig_amd.eval_output import EvalWriter, GRIDS, crops_of
    m = product_trainer('generator_spade_attn', 2, 64)
    with torch.no_grad():
        outs = m.forward(keep_data_for_visuals=True)
        images = m.eval_images_u8(outs)
    vis = m.get_current_visuals()
    assert list(images) == ['source', 'imitators', 'gt']
    for sub, key in GRIDS:
        assert images[sub].shape == (2, 64, 64, 3) and images[sub].dtype == torch.uint8 and images[sub].is_cuda
        assert np.array_equal(images[sub].cpu().numpy(), np.stack(crops_of(vis[key], 2, 64))), sub
    assert not torch.equal(images['imitators'], images['gt'])
    # without the visuals: the same bytes from a plain forward
    with torch.no_grad():
        again = m.eval_images_u8(m.forward())
    assert torch.equal(again['source'], images['source']) and torch.equal(again['gt'], images['gt'])
    # (a second forward may differ in the last bit of a norm's atomically summed statistics: one grey level at a truncation)
    assert (again['imitators'].int() - images['imitators'].int()).abs().max().item() <= 1
    names_a, names_b = ['v1/0001.jpg', 'v2/0007.jpg'], ['v1/0002.jpg', 'v2/0009.jpg']
    for sub, how in (('grid', 'write'), ('bytes', 'write_images')):
        w = EvalWriter(str(tmp_path / sub), sav_gt=True, side=64)
        getattr(w, how)(vis if how == 'write' else images, names_a, names_b)
        w.close()
        assert w.written == 6
    for sub, _ in GRIDS:
        files = sorted(os.listdir(str(tmp_path / 'grid' / sub)))
        assert files == sorted(os.listdir(str(tmp_path / 'bytes' / sub))) == ['v1_0001_0002.png', 'v2_0007_0009.png']
        for f in files:
            with open(str(tmp_path / 'grid' / sub / f), 'rb') as x, open(str(tmp_path / 'bytes' / sub / f), 'rb') as y:
                assert x.read() == y.read(), (sub, f)


def test_score_model_runs_the_loop(pairs, tmp_path):
    """score_model on a stand-in model that hands out the fixture's images: the scorer's values and the writer's files."""
    from hoig_amd.eval_output import EvalWriter
    from hoig_amd.metrics.stream import score_model

    class Model(object):
        def set_input(self, batch):
            self.at = batch['at']

        def forward(self):
            assert not torch.is_grad_enabled()
            return self.at

        def eval_images_u8(self, at):
            sl = slice(at, at + 4)
            return {'source': pairs['gt'][sl], 'imitators': pairs['gen'][sl], 'gt': pairs['gt'][sl]}

    data = [dict(at=i, nameA=['v/%04d.jpg' % k for k in range(i, i + 4)], nameB=['v/%04d.jpg' % (k + 1) for k in range(i, i + 4)])
            for i in (0, 4, 8)]
    w = EvalWriter(str(tmp_path), sav_gt=True)
    got = score_model(Model(), data, _scorer(pairs, fid=None), writer=w)
    w.close()
    assert {k: got[k] for k in got} == {k: pairs['want'][k] for k in ('n', 'lpips', 'ssim', 'ms_ssim')}
    files = sorted(os.listdir(str(tmp_path / 'imitators')))
    assert len(files) == N and w.written == 3 * N
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / 'imitators' / files[5]))), pairs['gen'][5].cpu().numpy())
