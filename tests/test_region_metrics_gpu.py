"""The region scores on the MI355X (hoig_amd/csrc/region_metrics.hip, hoig_amd/metrics/regions.py, Scorer(regions=...)): the kernels
EQUAL to their CPU twins, which tests/test_region_metrics_cpu.py pins to numpy and Pillow, and the scorer's values equal to the same
functions called on Pillow-made crops."""
import itertools
import os

import numpy as np
import pytest
import torch

import metrics_reference as M
import region_metrics_reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
N, SIDE, SIZE, MIN_PIXELS, BATCH, DIMS = 8, 64, 32, 64, 3, 64
CALLS = (5, 1, 2)
KID = dict(subsets=4, subset_size=6, seed=1)
REGION_OPTS = dict(size=SIZE, min_pixels=MIN_PIXELS, batch=BATCH)


def _t(a, dev='cpu'):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _images(n, side, seed):
    """Seeded RGB images (smooth gradients plus noise, as metrics_reference.write_pngs makes them)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:side, 0:side] / float(side)
    out = []
    for _ in range(n):
        base = np.stack([np.sin(6.28 * (xx * rng.uniform(0.5, 3) + rng.uniform())), np.cos(6.28 * (yy * rng.uniform(0.5, 3) + rng.uniform())),
                         xx * yy], -1) * 0.5 + 0.5
        out.append(np.clip(base * 200 + rng.uniform(0, 55, size=base.shape), 0, 255).astype(np.uint8))
    return np.stack(out)


# ------------------------------------------------------------------------------------------------ the kernels against their twins
@pytest.mark.parametrize('shape', R.STATS_SHAPES + [(70, 90)], ids=lambda s: '%dx%d' % s)
def test_the_stats_kernel_equals_its_twin(shape):
    """(70, 90): 6300 pixels, two workgroups per image."""
    from hoig_amd.metrics import regions as G
    gen, gt, lab = R.stats_case(*shape)
    for regions, labels in ((2, lab), (7, np.random.default_rng(5).integers(0, 8, size=lab.shape, dtype=np.uint8))):
        want, want_status = G.region_stats(_t(gen), _t(gt), _t(labels), regions)
        got, status = G.region_stats(_t(gen, DEV), _t(gt, DEV), _t(labels, DEV), regions)
        assert torch.equal(got.cpu(), want), regions
        assert int(status.item()) == int(want_status) == ((1 | 3 << 8) if regions == 2 else 0)
    ref, _ = R.stats(gen, gt, lab)
    assert np.array_equal(G.region_stats(_t(gen, DEV), _t(gt, DEV), _t(lab, DEV))[0].cpu().numpy(), ref)


def test_the_box_kernel_equals_its_twin():
    from hoig_amd.metrics import regions as G
    H, W = 9, 12
    rows = [(x0, y0, x1, y1) for x0, x1 in itertools.combinations_with_replacement(range(W), 2)
            for y0, y1 in itertools.combinations_with_replacement(range(H), 2)]
    st = np.zeros((len(rows), 2, 8), np.int64)
    st[:, 1, 0] = 5
    st[:, 1, 3:7] = rows
    st[::7, 1, 0] = 4
    for min_pixels in (0, 4, 5, 6):
        want = G.region_boxes(_t(st), H, W, min_pixels)
        assert torch.equal(G.region_boxes(_t(st, DEV), H, W, min_pixels).cpu(), want)
        assert np.array_equal(want.numpy(), R.boxes(st, H, W, min_pixels))
    for H, W in ((20, 64), (64, 20)):
        st = np.zeros((2, 3, 8), np.int64)
        st[:, 1:, 0] = 100
        st[0, 1, 3:7], st[0, 2, 3:7] = (2, 1, 17, 16), (W - 18, H - 18, W - 1, H - 1)
        st[1, 1, 3:7], st[1, 2, 3:7] = (0, 0, W - 1, H - 1), (W // 2, H // 2, W // 2, H // 2)
        assert torch.equal(G.region_boxes(_t(st, DEV), H, W, 64).cpu(), G.region_boxes(_t(st), H, W, 64))


@pytest.mark.parametrize('case', R.CROP_CASES, ids=lambda c: '%dx%d-%d' % (c[0] + (c[1],)))
def test_the_crop_kernels_equal_their_twin_and_pillow(case):
    from hoig_amd.metrics import regions as G
    images, bxs = R.crop_case(case)
    want = G.region_crops(_t(images), _t(bxs), case[1])
    got = G.region_crops(_t(images, DEV), _t(bxs, DEV), case[1]).cpu()
    assert torch.equal(got, want)
    assert np.array_equal(got.numpy(), R.crops(images, bxs, case[1]))
    assert not got[0, -1].any()                                          # the invalid box of the batch


def test_two_regions_and_boxes_outside_the_image_give_zeros():
    """Two regions per image in one launch; a box that is not inside the image is treated as invalid, not followed."""
    from hoig_amd.metrics import regions as G
    images = R.content(3, 33, 47, 1)
    bxs = np.array([[[0, 0, 33, 1], [40, 26, 7, 1]], [[5, 4, 12, 1], [41, 0, 7, 1]], [[-1, 0, 8, 1], [0, 0, 34, 1]]], np.int32)
    got = G.region_crops(_t(images, DEV), _t(bxs, DEV), 16).cpu()
    assert torch.equal(got, G.region_crops(_t(images), _t(bxs), 16))
    ok = bxs.copy()
    ok[1, 1] = ok[2, 0] = ok[2, 1] = 0
    assert np.array_equal(got.numpy(), R.crops(images, ok, 16))


# ------------------------------------------------------------------------------------------------ the trainer's label map
def test_trainer_eval_regions_u8():
    import common
    from hoig_amd import synthetic
    m = common.product_trainer('generator_spade_attn', 2, 64)
    lab = m.eval_regions_u8()
    assert lab.shape == (2, 64, 64) and lab.dtype == torch.uint8 and lab.is_cuda
    n = m._n
    want = R.labels_from_masks(n['bg_mask'][2:, :, :, 0].cpu().numpy(), n['hand_mask'][2:, :, :, 0].cpu().numpy())
    assert np.array_equal(lab.cpu().numpy(), want)
    inp = synthetic.make_inputs(2, 64, seed=common.SEEDS['inputs'])
    assert np.array_equal(want, R.labels_from_masks(inp['bg_mask'][2:, 0].numpy(), inp['hand_mask'][2:, 0].numpy()))
    assert sorted(np.unique(want).tolist()) == [0, 1, 2]
    with torch.no_grad():
        assert list(m.eval_images_u8(m.forward())) == ['source', 'imitators', 'gt']


# ------------------------------------------------------------------------------------------------ the scorer
@pytest.fixture(scope='module')
def data():
    """8 image pairs at 64 x 64 with the target-view labels of make_inputs(8, 64, seed=8), the Pillow-made crops and the networks."""
    from hoig_amd import synthetic
    from hoig_amd.metrics.fid import InceptionFeatures
    from hoig_amd.metrics.lpips import LPIPS
    inp = synthetic.make_inputs(N, SIDE, seed=8)
    lab = R.labels_from_masks(inp['bg_mask'][N:, 0].numpy(), inp['hand_mask'][N:, 0].numpy())
    gen, gt = _images(N, SIDE, 30), _images(N, SIDE, 31)
    st, _ = R.stats(gen, gt, lab)
    bx = R.boxes(st, SIDE, SIDE, MIN_PIXELS)
    return dict(gen=gen, gt=gt, lab=lab, boxes=bx, crops=(R.crops(gen, bx, SIZE), R.crops(gt, bx, SIZE)),
                dev=(_t(gen, DEV), _t(gt, DEV), _t(lab, DEV)), inception=InceptionFeatures(M.inception_state_dict(5), DIMS, None, DEV),
                lpips=LPIPS(M.alexnet_state_dict(1), M.lpips_state_dict(2), precision='f32', device=DEV))


def _feed(s, d, calls=CALLS):
    at = 0
    for n in calls:
        s.update(*(t[at:at + n] for t in d['dev']))
        at += n
    assert at == N
    return s


def _batches(d, r):
    """(generated, ground truth) reference crops of region r on the device, in the scorer's batches."""
    g, t = _t(d['crops'][0][r], DEV), _t(d['crops'][1][r], DEV)
    return [(g[i:i + BATCH].contiguous(), t[i:i + BATCH].contiguous()) for i in range(0, N, BATCH)]


def test_the_scorer_without_networks(data):
    from hoig_amd.metrics import kernels as K
    from hoig_amd.metrics.ssim import ssim_nhwc
    from hoig_amd.metrics.stream import Scorer
    got = _feed(Scorer(fid=None, lpips=None, ssim=True, regions=dict(size=SIZE, min_pixels=MIN_PIXELS)), data, (N,)).result()
    want = R.scalars(data['gen'], data['gt'], data['lab'], MIN_PIXELS)
    print(got, want)
    assert got['n'] == N and got['n_hand'] == want['n_hand'] == 8 and got['n_object'] == want['n_object'] == 7
    for key in ('psnr', 'mae', 'psnr_hand', 'mae_hand', 'psnr_object', 'mae_object'):
        assert abs(got[key] - want[key]) <= 1e-12 * abs(want[key]), key
    for r, name in enumerate(R.NAMES):
        valid = _t(data['boxes'][:, r, 3] != 0, DEV)
        g, t = _t(data['crops'][0][r], DEV), _t(data['crops'][1][r], DEV)           # the default batch of 50: one short batch of 8
        per_image = ssim_nhwc(K.stage_images_u8(torch.cat([g, t]).contiguous(), None, ()), data_range=1.0).mean(1)
        assert got['ssim_' + name] == per_image[valid].double().mean().item()
    assert sorted(got) == sorted(['n', 'ssim', 'ms_ssim', 'psnr', 'mae'] + [k + '_' + r for r in R.NAMES for k in ('n', 'psnr', 'mae', 'ssim')])


def test_the_scorer_with_networks_and_any_grouping_of_updates(data):
    from hoig_amd.metrics import kernels as K
    from hoig_amd.metrics.feature_metrics import kid_from_features
    from hoig_amd.metrics.fid import calculate_frechet_distance
    from hoig_amd.metrics.fid_device import Moments, frechet_distance_device
    from hoig_amd.metrics.ssim import ssim_nhwc
    from hoig_amd.metrics.stream import Scorer
    kw = dict(fid=data['inception'], lpips=data['lpips'], ssim=True, img_size=SIDE, kid=KID, regions=REGION_OPTS)
    s = _feed(Scorer(**kw), data)
    got = s.result()
    want, want_dev = {}, {}
    for r, name in enumerate(R.NAMES):
        valid = _t(data['boxes'][:, r, 3] != 0, DEV)
        lp, ss, fg, ft = [], [], [], []
        for g, t in _batches(data, r):
            pair = torch.cat([g, t]).contiguous()
            lp.append(data['lpips'].distance_u8(pair))
            ss.append(ssim_nhwc(K.stage_images_u8(pair, None, ()), data_range=1.0).mean(1))
            fg.append(data['inception'].features_u8(g).clone())
            ft.append(data['inception'].features_u8(t).clone())
        want['lpips_' + name] = torch.cat(lp)[valid].double().mean().item()
        want['ssim_' + name] = torch.cat(ss)[valid].double().mean().item()
        fg, ft = torch.cat(fg)[valid].contiguous(), torch.cat(ft)[valid].contiguous()
        a, b = fg.double().cpu().numpy(), ft.double().cpu().numpy()
        want['fid_' + name] = calculate_frechet_distance(np.mean(a, axis=0), np.cov(a, rowvar=False), np.mean(b, axis=0), np.cov(b, rowvar=False))
        want['kid_' + name], want['kid_std_' + name] = kid_from_features(fg, ft, **KID)
        stats = Moments(DIMS, DEV).update(fg).statistics() + Moments(DIMS, DEV).update(ft).statistics()
        want_dev['fid_' + name] = frechet_distance_device(*stats)
    print(got, want)
    assert {k: got[k] for k in want} == want
    # result() left the state usable, and one update() of 8 gives the values of (5, 1, 2)
    assert s.result() == got
    assert _feed(Scorer(**kw), data, (N,)).result() == got
    # the device Frechet distance takes the same valid rows
    dev = _feed(Scorer(**dict(kw, lpips=None, ssim=False, kid=None, fid_device=True)), data).result()
    print(dev, want_dev)
    assert {k: dev[k] for k in want_dev} == want_dev


def test_update_does_not_wait_for_the_device(data):
    """Under torch's sync debug mode a synchronising copy raises: the region half of update() makes none with every metric on, boxes
    and validity stay on the device until result().  (The scorer's region half on its own: the whole-frame MS-SSIM uploads its
    level weights in every call, which that mode counts.)"""
    from hoig_amd.metrics.regions import RegionScores
    gen, gt, lab = data['dev']
    s = RegionScores(REGION_OPTS, data['inception'], data['lpips'], True, KID, True)
    s.update(gen[:4], gt[:4], lab[:4])                             # (first use: the tap tables and whatever the networks set up lazily)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        s.update(gen[4:], gt[4:], lab[4:])
        with pytest.raises(RuntimeError):
            s.result()                                             # (the host reads here, and only here)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    out = s.result()
    assert s.n == N and out['n_hand'] == 8 and out['n_object'] == 7


def test_the_label_map_goes_with_the_option_and_only_with_it(data):
    from hoig_amd.metrics.stream import Scorer
    gen, gt, lab = data['dev']
    on, off = Scorer(fid=None, lpips=None, ssim=True, regions=REGION_OPTS), Scorer(fid=None, lpips=None, ssim=True)
    with pytest.raises(ValueError):
        on.update(gen, gt)
    with pytest.raises(ValueError):
        off.update(gen, gt, lab)
    with pytest.raises(ValueError):
        on.update(gen, gt, lab[:, :32])
    with pytest.raises(ValueError):
        Scorer(fid=None, lpips=None, ssim=True, regions=dict(size=8))          # SSIM's window
    off.update(gen, gt)
    assert sorted(off.result()) == ['ms_ssim', 'n', 'ssim'] and off.regions is None
    # a label the map does not know is named; a region no image shows is an error too
    bad = lab.clone()
    bad[3, 0, 0] = 3
    on.update(gen, gt, bad)
    with pytest.raises(ValueError, match='label 3'):
        on.result()
    none = Scorer(fid=None, lpips=None, ssim=False, regions=REGION_OPTS)
    none.update(gen, gt, lab * (lab != 2).to(torch.uint8))
    with pytest.raises(ValueError, match='object'):
        none.result()


def test_the_writer_the_path_function_and_the_command_line(data, tmp_path, capsys):
    from hoig_amd.eval_output import EvalWriter
    from hoig_amd.metrics.__main__ import main
    from hoig_amd.metrics.regions import calculate_region_metrics_given_paths
    from hoig_amd.metrics.stream import Scorer, score_model
    gen, gt, lab = data['dev']

    class Model(object):
        def set_input(self, batch):
            self.at = batch['at']

        def forward(self):
            return self.at

        def eval_images_u8(self, at):
            return {'source': gt[at:at + 4], 'imitators': gen[at:at + 4], 'gt': gt[at:at + 4]}

        def eval_regions_u8(self):
            return lab[self.at:self.at + 4]

    batches = [dict(at=i, nameA=['v/%04d.jpg' % k for k in range(i, i + 4)], nameB=['v/%04d.jpg' % (k + 1) for k in range(i, i + 4)])
               for i in (0, 4)]
    w = EvalWriter(str(tmp_path), sav_gt=True, side=SIDE, sav_regions=True)
    got = score_model(Model(), batches, Scorer(fid=data['inception'], lpips=data['lpips'], ssim=True, img_size=SIDE, kid=KID,
                                               regions=REGION_OPTS), writer=w)
    w.close()
    assert w.written == 4 * N and sorted(os.listdir(str(tmp_path))) == ['gt', 'imitators', 'regions', 'source']
    files = sorted(os.listdir(str(tmp_path / 'regions')))
    assert files == sorted(os.listdir(str(tmp_path / 'gt'))) and len(files) == N
    from PIL import Image
    with Image.open(str(tmp_path / 'regions' / files[2])) as im:
        assert im.mode == 'L' and np.array_equal(np.asarray(im), data['lab'][2])
    dirs = [str(tmp_path / 'imitators'), str(tmp_path / 'gt')]
    paths = calculate_region_metrics_given_paths(dirs, str(tmp_path / 'regions'), SIZE, MIN_PIXELS, BATCH, fid=data['inception'],
                                                 lpips=data['lpips'], ssim=True, kid=KID, device=DEV)
    region_keys = [k for k in got if k in ('n', 'psnr', 'mae') or k.split('_')[-1] in R.NAMES]
    assert len(region_keys) == 3 + 2 * 8
    assert paths == {k: got[k] for k in region_keys}
    # a writer without the option is handed no label maps, and asks for none
    w = EvalWriter(str(tmp_path / 'plain'), sav_gt=False, side=SIDE)
    score_model(Model(), batches[:1], Scorer(fid=None, lpips=None, ssim=False, regions=REGION_OPTS), writer=w)
    w.close()
    assert sorted(os.listdir(str(tmp_path / 'plain'))) == ['imitators', 'source']
    # the command line, without any weights: PSNR, MAE and SSIM per region
    capsys.readouterr()
    v = main(['regions'] + dirs + ['--labels', str(tmp_path / 'regions'), '--region-size', str(SIZE), '--region-min-pixels', str(MIN_PIXELS),
                                   '--batch-size', str(BATCH), '--device', DEV])
    printed = dict(line.split(':  ') for line in capsys.readouterr().out.strip().split('\n') if ':  ' in line)
    keys = [k for k in region_keys if k.split('_')[0] in ('n', 'psnr', 'mae', 'ssim')]
    assert sorted(v) == sorted(keys) and v == {k: got[k] for k in keys}
    assert {k: float(x) for k, x in printed.items()} == {k: float(v[k]) for k in keys}
