"""SURVEY 8f row 4, CPU side: the loader's oracle (oracle/data_oracle.py -- parity UNPINNED for the OpenCV primitives: opencv-python
4.5.1.48 is not installed and the reference holds no vectors for its loader) against known answers that any correct restatement of
cv2.warpAffine / cv2.resize / cv2.Rodrigues / cv2.getAffineTransform must reproduce, the package's host geometry against the oracle,
and HOv3Dataset's host half on a synthetic directory tree."""
import numpy as np
import pytest
import torch

import data_fixture as FX
from oracle import data_oracle as O


def _img(h, w, c=3, seed=0):
    return np.random.Generator(np.random.Philox(key=[seed, h * w])).integers(0, 256, (h, w, c)).astype(np.uint8)


def test_warp_identity_and_integer_shift_copy_pixels():
    a = _img(19, 23)
    eye = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
    assert np.array_equal(O.warp_affine_linear_u8(a, eye, (23, 19)), a)
    sh = O.warp_affine_linear_u8(a, np.array([[1, 0, 3], [0, 1, -2]], np.float32), (23, 19))        # dst(x, y) = src(x - 3, y + 2)
    want = np.zeros_like(a)
    want[:17, 3:] = a[2:, :20]
    assert np.array_equal(sh, want)
    # a larger canvas: everything outside the source is the constant border 0
    big = O.warp_affine_linear_u8(a, np.array([[1, 0, 5], [0, 1, 4]], np.float32), (40, 30))
    assert np.array_equal(big[4:23, 5:28], a) and big[:4].max() == 0 and big[:, :5].max() == 0 and big[23:].max() == 0


def test_warp_half_pixel_blends_two_neighbours_with_round_half_up():
    a = _img(6, 9, 1, seed=3)
    out = O.warp_affine_linear_u8(a, np.array([[2, 0, 0], [0, 1, 0]], np.float32), (17, 6))           # dst(x) = src(x / 2)
    assert np.array_equal(out[:, 0:17:2, 0], a[:, :, 0])
    mid = (a[:, :-1, 0].astype(int) + a[:, 1:, 0] + 1) >> 1                                             # weights 1/2, 1/2: (a + b + 1) >> 1
    assert np.array_equal(out[:, 1:16:2, 0], mid)
    # a quarter-pixel shift: src x = dst x - 0.25 -> weights 1/4 on the left neighbour, 3/4 on the pixel itself
    q = O.warp_affine_linear_u8(a, np.array([[1, 0, 0.25], [0, 1, 0]], np.float32), (9, 6))
    want = (a[:, :-1, 0].astype(int) * 8 + a[:, 1:, 0].astype(int) * 24 + 16) >> 5
    assert np.array_equal(q[:, 1:, 0], want)
    assert np.array_equal(q[:, 0, 0], (a[:, 0, 0].astype(int) * 24 + 16) >> 5)                          # left neighbour = border 0


def test_resize_known_answers():
    a = _img(12, 16)
    assert np.array_equal(O.resize_linear_u8(a, (16, 12)), a)
    const = np.full((5, 7, 3), 201, np.uint8)
    assert np.array_equal(O.resize_linear_u8(const, (14, 10)), np.full((10, 14, 3), 201, np.uint8))
    # 2x along x only: out[2k] = (s[k-1] + 3 s[k] + 2) >> 2, out[2k+1] = (3 s[k] + s[k+1] + 2) >> 2 (edges replicate)
    row = _img(1, 9, 1, seed=5)
    up = O.resize_linear_u8(np.repeat(row, 3, axis=0), (18, 3))[1, :, 0].astype(int)
    s = row[0, :, 0].astype(int)
    sp = np.concatenate([s[:1], s, s[-1:]])
    assert np.array_equal(up[0::2], (sp[:-2] + 3 * s + 2) >> 2) and np.array_equal(up[1::2], (3 * s + sp[2:] + 2) >> 2)
    # against a float bilinear with the same sampling grid, everywhere within one grey level
    b = _img(24, 32, 3, seed=7)
    got = O.resize_linear_u8(b, (64, 48)).astype(float)
    ys = np.clip((np.arange(48) + 0.5) * 0.5 - 0.5, 0, 23); xs = np.clip((np.arange(64) + 0.5) * 0.5 - 0.5, 0, 31)
    y0, x0 = np.floor(ys).astype(int), np.floor(xs).astype(int)
    y1, x1 = np.minimum(y0 + 1, 23), np.minimum(x0 + 1, 31)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    bf = b.astype(float)
    ref = (bf[y0][:, x0] * (1 - fx) + bf[y0][:, x1] * fx) * (1 - fy) + (bf[y1][:, x0] * (1 - fx) + bf[y1][:, x1] * fx) * fy
    assert np.abs(got - ref).max() <= 1.0


def test_rodrigues_and_affine_known_answers():
    r = O.rodrigues(np.array([0, 0, np.pi / 2]))
    assert np.allclose(r, [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    assert np.array_equal(O.rodrigues(np.zeros((3, 1))), np.eye(3))
    g = np.random.Generator(np.random.Philox(key=[1, 2]))
    for _ in range(20):
        v = g.uniform(-2, 2, 3)
        R = O.rodrigues(v)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(R) - 1) < 1e-14
        assert np.allclose(R @ v, v, atol=1e-14)                                   # the axis is fixed
        assert O.rodrigues(v.astype(np.float32)).dtype == np.float32
    src = np.float32([[10, 20], [10, 70], [90, 20]]); dst = np.float32([[128, 128], [128, 256], [256, 128]])
    m = O.get_affine_transform(src, dst)
    assert np.allclose(m, [[1.6, 0, 112], [0, 2.56, 76.8]], atol=1e-12)
    for p, q in zip(src, dst):
        assert np.allclose(m @ [p[0], p[1], 1], q, atol=1e-10)
    verts = O.read_obj_vertices('# c\nv 1 2 3\nvn 0 0 1\nv -0.5 1e-3 7 0.1\nf 1 2 1\n\nvt 0 0\n')
    assert verts.dtype == np.float64 and np.array_equal(verts, [[1, 2, 3], [-0.5, 1e-3, 7]])


def test_host_geometry_matches_the_oracle():
    from hoig_amd.data import geometry as G
    g = np.random.Generator(np.random.Philox(key=[3, 4]))
    for _ in range(200):
        bbox = [g.uniform(0, 400), g.uniform(0, 300), g.uniform(50, 400), g.uniform(50, 400)]
        assert np.array_equal(G.patch_transform(bbox), O.patch_transform(bbox))
        v = g.uniform(-3, 3, (3, 1))
        assert np.array_equal(G.rodrigues(v), O.rodrigues(v)) and np.array_equal(G.rodrigues(v.astype(np.float32)), O.rodrigues(v.astype(np.float32)))


def test_dataset_host_half_on_a_synthetic_tree(tmp_path):
    from hoig_amd.data import DatasetFactory
    from hoig_amd.data.device_stage import collate_raw
    opt = FX.build(str(tmp_path), seed=2)
    ds = DatasetFactory.get_by_name('hov3', opt, True)
    assert ds.name == 'HOv3Dataset' and len(ds) == 2
    np.random.seed(0)
    rec = ds[1]
    a, b = rec['A'], rec['B']
    assert a['name'].startswith('MC2_0/') and b['name'].startswith('MC2_0/') and a['name'] != b['name']      # two frames of one video
    assert a['frame'].shape == (480, 640, 3) and a['frame'].dtype == torch.uint8 and a['mask'].shape == (240, 320, 3)
    assert a['objName'] == 5 and a['pose'].dtype == torch.float32 and a['obj_rot'].dtype == torch.float64
    FX.write_pairs(opt, [('ABF1_0/0001.png', 'MC2_0/0003.png'), ('MC2_0/0000.png', 'ABF1_0/0002.png'), ('ABF1_0/0000.png', 'ABF1_0/0003.png')])
    ds = DatasetFactory.get_by_name('hov3', opt, True)
    assert len(ds) == 3 and ds[0]['A']['name'] == 'ABF1_0/0001.png' and ds[0]['B']['name'] == 'MC2_0/0003.png' and ds[4]['A']['name'] == 'MC2_0/0000.png'
    raw = collate_raw([ds[0], ds[1]])
    assert raw['A']['frame'].shape == (2, 480, 640, 3) and raw['B']['objName'] == [5, 2] and raw['A']['bbox'].shape == (2, 4)
    # the decoded frame is what is on disk, in cv2.imread's channel order
    from PIL import Image
    disk = np.asarray(Image.open(str(tmp_path / 'images/train/ABF1/rgb/0001.png')))
    assert np.array_equal(raw['A']['frame'][0].numpy(), disk[:, :, ::-1])
    # and the oracle makes a plausible sample of it
    (va, vb) = FX.oracle_batch(opt, ['ABF1_0/0001.png'], ['MC2_0/0003.png'])
    assert va['image'].shape == (1, 3, 256, 256) and -1.0 <= va['image'].min() and va['image'].max() <= 1.0
    assert set(np.unique(va['mask'])) <= set((np.arange(256) / 128.0).astype(np.float32)) and va['mask'].max() > 1.9
    assert np.count_nonzero(vb['vertices_obj'][0].any(axis=1)) == 50 + 7 * 5
    with pytest.raises(ValueError):
        DatasetFactory.get_by_name('nope', opt, True)


def test_ycb_dataset_host_half_on_a_synthetic_tree(tmp_path):
    """The HOIG_DexYCB copy's loader (ycb_dataset.py:230-305): corner-form boxes, label files, the grasped object's pose indexed among
    the non-zero poses."""
    from hoig_amd.data import DatasetFactory
    from hoig_amd.data.device_stage import collate_raw
    opt = FX.build_ycb(str(tmp_path), seed=3)
    ds = DatasetFactory.get_by_name('ycb', opt, True)
    assert ds.name == 'YCBDataset' and len(ds) == 2
    v0, v1 = '20200709-subject-01/20200709_141754/836212060125', '20200813-subject-02/20200813_145612/932122062010'
    FX.write_pairs(opt, [(v0 + '/1', v1 + '/2'), (v1 + '/0', v0 + '/2')])
    ds = DatasetFactory.get_by_name('ycb', opt, True)
    rec = ds[0]
    a, b = rec['A'], rec['B']
    assert a['name'] == v0 + '/1' and b['name'] == v1 + '/2' and 'mask' not in a
    assert a['frame'].shape == (480, 640, 3) and a['cam'].shape == (4,) and a['pose'].shape == (51,) and a['shape'].shape == (10,)
    assert a['objName'] == FX.YCB_NAMES.index('019_pitcher_base') and b['objName'] == FX.YCB_NAMES.index('008_pudding_box')
    import pickle, os
    bb = pickle.load(open(os.path.join(str(tmp_path), 'params', 'DexYCB-bbx.pkl'), 'rb'))[v0]
    assert np.allclose(a['bbox'].numpy(), [bb[0], bb[1], bb[2] - bb[0], bb[3] - bb[1]])
    # video 0: ycb_grasp_ind = 1, but the pose in front of it is all zero -> the reference's list of non-zero poses is indexed with 1,
    # i.e. it takes the THIRD object's pose (ycb_dataset.py:155-168)
    label = np.load(os.path.join(str(tmp_path), 'images', v0, 'labels_000001.npz'))
    assert np.array_equal(a['obj_pose'][:3].numpy(), label['pose_y'][2].astype(np.float64)) and a['obj_pose'][3].tolist() == [0, 0, 0, 1]
    raw = collate_raw([ds[0], ds[1]])
    assert raw['A']['frame'].shape == (2, 480, 640, 3) and raw['A']['obj_pose'].shape == (2, 4, 4)
    want = FX.oracle_batch_ycb(opt, [v0 + '/1'])
    assert want['image'].shape == (1, 3, 256, 256) and np.count_nonzero(want['vertices_obj'][0].any(axis=1)) == 40 + 3 * 11


def test_loader_host_half_runs_without_a_gpu(tmp_path):
    """CustomDatasetDataLoader.load_raw_data(): worker processes decode and collate; nothing touches a device."""
    from hoig_amd.data import CustomDatasetDataLoader
    opt = FX.build(str(tmp_path), seed=4)
    pairs = [('ABF1_0/0001.png', 'MC2_0/0003.png'), ('MC2_0/0000.png', 'ABF1_0/0002.png'), ('ABF1_0/0000.png', 'ABF1_0/0003.png')]
    FX.write_pairs(opt, pairs)
    opt.n_threads_train = 2
    loader = CustomDatasetDataLoader(opt, is_for_train=True)
    assert len(loader) == 3 and loader.load_sampler() is None
    raws = list(loader.load_raw_data())
    assert [r['A']['frame'].shape[0] for r in raws] == [2, 1]
    assert [n for r in raws for n in r['A']['name']] == [p[0] for p in pairs]
    assert raws[0]['A']['frame'].dtype == torch.uint8 and raws[0]['B']['mask'].shape == (2, 240, 320, 3)


def test_random_pairs_follow_numpys_global_generator(tmp_path):
    """Without a pairs file sample i is video i mod n and two distinct frames drawn with np.random.choice (hov3_dataset.py:199-203):
    a seeded run visits the reference's pairs."""
    from hoig_amd.data import DatasetFactory
    opt = FX.build(str(tmp_path), seed=6)
    opt.num_repeats = 3
    ds = DatasetFactory.get_by_name('hov3', opt, True)
    assert len(ds) == 2 * 3
    np.random.seed(11)
    recs = [ds[i] for i in (0, 1, 5)]
    got = [(r['A']['name'], r['B']['name']) for r in recs]
    np.random.seed(11)
    frames = ['%04d.png' % k for k in range(4)]
    for (a, b), vid in zip(got, ('ABF1_0', 'MC2_0', 'MC2_0')):
        fa, fb = np.random.choice(frames, size=2, replace=False)
        assert (a, b) == ('%s/%s' % (vid, fa), '%s/%s' % (vid, fb)) and fa != fb


def test_missing_directories_and_files_are_named(tmp_path):
    from hoig_amd.data import DatasetFactory
    opt = FX.build(str(tmp_path), seed=7)
    opt.params_dir = 'nowhere'
    with pytest.raises(ValueError, match='param_dir'):
        DatasetFactory.get_by_name('hov3', opt, True)
    opt.params_dir, opt.images_dir = 'params', 'nowhere'
    with pytest.raises(ValueError, match='pic_dir'):
        DatasetFactory.get_by_name('hov3', opt, True)


def test_imread_follows_cv2_conventions(tmp_path):
    """imread_bgr = cv2.imread(IMREAD_COLOR): BGR order, EXIF orientation applied, 16-bit samples reduced to their high byte, alpha
    dropped, grey widened to three channels."""
    from PIL import Image
    from hoig_amd.data.hov3_dataset import imread_bgr
    rgb = _img(5, 7, 3, seed=9)
    Image.fromarray(rgb).save(tmp_path / 'a.png')
    assert np.array_equal(imread_bgr(str(tmp_path / 'a.png')), rgb[:, :, ::-1])
    exif = Image.Exif()
    exif[0x0112] = 6                                         # "rotate 90 degrees clockwise to display"
    Image.fromarray(rgb).save(tmp_path / 'r.png', exif=exif)
    assert np.array_equal(imread_bgr(str(tmp_path / 'r.png')), np.rot90(rgb, -1)[:, :, ::-1])
    g16 = np.random.Generator(np.random.Philox(key=[1, 2])).integers(0, 65536, (4, 6)).astype(np.uint16)
    Image.fromarray(g16).save(tmp_path / 'g.png')
    out = imread_bgr(str(tmp_path / 'g.png'))
    assert out.shape == (4, 6, 3) and np.array_equal(out[:, :, 0], (g16 >> 8).astype(np.uint8)) and np.array_equal(out[:, :, 0], out[:, :, 2])
    rgba = np.dstack([rgb, np.full((5, 7), 17, np.uint8)])
    Image.fromarray(rgba).save(tmp_path / 't.png')
    assert np.array_equal(imread_bgr(str(tmp_path / 't.png')), rgb[:, :, ::-1])
    Image.fromarray(rgb[:, :, 0]).save(tmp_path / 'l.png')
    assert np.array_equal(imread_bgr(str(tmp_path / 'l.png')), np.repeat(rgb[:, :, :1], 3, axis=2))


def test_imread_matches_cv2_when_available(tmp_path):
    """The decode itself (libjpeg through Pillow vs through OpenCV) and the OpenCV restatements can only be compared where cv2 exists;
    this image has none, so the test documents the gap instead of hiding it."""
    cv2 = pytest.importorskip('cv2')
    from PIL import Image
    from hoig_amd.data.hov3_dataset import imread_bgr
    yy, xx = np.mgrid[0:96, 0:128]
    img = (np.stack([xx * 1.7 + yy, yy * 2.1, (xx + yy) * 0.9], -1) % 256).astype(np.uint8)
    Image.fromarray(img).save(tmp_path / 'j.jpg', quality=90)
    Image.fromarray(img).save(tmp_path / 'p.png')
    for n in ('j.jpg', 'p.png'):
        assert np.array_equal(imread_bgr(str(tmp_path / n)), cv2.imread(str(tmp_path / n))), n
    a = _img(48, 64)
    m = np.array([[0.9, 0.1, 3.3], [-0.2, 1.1, 2.7]], np.float32)
    assert np.array_equal(O.warp_affine_linear_u8(a, m, (40, 30)), cv2.warpAffine(a, m, (40, 30)))
    assert np.array_equal(O.resize_linear_u8(a, (100, 70)), cv2.resize(a, (100, 70)))


def test_host_files_are_not_the_references(tmp_path):
    """the loader's host half keeps the reference's NAMES; its bodies are this package's own.  No file of hoig_amd/data shares
    more than a quarter of its non-trivial lines with a file of the reference's data packages (compared through the line digests of
    tests/golden/reference_data_lines.npz, made by tests/golden/make_golden_live_pins.py data_lines)."""
    import glob
    import os
    from common import line_digests, load_golden
    g = load_golden('reference_data_lines.npz')
    ref_lines = [set(g[k].tolist()) for k in g.files]
    assert len(ref_lines) >= 2 and all(ref_lines)
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'hoig_amd', 'data')
    for f in glob.glob(os.path.join(root, '*.py')):
        mine = line_digests(f).tolist()
        share = max(sum(1 for l in mine if l in r) for r in ref_lines) / max(1, len(mine))
        assert share <= 0.25, (f, share)
