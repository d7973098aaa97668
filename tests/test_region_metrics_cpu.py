"""The host side of the region scores (hoig_amd/csrc/region_metrics.h through the CPU twins of hoig_amd/metrics/regions.py): equal to
the restatements of tests/region_metrics_reference.py, which the first test pins to a case written out by hand."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

import region_metrics_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_p = lambda a: ctypes.c_void_p(a.ctypes.data)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_the_restatement_on_a_hand_written_case():
    """4 x 5: a 2 x 2 hand at (x 1..2, y 0..1), one object pixel at (4, 3); gen - gt = (1, -2, 3) in the hand, (0, 0, 10) on the object
    pixel and 0 elsewhere."""
    lab = np.array([[[0, 1, 1, 0, 0], [0, 1, 1, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 2]]], np.uint8)
    gt = np.full((1, 4, 5, 3), 100, np.uint8)
    gen = gt.copy()
    gen[0, :2, 1:3] = (101, 98, 103)
    gen[0, 3, 4] = (100, 100, 110)
    bg, hand = (lab == 0).astype(np.float32), (lab != 1).astype(np.float32)
    assert np.array_equal(R.labels_from_masks(bg, hand), lab)
    st, status = R.stats(gen, gt, lab)
    assert status == 0
    assert st[0].tolist() == [[20, 4 * 6 + 10, 4 * 14 + 100, 0, 0, 4, 3, 0], [4, 24, 56, 1, 0, 2, 1, 0], [1, 10, 100, 4, 3, 4, 3, 0]]
    # hand: side0 2, pad 1, side 4 (= H); left = clamp((1 + 2 + 1 - 4) // 2 = 0), top = clamp((0 + 1 + 1 - 4) // 2 = -1 -> 0)
    # object: side0 1, pad 1, side 3; left = clamp((4 + 4 + 1 - 3) // 2 = 3, 0, 5 - 3 = 2) = 2, top = clamp(2, 0, 1) = 1
    assert R.boxes(st, 4, 5, 1).tolist() == [[[0, 0, 4, 1], [2, 1, 3, 1]]]
    assert R.boxes(st, 4, 5, 2).tolist() == [[[0, 0, 4, 1], [0, 0, 0, 0]]]
    psnr, mae = R.psnr_mae(st[0, 1])
    assert mae == 2.0 and psnr == 10.0 * np.log10(255.0 ** 2 * 12 / 56)
    assert R.psnr_mae(np.array([3, 0, 0]))[0] == np.inf
    c = R.crops(gen, R.boxes(st, 4, 5, 2), 4)
    assert c.shape == (2, 1, 4, 4, 3) and np.array_equal(c[0, 0], gen[0, :, :4]) and not c[1].any()
    _, status = R.stats(gen, gt, np.where(lab == 2, 5, lab).astype(np.uint8))
    assert status == (1 | 5 << 8)


@pytest.mark.parametrize('shape', R.STATS_SHAPES, ids=lambda s: '%dx%d' % s)
def test_the_stats_twin_equals_the_restatement(shape):
    from hoig_amd.metrics import regions as G
    gen, gt, lab = R.stats_case(*shape)
    want, want_status = R.stats(gen, gt, lab)
    got, status = G.region_stats(_t(gen), _t(gt), _t(lab))
    assert np.array_equal(got.numpy(), want)
    assert int(status) == want_status == (1 | 3 << 8)
    if shape != (1, 1):
        assert want[0, 2, 0] == 0 and want[0, 2, 3:7].tolist() == [shape[1], shape[0], -1, -1]     # an empty region
        assert want[0, 1, 3:7].tolist() == [0, 0, shape[1] - 1, shape[0] - 1]                     # one on all four borders
        assert want[0, 0, 0] == shape[0] * shape[1] > want[0, 1, 0] + want[0, 2, 0]               # label 3 counts in row 0 only
    assert want[1, 2, 0] == 1                                                                     # a single pixel
    # seven regions: every label is its own row
    lab7 = np.random.default_rng(5).integers(0, 8, size=lab.shape, dtype=np.uint8)
    want, want_status = R.stats(gen, gt, lab7, 7)
    got, status = G.region_stats(_t(gen), _t(gt), _t(lab7), 7)
    assert np.array_equal(got.numpy(), want) and int(status) == want_status == 0


def test_the_box_twin_on_every_extent_of_a_9_by_12_image():
    from hoig_amd.metrics import regions as G
    H, W = 9, 12
    rows = [(x0, y0, x1, y1) for x0, x1 in itertools.combinations_with_replacement(range(W), 2)
            for y0, y1 in itertools.combinations_with_replacement(range(H), 2)]
    st = np.zeros((len(rows), 2, 8), np.int64)
    st[:, 1, 0] = 5
    st[:, 1, 3:7] = rows
    want = R.boxes(st, H, W, 5)
    assert np.array_equal(G.region_boxes(_t(st), H, W, 5).numpy(), want)
    assert want[:, 0, 3].all() and (want[:, 0, 2] <= H).all() and (want[:, 0, 0] + want[:, 0, 2] <= W).all()
    assert (want[:, 0, 1] + want[:, 0, 2] <= H).all() and want[:, 0, :2].min() == 0
    # min_pixels at exactly the count and one above; 0 asks for one pixel
    assert not G.region_boxes(_t(st), H, W, 6).numpy().any()
    st[0, 1, 0] = 0
    got = G.region_boxes(_t(st), H, W, 0).numpy()
    assert not got[0].any() and np.array_equal(got[1:], want[1:])


@pytest.mark.parametrize('shape', [(20, 64), (64, 20)], ids=lambda s: '%dx%d' % s)
def test_the_box_twin_where_the_padded_side_exceeds_the_smaller_dimension(shape):
    from hoig_amd.metrics import regions as G
    H, W = shape
    st = np.zeros((3, 3, 8), np.int64)
    st[:, 1:, 0] = 100
    st[0, 1, 3:7], st[0, 2, 3:7] = (2, 1, 17, 16), (W - 18, H - 18, W - 1, H - 1)       # 16 + 2 * 4 = 24 > 20
    st[1, 1, 3:7], st[1, 2, 3:7] = (0, 0, W - 1, H - 1), (W // 2, H // 2, W // 2, H // 2)
    st[2, 1, 3:7], st[2, 2, 3:7] = (5, 3, 9, 4), (W - 3, 0, W - 1, H - 1)
    want = R.boxes(st, H, W, 64)
    assert want[0, 0, 2] == 20 and want[1, 0, 2] == 20
    assert np.array_equal(G.region_boxes(_t(st), H, W, 64).numpy(), want)


@pytest.mark.parametrize('case', R.CROP_CASES, ids=lambda c: '%dx%d-%d' % (c[0] + (c[1],)))
def test_the_crop_twin_equals_pillow_every_byte(case):
    from hoig_amd.metrics import regions as G
    images, bxs = R.crop_case(case)
    want = R.crops(images, bxs, case[1])
    got = G.region_crops(_t(images), _t(bxs), case[1]).numpy()
    assert got.shape == want.shape == (1, len(case[2]) + 1, case[1], case[1], 3)
    assert np.array_equal(got, want)
    assert want[0, :-1].any() and not got[0, -1].any()                   # the last box is invalid: zeros


def test_the_tables_hold_the_resize_tables_of_every_side():
    from hoig_amd.metrics import kernels as K
    from hoig_amd.metrics import regions as G
    t = G.tables_host(40, 8)
    assert t[0] == 40 and t[1] == 8 and t.dtype == np.int32
    for side in (1, 3, 8, 37, 40):
        one = K.pil_table_host(side, 8)
        off, ksize = t[2 * side], t[2 * side + 1]
        assert ksize == one.shape[1] - 2
        assert np.array_equal(t[off:off + one.size].reshape(one.shape), one)
    assert t[2 * 40] + 8 * (2 + t[2 * 40 + 1]) == t.size


def test_invalid_arguments_are_refused():
    from hoig_amd import _lib as L
    buf = np.zeros(1 << 16, np.uint8)
    p = _p(buf)
    odd = ctypes.c_void_p(buf.ctypes.data + 1)
    stats_h, stats_d = L.lib.hoig_region_stats_u8_host, L.lib.hoig_region_stats_u8
    for N, H, W, Rg in ((1, 0, 8, 2), (1, 8, 4097, 2), (1, 8, 8, 0), (1, 8, 8, 8), (0, 8, 8, 2)):
        assert stats_h(p, p, p, N, H, W, Rg, p, p) == L.EINVAL
        assert stats_d(p, p, p, N, H, W, Rg, p, p, None) == L.EINVAL
        assert L.lib.hoig_region_boxes_host(p, N, H, W, Rg, 1, p) == L.EINVAL
        assert L.lib.hoig_region_boxes(p, N, H, W, Rg, 1, p, None) == L.EINVAL
        assert L.lib.hoig_region_crop_resize_u8_host(p, N, H, W, p, Rg, 8, p) == L.EINVAL
        assert L.lib.hoig_region_crop_resize_u8(p, N, H, W, p, Rg, 8, p, p, p, None) == L.EINVAL
        assert L.lib.hoig_region_crop_workspace_bytes(N, H, W, Rg, 8) == L.EINVAL
    for S in (3, 513):
        assert L.lib.hoig_region_crop_resize_u8_host(p, 1, 8, 8, p, 2, S, p) == L.EINVAL
        assert L.lib.hoig_region_crop_resize_u8(p, 1, 8, 8, p, 2, S, p, p, p, None) == L.EINVAL
        assert L.lib.hoig_region_crop_workspace_bytes(1, 8, 8, 2, S) == L.EINVAL
        assert L.lib.hoig_region_tables_bytes(8, S) == L.EINVAL and L.lib.hoig_region_tables(8, S, p) == L.EINVAL
    assert L.lib.hoig_region_tables_bytes(0, 8) == L.EINVAL and L.lib.hoig_region_tables_bytes(4097, 8) == L.EINVAL
    # misaligned dst / workspace, a NULL pointer: before any launch
    assert L.lib.hoig_region_crop_resize_u8(p, 1, 8, 8, p, 2, 8, p, odd, p, None) == L.EINVAL
    assert L.lib.hoig_region_crop_resize_u8(p, 1, 8, 8, p, 2, 8, p, p, odd, None) == L.EINVAL
    assert L.lib.hoig_region_crop_resize_u8(p, 1, 8, 8, p, 2, 8, None, p, p, None) == L.EINVAL
    assert stats_d(p, p, p, 1, 8, 8, 2, odd, p, None) == L.EINVAL
    assert L.lib.hoig_region_crop_workspace_bytes(2, 5, 7, 2, 6) == 2 * 2 * 92       # 5 * 6 * 3 = 90 bytes, a crop on a word
    # three channels only: the Python layer refuses anything else before it reaches the C ABI, which has no C argument
    from hoig_amd.metrics import regions as G
    with pytest.raises(ValueError):
        G.region_stats(torch.zeros(1, 8, 8, 4, dtype=torch.uint8), torch.zeros(1, 8, 8, 4, dtype=torch.uint8),
                       torch.zeros(1, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError):
        G.region_crops(torch.zeros(1, 8, 8, 4, dtype=torch.uint8), torch.zeros(1, 2, 4, dtype=torch.int32), 8)


def test_options_and_the_scalar_formulas():
    from hoig_amd.metrics import regions as G
    assert G.region_options(None) is None and G.region_options(True) == dict(size=128, min_pixels=64, batch=50)
    assert G.region_options(dict(size=32)) == dict(size=32, min_pixels=64, batch=50)
    for bad in (dict(side=3), dict(size=3), dict(size=513), dict(batch=0), 7):
        with pytest.raises(ValueError):
            G.region_options(bad)
    with pytest.raises(ValueError):
        G.RegionScores(dict(size=8), ssim=True)                           # SSIM's 11-tap window
    G.RegionScores(dict(size=8), ssim=False)
    rows = np.array([[4, 24, 56, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0, 0, 0]], np.int64)
    psnr, mae = G.psnr_mae(rows)
    assert (psnr[0], mae[0]) == R.psnr_mae(rows[0]) and psnr[1] == np.inf and mae[1] == 0.0
    bg, hand = torch.tensor([[1.0, 0.0, 0.0]]), torch.tensor([[1.0, 1.0, 0.0]])
    assert G.labels_from_masks(bg, hand).tolist() == [[0, 2, 1]] == R.labels_from_masks(bg.numpy(), hand.numpy()).tolist()


def test_the_twins_under_a_host_address_sanitizer_build(tmp_path):
    """The statistics, boxes, tables and crops built with -fsanitize=address, every buffer a heap block of exactly its size
    (tests/region_metrics_asan_driver.cpp, a program of its own, no preload): no report, and the bytes of the library's twins."""
    import shutil
    from hoig_amd.metrics import regions as G
    cxx = shutil.which(os.environ.get('CXX', 'c++'))
    flags = ['-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address', '-static-libasan']
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    if cxx is None or subprocess.run([cxx] + flags + [str(probe), '-o', str(tmp_path / 'probe')], stdout=subprocess.DEVNULL,
                                     stderr=subprocess.DEVNULL).returncode != 0:
        pytest.skip('no host C++ compiler that links an AddressSanitizer runtime (an empty program does not build with %s)' % ' '.join(flags))
    exe = str(tmp_path / 'region_metrics_asan_driver')
    src = [os.path.join(ROOT, 'hoig_amd', 'csrc', 'region_metrics_host.cpp'), os.path.join(ROOT, 'tests', 'region_metrics_asan_driver.cpp')]
    build = subprocess.run([cxx] + flags + ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'hoig_amd', 'csrc')] + src +
                           ['-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout

    def fnv(a):
        h = 2166136261
        for v in np.ascontiguousarray(a).view(np.uint8).reshape(-1).tolist():
            h = ((h ^ v) * 16777619) & 0xFFFFFFFF
        return h

    cases = [(3, 1, 1, 4), (2, 5, 7, 6), (3, 33, 65, 8), (2, 40, 52, 11)]
    args, want = [], []
    for n, h, w, s in cases:
        args += [n, h, w, s]
        i = np.arange(n * h * w * 3, dtype=np.uint64)
        gen = (((i * 2654435761 + (h * 31 + w)) & 0xFFFFFFFF) >> 24).astype(np.uint8).reshape(n, h, w, 3)
        gt = (((i * 2654435761 + (h * 31 + w + 7)) & 0xFFFFFFFF) >> 24).astype(np.uint8).reshape(n, h, w, 3)
        k, y, x = np.mgrid[0:n, 0:h, 0:w]
        hand = (x >= w // 8 + k) & (x < w // 2) & (y >= h // 8) & (y < h // 2 + k)
        lab = np.where(hand, 1, np.where((x >= w // 2) & (x < w - k) & (y >= h // 2), 2, 0)).astype(np.uint8)
        st, status = G.region_stats(_t(gen), _t(gt), _t(lab))
        bx = G.region_boxes(st, h, w, 1)
        crops = G.region_crops(_t(gen), bx, s)
        assert np.array_equal(crops.numpy(), R.crops(gen, bx.numpy(), s))
        want.append('0000%d %d %d %d %d' % (int(status), fnv(st.numpy()), fnv(bx.numpy()), fnv(G.tables_host(min(h, w), s)), fnv(crops.numpy())))
    run = subprocess.run([exe] + [str(v) for v in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0 and 'AddressSanitizer' not in run.stdout, run.stdout[-3000:]
    assert run.stdout.split('\n')[:len(want)] == want
