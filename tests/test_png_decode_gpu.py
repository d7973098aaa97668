"""The PNG decoder on the MI355X (hoig_png_decode_u8): every output byte and status word EQUAL to the CPU twin's, which
tests/test_png_decode_cpu.py holds against Pillow and zlib; the same batches against Pillow directly; the directory functions with
device_png_decode=True EQUAL to the default calls."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import metrics_reference as M
import png_decode_reference as G
import png_reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def both(plans, bgr=False):
    got, status = G.decode_device(plans, bgr)
    want, want_status = G.decode_host(plans, bgr)
    assert status == want_status, [G.D().status_text(s) for s in status]
    for i, (g, w, s) in enumerate(zip(got, want, status)):
        if s == 0:
            assert np.array_equal(g, w), i
    return got, status


@pytest.mark.parametrize('bgr', [False, True])
def test_a_mixed_batch_equals_the_twin_and_pillow(bgr):
    files = G.mixed_batch_files()
    plans = [G.plan_of(f) for f in files]
    assert {(p.color_type, p.bit_depth) for p in plans} == {(c, d) for c, d, _ in G.KINDS}
    assert max(p.width * p.height for p in plans) == 255 * 257
    got, status = both(plans, bgr)
    assert status == [0] * len(plans)
    for g, f in zip(got, files):
        want = G.pillow_rgb(f)
        assert np.array_equal(g, want[..., ::-1] if bgr else want)


def test_four_images_at_the_workload_shape_wrap_the_window():
    files = [G.save(Image.fromarray(R.content(k, 256, 256, 3, seed=3))) for k in ('noise55', 'smooth', 'rect')]
    files.append(dict(G.own_files())['own-noise55-256x256x3'])
    plans = [G.plan_of(f) for f in files]
    assert all(p.filtered_bytes > 32768 for p in plans)
    got, status = both(plans)
    assert status == [0] * 4
    for g, f in zip(got, files):
        assert np.array_equal(g, G.pillow_rgb(f))


def test_the_workspace_window_gives_the_same_bytes():
    """tuning key png_window = 1: matches read the filtered stream in the workspace instead of the LDS ring"""
    L = R.lib()
    prev = L.set_tuning('png_window', 1)
    try:
        assert prev == 0                                       # the ring is the default
        test_four_images_at_the_workload_shape_wrap_the_window()
        test_crafted_streams_as_images()
        test_bad_streams_between_good_images()
    finally:
        L.set_tuning('png_window', prev)


@pytest.mark.parametrize('size', [(1, 1), (7, 1)], ids=lambda s: '%dx%d' % s)
def test_a_single_small_image(size):
    for name, f in G.pillow_files(sizes=(size,), settings=[{'compress_level': 6}]):
        (got,), (status,) = both([G.plan_of(f)])
        assert status == 0 and np.array_equal(got, G.pillow_rgb(f)), name


def test_crafted_streams_as_images():
    """the token writer's edge cases as one-row grey images: every match length at the short distances, the longest distances, token
    lists that wrap, far matches between literals"""
    P = G.D().Plan
    streams = []
    head = np.random.RandomState(3).randint(0, 256, 70).astype(np.uint8).tobytes()
    for dist in (1, 2, 3, 63, 64, 65):
        t = G.FixedTokens()
        t.literal(0)
        t.literals(head)
        for length in range(3, 259):
            t.match(length, dist)
            t.literal(length & 255)
        streams.append(t)
    for dist in (32767, 32768):
        t = G.FixedTokens()
        t.literal(0)
        t.literals(np.random.RandomState(dist).randint(0, 256, 32768).astype(np.uint8).tobytes())
        for length in (3, 64, 65, 258, 17):
            t.match(length, dist)
        t.match(258, dist)
        streams.append(t)
    t = G.FixedTokens()
    t.literals(b'\x00bc')
    for _ in range(200):
        t.match(3, 3)
    streams.append(t)
    t = G.FixedTokens()
    t.literal(0)
    t.literals(np.random.RandomState(9).randint(0, 256, 20000).astype(np.uint8).tobytes())
    for k in range(150):
        t.match(3 + k, 16257 + 20 * k)
        t.literal(k)
    streams.append(t)
    plans = [P(len(t.expected) - 1, 1, 0, 8, t.stream(), None) for t in streams]
    got, status = both(plans)
    assert status == [0] * len(plans)
    for g, t in zip(got, streams):
        assert g[0, :, 0].tobytes() == bytes(t.expected[1:])


def test_bad_streams_between_good_images():
    bad = G.bad_plans()
    good = [f for _, f in G.hand_filtered_files()[:len(bad)]]
    plans, want = [], []
    for (name, plan, bit), f in zip(bad, good):
        plans += [plan, G.plan_of(f)]
        want += [bit, 0]
    _, host_status = G.decode_host(plans)
    assert host_status == want                                 # the twin first
    got, status = both(plans)                                   # device == twin, guard bands inside
    assert status == want, [G.D().status_text(s) for s in status]
    for g, f in zip(got[1::2], good):
        assert np.array_equal(g, G.pillow_rgb(f))


def test_the_python_wrapper_and_a_side_stream_with_its_input_uploaded_there():
    D = G.D()
    files = [f for _, f in G.pillow_files(sizes=((64, 48),), settings=[{'compress_level': 6}])]
    want = np.stack([G.pillow_rgb(f) for f in files])
    got = D.decode_u8(files, DEV)
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(D.decode_u8(files, DEV, bgr=True).cpu().numpy(), want[..., ::-1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = D.decode_u8(files, DEV)                          # the bytes and the plans are uploaded on `side`, then the launches
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    name, plan, bit = G.bad_plans()[0]
    with pytest.raises(ValueError, match=D.status_text(bit)):
        D.decode_u8([G.png_file(plan.width, plan.height, 8, 0, plan.stream)], DEV)


# ---- end to end on directories

@pytest.fixture(scope='module')
def dirs(tmp_path_factory):
    """two directories of 6 Pillow-written PNGs at 64 x 48; one file of the first is 16-bit (the host route inside a device batch)"""
    root = tmp_path_factory.mktemp('png_decode_dirs')
    out = []
    for d, seed in (('gen', 30), ('gt', 31)):
        os.makedirs(str(root / d))
        for i in range(6):
            img = R.content('noise55', 48, 64, 3, seed=seed * 10 + i)
            name = str(root / d / ('%04d.png' % i))
            if d == 'gen' and i == 2:
                Image.fromarray((img[..., 0].astype(np.uint16) * 257)).save(name)
            else:
                Image.fromarray(img).save(name)
        out.append(str(root / d))
    return out


def count_opens(monkeypatch):
    seen = []
    real = Image.open

    def counting(fp, *a, **kw):
        seen.append(str(fp))
        return real(fp, *a, **kw)

    monkeypatch.setattr(Image, 'open', counting)
    return seen


def test_ssim_on_directories_equals_the_default_and_opens_no_supported_file(dirs, monkeypatch):
    from hoig_amd.metrics.ssim import calculate_ssim_given_paths
    monkeypatch.delenv('HOIG_DEVICE_PNG_DECODE', raising=False)
    want = calculate_ssim_given_paths(dirs, 256, 4, DEV)
    seen = count_opens(monkeypatch)
    got = calculate_ssim_given_paths(dirs, 256, 4, DEV, device_png_decode=True)
    print(got, want)
    assert got == want
    assert [os.path.basename(s) for s in seen] == ['0002.png'] and os.path.dirname(seen[0]) == dirs[0]     # the 16-bit file alone
    del seen[:]
    monkeypatch.setenv('HOIG_DEVICE_PNG_DECODE', '1')
    assert calculate_ssim_given_paths(dirs, 256, 4, DEV) == want and len(seen) == 1
    del seen[:]
    assert calculate_ssim_given_paths(dirs, 256, 4, DEV, device_png_decode=False) == want and len(seen) == 12


def test_the_command_line_flag_in_a_fresh_process(dirs):
    env = {k: v for k, v in os.environ.items() if k != 'HOIG_DEVICE_PNG_DECODE'}
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    outs = []
    for flag in ([], ['--device-png-decode']):
        run = subprocess.run([sys.executable, '-m', 'hoig_amd.metrics', 'ssim'] + dirs + ['--batch-size', '4'] + flag, env=env, cwd=ROOT,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert run.returncode == 0, run.stdout[-3000:]
        outs.append([line for line in run.stdout.split('\n') if line.startswith('SSIM')])
    assert outs[0] == outs[1] and len(outs[0]) == 1


def test_lpips_and_fid_features_equal_the_default_on_seeded_weights(tmp_path, monkeypatch):
    from hoig_amd.metrics import images as I
    from hoig_amd.metrics.fid import InceptionFeatures, get_activations
    from hoig_amd.metrics.lpips import LPIPS, calculate_lpips_given_paths
    monkeypatch.delenv('HOIG_DEVICE_PNG_DECODE', raising=False)
    a, b = str(tmp_path / 'gen'), str(tmp_path / 'gt')
    M.write_pngs(a, 4, 64, 40), M.write_pngs(b, 4, 64, 41)
    lp = LPIPS(M.alexnet_state_dict(1), M.lpips_state_dict(2), precision='f32', device=DEV)
    want = calculate_lpips_given_paths([a, b], 256, 3, model=lp)
    seen = count_opens(monkeypatch)
    got = calculate_lpips_given_paths([a, b], 256, 3, model=lp, device_png_decode=True)
    print(got, want)
    assert got == want and seen == []
    inc = InceptionFeatures(M.inception_state_dict(5), 64, None, DEV)
    files = I.list_images(a)
    want = get_activations(files, inc, 3, 64)
    del seen[:]
    got = get_activations(files, inc, 3, 64, device_png_decode=True)
    assert np.array_equal(got, want) and seen == []
