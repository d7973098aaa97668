"""The device JPEG decoder's host side (hoig_amd/data/jpeg.py, hoig_amd/csrc/jpeg_entropy.h through its CPU twin
hoig_jpeg_entropy_host) and the loader option that feeds it.

The reference is tests/jpeg_reference.py, a numpy restatement of the decode Pillow (libjpeg-turbo) performs; the first test here pins
THAT to Pillow, every byte, over 13 sizes x 6 modes x 4 qualities = 312 encodings, so that "equal to the restatement" means "equal to
Pillow" everywhere else (tests/test_jpeg_gpu.py compares the device with Pillow directly as well)."""
import contextlib
import ctypes
import functools
import io
import mmap
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import data_fixture as FX
import jpeg_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_p = lambda a: ctypes.c_void_p(a.ctypes.data)


@functools.lru_cache(maxsize=None)
def case(w, h, mode, quality):
    """-> (file bytes, reference info, reference coefficients)"""
    data = R.encode(R.content(w, h, 1 + quality % 7), mode, quality)
    info, coefs = R.decode_coefficients(data)
    return data, info, coefs


def grid(sizes=R.SIZES, modes=R.MODES, qualities=R.QUALITIES):
    return [(w, h, m, q) for (w, h) in sizes for m in modes for q in qualities]


def host_entropy(files):
    """[(bytes, plan)] -> (packed bytes, plan records with the workspace laid out, intervals, workspace uint8, status int32) after
    hoig_jpeg_entropy_host."""
    from hoig_amd import _lib as L
    from hoig_amd.data import jpeg as J
    buf, plans, ivs = J.pack(files)
    size = L.lib.hoig_jpeg_decode_workspace_bytes(_p(plans), len(files))
    assert size > 0, size
    work = np.full(size, 0x5A, np.uint8)               # (not zero: a block the decoder skips would show)
    status = np.full(len(files), -1, np.int32)
    rc = L.lib.hoig_jpeg_entropy_host(_p(buf), buf.size, _p(plans), len(files), _p(ivs), ivs.size, _p(work), work.size, _p(status))
    assert rc == 0, rc
    return buf, plans, ivs, work, status


def flat(coefs):
    return np.concatenate([c.reshape(-1) for c in coefs])


@pytest.mark.parametrize('mode', R.MODES)
def test_the_restatement_equals_pillow_every_byte(mode):
    for w, h, m, q in grid(modes=[mode]):
        data, info, coefs = case(w, h, m, q)
        assert np.array_equal(R.reconstruct(info, coefs), R.pillow_bgr(data)), (w, h, m, q)


def test_the_grid_reaches_the_special_cases():
    """What the grid is there for: chroma planes of width <= 2 (replicated) and just above (filtered), odd sizes whose last chroma
    column / row is half used, restart intervals, optimised tables, 16-bit-free baseline tables at quality 100."""
    from hoig_amd.data import jpeg as J
    assert J.parse(case(3, 9, '420', 75)[0])['hs'] == 2 and -(-3 // 2) <= 2 < -(-5 // 2)
    assert J.parse(case(640, 480, 'restart', 75)[0])['restart_interval'] > 0
    assert len(J.parse(case(640, 480, 'restart', 75)[0])['intervals']) > 100
    std, opt = J.parse(case(48, 64, '420', 75)[0]), J.parse(case(48, 64, 'optimize', 75)[0])
    assert not np.array_equal(std['ac_counts'], opt['ac_counts'])
    assert J.parse(case(17, 23, 'grey', 75)[0])['ncomp'] == 1


@pytest.mark.parametrize('mode', R.MODES)
def test_the_host_twin_gives_the_restatements_coefficients(mode):
    from hoig_amd.data import jpeg as J
    for w, h, m, q in grid(modes=[mode]):
        data, info, coefs = case(w, h, m, q)
        plan = J.parse(data)
        assert plan is not None, (w, h, m, q)
        assert (plan['width'], plan['height'], plan['ncomp']) == (w, h, len(info['comps']))
        _, plans, _, work, status = host_entropy([(data, plan)])
        want = flat(coefs)
        assert status[0] == 0, (w, h, m, q, J.status_text(int(status[0])))
        assert plans[0]['coef_off'] == 0 and plans[0]['plane_off'] == want.size * 2
        assert np.array_equal(work[:want.size * 2].view(np.int16), want), (w, h, m, q)
        assert (work[want.size * 2:] == 0x5A).all()                     # nothing written behind the coefficients


def test_the_host_twin_takes_a_batch_of_different_sizes():
    from hoig_amd.data import jpeg as J
    cases = [case(17, 23, '420', 75), case(48, 64, 'restart', 95), case(9, 3, 'grey', 30), case(33, 50, '422', 100)]
    _, plans, _, work, status = host_entropy([(c[0], J.parse(c[0])) for c in cases])
    assert not status.any()
    for rec, (_, _, coefs) in zip(plans, cases):
        want = flat(coefs)
        assert np.array_equal(work[rec['coef_off']:rec['coef_off'] + want.size * 2].view(np.int16), want)


# ---- files outside the supported set
def _jpeg(img, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'JPEG', **kw)
    return buf.getvalue()


def _edit(data, at, new):
    return data[:at] + bytes(new) + data[at + len(new):]


def unsupported_files():
    from PIL import Image
    img = R.content(40, 31, 3)
    base = _jpeg(img, quality=85, subsampling=2)
    sof = base.index(b'\xff\xc0')
    sos = base.index(b'\xff\xda')
    exif = Image.Exif()
    exif[0x0112] = 6
    cmyk = io.BytesIO()
    Image.fromarray(np.dstack([img, img[:, :, :1]]), 'CMYK').save(cmyk, 'JPEG')
    first_component_only = base[:sos] + b'\xff\xda\x00\x08\x01' + base[sos + 5:sos + 7] + b'\x00\x3f\x00' + base[sos + 14:]
    return {
        'progressive (written by Pillow)': _jpeg(img, quality=85, progressive=True),
        'arithmetic coding (SOF9: marker edited)': _edit(base, sof + 1, [0xC9]),
        '12-bit samples (precision byte edited)': _edit(base, sof + 4, [12]),
        'four components (CMYK, written by Pillow)': cmyk.getvalue(),
        'a scan of one component out of three (scan header rewritten)': first_component_only,
        'a second scan behind the first (EOI replaced by SOS)': base[:-2] + b'\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00\xff\xd9',
        'sampling 4:1:1 (factor byte edited)': _edit(base, sof + 11, [0x41]),
        'sampling 4:4:0 (factor byte edited)': _edit(base, sof + 11, [0x12]),
        'Adobe transform 0, RGB (written by Pillow, keep_rgb)': _jpeg(img, quality=85, keep_rgb=True),
        'EXIF orientation 6 (written by Pillow)': _jpeg(img, quality=85, exif=exif),
        'fill bytes in front of EOI (an FF inserted)': base[:-2] + b'\xff' + base[-2:],
        'not a JPEG': b'\x89PNG\r\n\x1a\n' + bytes(40),
        'cut inside the headers': base[:sof + 6],
    }


def test_parse_declines_everything_outside_the_supported_set():
    from hoig_amd.data import jpeg as J
    img = R.content(40, 31, 3)
    assert J.parse(_jpeg(img, quality=85, subsampling=2)) is not None
    files = unsupported_files()
    assert b'Adobe' in files['Adobe transform 0, RGB (written by Pillow, keep_rgb)']
    for what, data in files.items():
        assert J.parse(data) is None, what
    # EXIF orientation 1 and an Adobe marker that says YCbCr are inside
    from PIL import Image
    exif = Image.Exif()
    exif[0x0112] = 1
    data = _jpeg(img, quality=85, exif=exif)
    assert b'Exif' in data and J.parse(data) is not None
    assert np.array_equal(R.decode_bgr(data), R.pillow_bgr(data))


# ---- corrupt streams through the host twin
PAGE = mmap.PAGESIZE


@contextlib.contextmanager
def at_the_end_of_an_allocation(data):
    """`data` placed so that its last byte is the last byte of a mapping whose next page is inaccessible: a read one byte past the
    stream ends the process (which is how this test fails)."""
    libc = ctypes.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    pages = -(-len(data) // PAGE)
    mm = mmap.mmap(-1, (pages + 1) * PAGE)
    anchor = ctypes.c_char.from_buffer(mm)
    base = ctypes.addressof(anchor)
    start = pages * PAGE - len(data)
    mm[start:start + len(data)] = data
    assert libc.mprotect(base + pages * PAGE, PAGE, 0) == 0, os.strerror(ctypes.get_errno())
    try:
        yield base + start
    finally:
        libc.mprotect(base + pages * PAGE, PAGE, 3)
        del anchor
        mm.close()


def host_status(data, plan):
    """hoig_jpeg_entropy_host on one file that sits at the end of an allocation -> its status word"""
    from hoig_amd import _lib as L
    from hoig_amd.data import jpeg as J
    _, plans, ivs = J.pack([(data, plan)])
    size = L.lib.hoig_jpeg_decode_workspace_bytes(_p(plans), 1)
    assert size > 0
    work, status = np.zeros(size, np.uint8), np.full(1, -1, np.int32)
    with at_the_end_of_an_allocation(data) as addr:
        rc = L.lib.hoig_jpeg_entropy_host(ctypes.c_void_p(addr), len(data), _p(plans), 1, _p(ivs), ivs.size, _p(work), work.size, _p(status))
    assert rc == 0, rc
    return int(status[0])


def corrupt_streams():
    """-> [(what, bytes, must the status be an error whatever the content)].  Truncations, an injected marker and a lost or
    misnumbered restart marker are errors whatever the content.  A flipped byte inside the entropy-coded data may land in a
    coefficient's magnitude bits and give a VALID stream of another image, which no decoder can tell from an intact file: for those
    the restatement (tests/jpeg_reference.py, bit-serial, no shared code) is the judge -- see the test."""
    out = []
    for mode in ('420', 'restart', 'grey'):
        data = case(48, 64, mode, 75)[0]
        sos = data.index(b'\xff\xda')
        scan = sos + 2 + ((data[sos + 2] << 8) | data[sos + 3])
        n = len(data)
        for cut in (scan, scan + 1, scan + 7, (scan + n) // 2, n - 40, n - 3):
            out.append(('%s cut at %d of %d' % (mode, cut, n), data[:cut], True))
        mid = (scan + n) // 2
        out.append((mode + ' with an EOI marker in the middle of the data', _edit(data, mid, [0xFF, 0xD9]), True))
        out.append((mode + ' ending in a lone FF', data[:mid] + b'\xff', True))
        g = np.random.Generator(np.random.Philox(key=[11, len(mode)]))
        for at in g.integers(scan, n - 2, 24):
            flipped = _edit(data, int(at), [data[int(at)] ^ (1 << int(g.integers(0, 8)))])
            out.append(('%s with byte %d flipped' % (mode, at), flipped, False))
    data = case(48, 64, 'restart', 75)[0]
    first = data.index(b'\xff\xd0', data.index(b'\xff\xda'))
    out.append(('restart marker removed', data[:first] + data[first + 2:], True))
    out.append(('restart marker out of order', _edit(data, first + 1, [0xD3]), True))
    return out


def test_corrupt_streams_end_with_a_status_inside_the_buffer():
    """Every corrupt stream: the call returns, reads nothing behind the stream (which ends where an inaccessible page begins) and
    reports known status bits.  Structural damage must be an error.  A stream with a flipped byte goes through the restatement too:
    where that fails (no code matches, a run leaves the block, it reads into a marker, a restart marker is not where it must be) or
    ends with whole bytes left in front of the marker, the status must be an error; where it accepts the stream, the status must be 0
    and the coefficients must be the restatement's."""
    from hoig_amd.data import jpeg as J
    known = J.ECODE | J.EOVERRUN | J.EMARKER | J.ETRAILING
    seen, rejected, accepted = 0, 0, 0
    for what, data, must_fail in corrupt_streams():
        plan = J.parse(data)
        if plan is None:                                # (a flip that made a marker: the loader leaves such a file to the host decoder)
            assert not must_fail, what
            continue
        status = host_status(data, plan)
        assert status & ~known == 0, what
        if must_fail:
            assert status != 0, what
            seen |= status
            continue
        try:
            info, coefs = R.decode_coefficients(data)
            valid = info['left'] == 0
        except (ValueError, AssertionError, IndexError):
            valid = False
        if valid:
            _, _, _, work, again = host_entropy([(data, plan)])
            want = flat(coefs)
            assert status == 0 and again[0] == 0 and np.array_equal(work[:want.size * 2].view(np.int16), want), what
            accepted += 1
        else:
            assert status != 0, what
            rejected += 1
    assert seen & J.EOVERRUN and seen & J.EMARKER
    assert rejected >= 10 and accepted >= 1, (rejected, accepted)      # both kinds of flip occur among the 72
    # an intact file in the same position is clean
    data = case(48, 64, 'restart', 75)[0]
    assert host_status(data, J.parse(data)) == 0


def test_a_table_that_is_no_prefix_code_is_an_error_status():
    from hoig_amd import _lib as L
    from hoig_amd.data import jpeg as J
    data = case(16, 16, '420', 75)[0]
    plan = J.parse(data)
    plan['ac_counts'] = plan['ac_counts'].copy()
    plan['ac_counts'][0, 0] = 3                          # three codes of one bit
    assert host_status(data, plan) == J.ECODE
    plan = J.parse(data)
    plan['width'] = 70000
    _, plans, _ = J.pack([(data, plan)])
    assert L.lib.hoig_jpeg_decode_workspace_bytes(_p(plans), 1) == L.EUNSUPPORTED


# ---- the loader option
def jpeg_frames(opt, quality=90):
    """Turn the frames of an FX.build tree into 4:2:0 JPEGs and rewrite its listings (tests/data_fixture.py writes PNG frames)."""
    from PIL import Image
    pics = os.path.join(opt.data_dir, opt.images_dir, 'train')
    for seq in sorted(os.listdir(pics)):
        for name in sorted(os.listdir(os.path.join(pics, seq, 'rgb'))):
            path = os.path.join(pics, seq, 'rgb', name)
            Image.open(path).save(path[:-4] + '.jpg', quality=quality, subsampling=2)
            os.remove(path)
    for n in ('HOv3-CR_train_new.pkl', 'HOv3-CR_test_new.pkl'):
        path = os.path.join(opt.data_dir, opt.params_dir, n)
        vids = pickle.load(open(path, 'rb'))
        with open(path, 'wb') as f:
            pickle.dump({v: [x[:-4] + '.jpg' for x in frames] for v, frames in vids.items()}, f)
    return opt


def _no_host_decode_of_jpeg(monkeypatch):
    from hoig_amd.data import hov3_dataset, ycb_dataset
    real = hov3_dataset.imread_bgr

    def guarded(path):
        assert not path.lower().endswith(('.jpg', '.jpeg')), 'the host decoder was called for ' + path
        return real(path)
    monkeypatch.setattr(hov3_dataset, 'imread_bgr', guarded)
    monkeypatch.setattr(ycb_dataset, 'imread_bgr', guarded)
    return real


@pytest.mark.parametrize('tree', ['hov3', 'ycb'])
def test_with_the_option_a_dataset_item_carries_the_files_bytes(tmp_path, monkeypatch, tree):
    from hoig_amd.data import DatasetFactory
    from hoig_amd.data import jpeg as J
    from hoig_amd.data.device_stage import collate_raw
    monkeypatch.delenv('HOIG_DEVICE_JPEG', raising=False)
    if tree == 'hov3':
        opt = jpeg_frames(FX.build(str(tmp_path), seed=5, frames=3, frame_hw=(96, 128), mask_hw=(48, 64)))
        FX.write_pairs(opt, [('ABF1_0/0001.jpg', 'MC2_0/0002.jpg'), ('MC2_0/0000.jpg', 'ABF1_0/0002.jpg')])
        path_of = lambda name: os.path.join(opt.data_dir, 'images', 'train', name.split('_')[0], 'rgb', name.split('/')[1])
    else:
        opt = FX.build_ycb(str(tmp_path), seed=6)
        vid = '20200709-subject-01/20200709_141754/836212060125'
        FX.write_pairs(opt, [(vid + '/1', vid + '/2'), (vid + '/0', vid + '/2')])
        path_of = lambda name: os.path.join(opt.data_dir, 'images', name.rsplit('/', 1)[0], 'color_%06d.jpg' % int(name.rsplit('/', 1)[1]))
    off = DatasetFactory.get_by_name(tree, opt, True)[0]
    real = _no_host_decode_of_jpeg(monkeypatch)
    opt.device_jpeg = True
    ds = DatasetFactory.get_by_name(tree, opt, True)
    on = ds[0]
    for side in ('A', 'B'):
        a, b = off[side], on[side]
        assert 'frame' in a and 'jpeg' not in a                      # the option off: the record of before
        assert set(b) == (set(a) - {'frame'}) | {'jpeg', 'jpeg_plan'}
        path = path_of(b['name'])
        assert bytes(b['jpeg'].numpy()) == open(path, 'rb').read() and b['jpeg_plan']['path'] == path
        assert np.array_equal(a['frame'].numpy(), real(path)) and a['frame'].shape == (b['jpeg_plan']['height'], b['jpeg_plan']['width'], 3)
        for k in set(a) - {'frame'}:
            assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k
    # the environment variable is the same switch
    del opt.device_jpeg
    monkeypatch.setenv('HOIG_DEVICE_JPEG', '1')
    assert 'jpeg' in DatasetFactory.get_by_name(tree, opt, True)[0]['A']
    # a collated batch: one packed buffer, each file at its offset, plan records that the host twin decodes to the reference's coefficients
    raw = collate_raw([on, ds[1]])
    files = raw['A']['jpeg']
    assert raw['A']['frame'] == [None, None] and files['slots'] == [0, 1] and files['bytes'].numel() % 16 == 0
    plans = files['plans'].numpy().view(J.PLAN_DTYPE)
    for i, rec in enumerate(plans):
        data = open(files['paths'][i], 'rb').read()
        plan = J.parse(data)
        start = int(rec['data_off']) - plan['scan_offset']
        assert bytes(files['bytes'][start:start + len(data)].numpy()) == data
        assert rec['out_off'] == i * plan['height'] * plan['width'] * 3


def test_a_file_the_device_does_not_take_stays_a_decoded_frame(tmp_path, monkeypatch):
    """A progressive JPEG and a PNG among baseline files: their records carry 'frame' as before, and the batch mixes both kinds."""
    from PIL import Image
    from hoig_amd.data import DatasetFactory
    from hoig_amd.data.device_stage import collate_raw
    monkeypatch.delenv('HOIG_DEVICE_JPEG', raising=False)
    opt = jpeg_frames(FX.build(str(tmp_path), seed=5, frames=3, frame_hw=(96, 128), mask_hw=(48, 64)))
    rgb = os.path.join(opt.data_dir, 'images', 'train', 'ABF1', 'rgb')
    Image.open(os.path.join(rgb, '0001.jpg')).save(os.path.join(rgb, '0001.jpg'), quality=90, progressive=True)
    FX.write_pairs(opt, [('ABF1_0/0001.jpg', 'MC2_0/0002.jpg'), ('ABF1_0/0000.jpg', 'ABF1_0/0001.jpg')])
    opt.device_jpeg = True
    ds = DatasetFactory.get_by_name('hov3', opt, True)
    a, b = ds[0], ds[1]
    assert 'frame' in a['A'] and 'jpeg' not in a['A'] and 'jpeg' in a['B']
    want = np.asarray(Image.open(os.path.join(rgb, '0001.jpg')).convert('RGB'))[:, :, ::-1]
    assert np.array_equal(a['A']['frame'].numpy(), want)
    raw = collate_raw([a, b])
    assert [f is None for f in raw['A']['frame']] == [False, True] and raw['A']['jpeg']['slots'] == [1]
    assert raw['A']['jpeg']['plans'].numpy().view('<i8')[1] == 96 * 128 * 3          # out_off: slot 1 of the batch
    assert torch.is_tensor(raw['A']['mask']) and raw['A']['mask'].shape[0] == 2
    assert raw['B']['jpeg']['slots'] == [0] and torch.equal(raw['B']['frame'][1], a['A']['frame'])


def test_without_the_option_a_worker_imports_what_it_imported_before(tmp_path):
    code = '''
import sys
sys.path[:0] = [%r, %r]
import data_fixture as FX
from hoig_amd.data import DatasetFactory
opt = FX.build_ycb(%r, seed=6)
item = DatasetFactory.get_by_name('ycb', opt, True)[0]
assert 'frame' in item['A'] and 'hoig_amd.data.jpeg' not in sys.modules, sorted(m for m in sys.modules if 'jpeg' in m.lower())
opt.device_jpeg = True
item = DatasetFactory.get_by_name('ycb', opt, True)[0]
assert 'jpeg' in item['A'] and 'hoig_amd.data.jpeg' in sys.modules
print('ok')
''' % (ROOT, os.path.join(ROOT, 'tests'), str(tmp_path))
    env = {k: v for k, v in os.environ.items() if k != 'HOIG_DEVICE_JPEG'}
    out = subprocess.run([sys.executable, '-c', code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip().endswith('ok'), out.stdout


def test_corrupt_streams_under_a_host_address_sanitizer_build_of_the_twin(tmp_path):
    """The same corrupt streams (and the intact ones) through jpeg_host.cpp built with -fsanitize=address, each buffer a heap block of
    exactly its size (tests/jpeg_asan_driver.cpp): no report, and the statuses of the library's twin."""
    import shutil
    import struct
    from hoig_amd import _lib as L
    from hoig_amd.data import jpeg as J
    cxx = shutil.which(os.environ.get('CXX', 'c++'))
    flags = ['-O1', '-g', '-std=c++17', '-fsanitize=address', '-static-libasan']
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    if cxx is None or subprocess.run([cxx] + flags + [str(probe), '-o', str(tmp_path / 'probe')], stdout=subprocess.DEVNULL,
                                     stderr=subprocess.DEVNULL).returncode != 0:
        pytest.skip('no host C++ compiler that links an AddressSanitizer runtime (an empty program does not build with %s)' % ' '.join(flags))
    exe = str(tmp_path / 'jpeg_asan_driver')
    src = [os.path.join(ROOT, 'hoig_amd', 'csrc', 'jpeg_host.cpp'), os.path.join(ROOT, 'tests', 'jpeg_asan_driver.cpp')]
    build = subprocess.run([cxx] + flags + ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'hoig_amd', 'csrc')] + src +
                           ['-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    streams = [(w, d) for w, d, _ in corrupt_streams()] + [('intact ' + m, case(48, 64, m, 75)[0]) for m in R.MODES]
    blob, want = [], []
    for what, data in streams:
        plan = J.parse(data)
        if plan is None:
            continue
        _, plans, ivs = J.pack([(data, plan)])
        size = L.lib.hoig_jpeg_decode_workspace_bytes(_p(plans), 1)
        coef_bytes = int(plans[0]['plane_off'])                     # (the coefficient part: all the twin writes)
        assert 0 < coef_bytes < size
        blob.append(struct.pack('<qqq', len(data), ivs.size, coef_bytes) + plans.tobytes() + data + ivs.tobytes())
        want.append('0 %d' % host_status(data, plan))
    case_file = tmp_path / 'cases.bin'
    case_file.write_bytes(struct.pack('<i', len(blob)) + b''.join(blob))
    run = subprocess.run([exe, str(case_file)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0 and 'AddressSanitizer' not in run.stdout, run.stdout[-3000:]
    assert run.stdout.split('\n')[:len(want)] == want and len(want) > 80
