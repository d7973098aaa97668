"""The PNG decoder through its host twins (hoig_amd/csrc/png_decode_host.cpp: the per-lane code of the kernels, a workgroup walked lane
by lane).  Inflate alone is held against zlib.decompress, whole files against np.asarray(Image.open(f).convert('RGB')); never against
the decoder itself."""
import io
import os
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

import png_decode_reference as G
import png_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (0, 1, 2, 3, 258, 259, 32767, 32768, 32769, 70000, 200000)


def contents(n):
    rng = np.random.RandomState(n % 1000 + 1)
    out = {'noise': rng.randint(0, 256, n).astype(np.uint8).tobytes(), 'zeros': bytes(n), 'text': G.text_like(n, seed=n % 7)}
    side = max(1, int(np.ceil(np.sqrt(n / 3.0))))
    for kind in R.CLASSES[:5]:
        out[kind] = R.content(kind, side, side, 3, seed=2).tobytes()[:n]
    return out


def compressed(raw):
    for level in (0, 1, 6, 9):
        yield 'level%d' % level, zlib.compress(raw, level)
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
    yield 'fixed', co.compress(raw) + co.flush()


def check_inflate(z, want, what):
    assert zlib.decompress(z) == want, what                     # the crafted or compressed stream is valid in the first place
    got, status = G.inflate_host(z, len(want))
    assert status == 0, (what, G.D().status_text(status))
    assert got == want, what


@pytest.mark.parametrize('n', LENGTHS)
def test_inflate_equals_zlib_on_zlibs_streams(n):
    for kind, raw in contents(n).items():
        assert len(raw) == n
        for how, z in compressed(raw):
            check_inflate(z, raw, (n, kind, how))


def test_inflate_equals_zlib_on_the_encoders_crafted_streams():
    fib = [1, 1]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    vals = np.repeat(np.arange(17, dtype=np.uint8) * 13 + 5, fib[1:])
    np.random.RandomState(5).shuffle(vals)
    z, _ = R.deflate_host(vals.tobytes(), dist_c=-1)
    lit, _ = R.first_block_code_lengths(z)
    assert max(lit) == 15                                        # 15-bit codes
    check_inflate(z, vals.tobytes(), 'fibonacci')
    check_inflate(R.deflate_host(vals.tobytes())[0], vals.tobytes(), 'fibonacci with matches')
    block = np.random.RandomState(8).randint(0, 256, 600).astype(np.uint8).tobytes()
    check_inflate(R.deflate_host(block * 6)[0], block * 6, 'one distance code')
    check_inflate(R.deflate_host(b'\x07' * 5000)[0], b'\x07' * 5000, 'one distance code at distance 1')
    check_inflate(R.deflate_host(b'\x07' * 5000, dist_c=-1)[0], b'\x07' * 5000, 'no match, a single literal')
    check_inflate(R.deflate_host(block, dist_c=-1)[0], block, 'no match')
    for seg in R.SEGMENTS:
        check_inflate(R.deflate_host(block * 120, segment_bytes=seg)[0], block * 120, 'matches across segments')
    check_inflate(R.deflate_host(b'')[0], b'', 'nothing')


def test_every_match_length_at_the_short_distances():
    head = np.random.RandomState(3).randint(0, 256, 70).astype(np.uint8).tobytes()
    for dist in (1, 2, 3, 63, 64, 65):
        t = G.FixedTokens()
        t.literals(head)
        for length in range(3, 259):
            t.match(length, dist)
            t.literal(length & 255)
        check_inflate(t.stream(), bytes(t.expected), dist)


@pytest.mark.parametrize('dist', [32767, 32768])
def test_the_longest_distances_behind_a_32k_head(dist):
    head = np.random.RandomState(dist).randint(0, 256, 32768).astype(np.uint8).tobytes()
    t = G.FixedTokens()
    t.literals(head)
    for length in (3, 64, 65, 258, 17):
        t.match(length, dist)
    t.literals(b'xyz')
    t.match(258, dist)
    check_inflate(t.stream(), bytes(t.expected), dist)


def test_a_match_that_ends_the_output_and_token_lists_that_wrap():
    t = G.FixedTokens()
    t.literals(b'abcdefg')
    t.match(258, 7)
    check_inflate(t.stream(), bytes(t.expected), 'a match ends the output')
    t = G.FixedTokens()
    t.literals(b'abc')
    for _ in range(200):
        t.match(3, 3)
    check_inflate(t.stream(), bytes(t.expected), '200 matches of 3')
    t = G.FixedTokens()                                          # far matches between literals: the rounds they end
    t.literals(np.random.RandomState(9).randint(0, 256, 20000).astype(np.uint8).tobytes())
    for k in range(150):
        t.match(3 + k, 16257 + 20 * k)
        t.literal(k)
    check_inflate(t.stream(), bytes(t.expected), 'far matches between literals')


# ---- whole files

def check_files(files):
    D = G.D()
    for name, f in files:
        want = G.pillow_rgb(f)
        plan, why = D.parse(f)
        assert plan is not None, (name, why)
        (got,), (status,) = G.decode_host([plan])
        assert status == 0, (name, D.status_text(status))
        assert np.array_equal(got, want), name
        (bgr,), _ = G.decode_host([plan], bgr=True)
        assert np.array_equal(bgr, want[..., ::-1]), name


@pytest.mark.parametrize('size', G.SIZES, ids=lambda s: '%dx%d' % s)
def test_pillow_written_files_decode_to_pillows_pixels(size):
    files = G.pillow_files(sizes=(size,))
    depths = {(G.plan_of(f).color_type, G.plan_of(f).bit_depth) for _, f in files}
    # what Pillow wrote for the modes asked for (it lowers a palette file's depth to what the colours in use need: on a few pixels
    # there are fewer than 200 or 16 of them)
    assert {(0, 1), (0, 8), (4, 8), (6, 8), (2, 8), (3, 1)} <= depths
    if size[0] * size[1] >= 64 * 48:
        assert {(3, 8), (3, 4)} <= depths
    check_files(files)


def test_the_encoders_files_decode_with_all_five_filters_and_25_idats():
    files = G.own_files()
    big = dict(files)['own-noise55-256x256x3']
    _, idat, filtered = R.parse(big)
    assert len(idat) >= 25
    types = set()
    for _, f in files:
        plan = G.plan_of(f)
        rows = np.frombuffer(zlib.decompress(plan.stream), np.uint8).reshape(plan.height, -1)
        types |= set(rows[:, 0].tolist())
    assert types == {0, 1, 2, 3, 4}
    check_files(files)


def test_hand_filtered_files_of_every_kind_and_filter_type():
    files = G.hand_filtered_files()
    assert len(files) == 6 * len(G.KINDS)
    check_files(files)


def test_recut_idats_empty_idats_and_ancillary_chunks():
    check_files(G.recut_files())


def test_a_batch_of_every_kind_in_one_call():
    files = G.mixed_batch_files()
    plans = [G.plan_of(f) for f in files]
    assert {(p.color_type, p.bit_depth) for p in plans} == {(c, d) for c, d, _ in G.KINDS}
    got, status = G.decode_host(plans)
    assert status == [0] * len(plans)
    for g, f in zip(got, files):
        assert np.array_equal(g, G.pillow_rgb(f))


def test_parse_sends_unsupported_files_to_the_host_with_a_reason():
    D = G.D()
    for name, f, word in G.unsupported_files():
        plan, why = D.parse(f)
        assert plan is None and word in why, (name, why)
    for junk in (b'', b'\x89PNG', G.R_SIG, G.R_SIG + b'\x00' * 7, G.R_SIG + G.chunk(b'IEND', b''), bytes(100)):
        plan, why = D.parse(junk)
        assert plan is None and why


# ---- bad streams

def test_every_bad_stream_is_refused_by_zlib_or_pillow_first():
    for name, z, expect, _ in G.bad_streams():
        assert G.refused(z, expect), name
    for name, plan, bit in G.bad_plans():
        if bit == R.lib().PNG_EFILTER:
            with pytest.raises(OSError):
                G.pillow_rgb(G.png_file(plan.width, plan.height, plan.bit_depth, plan.color_type, plan.stream))
    assert {bit for _, _, _, bit in G.bad_streams()} | {R.lib().PNG_EFILTER} == {b for b, _ in G.D().STATUS_BITS}


def test_each_bad_stream_raises_its_one_status_bit():
    for name, z, expect, bit in G.bad_streams():
        _, status = G.inflate_host(z, expect)                   # the guard bands are checked inside
        assert status == bit, (name, G.D().status_text(status))


def test_bad_images_in_a_batch_leave_the_good_ones_exact():
    bad = G.bad_plans()
    good = [f for _, f in G.hand_filtered_files()[:len(bad)]]
    plans, want = [], []
    for (name, plan, bit), f in zip(bad, good):
        plans += [plan, G.plan_of(f)]
        want += [bit, 0]
    got, status = G.decode_host(plans)                          # the guard bands are checked inside
    assert status == want, [G.D().status_text(s) for s in status]
    for g, f in zip(got[1::2], good):
        assert np.array_equal(g, G.pillow_rgb(f))


def test_invalid_plans_are_refused_before_anything_runs():
    L, D = R.lib(), G.D()
    plan = G.plan_of(G.save(G.pillow_image('RGB', 17, 9)))
    buf, plans, out_bytes, ws_bytes = D.pack([plan])
    out, ws, st = np.full(out_bytes, 0x5A, np.uint8), np.full(ws_bytes, 0x5A, np.uint8), np.full(1, -7, np.int32)

    def both(nbytes=buf.size, out_b=out_bytes, ws_b=ws_bytes):
        host = L.lib.hoig_png_decode_host(G._p(buf), nbytes, plans, 1, G._p(out), out_b, G._p(st), G._p(ws), ws_b, 0)
        # the device entry refuses on the host, before any launch (no device is touched: the pointers are host memory)
        dev = L.lib.hoig_png_decode_u8(G._p(buf), nbytes, plans, G._p(buf), 1, G._p(out), out_b, G._p(st), G._p(ws), ws_b, 0, None)
        assert host == dev
        return host

    assert both(out_b=out_bytes - 1) == L.EINVAL and both(ws_b=ws_bytes - 16) == L.EINVAL and both(nbytes=buf.size - 16) == L.EINVAL
    for field, value, want in (('color_type', 5, L.EUNSUPPORTED), ('bit_depth', 16, L.EUNSUPPORTED), ('bit_depth', 4, L.EUNSUPPORTED),
                               ('width', 0, L.EINVAL), ('data_off', 8, L.EINVAL), ('out_off', -1, L.EINVAL), ('filt_off', 8, L.EINVAL)):
        keep = getattr(plans[0], field)
        setattr(plans[0], field, value)
        assert both() == want, field
        if field != 'filt_off':
            assert L.lib.hoig_png_decode_workspace_bytes(plans, 1) == want, field
        setattr(plans[0], field, keep)
    plans[0].color_type, plans[0].pal_entries = 3, 0              # a palette image without a palette
    assert both() == L.EUNSUPPORTED
    plans[0].color_type, plans[0].width, plans[0].height = 2, 1 << 20, 1 << 20       # a filtered stream of 2^31 bytes and more
    assert L.lib.hoig_png_decode_workspace_bytes(plans, 1) == L.EUNSUPPORTED
    assert (out == 0x5A).all() and (ws == 0x5A).all() and st[0] == -7


# ---- the Python wrapper and the option

def test_the_python_wrapper_equals_pillow():
    D = G.D()
    files = [f for _, f in G.pillow_files(sizes=((17, 9),), settings=[{'compress_level': 6}])]
    got = D.decode_u8_host(files)
    assert got.shape == (len(files), 9, 17, 3) and got.dtype == np.uint8
    for g, f in zip(got, files):
        assert np.array_equal(g, G.pillow_rgb(f))
    assert np.array_equal(D.decode_u8_host(files, bgr=True), got[..., ::-1])
    assert D.decode_u8_host([]).shape[0] == 0
    with pytest.raises(ValueError, match='differ in size'):
        D.decode_u8_host([files[0], G.save(G.pillow_image('RGB', 3, 5))])
    with pytest.raises(ValueError, match='interlaced'):
        D.decode_u8_host([G.unsupported_files()[0][1]])
    name, plan, bit = G.bad_plans()[0]
    bad = G.png_file(plan.width, plan.height, 8, 0, plan.stream)
    with pytest.raises(ValueError, match=D.status_text(bit)):
        D.decode_u8_host([bad])
    assert D.status_text(0) == 'ok' and 'Adler' in D.status_text(R.lib().PNG_EADLER | R.lib().PNG_ECODE)


def test_the_option_is_off_unless_asked_for(tmp_path, monkeypatch):
    """With the argument absent (and the variable unset) DeviceBatches and the directory functions never import or call the decoder."""
    import builtins
    import sys
    from hoig_amd.metrics import images as I
    monkeypatch.delenv('HOIG_DEVICE_PNG_DECODE', raising=False)
    for mod in [m for m in sys.modules if m.endswith('png_decode')]:
        monkeypatch.delitem(sys.modules, mod)
    real = builtins.__import__

    def guard(name, globals=None, locals=None, fromlist=(), level=0):
        if name.endswith('png_decode') or 'png_decode' in (fromlist or ()):
            raise AssertionError('the device PNG decoder was imported with the option off')
        return real(name, globals, locals, fromlist, level)

    monkeypatch.setattr(builtins, '__import__', guard)
    names = []
    for i in range(3):
        names.append(str(tmp_path / ('%d.png' % i)))
        Image.fromarray(R.content('noise55', 9, 17, 3, seed=i)).save(names[-1])
    for kw in ({}, {'device_png_decode': False}, {'device_png_decode': None}):
        b = I.DeviceBatches([names], 'cpu', **kw)
        assert b.device_png_decode is False
        (batch,) = list(b)
        assert np.array_equal(batch.numpy(), np.stack([np.asarray(Image.open(n)) for n in names]))
    assert I.png_decode_option(None) is False and I.png_decode_option(True) is True
    monkeypatch.setenv('HOIG_DEVICE_PNG_DECODE', '1')
    assert I.png_decode_option(None) is True and I.png_decode_option(False) is False
    assert I.DeviceBatches([names], 'cpu').device_png_decode is True
    assert I.DeviceBatches([names], 'cpu', device_png_decode=False).device_png_decode is False
    # asked for, the decoder is reached: the import guard fires
    with pytest.raises(AssertionError, match='imported with the option off'):
        list(I.DeviceBatches([names], 'cpu', device_png_decode=True))


def test_the_directory_functions_take_the_argument_and_the_cli_the_flag():
    import inspect
    from hoig_amd.metrics import __main__ as M
    from hoig_amd.metrics import fid, lpips, ssim
    for fn in (fid.get_activations, fid.calculate_activation_statistics, fid.compute_statistics_of_path, fid.calculate_fid_given_paths,
               lpips.calculate_lpips_given_paths, ssim.calculate_ssim_given_paths):
        assert inspect.signature(fn).parameters['device_png_decode'].default is None, fn.__name__
    assert M.parser().parse_args(['ssim', 'a', 'b']).device_png_decode is None
    assert M.parser().parse_args(['ssim', 'a', 'b', '--device-png-decode']).device_png_decode is True


# ---- the twins under a host sanitizer

def fnv(data, h=2166136261):
    for v in bytes(data):
        h = ((h ^ v) * 16777619) & 0xFFFFFFFF
    return h


def test_the_host_twins_under_a_host_address_sanitizer_build(tmp_path):
    """png_decode_host.cpp built with -fsanitize=address into a program of its own (tests/png_decode_asan_driver.cpp), every buffer a
    heap block of exactly its size: no report on the bad streams and a sample of the good files, and the library twin's results."""
    import shutil
    import struct
    cxx = shutil.which(os.environ.get('CXX', 'c++'))
    flags = ['-O1', '-g', '-std=c++17', '-fsanitize=address', '-static-libasan']
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    if cxx is None or subprocess.run([cxx] + flags + [str(probe), '-o', str(tmp_path / 'probe')], stdout=subprocess.DEVNULL,
                                     stderr=subprocess.DEVNULL).returncode != 0:
        pytest.skip('no host C++ compiler that links an AddressSanitizer runtime (an empty program does not build with %s)' % ' '.join(flags))
    exe = str(tmp_path / 'png_decode_asan_driver')
    src = [os.path.join(ROOT, 'hoig_amd', 'csrc', 'png_decode_host.cpp'), os.path.join(ROOT, 'tests', 'png_decode_asan_driver.cpp')]
    build = subprocess.run([cxx] + flags + ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'hoig_amd', 'csrc')] + src +
                           ['-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    plans = [p for _, p, _ in G.bad_plans()]
    plans += [G.plan_of(f) for n, f in G.hand_filtered_files() if n.endswith('cycle')]
    plans += [G.plan_of(f) for _, f in G.pillow_files(sizes=((1, 1), (64, 48)), settings=[{'compress_level': 6}])]
    plans += [G.plan_of(f) for _, f in G.own_files()[:2]]
    blob, want = struct.pack('<i', len(plans)), []
    for p in plans:
        pal = p.palette or b''
        blob += struct.pack('<7i', p.width, p.height, p.color_type, p.bit_depth, len(p.stream), len(pal), len(plans) % 2) + p.stream + pal
        (got,), (status,) = G.decode_host([p], bgr=len(plans) % 2)
        want.append('%d %d' % (status, fnv(got) if status == 0 else 0))
    cases = tmp_path / 'cases.bin'
    cases.write_bytes(blob)
    run = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0 and 'AddressSanitizer' not in run.stdout, run.stdout[-3000:]
    assert run.stdout.split('\n')[:len(want)] == want
