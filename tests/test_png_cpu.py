"""The PNG encoder through its host twins (hoig_amd/csrc/png_host.cpp: the per-lane code of the kernels, a workgroup walked lane by lane).

What a file must be: ordinary PNG that Pillow opens to the input, one IDAT per segment (plus the Adler-32's), every CRC-32 right; how
small it must be is computed here from Pillow and zlib on the same input, never by the code under test."""
import ctypes
import heapq
import io
import os
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

import png_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_p = R._p


@pytest.fixture(scope='module')
def big():
    """class -> (image, filtered stream, file) at 256 x 256 x 3, the default segment size; encoded once"""
    out = {}
    for kind in R.CLASSES:
        img = R.content(kind, 256, 256, 3, seed=3)
        out[kind] = (img, R.filter_stream(img).tobytes(), R.encode_host(img[None])[0])
    return out


@pytest.mark.parametrize('shape', [s for s, _, _ in R.SHAPES] + [R.MIXED], ids=lambda s: '%dx%dx%d' % s)
def test_the_filter_twin_equals_the_restatement(shape):
    for kind in R.CLASSES:
        img = R.content(kind, *shape)
        assert np.array_equal(R.filter_host(img), R.filter_stream(img)), kind


def test_the_restatement_picks_every_filter_and_breaks_ties_low():
    types = set()
    for kind in R.CLASSES:
        img = R.content(kind, 33, 17, 3)
        types |= set(R.filter_stream(img).reshape(33, -1)[:, 0].tolist())
    assert types == {0, 1, 2, 3, 4}
    assert R.filter_stream(np.zeros((3, 4, 3), np.uint8)).reshape(3, -1)[:, 0].tolist() == [0, 0, 0]      # all five sums equal


def check_file(png, img, segment_bytes):
    h, w, c = img.shape
    ihdr, idat, inflated = R.parse(png)
    assert ihdr == (w, h, 8, 2 if c == 3 else 0, 0, 0, 0)
    got = np.asarray(Image.open(io.BytesIO(png)))
    assert got.dtype == np.uint8 and np.array_equal(got.reshape(h, w, c), img)
    filtered = R.filter_stream(img).tobytes()
    assert inflated == filtered
    seg = segment_bytes or 8192
    nseg = -(-len(filtered) // seg)
    assert nseg <= len(idat) <= nseg + 1
    assert len(png) <= R.lib().lib.hoig_png_encode_bound(h, w, c, segment_bytes)
    return idat


@pytest.mark.parametrize('case', R.CASES, ids=R.CASE_IDS)
def test_a_file_decodes_to_its_input(case):
    shape, seg, kind = case
    img = R.content(kind, *shape)
    idat = check_file(R.encode_host(img[None], seg)[0], img, seg)
    # every segment ends on a byte boundary with an empty stored block
    n = -(-(shape[0] * (1 + shape[1] * shape[2])) // (seg or 8192))
    for k in range(n):
        assert idat[k][-4:] == b'\x00\x00\xff\xff'
    assert idat[0][:2] == b'\x78\x01'


def test_the_mixed_batch_and_the_workload_shape(big):
    batch = R.mixed_batch()
    files = R.encode_host(batch)
    assert len(files) == 5
    for png, img in zip(files, batch):
        check_file(png, img, 0)
    for kind in R.CLASSES:
        check_file(big[kind][2], big[kind][0], 0)
    # a batch is its images one by one
    assert files[3] == R.encode_host(batch[3:4])[0]


def test_the_python_wrapper_gives_the_twins_files():
    from hoig_amd import png
    batch = R.mixed_batch()[:2, :40, :70]
    assert png.encode_u8_host(batch, 4096) == R.encode_host(batch, 4096)
    assert png.encode_u8_host(batch[:0]) == []
    assert png.SEGMENT_BYTES == 8192


# ---- crafted streams for the Huffman edge cases

def huffman_depth(freqs):
    heap = [(f, i, 0) for i, f in enumerate(freqs) if f]
    heapq.heapify(heap)
    tick = len(freqs)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], tick, max(a[2], b[2]) + 1))
        tick += 1
    return heap[0][2]


def roundtrip(stream, **kw):
    z, segs = R.deflate_host(stream, **kw)
    assert zlib.decompress(z) == bytes(stream)
    assert z[:2] == b'\x78\x01' and len(z) == 6 + int(segs.sum())
    return z, segs


def kraft(lens):
    return sum(2.0 ** -n for n in lens if n)


def test_a_fibonacci_histogram_needs_the_length_limiter():
    """17 byte values with the Fibonacci counts 1, 2, 3, 5 .. 2584 (6763 bytes, one segment), shuffled: with the end-of-block symbol's
    count of 1 in front the histogram is the Fibonacci sequence, whose unlimited Huffman tree is a chain 17 deep; deflate allows 15.
    A shuffle of so few values repeats many 3-byte strings, so the histogram is pinned by switching the match search off (dist_c = -1);
    with it on the same stream must still come back."""
    fib = [1, 1]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    assert huffman_depth(fib) == 17 and sum(fib[1:]) < 8192
    vals = np.repeat(np.arange(17, dtype=np.uint8) * 13 + 5, fib[1:])
    np.random.RandomState(5).shuffle(vals)
    z, segs = roundtrip(vals.tobytes(), dist_c=-1)
    assert len(segs) == 1 and segs[0] < len(vals) // 2          # a dynamic block, not the stored fallback
    lit, dist = R.first_block_code_lengths(z)
    assert sum(1 for n in lit if n) == 18 and max(lit) == 15 and kraft(lit) == 1.0
    assert sorted(n for n in lit if n)[:3] == [1, 2, 3]         # the limiter took its bits from the deep end
    assert dist == [1, 1]                                        # no match at all: two one-bit codes, a complete code
    roundtrip(vals.tobytes())


def test_the_degenerate_codes_are_complete():
    z, _ = roundtrip(b'\x07' * 5000, dist_c=-1)                  # a single distinct literal, no match
    lit, dist = R.first_block_code_lengths(z)
    assert [n for n in lit if n] == [1, 1] and lit[7] == 1 and lit[256] == 1 and dist == [1, 1]
    z, _ = roundtrip(b'\x07' * 5000)                             # one literal, then matches at distance 1: one distance code
    lit, dist = R.first_block_code_lengths(z)
    assert kraft(lit) == 1.0 and kraft(dist) == 1.0 and dist == [1, 1]
    block = np.random.RandomState(8).randint(0, 256, 600).astype(np.uint8).tobytes()
    z, _ = roundtrip(block * 6)                                  # one distance code that is not code 0
    lit, dist = R.first_block_code_lengths(z)
    assert kraft(lit) == 1.0 and kraft(dist) == 1.0 and sum(1 for n in dist if n) == 2 and dist[0] == 1 and dist[-1] == 1


def test_every_byte_value_and_every_match_length():
    rng = np.random.RandomState(6)
    base = rng.randint(0, 256, 300).astype(np.uint8).tobytes()
    parts = [bytes(range(256)), base]
    for length in range(3, 259):
        parts += [base[:length], bytes(rng.randint(0, 256, 2).astype(np.uint8))]
    stream = b''.join(parts)
    for seg in R.SEGMENTS:
        roundtrip(stream, segment_bytes=seg)


def test_matches_at_one_distance_only():
    block = np.random.RandomState(7).randint(0, 256, 100).astype(np.uint8).tobytes()
    z, _ = roundtrip(block * 40)
    assert len(z) < 1000                                         # 3900 bytes of repeats went as matches
    z, _ = roundtrip(block * 40, dist_c=100)                     # the same distance as a fixed candidate
    assert len(z) < 1000


def test_one_repeated_byte_three_bytes_and_nothing():
    z, _ = roundtrip(b'\x07' * 5000)
    assert len(z) < 200
    roundtrip(b'\x07' * 70000, segment_bytes=32768, dist_c=3, dist_row=769)
    roundtrip(b'abc')
    roundtrip(b'aaa')
    roundtrip(b'a')
    z, segs = roundtrip(b'')
    assert len(segs) == 1


# ---- sizes, against Pillow and zlib on the same input

def huffman_only_size(filtered, seg=8192):
    """zlib Z_HUFFMAN_ONLY on the same filtered stream in the same segments with the same 17 bytes of framing each, plus the file's
    fixed parts (signature, IHDR, zlib header, the Adler-32 chunk, IEND)."""
    total = 33 + 2 + 16 + 12
    for at in range(0, len(filtered), seg):
        co = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
        total += len(co.compress(filtered[at:at + seg]) + co.flush(zlib.Z_FINISH)) + 17
    return total


def pillow_size(img):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format='PNG')
    return buf.tell()


@pytest.mark.parametrize('kind', ['noise55', 'noise6'])
def test_on_photograph_like_content_a_file_is_within_5_percent_of_pillows(big, kind):
    img, _, png = big[kind]
    ours, theirs = len(png), pillow_size(img)
    print(kind, ours, theirs)
    assert ours <= 1.05 * theirs


@pytest.mark.parametrize('kind', ['smooth', 'rect', 'zeros'])
def test_on_smooth_content_the_matcher_beats_huffman_only(big, kind):
    _, filtered, png = big[kind]
    ours, theirs = len(png), huffman_only_size(filtered)
    print(kind, ours, theirs)
    assert ours < theirs


def test_uniform_noise_costs_under_one_percent_and_a_kilobyte(big):
    _, filtered, png = big['uniform']
    print(len(png), len(filtered))
    assert len(png) <= len(filtered) * 1.01 + 1024


# ---- refused arguments

def test_invalid_arguments_are_refused_and_nothing_is_written():
    L = R.lib()
    bound, ws, host, dev = (L.lib.hoig_png_encode_bound, L.lib.hoig_png_encode_workspace_bytes, L.lib.hoig_png_encode_host,
                            L.lib.hoig_png_encode_u8)
    assert bound(8, 8, 3, 1000) == L.EINVAL and ws(1, 8, 8, 3, 1000) == L.EINVAL
    for h, w, c in ((8, 8, 2), (8, 8, 4), (0, 8, 3), (8, 0, 3), (65536, 32768, 1)):        # the last: a stream of 2^31 bytes and more
        assert bound(h, w, c, 0) == L.EUNSUPPORTED and ws(1, h, w, c, 0) == L.EUNSUPPORTED
    assert ws(0, 8, 8, 3, 0) == L.EINVAL
    good = bound(8, 8, 3, 0)
    assert good >= 33 + 8 * 25 + 22 + 2 + 28 and bound(8, 8, 3, 8192) == good
    src = np.zeros((1, 8, 8, 4), np.uint8)
    out = np.full(4096, 0x5A, np.uint8)
    sizes = np.full(1, -7, np.int32)
    calls = [(8, 8, 3, good, 1000, L.EINVAL), (8, 8, 2, good, 0, L.EUNSUPPORTED), (8, 8, 4, good, 0, L.EUNSUPPORTED),
             (0, 8, 3, good, 0, L.EUNSUPPORTED), (8, 8, 3, 100, 0, L.EINVAL)]
    for h, w, c, stride, seg, want in calls:
        assert host(_p(src), 1, h, w, c, _p(out), stride, _p(sizes), seg) == want
        # the device entry refuses on the host, before any launch (no device is touched: the pointers are host memory)
        assert dev(_p(src), 1, h, w, c, _p(out), stride, _p(sizes), _p(out), 1 << 20, seg, None) == want
    need = ws(1, 8, 8, 3, 0)
    assert need > 0
    assert dev(_p(src), 1, 8, 8, 3, _p(out), good, _p(sizes), _p(out), need - 1, 0, None) == L.EINVAL       # an undersized workspace
    assert (out == 0x5A).all() and sizes[0] == -7
    size = ctypes.c_int64(-7)
    assert L.lib.hoig_png_deflate_host(_p(src), 64, 1000, 0, 0, _p(out), 4096, ctypes.byref(size), None) == L.EINVAL
    assert L.lib.hoig_png_deflate_host(_p(src), 64, 0, 0, 0, _p(out), 70, ctypes.byref(size), None) == L.EINVAL   # out too small
    assert (out == 0x5A).all() and size.value == -7
    assert L.lib.hoig_png_filter_host(_p(src), 8, 8, 4, _p(out)) == L.EUNSUPPORTED and (out == 0x5A).all()


# ---- the twin under a host sanitizer

def driver_content(mode, n, seed):
    i = np.arange(n, dtype=np.uint64)
    if mode == 0:
        return (((i * 2654435761 + seed) & 0xFFFFFFFF) >> 24).astype(np.uint8)
    if mode == 1:
        return np.zeros(n, np.uint8)
    return ((i >> 4) & 0xFF).astype(np.uint8)


def test_the_host_twins_under_a_host_address_sanitizer_build(tmp_path):
    """png_host.cpp built with -fsanitize=address into a program of its own (tests/png_asan_driver.cpp), every buffer a heap block of
    exactly its size: no report, and the files of the library's twin."""
    import shutil
    cxx = shutil.which(os.environ.get('CXX', 'c++'))
    flags = ['-O1', '-g', '-std=c++17', '-fsanitize=address', '-static-libasan']
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    if cxx is None or subprocess.run([cxx] + flags + [str(probe), '-o', str(tmp_path / 'probe')], stdout=subprocess.DEVNULL,
                                     stderr=subprocess.DEVNULL).returncode != 0:
        pytest.skip('no host C++ compiler that links an AddressSanitizer runtime (an empty program does not build with %s)' % ' '.join(flags))
    exe = str(tmp_path / 'png_asan_driver')
    src = [os.path.join(ROOT, 'hoig_amd', 'csrc', 'png_host.cpp'), os.path.join(ROOT, 'tests', 'png_asan_driver.cpp')]
    build = subprocess.run([cxx] + flags + ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'hoig_amd', 'csrc')] + src +
                           ['-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    args, want = [], []
    for shape, segs, _ in R.SHAPES:
        for mode in (0, 1, 2):
            seg = segs[0]
            h, w, c = shape
            args += [h, w, c, seg, mode]
            a = driver_content(mode, 2 * h * w * c, h * 31 + w).reshape(2, h, w, c)
            fnv = 2166136261
            for png in R.encode_host(a, seg):
                for v in png:
                    fnv = ((fnv ^ v) * 16777619) & 0xFFFFFFFF
            want.append('0 %d' % fnv)
    run = subprocess.run([exe, '2'] + [str(v) for v in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0 and 'AddressSanitizer' not in run.stdout, run.stdout[-3000:]
    assert run.stdout.split('\n')[:len(want)] == want


# ---- the option is off unless asked for

def test_eval_writer_stays_on_pillow_unless_asked(tmp_path, monkeypatch):
    from hoig_amd import eval_output as E
    monkeypatch.delenv('HOIG_DEVICE_PNG', raising=False)
    seen = []
    monkeypatch.setattr(E, '_save_png', lambda arr, path: seen.append((np.array(arr), path)))
    images = {k: R.mixed_batch()[:2, :16, :16] + i for i, k in enumerate(('source', 'imitators', 'gt'))}
    names_a, names_b = ['v1/0001.jpg', 'v2/0002.jpg'], ['v1/0005.jpg', 'v2/0009.jpg']
    for kw in ({}, {'device_png': False}):
        del seen[:]
        w = E.EvalWriter(str(tmp_path / ('o%d' % len(kw))), workers=0, **kw)
        assert w.device_png is False
        w.write_images(images, names_a, names_b)
        w.close()
        assert [os.path.relpath(p, w.out_dir) for _, p in seen] == [os.path.join(s, n) for s in ('source', 'imitators', 'gt')
                                                                     for n in ('v1_0001_0005.png', 'v2_0002_0009.png')]
        for (arr, _), want in zip(seen, [images[s][i] for s in ('source', 'imitators', 'gt') for i in (0, 1)]):
            assert np.array_equal(arr, want)
    # asked for, host arrays still go through Pillow: only device tensors are encoded on the device
    del seen[:]
    w = E.EvalWriter(str(tmp_path / 'on'), workers=0, device_png=True)
    w.write_images(images, names_a, names_b)
    w.close()
    assert len(seen) == 6
    monkeypatch.setenv('HOIG_DEVICE_PNG', '1')
    assert E.EvalWriter(str(tmp_path / 'env'), workers=0).device_png is True
    assert E.EvalWriter(str(tmp_path / 'env'), workers=0, device_png=False).device_png is False
