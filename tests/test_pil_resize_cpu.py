"""The host side of the Pillow-exact 8-bit bilinear resize (hoig_amd/csrc/pil_resize.h through hoig_pil_bilinear_table and the CPU twin
hoig_resize_pil_bilinear_u8_host).

The first test pins tests/pil_resize_reference.py to Pillow in every byte; the tables, which Pillow does not expose, are then compared
with that restatement, and the twin with Pillow directly."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pil_resize_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_p = lambda a: ctypes.c_void_p(a.ctypes.data)
IDS = ['%dx%d-%dx%d' % (c[0] + c[1]) for c in R.CASES]


def host_resize(a, size):
    from hoig_amd import _lib as L
    a = np.ascontiguousarray(a)
    out = np.full((a.shape[0], size[0], size[1], 3), 0x5A, np.uint8)
    rc = L.lib.hoig_resize_pil_bilinear_u8_host(_p(a), a.shape[0], a.shape[1], a.shape[2], a.shape[3], _p(out), size[0], size[1])
    assert rc == 0, rc
    return out


@pytest.mark.parametrize('binary', [False, True])
@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_the_restatement_equals_pillow_every_byte(case, binary):
    (h, w), size = case
    a = R.content(2, h, w, h * 31 + w, binary)
    got = R.resize(a, size)
    assert got.shape == (2,) + size + (3,)
    assert np.array_equal(got, R.pillow(a, size))


@pytest.mark.parametrize('binary', [False, True])
def test_the_restatement_equals_pillow_on_the_chain(binary):
    (h, w), mid, side = R.CHAIN
    a = R.content(2, h, w, 5, binary)
    want = R.pillow(R.pillow(a, (mid, mid)), (side, side))
    assert np.array_equal(R.resize(R.resize(a, (mid, mid)), (side, side)), want)


def test_the_cases_reach_the_special_paths():
    xmin, n, _ = R.coefficients(5, 3)
    assert xmin[0] == 0 and xmin[-1] + n[-1] == 5 and n.max() > n.min()      # windows cut at both edges
    assert R.ksize(1, 4) == 3 and R.ksize(512, 256) == 5 and R.ksize(299, 64) == 11
    assert R.coefficients(1, 4)[1].tolist() == [1, 1, 1, 1]


@pytest.mark.parametrize('pair', R.axis_pairs(), ids=lambda p: '%d-%d' % p)
def test_the_table_builder_gives_the_restatements_taps(pair):
    from hoig_amd import _lib as L
    from hoig_amd.metrics import kernels as K
    n_in, n_out = pair
    xmin, n, k = R.coefficients(n_in, n_out)
    assert L.lib.hoig_pil_bilinear_ksize(n_in, n_out) == R.ksize(n_in, n_out) == k.shape[1]
    table = K.pil_table_host(n_in, n_out)
    assert table.shape == (n_out, 2 + k.shape[1]) and table.dtype == np.int32
    assert np.array_equal(table[:, 0], xmin) and np.array_equal(table[:, 1], n)
    assert np.array_equal(table[:, 2:], k)
    assert (table[:, 2:] >= 0).all() and (255 * table[:, 2:].astype(np.int64).sum(1) + (1 << 21) < 2 ** 31).all()


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_the_host_twin_equals_pillow_every_byte(case):
    (h, w), size = case
    for binary in (False, True):
        a = R.content(3, h, w, h * 17 + w, binary)
        assert np.array_equal(host_resize(a, size), R.pillow(a, size)), binary


def test_the_host_twin_equals_pillow_on_the_chain():
    (h, w), mid, side = R.CHAIN
    a = R.content(3, h, w, 9)
    want = R.pillow(R.pillow(a, (mid, mid)), (side, side))
    assert np.array_equal(host_resize(host_resize(a, (mid, mid)), (side, side)), want)


def test_invalid_arguments_are_refused():
    from hoig_amd import _lib as L
    src, dst = np.zeros((1, 8, 8, 4), np.uint8), np.zeros((1, 4097, 8, 4), np.uint8)
    host = L.lib.hoig_resize_pil_bilinear_u8_host
    assert host(_p(src), 1, 8, 8, 4, _p(dst), 8, 8) == L.EINVAL                # C = 4
    assert host(_p(src), 1, 8, 8, 3, _p(dst), 0, 8) == L.EINVAL                # size 0
    assert host(_p(src), 1, 8, 0, 3, _p(dst), 8, 8) == L.EINVAL
    assert host(_p(src), 1, 8, 8, 3, _p(dst), 8, 4097) == L.EINVAL             # size 4097
    assert host(_p(src), 1, 4097, 8, 3, _p(dst), 8, 8) == L.EINVAL
    assert host(_p(src), 1, 8, 8, 3, _p(dst), 4, 4) == L.OK
    # the device entry and its helpers check before any launch
    dev, ws = L.lib.hoig_resize_pil_bilinear_u8, L.lib.hoig_resize_pil_bilinear_u8_workspace_bytes
    for args in ((1, 8, 8, 4, 8, 8), (1, 8, 8, 3, 0, 8), (1, 8, 8, 3, 8, 4097), (1, 4097, 8, 3, 8, 8), (1, 8, 0, 3, 8, 8)):
        B, H, W, C, Ho, Wo = args
        assert ws(*args) == L.EINVAL
        assert dev(_p(src), B, H, W, C, _p(dst), Ho, Wo, None, None, None, None) == L.EINVAL
    assert ws(2, 8, 8, 3, 8, 4) == 0 and ws(2, 8, 8, 3, 4, 8) == 0 and ws(2, 8, 8, 3, 4, 4) == 2 * 8 * 4 * 3
    assert L.lib.hoig_pil_bilinear_ksize(0, 8) == L.EINVAL and L.lib.hoig_pil_bilinear_ksize(8, 4097) == L.EINVAL
    assert L.lib.hoig_pil_bilinear_table(8, 0, _p(src)) == L.EINVAL


def test_the_host_twin_under_a_host_address_sanitizer_build(tmp_path):
    """The table builder and the twin built with -fsanitize=address, every buffer a heap block of exactly its size
    (tests/pil_resize_asan_driver.cpp, a program of its own): no report, and the bytes of the library's twin."""
    import shutil
    cxx = shutil.which(os.environ.get('CXX', 'c++'))
    flags = ['-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address', '-static-libasan']
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    if cxx is None or subprocess.run([cxx] + flags + [str(probe), '-o', str(tmp_path / 'probe')], stdout=subprocess.DEVNULL,
                                     stderr=subprocess.DEVNULL).returncode != 0:
        pytest.skip('no host C++ compiler that links an AddressSanitizer runtime (an empty program does not build with %s)' % ' '.join(flags))
    exe = str(tmp_path / 'pil_resize_asan_driver')
    src = [os.path.join(ROOT, 'hoig_amd', 'csrc', 'pil_resize_host.cpp'), os.path.join(ROOT, 'tests', 'pil_resize_asan_driver.cpp')]
    build = subprocess.run([cxx] + flags + ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'hoig_amd', 'csrc')] + src +
                           ['-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    cases = R.CASES + [((7, 5), (1, 1)), ((3, 1000), (9, 2))]
    args, want = [], []
    for (h, w), (ho, wo) in cases:
        args += [h, w, ho, wo]
        i = np.arange(2 * h * w * 3, dtype=np.uint64)
        a = (((i * 2654435761 + (h * 31 + w)) & 0xFFFFFFFF) >> 24).astype(np.uint8).reshape(2, h, w, 3)
        fnv = 2166136261
        for v in host_resize(a, (ho, wo)).reshape(-1).tolist():
            fnv = ((fnv ^ v) * 16777619) & 0xFFFFFFFF
        want.append('0 %d' % fnv)
    run = subprocess.run([exe, '2'] + [str(v) for v in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0 and 'AddressSanitizer' not in run.stdout, run.stdout[-3000:]
    assert run.stdout.split('\n')[:len(want)] == want
