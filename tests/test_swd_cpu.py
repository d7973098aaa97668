"""The sliced Wasserstein distance through its CPU twins (hoig_amd/csrc/swd_host.cpp, the inline functions of swd.h; docs/swd.md):
every check of tests/swd_reference.py on device 'cpu', and the twins in a program of their own under a host sanitizer.
tests/test_swd_gpu.py runs the same checks on the kernels and compares them with these twins bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import swd_reference as R

DEV = 'cpu'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_binding_declares_the_swd():
    from hoig_amd import _lib as L
    names = set(L.declared_symbols())
    for stem in ('hoig_swd_positions', 'hoig_swd_descriptors_u8', 'hoig_swd_channel_stats_f64', 'hoig_swd_project_f32',
                 'hoig_sort_segments_f32', 'hoig_swd_sorted_l1_f64'):
        for sym in (stem, stem + '_host'):
            assert sym in names and hasattr(L.lib, sym)
    assert L.SORT_LDS_MAX >= 64 and L.SORT_TILE >= 64 and L.lib.hoig_swd_levels(256, 256) == 5 and L.lib.hoig_swd_levels(15, 99) == 0


@pytest.mark.parametrize('case', R.PYRAMID_CASES, ids=lambda c: '%dx%d' % c[:2])
def test_pyramid_and_descriptors_against_scipy(case):
    R.check_descriptors(DEV, case)


def test_descriptors_do_not_depend_on_the_split_of_the_stream():
    R.check_split(DEV)


@pytest.mark.parametrize('rows', R.STAT_ROWS)
def test_channel_statistics_against_longdouble(rows):
    R.check_stats(DEV, rows)


def test_a_constant_channel_is_a_status_and_a_value_error():
    R.check_degenerate(DEV)


@pytest.mark.parametrize('dirs', R.PROJ_DIRS)
@pytest.mark.parametrize('rows', R.PROJ_ROWS)
def test_projection_on_exact_integers_and_within_the_bound(rows, dirs):
    R.check_project_exact(DEV, rows, dirs)
    R.check_project(DEV, rows, dirs)


@pytest.mark.parametrize('i', range(12))
def test_sort_equals_numpy_at_every_edge_size(i):
    n = R.sort_sizes()[i]
    for j, kind in enumerate(R.SORT_KINDS):
        R.check_sort(DEV, (1, 3)[(i + j) % 2], n, kind)


@pytest.mark.parametrize('case', R.SORT_LARGE, ids=lambda c: '%dx%d-%s' % c)
def test_sort_of_many_and_of_long_segments(case):
    R.check_sort(DEV, *case)


def test_sort_nan_is_a_status_and_unaligned_keys_are_sorted():
    from hoig_amd import _lib as L
    for n in (100, L.SORT_TILE + 904):
        R.check_sort_nan(DEV, n)
        R.check_sort_unaligned(DEV, n)


@pytest.mark.parametrize('N', R.L1_SIZES)
def test_sorted_l1(N):
    R.check_l1_exact(DEV, N)
    R.check_l1(DEV, N)


def test_end_to_end_against_the_float64_reference():
    R.check_end_to_end(DEV)


def test_argument_errors():
    R.check_argument_errors(DEV)


def test_the_command_line_knows_the_metric():
    from hoig_amd.metrics.__main__ import parser
    a = parser().parse_args(['swd', 'a', 'b', '--swd-patches', '5', '--swd-repeats', '2', '--swd-dirs', '8', '--swd-levels', '2',
                             '--swd-seed', '3'])
    assert (a.metric, a.swd_patches, a.swd_repeats, a.swd_dirs, a.swd_levels, a.swd_seed) == ('swd', 5, 2, 8, 2, 3)
    d = parser().parse_args(['swd', 'a', 'b'])
    assert (d.swd_patches, d.swd_repeats, d.swd_dirs, d.swd_levels, d.swd_seed) == (128, 4, 128, None, 0)


def test_the_twins_under_a_host_sanitizer_build(tmp_path):
    """swd_host.cpp built with -fsanitize=address,undefined into a program of its own (tests/swd_asan_driver.cpp), every buffer a heap
    block of exactly its size, over the smallest shapes and the sort's edge sizes: no report, and the library's twins' results."""
    from hoig_amd import _lib as L
    from hoig_amd.metrics import swd as S
    # (the compiler, the flags and the reasons for them: tests/test_grad_guard_cpu.py)
    cxx = shutil.which(os.environ.get('CXX', 'c++'))
    assert cxx is not None, 'no host C++ compiler (c++, or $CXX) on PATH'
    flags = ['-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
             '-static-libasan']
    exe = str(tmp_path / 'swd_asan_driver')
    src = [os.path.join(ROOT, 'hoig_amd', 'csrc', 'swd_host.cpp'), os.path.join(ROOT, 'tests', 'swd_asan_driver.cpp')]
    build = subprocess.run([cxx] + flags + ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'hoig_amd', 'csrc')] + src +
                           ['-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    sizes = [1, 2, 65, L.SORT_LDS_MAX, L.SORT_LDS_MAX + 1, L.SORT_TILE + 1]
    for H, W, levels in ((16, 16, 1), (32, 48, 2)):
        run = subprocess.run([exe, str(H), str(W), str(levels)] + [str(n) for n in sizes], stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True, timeout=120)
        assert run.returncode == 0 and 'Sanitizer' not in run.stdout and 'runtime error' not in run.stdout, run.stdout[-3000:]
        out = run.stdout.split('\n')
        assert out[0] == '0', run.stdout[:500]
        # the driver's images: pixel (i, y, x, c) = (i * 53 + y * 31 + x * 17 + c * 101 + ((x * y) % 7) * 9) % 256; 2 images, 3 patches, seed 11
        i, y, x, c = np.meshgrid(np.arange(2), np.arange(H), np.arange(W), np.arange(3), indexing='ij')
        u8 = ((i * 53 + y * 31 + x * 17 + c * 101 + ((x * y) % 7) * 9) % 256).astype(np.uint8)
        rows = S.laplacian_descriptors_u8(u8, levels, 3, 11, 1, 4)
        stats, status = S.channel_stats(rows[levels - 1])
        d = np.fromfunction(lambda k, j: ((k * 7 + j * 3) % 11 - 5) / 8.0, (147, 2)).astype(np.float32)
        proj = S.project(rows[levels - 1], stats, R.to(DEV, d))
        S.sort_segments(proj)
        want = [float(rows[lv].double().sum()) for lv in range(levels)] + stats.numpy().ravel().tolist() + \
               [float(S.sorted_l1(proj[0], proj[1])[0]), float(proj[0, 0]), float(proj[1, -1])]
        got = [float.fromhex(v) for v in out[1].split()]
        assert int(status[0]) == 0 and got == want
        assert out[2].split() == ['1'] * len(sizes)             # every sort came out ascending with its multiset kept


def test_the_philox_restatement_gives_the_published_vectors():
    """The positions are held to a restatement of Philox4x32-10 in Python integers; the restatement is held to the known-answer vectors
    of Random123 (kat_vectors: counter and key all zeros, all ones)."""
    assert R.philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert R.philox4x32_10((0,) * 4, (0,) * 2) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
