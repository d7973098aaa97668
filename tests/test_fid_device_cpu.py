"""The fp64 FID statistics through their CPU twins (hoig_amd/csrc/fid_stats_host.cpp, the per-lane code of fid_stats.h): the checks,
truths and limits of tests/fid_device_reference.py on device 'cpu'.  tests/test_fid_device_gpu.py runs the same ones on the kernels."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import fid_device_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_p = lambda a: ctypes.c_void_p(a.ctypes.data)


@pytest.mark.parametrize('shape,f32,accumulate,symmetric', R.GEMM_CASES, ids=R.gemm_id)
def test_gemm_twin_against_longdouble(shape, f32, accumulate, symmetric):
    R.check_gemm('cpu', shape, f32, accumulate, symmetric)


def test_moments_twin_against_mean_and_cov():
    R.check_moments('cpu')


def test_pivoted_cholesky_twin():
    R.check_pchol('cpu')


@pytest.mark.parametrize('name', sorted(R.eig_matrices()))
def test_eigenvalue_twin_against_eigvalsh(name):
    R.check_eigvals('cpu', name, R.eig_matrices()[name])


@pytest.mark.parametrize('case', R.TRACE_CASES, ids=lambda c: '%d-%d' % c)
def test_trace_twin_against_mpmath(case):
    R.check_trace('cpu', case)


def test_trace_twin_closed_form_2048():
    R.check_closed_form('cpu')


def test_frechet_distance_twin_and_the_eps_branch():
    """The whole formula, from numpy arrays and from tensors; and on (2, 2), the rank-1 case in which the reference may take its 1e-6
    branch: the twin gives the value of the formula itself."""
    from hoig_amd.metrics.fid_device import frechet_distance_host_twin
    m1, s1, m2, s2 = R.case_statistics((200, 200))
    got = frechet_distance_host_twin(m1, s1, m2, s2)
    want = (m1 - m2).dot(m1 - m2) + np.trace(s1) + np.trace(s2) - 2 * R.trace_truth((200, 200))
    assert abs(got - want) <= 2 * R.trace_limit((200, 200)) * R.trace_truth((200, 200)) + 8 * 2.0 ** -52 * (np.trace(s1) + np.trace(s2))
    assert got == frechet_distance_host_twin(torch.from_numpy(m1), torch.from_numpy(s1), m2, s2)
    m1, s1, m2, s2 = R.case_statistics((2, 2))
    got = frechet_distance_host_twin(m1, s1, m2, s2)
    want = (m1 - m2).dot(m1 - m2) + np.trace(s1) + np.trace(s2) - 2 * R.trace_truth((2, 2))
    assert abs(got - want) <= 2 * R.trace_limit((2, 2)) * R.trace_truth((2, 2)) + 8 * 2.0 ** -52 * (np.trace(s1) + np.trace(s2))


def test_status_codes_leave_the_outputs_untouched():
    from hoig_amd import _lib as L
    from hoig_amd.metrics import fid_device as F
    lib = L.lib
    a, c = np.ones((4, 3)), np.full((3, 3), 5.0)
    gemm = lib.hoig_gemm_tn_f64_host
    assert gemm(_p(a), 2, _p(a), 3, None, _p(c), 3, 3, 3, 4, 0) == L.EINVAL                     # lda below the row length
    assert gemm(_p(a), 3, _p(a), 3, None, _p(c), 2, 3, 3, 4, 0) == L.EINVAL                     # ldc below it
    assert gemm(_p(a), 3, _p(a), 3, None, _p(c), 3, 0, 3, 4, 0) == L.EINVAL                     # M = 0
    assert gemm(_p(a), 3, _p(a), 3, None, _p(c), 3, 3, 3, 4, 8) == L.EINVAL                     # an unknown flag
    assert gemm(_p(a), 3, _p(c), 3, None, _p(c), 3, 3, 3, 3, L.GEMM_SYMMETRIC) == L.EINVAL      # symmetric with A != B
    assert gemm(_p(a), 3, _p(a), 3, _p(c), _p(c), 3, 3, 3, 4, 0) == L.EINVAL                    # a pivot on fp64 operands
    assert gemm(None, 3, _p(a), 3, None, _p(c), 3, 3, 3, 4, 0) == L.EINVAL
    assert (c == 5.0).all()
    # the device entries refuse the same before any launch
    assert lib.hoig_gemm_tn_f64(_p(a), 2, _p(a), 3, None, _p(c), 3, 3, 3, 4, 0, None) == L.EINVAL
    assert lib.hoig_pchol_f64(_p(c), 2, 3, _p(c), 3, _p(c), _p(c), _p(c), 1 << 20, None) == L.EINVAL
    assert lib.hoig_pchol_f64(_p(c), 3, 3, _p(c), 3, _p(c), _p(c), _p(c), 8, None) == L.EINVAL              # workspace too small
    assert lib.hoig_sym_eigvals_f64(_p(c), 3, 3, _p(c), _p(c), _p(c), 8, None) == L.EINVAL
    assert lib.hoig_pchol_f64_workspace_bytes(0) == L.EINVAL and lib.hoig_sym_eigvals_f64_workspace_bytes(0) == L.EINVAL
    assert lib.hoig_pchol_f64_workspace_bytes(64) == 32 + 2 * 64 * 8
    # a non-finite entry: the status, and L, piv, the rank and lambda as they were
    for bad in (np.nan, np.inf):
        s = np.eye(3)
        s[1, 2] = bad
        fac, piv, info = np.full((3, 3), 5.0), np.full(3, 9, np.int32), np.array([7, 0], np.int32)
        assert lib.hoig_pchol_f64_host(_p(s), 3, 3, _p(fac), 3, _p(piv), _p(info)) == L.EINVAL
        assert (fac == 5.0).all() and (piv == 9).all() and info.tolist() == [7, L.EINVAL]
        lam, einfo = np.full(3, 5.0), np.zeros(1, np.int32)
        assert lib.hoig_sym_eigvals_f64_host(_p(s), 3, 3, _p(lam), _p(einfo)) == L.EINVAL
        assert (lam == 5.0).all() and einfo.tolist() == [L.EINVAL]
        with pytest.raises(ValueError):
            F.frechet_distance_host_twin(np.zeros(3), s, np.zeros(3), np.eye(3))
    assert lib.hoig_pchol_f64_host(_p(c), 2, 3, _p(c), 3, _p(c), _p(c)) == L.EINVAL
    with pytest.raises(ValueError):
        F.frechet_distance_host_twin(np.zeros(3), np.eye(3), np.zeros(4), np.eye(4))
    with pytest.raises(ValueError):
        F.frechet_distance_host_twin(np.zeros(3), np.eye(3), np.zeros(3), np.eye(4))
    with pytest.raises(ValueError):
        F.Moments(4, 'cpu').update(torch.zeros((2, 5)))
    with pytest.raises(ValueError):
        F.Moments(4, 'cpu').update(torch.zeros((2, 4), dtype=torch.float64))


def test_the_option_is_off_by_default(monkeypatch):
    import inspect
    from hoig_amd.metrics import fid, stream
    from hoig_amd.metrics.fid_device import fid_device_option
    monkeypatch.delenv('HOIG_DEVICE_FID', raising=False)
    assert fid_device_option(None) is False and fid_device_option(True) is True
    monkeypatch.setenv('HOIG_DEVICE_FID', '1')
    assert fid_device_option(None) is True and fid_device_option(False) is False
    assert inspect.signature(stream.Scorer.__init__).parameters['fid_device'].default is None
    for f in (fid.calculate_activation_statistics, fid.compute_statistics_of_path, fid.calculate_fid_given_paths):
        assert inspect.signature(f).parameters['device_stats'].default is None
    assert 'device_stats' not in inspect.signature(fid.get_activations).parameters


def test_the_twins_under_a_host_address_sanitizer_build(tmp_path):
    """fid_stats_host.cpp built with -fsanitize=address into a program of its own (tests/fid_stats_asan_driver.cpp), every buffer a heap
    block of exactly its size: no report, and the library's twin's results."""
    import shutil
    from hoig_amd import _lib as L
    cxx = shutil.which(os.environ.get('CXX', 'c++'))
    flags = ['-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address', '-static-libasan']
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    if cxx is None or subprocess.run([cxx] + flags + [str(probe), '-o', str(tmp_path / 'probe')], stdout=subprocess.DEVNULL,
                                     stderr=subprocess.DEVNULL).returncode != 0:
        pytest.skip('no host C++ compiler that links an AddressSanitizer runtime (an empty program does not build with %s)' % ' '.join(flags))
    exe = str(tmp_path / 'fid_stats_asan_driver')
    src = [os.path.join(ROOT, 'hoig_amd', 'csrc', 'fid_stats_host.cpp'), os.path.join(ROOT, 'tests', 'fid_stats_asan_driver.cpp')]
    build = subprocess.run([cxx] + flags + ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'hoig_amd', 'csrc')] + src +
                           ['-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    K, M, N = 130, 39, 24
    run = subprocess.run([exe, str(K), str(M), str(N)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0 and 'AddressSanitizer' not in run.stdout, run.stdout[-3000:]
    # the driver's operands and calls, restated on the library's twins
    x = lambda rows, cols: ((np.arange(rows)[:, None] * 31 + np.arange(cols)[None, :] * 17) % 23 - 11) / 8.0

    def fnv(arr):
        h = 2166136261
        for v in arr.tobytes():
            h = ((h ^ v) * 16777619) & 0xFFFFFFFF
        return h

    def factor_and_eigenvalues(suffix, g):
        n = g.shape[0]
        fac, piv, info = np.zeros((n, n)), np.zeros(n, np.int32), np.zeros(2, np.int32)
        lam, einfo = np.zeros(n), np.zeros(1, np.int32)
        assert L.lib.hoig_pchol_f64_host(_p(g), n, n, _p(fac), n, _p(piv), _p(info)) == 0
        assert L.lib.hoig_sym_eigvals_f64_host(_p(g), n, n, _p(lam), _p(einfo)) == 0
        return ['pchol%s 0 %d %d' % (suffix, info[0], fnv(fac)), 'eig%s 0 %d' % (suffix, fnv(lam))], int(info[0])

    a, b = x(K, M), x(K, N)
    c, g = np.zeros((M, N)), np.zeros((N, N))
    assert L.lib.hoig_gemm_tn_f64_host(_p(a), M, _p(b), N, None, _p(c), N, M, N, K, 0) == 0
    assert L.lib.hoig_gemm_tn_f64_host(_p(c), N, _p(c), N, None, _p(g), N, N, N, M, L.GEMM_SYMMETRIC) == 0
    lines, _ = factor_and_eigenvalues('', g)
    lines1, rank1 = factor_and_eigenvalues('1', np.outer(np.arange(1.0, 6.0), np.arange(1.0, 6.0)))
    assert rank1 == 1
    want = ['gemm 0 %d' % fnv(c), 'gram 0 %d' % fnv(g)] + lines + lines1
    assert run.stdout.split('\n')[:len(want)] == want
