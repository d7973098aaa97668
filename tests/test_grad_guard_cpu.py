"""The gradient guard's statistics and decision through their CPU twins (hoig_amd/csrc/grad_guard_host.cpp, the per-lane code of
grad_guard.h): the cases, truths and limits of tests/grad_guard_reference.py on device 'cpu'.  tests/test_grad_guard_gpu.py runs the
same ones on the kernels."""
import pytest

import grad_guard_reference as R

CASES = R.cases()


@pytest.mark.parametrize('nonfinite', [False, True], ids=['finite', 'nonfinite'])
@pytest.mark.parametrize('n,tname', [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_stats_twin_against_fsum(n, tname, nonfinite):
    R.check_stats('cpu', n, tname, nonfinite)


def test_stats_twin_does_not_depend_on_alignment():
    R.check_misaligned('cpu')


@pytest.mark.parametrize('name', sorted(R.REFUSED))
def test_stats_twin_refuses_and_leaves_the_outputs(name):
    R.check_refused('cpu', name)


def test_decide_twin_is_the_formula():
    R.check_decide('cpu')


def test_the_binding_declares_the_guard():
    from hoig_amd import _lib as L
    names = set(L.declared_symbols())
    for sym in ('hoig_grad_stats', 'hoig_grad_stats_host', 'hoig_grad_stats_workspace_bytes', 'hoig_guard_decide', 'hoig_guard_decide_host',
                'hoig_adam_tick_guarded', 'hoig_adam_step_dev_guarded', 'hoig_adam_pack_step_guarded'):
        assert sym in names and hasattr(L.lib, sym)
    assert R.CH % 1024 == 0 and R.BIG > R.GRID * R.CH


def test_the_twins_under_a_host_sanitizer_build(tmp_path):
    """grad_guard_host.cpp built with -fsanitize=address,undefined into a program of its own (tests/grad_guard_asan_driver.cpp), every
    buffer a heap block of exactly its size, over the odd tables of the reference: no report, and the library's twin's results."""
    import ctypes
    import os
    import shutil
    import subprocess
    import numpy as np
    from hoig_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # A host C++ compiler with the sanitizer runtimes is part of what this suite runs on, like hipcc: its absence is a failure here,
    # not a skip -- this is the only memory-safety check the twins have.
    # -static-libasan: the driver must run wherever the suite runs, also in a process environment that preloads a library of its own;
    # the shared ASan runtime refuses to start unless it comes first in the library list, the static one is part of the program.
    # (GCC's spelling; the flags are GCC's, and the compiler is the system's `c++` unless CXX names another GCC.)
    cxx = shutil.which(os.environ.get('CXX', 'c++'))
    assert cxx is not None, 'no host C++ compiler (c++, or $CXX) on PATH'
    flags = ['-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
             '-static-libasan']
    exe = str(tmp_path / 'grad_guard_asan_driver')
    src = [os.path.join(root, 'hoig_amd', 'csrc', 'grad_guard_host.cpp'), os.path.join(root, 'tests', 'grad_guard_asan_driver.cpp')]
    build = subprocess.run([cxx] + flags + ['-I' + os.path.join(root, 'include'), '-I' + os.path.join(root, 'hoig_amd', 'csrc')] + src +
                           ['-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    for n in (1, 3, 257, R.CH - 1, R.CH + 1, 3 * R.CH + 5):
        for tname, rows in R.tables(n).items():
            if tname == 'ones' and n > 4:
                continue
            args = [str(n)] + [str(v) for row in rows for v in row]
            run = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
            assert run.returncode == 0 and 'Sanitizer' not in run.stdout and 'runtime error' not in run.stdout, run.stdout[-3000:]
            out = run.stdout.split('\n')
            assert int(out[0]) == 0
            got = np.array([[float.fromhex(v) for v in line.split()] for line in out[1:2 + len(rows)]])
            i = np.arange(n, dtype=np.int64)
            x = (((i * 37 + 11) % 41) - 20).astype(np.float32) * np.float32(0.125)
            x[i % 97 == 5] = np.inf
            x[i % 101 == 3] = np.nan
            rc, total, seg = R.run_stats('cpu', x, rows)
            assert rc == 0 and got[0].tobytes() == total.tobytes() and got[1:].tobytes() == seg.tobytes(), (n, tname)
    bad = subprocess.run([exe, '100', '50', '10', '10', '10'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert bad.returncode == 0 and bad.stdout.split('\n')[0] == str(L.EINVAL) and 'Sanitizer' not in bad.stdout
