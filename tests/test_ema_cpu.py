"""The weight EMA through its CPU twins (hoig_amd/csrc/ema_host.cpp, the inline functions of ema.h; docs/ema.md): the update against
numpy's fp32 arithmetic and the schedule against Python doubles, both bit for bit; the fp32 recurrence against a float64 one within
the derived bound; the twins in a program of their own under a host sanitizer; the options.  tests/test_ema_gpu.py compares the
kernels with these twins."""
import types

import numpy as np
import pytest

import ema_reference as R


def test_the_binding_declares_the_ema():
    from hoig_amd import _lib as L
    names = set(L.declared_symbols())
    for sym in ('hoig_ema_tick', 'hoig_ema_tick_host', 'hoig_ema_update', 'hoig_ema_update_host', 'hoig_swap_f32'):
        assert sym in names and hasattr(L.lib, sym)


@pytest.mark.parametrize('n', R.SIZES)
def test_update_twin_is_numpy_fp32_arithmetic(n):
    """Twenty chained updates, schedule and all: every average is numpy's e + (p - e) * w with each operation rounded to fp32."""
    rng = np.random.default_rng(1000 + n)
    ema = R.aligned_f32(n, R.values(rng, n))
    want = ema.copy()
    state = np.array([0.999, 1.0, 0.0], dtype=np.float64)
    derived = np.zeros(1, dtype=np.float32)
    for k in range(20):
        param = R.aligned_f32(n, R.values(rng, n))
        keep = param.copy()
        assert R.tick_host(state, derived) == 0
        assert R.update_host(ema, param, n, derived) == 0
        w, _ = R.py_tick(0.999, True, float(k))
        want = R.numpy_update(want, param, w)
        assert np.isfinite(want).all() and (np.abs(want[want != 0]) >= np.finfo(np.float32).tiny).all()
        assert ema.tobytes() == want.tobytes(), (n, k)
        assert param.tobytes() == keep.tobytes()
    assert state[2] == 20.0


@pytest.mark.parametrize('warmup', [True, False], ids=['warmup', 'flat'])
@pytest.mark.parametrize('decay', R.DECAYS)
def test_tick_twin_is_the_schedule_in_python_doubles(decay, warmup):
    state = np.array([decay, 1.0 if warmup else 0.0, 0.0], dtype=np.float64)
    derived = np.zeros(1, dtype=np.float32)
    skip = np.array([1.0, 1.0], dtype=np.float32)
    go = np.array([0.25, 0.0], dtype=np.float32)
    for t in range(41):
        before = state.tobytes(), derived.tobytes()
        assert R.tick_host(state, derived, skip) == 0
        assert (state.tobytes(), derived.tobytes()) == before           # a skipped step: nothing moves
        assert R.tick_host(state, derived, go if t % 2 else None) == 0
        w, count = R.py_tick(decay, warmup, float(t))
        assert derived[0] == w and derived.tobytes() == np.array([w]).tobytes()
        assert state[2] == count and state[0] == decay and state[1] == (1.0 if warmup else 0.0)
    if warmup and decay > 0.5:
        assert derived[0] > np.float32(1.0 - decay)                     # (still on the ramp at t = 40: 41 / 50 < decay)


def test_twins_refuse_and_leave_the_outputs():
    from hoig_amd import _lib as L
    n = 8
    ema, param = R.aligned_f32(n, 1.0), R.aligned_f32(n, 2.0)
    derived = np.array([0.5], dtype=np.float32)
    big = R.aligned_f32(n + 4, 3.0)
    cases = [(None, param, n), (ema, None, n), (ema, param, 0), (ema, param, -1), (ema, ema, n), (big[1:], param, n), (ema, big[1:], n),
             (big[:n], big[4:], n)]
    for e, p, cnt in cases:
        assert R.update_host(e, p, cnt, derived) == L.EINVAL
    assert R.update_host(ema, param, n, None) == L.EINVAL
    assert (ema == 1.0).all() and (param == 2.0).all() and (big == 3.0).all()
    assert R.tick_host(None, derived) == L.EINVAL and R.tick_host(np.zeros(3), None) == L.EINVAL


@pytest.mark.parametrize('decay,warmup', [(0.999, True), (0.9, False)], ids=['warmup', 'flat'])
def test_fp32_average_stays_within_the_bound_of_a_float64_recurrence(decay, warmup):
    """After K updates |ema_fp32 - ema_fp64| <= 8 K 2^-24 M, M the largest |param| or |ema| seen.  Per update: the sum rounds once
    (<= 2^-24 M); the difference and the product round once each (<= 2 * 2^-24 |p - e| <= 4 * 2^-24 M); the fp32 cast of 1 - beta moves
    the product by <= 2^-24 |p - e| <= 2 * 2^-24 M; what was there before is carried with a factor beta < 1.  Seven units per update;
    eight are allowed."""
    K, n = 50, 4099
    rng = np.random.default_rng(7)
    ema = R.aligned_f32(n, R.values(rng, n))
    ema64 = ema.astype(np.float64)
    M = float(np.abs(ema).max())
    state = np.array([decay, 1.0 if warmup else 0.0, 0.0], dtype=np.float64)
    derived = np.zeros(1, dtype=np.float32)
    for k in range(K):
        param = R.aligned_f32(n, R.values(rng, n))
        beta = min(decay, (1.0 + k) / (10.0 + k)) if warmup else decay
        assert R.tick_host(state, derived) == 0 and R.update_host(ema, param, n, derived) == 0
        ema64 = ema64 + (param.astype(np.float64) - ema64) * (1.0 - beta)
        M = max(M, float(np.abs(param).max()), float(np.abs(ema).max()), float(np.abs(ema64).max()))
    err = float(np.abs(ema.astype(np.float64) - ema64).max())
    bound = 8 * K * 2.0 ** -24 * M
    print('K = %d: max |fp32 - fp64| = %.3e, bound %.3e (M = %.4f)' % (K, err, bound, M))
    assert err <= bound


def test_the_twins_under_a_host_sanitizer_build(tmp_path):
    """ema_host.cpp built with -fsanitize=address,undefined into a program of its own (tests/ema_asan_driver.cpp), every buffer a heap
    block of exactly its size, over the odd sizes: no report, and the library's twin's results."""
    import os
    import shutil
    import subprocess
    from hoig_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # (the compiler, the flags and the reasons for them: tests/test_grad_guard_cpu.py)
    cxx = shutil.which(os.environ.get('CXX', 'c++'))
    assert cxx is not None, 'no host C++ compiler (c++, or $CXX) on PATH'
    flags = ['-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
             '-static-libasan']
    exe = str(tmp_path / 'ema_asan_driver')
    src = [os.path.join(root, 'hoig_amd', 'csrc', 'ema_host.cpp'), os.path.join(root, 'tests', 'ema_asan_driver.cpp')]
    build = subprocess.run([cxx] + flags + ['-I' + os.path.join(root, 'include'), '-I' + os.path.join(root, 'hoig_amd', 'csrc')] + src +
                           ['-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    K = 6
    for n in R.SIZES:
        run = subprocess.run([exe, str(n), str(K)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert run.returncode == 0 and 'Sanitizer' not in run.stdout and 'runtime error' not in run.stdout, run.stdout[-3000:]
        out = run.stdout.split('\n')
        assert int(out[0]) == 0
        count, w = (float.fromhex(v) for v in out[1].split())
        got = np.array([float.fromhex(v) for v in out[2:2 + n]], dtype=np.float32)
        i = np.arange(n, dtype=np.int64)
        ema = R.aligned_f32(n, (((i * 17 + 3) % 29) - 14).astype(np.float32) * np.float32(0.0625))
        state = np.array([0.999, 1.0, 0.0], dtype=np.float64)
        derived = np.zeros(1, dtype=np.float32)
        for k in range(K):
            param = R.aligned_f32(n, (((i * 37 + 11 + 13 * k) % 41) - 20).astype(np.float32) * np.float32(0.03125))
            assert R.tick_host(state, derived) == 0 and R.update_host(ema, param, n, derived) == 0
        assert count == state[2] == K and np.float32(w) == derived[0]
        assert got.tobytes() == ema.tobytes(), n
    bad = subprocess.run([exe, '0', '1'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert bad.returncode == 0 and bad.stdout.split('\n')[0] == str(L.EINVAL) and 'Sanitizer' not in bad.stdout


# ------------------------------------------------------------------------------------------------ options (host only)
def _opt(**kw):
    return types.SimpleNamespace(**kw)


def test_options_parse():
    from hoig_amd.ema import parse_options
    assert parse_options(_opt(), True, {}) == (None, True, False)
    assert parse_options(_opt(ema_decay=0), True, {}) == (None, True, False)
    assert parse_options(_opt(ema_decay=None), True, {'HOIG_EMA_DECAY': ''}) == (None, True, False)
    assert parse_options(_opt(ema_decay=0.999, ema_warmup=False), True, {}) == (0.999, False, False)
    assert parse_options(_opt(), True, {'HOIG_EMA_DECAY': '0.99', 'HOIG_EVAL_EMA': '1'}) == (0.99, True, True)
    assert parse_options(_opt(ema_decay='0.5', eval_ema=False), True, {'HOIG_EVAL_EMA': '1'}) == (0.5, True, False)
    assert parse_options(_opt(ema_decay=0.9), True, {'HOIG_EMA_DECAY': '0.5'}) == (0.9, True, False)       # (the option wins)
    assert parse_options(_opt(eval_ema=True), False, {}) == (None, True, True)      # eval-only: the saved average is loaded as G


@pytest.mark.parametrize('bad', [1.0, -0.1, 'x', 1.5, float('nan'), True])
def test_options_refuse_a_decay_outside_the_open_interval(bad):
    from hoig_amd.ema import parse_options
    with pytest.raises(ValueError, match='ema_decay'):
        parse_options(_opt(ema_decay=bad), True, {})
    if isinstance(bad, (float, str)) and not isinstance(bad, bool):
        with pytest.raises(ValueError, match='ema_decay'):
            parse_options(_opt(), True, {'HOIG_EMA_DECAY': str(bad)})


def test_options_refuse_eval_ema_on_a_training_model_without_a_decay():
    from hoig_amd.ema import parse_options
    with pytest.raises(ValueError, match='eval_ema'):
        parse_options(_opt(eval_ema=True), True, {})
    with pytest.raises(ValueError, match='eval_ema'):
        parse_options(_opt(ema_decay=0.0), True, {'HOIG_EVAL_EMA': '1'})
