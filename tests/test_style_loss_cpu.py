"""The opt-in style (Gram-matrix) term of G through its CPU twin (hoig_amd/csrc/style_loss_host.cpp, the inline functions of
style_loss.h; docs/style_loss.md) against the float64 restatement of tests/style_loss_reference.py, within the bounds the document
derives; identical inputs, null and pre-filled slots, a NaN; the option parser; the entry points' refusals; and the twin in a program of
its own under a host sanitizer.  tests/test_style_loss_gpu.py compares the kernels with this twin."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import style_loss_reference as R

DEV = 'cpu'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ids = lambda v: 'x'.join(str(s) for s in v)


def test_the_binding_declares_the_entry_points():
    from hoig_amd import _lib as L
    names = set(L.declared_symbols())
    for sym in ('hoig_style_gram', 'hoig_style_dfeat', 'hoig_style_workspace_bytes', 'hoig_style_gram_host', 'hoig_style_dfeat_host'):
        assert sym in names and hasattr(L.lib, sym)
    assert R.T % 32 == 0 and R.K % 2 == 0 and (L.STYLE_MAX_N, L.STYLE_MAX_P, L.STYLE_MAX_C) == (4096, 2 ** 22, 512)
    ws = L.lib.hoig_style_workspace_bytes
    # one raw fp32 tile per (image of the 2N, tile pair, chunk) and one double per (image of the N, tile pair)
    tile = R.T * R.T * 4
    assert ws(1, 1, 16) == 2 * tile + 8
    assert ws(8, 16 * 16, 512) == 16 * 36 * tile + 8 * 36 * 8
    assert ws(3, 2 * R.K + 3, R.T + 16) == 6 * 3 * 3 * tile + 3 * 3 * 8
    for bad in ((0, 4, 16), (4097, 4, 16), (1, 0, 16), (1, 2 ** 22 + 1, 16), (1, 4, 0), (1, 4, 8), (1, 4, 24), (1, 4, 528), (-1, -1, -1)):
        assert ws(*bad) < 0, bad


@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'raw'])
@pytest.mark.parametrize('shape', R.SHAPES, ids=_ids)
def test_twin_against_float64(shape, relu):
    x, y = R.case(shape, relu=relu)
    want = R.reference(x, y)
    got = R.run(DEV, x, y)
    rg, rv = R.check(got, want, x, shape)
    # the feature gradient: the chain against float64 Fx S with the twin's own S, and against the reference's signs outside the
    # entries whose sign is not settled
    dfx = R.dfeat(DEV, x, got['S'])
    N, H, W, C = shape
    exact = np.matmul(x.reshape(N, H * W, C).astype(np.float64), got['S'].astype(np.float64)).reshape(shape)
    bound = R.grad_bound(x, got['S'])
    err = np.abs(dfx - exact)
    assert (err <= bound).all()
    rd = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    assert (np.abs(dfx - R.grad_reference(x, want)) <= R.grad_bound(x, got['S'], want['amb'])).all()
    print('style_loss ratio %s %s gram %.4f value %.4f gradient %.4f unsettled %d of %d' % (
        _ids(shape), 'relu' if relu else 'raw', rg, rv, rd, int(want['amb'].sum()), want['amb'].size))


def test_identical_inputs_give_exactly_zero():
    x, _ = R.case((3, 7, 11, R.T + 16))
    got = R.run(DEV, x, x.copy())
    assert got['term'][0] == 0.0 and got['report'][0] == 0.0 and got['S'].tobytes() == bytes(got['S'].nbytes)
    assert got['gram'][:3].tobytes() == got['gram'][3:].tobytes()
    t = torch.from_numpy(x)
    from hoig_amd import style_loss as SL
    S = SL.gram(t, t, 3.0)                               # x is y: the same memory on both sides
    assert S.numpy().tobytes() == bytes(S.numel() * 4)
    assert R.dfeat(DEV, x, S.numpy()).tobytes() == bytes(x.nbytes)


def test_null_slots_and_slots_that_hold_a_value():
    x, y = R.case((1, 1, R.K + 1, R.T + 16), seed=1)
    full = R.run(DEV, x, y)
    none = R.run(DEV, x, y, term=False, report=False, gram=False)
    assert none['S'].tobytes() == full['S'].tobytes() and none['term'] is None and none['gram'] is None
    added = R.run(DEV, x, y, init=0.5)
    assert added['term'][0] == np.float32(0.5) + full['term'][0] and added['report'][0] == np.float32(0.5) + full['report'][0]
    assert added['S'].tobytes() == full['S'].tobytes() and full['term'][0] > 0
    # the scale enters the term and the magnitude of S alone
    other = R.run(DEV, x, y, scale=2.5)
    assert other['report'][0] == full['report'][0] and other['gram'].tobytes() == full['gram'].tobytes()
    assert np.array_equal(np.sign(other['S']), np.sign(full['S'])) and np.abs(other['S']).max() == R.coeff(x.shape, 2.5)
    zero = R.run(DEV, x, y, scale=0.0)
    assert zero['term'][0] == 0.0 and not zero['S'].any() and zero['report'][0] == full['report'][0]


def test_a_nan_feature_gives_a_nan_term_and_finite_signs():
    x, y = R.case((1, 5, 5, 32), seed=2)
    x[0, 2, 3, 7] = np.nan
    got = R.run(DEV, x, y)
    assert np.isnan(got['term'][0]) and np.isnan(got['report'][0]) and np.isfinite(got['S']).all()
    assert not got['S'][0, 7, :].any() and not got['S'][0, :, 7].any() and got['S'].any()


def _slots(n=3):
    class Slots(object):                     # (ops.LossSlots needs the device library's hoig_sum: the layout alone is enough here)
        buf = torch.zeros(n)
    return Slots()


def test_the_autograd_function_on_cpu_tensors():
    from hoig_amd import style_loss as SL
    shape = (3, 7, 11, R.T + 16)
    x, y = R.case(shape, seed=4)
    s = _slots()
    tx = torch.from_numpy(x).requires_grad_(True)
    for _ in range(2):
        out = SL.style_loss(tx, torch.from_numpy(y), R.SCALE, (s, 0), (s, 2))
    out.backward()
    once = R.run(DEV, x, y)
    assert tx.grad.numpy().tobytes() == R.dfeat(DEV, x, once['S']).tobytes()          # (only the last call's graph was differentiated)
    assert s.buf[0] == once['term'][0] + once['term'][0] and s.buf[2] == once['report'][0] + once['report'][0] and s.buf[1] == 0
    # without a report slot, and without a gradient: no gradient work
    s = _slots()
    calls = []
    real = SL.dfeat
    SL.dfeat = lambda *a: (calls.append(1), real(*a))[1]
    try:
        out = SL.style_loss(torch.from_numpy(x), torch.from_numpy(y), R.SCALE, (s, 1))
        assert not out.requires_grad and s.buf[1] == once['term'][0] and s.buf[0] == 0 and s.buf[2] == 0
        w = torch.ones((), requires_grad=True)
        (SL.style_loss(torch.from_numpy(x), torch.from_numpy(y), R.SCALE, (s, 1)) * w).backward()
        assert not calls
        tx.grad = None
        SL.style_loss(tx, torch.from_numpy(y), R.SCALE, (s, 1)).backward()
        assert calls == [1]
    finally:
        SL.dfeat = real
    with pytest.raises(ValueError, match='scale'):
        SL.style_loss(tx, torch.from_numpy(y), float('nan'), (s, 0))


def test_the_python_calls_check_their_tensors():
    from hoig_amd import style_loss as SL
    f = torch.zeros(1, 4, 4, 16)
    with pytest.raises(TypeError):
        SL.gram(f.double(), f.double(), 1.0)
    with pytest.raises(TypeError):
        SL.gram(f[..., ::2], f[..., ::2], 1.0)
    with pytest.raises(ValueError):
        SL.gram(f, f[:, :2], 1.0)
    with pytest.raises(ValueError):
        SL.gram(f, f, 1.0, out_gram=torch.zeros(1, 16, 16, dtype=torch.float64))
    with pytest.raises(ValueError):
        SL.dfeat(f, torch.zeros(1, 16, 8))
    from hoig_amd import _lib as L
    with pytest.raises(L.HoigKernelError, match='unsupported'):
        SL.gram(torch.zeros(1, 4, 4, 24), torch.zeros(1, 4, 4, 24), 1.0)


def test_entry_points_refuse_and_write_nothing():
    from hoig_amd import _lib as L
    N, P, C = 2, 9, 32
    fx, fy = torch.ones(N, P, C), torch.zeros(N, P, C)
    S, d = torch.full((N, C, C), 7.0), torch.full((N, P, C), 7.0)
    slot, gram = torch.full((4,), 7.0), torch.full((2 * N, C, C), 7.0, dtype=torch.float64)
    good = [fx.data_ptr(), fy.data_ptr(), N, P, C, 1.0, S.data_ptr(), slot.data_ptr(), slot.data_ptr() + 4, gram.data_ptr()]
    cases = [(0, None, L.EINVAL), (1, None, L.EINVAL), (6, None, L.EINVAL), (0, fx.data_ptr() + 4, L.EINVAL), (6, S.data_ptr() + 8, L.EINVAL),
             (7, slot.data_ptr() + 2, L.EINVAL), (9, gram.data_ptr() + 8, L.EINVAL), (6, fx.data_ptr(), L.EINVAL),
             (6, fy.data_ptr() + 64, L.EINVAL), (9, fx.data_ptr(), L.EINVAL), (5, float('nan'), L.EINVAL), (5, float('inf'), L.EINVAL),
             (5, -1.0, L.EINVAL), (2, 0, L.EINVAL), (3, 0, L.EINVAL), (4, 0, L.EINVAL), (2, -3, L.EINVAL),
             (2, 4097, L.EUNSUPPORTED), (3, 2 ** 22 + 1, L.EUNSUPPORTED), (4, 8, L.EUNSUPPORTED), (4, 24, L.EUNSUPPORTED),
             (4, 528, L.EUNSUPPORTED)]
    for i, v, rc in cases:
        bad = list(good)
        bad[i] = v
        assert L.lib.hoig_style_gram_host(*bad) == rc, (i, v)
    assert bool((S == 7.0).all()) and bool((slot == 7.0).all()) and bool((gram == 7.0).all())
    assert L.lib.hoig_style_gram_host(*good) == L.OK
    assert float(slot[0]) == 7.0 + 1.0 / C and float(slot[1]) == 7.0 + 1.0 / C and bool((gram[:N] == 1.0 / C).all())
    good = [fx.data_ptr(), S.data_ptr(), N, P, C, d.data_ptr()]
    cases = [(0, None, L.EINVAL), (1, None, L.EINVAL), (5, None, L.EINVAL), (5, d.data_ptr() + 4, L.EINVAL), (5, fx.data_ptr(), L.EINVAL),
             (5, S.data_ptr() + 16, L.EINVAL), (2, 0, L.EINVAL), (3, -1, L.EINVAL), (4, 0, L.EINVAL), (2, 4097, L.EUNSUPPORTED),
             (3, 2 ** 22 + 1, L.EUNSUPPORTED), (4, 40, L.EUNSUPPORTED), (4, 1024, L.EUNSUPPORTED)]
    for i, v, rc in cases:
        bad = list(good)
        bad[i] = v
        assert L.lib.hoig_style_dfeat_host(*bad) == rc, (i, v)
    assert bool((d == 7.0).all())
    assert L.lib.hoig_style_dfeat_host(*good) == L.OK and not bool((d == 7.0).any())


# ------------------------------------------------------------------------------------------------ options
def _opt(**kw):
    return types.SimpleNamespace(**kw)


def test_the_parser_accepts_the_documented_spellings():
    from hoig_amd.style_loss import active, parse_options
    d = parse_options(_opt(), environ={})
    assert d == dict(weight=0.0, levels=(2, 3, 4, 5), level_weights=(1.0, 1.0, 1.0, 1.0)) and not active(d)
    d = parse_options(_opt(lambda_style='10', style_levels=' 1, 5 ', style_level_weights='0.5,2'), environ={})
    assert d == dict(weight=10.0, levels=(1, 5), level_weights=(0.5, 2.0)) and active(d)
    d = parse_options(_opt(style_levels=[3], style_level_weights=(4,)), environ={'HOIG_LAMBDA_STYLE': '3'})
    assert d == dict(weight=3.0, levels=(3,), level_weights=(4.0,)) and active(d)
    # the option wins over the environment; '' and None are unset
    assert not active(parse_options(_opt(lambda_style=0), environ={'HOIG_LAMBDA_STYLE': '3'}))
    assert active(parse_options(_opt(lambda_style=None, style_levels=''), environ={'HOIG_LAMBDA_STYLE': '3'}))
    assert not active(parse_options(_opt(lambda_style=''), environ={'HOIG_LAMBDA_STYLE': ''}))
    assert parse_options(_opt(style_levels=4), environ={})['levels'] == (4,)


@pytest.mark.parametrize('kw,word', [
    (dict(lambda_style=-1.0), 'lambda_style'), (dict(lambda_style='much'), 'lambda_style'), (dict(lambda_style=float('nan')), 'lambda_style'),
    (dict(lambda_style=float('inf')), 'lambda_style'), (dict(lambda_style=True), 'lambda_style'), (dict(lambda_style=[1]), 'lambda_style'),
    (dict(style_levels='0,2'), 'style_levels'), (dict(style_levels='2,6'), 'style_levels'), (dict(style_levels='2,2'), 'style_levels'),
    (dict(style_levels='two'), 'style_levels'), (dict(style_levels=2.5), 'style_levels'), (dict(style_levels=True), 'style_levels'),
    (dict(style_levels=','), 'style_levels'), (dict(style_level_weights='1,1'), 'style_level_weights'),
    (dict(style_level_weights='1,1,1,-1'), 'style_level_weights'), (dict(style_level_weights='1,1,1,x'), 'style_level_weights'),
    (dict(style_level_weights='1,1,1,nan'), 'style_level_weights')], ids=str)
def test_the_parser_raises_on_each_bad_value(kw, word):
    from hoig_amd.style_loss import parse_options
    with pytest.raises(ValueError, match=word) as ex:
        parse_options(_opt(**kw), environ={})
    assert repr(list(kw.values())[0]) in str(ex.value)          # the offending value is in the message
    with pytest.raises(ValueError, match='lambda_style'):
        parse_options(_opt(), environ={'HOIG_LAMBDA_STYLE': 'x'})


# ------------------------------------------------------------------------------------------------ the twin under a sanitizer
ASAN_SHAPES = [(1, 1, 16), (3, 77, 80), (1, R.K + 1, 2 * R.T + 16), (2, R.K - 1, R.T - 16)]


def test_the_twin_under_a_host_sanitizer_build(tmp_path):
    """style_loss_host.cpp built with -fsanitize=address,undefined into a program of its own (tests/style_loss_asan_driver.cpp), every
    buffer a heap block of exactly its size: no report, and the library twin's bits."""
    # (the compiler, the flags and the reasons for them: tests/test_grad_guard_cpu.py)
    cxx = shutil.which(os.environ.get('CXX', 'c++'))
    assert cxx is not None, 'no host C++ compiler (c++, or $CXX) on PATH'
    flags = ['-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
             '-static-libasan']
    exe = str(tmp_path / 'style_loss_asan_driver')
    src = [os.path.join(ROOT, 'hoig_amd', 'csrc', 'style_loss_host.cpp'), os.path.join(ROOT, 'tests', 'style_loss_asan_driver.cpp')]
    build = subprocess.run([cxx] + flags + ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'hoig_amd', 'csrc')] + src +
                           ['-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    for N, P, C in ASAN_SHAPES:
        run = subprocess.run([exe, str(N), str(P), str(C)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert run.returncode == 0 and 'Sanitizer' not in run.stdout and 'runtime error' not in run.stdout, run.stdout[-3000:]
        lines = run.stdout.strip().split('\n')
        assert len(lines) == 2 and all(ln.split()[0] == '0' for ln in lines), run.stdout[:500]
        # the driver's inputs (its function `value`), through the library's twin
        k = np.arange(N * P * C, dtype=np.int64)
        x = (np.maximum((k * 37) % 41 - 20, 0).astype(np.float32) * np.float32(0.046875)).reshape(N, 1, P, C)
        y = (np.maximum((k * 29 + 7) % 43 - 21, 0).astype(np.float32) * np.float32(0.046875)).reshape(N, 1, P, C)
        got = R.run(DEV, x, y)
        seq = lambda a: float(a.astype(np.float64).reshape(-1).cumsum()[-1])
        f = lines[0].split()
        assert [float.fromhex(v) for v in f[1:3]] == [float(np.float32(0.5) + got['term'][0]), float(np.float32(0.25) + got['report'][0])]
        assert [float.fromhex(v) for v in f[3:6]] == [seq(got['S']), seq(np.abs(got['S'])), seq(got['gram'])]
        assert int(f[6]) == 0 and float.fromhex(f[7]) == seq(R.dfeat(DEV, x, got['S']))
        other = R.run(DEV, x, y, scale=2.5, term=False, report=False, gram=False)
        assert float.fromhex(lines[1].split()[1]) == seq(other['S'])
