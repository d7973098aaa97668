"""The opt-in GAN objectives and the LeCam regulariser through their CPU twins (hoig_amd/csrc/gan_loss_host.cpp, the inline functions of
gan_loss.h; docs/gan_objectives.md) against the float64 restatement of tests/gan_objectives_reference.py, within the bounds the document
derives; the state's tick; the option parser; and the twins in a program of their own under a host sanitizer.
tests/test_gan_objectives_gpu.py compares the kernels with these twins."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import gan_objectives_reference as R

DEV = 'cpu'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = sorted(R.MODES.items(), key=lambda kv: kv[1])
FORMS = sorted(R.FORMS.items(), key=lambda kv: kv[1])
S, LAM = 0.75, 0.3
_ids = lambda v: v[0] if isinstance(v[0], str) else '%dx%d' % v


def _ulps(mode):
    return R.ULPS['host'] if mode == R.LOGISTIC else R.ULPS['exact']


def _ab(sizes, seed=0):
    return R.logits(sizes[0], 11 + seed), R.logits(sizes[1], 23 + seed)


def test_the_binding_declares_the_heads():
    from hoig_amd import _lib as L
    names = set(L.declared_symbols())
    for sym in ('hoig_gan_d_loss', 'hoig_gan_d_loss_host', 'hoig_gan_d_loss_workspace_bytes', 'hoig_gan_g_loss', 'hoig_gan_g_loss_host',
                'hoig_gan_g_loss_workspace_bytes'):
        assert sym in names and hasattr(L.lib, sym)
    assert (L.GAN_LSGAN, L.GAN_HINGE, L.GAN_LOGISTIC, L.LECAM_PAPER, L.LECAM_RELU) == (R.LSGAN, R.HINGE, R.LOGISTIC, R.PAPER, R.RELU)
    assert (L.LECAM_STATE_WORDS, L.GAN_THREADS, L.GAN_CHUNK, L.GAN_MAX_GRID) == (R.STATE_WORDS, R.THREADS, R.CHUNK, R.MAX_GRID)
    # one partial of six doubles per workgroup, and never more workgroups than the cap
    assert L.lib.hoig_gan_d_loss_workspace_bytes(1, 1) == 2 * 48 and L.lib.hoig_gan_g_loss_workspace_bytes(R.CHUNK + 1) == 2 * 48
    assert L.lib.hoig_gan_d_loss_workspace_bytes(10 ** 6, 10 ** 6) == R.MAX_GRID * 48
    assert L.lib.hoig_gan_d_loss_workspace_bytes(0, 5) < 0 and L.lib.hoig_gan_g_loss_workspace_bytes(0) < 0


@pytest.mark.parametrize('sizes', R.SIZES, ids=_ids)
@pytest.mark.parametrize('mode', MODES, ids=_ids)
def test_d_head_without_a_state_against_float64(mode, sizes):
    a, b = _ab(sizes)
    got = R.run_d(DEV, mode[1], a, b, S)
    want, bound = R.d_step(mode[1], a, b, S, ulps=_ulps(mode[1]))
    R.check_d(got, want, bound, (mode, sizes))
    assert got['reg'] == 0.0 and got['state'] is None


@pytest.mark.parametrize('sizes', [R.SIZES[0], R.SIZES[2], R.SIZES[4], R.SIZES[5], R.SIZES[6]], ids=_ids)
@pytest.mark.parametrize('started', [False, True], ids=['before_start', 'after_start'])
@pytest.mark.parametrize('form', FORMS, ids=_ids)
@pytest.mark.parametrize('mode', MODES, ids=_ids)
def test_d_head_with_the_regulariser_against_float64(mode, form, started, sizes):
    a, b = _ab(sizes, 1)
    st = R.new_state(gamma=0.9, start=5, count=7 if started else 4, alpha_r=0.4375, alpha_f=-0.3)
    got = R.run_d(DEV, mode[1], a, b, S, LAM, form[1], st)
    want, bound = R.d_step(mode[1], a, b, S, LAM, form[1], st, ulps=_ulps(mode[1]))
    R.check_d(got, want, bound, (mode, form, started, sizes))
    assert (want['reg'] > 0.0) == started and (got['reg'] > 0.0) == started
    if not started:        # weight 0: the term, and every gradient, is the objective's alone
        plain = R.run_d(DEV, mode[1], a, b, S)
        assert got['obj'] == plain['obj'] and got['da'].tobytes() == plain['da'].tobytes() and got['db'].tobytes() == plain['db'].tobytes()
    # the tick used this step's means, after the regulariser read the old anchors
    ref = R.tick(st, want['mean_a'], want['mean_b'])
    assert got['state']['count'] == ref['count'] and got['state']['bad'] == 0
    for k in ('alpha_r', 'alpha_f'):
        assert abs(got['state'][k] - ref[k]) <= R.anchor_bound(1, [want['mean_a'], want['mean_b'], st[k]]) + bound['mean_a'] + bound['mean_b']
    assert got['state']['gamma'] == 0.9 and got['state']['start'] == 5


@pytest.mark.parametrize('sizes', R.SIZES, ids=_ids)
@pytest.mark.parametrize('mode', MODES, ids=_ids)
def test_g_head_against_float64(mode, sizes):
    b = R.logits(sizes[0], 5)
    got = R.run_g(DEV, mode[1], b, S)
    want, bound = R.g_step(mode[1], b, S, ulps=_ulps(mode[1]))
    assert abs(float(got['obj']) - want['obj']) <= bound['obj'], (float(got['obj']), want['obj'], bound['obj'])
    assert (np.abs(got['db'].astype(np.float64) - want['db']) <= bound['db']).all()


def test_the_kinks_and_exact_zeros_take_the_documented_subgradient():
    x = np.array([1.0, -1.0, 0.0, -0.0, 2.0, -2.0], np.float32)
    got = R.run_d(DEV, R.HINGE, x, x, 6.0)                      # s / n = 1
    assert got['da'].tolist() == [0.0, -1.0, -1.0, -1.0, 0.0, -1.0]      # d max(0, 1 - a): 0 at the kink a = 1
    assert got['db'].tolist() == [1.0, 0.0, 1.0, 1.0, 1.0, 0.0]          # d max(0, 1 + b): 0 at the kink b = -1
    assert got['obj'] == 14.0                                            # 6 mean(0, 2, 1, 1, 0, 3) + 6 mean(2, 0, 1, 1, 3, 0)
    got = R.run_d(DEV, R.LSGAN, x, x, 6.0)
    assert got['da'].tolist() == [0.0, -4.0, -2.0, -2.0, 2.0, -6.0] and got['db'].tolist() == [4.0, 0.0, 2.0, 2.0, 6.0, -2.0]
    st = R.new_state(start=1, count=1, alpha_r=0.0, alpha_f=0.0)
    relu = R.run_d(DEV, R.HINGE, x, x, 0.0, 6.0, R.RELU, st)    # lambda / n = 1, the objective's weight 0
    assert relu['da'].tolist() == [2.0, 0.0, 0.0, 0.0, 4.0, 0.0]         # d max(0, a - 0)^2
    assert relu['db'].tolist() == [0.0, -2.0, 0.0, 0.0, 0.0, -4.0]       # d max(0, 0 - b)^2
    assert relu['reg'] == np.float32(5.0 / 6.0 + 5.0 / 6.0)


@pytest.mark.parametrize('mode', MODES, ids=_ids)
def test_null_gradients_leave_the_sums_and_the_state(mode):
    a, b = _ab(R.SIZES[4], 2)
    st = R.new_state(gamma=0.9, start=2, count=3, alpha_r=0.2, alpha_f=-0.1)
    with_g, without = R.run_d(DEV, mode[1], a, b, S, LAM, R.PAPER, st), R.run_d(DEV, mode[1], a, b, S, LAM, R.PAPER, st, grads=False)
    assert without['da'] is None and without['db'] is None
    for k in ('obj', 'mean_a', 'mean_b', 'reg'):
        assert with_g[k].tobytes() == without[k].tobytes()
    assert with_g['words'] == without['words']
    g1, g0 = R.run_g(DEV, mode[1], b, S), R.run_g(DEV, mode[1], b, S, grads=False)
    assert g1['obj'].tobytes() == g0['obj'].tobytes() and g0['db'] is None


def test_a_null_state_leaves_the_term_without_a_regulariser():
    a, b = _ab(R.SIZES[3], 3)
    st = R.new_state(start=1, count=4, alpha_r=0.5, alpha_f=-0.5)
    with_reg, without = R.run_d(DEV, R.HINGE, a, b, S, LAM, R.PAPER, st), R.run_d(DEV, R.HINGE, a, b, S, LAM, R.PAPER, None)
    want, bound = R.d_step(R.HINGE, a, b, S)
    R.check_d(without, want, bound)
    assert without['reg'] == 0.0 and with_reg['reg'] > 0.0
    assert abs(float(with_reg['obj']) - float(without['obj']) - LAM * float(with_reg['reg'])) <= 4 * R.u * abs(float(with_reg['obj']))


def test_the_slots_are_added_to():
    a, b = _ab(R.SIZES[1], 4)
    zero, one = R.run_d(DEV, R.HINGE, a, b, S), R.run_d(DEV, R.HINGE, a, b, S, init=1.0)
    for k in ('obj', 'mean_a', 'mean_b', 'reg'):
        assert one[k] == np.float32(1.0) + zero[k]
    assert R.run_g(DEV, R.LOGISTIC, b, S, init=1.0)['obj'] == np.float32(1.0) + R.run_g(DEV, R.LOGISTIC, b, S)['obj']


@pytest.mark.parametrize('form', FORMS, ids=_ids)
def test_five_ticks_follow_the_recurrence_and_the_first_sets_the_anchors(form):
    st = R.new_state(gamma=0.75, start=3)
    ref = dict(st)
    means, regs = [], []
    for k in range(5):
        a, b = R.logits(130, 100 + k) + np.float32(0.5 * k), R.logits(77, 200 + k) - np.float32(0.25 * k)
        want, bound = R.d_step(R.HINGE, a, b, S, LAM, form[1], st)       # (the regulariser against the anchors the twin itself holds)
        got = R.run_d(DEV, R.HINGE, a, b, S, LAM, form[1], st)
        ref = R.tick(ref, want['mean_a'], want['mean_b'])
        st = got['state']
        means += [want['mean_a'], want['mean_b']]
        regs.append(float(got['reg']))
        assert st['count'] == k + 1 and st['bad'] == 0
        assert abs(float(got['reg']) - want['reg']) <= bound['reg']
        if k == 0:     # the first tick SETS the anchors: they are the step's means, whatever they were
            assert st['alpha_r'] == st['last_r'] and st['alpha_f'] == st['last_f']
        for key in ('alpha_r', 'alpha_f'):
            assert abs(st[key] - ref[key]) <= R.anchor_bound(k + 1, means) + bound['mean_a'] + bound['mean_b'], (k, key)
    assert regs[:3] == [0.0, 0.0, 0.0] and regs[3] > 0.0 and regs[4] > 0.0        # start 3: the counts before the steps are 0 .. 4


def test_a_nan_logit_refuses_the_tick():
    a, b = _ab(R.SIZES[2], 5)
    st = R.new_state(gamma=0.9, start=1, count=6, alpha_r=0.25, alpha_f=-0.125)
    for side in (0, 1):
        x = [a.copy(), b.copy()]
        x[side][17] = np.nan
        got = R.run_d(DEV, R.HINGE, x[0], x[1], S, LAM, R.PAPER, st)
        assert got['state'] == dict(st, bad=1)
    inf = a.copy()
    inf[3] = np.inf
    assert R.run_d(DEV, R.LSGAN, inf, b, S, LAM, R.RELU, st)['state'] == dict(st, bad=1)
    # ... and a second refusal counts on
    assert R.run_d(DEV, R.LSGAN, inf, b, S, LAM, R.RELU, dict(st, bad=1))['state']['bad'] == 2


def test_entry_points_refuse_bad_arguments():
    from hoig_amd import _lib as L
    from hoig_amd._twin import ptr
    a, b = torch.zeros(8), torch.zeros(8)
    da, slot = torch.zeros(8), torch.zeros(1)
    state = torch.zeros(R.STATE_WORDS, dtype=torch.int64)
    good = [R.HINGE, ptr(a), 8, ptr(b), 8, 1.0, 0.5, R.PAPER, ptr(state), ptr(da), None, ptr(slot), None, None, None]
    assert L.lib.hoig_gan_d_loss_host(*good) == L.OK
    for i, v in ((0, 3), (0, -1), (1, None), (2, 0), (3, None), (4, -2), (5, float('nan')), (6, -0.5), (6, float('inf')), (7, 2),
                 (8, state.data_ptr() + 4), (9, da.data_ptr() + 2), (9, b.data_ptr()), (11, slot.data_ptr() + 1)):
        bad = list(good)
        bad[i] = v
        assert L.lib.hoig_gan_d_loss_host(*bad) == L.EINVAL, (i, v)
    assert L.lib.hoig_gan_g_loss_host(R.HINGE, ptr(b), 8, 1.0, None, ptr(slot)) == L.OK
    for args in ((5, ptr(b), 8, 1.0, None, ptr(slot)), (R.HINGE, None, 8, 1.0, None, ptr(slot)), (R.HINGE, ptr(b), 0, 1.0, None, ptr(slot))):
        assert L.lib.hoig_gan_g_loss_host(*args) == L.EINVAL


# ------------------------------------------------------------------------------------------------ options
def _opt(**kw):
    return types.SimpleNamespace(**kw)


def test_the_parser_accepts_the_documented_spellings():
    from hoig_amd import _lib as L
    from hoig_amd.gan_loss import active, parse_options
    d = parse_options(_opt(), environ={})
    assert d == dict(mode=L.GAN_LSGAN, lecam=0.0, decay=0.99, start=1000, form=L.LECAM_PAPER) and not active(d)
    assert parse_options(_opt(gan_mode='Hinge'), environ={})['mode'] == L.GAN_HINGE
    assert parse_options(_opt(gan_mode=' logistic '), environ={})['mode'] == L.GAN_LOGISTIC
    assert parse_options(_opt(), environ={'HOIG_GAN_MODE': 'hinge', 'HOIG_LECAM': '0.3'}) == \
        dict(mode=L.GAN_HINGE, lecam=0.3, decay=0.99, start=1000, form=L.LECAM_PAPER)
    # the option wins over the environment; '' and None are unset
    assert parse_options(_opt(gan_mode='lsgan', lecam=None), environ={'HOIG_GAN_MODE': 'hinge', 'HOIG_LECAM': ''})['mode'] == L.GAN_LSGAN
    d = parse_options(_opt(lecam='0.01', lecam_decay=0.9, lecam_start='20', lecam_form='RELU'), environ={})
    assert d == dict(mode=L.GAN_LSGAN, lecam=0.01, decay=0.9, start=20, form=L.LECAM_RELU) and active(d)
    assert active(parse_options(_opt(gan_mode='hinge'), environ={})) and not active(parse_options(_opt(lecam=0), environ={}))


@pytest.mark.parametrize('kw,word', [
    (dict(gan_mode='wgan'), 'gan_mode'), (dict(gan_mode=1), 'gan_mode'), (dict(lecam=-0.1), 'lecam'), (dict(lecam='much'), 'lecam'),
    (dict(lecam=float('nan')), 'lecam'), (dict(lecam=float('inf')), 'lecam'), (dict(lecam=True), 'lecam'),
    (dict(lecam_decay=0.0), 'lecam_decay'), (dict(lecam_decay=1.0), 'lecam_decay'), (dict(lecam_decay='x'), 'lecam_decay'),
    (dict(lecam_start=0), 'lecam_start'), (dict(lecam_start=2.5), 'lecam_start'), (dict(lecam_start='soon'), 'lecam_start'),
    (dict(lecam_form='square'), 'lecam_form'), (dict(lecam_form=0), 'lecam_form')], ids=str)
def test_the_parser_raises_on_each_bad_value(kw, word):
    from hoig_amd.gan_loss import parse_options
    with pytest.raises(ValueError, match=word) as ex:
        parse_options(_opt(**kw), environ={})
    assert repr(list(kw.values())[0]) in str(ex.value)          # the offending value is in the message
    with pytest.raises(ValueError, match='gan_mode'):
        parse_options(_opt(), environ={'HOIG_GAN_MODE': 'wgan'})


def test_the_state_class_round_trips_its_words():
    from hoig_amd import _lib as L
    from hoig_amd.gan_loss import LeCam
    lc = LeCam('cpu', 0.3, decay=0.9, start=5, form=L.LECAM_RELU)
    assert R.words_state(lc.state.numpy()) == R.new_state(gamma=0.9, start=5)
    a, b = _ab((130, 5))
    for _ in range(3):
        got = R.run_d(DEV, R.HINGE, a, b, S, 0.3, R.RELU, R.words_state(lc.state.numpy()))
        lc.state.copy_(torch.from_numpy(np.frombuffer(got['words'], np.int64).copy()))
    sd = lc.state_dict()
    assert sd['count'] == 3 and sd['decay'] == 0.9 and sd['start'] == 5 and sd['form'] == 'relu' and sd['bad'] == 0
    other = LeCam('cpu', 0.3, decay=0.9, start=5, form=L.LECAM_RELU)
    other.load_state_dict(sd)
    assert other.state.numpy().tobytes() == lc.state.numpy().tobytes()
    assert lc.report() == dict(real=sd['alpha_real'], fake=sd['alpha_fake'], count=3, bad=0)
    lc.reset()
    assert lc.state_dict()['count'] == 0
    with pytest.raises(ValueError):
        LeCam('cpu', 0.0)


# ------------------------------------------------------------------------------------------------ the twins under a sanitizer
def test_the_twins_under_a_host_sanitizer_build(tmp_path):
    """gan_loss_host.cpp built with -fsanitize=address,undefined into a program of its own (tests/gan_objectives_asan_driver.cpp), every
    buffer a heap block of exactly its size, at the sizes above: no report, and -- outside the logistic objective, whose expf / log1pf
    another compiler may evaluate differently -- the library's twins' bits."""
    # (the compiler, the flags and the reasons for them: tests/test_grad_guard_cpu.py)
    cxx = shutil.which(os.environ.get('CXX', 'c++'))
    assert cxx is not None, 'no host C++ compiler (c++, or $CXX) on PATH'
    flags = ['-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
             '-static-libasan']
    exe = str(tmp_path / 'gan_objectives_asan_driver')
    src = [os.path.join(ROOT, 'hoig_amd', 'csrc', 'gan_loss_host.cpp'), os.path.join(ROOT, 'tests', 'gan_objectives_asan_driver.cpp')]
    build = subprocess.run([cxx] + flags + ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'hoig_amd', 'csrc')] + src +
                           ['-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    for n_a, n_b in R.SIZES:
        run = subprocess.run([exe, str(n_a), str(n_b)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert run.returncode == 0 and 'Sanitizer' not in run.stdout and 'runtime error' not in run.stdout, run.stdout[-3000:]
        lines = run.stdout.strip().split('\n')
        assert len(lines) == 3 * 6 and all(ln.split()[0] == '0' for ln in lines), run.stdout[:500]
        # the driver's logits (its function `logit`), through the library's twins
        def logit(n, side):
            i = np.arange(n, dtype=np.int64)
            k = (i * 37 + side * 11) % 41
            x = ((k - 20).astype(np.float32) * np.float32(0.171875) + np.float32(0.25 if side else -0.125)).astype(np.float32)
            x[k == 0], x[k == 1], x[k == 2] = 0.0, 1.0, -1.0
            return x
        a, b = logit(n_a, 0), logit(n_b, 1)
        for mode in (R.LSGAN, R.HINGE):
            rows = lines[6 * mode:6 * mode + 6]
            at = 0
            for form in (R.PAPER, R.RELU):
                st = R.new_state(gamma=0.9, start=1)
                for _ in range(2):
                    got = R.run_d(DEV, mode, a, b, 0.5, 0.3, form, st)
                    st = got['state']
                    f = rows[at].split()
                    assert [float.fromhex(v) for v in f[1:5]] == [float(got[k]) for k in ('obj', 'mean_a', 'mean_b', 'reg')]
                    assert float.fromhex(f[5]) == float(got['da'].astype(np.float64).cumsum()[-1])
                    assert float.fromhex(f[6]) == float(got['db'].astype(np.float64).cumsum()[-1])
                    assert [int(v, 16) for v in f[7:]] == [int(v) for v in np.frombuffer(got['words'], np.uint64)]
                    at += 1
            assert float.fromhex(rows[4].split()[1]) == float(R.run_d(DEV, mode, a, b, 0.5, grads=False)['obj'])
            assert float.fromhex(rows[5].split()[1]) == float(R.run_g(DEV, mode, b, 0.5)['obj'])
