"""The discriminator augmentation through its CPU twins (hoig_amd/csrc/d_augment_host.cpp, the inline functions of d_augment.h;
docs/d_augment.md): the draws against Philox and the word table in Python integers, word for word; the forward and the backward against
DiffAugment's published functions in float64 within bounds derived from the operation counts; handcrafted records; the adaptive
controller against Python doubles; refusals; the options; the twins in a program of their own under a host sanitizer.
tests/test_d_augment_gpu.py compares the kernels with these twins."""
import itertools
import types

import numpy as np
import pytest

import d_augment_reference as R

SYMBOLS = ['hoig_daug_ws_floats'] + ['hoig_daug_%s%s' % (n, h) for n in ('tick', 'draw', 'adapt', 'fwd', 'bwd') for h in ('', '_host')]


def test_the_binding_declares_the_augmentation():
    from hoig_amd import _lib as L
    names = set(L.declared_symbols())
    for sym in SYMBOLS:
        assert sym in names and hasattr(L.lib, sym) and sym in L._SIGS
    assert (L.DAUG_COLOR, L.DAUG_TRANSLATION, L.DAUG_CUTOUT) == (R.COLOR, R.TRANSLATION, R.CUTOUT)
    assert (L.DAUG_STATE_WORDS, L.DAUG_MAX_PARTS) == (R.STATE_WORDS, R.MAX_PARTS)
    assert L.lib.hoig_daug_ws_floats(3) == 3 * R.MAX_PARTS and L.lib.hoig_daug_ws_floats(0) == L.EINVAL


def test_philox_known_answers():
    """The three Random123 known answers for philox4x32-10 (kat_vectors)."""
    kat = [((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
           ((R.M32,) * 4, (R.M32,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')]
    for ctr, key, want in kat:
        assert ' '.join('%08x' % w for w in R.philox4x32_10(ctr, key)) == want


# ------------------------------------------------------------------------------------------------ draws
@pytest.mark.parametrize('hw', [(5, 7), (8, 8), (6, 10), (64, 64), (256, 256)], ids=lambda v: '%dx%d' % v)
def test_draw_twin_is_the_python_statement_word_for_word(hw):
    H, W = hw
    B = 5
    for step, site, rank, p, policy in itertools.product((0, 1, 2 ** 32 + 5), (0, 1, 2), (0, 3), (0.0, 0.3, 1.0), R.POLICIES):
        state = R.make_state(step=step, p=p, policy=policy, seed=11, rank=rank)
        before = state.copy()
        got = R.twin_draw(state, site, B, H, W)
        want = R.py_draw(step, site, B, H, W, p, policy, seed=11, rank=rank)
        assert got.tobytes() == want.tobytes(), (step, site, rank, p, policy)
        assert state.tobytes() == before.tobytes()
        if p == 0.0:
            assert (got == R.record()).all()
        if p == 1.0:
            assert (got[:, 7] == policy).all()


def test_draws_differ_by_step_site_rank_and_seed():
    base = R.twin_draw(R.make_state(step=3, seed=1, rank=0), 0, 4, 16, 16)
    for other in (R.twin_draw(R.make_state(step=4, seed=1, rank=0), 0, 4, 16, 16), R.twin_draw(R.make_state(step=3, seed=1, rank=0), 1, 4, 16, 16),
                  R.twin_draw(R.make_state(step=3, seed=1, rank=1), 0, 4, 16, 16), R.twin_draw(R.make_state(step=3, seed=2, rank=0), 0, 4, 16, 16)):
        assert not (base[:, :7] == other[:, :7]).all(axis=1).any()


@pytest.mark.parametrize('hw', [(5, 7), (8, 8), (6, 10)], ids=lambda v: '%dx%d' % v)
def test_every_shift_and_centre_occurs_and_none_falls_outside(hw):
    H, W = hw
    rec = np.concatenate([R.twin_draw(R.make_state(step=s), 2, 64, H, W) for s in range(64)])          # 4096 draws
    assert (rec[:, 7] == 7).all()
    ints = rec[:, 3:7].copy().view(np.int32)
    sy, sx, zy, zx = R.shift_of(H), R.shift_of(W), R.cut_of(H), R.cut_of(W)
    assert sorted(set(ints[:, 0])) == list(range(-sy, sy + 1)) and sorted(set(ints[:, 1])) == list(range(-sx, sx + 1))
    assert sorted(set(ints[:, 2] + zy // 2)) == list(range(0, H + 1 - zy % 2))
    assert sorted(set(ints[:, 3] + zx // 2)) == list(range(0, W + 1 - zx % 2))
    f = rec[:, :3].copy().view(np.float32)
    assert (f[:, 0] >= -0.5).all() and (f[:, 0] < 0.5).all() and (f[:, 1] >= 0).all() and (f[:, 1] < 2).all()
    assert (f[:, 2] >= 0.5).all() and (f[:, 2] < 1.5).all()


def test_gates_apply_each_family_with_probability_p():
    """4096 samples at p = 0.3: each gate is a Bernoulli(0.3) word, so each count lies within 5 sigma (147) of 1229; the three
    gates are separate words, so all eight flag values occur."""
    rec = np.concatenate([R.twin_draw(R.make_state(step=s, p=0.3), 0, 64, 8, 8) for s in range(64)])
    for bit in (R.COLOR, R.TRANSLATION, R.CUTOUT):
        assert abs(int(((rec[:, 7] & bit) != 0).sum()) - 1229) <= 147
    assert sorted(set(rec[:, 7])) == list(range(8))


# ------------------------------------------------------------------------------------------------ forward and backward
def _data(B, H, W, k, seed):
    rng = np.random.default_rng(seed)
    img = rng.uniform(-1, 1, (B, H, W, 3)).astype(np.float32)
    cond = rng.uniform(-1, 1, (B, H, W, k)).astype(np.float32)
    g = rng.uniform(-1, 1, (B, H, W, 3 + k)).astype(np.float32)
    return img, cond, g


CASES = [(hw, B, k) for hw in R.SHAPES for B in (1, 3) for k in R.KS] + [((40, 40), 1, 2)]      # (the last: two partial sums per sample)


@pytest.mark.parametrize('hw,B,k', CASES, ids=lambda v: '%dx%d' % v if isinstance(v, tuple) else str(v))
def test_forward_twin_against_diffaugment_in_float64(hw, B, k):
    """Records drawn at p = 1 with every family.  |x| <= 1, b in [-0.5, 0.5), s in [0, 2), k in [0.5, 1.5): p = x + b, m, q, mu and
    the output all stay below 8 in magnitude (|p - m| <= 4/3, so |(p - m) s| <= 8/3; |m - mu| <= 2), so one fp32 rounding costs at
    most E = 8 * 2^-24.  In units of E: p 1; m = ((p0 + p1) + p2) / 3 at most 4; (p - m) 6, times s 13, plus m 18 = q; with e the
    error of mu: (q - mu) 19 + e, times k 29.5 + 1.5 e, plus mu 30.5 + 2.5 e.  mu = M + b: one rounding (E) plus the error of the
    mean M, whose terms pass through at most `depth` additions and one division, |M| <= 1: depth * 2^-24
    (d_augment_reference.sum_depth).  Pixels that are cut or shifted in from outside are exact zeros; condition channels are copies."""
    H, W = hw
    img, cond, _ = _data(B, H, W, k, 100 * H + W + k)
    params = R.twin_draw(R.make_state(step=H * W + k, p=1.0), 1, B, H, W)
    got = R.twin_fwd(img, cond, params)
    want = R.diffaugment_f64(img, cond, params)
    err = float(np.abs(got.astype(np.float64) - want).max())
    bound = R.fwd_bound(H, W)
    print('fwd %dx%d B %d k %d: max |fp32 - fp64| = %.3e, bound %.3e' % (H, W, B, k, err, bound))
    assert err <= bound
    assert (got[..., 3:].astype(np.float64) == want[..., 3:]).all()
    assert (got[(want == 0.0).all(axis=-1)] == 0.0).all()


@pytest.mark.parametrize('hw,B,k', CASES, ids=lambda v: '%dx%d' % v if isinstance(v, tuple) else str(v))
def test_backward_twin_against_diffaugment_in_float64(hw, B, k):
    """|g| <= 1 and the ranges above: dq = k g (|dq| < 1.5), its channel sum (< 4.5), s dq (< 3), (1 - s) mean (< 1.5), dp (< 4.5)
    and dimg (< 5) stay below 8, so one rounding costs at most E = 8 * 2^-24.  In units of E: dq 1; ((dq0 + dq1) + dq2) / 3 at most
    3; 1 - s rounds once (< 1 after the product with the mean), so (1 - s) mean 5; s dq 3; their sum 9; plus c = dmu / (3HW), with
    its error, 10 + e.  c = (1 - k) G / (3HW), |c| <= 1/2: the terms of G pass through at most `depth` additions, then 1 - k, the
    product and the division round: (depth + 3) * 2^-24."""
    H, W = hw
    img, cond, g = _data(B, H, W, k, 200 * H + W + k)
    params = R.twin_draw(R.make_state(step=H * W + k, p=1.0), 0, B, H, W)
    got = R.twin_bwd(g, params)
    _, want = R.diffaugment_f64(img, cond, params, g)
    err = float(np.abs(got.astype(np.float64) - want).max())
    bound = R.bwd_bound(H, W)
    print('bwd %dx%d B %d k %d: max |fp32 - fp64| = %.3e, bound %.3e' % (H, W, B, k, err, bound))
    assert err <= bound


def _handcrafted(H, W):
    """name -> record: the largest shift each way, a box over each edge and each corner, colour only, geometry only."""
    sy, sx, zy, zx = R.shift_of(H), R.shift_of(W), R.cut_of(H), R.cut_of(W)
    T, C, K = R.TRANSLATION, R.CUTOUT, R.COLOR
    recs = {'up': R.record(ty=-sy, flags=T), 'down': R.record(ty=sy, flags=T), 'left': R.record(tx=-sx, flags=T),
            'right': R.record(tx=sx, flags=T), 'diag': R.record(ty=sy, tx=-sx, flags=T),
            'color': R.record(b=-0.25, s=1.75, k=0.625, flags=K),
            'geometry': R.record(ty=-sy, tx=sx, cy0=1, cx0=0, flags=T | C),
            'all': R.record(b=0.375, s=0.25, k=1.375, ty=sy, tx=sx, cy0=H - zy, cx0=W - zx, flags=K | T | C)}
    lo_y, hi_y, lo_x, hi_x = -(zy // 2), H - zy // 2 - zy % 2, -(zx // 2), W - zx // 2 - zx % 2       # the extreme drawn origins
    for ny, y0 in (('top', lo_y), ('mid', (H - zy) // 2), ('bottom', hi_y)):
        for nx, x0 in (('left', lo_x), ('mid', (W - zx) // 2), ('right', hi_x)):
            recs['box_%s_%s' % (ny, nx)] = R.record(cy0=y0, cx0=x0, flags=C)
    return recs


@pytest.mark.parametrize('hw', R.SHAPES, ids=lambda v: '%dx%d' % v)
def test_handcrafted_records(hw):
    """Each record on its own sample: the forward and the backward within the bounds above, the cut and shifted-in pixels exact zeros, and
    exact copies wherever colour is off."""
    H, W = hw
    recs = _handcrafted(H, W)
    B, k = len(recs), 2
    img, cond, g = _data(B, H, W, k, 31 * H + W)
    params = np.stack(list(recs.values()))
    got, dgot = R.twin_fwd(img, cond, params), R.twin_bwd(g, params)
    want, dwant = R.diffaugment_f64(img, cond, params, g)
    assert float(np.abs(got - want).max()) <= R.fwd_bound(H, W) and float(np.abs(dgot - dwant).max()) <= R.bwd_bound(H, W)
    for i, (name, rec) in enumerate(recs.items()):
        if not rec[7] & R.COLOR:
            assert (got[i].astype(np.float64) == want[i]).all() and (dgot[i].astype(np.float64) == dwant[i]).all(), name
        assert (got[i][(want[i] == 0).all(axis=-1)] == 0).all(), name
        if name.startswith('box'):
            zeros = int((want[i] == 0).all(axis=-1).sum())
            y0, x0 = int(np.int32(rec[5])), int(np.int32(rec[6]))
            rows = min(y0 + R.cut_of(H), H) - max(y0, 0)
            cols = min(x0 + R.cut_of(W), W) - max(x0, 0)
            assert zeros == rows * cols > 0, name
    sy = R.shift_of(H)
    if sy:
        i = list(recs).index('down')                         # out(y) = in(y + sy): the last sy rows come from outside
        assert (got[i][:H - sy, :, :3] == img[i][sy:]).all() and (got[i][H - sy:] == 0).all()


@pytest.mark.parametrize('hw,B,k', [((5, 7), 3, 1), ((8, 8), 1, 4), ((9, 4), 3, 7), ((16, 16), 3, 16)], ids=str)
def test_all_flags_clear_is_the_concatenation_bitwise(hw, B, k):
    H, W = hw
    img, cond, g = _data(B, H, W, k, 7)
    img[0, 0, 0, 0], g[0, 0, 0, 1] = -0.0, -0.0          # (a copy keeps the sign of a zero; x + 0 and x * 1 + 0 would not)
    params = np.stack([R.record()] * B)
    params[:, :3] = R.record(b=0.3, s=0.2, k=0.7)[:3]   # (values of a family whose flag is clear are not read)
    got, dgot = R.twin_fwd(img, cond, params), R.twin_bwd(g, params)
    assert got.tobytes() == np.concatenate([img, cond], axis=-1).tobytes()
    assert dgot.tobytes() == np.ascontiguousarray(g[..., :3]).tobytes()


# ------------------------------------------------------------------------------------------------ the controller
def _feed(state, ctl, values):
    d = R.aligned(len(values), np.float32, values)
    assert R.adapt_host(state, d, len(values)) == 0
    ctl.feed(int((d > 0).sum()), int((d < 0).sum()), len(values))


def test_adapt_twin_is_the_python_controller():
    interval, inc = 3, 0.125
    state = R.make_state(p=0.25, target=0.6, interval=interval, increment=inc)
    ctl = R.PyController(0.25, 0.6, interval, inc)
    up = lambda: np.full(37, 0.5)                                            # r = 31 / 37 > 0.6 with the zeros below: p rises
    down = lambda: np.where(np.arange(37) % 2 == 0, 0.5, -0.5)               # r about 0 < 0.6: p falls
    seen = []
    for phase, n in ((up, 8 * interval), (down, 10 * interval), (up, 2 * interval + 1)):
        for j in range(n):
            before = R.state_p(state)
            v = phase().astype(np.float32)
            v[::7] = 0.0                                                    # zeros count in the total only
            _feed(state, ctl, v)
            assert R.state_p(state) == ctl.p and R._w2f(state[R.RT]) == ctl.rt
            assert (int(state[R.POS]), int(state[R.NEG]), int(state[R.TOTAL]), int(state[R.STEPS])) == (ctl.pos, ctl.neg, ctl.total, ctl.steps)
            if int(state[R.STEPS]) != 0:
                assert R.state_p(state) == before                           # p moves only on the interval's last step
            else:
                assert state[R.POS] == state[R.NEG] == state[R.TOTAL] == 0   # and the counters clear there
            seen.append(R.state_p(state))
    assert max(seen) == 1.0 and min(seen) == 0.0                              # clamped at both ends
    assert seen[3 * interval - 1] == 0.25 + 3 * inc and seen[-1] == 2 * inc and int(state[R.STEPS]) == 1
    assert int(state[R.STEP]) == 0 and int(state[R.ADJUSTS]) == 20


def test_tick_twin_counts_past_32_bits():
    state = R.make_state(step=2 ** 32 - 1)
    rest = state[1:].copy()
    assert R.tick_host(state) == 0 and int(state[R.STEP]) == 2 ** 32
    assert R.tick_host(state) == 0 and int(state[R.STEP]) == 2 ** 32 + 1 and (state[1:] == rest).all()


def test_twins_refuse_and_leave_the_outputs():
    from hoig_amd import _lib as L
    B, H, W, k = 2, 4, 4, 2
    state = R.make_state()
    s0 = state.copy()
    params = R.aligned(B * 8, np.uint32, 7)
    img, cond = R.aligned(B * H * W * 3, np.float32, 1.0), R.aligned(B * H * W * k, np.float32, 2.0)
    out, g = R.aligned(B * H * W * (3 + k), np.float32, 3.0), R.aligned(B * H * W * (3 + k), np.float32, 4.0)
    dimg, ws = R.aligned(B * H * W * 3, np.float32, 5.0), R.aligned(B * R.MAX_PARTS, np.float32, 6.0)
    bytes_ = R.aligned(64, np.uint8, 0)
    off1 = bytes_[1:].ctypes.data                                               # an odd address
    for args in [(None, 0, B, H, W, params), (state, 0, B, H, W, None), (state, -1, B, H, W, params), (state, 3, B, H, W, params),
                 (state, 0, 0, H, W, params), (state, 0, B, 0, W, params), (state, 0, B, H, -2, params), (state, 0, B, H, W, params[1:])]:
        assert R.draw_host(*args) == L.EINVAL
    assert L.lib.hoig_daug_draw_host(off1, 0, B, H, W, params.ctypes.data) == L.EINVAL
    assert R.tick_host(None) == L.EINVAL and L.lib.hoig_daug_tick_host(off1) == L.EINVAL
    assert R.adapt_host(None, g, 4) == L.EINVAL and R.adapt_host(state, None, 4) == L.EINVAL and R.adapt_host(state, g, 0) == L.EINVAL
    assert L.lib.hoig_daug_adapt_host(state.ctypes.data, off1, 4) == L.EINVAL
    for args in [(None, cond, params, out, B, H, W, k, ws), (img, None, params, out, B, H, W, k, ws), (img, cond, None, out, B, H, W, k, ws),
                 (img, cond, params, None, B, H, W, k, ws), (img, cond, params, out, B, H, W, k, None), (img, cond, params, out, 0, H, W, k, ws),
                 (img, cond, params, out, B, -1, W, k, ws), (img, cond, params, out, B, H, 0, k, ws), (img, cond, params, out, B, H, W, 0, ws),
                 (img, cond, params[1:], out, B, H, W, k, ws), (img, cond, params, img, B, H, W, k, ws), (img, cond, params, out, B, H, W, k, img)]:
        assert R.fwd_host(*args) == L.EINVAL
    assert L.lib.hoig_daug_fwd_host(img.ctypes.data, cond.ctypes.data, params.ctypes.data, off1, 1, 1, 1, 1, ws.ctypes.data) == L.EINVAL
    for args in [(None, params, dimg, B, H, W, k, ws), (g, None, dimg, B, H, W, k, ws), (g, params, None, B, H, W, k, ws),
                 (g, params, dimg, B, H, W, k, None), (g, params, dimg, 0, H, W, k, ws), (g, params, dimg, B, H, W, -1, ws),
                 (g, params[1:], dimg, B, H, W, k, ws), (g, params, g, B, H, W, k, ws)]:
        assert R.bwd_host(*args) == L.EINVAL
    assert state.tobytes() == s0.tobytes() and (params == 7).all() and (img == 1).all() and (cond == 2).all() and (out == 3).all()
    assert (g == 4).all() and (dimg == 5).all() and (ws == 6).all()


# ------------------------------------------------------------------------------------------------ under a host sanitizer
def test_the_twins_under_a_host_sanitizer_build(tmp_path):
    """d_augment_host.cpp built with -fsanitize=address,undefined into a program of its own (tests/d_augment_asan_driver.cpp), every
    buffer a heap block of exactly its size: no report, and the library's twin's results."""
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
    exe = str(tmp_path / 'd_augment_asan_driver')
    src = [os.path.join(root, 'hoig_amd', 'csrc', 'd_augment_host.cpp'), os.path.join(root, 'tests', 'd_augment_asan_driver.cpp')]
    build = subprocess.run([cxx] + flags + ['-I' + os.path.join(root, 'include'), '-I' + os.path.join(root, 'hoig_amd', 'csrc')] + src +
                           ['-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    for B, H, W, k in [(1, 5, 7, 1), (3, 9, 4, 7), (2, 16, 16, 16), (2, 40, 40, 2)]:
        run = subprocess.run([exe] + [str(v) for v in (B, H, W, k)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert run.returncode == 0 and 'Sanitizer' not in run.stdout and 'runtime error' not in run.stdout, run.stdout[-3000:]
        out = run.stdout.split('\n')
        assert int(out[0]) == 0
        npix, C = B * H * W, 3 + k
        i = np.arange(npix * C, dtype=np.int64)
        img = ((((i[:npix * 3] * 17 + 3) % 29) - 14).astype(np.float32) * np.float32(0.0625)).reshape(B, H, W, 3)
        cond = ((((i[:npix * k] * 37 + 11) % 41) - 20).astype(np.float32) * np.float32(0.03125)).reshape(B, H, W, k)
        g = ((((i * 13 + 5) % 23) - 11).astype(np.float32) * np.float32(0.0625)).reshape(B, H, W, C)
        state = R.make_state(step=4, p=1.0, seed=1, rank=2, target=0.6, interval=2, increment=0.25)
        assert R.tick_host(state) == 0
        params = R.twin_draw(state, 1, B, H, W)
        at = 1
        assert [int(v, 16) for v in out[at:at + B * 8]] == params.ravel().tolist()
        at += B * 8
        got = np.array([float.fromhex(v) for v in out[at:at + npix * C]], dtype=np.float32)
        assert got.tobytes() == R.twin_fwd(img, cond, params).tobytes()
        at += npix * C
        dgot = np.array([float.fromhex(v) for v in out[at:at + npix * 3]], dtype=np.float32)
        assert dgot.tobytes() == R.twin_bwd(g, params).tobytes()
        at += npix * 3
        flat = R.aligned(g.size, np.float32, g.ravel())
        for _ in range(3):
            assert R.adapt_host(state, flat, g.size) == 0
        step, p, pos, neg, steps = out[at].split()
        assert (int(step), float.fromhex(p), int(pos), int(neg), int(steps)) == (
            5, R.state_p(state), int(state[R.POS]), int(state[R.NEG]), int(state[R.STEPS]))
        assert int(steps) == 1 and R.state_p(state) == 0.75
    bad = subprocess.run([exe, '0', '4', '4', '1'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert bad.returncode == 0 and bad.stdout.split('\n')[0] == str(L.EINVAL) and 'Sanitizer' not in bad.stdout


# ------------------------------------------------------------------------------------------------ options (host only)
def _opt(**kw):
    return types.SimpleNamespace(**kw)


def test_options_parse():
    from hoig_amd.d_augment import parse_options
    assert parse_options(_opt(), {}) is None
    for off in ('', 'off', None, False, ' OFF '):
        assert parse_options(_opt(d_augment=off), {}) is None
    assert parse_options(_opt(), {'HOIG_D_AUGMENT': ''}) is None and parse_options(_opt(), {'HOIG_D_AUGMENT': 'off'}) is None
    full = parse_options(_opt(d_augment='color,translation,cutout'), {})
    assert full == dict(policy=7, p=1.0, adaptive=False, target=0.6, interval=4, kimg=500.0, seed=0)
    assert parse_options(_opt(d_augment=' Cutout , color '), {})['policy'] == R.CUTOUT | R.COLOR
    env = parse_options(_opt(), {'HOIG_D_AUGMENT': 'translation', 'HOIG_D_AUGMENT_P': '0.25'})
    assert (env['policy'], env['p'], env['adaptive']) == (R.TRANSLATION, 0.25, False)
    won = parse_options(_opt(d_augment='color', d_augment_p=0.5), {'HOIG_D_AUGMENT': 'cutout', 'HOIG_D_AUGMENT_P': 'adaptive'})
    assert (won['policy'], won['p'], won['adaptive']) == (R.COLOR, 0.5, False)                # (the option wins)
    ada = parse_options(_opt(d_augment='color', d_augment_p='adaptive', d_augment_target=0.5, d_augment_interval=8, d_augment_kimg=100,
                             d_augment_seed=9), {})
    assert ada == dict(policy=R.COLOR, p=0.0, adaptive=True, target=0.5, interval=8, kimg=100.0, seed=9)
    assert parse_options(_opt(d_augment='color', d_augment_p=0), {})['p'] == 0.0


@pytest.mark.parametrize('bad', ['colour', 'color,flip', 'color;cutout', 'on'])
def test_options_refuse_an_unknown_word(bad):
    from hoig_amd.d_augment import parse_options
    with pytest.raises(ValueError, match='d_augment'):
        parse_options(_opt(d_augment=bad), {})
    with pytest.raises(ValueError, match='d_augment'):
        parse_options(_opt(), {'HOIG_D_AUGMENT': bad})


@pytest.mark.parametrize('bad', [-0.1, 1.5, 'x', float('nan'), True])
def test_options_refuse_a_probability_outside_the_unit_interval(bad):
    from hoig_amd.d_augment import parse_options
    with pytest.raises(ValueError, match='d_augment_p'):
        parse_options(_opt(d_augment='color', d_augment_p=bad), {})
    assert parse_options(_opt(d_augment_p=bad), {}) is None          # (not read with the option off)


def test_options_refuse_a_bad_adaptive_schedule():
    from hoig_amd.d_augment import parse_options
    for kw in (dict(d_augment_interval=0), dict(d_augment_kimg=0), dict(d_augment_target=1.5)):
        with pytest.raises(ValueError, match='adaptive'):
            parse_options(_opt(d_augment='color', d_augment_p='adaptive', **kw), {})
        assert parse_options(_opt(d_augment='color', **kw), {})['adaptive'] is False      # (read only in adaptive mode)
