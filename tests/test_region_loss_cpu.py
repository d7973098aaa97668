"""The opt-in region reconstruction term of G through its CPU twin (hoig_amd/csrc/region_loss_host.cpp, the inline functions of
region_loss.h; docs/region_loss.md) against the float64 restatement of tests/region_loss_reference.py, within the bounds the document
derives; the edges of validity; the option parser; the entry point's refusals; and the twin in a program of its own under a host
sanitizer.  tests/test_region_loss_gpu.py compares the kernels with this twin."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import region_loss_reference as R

DEV = 'cpu'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ids = lambda v: 'x'.join(str(s) for s in v)


def test_the_binding_declares_the_head():
    from hoig_amd import _lib as L
    names = set(L.declared_symbols())
    for sym in ('hoig_region_loss', 'hoig_region_loss_host', 'hoig_region_loss_workspace_bytes'):
        assert sym in names and hasattr(L.lib, sym)
    assert (L.RLOSS_THREADS, L.RLOSS_TILE, L.RLOSS_COUNT_TILE, L.RLOSS_MAX_R, L.RLOSS_MAX_N, L.RLOSS_MAX_C) == \
        (R.THREADS, R.TILE, R.COUNT_TILE, R.MAX_R, R.MAX_N, R.MAX_C)
    assert L.RLOSS_MAX_R == L.REGION_MAX and L.REGION_BAD_LABEL == R.BAD_LABEL
    ws = L.lib.hoig_region_loss_workspace_bytes
    # head (counts, ticket, largest bad label), scales and V, rows, one partial of R + 2 doubles per workgroup; blocks of 16 bytes
    assert ws(1, 1, 1, 1, 0) == 16 + 16 + 16 + 16
    assert ws(8, 256, 256, 3, 2) == 112 + 112 + 8 * 4 * 8 + 8 * 48 * 4 * 8
    assert ws(1, 300, 300, 3, 2) - ws(1, 1, 1, 3, 2) == 65 * 4 * 8          # 66 workgroups against 1
    for bad in ((0, 4, 4, 3, 2), (R.MAX_N + 1, 4, 4, 3, 2), (1, 0, 4, 3, 2), (1, 4, 4097, 3, 2), (1, 4, 4, 0, 2), (1, 4, 4, R.MAX_C + 1, 2),
                (1, 4, 4, 3, -1), (1, 4, 4, 3, R.MAX_R + 1), (-1, -1, -1, -1, -1)):
        assert ws(*bad) < 0, bad


@pytest.mark.parametrize('shape', R.SHAPES, ids=_ids)
def test_twin_against_float64(shape):
    pred, target, labels = R.case(shape)
    want = R.reference(pred, target, labels)
    got = R.run(DEV, pred, target, labels)
    rg, rv = R.check(got, want, shape)
    print('region_loss ratio %s gradient %.4f value %.4f' % (_ids(shape), rg, rv))
    assert (want['sign'] == 0).any() or shape[1] * shape[2] < 4         # (elements with d exactly 0 are in the case)
    # the frame part in the region slot when term_all has none of its own
    one = R.run(DEV, pred, target, labels, split=False)
    R.check(one, want, shape)
    assert one['dpred'].tobytes() == got['dpred'].tobytes()


@pytest.mark.parametrize('regions', [0, 1, 7])
def test_other_region_counts_against_float64(regions):
    pred, target, labels = R.case((2, 9, 13, 3), seed=regions, regions=regions)
    lam = tuple(0.5 * r for r in range(regions + 1))
    want = R.reference(pred, target, labels, lam=lam, min_pixels=2)
    R.check(R.run(DEV, pred, target, labels, lam=lam, min_pixels=2), want, regions)
    assert want['V'].min() > 0


def _edge_case():
    """(3, 16, 16, 3), min_pixels 10: image 0 without a hand pixel, image 1 with a hand of 9, image 2 with one of exactly 10."""
    pred, target, labels = R.case((3, 16, 16, 3), seed=3)
    labels[labels == 1] = 0
    labels[1].reshape(-1)[5:14] = 1
    labels[2].reshape(-1)[20:30] = 1
    return pred, target, labels


def test_a_row_is_valid_from_min_pixels_on():
    pred, target, labels = _edge_case()
    want = R.reference(pred, target, labels, min_pixels=10)
    got = R.run(DEV, pred, target, labels, min_pixels=10)
    R.check(got, want)
    assert got['counts'][:, 1].tolist() == [0, 9, 10] and want['V'].tolist() == [3, 1, 3]
    # the hand pixels of the invalid row carry the frame part alone, exactly; those of the valid row more
    fa = np.float32(R.LAM_ALL / pred.size)
    hand1, hand2 = np.abs(got['dpred'][1][labels[1] == 1]), np.abs(got['dpred'][2][labels[2] == 1])
    assert set(np.unique(hand1).tolist()) <= {0.0, float(fa)}
    assert (hand2[hand2 > 0] > fa).all()
    # one pixel more and image 1 counts: V_hand = 2
    assert R.reference(pred, target, labels, min_pixels=9)['V'].tolist() == [3, 2, 3]
    R.check(R.run(DEV, pred, target, labels, min_pixels=9), R.reference(pred, target, labels, min_pixels=9))


def test_with_no_valid_image_the_region_term_is_exactly_zero():
    pred, target, labels = _edge_case()
    lam = (0.0, 10.0, 0.0)
    got = R.run(DEV, pred, target, labels, lam=lam, min_pixels=11)
    want = R.reference(pred, target, labels, lam=lam, min_pixels=11)
    R.check(got, want)
    assert want['V'][1] == 0 and float(got['terms_r'][1]) == 0.0 and float(got['term'][0]) == 0.0
    fa = np.float32(R.LAM_ALL / pred.size)
    assert np.array_equal(got['dpred'], (want['sign'] * np.float64(fa)).astype(np.float32))       # the frame part, exactly
    assert all(np.isfinite(v).all() for v in got.values())
    # ... and with every region invalid and no frame weight, nothing but zeros
    none = R.run(DEV, pred, target, labels, lam=(0.0, 1.0, 1.0), lam_all=0.0, min_pixels=100000)
    assert not none['dpred'].any() and not none['term'].any() and not none['terms_r'].any() and not none['term_all'].any()


def test_sign_of_zero_is_zero_by_value():
    """hoig_loss_accumulate(HOIG_LOSS_L1) gives d > 0 ? 1 : (d < 0 ? -1 : 0) (pointwise.hip): 0 at d = +0 and d = -0."""
    pred = np.array([0.5, 0.25, -0.0, 0.0, -1.0, 2.0], np.float32).reshape(1, 1, 2, 3)
    target = np.array([0.5, 0.5, 0.0, -0.0, -1.0, 1.0], np.float32).reshape(1, 1, 2, 3)
    labels = np.array([[[1, 2]]], np.uint8)
    got = R.run(DEV, pred, target, labels, lam=(0.0, 3.0, 6.0), lam_all=6.0, min_pixels=1)
    # frame part 6 / 6 = 1; hand: 3 / (1 * 3 * 1) = 1; object: 6 / 3 = 2
    assert got['dpred'].reshape(-1).tolist() == [0.0, -2.0, 0.0, 0.0, 0.0, 3.0]
    assert got['terms_r'].tolist() == [0.0, np.float32(0.25 / 3), np.float32(1.0 / 3)]
    assert float(got['term_all'][0]) == np.float32(6.0 * (1.25 / 6)) and float(got['term'][0]) == np.float32(3.0 * (0.25 / 3) + 6.0 * (1.0 / 3))


def test_a_label_above_r_is_in_the_frame_only_and_sets_the_status():
    pred, target, labels = R.case((2, 16, 16, 3), seed=5)
    labels[1, 3, 4] = 7
    labels[0, 0, 9] = 5
    want = R.reference(pred, target, labels)
    got = R.run(DEV, pred, target, labels)
    R.check(got, want)
    assert int(got['status'][0]) == (R.BAD_LABEL | (7 << 8)) and got['counts'].sum() == 2 * 256 - 2
    fa = np.float32(R.LAM_ALL / pred.size)
    assert set(np.abs(got['dpred'][1, 3, 4]).tolist()) <= {0.0, float(fa)}
    # with 7 regions the same map is clean
    lam7 = (0.0, 10.0, 2.5, 0.0, 0.0, 1.0, 0.0, 2.0)
    got7 = R.run(DEV, pred, target, labels, lam=lam7, min_pixels=1)
    R.check(got7, R.reference(pred, target, labels, lam=lam7, min_pixels=1))
    assert int(got7['status'][0]) == 0 and got7['counts'][1, 7] == 1


def test_a_nan_in_pred_gets_the_gradient_zero_and_makes_its_sums_nan():
    pred, target, labels = R.case((2, 16, 16, 3), seed=6)
    labels[0, 2, 2] = 1
    pred[0, 2, 2, 1] = np.nan
    got = R.run(DEV, pred, target, labels)
    clean = pred.copy()
    clean[0, 2, 2, 1] = target[0, 2, 2, 1]
    ref = R.run(DEV, clean, target, labels)
    assert np.array_equal(got['dpred'], ref['dpred']) and got['dpred'][0, 2, 2, 1] == 0.0        # sign(NaN) = 0, like sign(0)
    assert np.isnan(got['term_all'][0]) and np.isnan(got['term'][0]) and np.isnan(got['terms_r'][1])
    assert got['terms_r'][2] == ref['terms_r'][2] and got['terms_r'][0] == ref['terms_r'][0]       # the object's sum holds no NaN
    assert np.array_equal(got['counts'], ref['counts']) and int(got['status'][0]) == 0


def test_null_outputs_leave_the_rest_unchanged():
    pred, target, labels = R.case(R.SHAPES[3], seed=7)
    full = R.run(DEV, pred, target, labels)
    for kw in (dict(grads=False), dict(reports=False), dict(counts=False), dict(grads=False, reports=False, counts=False)):
        part = R.run(DEV, pred, target, labels, **kw)
        for k, v in part.items():
            assert v is None or v.tobytes() == full[k].tobytes(), (kw, k)
        assert all(part[k] is None for k, name in (('dpred', 'grads'), ('terms_r', 'reports'), ('counts', 'counts')) if name in kw)


def test_the_slots_are_added_to():
    pred, target, labels = R.case(R.SHAPES[2], seed=8)
    zero, one = R.run(DEV, pred, target, labels), R.run(DEV, pred, target, labels, init=1.0)
    for k in ('term', 'terms_r', 'term_all'):
        assert np.array_equal(one[k], np.float32(1.0) + zero[k])
    assert one['dpred'].tobytes() == zero['dpred'].tobytes()


def test_entry_point_refuses_bad_arguments():
    import ctypes
    from hoig_amd import _lib as L
    from hoig_amd._twin import ptr
    p, t, d = torch.zeros(2, 4, 4, 3), torch.zeros(2, 4, 4, 3), torch.zeros(2, 4, 4, 3)
    lab, slot, cnt, st = torch.zeros(2, 4, 4, dtype=torch.uint8), torch.zeros(4), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    lam = (ctypes.c_double * 8)(0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    lamp = ctypes.cast(lam, ctypes.c_void_p)
    neg, nan = (ctypes.c_double * 3)(0.0, -1.0, 1.0), (ctypes.c_double * 3)(0.0, float('nan'), 1.0)
    good = [ptr(p), ptr(t), ptr(lab), 2, 4, 4, 3, 2, lamp, 1.0, 4, ptr(d), ptr(slot), None, None, ptr(cnt), ptr(st)]
    assert L.lib.hoig_region_loss_host(*good) == L.OK
    for i, v in ((0, None), (1, None), (2, None), (3, 0), (3, -2), (3, R.MAX_N + 1), (4, -1), (5, 0), (5, 4097), (6, 0), (6, -3), (6, R.MAX_C + 1),
                 (7, -1), (7, R.MAX_R + 1), (8, None), (8, ctypes.cast(neg, ctypes.c_void_p)), (8, ctypes.cast(nan, ctypes.c_void_p)),
                 (9, -1.0), (9, float('inf')), (9, float('nan')), (10, 0), (10, -5), (11, d.data_ptr() + 2), (11, p.data_ptr()),
                 (11, t.data_ptr() + 16), (12, None), (12, slot.data_ptr() + 1), (13, slot.data_ptr() + 2), (14, slot.data_ptr() + 3),
                 (15, cnt.data_ptr() + 1), (16, None), (16, st.data_ptr() + 2)):
        bad = list(good)
        bad[i] = v
        assert L.lib.hoig_region_loss_host(*bad) == L.EINVAL, (i, v)
    assert not d.any() and not slot.any()


def test_the_python_head_checks_its_tensors():
    from hoig_amd import region_loss as RL
    p, lab, slot = torch.zeros(1, 4, 4, 3), torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1)
    with pytest.raises(TypeError):
        RL.head(p.double(), p.double(), lab, (0, 1, 1), 1.0, 4, slot)
    with pytest.raises(ValueError):
        RL.head(p, p, lab[:, :2], (0, 1, 1), 1.0, 4, slot)
    with pytest.raises(ValueError):
        RL.head(p, p, lab, (0, 1, 1), 1.0, 4, slot, terms_r=torch.zeros(2))


# ------------------------------------------------------------------------------------------------ options
def _opt(**kw):
    return types.SimpleNamespace(**kw)


def test_the_parser_accepts_the_documented_spellings():
    from hoig_amd.region_loss import active, parse_options
    d = parse_options(_opt(), environ={})
    assert d == dict(hand=0.0, obj=0.0, views='both', min_pixels=64) and not active(d)
    d = parse_options(_opt(lambda_rec_hand=10, lambda_rec_obj='2.5', region_loss_views=' SRC ', region_loss_min_pixels='4'), environ={})
    assert d == dict(hand=10.0, obj=2.5, views='src', min_pixels=4) and active(d)
    d = parse_options(_opt(), environ={'HOIG_LAMBDA_REC_HAND': '3', 'HOIG_LAMBDA_REC_OBJ': ''})
    assert d == dict(hand=3.0, obj=0.0, views='both', min_pixels=64) and active(d)
    # the option wins over the environment; '' and None are unset
    d = parse_options(_opt(lambda_rec_hand=0, lambda_rec_obj=None), environ={'HOIG_LAMBDA_REC_HAND': '3', 'HOIG_LAMBDA_REC_OBJ': '1'})
    assert (d['hand'], d['obj']) == (0.0, 1.0) and active(d)
    assert active(parse_options(_opt(lambda_rec_obj=1e-3, region_loss_views='tsf', region_loss_min_pixels=1.0), environ={}))


@pytest.mark.parametrize('kw,word', [
    (dict(lambda_rec_hand=-1.0), 'lambda_rec_hand'), (dict(lambda_rec_hand='much'), 'lambda_rec_hand'),
    (dict(lambda_rec_hand=float('nan')), 'lambda_rec_hand'), (dict(lambda_rec_hand=float('inf')), 'lambda_rec_hand'),
    (dict(lambda_rec_hand=True), 'lambda_rec_hand'), (dict(lambda_rec_obj=-0.5), 'lambda_rec_obj'), (dict(lambda_rec_obj=[1]), 'lambda_rec_obj'),
    (dict(region_loss_views='all'), 'region_loss_views'), (dict(region_loss_views=1), 'region_loss_views'),
    (dict(region_loss_min_pixels=0), 'region_loss_min_pixels'), (dict(region_loss_min_pixels=2.5), 'region_loss_min_pixels'),
    (dict(region_loss_min_pixels='few'), 'region_loss_min_pixels'), (dict(region_loss_min_pixels=True), 'region_loss_min_pixels'),
    (dict(region_loss_min_pixels=-3), 'region_loss_min_pixels')], ids=str)
def test_the_parser_raises_on_each_bad_value(kw, word):
    from hoig_amd.region_loss import parse_options
    with pytest.raises(ValueError, match=word) as ex:
        parse_options(_opt(**kw), environ={})
    assert repr(list(kw.values())[0]) in str(ex.value)          # the offending value is in the message
    with pytest.raises(ValueError, match='lambda_rec_obj'):
        parse_options(_opt(), environ={'HOIG_LAMBDA_REC_OBJ': 'x'})


def test_the_autograd_function_on_cpu_tensors_adds_twice_into_one_slot():
    from hoig_amd import region_loss as RL
    pred, target, labels = R.case(R.SHAPES[2], seed=9)

    class Slots(object):                     # (ops.LossSlots needs the device library's hoig_sum: the layout alone is enough here)
        buf = torch.zeros(6)

    s = Slots()
    tp = torch.from_numpy(pred).requires_grad_(True)
    for _ in range(2):
        out = RL.region_l1_loss(tp, torch.from_numpy(target), torch.from_numpy(labels), R.LAM, R.LAM_ALL, R.MIN_PIXELS, (s, 0),
                                into_regions=(s, 2), into_all=(s, 1))
    out.backward()
    once = R.run(DEV, pred, target, labels)
    assert tp.grad.numpy().tobytes() == once['dpred'].tobytes()
    assert s.buf[0] == once['term'][0] + once['term'][0] and s.buf[1] == once['term_all'][0] + once['term_all'][0]
    assert np.array_equal(s.buf[2:5].numpy(), once['terms_r'] + once['terms_r']) and s.buf[5] == 0


# ------------------------------------------------------------------------------------------------ the twin under a sanitizer
def test_the_twin_under_a_host_sanitizer_build(tmp_path):
    """region_loss_host.cpp built with -fsanitize=address,undefined into a program of its own (tests/region_loss_asan_driver.cpp), every
    buffer a heap block of exactly its size, at the shapes above: no report, and the library twin's bits."""
    # (the compiler, the flags and the reasons for them: tests/test_grad_guard_cpu.py)
    cxx = shutil.which(os.environ.get('CXX', 'c++'))
    assert cxx is not None, 'no host C++ compiler (c++, or $CXX) on PATH'
    flags = ['-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
             '-static-libasan']
    exe = str(tmp_path / 'region_loss_asan_driver')
    src = [os.path.join(ROOT, 'hoig_amd', 'csrc', 'region_loss_host.cpp'), os.path.join(ROOT, 'tests', 'region_loss_asan_driver.cpp')]
    build = subprocess.run([cxx] + flags + ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'hoig_amd', 'csrc')] + src +
                           ['-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    for shape in R.SHAPES:
        N, H, W, C = shape
        run = subprocess.run([exe] + [str(v) for v in shape], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert run.returncode == 0 and 'Sanitizer' not in run.stdout and 'runtime error' not in run.stdout, run.stdout[-3000:]
        lines = run.stdout.strip().split('\n')
        assert len(lines) == 2 and all(ln.split()[0] == '0' for ln in lines), run.stdout[:500]
        # the driver's inputs (its functions `value` and `label`), through the library's twin
        k = np.arange(N * H * W * C, dtype=np.int64)
        pred = (((k * 37) % 41 - 20).astype(np.float32) * np.float32(0.046875)).reshape(shape)
        target = (((k * 29 + 7) % 43 - 21).astype(np.float32) * np.float32(0.046875)).reshape(shape)
        q = np.arange(N * H * W, dtype=np.int64)
        labels = np.where(q % 97 == 96, 7, (q * 5 + q // 3) % 3).astype(np.uint8).reshape(N, H, W)
        lam = (0.25, 10.0, 2.5)
        got = R.run(DEV, pred, target, labels, lam=lam, lam_all=30.0, min_pixels=2)
        f = lines[0].split()
        assert [float.fromhex(v) for v in f[1:6]] == [float(got['term'][0]), float(got['term_all'][0])] + [float(v) for v in got['terms_r']]
        assert float.fromhex(f[6]) == float(got['dpred'].astype(np.float64).reshape(-1).cumsum()[-1])
        assert int(f[7]) == int(got['status'][0]) and [int(v) for v in f[8:]] == got['counts'].reshape(-1).tolist()
        none = R.run(DEV, pred, target, labels, lam=lam, lam_all=30.0, min_pixels=2, grads=False, reports=False, counts=False, split=False)
        f = lines[1].split()
        assert float.fromhex(f[1]) == float(none['term'][0]) and int(f[2]) == int(none['status'][0])
