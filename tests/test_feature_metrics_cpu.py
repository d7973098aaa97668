"""KID and precision / recall through their CPU twins (hoig_amd/csrc/feature_metrics_host.cpp, the per-lane code of
feature_metrics.h): the checks, truths and limits of tests/feature_metrics_reference.py on device 'cpu'.
tests/test_feature_metrics_gpu.py runs the same ones on the kernels."""
import ctypes

import numpy as np
import pytest
import torch

import feature_metrics_reference as R

_p = lambda a: ctypes.c_void_p(a.ctypes.data)

SYMBOLS = ('hoig_kid_workspace_bytes', 'hoig_kid_poly_f64', 'hoig_kid_poly_f64_host', 'hoig_kid_finish_f64', 'hoig_kid_finish_f64_host',
           'hoig_knn_workspace_bytes', 'hoig_knn_radius_f64', 'hoig_knn_radius_f64_host', 'hoig_manifold_hits_workspace_bytes',
           'hoig_manifold_hits_f64', 'hoig_manifold_hits_f64_host')


def test_the_binding_declares_the_feature_metrics():
    from hoig_amd import _lib as L
    names = set(L.declared_symbols())
    for sym in SYMBOLS:
        assert sym in names and hasattr(L.lib, sym)
        assert sym in L._SIGS or sym.endswith('_workspace_bytes')


def test_workspace_sizes():
    from hoig_amd import _lib as L
    lib = L.lib
    assert 0 < lib.hoig_kid_workspace_bytes(100, 1000) < 8 * 1000 ** 2            # no Gram matrix can hide in it
    assert lib.hoig_kid_workspace_bytes(100, 1000) == 100 * 3 * 16 * 16 * 8
    for S, m in ((0, 1000), (-1, 1000), (100, 1), (100, 0)):
        assert lib.hoig_kid_workspace_bytes(S, m) == L.EINVAL
    assert lib.hoig_knn_workspace_bytes(1) == L.EINVAL and lib.hoig_knn_workspace_bytes(130) == (130 + 2 * 130 * 8) * 8
    assert lib.hoig_manifold_hits_workspace_bytes(0, 5) == L.EINVAL
    assert lib.hoig_manifold_hits_workspace_bytes(130, 33) == (130 + 33) * 8 + 2 * 33 * 4


@pytest.mark.parametrize('case', R.KID_CASES, ids=R.kid_id)
def test_kid_twin_against_longdouble(case):
    R.check_kid('cpu', case)


@pytest.mark.parametrize('onehot', [False, True], ids=['integers', 'onehot'])
def test_kid_twin_lane_maps_on_exact_integers(onehot):
    R.check_kid_exact('cpu', onehot)


def test_kid_finishing_twin():
    R.check_finish('cpu')


@pytest.mark.parametrize('case', R.RADII_CASES, ids=lambda c: '%dx%d-k%d' % c)
def test_radii_twin_against_sorted_longdouble_distances(case):
    R.check_radii('cpu', case)


def test_radii_twin_of_duplicated_rows():
    """Two equal rows: their radius is 0 for k = 1 (within the limit; the norms and the product round apart), never negative, never NaN."""
    R.check_radii('cpu', (40, 37, 1), duplicate=True)
    R.check_radii('cpu', (40, 37, 3), duplicate=True)


def test_the_reference_counts_are_informative():
    assert R.prc_reference_is_informative()


@pytest.mark.parametrize('case', R.PRC_CASES, ids=R.prc_id)
def test_hits_twin_counts_equal_the_reference(case):
    R.check_prc('cpu', case)


def test_kid_from_features_draw_order_and_arguments():
    """The documented draw: one RandomState(seed), per subset choice(nx, m) then choice(ny, m); the value is kid_sums on that table."""
    from hoig_amd.metrics import feature_metrics as F
    x, y, _, _ = R.kid_inputs((37, 65, 1, 3))
    tx, ty = torch.from_numpy(x), torch.from_numpy(y)
    rng = np.random.RandomState(4)
    ix, iy = [], []
    for _ in range(3):
        ix.append(rng.choice(x.shape[0], 20, replace=False))
        iy.append(rng.choice(y.shape[0], 20, replace=False))
    out, _ = F.kid_sums(tx, ty, np.stack(ix), np.stack(iy), 2, 0.25, 0.5)
    mmd = out[:, 3].numpy()
    assert F.kid_from_features(tx, ty, subsets=3, subset_size=20, seed=4, degree=2, gamma=0.25, coef0=0.5) == (float(np.mean(mmd)), float(np.std(mmd)))
    # m = min(subset_size, nx, ny); gamma None is 1 / dims
    assert F.kid_from_features(tx, ty, subsets=2) == F.kid_from_features(tx, ty, subsets=2, subset_size=y.shape[0], gamma=1.0 / 37)
    with pytest.raises(ValueError):
        F.kid_from_features(tx[:1], ty)                    # m < 2
    with pytest.raises(ValueError):
        F.kid_from_features(tx, ty, degree=5)
    with pytest.raises(ValueError):
        F.kid_from_features(tx, ty[:, :5])
    with pytest.raises(ValueError):
        F.precision_recall_from_features(tx, ty, k=9)


def test_status_words():
    from hoig_amd import _lib as L
    from hoig_amd.metrics import feature_metrics as F
    x, y, ix, iy = R.kid_inputs((5, 17, 3, 3))
    # a NaN feature: the status, a NaN result, and a ValueError from the Python layer
    bad = x.copy()
    bad[ix[1, 4], 2] = np.nan
    out, status = F.kid_sums(torch.from_numpy(bad), torch.from_numpy(y), ix, iy)
    assert status.tolist() == [L.FM_NONFINITE] and np.isnan(out.numpy()).all()
    with pytest.raises(ValueError):
        F.kid_from_features(torch.from_numpy(bad), torch.from_numpy(y), subsets=2)
    with pytest.raises(ValueError):
        F.precision_recall_from_features(torch.from_numpy(bad), torch.from_numpy(y[:, :5]))
    # an index outside its set is refused on the host
    for table in (ix, iy):
        for value in (-1, 99):
            wrong = table.copy()
            wrong[2, 0] = value
            with pytest.raises(ValueError):
                F.kid_sums(torch.from_numpy(x), torch.from_numpy(y), *((wrong, iy) if table is ix else (ix, wrong)))
    # the kernels' own clamp, on the twin: the table reaches the entry point unchecked; nothing outside X is read, the status says so
    wrong = ix.copy()
    wrong[0, 3], wrong[2, 5] = 10 ** 6, -7
    out, status = np.zeros((3, 4)), np.zeros(1, np.int32)
    xs, ys = np.ascontiguousarray(x), np.ascontiguousarray(y)
    assert L.lib.hoig_kid_poly_f64_host(_p(xs), xs.shape[0], _p(ys), ys.shape[0], 5, _p(wrong), _p(iy), 3, 17, 0.2, 1.0, 3, _p(out),
                                        _p(status)) == 0
    assert status.tolist() == [L.FM_CLAMPED] and np.isnan(out).all()
    # invalid arguments are refused before anything is written
    out[:] = 5.0
    call = lambda **kw: L.lib.hoig_kid_poly_f64_host(_p(xs), kw.get('nx', xs.shape[0]), _p(ys), ys.shape[0], kw.get('D', 5), _p(ix), _p(iy),
                                                     kw.get('S', 3), kw.get('m', 17), 0.2, 1.0, kw.get('degree', 3), _p(out), _p(status))
    for kw in (dict(nx=0), dict(D=0), dict(S=0), dict(m=1), dict(degree=0), dict(degree=5)):
        assert call(**kw) == L.EINVAL
    assert (out == 5.0).all()
    # the device entries refuse the same before any launch
    assert L.lib.hoig_kid_poly_f64(_p(xs), xs.shape[0], _p(ys), ys.shape[0], 5, _p(ix), _p(iy), 3, 17, 0.2, 1.0, 5, _p(out), _p(status),
                                   _p(out), 1 << 20, None) == L.EINVAL
    assert L.lib.hoig_kid_poly_f64(_p(xs), xs.shape[0], _p(ys), ys.shape[0], 5, _p(ix), _p(iy), 3, 17, 0.2, 1.0, 3, _p(out), _p(status),
                                   _p(out), 8, None) == L.EINVAL                  # workspace too small
    r = np.zeros(24)
    assert L.lib.hoig_knn_radius_f64(_p(xs), xs.shape[0], 5, None, 9, _p(r), _p(status), _p(out), 1 << 20, None) == L.EINVAL
    assert L.lib.hoig_knn_radius_f64_host(_p(xs), xs.shape[0], 5, None, 0, _p(r), _p(status)) == L.EINVAL
    assert L.lib.hoig_manifold_hits_f64(_p(xs), xs.shape[0], _p(r), _p(ys), ys.shape[0], 5, None, _p(out), _p(status), _p(out), 8,
                                        None) == L.EINVAL


def test_feature_bank_and_the_scorer_arguments():
    import inspect
    from hoig_amd.metrics import feature_metrics as F
    from hoig_amd.metrics import stream
    bank = F.FeatureBank(4, 'cpu')
    with pytest.raises(ValueError):
        bank.rows()
    block = torch.arange(8, dtype=torch.float32).reshape(2, 4)
    bank.append(block).append(block[:1] + 100)
    block += 1                                                    # (the bank holds copies)
    other = bank.copy().append(block)
    assert bank.n == 3 and other.n == 5
    assert bank.rows().tolist() == [[0, 1, 2, 3], [4, 5, 6, 7], [100, 101, 102, 103]]
    with pytest.raises(ValueError):
        bank.append(torch.zeros((2, 5)))
    with pytest.raises(ValueError):
        bank.append(torch.zeros((2, 4), dtype=torch.float64))
    params = inspect.signature(stream.Scorer.__init__).parameters
    assert params['kid'].default is None and params['prc'].default is None
    s = stream.Scorer(ssim=False)
    assert s.kid is None and s.prc is None and s._bank_gen is None
    for kw in (dict(kid=True), dict(prc=True), dict(kid={'subsets': 3})):
        with pytest.raises(ValueError):
            stream.Scorer(ssim=False, **kw)                       # no FID network
    with pytest.raises(ValueError):
        F._options(3, 'kid')
