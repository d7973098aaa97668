"""The fp64 FID statistics on the MI355X (hoig_amd/csrc/fid_stats.hip through hoig_amd/metrics/fid_device.py): every check of
tests/test_fid_device_cpu.py on the kernels, against the same truths with the same limits (tests/fid_device_reference.py); the stages
that are a function of their input alone equal their CPU twins bit for bit; and Scorer(fid_device=True), the directory functions'
device_stats and the command line's --device-fid against the default path."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fid_device_reference as R
import metrics_reference as MR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
N, DIMS = 12, 64
CALLS = (5, 1, 6)
_p = lambda a: ctypes.c_void_p(a.ctypes.data)
_t = lambda t: ctypes.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------- the kernels against the truths
@pytest.mark.parametrize('shape,f32,accumulate,symmetric', R.GEMM_CASES, ids=R.gemm_id)
def test_gemm_kernel_against_longdouble(shape, f32, accumulate, symmetric):
    R.check_gemm(DEV, shape, f32, accumulate, symmetric)


def test_gemm_kernel_lane_maps_on_exact_integers():
    """Small integers make every product and sum exact, so a wrong row or column map shows as a wrong element, not as an error size:
    more than one workgroup, ragged edges, every mode."""
    from hoig_amd import _lib as L
    from hoig_amd.metrics.fid_device import gemm_tn
    g = np.random.default_rng(2)
    a, b = g.integers(-8, 9, (37, 150)).astype(np.float64), g.integers(-8, 9, (37, 81)).astype(np.float64)
    got = gemm_tn(R.to(DEV, a), R.to(DEV, b), torch.empty((150, 81), dtype=torch.float64, device=DEV))
    assert np.array_equal(R.back(got), a.T @ b)
    ta = R.to(DEV, a)
    got = gemm_tn(ta, ta, torch.ones((150, 150), dtype=torch.float64, device=DEV), L.GEMM_SYMMETRIC | L.GEMM_ACCUMULATE)
    assert np.array_equal(R.back(got), a.T @ a + 1.0)
    ta, pivot = R.to(DEV, a.astype(np.float32)), g.integers(-4, 5, 150).astype(np.float64)
    got = gemm_tn(ta, ta, torch.empty((150, 150), dtype=torch.float64, device=DEV), L.GEMM_SYMMETRIC | L.GEMM_F32, R.to(DEV, pivot))
    assert np.array_equal(R.back(got), (a - pivot).T @ (a - pivot))


def test_moments_kernel_against_mean_and_cov():
    R.check_moments(DEV)


def test_pivoted_cholesky_kernel_and_its_twin_bit_for_bit():
    dev, host = R.check_pchol(DEV), R.check_pchol('cpu')
    for n in dev:
        for got, want in zip(dev[n], host[n]):
            assert np.array_equal(got, want), n


@pytest.mark.parametrize('name', sorted(R.eig_matrices()))
def test_eigenvalue_kernel_against_eigvalsh_and_its_twin_bit_for_bit(name):
    from hoig_amd import _lib as L
    a = R.eig_matrices()[name]
    n = a.shape[0]
    lam = R.check_eigvals(DEV, name, a)
    # the twin's tridiagonal, and bisection on it: the same code on equal input
    d, e, want = np.zeros(n), np.zeros(n), np.zeros(n)
    assert L.lib.hoig_sym_tridiag_f64_host(_p(a), n, n, _p(d), _p(e)) == 0
    assert L.lib.hoig_tridiag_eigvals_f64_host(_p(d), _p(e), n, _p(want)) == 0
    td, te, got = R.to(DEV, d), R.to(DEV, e), torch.zeros(n, dtype=torch.float64, device=DEV)
    L.call('hoig_tridiag_eigvals_f64', _t(td), _t(te), n, _t(got), torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(R.back(got), want)
    # the kernels' own tridiagonal is the twin's too (every sum in the same order), and so are the eigenvalues
    nbytes = L.lib.hoig_sym_eigvals_f64_workspace_bytes(n)
    ws = torch.zeros(nbytes // 8, dtype=torch.float64, device=DEV)
    out, info = torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    ta = R.to(DEV, a)
    L.call('hoig_sym_eigvals_f64', _t(ta), n, n, _t(out), _t(info), _t(ws), nbytes, torch.cuda.current_stream().cuda_stream)
    tri = R.back(ws)[4 + n * n:4 + n * n + 2 * n]
    assert np.array_equal(tri[:n], d) and np.array_equal(tri[n:2 * n - 1], e[:n - 1])
    assert np.array_equal(R.back(out), want) and np.array_equal(lam, want)


@pytest.mark.parametrize('case', R.TRACE_CASES, ids=lambda c: '%d-%d' % c)
def test_trace_kernels_against_mpmath(case):
    R.check_trace(DEV, case)


def test_trace_kernels_closed_form_2048():
    R.check_closed_form(DEV)


def test_a_non_finite_entry_is_a_status_on_the_device():
    from hoig_amd.metrics import fid_device as F
    s = np.eye(70)
    s[3, 69] = np.nan
    fac, piv, info = F.pivoted_cholesky(R.to(DEV, s))
    assert R.back(info).tolist() == [0, -1] and (R.back(fac) == 0).all() and (R.back(piv) == -1).all()
    lam, einfo = F.sym_eigvals(R.to(DEV, s))
    assert R.back(einfo).tolist() == [-1] and np.isnan(R.back(lam)).all()
    with pytest.raises(ValueError):
        F.frechet_distance_device(np.zeros(70), s, np.zeros(70), np.eye(70))
    with pytest.raises(ValueError):
        F.frechet_distance_device(np.zeros(70), np.eye(70), np.zeros(70), np.eye(71))


# ---------------------------------------------------------------------------------------------- the scorer and the path functions
@pytest.fixture(scope='module')
def pairs(tmp_path_factory):
    """The recipe of tests/test_metrics_stream_gpu.py: 12 pairs of 256 x 256 PNGs, their bytes on the device, the network."""
    from PIL import Image
    from hoig_amd.metrics.fid import InceptionFeatures
    root = tmp_path_factory.mktemp('fid_pairs')
    a, b = str(root / 'gen'), str(root / 'gt')
    read = lambda names: torch.from_numpy(np.stack([np.asarray(Image.open(n).convert('RGB')) for n in names])).to(DEV)
    gen, gt = read(MR.write_pngs(a, N, 256, 20)), read(MR.write_pngs(b, N, 256, 21))
    sd = MR.inception_state_dict(5)
    return dict(dirs=[a, b], gen=gen, gt=gt, sd=sd, inception=InceptionFeatures(sd, DIMS, None, DEV), root=root)


def _scorer(p, **over):
    from hoig_amd.metrics.stream import Scorer
    kw = dict(fid=p['inception'], lpips=None, ssim=False)
    kw.update(over)
    return Scorer(**kw)


def _feed(s, gen, gt, calls=CALLS):
    at = 0
    for n in calls:
        s.update(gen[at:at + n], gt[at:at + n])
        at += n
    assert at == gen.shape[0]
    return s


def _fid_limit(tr):
    """2 (recorded rank-deficient limit + scipy's recorded error) Tr: 12 images in 64 dims are rank 11."""
    return 2 * (R.trace_limit((40, 25)) + R.SCIPY_RANK_DEFICIENT) * tr


def _trace_of(fid, stats1, stats2):
    (m1, s1), (m2, s2) = stats1, stats2
    return 0.5 * ((m1 - m2).dot(m1 - m2) + np.trace(s1) + np.trace(s2) - fid)


@pytest.mark.parametrize('fid_batch', [50, 5])
def test_the_scorer_with_device_fid_against_the_default_path(pairs, fid_batch):
    """fid_batch 50: everything is the short last batch of result(); 5: two streamed batches of each set and a short one."""
    from hoig_amd.metrics.fid import get_activations
    plain = _feed(_scorer(pairs, fid_batch=fid_batch, fid_device=False), pairs['gen'], pairs['gt'])
    dev = _feed(_scorer(pairs, fid_batch=fid_batch, fid_device=True), pairs['gen'], pairs['gt'])
    assert dev.fid_device and not plain.fid_device and (dev._feat_gen.n == (0 if fid_batch == 50 else 10))
    want_mu, want_sigma = plain.statistics()
    mu, sigma = dev.statistics()
    x = get_activations(sorted(os.path.join(pairs['dirs'][0], f) for f in os.listdir(pairs['dirs'][0])), pairs['inception'], fid_batch, DIMS)
    assert np.array_equal(np.mean(x, axis=0), want_mu)                      # (the same features in the same batches)
    lim_mu, lim_sigma = R.moments_limits(x, x[:min(fid_batch, N)].mean(0))
    e_mu, e_sigma = np.abs(mu - want_mu), np.abs(sigma - want_sigma)
    print('mu err / limit %.3g sigma err / limit %.3g' % ((e_mu / lim_mu).max(), (e_sigma / lim_sigma).max()))
    assert (e_mu <= lim_mu).all() and (e_sigma <= lim_sigma).all()
    want, got = plain.result(), dev.result()
    assert sorted(got) == ['fid', 'n'] and got['n'] == N
    tr = _trace_of(want['fid'], plain.statistics(), (lambda s: s._statistics(s._feat_gt, s._fid_gt))(plain))
    print('fid', got['fid'], 'default', want['fid'], 'Tr', tr, 'limit', _fid_limit(tr))
    assert tr > 0 and abs(got['fid'] - want['fid']) <= _fid_limit(tr)
    # another grouping of the updates: the same batches reach the kernels, so the same value
    other = _feed(_scorer(pairs, fid_batch=fid_batch, fid_device=True), pairs['gen'], pairs['gt'], (3, 4, 5)).result()
    assert abs(other['fid'] - got['fid']) <= _fid_limit(tr)
    assert other['fid'] == got['fid']


def test_result_leaves_the_device_state_as_it_is(pairs):
    s = _scorer(pairs, fid_batch=5, fid_device=True)
    _feed(s, pairs['gen'][:7], pairs['gt'][:7], (3, 4))
    part = s.result()
    assert part['n'] == 7 and s._feat_gen.n == 5
    assert part == s.result()
    _feed(s, pairs['gen'][7:], pairs['gt'][7:], (5,))
    fresh = _feed(_scorer(pairs, fid_batch=5, fid_device=True), pairs['gen'], pairs['gt'], (12,))
    assert s.result() == fresh.result()
    assert all(np.array_equal(a, b) for a, b in zip(s.statistics(), fresh.statistics()))


def test_fid_reference_as_npz_and_as_a_tuple(pairs):
    ref = _feed(_scorer(pairs, fid_batch=5, fid_device=True), pairs['gt'], pairs['gen'])
    path = str(pairs['root'] / 'gt_stats_device.npz')
    ref.save_statistics(path)
    with np.load(path) as f:
        assert sorted(f.keys()) == ['mu', 'sigma'] and f['mu'].shape == (DIMS,) and f['sigma'].shape == (DIMS, DIMS)
        mu, sigma = f['mu'][:], f['sigma'][:]
    both = _feed(_scorer(pairs, fid_batch=5, fid_device=True), pairs['gen'], pairs['gt']).result()
    for given in (path, (mu, sigma)):
        got = _feed(_scorer(pairs, fid_batch=5, fid_device=True, fid_reference=given), pairs['gen'], pairs['gt']).result()
        assert got == both


def test_update_does_not_wait_for_the_device(pairs):
    """Under torch's sync debug mode a device-to-host copy raises: the default path's update() does, the device path's does not."""
    dev, plain = _scorer(pairs, fid_batch=5, fid_device=True), _scorer(pairs, fid_batch=5, fid_device=False)
    for s in (dev, plain):
        s.update(pairs['gen'][:5], pairs['gt'][:5])                # (first use: whatever the network sets up lazily)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        dev.update(pairs['gen'][5:], pairs['gt'][5:])
        with pytest.raises(RuntimeError):
            plain.update(pairs['gen'][5:], pairs['gt'][5:])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert dev._feat_gen.n == 10 and dev.result()['n'] == N


def test_the_path_functions_and_the_command_line(pairs, tmp_path):
    from hoig_amd.metrics.__main__ import main
    from hoig_amd.metrics.fid import calculate_fid_given_paths, compute_statistics_of_path
    weights = str(tmp_path / 'inception.pth')
    torch.save(pairs['sd'], weights)
    want = calculate_fid_given_paths(pairs['dirs'], 5, DEV, DIMS, weights=pairs['sd'], device_stats=False)
    got = calculate_fid_given_paths(pairs['dirs'], 5, DEV, DIMS, weights=pairs['sd'], device_stats=True)
    stats = [compute_statistics_of_path(d, pairs['inception'], 5, DIMS) for d in pairs['dirs']]
    tr = _trace_of(want, *stats)
    print('paths', got, want, 'Tr', tr, 'limit', _fid_limit(tr))
    assert abs(got - want) <= _fid_limit(tr)
    argv = ['fid'] + pairs['dirs'] + ['--batch-size', '5', '--dims', str(DIMS), '--inception-weights', weights]
    assert main(argv) == want
    env = {k: v for k, v in os.environ.items() if k != 'HOIG_DEVICE_FID'}
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    run = subprocess.run([sys.executable, '-m', 'hoig_amd.metrics'] + argv + ['--device-fid'], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:]
    lines = [line for line in run.stdout.split('\n') if line.startswith('FID: ')]
    assert len(lines) == 1
    assert float(lines[0].split()[1]) == got
