"""KID and precision / recall on the MI355X (hoig_amd/csrc/feature_metrics.hip through hoig_amd/metrics/feature_metrics.py): every
check of tests/test_feature_metrics_cpu.py on the kernels, against the same truths with the same limits
(tests/feature_metrics_reference.py); the finishing stage equals its CPU twin bit for bit; and Scorer(kid=, prc=), the directory
functions and the command line against the feature functions on the same features."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import feature_metrics_reference as R
import metrics_reference as MR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
N, DIMS, SIDE = 12, 64, 64
CALLS = (5, 1, 6)
KID = dict(subsets=4, subset_size=7, seed=3)
PRC = dict(k=2)


# ---------------------------------------------------------------------------------------------- the kernels against the truths
@pytest.mark.parametrize('case', R.KID_CASES, ids=R.kid_id)
def test_kid_kernel_against_longdouble(case):
    R.check_kid(DEV, case)


@pytest.mark.parametrize('onehot', [False, True], ids=['integers', 'onehot'])
def test_kid_kernel_lane_maps_on_exact_integers(onehot):
    R.check_kid_exact(DEV, onehot)


def test_kid_finishing_kernel_and_its_twin_bit_for_bit():
    assert np.array_equal(R.check_finish(DEV), R.check_finish('cpu'))


def test_kid_kernel_on_unaligned_rows():
    """D a multiple of 4 takes the 16-byte loads only from a 16-byte aligned base: a view one float into a buffer takes the scalar
    loads, and both give the sums of the exact-integer case."""
    from hoig_amd.metrics import feature_metrics as F
    g = np.random.default_rng(9)
    x, y = g.integers(-3, 4, (70, 64)).astype(np.float32), g.integers(-3, 4, (66, 64)).astype(np.float32)
    ix, iy = np.stack([g.permutation(70)[:65]]).astype(np.int32), np.stack([g.permutation(66)[:65]]).astype(np.int32)
    want = R.kid_exact_sums(x, y, ix, iy)
    tx, ty = R.to(DEV, x), R.to(DEV, y)
    shifted = torch.zeros(70 * 64 + 1, dtype=torch.float32, device=DEV)[1:].view(70, 64).copy_(tx)
    assert tx.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    for first in (tx, shifted):
        out, status = F.kid_sums(first, ty, ix, iy, 3, 0.125, 1.0)
        assert R.back(status).tolist() == [0] and np.array_equal(R.back(out)[:, :3], want)


@pytest.mark.parametrize('case', R.RADII_CASES, ids=lambda c: '%dx%d-k%d' % c)
def test_radii_kernel_against_sorted_longdouble_distances(case):
    R.check_radii(DEV, case)


def test_radii_kernel_of_duplicated_rows():
    R.check_radii(DEV, (40, 37, 1), duplicate=True)
    R.check_radii(DEV, (40, 37, 3), duplicate=True)


@pytest.mark.parametrize('case', R.PRC_CASES, ids=R.prc_id)
def test_hits_kernel_counts_equal_the_reference(case):
    R.check_prc(DEV, case)


def test_a_nan_feature_is_a_status_on_the_device():
    from hoig_amd import _lib as L
    from hoig_amd.metrics import feature_metrics as F
    x, y, ix, iy = R.kid_inputs((5, 17, 3, 3))
    x[ix[1, 4], 2] = np.nan
    out, status = F.kid_sums(R.to(DEV, x), R.to(DEV, y), ix, iy)
    assert R.back(status).tolist() == [L.FM_NONFINITE] and np.isnan(R.back(out)).all()
    with pytest.raises(ValueError):
        F.kid_from_features(R.to(DEV, x), R.to(DEV, y), subsets=2)
    with pytest.raises(ValueError):
        F.precision_recall_from_features(R.to(DEV, x), R.to(DEV, y))
    wrong = ix.copy()
    wrong[0, 0] = x.shape[0]
    with pytest.raises(ValueError):                                 # (refused on the host: the device never sees a bad table)
        F.kid_sums(R.to(DEV, y), R.to(DEV, y), wrong, iy)


# ---------------------------------------------------------------------------------------------- the scorer and the path functions
@pytest.fixture(scope='module')
def pairs(tmp_path_factory):
    """The recipe of tests/test_fid_device_gpu.py at 64 x 64: 12 pairs of PNGs, their bytes on the device, the network, and the
    features of both directories as get_activations gives them, cast back to fp32."""
    from PIL import Image
    from hoig_amd.metrics.fid import InceptionFeatures, get_activations
    root = tmp_path_factory.mktemp('feature_pairs')
    a, b = str(root / 'gen'), str(root / 'gt')
    read = lambda names: torch.from_numpy(np.stack([np.asarray(Image.open(n).convert('RGB')) for n in names])).to(DEV)
    gen, gt = read(MR.write_pngs(a, N, SIDE, 20)), read(MR.write_pngs(b, N, SIDE, 21))
    sd = MR.inception_state_dict(5)
    net = InceptionFeatures(sd, DIMS, None, DEV)
    files = lambda d: sorted(os.path.join(d, f) for f in os.listdir(d))
    feats = {size: [torch.from_numpy(get_activations(files(d), net, size, DIMS).astype(np.float32)).to(DEV) for d in (a, b)]
             for size in (50, 5)}
    return dict(dirs=[a, b], gen=gen, gt=gt, sd=sd, inception=net, root=root, feats=feats)


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


def _want(p, fid_batch):
    from hoig_amd.metrics import feature_metrics as F
    gen, gt = p['feats'][fid_batch]
    mean, std = F.kid_from_features(gen, gt, **KID)
    want = dict(kid=mean, kid_std=std)
    want.update(F.precision_recall_from_features(gt, gen, **PRC))
    return want


@pytest.mark.parametrize('fid_device', [False, True], ids=['host-fid', 'device-fid'])
@pytest.mark.parametrize('fid_batch', [50, 5])
def test_the_scorer_with_kid_and_prc_equals_the_feature_functions(pairs, fid_batch, fid_device):
    """Bit for bit: the same kernels on the same bytes.  fid_batch 50: everything is the short last batch; 5: two banked batches
    of each stream and a short one."""
    want = _want(pairs, fid_batch)
    assert np.isfinite(list(want.values())).all()
    s = _feed(_scorer(pairs, fid_batch=fid_batch, fid_device=fid_device, kid=KID, prc=PRC), pairs['gen'], pairs['gt'])
    assert s._bank_gen.n == s._bank_gt.n == (0 if fid_batch == 50 else 10)
    got = s.result()
    assert sorted(got) == ['density', 'fid', 'kid', 'kid_std', 'n', 'precision', 'recall']
    assert {k: got[k] for k in want} == want
    assert got['fid'] == _feed(_scorer(pairs, fid_batch=fid_batch, fid_device=fid_device), pairs['gen'], pairs['gt']).result()['fid']
    # result() leaves the state as it is
    assert s.result() == got and s._bank_gen.n == (0 if fid_batch == 50 else 10)


def test_true_takes_the_defaults_and_one_option_alone(pairs):
    from hoig_amd.metrics import feature_metrics as F
    gen, gt = pairs['feats'][5]
    got = _feed(_scorer(pairs, fid_batch=5, kid=True), pairs['gen'], pairs['gt']).result()
    assert sorted(got) == ['fid', 'kid', 'kid_std', 'n'] and (got['kid'], got['kid_std']) == F.kid_from_features(gen, gt)
    got = _feed(_scorer(pairs, fid_batch=5, prc=True), pairs['gen'], pairs['gt']).result()
    assert sorted(got) == ['density', 'fid', 'n', 'precision', 'recall']
    assert {k: got[k] for k in ('precision', 'recall', 'density')} == F.precision_recall_from_features(gt, gen)


def test_with_both_options_off_the_scorer_is_the_parents(pairs):
    plain = _feed(_scorer(pairs, fid_batch=5), pairs['gen'], pairs['gt'])
    off = _feed(_scorer(pairs, fid_batch=5, kid=None, prc=False), pairs['gen'], pairs['gt'])
    assert off._bank_gen is None and off._bank_gt is None
    assert sorted(off.result()) == ['fid', 'n'] and off.result() == plain.result()


def test_result_leaves_the_banks_as_they_are_and_update_goes_on(pairs):
    s = _scorer(pairs, fid_batch=5, kid=KID, prc=PRC)
    _feed(s, pairs['gen'][:8], pairs['gt'][:8], (3, 5))
    part = s.result()
    assert part['n'] == 8 and s._bank_gen.n == 5 and part == s.result()
    _feed(s, pairs['gen'][8:], pairs['gt'][8:], (4,))
    fresh = _feed(_scorer(pairs, fid_batch=5, kid=KID, prc=PRC), pairs['gen'], pairs['gt'], (12,))
    assert s.result() == fresh.result()


def test_the_constructor_refuses_what_cannot_be_computed(pairs):
    mu, sigma = np.zeros(DIMS), np.eye(DIMS)
    for kw in (dict(kid=True), dict(prc=True)):
        with pytest.raises(ValueError):
            _scorer(pairs, fid_reference=(mu, sigma), **kw)
        with pytest.raises(ValueError):
            _scorer(pairs, fid=None, **kw)
    with pytest.raises(ValueError):
        _scorer(pairs, kid=3)


def test_the_path_functions_and_the_command_line(pairs, tmp_path):
    from hoig_amd.metrics.__main__ import main
    from hoig_amd.metrics.feature_metrics import calculate_kid_given_paths, calculate_prc_given_paths
    want = _want(pairs, 5)
    assert calculate_kid_given_paths(pairs['dirs'], 5, DEV, DIMS, weights=pairs['sd'], **KID) == (want['kid'], want['kid_std'])
    prc = calculate_prc_given_paths(pairs['dirs'], 5, DEV, DIMS, weights=pairs['sd'], **PRC)
    assert prc == {k: want[k] for k in ('precision', 'recall', 'density')}
    weights = str(tmp_path / 'inception.pth')
    torch.save(pairs['sd'], weights)
    common = pairs['dirs'] + ['--batch-size', '5', '--dims', str(DIMS), '--inception-weights', weights]
    kid_argv = ['kid'] + common + ['--kid-subsets', str(KID['subsets']), '--kid-subset-size', str(KID['subset_size']), '--kid-seed',
                                   str(KID['seed'])]
    prc_argv = ['prc'] + common + ['--prc-k', str(PRC['k'])]
    assert main(kid_argv) == (want['kid'], want['kid_std']) and main(prc_argv) == prc
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')

    def printed(argv, head):
        run = subprocess.run([sys.executable, '-m', 'hoig_amd.metrics'] + argv, env=env, cwd=ROOT, stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True, timeout=300)
        assert run.returncode == 0, run.stdout[-3000:]
        lines = [line for line in run.stdout.split('\n') if line.startswith(head)]
        assert len(lines) == 1
        return lines[0].split()

    words = printed(kid_argv, 'KID: ')
    assert len(words) == 3 and (float(words[1]), float(words[2])) == (want['kid'], want['kid_std'])
    words = printed(prc_argv, 'Precision: ')
    assert words[0::2] == ['Precision:', 'Recall:', 'Density:']
    assert [float(w) for w in words[1::2]] == [want['precision'], want['recall'], want['density']]
