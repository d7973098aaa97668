"""The sliced Wasserstein distance on the MI355X (hoig_amd/csrc/swd.hip through hoig_amd/metrics/swd.py): every check of
tests/test_swd_cpu.py on the kernels, against the same truths with the same limits (tests/swd_reference.py); the kernels against
their CPU twins bit for bit; and Scorer(swd=), the directory function and the command line against swd_from_banks on the same
images."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_reference as MR
import swd_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
N, SIDE = 12, 64
CALLS = (5, 1, 6)
SWD = dict(patches=5, repeats=2, dirs=8, seed=3)


# ---------------------------------------------------------------------------------------------- the kernels against the truths
@pytest.mark.parametrize('case', R.PYRAMID_CASES, ids=lambda c: '%dx%d' % c[:2])
def test_pyramid_and_descriptors_against_scipy_and_the_twin(case):
    got, twin = R.check_descriptors(DEV, case), R.check_descriptors('cpu', case)
    for a, b in zip(got, twin):
        assert a.tobytes() == b.tobytes()


def test_descriptors_do_not_depend_on_the_split_of_the_stream():
    R.check_split(DEV)


@pytest.mark.parametrize('rows', R.STAT_ROWS)
def test_channel_statistics_against_longdouble_and_the_twin(rows):
    assert R.check_stats(DEV, rows).tobytes() == R.check_stats('cpu', rows).tobytes()


def test_a_constant_channel_is_a_status_and_a_value_error():
    R.check_degenerate(DEV)


@pytest.mark.parametrize('dirs', R.PROJ_DIRS)
@pytest.mark.parametrize('rows', R.PROJ_ROWS)
def test_projection_on_exact_integers_within_the_bound_and_against_the_twin(rows, dirs):
    R.check_project_exact(DEV, rows, dirs)
    assert R.check_project(DEV, rows, dirs).tobytes() == R.check_project('cpu', rows, dirs).tobytes()


@pytest.mark.parametrize('i', range(12))
def test_sort_equals_numpy_at_every_edge_size(i):
    n = R.sort_sizes()[i]
    for j, kind in enumerate(R.SORT_KINDS):
        R.check_sort(DEV, (1, 3)[(i + j) % 2], n, kind)


@pytest.mark.parametrize('case', R.SORT_LARGE, ids=lambda c: '%dx%d-%s' % c)
def test_sort_of_many_and_of_long_segments(case):
    R.check_sort(DEV, *case)


def test_sort_nan_is_a_status_and_unaligned_keys_are_sorted():
    from hoig_amd import _lib as L
    for n in (100, L.SORT_TILE + 904):
        R.check_sort_nan(DEV, n)
        R.check_sort_unaligned(DEV, n)


@pytest.mark.parametrize('N', R.L1_SIZES)
def test_sorted_l1_exact_on_integers_and_against_the_twin(N):
    R.check_l1_exact(DEV, N)
    assert R.check_l1(DEV, N).tobytes() == R.check_l1('cpu', N).tobytes()


def test_end_to_end_against_the_float64_reference_and_the_twin():
    assert R.check_end_to_end(DEV) == R.check_end_to_end('cpu')


def test_argument_errors():
    R.check_argument_errors(DEV)


# ---------------------------------------------------------------------------------------------- the scorer and the path function
@pytest.fixture(scope='module')
def pairs(tmp_path_factory):
    """12 pairs of PNGs at 64 x 64 (the recipe of tests/test_feature_metrics_gpu.py) and their bytes on the device."""
    from PIL import Image
    root = tmp_path_factory.mktemp('swd_pairs')
    a, b = str(root / 'gen'), str(root / 'gt')
    read = lambda names: torch.from_numpy(np.stack([np.asarray(Image.open(n).convert('RGB')) for n in names])).to(DEV)
    gen, gt = read(MR.write_pngs(a, N, SIDE, 30)), read(MR.write_pngs(b, N, SIDE, 31))
    return dict(dirs=[a, b], gen=gen, gt=gt)


def _want(p):
    from hoig_amd.metrics import swd as S
    banks = S.banks_for(S.swd_options(SWD), DEV)
    banks[0].append(p['gen'])
    banks[1].append(p['gt'])
    return S.swd_from_banks(banks[0], banks[1], SWD['repeats'], SWD['dirs'], SWD['seed'])


def _feed(s, gen, gt, calls=CALLS):
    at = 0
    for n in calls:
        s.update(gen[at:at + n], gt[at:at + n])
        at += n
    assert at == gen.shape[0]
    return s


def test_the_scorer_without_any_network_equals_the_bank_function(pairs):
    from hoig_amd.metrics.stream import Scorer
    want = _want(pairs)
    assert len(want['swd_levels']) == 3 and np.isfinite(want['swd_levels']).all() and want['swd'] > 0.0
    s = _feed(Scorer(fid=None, lpips=None, ssim=False, swd=SWD), pairs['gen'], pairs['gt'])
    got = s.result()
    assert sorted(got) == ['n', 'swd', 'swd_levels'] and got['n'] == N
    assert got['swd'] == want['swd'] and got['swd_levels'] == want['swd_levels']
    # result() leaves the state usable: the same again, and update() goes on
    assert s.result() == got
    part = _feed(Scorer(fid=None, lpips=None, ssim=False, swd=SWD), pairs['gen'][:8], pairs['gt'][:8], (3, 5))
    assert part.result()['n'] == 8 and part.result()['swd'] != got['swd']
    _feed(part, pairs['gen'][8:], pairs['gt'][8:], (4,))
    assert part.result() == got


def test_swd_beside_ssim_and_with_the_option_off_the_parents_keys(pairs):
    from hoig_amd.metrics.stream import Scorer
    plain = _feed(Scorer(fid=None, lpips=None, ssim=True), pairs['gen'], pairs['gt']).result()
    off = _feed(Scorer(fid=None, lpips=None, ssim=True, swd=None), pairs['gen'], pairs['gt'])
    assert off._swd_gen is None and sorted(off.result()) == ['ms_ssim', 'n', 'ssim'] and off.result() == plain
    assert _feed(Scorer(fid=None, lpips=None, ssim=True, swd=False), pairs['gen'], pairs['gt']).result() == plain
    both = _feed(Scorer(fid=None, lpips=None, ssim=True, swd=SWD), pairs['gen'], pairs['gt']).result()
    assert sorted(both) == ['ms_ssim', 'n', 'ssim', 'swd', 'swd_levels']
    assert both['ssim'] == plain['ssim'] and both['swd'] == _want(pairs)['swd']
    with pytest.raises(ValueError):
        Scorer(fid=None, lpips=None, ssim=False, swd=dict(subsets=3))


def test_the_path_function_and_the_command_line(pairs):
    from hoig_amd.metrics.__main__ import main
    from hoig_amd.metrics.swd import calculate_swd_given_paths
    want = _want(pairs)
    assert calculate_swd_given_paths(pairs['dirs'], 5, DEV, **SWD) == want
    assert calculate_swd_given_paths(pairs['dirs'], 50, DEV, device_png_decode=True, **SWD) == want
    argv = ['swd'] + pairs['dirs'] + ['--batch-size', '5', '--swd-patches', str(SWD['patches']), '--swd-repeats', str(SWD['repeats']),
                                      '--swd-dirs', str(SWD['dirs']), '--swd-seed', str(SWD['seed'])]
    assert main(argv) == want
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    run = subprocess.run([sys.executable, '-m', 'hoig_amd.metrics'] + argv, env=env, cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:]
    lines = [line for line in run.stdout.split('\n') if line.startswith('SWD: ')]
    assert len(lines) == 1
    words = lines[0].split()
    assert [float(w) for w in words[1:]] == [want['swd']] + want['swd_levels']
