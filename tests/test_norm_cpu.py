"""The bound of the instance-norm conditioning cases (tests/norm_reference.py: err <= max(8 * e_ref, 2e-6), e_ref = the error of
torch's own fp32 instance_norm on the same input) before a GPU is involved: fp32 emulations of the formulas the kernels use show
that a stable formula reaches the bound on EVERY conditioning input -- the two-pass one of the tile kernel, the pivot-shifted sums with
the median-of-means pivot of the streaming kernels, the plain sums with the centred recomputation of hoig_inorm_stats_from_sums --
and that the inputs tell the formulas apart: plain sums alone break it from |mean|/sigma = 10 up, and sums shifted by pixel 0 break it
when that pixel (or the corner block) has been moved."""
import pytest
import torch
import torch.nn.functional as F

import norm_reference as R

SIZES = [(32, 32), (64, 64), (256, 256)]


def _errors(x, emu):
    """per (image, channel): (error of the emulation's output, mean, rstd) and the same of torch's fp32 kernel, against float64."""
    ref = R.stats64(x)
    y64 = R.reference(x)['y']
    y32 = F.instance_norm(x.permute(0, 3, 1, 2).contiguous(), eps=R.EPS).permute(0, 2, 3, 1)
    m32, r32 = R.stats32_torch(x)
    y, mean, rstd = emu(x)
    got = (R.img_chan_err(y, y64), R.mean_err(mean, ref), R.rstd_err(rstd, ref))
    want = (R.img_chan_err(y32, y64), R.mean_err(m32, ref), R.rstd_err(r32, ref))
    return got, want


def _inside(got, want):
    """every (image, channel) inside the bound made from the TENSOR's e_ref (as the GPU test asserts it), and the worst err / bound"""
    worst = 0.0
    for g, w in zip(got, want):
        worst = max(worst, g.max().item() / R.bound(w.max().item()))
    return worst


@pytest.mark.parametrize('hw', SIZES)
def test_stable_formulas_stay_inside_the_bound_on_every_conditioning_input(hw):
    for name, x in R.conditioning_inputs(*hw).items():
        for label, emu in (('two-pass', R.emu_two_pass), ('median-of-means pivot', R.emu_pivot), ('sums + recomputation', R.emu_sums_repaired)):
            got, want = _errors(x, emu)
            worst = _inside(got, want)
            print('%-14s %3dx%-3d %-24s err/bound %.3f' % (name, hw[0], hw[1], label, worst))
            assert worst <= 1.0, (name, label, worst)
            assert all(torch.isfinite(g).all() for g in got)


@pytest.mark.parametrize('hw', SIZES[1:])
def test_plain_sums_break_the_bound_from_ratio_10_up(hw):
    cases = R.conditioning_inputs(*hw)
    for r in R.RATIOS:
        got, want = _errors(cases['ratio%g' % r], R.emu_plain)
        err, e_ref = got[0].max().item(), want[0].max().item()
        print('ratio %6g: plain sums %.2e, torch fp32 %.2e, bound %.2e' % (r, err, e_ref, R.bound(e_ref)))
        assert (err > R.bound(e_ref)) == (r >= 10), r           # (<= 3: what the kernel keeps the plain sums for)
        assert (err > R.TOL) == (r >= 100), r                   # the project's plain operator bound goes from 100 up


@pytest.mark.parametrize('hw', SIZES[1:])
def test_a_single_pixel_pivot_breaks_the_bound_when_that_pixel_is_moved(hw):
    cases = R.conditioning_inputs(*hw)
    for name in ('pixel0+100', 'pixel0+1000', 'corner3x3+100', 'corner3x3+1000', 'ratio10,pixel0+1000', 'ratio10,corner3x3-1000'):
        got, want = _errors(cases[name], lambda x: R.emu_pivot(x, 'pixel0'))
        worst = _inside(got, want)
        print('%-16s pixel-0 pivot: err/bound %.1f' % (name, worst))
        assert worst > 1.0, (name, worst)
    # the pivot the kernel uses now never reads pixel 0 of these maps, and one spoiled group of four cannot move a median of three
    for hw_ in (hw[0] * hw[1], 1024, 1025, 4, 15, 16, 1100):
        px = R.pivot_pixels(hw_)
        assert all(0 <= p < hw_ for g in px for p in g)
    assert 0 not in sum(R.pivot_pixels(hw[0] * hw[1]), [])


def test_the_median_pivot_survives_a_spoiled_group():
    """1000 sigma on any ONE of the twelve pivot pixels: still inside the bound."""
    base, _ = R.ratio_input(1, 64, 64, (0.0, 10.0, -30.0, 3.0), seed=5)
    ref_sigma = R.stats64(base)['sigma'].float()
    for group in R.pivot_pixels(64 * 64):
        x = base.clone()
        x.view(1, -1, 4)[:, group[1]] += 1000.0 * ref_sigma
        got, want = _errors(x, R.emu_pivot)
        assert _inside(got, want) <= 1.0


@pytest.mark.parametrize('kind,Ci,Co', [('s1', 32, 64), ('s2', 32, 64), ('convT', 64, 64), ('stem7', 3, 64), ('f6', 64, 64)])
def test_the_conditioned_convolutions_reach_their_ratio(kind, Ci, Co):
    """R.conv_problem (the from-sums cases build their inputs with it): in float64 the convolution's output has the wanted
    |mean| / sigma in every channel, within a factor two."""
    for ratio in R.RATIOS[1:]:
        x, w = R.conv_problem(kind, 1, Ci, Co, 32, 32, ratio, seed=3)
        h = R.conv_reference(kind, x, w).permute(0, 2, 3, 1)
        got = R.achieved_ratio(h)
        assert bool(((got > ratio / 2) & (got < ratio * 2)).all()), (kind, ratio, got.min().item(), got.max().item())
    far = conv_corner_displacement(kind, Ci, Co, 32, 32, 1000.0)
    assert far.median().item() > 10.0                           # pixel 0 of most channels sits many sigma from the channel


def conv_corner_displacement(kind, Ci, Co, Ho, Wo, moved):
    """|output pixel 0 - channel mean| in units of the sigma the channel has WITHOUT the move, per channel"""
    x0, w = R.conv_problem(kind, 1, Ci, Co, Ho, Wo, 0.0, seed=3)
    x1, _ = R.conv_problem(kind, 1, Ci, Co, Ho, Wo, 0.0, seed=3, moved=moved)
    s = R.stats64(R.conv_reference(kind, x0, w).permute(0, 2, 3, 1))
    h = R.conv_reference(kind, x1, w).permute(0, 2, 3, 1)
    return (h[0, 0, 0].double() - s['mean'][0]).abs() / s['sigma'][0]
