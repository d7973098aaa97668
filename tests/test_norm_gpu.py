"""Instance-norm kernels (hoig_amd/csrc/norm.hip) per path, driven through the C ABI so that the path is chosen and not guessed:

  tile    hoig_inorm_fwd_fused / hoig_inorm_bwd_fused(_add)(_split)           one launch, maps of <= 1024 pixels, C % 32 == 0
  stream  hoig_inorm_stats + hoig_inorm_apply(_ld) / hoig_inorm_bwd(_ld)(_add_ld)(_split)
  sums    hoig_inorm_stats_from_sums over the sums a real producer left (hoig_conv2d_fwd_packed_stats: 3x3 stride 1, stride 2,
          ConvTranspose; hoig_conv2d_fwd_stats: the 7x7 stem; hoig_conv2d_fwd_f6_ex) + the streaming apply / backward

against torch.nn.functional.instance_norm + autograd in float64 on the CPU (tests/norm_reference.py).  Well-conditioned input: the
suite's bound TOL = 1e-4 (5 * TOL for gradients), max-norm relative over the tensor AND per channel.  Conditioning cases: the bound
is made from the error of torch's own fp32 kernel on the same input (norm_reference.bound).  After every call the first 2^18 floats
of the workspace are zero again.  A thinner layer of cases goes through hoig_amd.ops to hold the dispatch of hoig_amd/ops_norm.py.

Measured on an MI355X (err / e_ref per conditioning case): docs/norm_conditioning.md.  The file adds about 20 s to `-m gpu`."""
import ctypes

import pytest
import torch

import norm_reference as R

pytestmark = pytest.mark.gpu

POOL = 1 << 18
TOL = R.TOL
SENT = -7.25                      # what output buffers hold before a call: a refused call must leave it there
NONE, RELU, LRELU = R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU
SLOPE = 0.2


def _L():
    from hoig_amd import _lib as L
    return L


def _p(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off)


def _st():
    return torch.cuda.current_stream().cuda_stream


_WS = []


def workspace():
    """ONE zero-initialised workspace for the whole file: every call finds what the call before it left (include/hoig_kernels.h: the
    accumulators are zero on entry and zero on return), whatever the order of the cases."""
    if not _WS:
        _WS.append(torch.zeros(2 * POOL + 64, dtype=torch.float32, device='cuda'))
    return _WS[0]


@pytest.fixture(autouse=True)
def _leave_the_workspace_usable():
    """a test that failed between a producer and its consumer must not make every later test fail too (the checks of the contract are
    the assert_clean calls after every kernel call, not this)"""
    yield
    if _WS:
        torch.cuda.synchronize()
        _WS[0].zero_()


def assert_clean(what=''):
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(workspace()[:POOL])) == 0, 'accumulators left dirty ' + what


def new_out(*shape, dtype=torch.float32):
    return torch.full(shape, SENT, dtype=dtype, device='cuda')


# ------------------------------------------------------------------------------------------------------------------ drivers
class Params:
    """the p0 / p1 operands of a mode: device pointers for the kernels, CPU tensors for the reference"""

    def __init__(self, mode, ld2c, shape, g, zero_bias=False):
        B, H, W, C = shape
        self.mode, self.ld, self.ld2c = mode, C, ld2c
        self.p0 = self.p1 = self.c0 = self.c1 = self.keep = None
        if mode == 1:
            self.c0 = torch.randn(C, generator=g) * 0.5 + 1.0
            self.c1 = torch.zeros(C) if zero_bias else torch.randn(C, generator=g) * 0.5
            self.keep = (self.c0.cuda(), self.c1.cuda())
            self.p0, self.p1 = _p(self.keep[0]), _p(self.keep[1])
        elif mode == 2 and ld2c:                 # gamma | beta side by side in ONE [., 2C] tensor
            gb = torch.randn(B, H, W, 2 * C, generator=g) * 0.3
            self.c0, self.c1 = gb[..., :C].contiguous(), gb[..., C:].contiguous()
            self.keep = (gb.cuda(),)
            self.p0, self.p1, self.ld = _p(self.keep[0]), _p(self.keep[0], 4 * C), 2 * C
        elif mode == 2:
            self.c0, self.c1 = torch.randn(B, H, W, C, generator=g) * 0.3, torch.randn(B, H, W, C, generator=g) * 0.3
            self.keep = (self.c0.cuda(), self.c1.cuda())
            self.p0, self.p1 = _p(self.keep[0]), _p(self.keep[1])


def forward(path, xd, P, act=NONE, slope=0.0, residual=None):
    """-> rc, y, mean, rstd.  path 'sums': the accumulators hold the sums of xd (conv_with_sums)."""
    L = _L()
    B, H, W, C = xd.shape
    HW = H * W
    y, mean, rstd = new_out(*xd.shape), new_out(B * C), new_out(B * C)
    if path == 'tile':
        rc = L.lib.hoig_inorm_fwd_fused(_p(xd), P.mode, P.p0, P.p1, P.ld, act, slope, _p(residual), R.EPS, _p(y), _p(mean), _p(rstd), B, HW, C, _st())
        return rc, y, mean, rstd
    if path == 'stream':
        rc = L.lib.hoig_inorm_stats(_p(xd), B, HW, C, R.EPS, _p(mean), _p(rstd), _p(workspace()), _st())
    else:
        rc = L.lib.hoig_inorm_stats_from_sums(_p(xd), B, HW, C, R.EPS, _p(mean), _p(rstd), _p(workspace()), _st())
    if rc != 0:
        return rc, y, mean, rstd
    if P.ld == C and (B + H) % 2:               # (both spellings of the apply entry point get their share of the cases)
        rc = L.lib.hoig_inorm_apply(_p(xd), _p(mean), _p(rstd), P.mode, P.p0, P.p1, act, slope, _p(residual), _p(y), B, HW, C, _st())
    else:
        rc = L.lib.hoig_inorm_apply_ld(_p(xd), _p(mean), _p(rstd), P.mode, P.p0, P.p1, P.ld, act, slope, _p(residual), _p(y), B, HW, C, _st())
    return rc, y, mean, rstd


def backward(path, form, xd, mean, rstd, P, y, dy, act=NONE, slope=0.0, addend=None):
    """form 'plain' | 'add' | 'split' (split: dx comes back as bf16 planes [B, H, W, 2, C]; takes the addend when one is given).
    -> rc, dx, dp0, dp1 (affine: [C] accumulators that started at zero; SPADE: NHWC)."""
    L = _L()
    B, H, W, C = xd.shape
    HW = H * W
    dx = new_out(B, H, W, 2, C, dtype=torch.bfloat16) if form == 'split' else new_out(*xd.shape)
    d0 = d1 = q0 = q1 = None
    if P.mode == 1:
        d0, d1 = torch.zeros(C, device='cuda'), torch.zeros(C, device='cuda')
        q0, q1 = _p(d0), _p(d1)
    elif P.mode == 2 and P.ld2c:
        dgb = new_out(B, H, W, 2 * C)
        d0, d1 = dgb[..., :C], dgb[..., C:]
        q0, q1 = _p(dgb), _p(dgb, 4 * C)
    elif P.mode == 2:
        d0, d1 = new_out(*xd.shape), new_out(*xd.shape)
        q0, q1 = _p(d0), _p(d1)
    head = (_p(xd), _p(mean), _p(rstd), P.mode, P.p0, P.p1, P.ld, _p(y), _p(dy), act, slope)
    tail = (q0, q1, B, HW, C)
    if path == 'tile':
        if form == 'plain':
            rc = L.lib.hoig_inorm_bwd_fused(*head, _p(dx), *tail, _st())
        elif form == 'add':
            rc = L.lib.hoig_inorm_bwd_fused_add(*head, _p(addend), _p(dx), *tail, _st())
        else:
            rc = L.lib.hoig_inorm_bwd_fused_add_split(*head, _p(addend), _p(dx), *tail, _st())
    else:
        ws = _p(workspace())
        if form == 'plain' and P.ld == C and (B + H) % 2:
            rc = L.lib.hoig_inorm_bwd(_p(xd), _p(mean), _p(rstd), P.mode, P.p0, P.p1, _p(y), _p(dy), act, slope, _p(dx), *tail, ws, _st())
        elif form == 'plain':
            rc = L.lib.hoig_inorm_bwd_ld(*head, _p(dx), *tail, ws, _st())
        elif form == 'add':
            rc = L.lib.hoig_inorm_bwd_add_ld(*head, _p(addend), _p(dx), *tail, ws, _st())
        else:
            rc = L.lib.hoig_inorm_bwd_add_ld_split(*head, _p(addend), _p(dx), *tail, ws, _st())
    return rc, dx, d0, d1


def well_conditioned(shape, seed):
    """channels of different magnitudes (1e-2 .. 1e2) and offsets (|mean| / sigma <= 1.5)"""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    scale = torch.logspace(-2, 2, C)[torch.randperm(C, generator=g)]
    off = torch.rand(C, generator=g) * 3.0 - 1.5
    return (torch.randn(B, H, W, C, generator=g) + off) * scale, g


def affine_scale(x, dy, y_gpu, P, act, slope):
    """sum |terms| of dbias and dweight per channel in float64: the scale an error of those SUMS is measured against"""
    s = R.stats64(x)
    xh = (x.double() - s['mean'][:, None, None, :]) * s['rstd'][:, None, None, :]
    g = dy.double()
    if act != NONE:
        yy = y_gpu.double().cpu()
        g = g * torch.where(yy > 0, torch.ones_like(yy), torch.full_like(yy, slope if act == LRELU else 0.0))
    C = x.shape[-1]
    return (g * xh).abs().reshape(-1, C).sum(0), g.abs().reshape(-1, C).sum(0)


def order_bound(x, dy, y_gpu, P, act, slope):
    """The streaming backward sums g' and g' * xhat over a map's chunks with fp32 atomics, so two launches on the SAME arguments differ
    in the last bits of the two sums whenever a map has more than one chunk.  -> per element, the most that can move dx: both sums
    off by 1024 * 2^-24 of their sum of absolute terms (128 chunks, LDS partials, lanes).  A flipped activation mask moves its element by
    rstd * |scale * dy| * (1 - slope): with |dy| >= half the channel's magnitude that is four orders of magnitude above this bound."""
    s = R.stats64(x)
    sw, sb = affine_scale(x, dy, y_gpu, P, act, slope)              # per channel over the batch: an upper bound of each image's
    n = x.shape[1] * x.shape[2]
    xh = ((x.double() - s['mean'][:, None, None, :]) * s['rstd'][:, None, None, :]).abs()
    sc = P.c0.double().abs() if P.mode == 1 else 2.5 if P.mode == 2 else 1.0          # (SPADE: |1 + gamma| < 2.5 for gamma ~ 0.3 N(0, 1))
    return (s['rstd'][:, None, None, :] * sc * (sb + xh * sw) / n * (1024 * 2.0 ** -24)).float().cuda()


def check_split(dx_planes, dx_fp32, slack=None):
    """the planes are hoig_split_planes_bf16 of the fp32 form's dx bit for bit, and un-split they give it back to bf16x2 precision.
    slack (see order_bound): the two come from two launches of the streaming backward, which agree to the order of their atomics only --
    the planes then have to un-split to within bf16x2 precision of a value that close (the split itself is the one function store_split
    of both backward kernels, held bit for bit by the tile cases)."""
    L = _L()
    C = dx_fp32.shape[-1]
    npix = dx_fp32.numel() // C
    want = torch.empty_like(dx_planes)
    L.call('hoig_split_planes_bf16', _p(dx_fp32), _p(want), npix, C, _st())
    back = torch.empty_like(dx_fp32)
    L.call('hoig_unsplit_planes_bf16', _p(dx_planes), _p(back), npix, C, _st())
    torch.cuda.synchronize()
    if slack is None:
        assert torch.equal(dx_planes.view(torch.int16), want.view(torch.int16))
        slack = 1e-37
    assert bool(((back - dx_fp32).abs() <= dx_fp32.abs() * 2.0 ** -15 + slack).all())


def check_case(path, shape, mode, ld2c, act, with_res, seed, forms=('plain', 'add', 'split'), x=None, sums_ready=False, cond=None):
    """forward + every backward form of one configuration against float64.  cond: None -> the TOL bounds; a label -> the bound made from
    torch's fp32 error on the same input, and a printed line per quantity.  -> dict of err / bound per quantity."""
    slope = SLOPE if act == LRELU else 0.0
    if x is None:
        x, g = well_conditioned(shape, seed)
    else:
        g = torch.Generator().manual_seed(seed)
    shape = tuple(x.shape)
    B, H, W, C = shape
    xd = x if x.is_cuda else x.cuda()
    x = x.cpu()
    P = Params(mode, ld2c, shape, g)
    chan = torch.logspace(-1, 1, C)[torch.randperm(C, generator=g)]
    res = torch.randn(shape, generator=g) * chan if with_res else None
    resd = res.cuda() if with_res else None
    rc, y, mean, rstd = forward('sums' if sums_ready else path, xd, P, act, slope, resd)
    assert rc == 0, rc
    assert_clean('after the forward')
    ref = R.reference(x, mode, P.c0, P.c1, act, slope, res)
    st64 = R.stats64(x)
    out, fails = {}, []

    def judge(name, got_err, ref_err=None, grad=False):
        """got_err: [.., C]-shaped per-(image, channel) errors or a float"""
        e = float(got_err.max()) if torch.is_tensor(got_err) else got_err
        if cond is None:
            lim = 5 * TOL if grad else TOL
        else:
            lim = R.bound(float(ref_err.max()) if torch.is_tensor(ref_err) else ref_err)
        out[name] = '%.2g' % (e / lim) if cond is None else '%.2g/%.2g' % (e, float(ref_err.max()) if torch.is_tensor(ref_err) else ref_err)
        if not e <= lim:                         # (reported together below, after the line of figures is printed)
            fails.append('%s %s %r mode %d act %d: %s error %.3g > %.3g' % (path, cond or '', shape, mode, act, name, e, lim))

    if cond is None:
        judge('y', R.rel_err(y, ref['y']))
        judge('y/chan', R.chan_err(y, ref['y']))
        judge('mean', R.mean_err(mean, st64))
        judge('rstd', R.rstd_err(rstd, st64))
    else:
        ref32 = R.reference(x, mode, P.c0, P.c1, act, slope, res, dtype=torch.float32)
        m32, r32 = R.stats32_torch(x)
        pre = ref['y'] if act == NONE else R.reference(x, mode, P.c0, P.c1, NONE, 0.0, res)['y']      # (see R.img_chan_err)
        judge('y', R.img_chan_err(y, ref['y'], pre), R.img_chan_err(ref32['y'], ref['y'], pre))
        judge('mean', R.mean_err(mean, st64), R.mean_err(m32, st64))
        judge('rstd', R.rstd_err(rstd, st64), R.rstd_err(r32, st64))
    assert bool(torch.isfinite(y).all() and torch.isfinite(mean).all() and torch.isfinite(rstd).all())

    # ---- backward: dy and the addend with channels of different magnitudes
    dy = torch.randn(shape, generator=g)
    dy = (dy + 0.5 * torch.sign(dy)) * chan.flip(0)            # |dy| >= half the channel's magnitude (order_bound)
    add = torch.randn(shape, generator=g) * chan.flip(0) * 0.5
    dyd, addd = dy.cuda(), add.cuda()
    y_act = None
    if act != NONE:
        y_act = y if not with_res else None
        assert not with_res
    refb = R.reference(x, mode, P.c0, P.c1, act, slope, None, dy=dy, mask_from=y_act)
    refb32 = R.reference(x, mode, P.c0, P.c1, act, slope, None, dy=dy, mask_from=y_act, dtype=torch.float32) if cond else None
    y_null_ok = act in (RELU, LRELU) and mode in (0, 1)
    bpath = 'stream' if path == 'sums' else path
    one_launch_order = bpath == 'tile' or H * W <= 16            # deterministic sums: results are reproducible bit for bit
    slack = None if one_launch_order else order_bound(x, dy, y_act, P, act, slope)
    got = {}
    for form in forms:
        for y_passed in ((True, False) if y_null_ok else (True,)):
            rc, dx, d0, d1 = backward(bpath, form, xd, mean, rstd, P, y_act if y_passed else None, dyd, act, slope,
                                      addd if form == 'add' or (form == 'split' and seed % 2) else None)
            assert rc == 0, (form, rc)
            assert_clean('after the %s backward' % form)
            got[(form, y_passed)] = (dx, d0, d1)
        if y_null_ok:                            # the mask recomputed from x is the mask of y: identical results, not close ones
            a, b = got[(form, True)], got[(form, False)]
            if one_launch_order:
                assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)), 'dx with y and with y = NULL differ (%s, %s)' % (path, form)
            else:
                fa, fb = (t[0] if form != 'split' else t[0][..., 0, :].float() + t[0][..., 1, :].float() for t in (a, b))
                room = slack + fa.abs() * (2.0 ** -14 if form == 'split' else 2.0 ** -22)      # (+ the rounding of the result itself: bf16x2 planes; dx + addend)
                assert bool(((fa - fb).abs() <= room).all()), 'dx with y and with y = NULL differ beyond the order of the atomics (%s, %s)' % (path, form)
            if mode == 1:
                sw, sb = affine_scale(x, dy, y_act, P, act, slope)                            # (atomics: order only, see order_bound)
                assert bool(((a[1] - b[1]).abs().cpu() <= 1024 * 2.0 ** -24 * sw).all() and ((a[2] - b[2]).abs().cpu() <= 1024 * 2.0 ** -24 * sb).all())
    for form in forms:
        dx, d0, d1 = got[(form, True)]
        has_add = form == 'add' or (form == 'split' and seed % 2)
        want = refb['dx'] + (add.double() if has_add else 0.0)
        if form == 'split':
            if ('add', True) in got and has_add:
                check_split(dx, got[('add', True)][0], slack)
            elif ('plain', True) in got and not has_add:
                check_split(dx, got[('plain', True)][0], slack)
            dxf = dx[..., 0, :].float() + dx[..., 1, :].float()
            assert R.rel_err(dxf, want) <= 5 * TOL
            continue
        if cond is None:
            judge('dx:' + form, R.rel_err(dx, want), grad=True)
            judge('dx/chan:' + form, R.chan_err(dx, want), grad=True)
        else:
            want32 = refb32['dx'].double() + (add.double() if has_add else 0.0)
            judge('dx:' + form, R.img_chan_err(dx, want), R.img_chan_err(want32, want))
        if mode == 2:
            for nm, d, k in (('dgamma', d0, 'dp0'), ('dbeta', d1, 'dp1')):
                if cond is None:
                    judge(nm, R.rel_err(d, refb[k]), grad=True)
                    judge(nm + '/chan', R.chan_err(d, refb[k]), grad=True)
                else:
                    judge(nm, R.img_chan_err(d, refb[k]), R.img_chan_err(refb32[k], refb[k]))
        elif mode == 1:
            sw, sb = affine_scale(x, dy, y_act, P, act, slope)
            for nm, d, k, sc in (('dweight', d0, 'dp0', sw), ('dbias', d1, 'dp1', sb)):
                e = (d.double().cpu() - refb[k]).abs() / sc.clamp_min(1e-30)
                if cond is None:
                    judge(nm, R.rel_err(d, refb[k]), grad=True)
                    judge(nm + '/chan', e, grad=True)
                else:
                    judge(nm, e, (refb32[k].double() - refb[k]).abs() / sc.clamp_min(1e-30))
    if cond is not None:
        print('COND %-6s %-26s %6d px mode %d%s act %d | ' % (path, cond, H * W, mode, 'L' if ld2c else ' ', act) +
              ' '.join('%s %s' % kv for kv in out.items()))
    assert not fails, '; '.join(fails)
    return out


# (mode, gamma|beta in one [., 2C] tensor, activation, residual)
CONFIGS = [(0, False, NONE, False), (0, False, RELU, False), (0, False, LRELU, False), (0, False, NONE, True),
           (1, False, NONE, False), (1, False, RELU, False), (1, False, LRELU, False), (1, False, NONE, True),
           (2, False, NONE, False), (2, False, RELU, False), (2, False, LRELU, False),
           (2, True, NONE, False), (2, True, RELU, False), (2, True, LRELU, False)]


# ---------------------------------------------------------------------------------------------------- modes x epilogues x forms
@pytest.mark.parametrize('path,shape', [('tile', (2, 25, 40, 32)), ('tile', (1, 32, 32, 64)), ('stream', (2, 33, 37, 8)), ('stream', (1, 25, 41, 32))])
@pytest.mark.parametrize('mode,ld2c,act,with_res', CONFIGS)
def test_every_mode_epilogue_and_backward_form(path, shape, mode, ld2c, act, with_res):
    check_case(path, shape, mode, ld2c, act, with_res, seed=sum(shape) + 7 * mode + act)


TILE_SHAPES = [(1, 32, 32, 32), (3, 32, 32, 64), (1, 2, 2, 32), (1, 3, 5, 64), (1, 4, 4, 32), (16, 8, 8, 32), (1, 4, 4, 512), (1, 2, 2, 1024),
               (1, 2, 2, 2048), (2, 31, 33, 32)]
STREAM_SHAPES = [(1, 32, 32, 32), (1, 25, 41, 32), (2, 33, 37, 8), (1, 1, 1100, 16), (3, 17, 61, 4), (1, 129, 129, 8), (1, 2, 2, 4), (1, 3, 5, 8),
                 (1, 4, 4, 16), (1, 256, 256, 64), (1, 5, 7, 64), (1, 5, 7, 512), (1, 5, 7, 1024), (1, 5, 7, 1536), (1, 5, 7, 2048), (16, 6, 6, 32),
                 (3, 40, 40, 16)]


@pytest.mark.parametrize('path,shape', [('tile', s) for s in TILE_SHAPES] + [('stream', s) for s in STREAM_SHAPES])
def test_shapes(path, shape):
    """the 1024 / 1025-pixel switch from both sides, short and empty last chunks, more than 128 chunks' worth, 1 .. 16 pixels, the
    stem's map, every channel width class of the streaming kernels (CV < NT, == NT, > NT with and without a short last round)"""
    i = (TILE_SHAPES if path == 'tile' else STREAM_SHAPES).index(shape)
    for j in (i, i + 5, i + 9)[:1 if shape[1] * shape[2] * shape[3] > 1 << 20 else 3]:
        mode, ld2c, act, with_res = CONFIGS[j % len(CONFIGS)]
        check_case(path, shape, mode, ld2c, act, with_res, seed=100 + j)


def test_accumulator_pool_edges_and_the_sequence_large_small_large():
    """B * 2 * C just below the 2^18 accumulators, exactly at them, then a small call, then large again (the backward's sums live
    outside the pool, so a later, larger call never finds them inside its accumulators); above the pool the call is refused"""
    L = _L()
    for k, shape in enumerate([(63, 2, 2, 2048), (1, 3, 5, 8), (64, 2, 2, 2048), (2, 33, 37, 8), (64, 2, 3, 2048)]):
        mode, ld2c, act, with_res = CONFIGS[(4 + 3 * k) % len(CONFIGS)]
        check_case('stream', shape, mode, ld2c, act, with_res, seed=200 + k, forms=('plain', 'add'))
    B, H, W, C = 65, 1, 2, 2048
    xd = torch.randn(B, H, W, C, device='cuda')
    P = Params(0, False, (B, H, W, C), torch.Generator().manual_seed(0))
    rc, y, mean, rstd = forward('stream', xd, P)
    assert rc == L.EUNSUPPORTED and bool((mean == SENT).all() and (rstd == SENT).all() and (y == SENT).all())
    rc, dx, _, _ = backward('stream', 'plain', xd, mean, rstd, P, None, xd)
    assert rc == L.EUNSUPPORTED and bool((dx == SENT).all())
    assert_clean('after refused calls')
    rc, y, mean, rstd = forward('tile', xd, P)                   # (the one-launch kernel has no accumulators: it takes the shape)
    assert rc == 0 and R.rel_err(y, R.reference(xd.cpu())['y']) < TOL


@pytest.mark.parametrize('C', [36, 96, 160, 6])
def test_refused_widths_come_back_as_unsupported_and_touch_nothing(C):
    """widths the kernels have no tiling for: HOIG_EUNSUPPORTED from the C ABI, a Python exception naming the operator from ops; outputs
    untouched, accumulators still zero -- not a silent wrong answer"""
    L = _L()
    from hoig_amd import ops
    for shape in ((2, 8, 8, C), (1, 40, 40, C)):
        xd = torch.randn(*shape, device='cuda')
        P = Params(0, False, shape, torch.Generator().manual_seed(0))
        tile_takes_it = C % 32 == 0 and shape[1] * shape[2] <= 1024          # (96 and 160 are widths of the one-launch kernel)
        for path in ('stream',) if tile_takes_it else ('tile', 'stream'):
            rc, y, mean, rstd = forward(path, xd, P)
            assert rc == L.EUNSUPPORTED, (path, rc)
            assert bool((y == SENT).all() and (mean == SENT).all() and (rstd == SENT).all())
            for form in ('plain', 'add', 'split'):
                if C % 4 and form == 'split':
                    continue
                rc, dx, _, _ = backward(path, form, xd, mean, rstd, P, None, xd, addend=xd if form == 'add' else None)
                assert rc == L.EUNSUPPORTED, (path, form, rc)
                assert bool((dx.float() == SENT).all())
        assert_clean('after refused calls')
        gb = torch.randn(shape[0], shape[1], shape[2], 2 * C, device='cuda')
        if tile_takes_it:
            assert R.rel_err(ops.instance_norm(xd), R.reference(xd.cpu())['y']) < TOL
        else:
            with pytest.raises(L.HoigKernelError, match='hoig_inorm'):
                ops.instance_norm(xd)
            with pytest.raises(L.HoigKernelError, match='hoig_inorm'):
                ops.spade_norm_fused(xd, gb)
        torch.cuda.synchronize()
        for ws in ops._norm_ws.values():
            assert int(torch.count_nonzero(ws[:POOL])) == 0
    big = torch.randn(8193, 1, 1, 16, device='cuda')              # B * 2 * C above the accumulator pool, streaming width
    with pytest.raises(L.HoigKernelError, match='hoig_inorm'):
        ops.instance_norm(big)


def test_fold_is_the_norm_as_one_fma():
    """hoig_inorm_fold: scale = rstd * gamma, shift = beta - mean * scale, rows ld_out apart (nullable gamma / beta = 1 / 0); what lies
    between the rows stays untouched"""
    L = _L()
    B, C, ld = 3, 40, 56
    g = torch.Generator().manual_seed(4)
    mean, rstd = torch.randn(B * C, generator=g).cuda() * 30, (torch.rand(B * C, generator=g) * 300 + 0.01).cuda()
    gamma, beta = torch.randn(C, generator=g).cuda(), torch.randn(C, generator=g).cuda()
    for ga, be in ((gamma, beta), (None, None), (gamma, None)):
        scale, shift = new_out(B, ld), new_out(B, ld)
        L.call('hoig_inorm_fold', _p(mean), _p(rstd), _p(ga), _p(be), B, C, _p(scale), _p(shift), ld, _st())
        torch.cuda.synchronize()
        sc = rstd.double().view(B, C) * (ga.double() if ga is not None else 1.0)
        sh = (be.double() if be is not None else 0.0) - mean.double().view(B, C) * sc
        assert R.rel_err(scale[:, :C], sc) < 1e-6 and ((shift[:, :C].double() - sh).abs() <= 1e-6 * (sh.abs() + (mean.double().view(B, C) * sc).abs())).all()
        assert bool((scale[:, C:] == SENT).all() and (shift[:, C:] == SENT).all())
    assert L.lib.hoig_inorm_fold(_p(mean), _p(rstd), None, None, B, C, _p(scale), _p(shift), C - 4, _st()) == L.EINVAL


# ------------------------------------------------------------------------------------------------------------------ exact checks
@pytest.mark.parametrize('path,shape', [('tile', (3, 32, 32, 32)), ('tile', (2, 25, 40, 64)), ('stream', (3, 32, 32, 32)), ('stream', (2, 33, 37, 16)),
                                        ('stream', (1, 128, 128, 8))])
def test_dbias_of_relu_with_unit_dy_is_the_count_of_positive_outputs_exactly(path, shape):
    """affine mode, bias 0, dy = 1, ReLU: dbias[c] = count(y > 0) over the batch, an integer below 2^24, exact in fp32 in any order of
    summation -- with y passed and with the mask recomputed from x.  The input is symmetric about zero and one value in five IS zero,
    so a fifth of the pre-activations sit within a rounding of zero: a mask that is not bit for bit the forward's shows up here."""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(B * H + C)
    half = torch.randint(-2, 3, (B, (H * W + 1) // 2, C), generator=g).float()
    x = torch.cat([half, -half], 1)[:, :H * W].reshape(B, H, W, C) * torch.logspace(-1, 1, C)
    xd = x.cuda()
    P = Params(1, False, shape, g, zero_bias=True)
    rc, y, mean, rstd = forward(path, xd, P, RELU)
    assert rc == 0
    count = (y > 0).sum(dim=(0, 1, 2)).float()
    assert 0 < int(count.min()) and int(count.max()) < B * H * W
    dy = torch.ones_like(xd)
    for y_arg in (y, None):
        for form in ('plain', 'add'):
            rc, dx, dw, db = backward(path, form, xd, mean, rstd, P, y_arg, dy, RELU, addend=xd if form == 'add' else None)
            assert rc == 0
            assert_clean()
            assert torch.equal(db, count), (path, form, y_arg is None, (db - count).abs().max().item())


@pytest.mark.parametrize('path', ['tile', 'stream', 'sums'])
def test_constant_channels(path):
    """sigma = 0: finite mean, rstd and outputs on every path, the outputs inside the conditioning bound taken absolutely; on the tile
    path the variance is centred, hence exactly 0, and rstd = 1 / sqrt(eps) to 1 ulp"""
    B, H, W, C = 2, 32, 32, 64
    if path == 'sums':
        xn, w = R.conv_problem('s1', 3, 32, 256, 64, 64, 0.0, seed=1, sigma_x=0.0, delta=0.01)
        xd = conv_with_sums('s1', xn, w)
    else:
        level = torch.tensor([3.0, -0.5, 0.0, 2.0, 1024.0, -7.0, 0.25, 100.0]).repeat(C // 8)
        xd = level.expand(B, H, W, C).contiguous().cuda()
    P = Params(0, False, tuple(xd.shape), torch.Generator().manual_seed(0))
    rc, y, mean, rstd = forward(path, xd, P)
    assert rc == 0
    assert_clean()
    assert bool(torch.isfinite(y).all() and torch.isfinite(mean).all() and torch.isfinite(rstd).all())
    x = xd.cpu()
    ref, ref32 = R.reference(x)['y'], R.reference(x, dtype=torch.float32)['y']
    e_ref = (ref32.double() - ref).abs().max().item()
    assert (y.double().cpu() - ref).abs().max().item() <= R.bound(e_ref)
    if path == 'tile':
        r0 = 1.0 / float(torch.tensor(R.EPS, dtype=torch.float32).double().sqrt())
        assert (rstd.double().cpu() - r0).abs().max().item() <= 2.0 ** -15          # 1 ulp of fp32 at 316.2
        assert torch.equal(mean.cpu().reshape(B, C), x[:, 0, 0, :])
        assert float(y.abs().max()) == 0.0
    dy = torch.randn_like(xd)
    rc, dx, _, _ = backward('stream' if path == 'sums' else path, 'plain', xd, mean, rstd, P, None, dy)
    assert rc == 0 and bool(torch.isfinite(dx).all())
    assert_clean()


# ----------------------------------------------------------------------------------------------- from-sums: the real producers
def conv_with_sums(kind, x_nchw, w):
    """the convolution `kind` of R.CONV_KINDS through the entry point that ALSO leaves the per-image channel sums of its output in
    workspace() -> the output (NHWC, on the GPU)"""
    L = _L()
    from hoig_amd import ops
    k, stride, transposed = R.CONV_KINDS[kind]
    xd = x_nchw.permute(0, 2, 3, 1).contiguous().cuda()
    B, Hi, Wi, Ci = xd.shape
    Co = w.shape[1] if transposed else w.shape[0]
    Ho, Wo = (Hi * 2, Wi * 2) if transposed else (Hi // stride, Wi // stride)
    wd = ops.pack_weight(w.cuda(), transposed=transposed)
    h = new_out(B, Ho, Wo, Co)
    ws = workspace()
    prec = L.PREC_F16F6 if kind == 'f6' else L.PREC_BF16X3
    d = L.ConvDesc(B, Hi, Wi, Ci, Ho, Wo, Co, k, k, stride, k // 2, 1 if transposed else 0, L.ACT_NONE, 0.0, prec)
    if kind == 'stem7':
        rc = L.lib.hoig_conv2d_fwd_stats(ctypes.byref(d), _p(xd), _p(wd), None, _p(h), _p(ws), _st())
    elif kind == 'f6':
        old = ops.set_f6_min_tiles(1)
        try:
            hi, _ = ops._packed_planes(wd, False, False)
            qh, ql = ops._f6_planes(wd)
            rc = L.lib.hoig_conv2d_fwd_f6_ex(ctypes.byref(d), _p(xd), 0, None, _p(hi), _p(qh), _p(ql), None, None, None, 0, _p(h), _p(ws), _st())
        finally:
            ops.set_f6_min_tiles(old)
    else:
        hi, lo = ops._packed_planes(wd, transposed, False)
        rc = L.lib.hoig_conv2d_fwd_packed_stats(ctypes.byref(d), _p(xd), _p(hi), _p(lo), None, _p(h), _p(ws), _st())
    assert rc == 0, 'the %s producer refused the layer (%d): the case would not test the hand-off' % (kind, rc)
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(ws[:B * 2 * Co])) > 0             # the sums are there
    return h


# kind -> (B, Ci, Co) at 64 x 64 outputs and at 256 x 256 outputs (enough tiles for the producer's kernel at either size)
SUMS_LAYERS = {'s1': ((3, 32, 256), (1, 32, 64)), 's2': ((2, 32, 128), (1, 32, 64)), 'convT': ((2, 64, 128), (1, 64, 64)),
               'stem7': ((2, 3, 64), (1, 3, 64)), 'f6': ((3, 64, 256), (1, 64, 64))}


@pytest.mark.parametrize('kind', list(SUMS_LAYERS))
@pytest.mark.parametrize('mode,ld2c,act,with_res', [CONFIGS[0], CONFIGS[5], CONFIGS[7], CONFIGS[10], CONFIGS[11]])
def test_from_sums_on_well_conditioned_layers(kind, mode, ld2c, act, with_res):
    """conv -> norm with the statistics taken from the convolution's epilogue, against the float64 norm of the convolution's OWN fp32
    output (so the convolution's arithmetic cancels out)"""
    B, Ci, Co = SUMS_LAYERS[kind][0]
    g = torch.Generator().manual_seed(len(kind) + mode)
    k, stride, transposed = R.CONV_KINDS[kind]
    Hi = 128 if (stride == 2 and not transposed) else 32 if transposed else 64
    x = torch.randn(B, Ci, Hi, Hi, generator=g) + 0.5
    w = torch.randn(*((Ci, Co, k, k) if transposed else (Co, Ci, k, k)), generator=g) * 0.05
    h = conv_with_sums(kind, x, w)
    assert tuple(h.shape) == (B, 64, 64, Co)
    check_case('sums', None, mode, ld2c, act, with_res, seed=11 + mode, forms=('plain', 'split'), x=h, sums_ready=True)


def _sums_cases(side):
    """(label, conv_problem keywords, intended ratio or None)"""
    out = [('ratio%g' % r, dict(ratio=r), r) for r in R.RATIOS]
    for kq in (10.0, 100.0, 1000.0):
        out.append(('corner+%g' % kq, dict(ratio=0.0, moved=kq), None))
    out.append(('ratio10,corner-1000', dict(ratio=10.0, moved=-1000.0), None))         # (the moved block is part of sigma: no ratio to hold)
    out.append(('spike', dict(ratio=0.0, sigma_x=0.0, delta=0.01, moved=1.0), None))
    out.append(('magnitudes', dict(ratio=3.0, sigma_x=120.0, magnitudes=True), 3.0))
    return out


SUMS_COND = [pytest.param(kind, 64, id='%s-64' % kind) for kind in SUMS_LAYERS] + \
            [pytest.param('s1', 256, id='s1-256'), pytest.param('stem7', 256, id='stem7-256')] + \
            [pytest.param(kind, 256, id='%s-256' % kind, marks=pytest.mark.gpu_slow) for kind in ('s2', 'convT', 'f6')]


@pytest.mark.parametrize('kind,side', SUMS_COND)
def test_conditioning_from_sums(kind, side):
    """the conditioning cases on the from-sums path: the convolution's INPUT is built so that its OUTPUT has the wanted |mean| / sigma
    (checked in float64 on what the kernel wrote: within a factor two), a moved corner, a single spike, channels at 1e4 and 1e-4.

    At 65536 pixels these cases are what made the convolution epilogues accumulate in fp64: with several hundred fp32 atomics per
    address 'ratio10,corner-1000' measured 2.1e-06 .. 2.4e-06 against the floor of 2e-06 (1e-6 of relative error in sum y, entering
    the variance through -2 mean d(mean)); with fp64 accumulators it measures 2e-07."""
    B, Ci, Co = SUMS_LAYERS[kind][0 if side == 64 else 1]
    k = R.CONV_KINDS[kind][0]
    failed = []
    for i, (label, kw, want_ratio) in enumerate(_sums_cases(side)):
        kw = dict(kw)
        if kw.get('moved') and kw.get('sigma_x', 1.0) > 0:
            kw['moved'] *= (k * k * Ci) ** 0.5                   # K * |w[co, tap, 0]| ~ moved * sigma of the output channel
        if kw.pop('magnitudes', False):
            kw['row_scale'] = torch.tensor([1.0, 1e2, 1e-6]).repeat(Co // 3 + 1)[:Co]      # (256 * w has to stay an fp16 number)
        x, w = R.conv_problem(kind, B, Ci, Co, side, side, seed=40 + i, **kw)
        h = conv_with_sums(kind, x, w)
        got = R.achieved_ratio(h.cpu())
        if want_ratio:
            assert bool(((got > want_ratio / 2) & (got < want_ratio * 2)).all()), (label, got.min().item(), got.max().item())
        elif label.startswith('corner'):
            s = R.stats64(h.cpu())
            far = (h[:, 0, 0, :].double().cpu() - s['mean']).abs() / s['sigma']
            print('COND sums   %-26s corner pixel %.1f sigma (median over channels) from the channel mean' % (label, far.median().item()))
        mode, ld2c, act, with_res = CONFIGS[(3 * i + len(kind)) % len(CONFIGS)]
        if with_res:
            with_res = False
        try:
            check_case('sums', None, mode, ld2c, act, with_res, seed=300 + i, forms=('plain',), x=h, sums_ready=True,
                       cond='%s %s' % (kind, label))
        except AssertionError as e:
            failed.append(str(e).split('\n')[0])
    assert not failed, '\n'.join(failed)


# ------------------------------------------------------------------------------------------- conditioning: tile and streaming
@pytest.mark.parametrize('path,hw', [('tile', (32, 32)), ('stream', (32, 32)), ('stream', (64, 64)), ('stream', (256, 256))])
def test_conditioning(path, hw):
    """|mean| / sigma in {0, 3, 10, 30, 100, 1000} with both signs, pixel 0 and the corner 3x3 block moved by 10 .. 1000 sigma, a channel
    constant but for one pixel, channels at 1e4 and 1e-4: forward, mean, rstd, dx and the parameter gradients inside
    max(8 * e_ref, 2e-6), e_ref = the error of torch's fp32 CPU kernel on the same input"""
    failed = []
    for i, (label, x) in enumerate(R.conditioning_inputs(*hw).items()):
        if path == 'tile':                       # C % 32 == 0: the same channels several times over
            x = torch.cat([x] * (32 // x.shape[-1]), -1).contiguous()
        mode, ld2c, act, with_res = CONFIGS[(5 * i + (0 if path == 'tile' else 3)) % len(CONFIGS)]
        try:
            check_case(path, None, mode, ld2c, act, False, seed=400 + i, forms=('plain', 'add'), x=x, cond=label)
        except AssertionError as e:
            failed.append(str(e).split('\n')[0])
    assert not failed, '\n'.join(failed)


# --------------------------------------------------------------------------------------------------- the dispatch in ops_norm.py
@pytest.mark.parametrize('shape,expect', [((2, 32, 32, 64), 'tile'), ((2, 25, 41, 32), 'stream'), ((2, 16, 16, 16), 'stream'), ((1, 40, 48, 8), 'stream')])
@pytest.mark.parametrize('op', ['plain_relu', 'affine_res', 'affine_lrelu', 'spade', 'spade_fused_relu'])
def test_ops_dispatch(shape, expect, op):
    L = _L()
    from hoig_amd import ops
    B, H, W, C = shape
    x, g = well_conditioned(shape, seed=H + C)
    aw, ab = torch.randn(C, generator=g) * 0.5 + 1, torch.randn(C, generator=g) * 0.5
    ga, be = torch.randn(shape, generator=g) * 0.3, torch.randn(shape, generator=g) * 0.3
    res = torch.randn(shape, generator=g)
    dy = torch.randn(shape, generator=g)
    xd = x.cuda().requires_grad_(True)
    leaves = []
    if op == 'plain_relu':
        y = ops.instance_norm(xd, act=L.ACT_RELU)
        cfg = dict(mode=0, act=RELU)
    elif op == 'affine_res':
        leaves = [aw.cuda().requires_grad_(True), ab.cuda().requires_grad_(True)]
        y = ops.instance_norm(xd, leaves[0], leaves[1], residual=res.cuda())
        cfg = dict(mode=1, p0=aw, p1=ab, residual=res)
    elif op == 'affine_lrelu':
        leaves = [aw.cuda().requires_grad_(True), ab.cuda().requires_grad_(True)]
        y = ops.instance_norm(xd, leaves[0], leaves[1], act=L.ACT_LRELU, slope=SLOPE)
        cfg = dict(mode=1, p0=aw, p1=ab, act=LRELU, slope=SLOPE)
    elif op == 'spade':
        leaves = [ga.cuda().requires_grad_(True), be.cuda().requires_grad_(True)]
        y = ops.spade_norm(xd, leaves[0], leaves[1])
        cfg = dict(mode=2, p0=ga, p1=be)
    else:
        leaves = [torch.cat([ga, be], -1).cuda().requires_grad_(True)]
        y = ops.spade_norm_fused(xd, leaves[0], act=L.ACT_RELU)
        cfg = dict(mode=2, p0=ga, p1=be, act=RELU)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    for ws in ops._norm_ws.values():
        assert int(torch.count_nonzero(ws[:POOL])) == 0
    ref = R.reference(x, dy=dy, mask_from=y.detach() if 'act' in cfg else None, **cfg)
    assert R.rel_err(y, ref['y']) < TOL and R.chan_err(y, ref['y']) < TOL
    assert R.rel_err(xd.grad, ref['dx']) < 5 * TOL and R.chan_err(xd.grad, ref['dx']) < 5 * TOL
    if op == 'spade_fused_relu':
        assert R.rel_err(leaves[0].grad[..., :C], ref['dp0']) < 5 * TOL and R.rel_err(leaves[0].grad[..., C:], ref['dp1']) < 5 * TOL
    elif leaves:
        assert R.rel_err(leaves[0].grad, ref['dp0']) < 5 * TOL and R.rel_err(leaves[1].grad, ref['dp1']) < 5 * TOL


@pytest.mark.parametrize('kind,ratio', [('s1', 100.0), ('stem7', 30.0), ('convT', 1000.0)])
def test_ops_hand_the_sums_over_and_hold_the_bound_on_an_ill_conditioned_layer(kind, ratio):
    """conv -> instance norm through hoig_amd.ops on a layer whose output has |mean| / sigma = ratio: the hand-off happens (the norm reads
    the convolution's sums) and the result is inside the conditioning bound"""
    L = _L()
    from hoig_amd import ops
    B, Ci, Co = SUMS_LAYERS[kind][0]
    k, stride, transposed = R.CONV_KINDS[kind]
    x, w = R.conv_problem(kind, B, Ci, Co, 64, 64, ratio, seed=9)
    ops.set_precision('bf16x3')
    try:
        xd = x.permute(0, 2, 3, 1).contiguous().cuda()
        wd = ops.pack_weight(w.cuda(), transposed=transposed)
        ops._stats_pending.clear()
        with torch.no_grad():
            h = ops.conv_transpose2d(xd, wd, norm_next=True) if transposed else ops.conv2d(xd, wd, None, stride, k // 2, dead_bias=True)
            assert len(ops._stats_pending) == 1
            y = ops.instance_norm(h)
            assert not ops._stats_pending
        torch.cuda.synchronize()
    finally:
        ops.set_precision('f32')
    for ws in ops._norm_ws.values():
        assert int(torch.count_nonzero(ws[:POOL])) == 0
    hc = h.cpu()
    got = R.achieved_ratio(hc)
    assert bool(((got > ratio / 2) & (got < ratio * 2)).all())
    ref, ref32 = R.reference(hc)['y'], R.reference(hc, dtype=torch.float32)['y']
    err, e_ref = R.img_chan_err(y, ref).max().item(), R.img_chan_err(ref32, ref).max().item()
    print('COND ops    %s ratio %g: err %.3g, e_ref %.3g' % (kind, ratio, err, e_ref))
    assert err <= R.bound(e_ref), (err, e_ref)
