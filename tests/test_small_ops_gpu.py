"""The small kernels of pointwise.hip and sample.hip against float64 ATen, at the shapes their one-shape tests in test_ops_gpu.py
leave out: rectangular maps (all extents different, so that a swapped H / W shows), sizes beyond one pass of the capped grid
(2048 workgroups x 256 threads = 524288 work items; the loss / TV / sum reductions cap at 256 / 512 workgroups), pixel counts that
are no multiple of the vector width, pooling windows with ties, and the entry points that no test called directly."""
import pytest
import torch
import torch.nn.functional as F

from gpu_util import nhwc_cuda, nchw_cpu, poison_free_memory, rel_err

pytestmark = pytest.mark.gpu
GRID_PASS = 2048 * 256


@pytest.fixture(autouse=True)
def _unwritten_outputs_read_as_nan():
    poison_free_memory()


def _ops():
    from hoig_amd import ops
    return ops


def _lib():
    from hoig_amd import _lib as L
    return L


def _st():
    return torch.cuda.current_stream().cuda_stream


def _f(t):
    return t.detach().float()


# ---------------------------------------------------------------------------------------------------------------- sampling
def _sampling_grid(B, H, W, Ho, Wo, g):
    """Sampling positions in [-1.2, 1.2] plus, by construction: exactly -1 and +1 on each axis, exact pixel centres (2i+1)/n - 1, values
    beyond +-1, and rows of the -2 sentinel (utils/nmr.py:884)."""
    assert B >= 2 and Ho >= 8
    grid = torch.rand(B, Ho, Wo, 2, generator=g) * 2.4 - 1.2
    grid[0, 0, :, 0], grid[0, 1, :, 0], grid[0, 2, :, 1], grid[0, 3, :, 1] = -1.0, 1.0, -1.0, 1.0
    grid[0, 4, :, 0] = (2 * (torch.arange(Wo) % W).float() + 1) / W - 1
    grid[0, 5, :, 1] = (2 * (torch.arange(Wo) % H).float() + 1) / H - 1
    grid[0, 6, 0], grid[0, 6, 1], grid[0, 6, 2], grid[0, 6, 3] = torch.tensor([-1.0, -1.0]), torch.tensor([1.0, 1.0]), \
        torch.tensor([-1.0, 1.0]), torch.tensor([1.0, -1.0])
    grid[1, 0, :, 0], grid[1, 1, :, 1], grid[1, 2, :, 0], grid[1, 3, :, 1] = 1.5, 1.5, -1.5, -1.5
    grid[1, 4:6] = -2.0
    for ax in (0, 1):
        assert (grid[..., ax] == -1).any() and (grid[..., ax] == 1).any() and (grid[..., ax] > 1).any() and (grid[..., ax] < -1).any()
    assert (grid[1, 4:6] == -2).all()
    return grid


@pytest.mark.parametrize('B,C,H,W,Ho,Wo', [(2, 24, 9, 14, 11, 6),            # all four extents differ
                                           (3, 96, 20, 12, 48, 40)])        # 552960 outputs: a second pass of the grid
def test_grid_sample_rectangular(B, C, H, W, Ho, Wo):
    ops = _ops()
    g = torch.Generator().manual_seed(51)
    assert len({H, W, Ho, Wo}) == 4 and (B * Ho * Wo * C > GRID_PASS) == (C == 96)
    x = torch.randn(B, C, H, W, generator=g)
    grid = _sampling_grid(B, H, W, Ho, Wo, g)
    xr = x.double().requires_grad_(True)
    yr = F.grid_sample(xr, grid.double(), mode='bilinear', padding_mode='zeros', align_corners=False)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy.double())
    xd = nhwc_cuda(x).requires_grad_(True)
    y = ops.grid_sample(xd, grid.cuda())
    y.backward(nhwc_cuda(gy))
    e = rel_err(nchw_cpu(y), _f(yr)), rel_err(nchw_cpu(xd.grad), _f(xr.grad))
    print('SMALL grid_sample %s: out %.2e dx %.2e' % ((B, C, H, W, Ho, Wo), *e))
    assert e[0] < 1e-5 and e[1] < 1e-5
    assert torch.equal(nchw_cpu(y)[1, :, 4:6], torch.zeros(C, 2, Wo))       # the sentinel samples nothing


@pytest.mark.parametrize('B,C,Hi,Wi,Ho,Wo', [(2, 2, 64, 48, 24, 20), (1, 5, 13, 7, 7, 13), (2, 5, 7, 16, 13, 40), (1, 2, 9, 6, 1, 5),
                                             (2, 5, 1, 6, 4, 9)])
def test_resize_bilinear_ac_rectangular(B, C, Hi, Wi, Ho, Wo):
    ops = _ops()
    x = torch.randn(B, C, Hi, Wi, generator=torch.Generator().manual_seed(52))
    ref = F.interpolate(x.double(), size=(Ho, Wo), mode='bilinear', align_corners=True)
    e = rel_err(nchw_cpu(ops.resize_bilinear_ac(nhwc_cuda(x), Ho, Wo)), _f(ref))
    print('SMALL resize_bilinear_ac %s: %.2e' % ((B, C, Hi, Wi, Ho, Wo), e))
    assert e < 2e-5


@pytest.mark.parametrize('C', [12, 3])
@pytest.mark.parametrize('Hi,Wi,Ho,Wo', [(64, 48, 24, 20), (16, 10, 40, 24), (7, 13, 13, 7)])
def test_resize_nearest_rectangular(C, Hi, Wi, Ho, Wo):
    ops = _ops()
    x = torch.randn(2, C, Hi, Wi, generator=torch.Generator().manual_seed(53))
    ref = F.interpolate(x.double(), size=(Ho, Wo), mode='nearest')
    assert torch.equal(nchw_cpu(ops.resize_nearest(nhwc_cuda(x), Ho, Wo)).double(), ref)


@pytest.mark.parametrize('h', [5, 24])
def test_attn_flow_second_size(h):
    ops = _ops()
    from oracle import hogan_oracle as O
    T = torch.rand(2, 64, 64, 2, generator=torch.Generator().manual_seed(54)) * 2 - 1
    t = O.resize_trans(T, h).contiguous()                      # ATen's resize: the kernel under test is attn_flow alone
    assert rel_err(ops.attn_flow(t.cuda()), _f(O.attn_flow(T.double(), h))) < 2e-5


# ---------------------------------------------------------------------------------------------------------------- pooling
@pytest.mark.parametrize('B,C,H,W', [(2, 8, 6, 10), (4, 64, 96, 88)])       # 540672 outputs: a second pass of the grid
def test_maxpool_with_tied_windows(B, C, H, W):
    """VGG pools post-ReLU maps: windows of equal zeros.  The first maximum in scan order takes the gradient, as in ATen's CPU kernel."""
    ops = _ops()
    g = torch.Generator().manual_seed(55)
    assert (B * (H // 2) * (W // 2) * C > GRID_PASS) == (C == 64)
    x = torch.relu(torch.randn(B, C, H, W, generator=g))
    win = F.unfold(x.view(B * C, 1, H, W), 2, stride=2)        # [B*C, 4, windows]
    tied = ((win == win.max(1, keepdim=True).values).sum(1) > 1).float().mean().item()
    assert tied > 0.02, tied                                   # about 6 %: all four non-positive before the ReLU
    xr = x.double().requires_grad_(True)
    yr = F.max_pool2d(xr, 2, 2)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy.double())
    xd = nhwc_cuda(x).requires_grad_(True)
    y = ops.maxpool2(xd)
    y.backward(nhwc_cuda(gy))
    assert torch.equal(nchw_cpu(y).double(), yr.detach()) and torch.equal(nchw_cpu(xd.grad).double(), xr.grad)


# ---------------------------------------------------------------------------------------------------------------- losses
def _bce_pred(shape, g):
    """Probabilities that reach torch's clamps: within 1e-7 of 0 and of 1 (either target), and exactly 0 / 1 where the target agrees."""
    p = torch.rand(shape, generator=g) * 0.98 + 0.01
    t = (torch.rand(shape, generator=g) > 0.5).float()
    pf, tf = p.view(-1), t.view(-1)
    pf[0:4] = torch.tensor([1e-8, 1e-8, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24])
    tf[0:4] = torch.tensor([0.0, 1.0, 0.0, 1.0])
    pf[4:6], tf[4:6] = torch.tensor([0.0, 1.0]), torch.tensor([0.0, 1.0])
    assert pf[0] > 0 and pf[0] < 1e-7 and pf[2] < 1 and 1 - pf[2].double() < 1e-7
    return p, t


def _loss_case(name, shape, g):
    """-> (product loss on device leaves, float64 reference on CPU leaves, [(device leaf, reference leaf)], mask of ordinary elements)"""
    ops = _ops()
    dev = lambda t: t.cuda().requires_grad_(True)
    ref = lambda t: t.double().requires_grad_(True)
    plain = None
    if name == 'tv':
        B, H, W = shape
        m = torch.rand(B, 1, H, W, generator=g)
        md, mr = nhwc_cuda(m).requires_grad_(True), ref(m)
        lr = ((mr[:, :, :, :-1] - mr[:, :, :, 1:]).abs().mean() + (mr[:, :, :-1] - mr[:, :, 1:]).abs().mean()) * 3.0
        return ops.tv_loss(md, 3.0), lr, [(md, mr)], plain      # (one channel: NHWC and NCHW share their flat order)
    full = (shape[0], 3) + tuple(shape[1:])
    if name == 'bce':
        p, t = _bce_pred(full, g)
        plain = torch.ones(full, dtype=torch.bool)
        plain.view(-1)[:6] = False
    else:
        p, t = torch.randn(full, generator=g), torch.randn(full, generator=g)
    pd, pr = dev(p), ref(p)
    if name == 'l1':
        return ops.l1_loss(pd, t.cuda(), 10.0), F.l1_loss(pr, t.double()) * 10.0, [(pd, pr)], plain
    if name == 'mse':
        return ops.mse_loss(pd, t.cuda(), 0.5), F.mse_loss(pr, t.double()) * 0.5, [(pd, pr)], plain
    if name == 'bce':
        return ops.bce_loss(pd, t.cuda(), 1.5), F.binary_cross_entropy(pr, t.double()) * 1.5, [(pd, pr)], plain
    assert name == 'lsgan'
    return ops.lsgan_loss(pd, 1.0, 2.0), torch.mean((pr - 1) ** 2) * 2.0, [(pd, pr)], plain


@pytest.mark.parametrize('shape', [(2, 37, 53),                # rectangular, odd; 11766 = 2 mod 4 elements with three channels
                                   (4, 256, 272)])             # 835584 elements (TV: 278528 pixels): every workgroup of the capped grids loops
@pytest.mark.parametrize('name', ['l1', 'mse', 'bce', 'lsgan', 'tv'])
def test_losses_rectangular_and_beyond_the_capped_grid(name, shape):
    g = torch.Generator().manual_seed(56)
    n = shape[0] * shape[1] * shape[2]
    if shape[1] == 37:
        assert (3 * n) % 4 != 0 and n % 4 != 0
    else:
        assert 3 * n > 2 * 256 * 256 * 4 and n > 2 * 512 * 256
    loss, loss_r, pairs, plain = _loss_case(name, shape, g)
    loss.backward()
    loss_r.backward()
    ev = abs(loss.item() - loss_r.item()) / abs(loss_r.item())
    print('SMALL loss %-5s %s: value %.2e' % (name, shape, ev), end='')
    assert ev < 1e-4
    for d, r in pairs:
        dg, rg = d.grad.cpu().reshape(-1), _f(r.grad).reshape(-1)
        eg = rel_err(dg, rg)
        print(' grad %.2e' % eg, end='')
        assert eg < 1e-4
        if plain is not None:                                  # the clamped entries' gradients are ~1e7 times the others': those on their own
            eo = rel_err(dg[plain.reshape(-1)], rg[plain.reshape(-1)])
            print(' ordinary entries %.2e' % eo, end='')
            assert eo < 1e-4
    print()


@pytest.mark.parametrize('kind', ['l1', 'mse', 'bce'])
def test_loss_kernel_scalar_path_on_unaligned_pointers(kind):
    """hoig_loss_fwd_bwd with pred and dpred one float into a larger buffer (no 16-B alignment: the kernel's `vec == false` path): the
    results of the aligned call on the same values, and nothing written outside the n elements."""
    L = _lib()
    g = torch.Generator().manual_seed(57)
    n, k = 2 * 37 * 53 * 3, {'l1': L.LOSS_L1, 'mse': L.LOSS_MSE, 'bce': L.LOSS_BCE}[kind]
    p, t = (_bce_pred((n,), g) if kind == 'bce' else (torch.randn(n, generator=g), torch.randn(n, generator=g)))
    pa, ta = p.cuda(), t.cuda()
    pbuf = torch.zeros(n + 8, device='cuda')
    pbuf[1:n + 1] = pa
    dbuf = torch.full((n + 8,), 777.0, device='cuda')
    da = torch.empty(n, device='cuda')
    outs = torch.zeros(2, device='cuda')
    assert pa.data_ptr() % 16 == 0 and ta.data_ptr() % 16 == 0 and da.data_ptr() % 16 == 0 and pbuf.data_ptr() % 16 == 0
    L.call('hoig_loss_fwd_bwd', k, pa.data_ptr(), ta.data_ptr(), 0.0, 0.25, outs.data_ptr(), da.data_ptr(), n, _st())
    L.call('hoig_loss_fwd_bwd', k, pbuf.data_ptr() + 4, ta.data_ptr(), 0.0, 0.25, outs.data_ptr() + 4, dbuf.data_ptr() + 4, n, _st())
    a, u = outs.tolist()
    pr = p.double().requires_grad_(True)
    want = {'l1': lambda: (pr - t.double()).abs().sum(), 'mse': lambda: ((pr - t.double()) ** 2).sum(),
            'bce': lambda: F.binary_cross_entropy(pr, t.double(), reduction='sum')}[kind]()
    want.backward()
    assert abs(a - want.item()) < 1e-4 * want.item() and abs(u - want.item()) < 1e-4 * want.item()
    # the two paths add the same non-negative terms in another order, each through at most ~70 fp32 additions (46 per thread, the
    # workgroup's tree, 12 atomics): 70 * 2^-24 = 4.2e-6 of relative error apiece at the very most
    assert abs(a - u) <= 1e-5 * abs(a)
    assert torch.equal(dbuf[1:n + 1], da)
    assert rel_err(da, _f(pr.grad * 0.25)) < 1e-4
    assert bool((dbuf[:1] == 777.0).all()) and bool((dbuf[n + 1:] == 777.0).all())


def test_mean_of_four_million_elements():
    """hoig_sum over 2^22 elements (512 workgroups x 256 threads x 32 elements each, fp32 partials) against the float64 sum.
    Measured on the MI355X: 4.4e-7 (the limit is 1e-5)."""
    ops = _ops()
    x = torch.rand(1 << 22, generator=torch.Generator().manual_seed(58)) + 0.5
    want = x.double().mean().item()
    e = abs(ops.mean(x.cuda()).item() - want) / want
    print('SMALL mean 2^22: %.2e' % e)
    assert e < 1e-5


def test_compose_rectangular():
    ops = _ops()
    g = torch.Generator().manual_seed(59)
    B, H, W = 2, 37, 53
    ts = [torch.randn(B, 3, H, W, generator=g) for _ in range(3)] + [torch.rand(B, 1, H, W, generator=g) for _ in range(2)]
    r = [t.double().requires_grad_(True) for t in ts]
    img_r = r[3] * r[0] + (1 - r[3]) * (r[1] * r[4] + r[2] * (1 - r[4]))
    gy = torch.randn(B, 3, H, W, generator=g)
    img_r.backward(gy.double())
    d = [nhwc_cuda(t).requires_grad_(True) for t in ts]
    img = ops.compose(*d)
    img.backward(nhwc_cuda(gy))
    assert rel_err(nchw_cpu(img), _f(img_r)) < 1e-6
    for dd, rr in zip(d, r):
        assert rel_err(nchw_cpu(dd.grad), _f(rr.grad)) < 1e-4


# ---------------------------------------------------------------------------------------------------------------- add / activations
ACTS = {'relu': (1, 0.0, torch.relu), 'lrelu': (2, 0.2, lambda v: F.leaky_relu(v, 0.2)), 'tanh': (3, 0.0, torch.tanh),
        'sigmoid': (4, 0.0, torch.sigmoid)}
N_BIG = (1 << 21) + 2051                                       # n % 4 == 3; n / 4 float4 items > one pass of the grid (hoig_add)


@pytest.mark.parametrize('n', [1, 3, 4, 1023, N_BIG])
def test_add(n):
    ops = _ops()
    assert n != N_BIG or (n % 4 == 3 and n // 4 > GRID_PASS)
    g = torch.Generator().manual_seed(60)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ad, bd = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = ops.add(ad, bd)
    gy = torch.randn(n, generator=g)
    y.backward(gy.cuda())
    assert rel_err(y, _f(a.double() + b.double())) < 1e-6
    assert torch.equal(ad.grad.cpu(), gy) and torch.equal(bd.grad.cpu(), gy)


@pytest.mark.parametrize('n', [1, 3, 4, 1023, N_BIG])
@pytest.mark.parametrize('act', list(ACTS))
def test_add_act_and_act_bwd(act, n):
    ops = _ops()
    code, slope, fn = ACTS[act]
    g = torch.Generator().manual_seed(61)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ar, br = a.double().requires_grad_(True), b.double().requires_grad_(True)
    yr = fn(ar + br)
    gy = torch.randn(n, generator=g)
    yr.backward(gy.double())
    ad, bd = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = ops.add_act(ad, bd, code, slope)
    y.backward(gy.cuda())
    e = rel_err(y, _f(yr)), rel_err(ad.grad, _f(ar.grad)), rel_err(bd.grad, _f(br.grad))
    assert max(e) < 1e-6, e


# ---------------------------------------------------------------------------------------------------------------- column sums
COLSUM_ROWS = (1, 31, 33, 4097, 20000)     # one short slab; 32-row slabs with a short last one; the 512-workgroup cap (40 rows per slab)


def _act_output(act, shape, g):
    """Values an activation can output, on a 1/256 grid: y * y and 1 - y are then exact in float32, so dy * act'(y) has ONE rounding
    however the compiler contracts it, and bit-equality with the CPU's float32 product is attainable."""
    v = torch.randn(shape, generator=g)
    y = {'relu': torch.relu(v), 'lrelu': F.leaky_relu(v, 0.2), 'tanh': torch.tanh(v), 'sigmoid': torch.sigmoid(v)}[act]
    return (y * 256).round() / 256


def _act_grad_from_y(act, y, slope):
    one = torch.ones_like(y)
    return {'relu': torch.where(y > 0, one, 0 * one), 'lrelu': torch.where(y > 0, one, slope * one), 'tanh': 1 - y * y,
            'sigmoid': y * (1 - y)}[act]


@pytest.mark.parametrize('C', [3, 19, 64, 300, 1028])          # scalar and float4 kernels; lanes < C (300, 1028); several row lanes (3, 19, 64)
def test_act_bwd_colsum_and_colsum_accum(C):
    L = _lib()
    g = torch.Generator().manual_seed(62)
    for i, rows in enumerate(COLSUM_ROWS):
        act = list(ACTS)[(i + C) % 4]
        code, slope, _ = ACTS[act]
        y, dy = _act_output(act, (rows, C), g), torch.randn(rows, C, generator=g)
        want_g = dy * _act_grad_from_y(act, y, slope)          # float32 on the CPU
        yd, dyd = y.cuda(), dy.cuda()
        gd = torch.full((rows, C), float('nan'), device='cuda')
        bias0 = torch.randn(C, generator=g)
        dbias = bias0.cuda()
        L.call('hoig_act_bwd_colsum', yd.data_ptr(), dyd.data_ptr(), gd.data_ptr(), dbias.data_ptr(), code, slope, rows, C, _st())
        assert torch.equal(gd.cpu(), want_g), (act, rows, C)
        e1 = rel_err(dbias, _f(bias0.double() + want_g.double().sum(0)))
        out0 = torch.randn(C, generator=g)
        out = out0.cuda()
        L.call('hoig_colsum_accum', dyd.data_ptr(), out.data_ptr(), rows, C, _st())
        e2 = rel_err(out, _f(out0.double() + dy.double().sum(0)))
        print('SMALL colsum C=%d rows=%d %s: dbias %.2e accum %.2e' % (C, rows, act, e1, e2))
        assert e1 < 1e-5 and e2 < 1e-5, (act, rows, C, e1, e2)


# ---------------------------------------------------------------------------------------------------------------- channels, layout
@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('Cc', [1, 5, 16])
def test_copy_channels_offsets_and_accumulate(Cc, accumulate):
    L = _lib()
    g = torch.Generator().manual_seed(63)
    npix, Cx, x_off, Cy, y_off = 3 * 7 * 13, 21, 4, 27, 9      # 273 pixels: no multiple of 256
    x, y0 = torch.randn(npix, Cx, generator=g), torch.randn(npix, Cy, generator=g)
    xd, yd = x.cuda(), y0.cuda()
    L.call('hoig_copy_channels', xd.data_ptr(), yd.data_ptr(), npix, Cx, x_off, Cy, y_off, Cc, accumulate, _st())
    want = y0.clone()
    part = x[:, x_off:x_off + Cc]
    want[:, y_off:y_off + Cc] = want[:, y_off:y_off + Cc] + part if accumulate else part
    assert torch.equal(yd.cpu(), want)                          # the written channels, and every other one as it was


def test_cat_channels_of_three():
    ops = _ops()
    g = torch.Generator().manual_seed(64)
    ts = [torch.randn(2, c, 7, 13, generator=g) for c in (3, 16, 5)]
    ds = [nhwc_cuda(t).requires_grad_(True) for t in ts]
    y = ops.cat_channels(ds)
    assert torch.equal(nchw_cpu(y), torch.cat(ts, 1))
    gy = torch.randn(2, 24, 7, 13, generator=g)
    y.backward(nhwc_cuda(gy))
    for d, r in zip(ds, torch.split(gy, [3, 16, 5], 1)):
        assert torch.equal(nchw_cpu(d.grad), r)


@pytest.mark.parametrize('B,C,H,W', [(3, 19, 5, 33), (1, 33, 1, 1)])       # partial 32x32 tiles along both axes
def test_layout_conversions(B, C, H, W):
    ops = _ops()
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(65))
    nhwc = ops.nchw_to_nhwc(x.cuda())
    assert torch.equal(nhwc.cpu(), x.permute(0, 2, 3, 1).contiguous())
    assert torch.equal(ops.nhwc_to_nchw(nhwc).cpu(), x)
