"""The region reconstruction term (docs/region_loss.md) restated in float64 with numpy alone, the bounds the document derives, the
seeded cases, and the calls through hoig_amd.region_loss.head on CPU tensors (the twin) or device tensors (the kernels).  Shared by
tests/test_region_loss_cpu.py and tests/test_region_loss_gpu.py; nothing here is fitted to an observed error."""
import numpy as np

u = 2.0 ** -24          # the unit roundoff of fp32
e = 2.0 ** -53          # ... and of fp64
BAD_LABEL = 1           # HOIG_REGION_BAD_LABEL
THREADS, TILE, COUNT_TILE, MAX_R, MAX_N, MAX_C = 256, 4096, 4096, 7, 4096, 64     # the header's constants (checked by the CPU test)

# (N, H, W, C).  (3, 33, 65, 3): 6435 floats per image -- a ragged last vector, a ragged last workgroup, two workgroups per image.
# (1, 300, 300, 3): 66 workgroups for one image, more than a wave's 64 lanes: a finishing row longer than a wave.  (17, 3, 5, 3):
# 17 * 4 = 68 finishing rows, more than the finishing wave's 64 lanes.
SHAPES = [(1, 1, 1, 1), (1, 5, 7, 3), (2, 16, 16, 3), (3, 33, 65, 3), (2, 8, 8, 1), (1, 300, 300, 3), (17, 3, 5, 3)]
LAM, LAM_ALL, MIN_PIXELS = (0.0, 10.0, 2.5), 30.0, 4


def case(shape, seed=0, regions=2, zeros=True):
    """(pred, target, labels) of `shape`: images in [-1, 1], every eleventh element with d exactly 0, labels 0 .. regions seeded with
    every value (where the image has the pixels for it)."""
    N, H, W, C = shape
    g = np.random.default_rng([seed, N, H, W, C])
    pred = g.uniform(-1, 1, size=shape).astype(np.float32)
    target = g.uniform(-1, 1, size=shape).astype(np.float32)
    if zeros:
        flat_p, flat_t = pred.reshape(-1), target.reshape(-1)
        flat_p[::11] = flat_t[::11]
    labels = g.integers(0, regions + 1, size=(N, H, W)).astype(np.uint8)
    if H * W > regions:
        labels.reshape(N, -1)[:, :regions + 1] = np.arange(regions + 1, dtype=np.uint8)
    return pred, target, labels


def reference(pred, target, labels, lam=LAM, lam_all=LAM_ALL, min_pixels=MIN_PIXELS):
    """Section 1 of the issue in float64 -> dict(counts [N, R+1], V [R+1], status, L [R+1], L_all, regions = sum_r lam_r L_r,
    all = lam_all L_all, sign [N,H,W,C], A, B [N,H,W] (the frame and the region part of the gradient scale), grad)."""
    N, H, W, C = pred.shape
    R = len(lam) - 1
    d = pred.astype(np.float64) - target.astype(np.float64)
    ad = np.abs(d)
    counts = np.stack([(labels == r).reshape(N, -1).sum(1) for r in range(R + 1)], 1).astype(np.int64)
    valid = counts >= min_pixels
    V = valid.sum(0)
    bad = labels[labels > R]
    status = int(BAD_LABEL | (int(bad.max()) << 8)) if bad.size else 0
    L = np.zeros(R + 1)
    B = np.zeros((N, H, W))
    for r in range(R + 1):
        if V[r] == 0:
            continue
        acc = 0.0
        for i in range(N):
            if valid[i, r]:
                m = labels[i] == r
                acc += ad[i][m].sum() / (C * counts[i, r])
                B[i][m] = lam[r] / (float(V[r]) * C * counts[i, r])
        L[r] = acc / V[r]
    L_all = ad.sum() / (N * H * W * C)
    A = lam_all / (N * H * W * C)
    sign = np.where(d > 0, 1.0, np.where(d < 0, -1.0, 0.0))          # 0 at d = 0, and 0 for a NaN
    return dict(counts=counts, V=V, status=status, L=L, L_all=L_all, regions=float(np.dot(lam, L)), all=lam_all * L_all, sign=sign,
                A=A, B=B, grad=sign * (A + B)[..., None], n=N * H * W * C, N=N, R=R)


def grad_bound(want):
    """|dpred - sign (A + B)| <= (A + B) (2u + u^2 + 4e): each part is a double quotient (e) rounded once to fp32 (u), and the two are
    added in one fp32 add (one more u); the sign is exact."""
    return ((want['A'] + want['B']) * (2 * u + u * u + 4 * e))[..., None]


def value_bound(want, x):
    """|slot - x| <= |x| (2u + 2u^2 + 2 (n + N + R + 8) e): an fp32 difference has relative error <= u and the exact difference's sign;
    a sum of n doubles in any order is off by (n - 1) e of the sum of magnitudes (here every term is >= 0); the divisions, the sum over
    at most N images, the weights and the sum over R + 1 regions add N + R + 8 more e; the slot's own rounding is one more u."""
    return abs(x) * (2 * u + 2 * u * u + 2 * (want['n'] + want['N'] + want['R'] + 8) * e)


def run(dev, pred, target, labels, lam=LAM, lam_all=LAM_ALL, min_pixels=MIN_PIXELS, grads=True, reports=True, counts=True, split=True,
        init=0.0):
    """One call of the head on `dev` ('cpu': the twin) -> dict of numpy arrays: dpred, term, terms_r, term_all, counts, status (None
    where the pointer was null).  split: give term_all a slot of its own."""
    import torch
    from hoig_amd import region_loss as RL
    N, R = pred.shape[0], len(lam) - 1
    tp, tt, tl = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (pred, target, labels))
    slot = lambda n: torch.full((n,), init, dtype=torch.float32, device=dev)
    dp = torch.full(pred.shape, 7.0, dtype=torch.float32, device=dev) if grads else None
    term, terms_r, term_all = slot(1), slot(R + 1) if reports else None, slot(1) if split else None
    cnt = torch.full((N, R + 1), -1, dtype=torch.int32, device=dev) if counts else None
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    RL.head(tp, tt, tl, lam, lam_all, min_pixels, term, dpred=dp, terms_r=terms_r, term_all=term_all, counts=cnt, status=status)
    if dev != 'cpu':
        torch.cuda.synchronize()
    out = lambda t: None if t is None else t.cpu().numpy()
    return dict(dpred=out(dp), term=out(term), terms_r=out(terms_r), term_all=out(term_all), counts=out(cnt), status=out(status))


def same_bits(x, y, nan_payload=True):
    """Are two results of run() equal in every byte?  nan_payload=False: a NaN equals a NaN whatever its sign and payload bits."""
    for k in x:
        if (x[k] is None) != (y[k] is None):
            return False
        if x[k] is None:
            continue
        if nan_payload or x[k].dtype.kind != 'f':
            if x[k].tobytes() != y[k].tobytes():
                return False
        elif not np.array_equal(x[k], y[k], equal_nan=True) or not np.array_equal(np.signbit(x[k]) | np.isnan(x[k]),
                                                                                   np.signbit(y[k]) | np.isnan(y[k])):
            return False
    return True


def check(got, want, where=None):
    """A result of run() against reference(): counts, V and status equal; dpred exactly 0 or of the reference's sign, within
    grad_bound; the slots within value_bound.  Returns the largest error-to-bound ratios (gradient, values)."""
    m = None
    if got['counts'] is not None:
        assert np.array_equal(got['counts'], want['counts']), where
    assert int(got['status'][0]) == want['status'], (where, got['status'], want['status'])
    rg = 0.0
    if got['dpred'] is not None:
        g = got['dpred'].astype(np.float64)
        zero = want['sign'] == 0
        assert (g[zero] == 0).all(), where
        assert (np.sign(g[~zero]) == want['sign'][~zero]).all(), where
        err, bound = np.abs(g - want['grad']), np.broadcast_to(grad_bound(want), g.shape)
        assert (err <= bound).all(), (where, float((err - bound).max()))
        nz = bound > 0
        rg = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    rv = 0.0
    pairs = []
    if got['term_all'] is not None:
        pairs += [(float(got['term_all'][0]), want['all']), (float(got['term'][0]), want['regions'])]
    else:
        pairs += [(float(got['term'][0]), want['regions'] + want['all'])]
    if got['terms_r'] is not None:
        pairs += [(float(got['terms_r'][r]), want['L'][r]) for r in range(want['R'] + 1)]
    for have, ref in pairs:
        b = value_bound(want, ref)
        assert abs(have - ref) <= b, (where, have, ref, b)
        if b > 0:
            rv = max(rv, abs(have - ref) / b)
    return rg, rv
