"""A float64 restatement of the opt-in GAN objectives and the LeCam regulariser (docs/gan_objectives.md), written from the formulas --
Lim & Ye 2017 / Miyato et al. 2018 for the hinge, Goodfellow et al. 2014 for the non-saturating logistic form, Tseng et al. 2021 for
LeCam and the released code's relu form -- not from the kernels; with it the error bounds that docs/gan_objectives.md derives, as code.

Everything here is numpy float64 on the fp32 logits as given.  A result comes with its bound: the most the fp32 / fp64 arithmetic the
document prescribes may be away from the exact value."""
import math
import struct

import numpy as np

u = 2.0 ** -24            # fp32 unit roundoff
U = 2.0 ** -53            # fp64 unit roundoff
SLACK = 1.0 + 2.0 ** -10  # the second-order terms of every first-order bound below
LSGAN, HINGE, LOGISTIC = 0, 1, 2
PAPER, RELU = 0, 1
MODES = {'lsgan': LSGAN, 'hinge': HINGE, 'logistic': LOGISTIC}
FORMS = {'paper': PAPER, 'relu': RELU}
# documented worst errors (ulp) of (expf, log1pf): the host's from the GNU C library manual's table of known errors, the device's the
# OpenCL full-profile limits its math library is built to.  One ulp of y is at most 2 u |y|.
ULPS = {'host': (1, 1), 'device': (3, 2), 'exact': (0, 0)}
COUNT, ALPHA_R, ALPHA_F, GAMMA, START, BAD, LAST_R, LAST_F = range(8)
STATE_WORDS = 8
THREADS, CHUNK, MAX_GRID = 256, 512, 64
# the smallest sizes at which the layout can go wrong: one element; around a wave; a ragged last chunk over several workgroups; more
# chunks than the grid's cap, so that a workgroup walks several (and a ragged end); unequal sides
SIZES = [(1, 1), (63, 64), (64, 65), (65, 63), (3 * CHUNK + 77, 2 * CHUNK + 1), (MAX_GRID * CHUNK + 3 * CHUNK + 5, 130), (5, 130)]


def softplus(z):
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def term(mode, side, x, ulps=(0, 0)):
    """(value, derivative, |value error|, |derivative error|) per logit; side 0: D on real, 1: D on fake, 2: G on fake.  The errors
    are those of the fp32 evaluation the document prescribes (operation counts there)."""
    x = np.asarray(x, np.float64)
    ee, el = ulps
    if mode == LSGAN:
        t = x - (1.0, -1.0, 0.0)[side]
        k = 1 if side == 2 else 3                 # x * x: one rounding; (x -+ 1)^2: the difference's, twice, and the product's
        return t * t, 2 * t, k * u * t * t, (0 if side == 2 else 1) * u * np.abs(2 * t)
    if mode == HINGE:
        if side == 2:
            return -x, -np.ones_like(x), 0 * x, 0 * x
        t = 1.0 - x if side == 0 else 1.0 + x
        on = t > 0                                # (the rounded t has the sign of the exact one: the subgradient at the kink is 0)
        return np.where(on, t, 0.0), np.where(on, -1.0 if side == 0 else 1.0, 0.0), u * np.where(on, t, 0.0), 0 * x
    z = x if side == 1 else -x
    v, d = softplus(z), sigmoid(z)
    ev = (1 + 2 * (ee + el)) * u * v              # exp, log1p (its value is at most v), the sum's rounding
    ed = (3 + 3 * ee) * u * d                     # exp through 1 + e and e * r; the sum's, the quotient's, the product's roundings
    return v, (d if side == 1 else -d), ev, ed


def lecam(form, side, x, alpha):
    """(value, derivative, |value error|, |derivative error|) of the regulariser's term per logit against the other side's anchor;
    the kernels round the anchor to fp32 (u |alpha|), the difference (u |t|) and the square (u t^2)."""
    x = np.asarray(x, np.float64)
    t = x - alpha if (form == PAPER or side == 0) else alpha - x
    sign = 1.0 if (form == PAPER or side == 0) else -1.0
    et = u * (abs(alpha) + np.abs(t))
    if form == RELU:
        # a t within et of 0 may fall on the other side of the max: its whole value is then the error, and et covers it
        t = np.maximum(t, 0.0)
    return t * t, sign * 2 * t, 2 * np.abs(t) * et + et * et + u * t * t, 2 * et


def new_state(gamma=0.99, start=1000, count=0, alpha_r=0.0, alpha_f=0.0):
    return dict(count=count, alpha_r=alpha_r, alpha_f=alpha_f, gamma=gamma, start=start, bad=0, last_r=0.0, last_f=0.0)


def tick(st, ma, mb):
    """The state after a step whose means were ma = mean(a), mb = mean(b)."""
    st = dict(st)
    if not (math.isfinite(ma) and math.isfinite(mb)):
        st['bad'] += 1
        return st
    if st['count'] == 0:
        st['alpha_r'], st['alpha_f'] = ma, mb
    else:
        g = st['gamma']
        st['alpha_r'] = g * st['alpha_r'] + (1 - g) * ma
        st['alpha_f'] = g * st['alpha_f'] + (1 - g) * mb
    st['count'] += 1
    st['last_r'], st['last_f'] = ma, mb
    return st


def weight_on(st):
    return st is not None and st['count'] >= st['start']


def _sum_err(n, mean_abs):
    """an fp64 sum of n terms in any order, its division by n and a few more fp64 operations: (n + 8) U of the mean magnitude"""
    return (n + 8) * U * mean_abs


def d_step(mode, a, b, s, lam=0.0, form=PAPER, st=None, ulps=(0, 0)):
    """The D step on logits a (real), b (fake) with the state `st` as it stands BEFORE the step (None: no regulariser):
    dict(obj, da, db, mean_a, mean_b, reg) and dict of their bounds; `reg` is w R, without lambda."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = a.size, b.size
    va, dva, eva, eda = term(mode, 0, a, ulps)
    vb, dvb, evb, edb = term(mode, 1, b, ulps)
    obj = s * va.mean() + s * vb.mean()
    e_obj = abs(s) * (eva.mean() + evb.mean()) + _sum_err(na, abs(s) * np.abs(va).mean()) + _sum_err(nb, abs(s) * np.abs(vb).mean())
    # the gradient's scale s / n is rounded to fp32 and multiplied in fp32: two more roundings of the product
    da, db = s / na * dva, s / nb * dvb
    e_da, e_db = abs(s) / na * eda + 2 * u * np.abs(da), abs(s) / nb * edb + 2 * u * np.abs(db)
    reg = e_reg = 0.0
    if st is not None:
        ra, dra, era, edra = lecam(form, 0, a, st['alpha_f'])
        rb, drb, erb, edrb = lecam(form, 1, b, st['alpha_r'])
        if weight_on(st):
            reg = ra.mean() + rb.mean()
            e_reg = era.mean() + erb.mean() + _sum_err(na, ra.mean()) + _sum_err(nb, rb.mean())
            obj, e_obj = obj + lam * reg, e_obj + lam * e_reg + 4 * U * abs(obj + lam * reg)
            ga, gb = lam / na * dra, lam / nb * drb
            # ... likewise for lambda / n; and the sum of the two products rounds once more
            e_da = e_da + lam / na * edra + 2 * u * np.abs(ga) + u * np.abs(da + ga)
            e_db = e_db + lam / nb * edrb + 2 * u * np.abs(gb) + u * np.abs(db + gb)
            da, db = da + ga, db + gb
    ma, mb = a.mean(), b.mean()
    out = dict(obj=obj, da=da, db=db, mean_a=ma, mean_b=mb, reg=reg)
    # the four scalars are rounded to fp32 where they are added to their (zero) slots
    bound = dict(obj=(e_obj + u * abs(obj)) * SLACK, da=e_da * SLACK, db=e_db * SLACK,
                 mean_a=(_sum_err(na, np.abs(a).mean()) + u * abs(ma)) * SLACK, mean_b=(_sum_err(nb, np.abs(b).mean()) + u * abs(mb)) * SLACK,
                 reg=(e_reg + u * abs(reg)) * SLACK)
    return out, bound


def g_step(mode, b, s, ulps=(0, 0)):
    """The generator's term on D(fake): dict(obj, db) and their bounds."""
    b = np.asarray(b, np.float64)
    v, dv, ev, ed = term(mode, 2, b, ulps)
    obj, db = s * v.mean(), s / b.size * dv
    e_obj = abs(s) * ev.mean() + _sum_err(b.size, abs(s) * np.abs(v).mean()) + u * abs(obj)
    return dict(obj=obj, db=db), dict(obj=e_obj * SLACK, db=(abs(s) / b.size * ed + 2 * u * np.abs(db)) * SLACK)


def anchor_bound(k, means, fed_fp32=False):
    """|anchor after k ticks - the float64 recurrence|: three fp64 roundings per tick on values no larger than the largest mean; fed
    with fp32 roundings of the means (the trainer's report slots) a convex combination of them is off by at most u of the largest."""
    m = max(abs(x) for x in means)
    return (4 * k * U * m + (u * m if fed_fp32 else 0.0)) * SLACK


# ------------------------------------------------------------------------------------------------ inputs and the state's words
def logits(n, seed, kink=True):
    """fp32 logits around the objectives' interesting points: a normal cloud, exact zeros, and values at and next to the hinge's kinks."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 1.5 + rng.uniform(-0.5, 0.5)).astype(np.float32)
    if kink:
        special = np.array([0.0, 1.0, -1.0, -0.0, np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(-1), np.float32(-2)),
                            12.5, -30.0], np.float32)
        pos = rng.permutation(n)[:min(n, special.size)]
        x[pos] = special[:pos.size]
    return x


class _Anchors(object):
    """What gan_loss.d_head takes as `lecam`: a state tensor, a weight and a form."""

    def __init__(self, state, weight, form):
        self.state, self.weight, self.form = state, weight, form


def run_d(dev, mode, a, b, s, lam=0.0, form=PAPER, st=None, grads=True, init=0.0):
    """hoig_gan_d_loss on device `dev` ('cpu': the twin) -> dict(obj, mean_a, mean_b, reg: fp32 scalars; da, db: fp32 arrays or None;
    state: the reference state after the call, or None; words: its bytes).  The four slots start at `init`."""
    import torch
    from hoig_amd import gan_loss as G
    ta, tb = torch.from_numpy(np.ascontiguousarray(a)).to(dev), torch.from_numpy(np.ascontiguousarray(b)).to(dev)
    da, db = (torch.full_like(ta, 7.0), torch.full_like(tb, 7.0)) if grads else (None, None)
    slots = torch.full((4,), float(init), dtype=torch.float32, device=dev)
    lc = None
    if st is not None:
        lc = _Anchors(torch.from_numpy(state_words(st).view(np.int64).copy()).to(dev), float(lam), form)
    G.d_head(mode, ta, tb, s, lc, da, db, slots[0:1], slots[1:2], slots[2:3], slots[3:4])
    if dev != 'cpu':
        torch.cuda.synchronize()
    sl = slots.cpu().numpy()
    out = dict(obj=sl[0], mean_a=sl[1], mean_b=sl[2], reg=sl[3], da=None if da is None else da.cpu().numpy(),
               db=None if db is None else db.cpu().numpy(), state=None, words=b'')
    if lc is not None:
        w = lc.state.cpu().numpy()
        out['state'], out['words'] = words_state(w), w.tobytes()
    return out


def run_g(dev, mode, b, s, grads=True, init=0.0):
    """hoig_gan_g_loss on device `dev` -> dict(obj, db)."""
    import torch
    from hoig_amd import gan_loss as G
    tb = torch.from_numpy(np.ascontiguousarray(b)).to(dev)
    db = torch.full_like(tb, 7.0) if grads else None
    slot = torch.full((1,), float(init), dtype=torch.float32, device=dev)
    G.g_head(mode, tb, s, db, slot)
    if dev != 'cpu':
        torch.cuda.synchronize()
    return dict(obj=slot.cpu().numpy()[0], db=None if db is None else db.cpu().numpy())


def same_bits(x, y):
    """Two results of run_d / run_g, bit for bit."""
    for k in x:
        vx, vy = x[k], y[k]
        if isinstance(vx, dict) or vx is None or vy is None:
            if (vx is None) != (vy is None):
                return False
            continue
        if (vx if isinstance(vx, bytes) else np.asarray(vx).tobytes()) != (vy if isinstance(vy, bytes) else np.asarray(vy).tobytes()):
            return False
    return True


def check_d(got, want, bound, what=''):
    """The fp32 results `got` (run_d) against the float64 (want, bound) of d_step."""
    for k in ('obj', 'mean_a', 'mean_b', 'reg'):
        assert abs(float(got[k]) - want[k]) <= bound[k], (what, k, float(got[k]), want[k], bound[k])
    for k in ('da', 'db'):
        if got[k] is not None:
            err = np.abs(got[k].astype(np.float64) - want[k])
            i = int(np.argmax(err - bound[k]))
            assert (err <= bound[k]).all(), (what, k, i, float(got[k][i]), float(want[k][i]), float(np.broadcast_to(bound[k], err.shape)[i]))


def f2w(x):
    return struct.unpack('<Q', struct.pack('<d', float(x)))[0]


def w2f(w):
    return struct.unpack('<d', struct.pack('<Q', int(w) % 2 ** 64))[0]


def state_words(st):
    """The uint64 words of the device state for the reference state `st`."""
    w = np.zeros(STATE_WORDS, np.uint64)
    w[COUNT], w[START], w[BAD] = st['count'], st['start'], st['bad']
    for i, k in ((ALPHA_R, 'alpha_r'), (ALPHA_F, 'alpha_f'), (GAMMA, 'gamma'), (LAST_R, 'last_r'), (LAST_F, 'last_f')):
        w[i] = f2w(st[k])
    return w


def words_state(w):
    w = [int(v) for v in np.asarray(w).view(np.uint64)]
    return dict(count=w[COUNT], alpha_r=w2f(w[ALPHA_R]), alpha_f=w2f(w[ALPHA_F]), gamma=w2f(w[GAMMA]), start=w[START], bad=w[BAD],
                last_r=w2f(w[LAST_R]), last_f=w2f(w[LAST_F]))
