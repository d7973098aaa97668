"""What the Adam kernels must compute (adam_kernel, adam_dev_kernel, adam_tick_kernel in hoig_amd/csrc/pointwise.hip, adam_pack_kernel
in hoig_amd/csrc/weight_planes.hip; docs/optimizer_parity.md), without a GPU and without the project's code:

  adam64       the update in float64 with exact (double) scalars: the truth.
  adam32_twin  the same in numpy float32, one rounding per operation in the order of the kernel's comment, no FMA, with the six scalars
               rounded once from double as adam_tick_kernel makes them.  It is NOT what the kernel must equal (the compiler contracts
               a*b + c into an FMA, and divide / sqrt may differ in the last place): it says how much error fp32 arithmetic itself costs
               on a given row, which is the unit the device tests measure the kernels in.
  derived64    the six scalars of `derived`, in double.

Semantics (no weight decay, no amsgrad), per step, g' = g * (grad_scale * guard[0]):
  m += (g' - m)(1 - b1);  v = v b2 + (1 - b2) g'^2;  p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps),   bc = 1 - beta^step
guard[1] != 0: the step changes nothing and does not count.
"""
import math

import numpy as np

F32_MIN_NORMAL = float(np.finfo(np.float32).tiny)


def derived64(lr, b1, b2, eps, step):
    """(lr / bc1, 1 - b1, b2, 1 - b2, eps, sqrt(bc2)) of the 1-based step count `step`, as Python floats (doubles)."""
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return (lr / bc1, 1.0 - b1, b2, 1.0 - b2, eps, math.sqrt(bc2))


def _guards(guard, nsteps):
    """guard: None, one (scale, skip) pair for every step, or a list of pairs / None, one per step."""
    if guard is None:
        return [None] * nsteps
    if len(guard) == 2 and not isinstance(guard[0], (tuple, list, np.ndarray)) and guard[0] is not None:
        return [guard] * nsteps
    assert len(guard) == nsteps
    return list(guard)


def adam64(p, g_list, m, v, step0, lr, betas, eps, grad_scale=1, guard=None):
    """`len(g_list)` steps from the count `step0` (the first step taken is number step0 + 1).
    -> (p, m, v, [the update p_before - p_after of every step: zeros for a skipped one], the count afterwards), float64."""
    p, m, v = (np.array(a, dtype=np.float64) for a in (p, m, v))
    step, updates = int(step0), []
    for g, gd in zip(g_list, _guards(guard, len(g_list))):
        if gd is not None and float(gd[1]) != 0.0:
            updates.append(np.zeros_like(p))
            continue
        step += 1
        step_size, omb1, b2, omb2, eps_, bc2_sqrt = derived64(lr, betas[0], betas[1], eps, step)
        scale = float(grad_scale) * (float(gd[0]) if gd is not None else 1.0)
        gs = np.asarray(g, dtype=np.float64) * scale
        m = m + (gs - m) * omb1
        v = v * b2 + omb2 * (gs * gs)
        upd = step_size * (m / (np.sqrt(v) / bc2_sqrt + eps_))
        p = p - upd
        updates.append(upd)
    return p, m, v, updates, step


def _zero_or_normal(name, a):
    a = np.abs(np.asarray(a, dtype=np.float32))
    bad = (a != 0) & ~(a >= np.float32(F32_MIN_NORMAL))
    assert not bad.any(), 'float32 intermediate %s is subnormal or not finite at %d places (e.g. %r)' % (name, int(bad.sum()), a[bad][:3])
    assert np.isfinite(a).all(), 'float32 intermediate %s is not finite' % name


def adam32_twin(p, g_list, m, v, step0, lr, betas, eps, grad_scale=1, guard=None, check=True):
    """adam64's arguments and results, in float32: every operation rounds once, in the order
        gk = g * gscale;  m = m + (gk - m) * omb1;  v = v * b2 + omb2 * (gk * gk);  denom = sqrt(v) / bc2_sqrt + eps;
        p = p - step_size * (m / denom)
    with gscale = float(grad_scale) * guard[0] (one fp32 product, as the guarded kernels form it).
    check: assert that g * gscale, its square, (1 - b2) times that, v and sqrt(v) are each exactly 0 or a normal float32 -- on rows
    where that holds, how the device treats subnormals is not in question."""
    f = np.float32
    p, m, v = (np.array(a, dtype=f) for a in (p, m, v))
    step, updates = int(step0), []
    with np.errstate(divide='ignore', invalid='ignore'):
        for g, gd in zip(g_list, _guards(guard, len(g_list))):
            if gd is not None and float(gd[1]) != 0.0:
                updates.append(np.zeros_like(p))
                continue
            step += 1
            step_size, omb1, b2, omb2, eps_, bc2_sqrt = (f(x) for x in derived64(lr, betas[0], betas[1], eps, step))
            gscale = f(grad_scale) * f(gd[0]) if gd is not None else f(grad_scale)
            gk = np.asarray(g, dtype=f) * gscale
            t = gk - m
            t = t * omb1
            m = m + t
            a = v * b2
            gg = gk * gk
            c = omb2 * gg
            v = a + c
            s = np.sqrt(v)
            d = s / bc2_sqrt
            d = d + eps_
            q = m / d
            upd = step_size * q
            p = p - upd
            if check:
                for name, x in (('g*scale', gk), ('g^2', gg), ('(1-b2) g^2', c), ('v', v), ('sqrt(v)', s)):
                    _zero_or_normal(name, x)
            assert all(x.dtype == f for x in (p, m, v, upd))
            updates.append(upd)
    return p, m, v, updates, step


# ------------------------------------------------------------------------------------------------ rows and measures
def gradients(n, seed, sign_seed=None):
    """One row of gradients, float32: sign * 10^u with u uniform in [-12, 3]; where the row is long enough, a block of exact zeros and a
    block with |g| about 1e-9 (there eps = 1e-8 is most of the denominator).  The blocks sit at fixed fractions of the row, off multiples
    of 4 where they can be.  sign_seed: the signs come from it alone, so that rows of different `seed` share them (row_steps)."""
    rng = np.random.RandomState(seed)
    sign = rng.choice([-1.0, 1.0], n)
    if sign_seed is not None:
        sign = np.random.RandomState(sign_seed).choice([-1.0, 1.0], n)
    g = (sign * 10.0 ** rng.uniform(-12.0, 3.0, n)).astype(np.float32)
    if n >= 8:
        blk = max(2, min(n // 8, 4099))
        a = (n // 4) | 1
        g[a:a + blk] = 0.0
        b = (n // 2) | 1
        g[b:b + blk] = (sign[b:b + blk] * 1e-9 * rng.uniform(0.5, 2.0, blk)[:len(g[b:b + blk])]).astype(np.float32)
    return g


STEPS = (1, 2, 3, 10, 1000, 100000)        # the step counts a row goes through
LR, EPS = 2e-4, 1e-8


def row_steps(n, kind, grad_scale, guard_scale, betas=(0.5, 0.999), seed=0):
    """One row of n elements through STEPS, one SINGLE step at a time from inputs every party shares -- yields, per step count, a dict of
      p, g, m, v      the float32 inputs: p = 0 exactly (kind 'zero': the new parameter is then the negated update, with no rounding of
                      a large parameter on top) or randn (kind 'randn'); g = gradients(); m = v = 0 at step 1, afterwards the twin's
                      moments of the previous step of this row
      ref, twin       (p, m, v, update) of adam64 / adam32_twin for this one step
    guard_scale: None (an unguarded entry point) or guard[0]; the truth multiplies g by grad_scale * float32(guard_scale).
    An element's gradient keeps its sign from step to step.  If it did not, an element whose g comes close to -m b1 / (1 - b1) would
    cancel in m: its relative error is unbounded for kernel and twin alike, the row's worst relative error would be whatever that one
    element happens to give on either side, and a real error elsewhere in the row would hide under it (docs/optimizer_parity.md)."""
    rng = np.random.RandomState(977 * seed + 13 * (n % 100003) + 5)
    m, v = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    guard = None if guard_scale is None else (np.float32(guard_scale), 0.0)
    for k, step in enumerate(STEPS):
        g = gradients(n, 1000003 * seed + 7919 * k + n, sign_seed=31 * n + seed)
        p = np.zeros(n, dtype=np.float32) if kind == 'zero' else rng.standard_normal(n).astype(np.float32)
        args = ([g], m, v, step - 1, LR, betas, EPS, grad_scale, guard)
        pr, mr, vr, ur, sr = adam64(p, *args)
        pt, mt, vt, ut, st_ = adam32_twin(p, *args)
        assert sr == st_ == step
        yield dict(step=step, p=p, g=g, m=m, v=v, ref=(pr, mr, vr, ur[0]), twin=(pt, mt, vt, ut[0]))
        m, v = mt, vt


def limits(case):
    """The device bounds of one step of a row, from the reference and its twin alone:
      m, v, update: 4 x the twin's worst relative error over the row (the factor allows for FMA contraction and a last-place difference
                    in divide and sqrt)
      p (absolute, per element): 2^-24 |p_ref| (the final rounding of p) + 4 x the twin's largest absolute update error on the row"""
    (pr, mr, vr, ur), (pt, mt, vt, ut) = case['ref'], case['twin']
    return dict(m=4.0 * worst_rel(mt, mr), v=4.0 * worst_rel(vt, vr), update=4.0 * worst_rel(ut, ur),
                p=2.0 ** -24 * np.abs(pr) + 4.0 * float(np.max(np.abs(ut.astype(np.float64) - ur))))


def check_step(case, p, m, v, what=''):
    """Hold one step's device results (float32 arrays) to the bounds; -> the kernel-to-twin ratios {m, v, update} (update: only on
    p = 0 rows; a ratio is 0/0 = 0 where twin and device are both exact)."""
    (pr, mr, vr, ur) = case['ref']
    (pt, mt, vt, ut) = case['twin']
    lim = limits(case)
    assert zeros_agree(m, mr) and zeros_agree(v, vr), '%s: a moment is not 0 where the truth is exactly 0' % what
    got = {'m': worst_rel(m, mr), 'v': worst_rel(v, vr)}
    zero_row = not case['p'].any()
    if zero_row:
        upd = -p.astype(np.float64)                 # (0 - u: exact)
        assert zeros_agree(upd, ur), '%s: the update is not 0 where the truth is exactly 0' % what
        got['update'] = worst_rel(upd, ur)
    for k, e in got.items():
        assert e <= lim[k], '%s step %d: %s is off by %.3e relative, the limit (4 x twin) is %.3e' % (what, case['step'], k, e, lim[k])
    err = np.abs(p.astype(np.float64) - pr)
    assert (err <= lim['p']).all(), '%s step %d: p is off by %.3e at element %d (limit %.3e)' % (
        what, case['step'], err.max(), int(np.argmax(err - lim['p'])), float(lim['p'][np.argmax(err - lim['p'])]))
    return {k: (e / (lim[k] / 4.0) if lim[k] > 0 else (0.0 if e == 0 else float('inf'))) for k, e in got.items()}


# a ParamTree whose layout exercises the table builder (hoig_amd/nn.py: _build_plane_table, _build_plain_chunks); 'up.weight' is transposed
TREE_SHAPES = [
    ('a.weight', (64, 32, 3, 3)),             # a packed weight at offset 0: forward planes only (flag 1)
    ('b.weight', (32, 64, 3, 3)),             # ... back to back with a second one: data-gradient planes only (flag 2)
    ('c.weight', (64, 64, 1, 1)),             # ... and a third: both (flag 3)
    ('d.weight', (1024,)),                    # a plain run of exactly one chunk
    ('up.weight', (64, 96, 3, 3)),            # ConvTranspose: (Ci, Co, R, S), stored [Co][R][S][Ci]
    ('f.weight', (3, 64, 7, 7)),              # plain, longer than a chunk
    ('f.bias', (3,)),                         # numel % 4 = 3, 1, 2: alignment gaps
    ('g.weight', (5,)),
    ('g.bias', (6,)),
    ('s.mlp_gamma.weight', (32, 128, 3, 3)),  # gamma | beta: one fused (64, 128, 3, 3) row
    ('s.mlp_gamma.bias', (32,)),
    ('s.mlp_beta.weight', (32, 128, 3, 3)),
    ('s.mlp_beta.bias', (32,)),
    ('z.bias', (7,)),                         # a plain tail at the end of the buffer
]
TREE_TRANSPOSED = ('up.weight',)


def worst_rel(x, ref):
    """max_i |x_i - ref_i| / |ref_i| over the elements whose reference is not 0 (0.0 if there is none), in float64."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    nz = ref != 0
    return float(np.max(np.abs(x[nz] - ref[nz]) / np.abs(ref[nz]))) if nz.any() else 0.0


def zeros_agree(x, ref):
    """Where the reference is exactly 0, x is exactly 0 (either sign)."""
    x, ref = np.asarray(x), np.asarray(ref)
    return bool((x[ref == 0] == 0).all())
