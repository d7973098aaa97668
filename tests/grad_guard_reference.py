"""Truths, limits and the checks themselves for the gradient guard's statistics and decision (hoig_amd/csrc/grad_guard.*,
docs/grad_guard.md): tests/test_grad_guard_cpu.py runs every check through the CPU twins (device 'cpu'),
tests/test_grad_guard_gpu.py through the kernels (device 'cuda') -- the same cases, truths and limits.

Where the limit on the sum of squares comes from (u = 2^-53): the square of an fp32 value is exact in fp64, so the only roundings are
those of the additions, and every term is >= 0.  A sum whose longest chain of additions has L links is within L u / (1 - L u) of the
exact sum, relatively.  Every result is held to ITS OWN chain (chain(), below, from the constants of grad_guard.h): `total` to a
chunk's chain plus the second stage over all chunks, a row to the chains of the pieces it is made of plus the second stage over its
own pieces -- 25 + ceil(P / 1024) + 22 links for `total` over P chunks.
max |x| and the counts are exact, and compared with ==.
"""
import ctypes
import math

import numpy as np
import torch

from hoig_amd import _lib as L

U = 2.0 ** -53
CH = L.GRAD_CHUNK                 # elements of a stage-1 chunk: from the binding, so the cases follow the kernel
GRID = L.GRAD_MAX_GRID            # workgroups of one stage-1 round
NT, NT2, WAVE = 256, 1024, 64     # threads of a stage-1 / stage-2 workgroup (grad_guard.h)
INF, NAN = float('inf'), float('nan')

SIZES = [1, 3, 4, 255, 256, 257, CH - 1, CH, CH + 1, 3 * CH + 5]
BIG = (GRID + 37) * CH + 3        # more chunks than one round of workgroups


def chain(n, a=0, b=None, whole=True):
    """The longest chain of additions behind ONE result: `total` of a buffer of n elements (whole=True), or the row x[a:b].
    Stage 1: a chunk's partial has CH / NT additions in a thread, 6 in the butterfly and NT / 64 - 1 across the waves; a row takes
    it for every chunk it covers entirely, and for any other piece ceil(len / 64) additions in a lane and 6 in the butterfly.
    Stage 2: ceil(P / NT2) additions in a thread for the result's own P partials, 6 in the butterfly, NT2 / 64 - 1 across the waves.
    One more rounding for the truth (math.fsum rounds once)."""
    chunk = CH // NT + 6 + NT // WAVE - 1
    if whole:
        parts, stage1 = -(-n // CH), chunk
    else:
        c0, c1 = a // CH, (b - 1) // CH
        parts, stage1 = c1 - c0 + 1, 0
        for c in (c0, c1):          # (the chunks between the two are covered entirely)
            lo, hi = max(a, c * CH), min(b, min(n, (c + 1) * CH))
            entire = lo == c * CH and hi == min(n, (c + 1) * CH)
            stage1 = max(stage1, chunk if entire else -(-(hi - lo) // WAVE) + 6)
        if c1 - c0 >= 2:
            stage1 = max(stage1, chunk)
    return stage1 + -(-parts // NT2) + 6 + NT2 // WAVE - 1 + 1


def limit(n, a=0, b=None, whole=True):
    links = chain(n, a, b, whole)
    return links * U / (1.0 - links * U)


# ------------------------------------------------------------------------------------------------ tables
def tables(n):
    """name -> [[first, count], ..] for a buffer of n elements: every kind the size admits."""
    out = {'empty': [], 'whole': [[0, n]]}
    if n <= 257:
        out['ones'] = [[i, 1] for i in range(n)]
    if n >= 3:           # rows that start off a multiple of 4, gaps between them, the last row ends at n
        rows, at, k = [], 1, 0
        while at < n:
            cnt = min([2, 5, 1, 67, 3, 1030][k % 6], n - at)
            rows.append([at, cnt])
            at += cnt + [1, 2, 4, 7][k % 4]
            k += 1
            if at % 4 == 0:
                at += 1
            if len(rows) == 40:
                break
        if rows[-1][0] + rows[-1][1] < n:
            at = rows[-1][0] + rows[-1][1] + 1
            if at % 4 == 0:
                at += 1
            if at < n:
                rows.append([at, n - at])
            else:
                rows[-1][1] = n - rows[-1][0]
        out['odd_gaps_last'] = rows
    if n > CH:           # rows across chunk boundaries: a short one, one that ends with its chunk, one that is a chunk, the rest
        out['straddle'] = [[CH - 3, min(5, n - CH + 3)]]
        if n >= 3 * CH + 5:
            out['straddle'] = [[CH - 3, 5], [CH + 2, CH - 2], [2 * CH, CH], [3 * CH, n - 3 * CH]]
    if n == BIG:         # (one table with every kind of row: the truth of 4 M elements is the slow part of a case)
        out = {'empty': [], 'big_rows': [[0, 64], [64, 7 * CH + 1], [7 * CH + 68, 1], [8 * CH, (GRID + 20) * CH],
                                         [(GRID + 28) * CH + 1, n - (GRID + 28) * CH - 1]]}
    return out


# the shapes of tests/test_ops_gpu.py::test_fused_adam_with_planes_matches_the_two_launches and ::test_fused_adam_matches_torch
ADAM_SHAPES = {'s.weight': (64, 8, 7, 7), 's.bias': (64,), 'a.weight': (128, 64, 3, 3), 'a.bias': (128,), 'b.weight': (32, 96, 3, 3),
               'h.weight': (3, 64, 7, 7), 'h.bias': (3,), 'c.weight': (64, 32, 5, 5), 'd.weight': (96, 160, 1, 1), 'n.weight': (96,)}
SMALL_SHAPES = {'a.weight': (8, 4, 3, 3), 'a.bias': (8,), 'b.weight': (5,), 'b.bias': (5,)}


def tree_table(shapes=ADAM_SHAPES):
    """(n, rows) of a ParamTree over `shapes`, as GradGuard builds them (the tree pads every parameter to 4 elements: gaps)."""
    from hoig_amd.nn import ParamTree
    from hoig_amd.guard import _numel
    tree = ParamTree(shapes, torch.device('cpu'))
    rows = sorted([off, _numel(tree._internal[name][0])] for name, off in tree._offsets.items())
    return tree.flat.numel(), rows


def cases():
    """(id, n, table name) of every statistics case."""
    out = [('%d-%s' % (n, t), n, t) for n in SIZES + [BIG] for t in tables(n)]
    return out + [('tree-own', 'tree', 'own')]


def case_table(n, tname):
    if n == 'tree':
        return tree_table()
    return n, tables(n)[tname]


def values(n, rows, seed, nonfinite):
    """Seeded normal values, every row (and the rest) scaled by its own power of ten between 1e-30 and 1e30: squares taken in fp32 would
    overflow.  nonfinite: +Inf, -Inf and NaN at element 0, at element n - 1, inside the n % 4 tail, in a one-element row and in a gap,
    wherever the case has such a place."""
    rng = np.random.RandomState(seed)
    x = rng.standard_normal(n) * 10.0 ** rng.randint(-30, 31)
    for f, c in rows:
        x[f:f + c] = rng.standard_normal(c) * 10.0 ** rng.randint(-30, 31)
    x = x.astype(np.float32)
    assert np.isfinite(x).all()
    if nonfinite:
        covered = np.zeros(n, dtype=bool)
        for f, c in rows:
            covered[f:f + c] = True
        x[0] = INF
        x[n - 1] = -INF if n > 1 else INF
        if n % 4 and n > 4:
            x[n - (n % 4)] = NAN
        ones = [f for f, c in rows if c == 1]
        if ones:
            x[ones[len(ones) // 2]] = NAN
        gaps = np.flatnonzero(~covered)
        if len(gaps):
            x[gaps[len(gaps) // 2]] = -INF
        if n > CH + 1:
            x[CH] = NAN             # the first element of the second chunk
    return x


def truth(x, a, b):
    """{sum x^2, max |x|, non-finite count} of x[a:b], the sum exactly rounded."""
    v = x[a:b].astype(np.float64)
    fin = np.isfinite(v)
    f = v[fin]
    return math.fsum((f * f).tolist()), float(np.abs(f).max()) if len(f) else 0.0, float((~fin).sum())


# ------------------------------------------------------------------------------------------------ running it
def _cp(a):
    return ctypes.c_void_p(a.ctypes.data)


def _tp(t):
    return ctypes.c_void_p(t.data_ptr())


SENTINEL = -7.25


def run_stats(dev, x, rows, n=None):
    """hoig_grad_stats (dev 'cuda') or its twin ('cpu') -> (return code, total [3], seg_out [nseg][3]); the outputs start as SENTINEL.
    n: what the call is told instead of len(x) (the refusal cases)."""
    n = len(x) if n is None else n
    nseg = len(rows)
    segs = np.ascontiguousarray(np.array(rows if nseg else [[0, 0]], dtype=np.int64))
    total = np.full(3, SENTINEL)
    seg_out = np.full((max(nseg, 1), 3), SENTINEL)
    nbytes = L.lib.hoig_grad_stats_workspace_bytes(max(len(x), 1), nseg)
    assert nbytes > 0 and nbytes % 8 == 0
    if dev == 'cpu':
        ws = np.zeros(nbytes // 8)
        rc = L.lib.hoig_grad_stats_host(_cp(x), n, _cp(segs), nseg, _cp(seg_out), _cp(total), _cp(ws))
        return rc, total, seg_out[:nseg]
    xd = torch.from_numpy(x).cuda()
    sd = torch.from_numpy(segs).cuda()
    td, od = torch.from_numpy(total).cuda(), torch.from_numpy(seg_out).cuda()
    ws = torch.zeros(nbytes // 8, dtype=torch.float64, device='cuda')
    rc = L.lib.hoig_grad_stats(_tp(xd), n, _cp(segs), _tp(sd), nseg, _tp(od), _tp(td), _tp(ws),
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, td.cpu().numpy(), od.cpu().numpy()[:nseg]


def check_stats(dev, n, tname, nonfinite):
    n, rows = case_table(n, tname)
    x = values(n, rows, seed=n % 1000 + 7 * len(rows) + (1 if nonfinite else 0), nonfinite=nonfinite)
    rc, total, seg = run_stats(dev, x, rows)
    assert rc == L.OK
    worst = (0.0, 0.0, 0)
    for got, (a, b), whole in [(total, (0, n), True)] + [(seg[i], (f, f + c), False) for i, (f, c) in enumerate(rows)]:
        ss, mx, nf = truth(x, a, b)
        lim = limit(n, a, b, whole)
        err = abs(got[0] - ss) / ss if ss > 0 else abs(got[0])
        worst = max(worst, (err / lim, err, chain(n, a, b, whole)))
        assert np.isfinite(got[0]) and err <= lim, (a, b, got[0], ss, err, lim)
        assert got[1] == mx and got[2] == nf, (a, b, got, mx, nf)
    print('grad_stats %s n=%d rows=%d nonfinite=%d: the result nearest its limit: relative error %.2e = %.2f of the limit (chain %d)'
          % (dev, n, len(rows), nonfinite, worst[1], worst[0], worst[2]))
    if nonfinite:
        assert total[2] >= 1 and (n < 2 or total[2] >= 2)
    # `total` does not depend on the table: bit for bit what the call without one gives
    if rows:
        rc0, total0, _ = run_stats(dev, x, [])
        assert rc0 == L.OK and total0.tobytes() == total.tobytes()
    return x, rows, total, seg


def check_device_equals_twin(n, tname, nonfinite):
    """The kernels' outputs are the twin's, bit for bit, and a second run of the kernels gives the first one's."""
    n, rows = case_table(n, tname)
    x = values(n, rows, seed=n % 1000 + 7 * len(rows) + (1 if nonfinite else 0), nonfinite=nonfinite)
    rc_c, tot_c, seg_c = run_stats('cpu', x, rows)
    rc_d, tot_d, seg_d = run_stats('cuda', x, rows)
    rc_e, tot_e, seg_e = run_stats('cuda', x, rows)
    assert rc_c == rc_d == rc_e == L.OK
    assert tot_c.tobytes() == tot_d.tobytes() == tot_e.tobytes()
    assert seg_c.tobytes() == seg_d.tobytes() == seg_e.tobytes()


def check_misaligned(dev):
    """A buffer that starts 4 bytes off a 16-byte boundary: the same sums as the aligned copy (the order does not depend on alignment)."""
    n = 3 * CH + 5
    rows = tables(n)['straddle']
    x = values(n, rows, seed=5, nonfinite=False)
    want = run_stats(dev, x, rows)
    if dev == 'cpu':
        buf = np.zeros(n + 1, dtype=np.float32)
        buf[1:] = x
        got = run_stats(dev, buf[1:], rows)
    else:
        segs = np.array(rows, dtype=np.int64)
        xd = torch.zeros(n + 1, dtype=torch.float32, device='cuda')
        xd[1:].copy_(torch.from_numpy(x))
        sd = torch.from_numpy(segs).cuda()
        td = torch.zeros(3, dtype=torch.float64, device='cuda')
        od = torch.zeros(len(rows), 3, dtype=torch.float64, device='cuda')
        ws = torch.zeros(L.lib.hoig_grad_stats_workspace_bytes(n, len(rows)) // 8, dtype=torch.float64, device='cuda')
        rc = L.lib.hoig_grad_stats(ctypes.c_void_p(xd.data_ptr() + 4), n, _cp(segs), _tp(sd), len(rows), _tp(od), _tp(td), _tp(ws),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        got = (rc, td.cpu().numpy(), od.cpu().numpy())
    assert got[0] == want[0] == L.OK
    assert got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()


REFUSED = {'n_zero': (0, [[0, 1]]), 'n_negative': (-5, []), 'unsorted': (100, [[50, 10], [10, 10]]),
           'overlapping': (100, [[10, 20], [29, 5]]), 'past_the_end': (100, [[90, 11]]), 'first_past_the_end': (100, [[100, 1]]),
           'negative_first': (100, [[-1, 4]]), 'empty_row': (100, [[10, 0]])}


def check_refused(dev, name):
    n, rows = REFUSED[name]
    x = np.ones(128, dtype=np.float32)
    rc, total, seg = run_stats(dev, x, rows, n=n)
    assert rc == L.EINVAL
    assert (total == SENTINEL).all() and (seg == SENTINEL).all()
    assert L.lib.hoig_grad_stats_workspace_bytes(0, 0) < 0 and L.lib.hoig_grad_stats_workspace_bytes(10, -1) < 0


# ------------------------------------------------------------------------------------------------ the decision
def decide_model(total, pre_scale, max_norm, flags, record):
    """hoig_guard_decide in Python floats (IEEE doubles; math.sqrt is correctly rounded) -> guard (two fp32 values); updates record."""
    norm = pre_scale * math.sqrt(total[0])
    nonfinite = total[2]
    skip = nonfinite > 0 and bool(flags & L.GUARD_SKIP)
    scale, clipped = np.float32(1.0), False
    if max_norm > 0 and nonfinite == 0 and norm > max_norm:
        scale, clipped = np.float32(max_norm / (norm + 1e-6)), True
    record[0] += 1.0
    record[1] += 1.0 if skip else 0.0
    record[2] += 1.0 if clipped else 0.0
    record[3], record[4], record[5] = norm, pre_scale * total[1], nonfinite
    if math.isfinite(norm) and norm > record[6]:
        record[6] = norm
    return np.array([scale, 1.0 if skip else 0.0], dtype=np.float32)


def run_decide(dev, total, pre_scale, max_norm, flags, guard, record):
    """One call on the twin (numpy arrays, in place) or on the device (torch tensors, in place)."""
    if dev == 'cpu':
        return L.lib.hoig_guard_decide_host(_cp(total), pre_scale, max_norm, flags, _cp(guard), _cp(record))
    return L.lib.hoig_guard_decide(_tp(total), pre_scale, max_norm, flags, _tp(guard), _tp(record),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def decide_sequence():
    """Six calls on one record: watch on a clean and on a non-finite gradient, skip on a non-finite one, then clipping with max_norm
    just below the norm (fires) and just above it (does not), and a clip under watch.  -> [(total, pre_scale, max_norm, flags)]"""
    clean = np.array([1.2345678e7, 431.5, 0.0])
    bad = np.array([9.87e-3, 0.07, 3.0])
    big = np.array([3.3e61, 4.1e30, 0.0])
    norm = 0.125 * math.sqrt(big[0])
    return [(clean, 1.0, 0.0, 0), (bad, 0.5, 2.0, 0), (bad, 0.5, 1e-3, L.GUARD_SKIP),
            (big, 0.125, float(np.nextafter(norm, 0.0)), L.GUARD_SKIP), (big, 0.125, float(np.nextafter(norm, INF)), L.GUARD_SKIP),
            (clean, 1.0, 100.0, 0)]


def check_decide(dev):
    """The entry point against the formula, ==, call by call; `dev` 'cuda' also against the twin."""
    rec_m = np.zeros(7)
    rec_t = np.zeros(7)
    guard_t = np.zeros(2, dtype=np.float32)
    if dev == 'cuda':
        rec_d = torch.zeros(7, dtype=torch.float64, device='cuda')
        guard_d = torch.zeros(2, dtype=torch.float32, device='cuda')
    fired = []
    for total, pre, mx, flags in decide_sequence():
        before = rec_t[2]
        want = decide_model(total, pre, mx, flags, rec_m)
        assert run_decide('cpu', total, pre, mx, flags, guard_t, rec_t) == L.OK
        assert guard_t.tobytes() == want.tobytes() and rec_t.tobytes() == rec_m.tobytes(), (guard_t, want, rec_t, rec_m)
        if dev == 'cuda':
            assert run_decide('cuda', torch.from_numpy(total).cuda(), pre, mx, flags, guard_d, rec_d) == L.OK
            torch.cuda.synchronize()
            assert guard_d.cpu().numpy().tobytes() == guard_t.tobytes() and rec_d.cpu().numpy().tobytes() == rec_t.tobytes()
        fired.append((rec_t[2] > before, float(guard_t[1]) != 0.0))     # (a coefficient just below 1 rounds to 1.0f: ask the counter)
    # what the sequence is there to show: (clipped, skipped) per call, then the counters
    assert fired == [(False, False), (False, False), (False, True), (True, False), (False, False), (True, False)]
    assert rec_t[:3].tolist() == [6.0, 1.0, 2.0] and rec_t[5] == 0.0
    assert rec_t[6] == 0.125 * math.sqrt(3.3e61)
    # refused arguments leave guard and record as they are -- on the twin, and on the device's entry point when that is under test
    for total, pre, mx, flags in ((np.zeros(3), 1.0, 0.0, 2), (np.zeros(3), 0.0, 0.0, 0), (np.zeros(3), 1.0, -1.0, 0), (np.zeros(3), 1.0, NAN, 0)):
        g, bad = np.full(2, SENTINEL, dtype=np.float32), np.zeros(7)
        assert run_decide('cpu', total, pre, mx, flags, g, bad) == L.EINVAL
        assert (g == SENTINEL).all() and (bad == 0).all()
        if dev == 'cuda':
            gd, bd = torch.from_numpy(g).cuda(), torch.from_numpy(bad).cuda()
            assert run_decide('cuda', torch.from_numpy(total).cuda(), pre, mx, flags, gd, bd) == L.EINVAL
            torch.cuda.synchronize()
            assert (gd.cpu().numpy() == SENTINEL).all() and (bd.cpu().numpy() == 0).all()
