// Gradient guard (docs/grad_guard.md): the per-lane code that the kernels of grad_guard.hip and the CPU twins of grad_guard_host.cpp
// share, the order of every sum, and the workspace layout.  Both files are built with -ffp-contract=off.
//
// Statistics of x[0 .. n): sum of squares and max |x| over the finite elements, and the number of non-finite ones, for the whole
// buffer and for every row {first, count} of a sorted table.  Squares and sums are fp64 (the square of an fp32 value is exact there), so
// a result depends on the order of its additions only, and that order is a function of (n, table):
//   stage 1, chunk c = elements [c * GG_CHUNK, ..): thread t of 256 takes the four-element slots t, t + 256, .. of the chunk, element by
//     element; the 64 lanes of a wave meet in a butterfly (offsets 32 .. 1), the four waves are added in order 0, 1, 2, 3.  That is the
//     chunk's partial -- it never looks at the table.  Then, for every table row that meets the chunk, the piece (row ∩ chunk): a piece
//     that IS the chunk takes the chunk's partial; any other piece is made by one wave, lane l taking elements l, l + 64, .. of the
//     piece, then the butterfly.  The piece of (chunk c, row s) lives in slot c + s (rows are sorted and disjoint, so the slots of
//     consecutive pieces rise strictly and those of one row are adjacent);
//   stage 2, one workgroup of 1024 per result: thread t joins the partials t, t + 1024, .. in order, butterfly, the 16 waves in order.
// No floating-point atomics, no workgroup waits for another, and neither the grid size nor arrival order enters.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "hoig_kernels.h"

#if defined(__HIPCC__)
#define GG_HD __host__ __device__
#else
#define GG_HD
#endif

#define GG_CHUNK HOIG_GRAD_CHUNK  // elements of a stage-1 chunk
#define GG_WAVE 64
#define GG_NT 256                 // stage 1: four waves
#define GG_SLOTS (GG_CHUNK / (4 * GG_NT))
#define GG_NT2 1024               // stage 2: sixteen waves
#define GG_MAX_GRID 1024          // stage 1 walks the chunks with at most this many workgroups

struct gg_acc {
    double s, mx, nf;             // sum x^2 and max |x| over the finite elements; the number of non-finite ones
};

GG_HD inline gg_acc gg_zero() { return gg_acc{0.0, 0.0, 0.0}; }

GG_HD inline void gg_take(gg_acc &a, float x) {
    uint32_t bits;
    memcpy(&bits, &x, 4);
    if ((bits & 0x7f800000u) == 0x7f800000u) {
        a.nf = a.nf + 1.0;
        return;
    }
    const double d = (double)x, ad = fabs(d);
    a.s = a.s + d * d;
    if (ad > a.mx) a.mx = ad;
}

GG_HD inline gg_acc gg_join(const gg_acc &a, const gg_acc &b) { return gg_acc{a.s + b.s, a.mx > b.mx ? a.mx : b.mx, a.nf + b.nf}; }

GG_HD inline int64_t gg_chunks(int64_t n) { return (n + GG_CHUNK - 1) / GG_CHUNK; }

// thread t's share of the chunk x[base .. base + cnt): its slots in order, each slot's elements in order
GG_HD inline gg_acc gg_thread_chunk(const float *x, int64_t base, int cnt, int t) {
    gg_acc a = gg_zero();
    for (int j = 0; j < GG_SLOTS; ++j) {
        const int e = 4 * (t + GG_NT * j);
        for (int k = 0; k < 4 && e + k < cnt; ++k) gg_take(a, x[base + e + k]);
    }
    return a;
}

// lane l's share of the piece x[b .. e)
GG_HD inline gg_acc gg_lane_piece(const float *x, int64_t b, int64_t e, int lane) {
    gg_acc a = gg_zero();
    for (int64_t i = b + lane; i < e; i += GG_WAVE) gg_take(a, x[i]);
    return a;
}

// stage 2: thread t's share of the partials [first, last) (three doubles each)
GG_HD inline gg_acc gg_thread_parts(const double *parts, int64_t first, int64_t last, int t) {
    gg_acc a = gg_zero();
    for (int64_t i = first + t; i < last; i += GG_NT2) a = gg_join(a, gg_acc{parts[3 * i], parts[3 * i + 1], parts[3 * i + 2]});
    return a;
}

// row s of the table -> its piece slots [first, last) of stage 1
GG_HD inline void gg_row_slots(const int64_t *segs, int s, int64_t nchunk, int64_t *first, int64_t *last) {
    int64_t c0 = segs[2 * s] / GG_CHUNK, c1 = (segs[2 * s] + segs[2 * s + 1] - 1) / GG_CHUNK;
    if (c0 < 0) c0 = 0;
    if (c1 > nchunk - 1) c1 = nchunk - 1;
    *first = c0 + s, *last = c1 + s + 1;
}

// the first row that ends behind element `at` (nseg if none)
GG_HD inline int gg_first_row(const int64_t *segs, int nseg, int64_t at) {
    int lo = 0, hi = nseg;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (segs[2 * mid] + segs[2 * mid + 1] > at) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the workspace: chunk partials [nchunk][3], then piece slots [nchunk + nseg][3], doubles
inline int64_t gg_workspace_bytes(int64_t n, int nseg) {
    if (n <= 0 || nseg < 0) return HOIG_EINVAL;
    return (2 * gg_chunks(n) + nseg) * 3 * (int64_t)sizeof(double);
}

// rows inside [0, n), count >= 1, sorted, disjoint (gaps allowed)
inline bool gg_table_ok(int64_t n, const int64_t *segs, int nseg) {
    if (n <= 0 || nseg < 0 || (nseg > 0 && !segs)) return false;
    int64_t at = 0;
    for (int s = 0; s < nseg; ++s) {
        const int64_t f = segs[2 * s], c = segs[2 * s + 1];
        if (f < at || c < 1 || f >= n || c > n - f) return false;
        at = f + c;
    }
    return true;
}

// The decision (one thread on the device): total = the three statistics of the whole buffer, guard = {scale, skip}, record = seven
// doubles {steps seen, skipped, clipped, last norm, last max |x|, last non-finite count, largest finite norm}.
GG_HD inline void gg_decide(const double *total, double pre_scale, double max_norm, int flags, float *guard, double *record) {
    const double norm = pre_scale * sqrt(total[0]), nonfinite = total[2];
    const bool skip = nonfinite > 0.0 && (flags & HOIG_GUARD_SKIP);
    float scale = 1.0f;
    bool clipped = false;
    // a watched step with non-finite entries goes through as an unguarded one does: no coefficient from the finite rest
    if (max_norm > 0.0 && nonfinite == 0.0 && norm > max_norm) {
        scale = (float)(max_norm / (norm + 1e-6));
        clipped = true;
    }
    guard[0] = scale;
    guard[1] = skip ? 1.0f : 0.0f;
    record[0] = record[0] + 1.0;
    if (skip) record[1] = record[1] + 1.0;
    if (clipped) record[2] = record[2] + 1.0;
    record[3] = norm;
    record[4] = pre_scale * total[1];
    record[5] = nonfinite;
    if (norm - norm == 0.0 && norm > record[6]) record[6] = norm;
}
