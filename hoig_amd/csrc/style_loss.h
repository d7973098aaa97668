// The opt-in style (Gram-matrix) term of G (docs/style_loss.md): the argument checks, the layout of the workspace, the enumeration of
// the tile pairs, the per-entry code of the finishing pass and the last sums, shared by the kernels of style_loss.hip and the CPU twin
// of style_loss_host.cpp.  Both files are built with -ffp-contract=off.  The Gram partials and the feature gradient are k-ordered fmaf
// chains from +0 (the fp32 MFMA on the device, std::fmaf in the twin); everything after them is +, -, *, comparison, conversion and
// double division, in one order on either side.
#pragma once
#include <stdint.h>

#include "hoig_kernels.h"

#if defined(__HIPCC__)
#define ST_HD __host__ __device__
#else
#define ST_HD
#endif

constexpr int ST_T = HOIG_STYLE_TILE;            // edge of a Gram tile and columns of a gradient tile: 2 x 2 MFMA blocks of 32 x 32
constexpr int ST_K = HOIG_STYLE_CHUNK;           // pixels of one Gram partial: the longest fmaf chain of the Gram pass
constexpr int ST_NT = 256;                       // threads of a workgroup: four waves, one 32 x 32 block each
constexpr int ST_EPT = ST_T * ST_T / ST_NT;      // tile entries per thread of the finishing pass: t, t + 256, ...
constexpr int ST_ROWS = 64;                      // pixels of a gradient tile
static_assert(ST_T == 64 && ST_K % 2 == 0 && ST_EPT * ST_NT == ST_T * ST_T, "tile sizes");

struct st_args {
    const float *fx, *fy;
    int N, P, C;
    int tiles, pairs, chunks;            // tiles of ST_T channels, tile pairs tj >= ti, pixel chunks
    double scale, cp;                    // cp = (double)C * (double)P
    float c;                             // (float)(2 scale / (N C^3 P)): the magnitude of every non-zero entry of S
    float *S, *term, *report;            // term, report: fp32 slots that are ADDED to, or null
    double *gram;                        // [2N][C][C], or null
};

inline bool st_sizes_ok(int N, int P, int C) {
    return N >= 1 && N <= HOIG_STYLE_MAX_N && P >= 1 && P <= HOIG_STYLE_MAX_P && C >= 16 && C <= HOIG_STYLE_MAX_C && C % 16 == 0;
}
inline int st_tiles(int C) { return (C + ST_T - 1) / ST_T; }
inline int st_pairs(int C) { return st_tiles(C) * (st_tiles(C) + 1) / 2; }
inline int st_chunks(int P) { return (P + ST_K - 1) / ST_K; }

// ---- the workspace: [partials fp32 [2N][pairs][chunks][ST_T][ST_T] | sums fp64 [N][pairs]]
inline int64_t st_off_sums(int N, int P, int C) { return (int64_t)2 * N * st_pairs(C) * st_chunks(P) * ST_T * ST_T * 4; }
inline int64_t st_workspace_bytes(int N, int P, int C) {
    if (!st_sizes_ok(N, P, C)) return -1;
    return st_off_sums(N, P, C) + (int64_t)N * st_pairs(C) * 8;
}

inline bool st_finite(double x) { return x - x == 0.0; }
inline bool st_al(const void *p, int a, bool may_be_null) { return p ? !((uintptr_t)p & (uintptr_t)(a - 1)) : may_be_null; }
inline bool st_overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y ? y - x < (uintptr_t)na : x - y < (uintptr_t)nb;
}

// the Gram entry point's arguments -> st_args; HOIG_OK, HOIG_EUNSUPPORTED (sizes) or HOIG_EINVAL (everything else)
inline int st_pack(const float *fx, const float *fy, int N, int P, int C, double scale, float *S, float *term, float *report, double *gram,
                   st_args *a) {
    if (N < 1 || P < 1 || C < 1) return HOIG_EINVAL;
    if (!st_sizes_ok(N, P, C)) return HOIG_EUNSUPPORTED;
    if (!st_finite(scale) || scale < 0.0) return HOIG_EINVAL;
    if (!st_al(fx, 16, false) || !st_al(fy, 16, false) || !st_al(S, 16, false) || !st_al(gram, 16, true) || !st_al(term, 4, true) ||
        !st_al(report, 4, true))
        return HOIG_EINVAL;
    const int64_t nf = (int64_t)N * P * C * 4, ns = (int64_t)N * C * C * 4, ng = (int64_t)2 * N * C * C * 8;
    if (st_overlap(S, ns, fx, nf) || st_overlap(S, ns, fy, nf) || st_overlap(gram, ng, fx, nf) || st_overlap(gram, ng, fy, nf) ||
        st_overlap(gram, ng, S, ns))
        return HOIG_EINVAL;
    a->fx = fx, a->fy = fy, a->N = N, a->P = P, a->C = C;
    a->tiles = st_tiles(C), a->pairs = st_pairs(C), a->chunks = st_chunks(P);
    a->scale = scale, a->cp = (double)C * (double)P;
    a->c = (float)(2.0 * scale / ((double)N * (double)C * (double)C * (double)C * (double)P));
    a->S = S, a->term = term, a->report = report, a->gram = gram;
    return HOIG_OK;
}

// the gradient entry point's checks
inline int st_check_dfeat(const float *fx, const float *S, int N, int P, int C, const float *dfx) {
    if (N < 1 || P < 1 || C < 1) return HOIG_EINVAL;
    if (!st_sizes_ok(N, P, C)) return HOIG_EUNSUPPORTED;
    if (!st_al(fx, 16, false) || !st_al(S, 16, false) || !st_al(dfx, 16, false)) return HOIG_EINVAL;
    const int64_t nf = (int64_t)N * P * C * 4, ns = (int64_t)N * C * C * 4;
    if (st_overlap(dfx, nf, fx, nf) || st_overlap(dfx, nf, S, ns)) return HOIG_EINVAL;
    return HOIG_OK;
}

// pair index -> (ti, tj), tj >= ti: (0,0), (0,1), ..., (0,tiles-1), (1,1), ...
ST_HD inline void st_pair(int tiles, int pair, int *ti, int *tj) {
    int i = 0;
    while (pair >= tiles - i) pair -= tiles - i, ++i;
    *ti = i, *tj = i + pair;
}

// image `img` of the 2N: the x images first, then the y images
ST_HD inline const float *st_image(const st_args &a, int img) {
    return img < a.N ? a.fx + (int64_t)img * a.P * a.C : a.fy + (int64_t)(img - a.N) * a.P * a.C;
}

ST_HD inline const float *st_partial(const st_args &a, const float *partials, int img, int pair) {
    return partials + ((int64_t)img * a.pairs + pair) * a.chunks * (ST_T * ST_T);
}

// ---- the finishing pass, entry e = row ST_T + col of tile pair (ti, tj) of image n: the chunk partials of either side in index order in
// double, the division by C P, d = Gx - Gy, S (and the Gram matrices) at (i, j) and, above the diagonal tile, at (j, i).  Returns |d|;
// +0 for an entry outside the C x C matrix, which changes no bit of a sum that is >= +0 or NaN.  The sign is (d > 0) - (d < 0): 0 for a NaN.
ST_HD inline double st_entry(const st_args &a, const float *partials, int n, int pair, int ti, int tj, int e) {
    const int i = ti * ST_T + e / ST_T, j = tj * ST_T + e % ST_T;
    if (i >= a.C || j >= a.C) return 0.0;
    const float *px = st_partial(a, partials, n, pair) + e, *py = st_partial(a, partials, a.N + n, pair) + e;
    double gx = 0.0, gy = 0.0;
    for (int c = 0; c < a.chunks; ++c) gx += (double)px[(int64_t)c * (ST_T * ST_T)];
    for (int c = 0; c < a.chunks; ++c) gy += (double)py[(int64_t)c * (ST_T * ST_T)];
    gx = gx / a.cp, gy = gy / a.cp;
    const double d = gx - gy;
    const float s = (float)((d > 0.0) - (d < 0.0)) * a.c;
    const int64_t ij = (int64_t)i * a.C + j, ji = (int64_t)j * a.C + i, cc = (int64_t)a.C * a.C;
    a.S[n * cc + ij] = s;
    if (ti != tj) a.S[n * cc + ji] = s;
    if (a.gram) {
        a.gram[n * cc + ij] = gx, a.gram[(a.N + n) * cc + ij] = gy;
        if (ti != tj) a.gram[n * cc + ji] = gx, a.gram[(a.N + n) * cc + ji] = gy;
    }
    return __builtin_fabs(d);
}

// thread t of the workgroup (n, pair): its ST_EPT entries in ascending order
ST_HD inline double st_finish_lane(const st_args &a, const float *partials, int n, int pair, int ti, int tj, int t) {
    double s = 0.0;
    for (int k = 0; k < ST_EPT; ++k) s += st_entry(a, partials, n, pair, ti, tj, t + ST_NT * k);
    return s;
}

// the halving tree over `n` lanes' sums, in place (the twin's form; the kernel's LDS step and its shuffles add the same pairs, as
// gan_loss.h documents it): lane t takes t + n/2, then t + n/4, ..., then t + 1
inline double st_tree(double *acc, int n) {
    for (int s = n / 2; s > 0; s >>= 1)
        for (int t = 0; t < s; ++t) acc[t] = acc[t] + acc[t + s];
    return acc[0];
}

// a tile above the diagonal stands for its mirror image too
ST_HD inline double st_tile_sum(double tree, int ti, int tj) { return ti != tj ? tree + tree : tree; }

// lane t of the one-wave finishing launch: the workgroups' sums t, t + 64, ... in ascending order
ST_HD inline double st_last_lane(const st_args &a, const double *sums, int t) {
    double s = 0.0;
    for (int k = t; k < a.N * a.pairs; k += 64) s += sums[k];
    return s;
}

// one thread: L in double; each value rounded to fp32 where it is added to its slot
ST_HD inline void st_last(const st_args &a, double total) {
    const double L = total / ((double)a.N * (double)a.C * (double)a.C);
    if (a.term) *a.term = *a.term + (float)(a.scale * L);
    if (a.report) *a.report = *a.report + (float)L;
}
