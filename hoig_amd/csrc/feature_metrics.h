// Feature-space metrics in fp64 (docs/feature_metrics.md): KID's polynomial-kernel sums and the k-nearest-neighbour radii and ball
// memberships of precision / recall.  The per-lane code that the kernels of feature_metrics.hip and the CPU twins of
// feature_metrics_host.cpp share, the tile geometry and the workspace layouts.  Both files are built with -ffp-contract=off.
//
// Every kernel is one 64 x 64 tile of P Q^T (rows of row-major fp32 [n][D], widened to fp64, K walked in order) and an epilogue.  A
// workgroup has four waves; wave w owns the 32 x 32 quarter at rows 32 (w >> 1), columns 32 (w & 1) as 2 x 2 MFMA tiles, and value
// (i * 2 + j) * 4 + reg of lane l is the element at
//     row 32 (w >> 1) + 16 i + (l >> 4) + 4 reg,    column 32 (w & 1) + 16 j + (l & 15)
// -- the fp64 result map of v_mfma_f64_16x16x4_f64 (fid_stats.hip).  The twins fill the same 16 values per lane from their own dot
// products and run the same functions on them, so every reduction below is a function of the tile values alone.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fid_stats.h"

#define FM_TILE 64            // rows and columns of a workgroup's tile
#define FM_WAVES 4
#define FM_KMAX 8             // the largest k of hoig_knn_radius_f64: a list holds this many candidates whatever k is
#define FM_CHUNKS 16          // the most column (row) chunks of the radius (hits) grid
#define FM_STATUS_NONFINITE 1 // bits of a status word: a non-finite feature was read
#define FM_STATUS_CLAMPED 2   //                        an index of a gather table was outside its set and was clamped into it
#define FM_TERM_XX 0
#define FM_TERM_YY 1
#define FM_TERM_XY 2

FID_HD inline int fm_tiles(int n) { return (n + FM_TILE - 1) / FM_TILE; }

// the chunking of the radius / hits grids: at least two tiles per chunk, at most FM_CHUNKS chunks
FID_HD inline int fm_chunk_tiles(int tiles) {
    const int t = (tiles + FM_CHUNKS - 1) / FM_CHUNKS;
    return t < 2 ? 2 : t;
}
FID_HD inline int fm_chunks(int tiles) { return (tiles + fm_chunk_tiles(tiles) - 1) / fm_chunk_tiles(tiles); }

FID_HD inline int fm_lane_row(int wave, int lane, int i, int reg) { return 32 * (wave >> 1) + 16 * i + (lane >> 4) + 4 * reg; }
FID_HD inline int fm_lane_col(int wave, int lane, int j) { return 32 * (wave & 1) + 16 * j + (lane & 15); }

// an index of a gather table, clamped into [0, n)
FID_HD inline int fm_clamp_index(int idx, int n, int *clamped) {
    if (idx < 0) {
        *clamped = 1;
        return 0;
    }
    if (idx >= n) {
        *clamped = 1;
        return n - 1;
    }
    return idx;
}

// (gamma dot + coef0)^degree, degree in 1 .. 4, by repeated multiplication from the left
FID_HD inline double fm_poly(double dot, double gamma, double coef0, int degree) {
    const double b = gamma * dot + coef0;
    double p = b;
    for (int d = 1; d < degree; ++d) p = p * b;
    return p;
}

// One lane's share of a KID tile: tile (ti, tj) of term `term`, positions i, j < m of the subset.  xx and yy: the diagonal i == j is
// left out by position and a tile above the diagonal counts twice (its mirror tile does not run).  The 16 values in index order.
FID_HD inline double fm_kid_lane(const double *v, int wave, int lane, int ti, int tj, int term, int m, double gamma, double coef0,
                                 int degree) {
    const bool sym = term != FM_TERM_XY;
    const double weight = (sym && ti != tj) ? 2.0 : 1.0;
    double s = 0.0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 2; ++i)
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < 2; ++j)
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int reg = 0; reg < 4; ++reg) {
                const int row = ti * FM_TILE + fm_lane_row(wave, lane, i, reg), col = tj * FM_TILE + fm_lane_col(wave, lane, j);
                if (row >= m || col >= m || (sym && row == col)) continue;
                s = s + weight * fm_poly(v[(i * 2 + j) * 4 + reg], gamma, coef0, degree);
            }
    return s;
}

// is slot (ti, tj) of a term one that a workgroup fills?
FID_HD inline bool fm_kid_slot_runs(int term, int ti, int tj) { return term == FM_TERM_XY || tj >= ti; }

// One lane's share of a subset's sum over the partials of one term: slots lane, lane + 64, .. in order (those that run).
FID_HD inline double fm_kid_lane_finish(const double *part, int term, int nt, int lane) {
    double s = 0.0;
    for (int e = lane; e < nt * nt; e += FID_WAVE)
        if (fm_kid_slot_runs(term, e / nt, e % nt)) s = s + part[e];
    return s;
}

FID_HD inline double fm_mmd2(double sxx, double syy, double sxy, int m) {
    const double pairs = (double)m * (double)(m - 1), all = (double)m * (double)m;
    return (sxx / pairs + syy / pairs) - (2.0 * sxy) / all;
}

// one lane's share of |x - pivot|^2 of a row: columns lane, lane + 64, .. in order
FID_HD inline double fm_lane_sqnorm(const float *row, int D, const double *pivot, int lane) {
    double s = 0.0;
    for (int c = lane; c < D; c += FID_WAVE) {
        const double v = fid_operand(row, c, 1, pivot, c);
        s = s + v * v;
    }
    return s;
}

// |x|^2 + |y|^2 - 2 x.y, clamped at 0
FID_HD inline double fm_dist2(double nx, double ny, double dot) {
    const double d = (nx + ny) - 2.0 * dot;
    return d > 0.0 ? d : 0.0;          // (a NaN goes to 0 here; the status word reports it)
}

// the FM_KMAX smallest values seen, ascending: v is carried down the list (static indices only: the list stays in registers)
FID_HD inline void fm_insert(double *a, double v) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int s = 0; s < FM_KMAX; ++s)
        if (v < a[s]) {
            const double t = a[s];
            a[s] = v;
            v = t;
        }
}

FID_HD inline double fm_pick(const double *a, int k) {
    double r = a[0];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int s = 1; s < FM_KMAX; ++s)
        if (s == k - 1) r = a[s];
    return r;
}

// ---- workspaces ----
// hoig_kid_poly_f64: partials [S][3][nt * nt] doubles, slot ti * nt + tj, nt = fm_tiles(m) (what hoig_kid_finish_f64 reads)
// hoig_knn_radius_f64: norms [n] doubles, then candidates [chunks][n][FM_KMAX] doubles
// hoig_manifold_hits_f64: norms of X [nx], norms of Y [ny] doubles, then counts [chunks][ny] int32
