// Streaming FID statistics and the Frechet distance in fp64 (docs/fid_device.md): the per-lane code that the kernels of fid_stats.hip
// and the CPU twins of fid_stats_host.cpp share, and the workspace layouts.  Both files are built with -ffp-contract=off, so that a
// product and the sum it goes into round one after the other on both sides.
//
// Every reduction here is made by ONE wave: lane l adds the terms l, l + 64, l + 128, .. in that order, then the 64 partial sums meet
// in a butterfly (offsets 32, 16, .. 1; an addition commutes, so every lane ends with the same bits).  The twins walk the same order
// (fid_butterfly), which makes the pivoted Cholesky and the tridiagonalisation a function of their input alone, equal on both sides.
#pragma once
#include <math.h>
#include <stdint.h>

#include "hoig_kernels.h"

#if defined(__HIPCC__)
#define FID_HD __host__ __device__
#else
#define FID_HD
#endif

#define FID_WAVE 64
#define FID_ROWS_PER_WAVE 4        // rows of a matrix one wave owns in the row-parallel steps
#define FID_EPS 2.220446049250313e-16   // 2^-52
#define FID_SAFMIN 2.2250738585072014e-308

// workspace of hoig_pchol_f64: this header, then the remaining diagonal twice (step j reads copy j & 1 and writes the other one)
struct fid_pchol_head {
    double tol;        // the stop rule's D * 2^-52 * d0
    int32_t done;      // set once: every later step returns at once
    int32_t status;    // HOIG_EINVAL after a non-finite entry
    int32_t pad[4];
};
#define FID_PIVOTED (-HUGE_VAL)    // the remaining diagonal of a row that has been a pivot

// workspace of hoig_sym_eigvals_f64: this header, then W [n][n] (the matrix being reduced), d [n], e [n], v [n], p [n]
struct fid_eig_head {
    double tau;        // of the current reflector (0: the step has nothing to do)
    int32_t done;
    int32_t status;
    int32_t pad[4];
};

FID_HD inline bool fid_finite(double v) { return v - v == 0.0; }

// one operand element of the TN product: fp64 as it is, or fp32 widened (exact) minus the pivot of its column
FID_HD inline double fid_operand(const void *base, int64_t at, int f32, const double *pivot, int col) {
    if (!f32) return static_cast<const double *>(base)[at];
    const double v = (double)static_cast<const float *>(base)[at];
    return pivot ? v - pivot[col] : v;
}

// argmax with the lowest index on ties: is (v, i) to be taken over (bv, bi)?
FID_HD inline bool fid_better(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }

// one lane's share of sum a[k * sa] b[k * sb], k in [0, n)
FID_HD inline double fid_lane_dot(const double *a, int64_t sa, const double *b, int64_t sb, int n, int lane) {
    double s = 0.0;
    for (int k = lane; k < n; k += FID_WAVE) s = s + a[k * sa] * b[k * sb];
    return s;
}

// the Householder reflector of x = (x0, tail) with sigma = |tail|^2, as LAPACK's dlarfg: H = I - tau v v^T, v = (1, tail * scale),
// H x = (beta, 0).  sigma == 0: H = I (tau 0, beta x0).
FID_HD inline void fid_reflector(double x0, double sigma, double *tau, double *beta, double *scale) {
    if (sigma == 0.0) {
        *tau = 0.0, *beta = x0, *scale = 0.0;
        return;
    }
    const double nrm = sqrt(x0 * x0 + sigma);
    const double b = x0 >= 0.0 ? -nrm : nrm;
    *tau = (b - x0) / b, *beta = b, *scale = 1.0 / (x0 - b);
}

// ---- eigenvalues of the symmetric tridiagonal (d, e) by bisection, as LAPACK's dstebz: Gershgorin bounds, pivmin, Sturm counts ----
FID_HD inline void fid_gershgorin(const double *d, const double *e, int n, double *gl, double *gu, double *pivmin) {
    double lo = d[0], hi = d[0], emax = 0.0;
    for (int i = 0; i < n; ++i) {
        const double l = i > 0 ? fabs(e[i - 1]) : 0.0, r = i + 1 < n ? fabs(e[i]) : 0.0;
        const double a = d[i] - (l + r), b = d[i] + (l + r);
        if (a < lo) lo = a;
        if (b > hi) hi = b;
        if (r * r > emax) emax = r * r;
    }
    *pivmin = FID_SAFMIN * (emax > 1.0 ? emax : 1.0);
    const double tnorm = fabs(lo) > fabs(hi) ? fabs(lo) : fabs(hi);
    const double widen = 2.1 * tnorm * FID_EPS * n + 4.2 * *pivmin;
    *gl = lo - widen, *gu = hi + widen;
    if (tnorm == 0.0) *gl = 0.0, *gu = 0.0;     // every disc is the point 0: the zero matrix
}

// the number of eigenvalues below x
FID_HD inline int fid_sturm_count(const double *d, const double *e, int n, double x, double pivmin) {
    double q = d[0] - x;
    if (fabs(q) < pivmin) q = -pivmin;
    int c = q < 0.0 ? 1 : 0;
    for (int i = 1; i < n; ++i) {
        q = d[i] - (e[i - 1] * e[i - 1]) / q - x;
        if (fabs(q) < pivmin) q = -pivmin;
        c += q < 0.0 ? 1 : 0;
    }
    return c;
}

// eigenvalue number idx (ascending, from 0): halves [gl, gu] until it is 2 * 2^-52 * max(|lo|, |hi|) + 2 pivmin wide
FID_HD inline double fid_bisect(const double *d, const double *e, int n, int idx, double gl, double gu, double pivmin) {
    double lo = gl, hi = gu;
    if (lo == hi) return lo;
    for (int it = 0; it < 2200; ++it) {      // (an interval of doubles halves at most 2098 times)
        const double big = fabs(lo) > fabs(hi) ? fabs(lo) : fabs(hi);
        if (hi - lo <= 2.0 * FID_EPS * big + 2.0 * pivmin) break;
        const double mid = 0.5 * (lo + hi);
        if (!(mid > lo && mid < hi)) break;
        if (fid_sturm_count(d, e, n, mid, pivmin) > idx) hi = mid; else lo = mid;
    }
    return 0.5 * (lo + hi);
}
