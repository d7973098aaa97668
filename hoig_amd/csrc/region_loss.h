// The opt-in region reconstruction term of G (docs/region_loss.md): the argument checks, the layout of the workspace, the per-lane
// code of the value-and-gradient pass, the scales that the counting pass leaves and the finishing sums, shared by the kernels of
// region_loss.hip and the CPU twin of region_loss_host.cpp.  Both files are built with -ffp-contract=off.  Between input and output
// there is +, -, *, comparison, conversion and double division, in one order on either side: the twin gives the kernels' bits.
#pragma once
#include <stdint.h>

#include "hoig_kernels.h"

#if defined(__HIPCC__)
#define RL_HD __host__ __device__
#else
#define RL_HD
#endif

constexpr int RL_NT = HOIG_RLOSS_THREADS;
constexpr int RL_TILE = HOIG_RLOSS_TILE;              // floats of one image per workgroup: a workgroup never spans two images
constexpr int RL_VEC = 4;                             // floats of a vector: the flat stream is walked in whole 16-byte vectors
constexpr int RL_GROUPS = RL_TILE / (RL_VEC * RL_NT); // vectors per thread: thread t takes the vectors t, t + RL_NT, ... of its tile
constexpr int RL_MAXR = HOIG_RLOSS_MAX_R;
constexpr int RL_CTILE = HOIG_RLOSS_COUNT_TILE;       // labels of one image per workgroup of the counting pass (16 per thread)
static_assert(RL_GROUPS * RL_VEC * RL_NT == RL_TILE && RL_CTILE == 16 * RL_NT, "tile sizes");

// what every launch of the head needs to know; the same struct goes to the kernels and to the twin
struct rl_args {
    const float *pred, *target;
    const uint8_t *labels;
    float *dpred;                         // or null
    int N, H, W, C, R;
    int HW, E;                            // pixels and floats of one image (E <= 2^30)
    int tiles, ctiles;                    // workgroups per image: value-and-gradient pass, counting pass
    int min_pixels;
    float fa;                             // (float)(lambda_all / (N H W C)): the frame part of every gradient
    double lam[RL_MAXR + 1], lambda_all;
    float *term, *terms_r, *term_all;     // fp32 slots that are ADDED to (terms_r, term_all: or null)
    int32_t *counts_out, *status;         // counts_out: or null
};

// ---- the workspace: [head: counts int32 [N][R+1], ticket, largest bad label | scales fp32 [N][R+1], V int32 [R+1] | rows fp64
// [N][R+2] | partials fp64 [N][tiles][R+2]], every block 16-byte aligned.  The head is what the memset node zeroes.
struct rl_layout {
    int64_t head_bytes, off_scales, off_v, off_rows, off_partials, total;
};

RL_HD inline int64_t rl_up16(int64_t x) { return (x + 15) & ~(int64_t)15; }

inline rl_layout rl_make_layout(int N, int R, int tiles) {
    rl_layout l;
    const int64_t rows = (int64_t)N * (R + 1);
    l.head_bytes = rl_up16((rows + 2) * 4);
    l.off_scales = l.head_bytes;
    l.off_v = l.off_scales + rows * 4;
    l.off_rows = rl_up16(l.off_v + (R + 1) * 4);
    l.off_partials = l.off_rows + (int64_t)N * (R + 2) * 8;
    l.total = l.off_partials + (int64_t)N * tiles * (R + 2) * 8;
    return l;
}

inline bool rl_sizes_ok(int N, int H, int W, int C, int R) {
    return N >= 1 && N <= HOIG_RLOSS_MAX_N && H >= 1 && H <= 4096 && W >= 1 && W <= 4096 && C >= 1 && C <= HOIG_RLOSS_MAX_C && R >= 0 &&
           R <= RL_MAXR;
}

inline int rl_tiles(int H, int W, int C) { return (int)(((int64_t)H * W * C + RL_TILE - 1) / RL_TILE); }

inline int64_t rl_workspace_bytes(int N, int H, int W, int C, int R) {
    if (!rl_sizes_ok(N, H, W, C, R)) return -1;
    return rl_make_layout(N, R, rl_tiles(H, W, C)).total;
}

inline bool rl_finite(double x) { return x - x == 0.0; }

inline bool rl_overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y ? y - x < (uintptr_t)na : x - y < (uintptr_t)nb;
}

inline bool rl_w4(const void *p, bool may_be_null) { return p ? !((uintptr_t)p & 3) : may_be_null; }

// the entry points' arguments -> rl_args; false: HOIG_EINVAL
inline bool rl_pack(const float *pred, const float *target, const uint8_t *labels, int N, int H, int W, int C, int R, const double *lambda,
                    double lambda_all, int min_pixels, float *dpred, float *term, float *terms_r, float *term_all, int32_t *counts_out,
                    int32_t *status, rl_args *a) {
    if (!rl_sizes_ok(N, H, W, C, R) || !lambda || !labels || min_pixels < 1) return false;
    if (!rl_finite(lambda_all) || lambda_all < 0.0) return false;
    for (int r = 0; r <= R; ++r)
        if (!rl_finite(lambda[r]) || lambda[r] < 0.0) return false;
    if (!rl_w4(pred, false) || !rl_w4(target, false) || !rl_w4(dpred, true) || !rl_w4(term, false) || !rl_w4(terms_r, true) ||
        !rl_w4(term_all, true) || !rl_w4(counts_out, true) || !rl_w4(status, false))
        return false;
    const int64_t px = (int64_t)N * H * W, n4 = px * C * 4;
    if (rl_overlap(dpred, n4, pred, n4) || rl_overlap(dpred, n4, target, n4) || rl_overlap(dpred, n4, labels, px)) return false;
    a->pred = pred, a->target = target, a->labels = labels, a->dpred = dpred;
    a->N = N, a->H = H, a->W = W, a->C = C, a->R = R, a->HW = H * W, a->E = H * W * C;
    a->tiles = rl_tiles(H, W, C), a->ctiles = (H * W + RL_CTILE - 1) / RL_CTILE;
    a->min_pixels = min_pixels;
    a->fa = (float)(lambda_all / ((double)N * (double)H * (double)W * (double)C));
    for (int r = 0; r <= RL_MAXR; ++r) a->lam[r] = r <= R ? lambda[r] : 0.0;
    a->lambda_all = lambda_all;
    a->term = term, a->terms_r = terms_r, a->term_all = term_all, a->counts_out = counts_out, a->status = status;
    return true;
}

// ---- what the counting pass leaves: V_r, the gradient scale of every row -- (float)(lambda_r / (V_r C n_ir)), the quotient taken in
// double and rounded once; 0 for an invalid row --, counts_out and the status word.  One thread; `count(k)` reads count k = i (R+1) + r.
template <class Count>
RL_HD inline void rl_scales(const rl_args &a, Count count, int badmax, float *scales, int32_t *V) {
    const int R1 = a.R + 1;
    for (int r = 0; r < R1; ++r) {
        int v = 0;
        for (int i = 0; i < a.N; ++i) v += count(i * R1 + r) >= a.min_pixels ? 1 : 0;
        V[r] = v;
        for (int i = 0; i < a.N; ++i) {
            const int n = count(i * R1 + r);
            scales[i * R1 + r] = n >= a.min_pixels ? (float)(a.lam[r] / ((double)v * (double)a.C * (double)n)) : 0.f;
            if (a.counts_out) a.counts_out[i * R1 + r] = n;
        }
    }
    *a.status = badmax > 0 ? (HOIG_REGION_BAD_LABEL | (badmax << 8)) : 0;
}

// ---- the value-and-gradient pass.  16 bytes of the flat stream as one access where the hardware has it (the kernel, when the image's
// rows of pred, target and dpred start on 16 bytes), else float by float: the same four values either way.
RL_HD inline void rl_ld4(const float *p, float *v) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float4 x = *reinterpret_cast<const float4 *>(p);
    v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
#else
    v[0] = p[0], v[1] = p[1], v[2] = p[2], v[3] = p[3];
#endif
}
RL_HD inline void rl_st4(float *p, const float *v) {
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
#else
    p[0] = v[0], p[1] = v[1], p[2] = v[2], p[3] = v[3];
#endif
}

// Thread t of the workgroup that takes tile `tile` of image i: its RL_GROUPS vectors.  The pixel of an element is its index in the image
// divided by C.  sc[0 .. RT]: the scales of image i's rows (0 above R); acc[0 .. RT]: the running sums of |d| per region, acc[RT + 1]:
// the frame's.  RT >= R is a compile-time bound, so that the sums stay in registers: a label selects its sum by comparison, and adding
// the 0.0 of the others changes no bit (every sum is >= +0 or NaN).  The sign is that of hoig_loss_accumulate(HOIG_LOSS_L1): 0 at
// d = 0, and 0 for a NaN.
template <int RT>
RL_HD inline void rl_lane(const rl_args &a, int i, int tile, int t, bool vec, const float *sc, double *acc) {
    const int64_t base = (int64_t)i * a.E;
    const float *pr = a.pred + base, *tg = a.target + base;
    float *dp = a.dpred ? a.dpred + base : nullptr;
    const uint8_t *lb = a.labels + (int64_t)i * a.HW;
    for (int k = 0; k < RL_GROUPS; ++k) {
        const int e0 = tile * RL_TILE + RL_VEC * (t + RL_NT * k);
        if (e0 >= a.E) break;
        const int nv = a.E - e0 < RL_VEC ? a.E - e0 : RL_VEC;
        const bool whole = vec && nv == RL_VEC;
        float p[RL_VEC], q[RL_VEC], g[RL_VEC];
        if (whole) {
            rl_ld4(pr + e0, p), rl_ld4(tg + e0, q);
        } else {
            for (int j = 0; j < RL_VEC; ++j) p[j] = j < nv ? pr[e0 + j] : 0.f, q[j] = j < nv ? tg[e0 + j] : 0.f;
        }
        int px = e0 / a.C, rem = e0 - px * a.C;
        int lab = lb[px];
        for (int j = 0; j < RL_VEC; ++j) {
            g[j] = 0.f;
            if (j >= nv) break;
            const float d = p[j] - q[j];
            const float ad = __builtin_fabsf(d);
            const float s = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            const int l = lab <= a.R ? lab : -1;
            float sr = 0.f;
            for (int r = 0; r <= RT; ++r) {
                const bool m = l == r;
                sr = m ? sc[r] : sr;
                acc[r] += m ? (double)ad : 0.0;
            }
            acc[RT + 1] += (double)ad;
            g[j] = s * (a.fa + sr);
            if (++rem == a.C) {
                rem = 0, ++px;
                if (j + 1 < nv) lab = lb[px];
            }
        }
        if (dp) {
            if (whole) {
                rl_st4(dp + e0, g);
            } else {
                for (int j = 0; j < nv; ++j) dp[e0 + j] = g[j];
            }
        }
    }
}

// the workgroup's halving tree over the threads' sums, in place (the twin's form; the kernel's LDS step and its shuffles add the same
// pairs, as gan_loss.h documents it): thread t takes t + 128, then t + 64, ..., then t + 1
template <int RT>
inline void rl_tree(double (*acc)[RT + 2]) {
    for (int s = RL_NT / 2; s > 0; s >>= 1)
        for (int t = 0; t < s; ++t)
            for (int j = 0; j < RT + 2; ++j) acc[t][j] = acc[t][j] + acc[t + s][j];
}

// ---- the finishing pass.  Row rho = i (R + 2) + s of `rows`: the partials of image i's workgroups, first to last, of sum s (s <= R:
// region s; s = R + 1: the frame)
RL_HD inline double rl_row(const rl_args &a, const double *partials, int rho) {
    const int R2 = a.R + 2, i = rho / R2, s = rho - i * R2;
    double x = 0.0;
    for (int w = 0; w < a.tiles; ++w) x += partials[((int64_t)i * a.tiles + w) * R2 + s];
    return x;
}

// one thread, in index order: L_r, L_all and the term in double; each rounded to fp32 where it is added to its slot
RL_HD inline void rl_finish(const rl_args &a, const int32_t *counts, const int32_t *V, const double *rows) {
    const int R1 = a.R + 1, R2 = a.R + 2;
    double total = 0.0;
    for (int r = 0; r < R1; ++r) {
        double L = 0.0;
        if (V[r] > 0) {
            double s = 0.0;
            for (int i = 0; i < a.N; ++i) {
                const int n = counts[i * R1 + r];
                if (n >= a.min_pixels) s += rows[i * R2 + r] / ((double)a.C * (double)n);
            }
            L = s / (double)V[r];
        }
        total += a.lam[r] * L;
        if (a.terms_r) a.terms_r[r] = a.terms_r[r] + (float)L;
    }
    double f = 0.0;
    for (int i = 0; i < a.N; ++i) f += rows[i * R2 + R1];
    const double all = a.lambda_all * (f / ((double)a.N * (double)a.H * (double)a.W * (double)a.C));
    if (a.term_all) {
        *a.term_all = *a.term_all + (float)all;
        *a.term = *a.term + (float)total;
    } else {
        *a.term = *a.term + (float)(total + all);
    }
}
