// The opt-in GAN objectives and the LeCam regulariser (docs/gan_objectives.md): the per-element value and derivative of every
// objective, the regulariser in both forms, the state and its tick, and the layout of the sums, shared by the kernels of gan_loss.hip
// and the CPU twins of gan_loss_host.cpp.  Both files are built with -ffp-contract=off, so every fp32 operation below rounds once on
// either side.  Outside the logistic objective every operation is +, -, *, a comparison or a conversion: the twins give the kernels'
// bits.  The logistic objective calls expf / log1pf, which are the device library's on one side and the host's on the other.
#pragma once
#include <math.h>
#include <stdint.h>

#include "hoig_kernels.h"

#if defined(__HIPCC__)
#define GAN_HD __host__ __device__
#else
#define GAN_HD
#endif

// ---- the state: HOIG_LECAM_STATE_WORDS 64-bit words (doubles are stored as their bits)
enum {
    LECAM_COUNT = 0,      // int64: ticks taken (a tick with a non-finite mean is not one)
    LECAM_ALPHA_R = 1,    // double: the anchor of D(real), the moving average of mean(a); it regularises the FAKE logits
    LECAM_ALPHA_F = 2,    // double: the anchor of D(fake), the moving average of mean(b); it regularises the REAL logits
    LECAM_GAMMA = 3,      // double: the decay, in (0, 1)
    LECAM_START = 4,      // int64: the regulariser has weight once LECAM_COUNT, as it stands before the step, is >= this
    LECAM_BAD = 5,        // int64: ticks refused because mean(a) or mean(b) was not finite
    LECAM_LAST_R = 6,     // double: mean(a) of the last tick taken
    LECAM_LAST_F = 7,     // double: mean(b) of the last tick taken
};

GAN_HD inline double gan_f64(uint64_t w) {
    union { uint64_t u; double d; } c;
    c.u = w;
    return c.d;
}
GAN_HD inline uint64_t gan_u64(double d) {
    union { uint64_t u; double d; } c;
    c.d = d;
    return c.u;
}

// ---- what is done to one logit: the objective's term for it
enum {
    GAN_F_LS_REAL = 0,    // (x - 1)^2
    GAN_F_LS_FAKE = 1,    // (x + 1)^2
    GAN_F_LS_ZERO = 2,    // x^2                  (the generator's least-squares term)
    GAN_F_HINGE_REAL = 3, // max(0, 1 - x)
    GAN_F_HINGE_FAKE = 4, // max(0, 1 + x)
    GAN_F_NEG = 5,        // -x                   (the generator's hinge term)
    GAN_F_SP_NEG = 6,     // softplus(-x)         (logistic: D on real, and the generator's non-saturating term)
    GAN_F_SP_POS = 7,     // softplus(x)          (logistic: D on fake)
    GAN_F_NONE = -1,
};

// the term of the real logits (side 0) and of the fake logits (side 1) in the D step, and of the fake logits in the G step (side 2)
GAN_HD inline int gan_kind(int mode, int side) {
    if (mode == HOIG_GAN_LSGAN) return side == 0 ? GAN_F_LS_REAL : (side == 1 ? GAN_F_LS_FAKE : GAN_F_LS_ZERO);
    if (mode == HOIG_GAN_HINGE) return side == 0 ? GAN_F_HINGE_REAL : (side == 1 ? GAN_F_HINGE_FAKE : GAN_F_NEG);
    if (mode == HOIG_GAN_LOGISTIC) return side == 1 ? GAN_F_SP_POS : GAN_F_SP_NEG;
    return GAN_F_NONE;
}

// softplus(z) = max(z, 0) + log1p(exp(-|z|)) and its derivative, the sigmoid, from the same exp(-|z|) <= 1: nothing overflows
GAN_HD inline void gan_softplus(float z, float *v, float *d) {
    const float az = z < 0.f ? -z : z;
    const float e = expf(-az);
    *v = (z > 0.f ? z : 0.f) + log1pf(e);
    const float r = 1.f / (1.f + e);
    *d = z >= 0.f ? r : e * r;
}

// value and derivative of term `kind` at x.  The subgradient of max(0, .) at its kink is 0.
GAN_HD inline void gan_term(int kind, float x, float *v, float *d) {
    switch (kind) {
    case GAN_F_LS_REAL: { const float t = x - 1.f; *v = t * t, *d = 2.f * t; return; }
    case GAN_F_LS_FAKE: { const float t = x + 1.f; *v = t * t, *d = 2.f * t; return; }
    case GAN_F_LS_ZERO: *v = x * x, *d = 2.f * x; return;
    case GAN_F_HINGE_REAL: { const float t = 1.f - x; const bool on = t > 0.f; *v = on ? t : 0.f, *d = on ? -1.f : 0.f; return; }
    case GAN_F_HINGE_FAKE: { const float t = 1.f + x; const bool on = t > 0.f; *v = on ? t : 0.f, *d = on ? 1.f : 0.f; return; }
    case GAN_F_NEG: *v = -x, *d = -1.f; return;
    case GAN_F_SP_NEG: { float dz; gan_softplus(-x, v, &dz); *d = -dz; return; }
    default: gan_softplus(x, v, d); return;
    }
}

// the regulariser's term of one logit against the OTHER side's anchor (fp32) and its derivative.  side 0: a real logit against
// alpha_F; side 1: a fake logit against alpha_R.  paper: (x - alpha)^2 on both sides; relu: max(0, a - alpha_F)^2, max(0, alpha_R - b)^2.
GAN_HD inline void gan_lecam(int form, int side, float x, float alpha, float *v, float *d) {
    if (form == HOIG_LECAM_PAPER) {
        const float t = x - alpha;
        *v = t * t, *d = 2.f * t;
        return;
    }
    const float t = side == 0 ? x - alpha : alpha - x;
    const float r = t > 0.f ? t : 0.f;
    *v = r * r;
    *d = side == 0 ? 2.f * r : -(2.f * r);
}

// ---- the layout of the sums, a function of the two sizes alone.  The logits are cut into chunks of HOIG_GAN_CHUNK: those of a first,
// then those of b (a chunk never holds both).  G = min(chunks, HOIG_GAN_MAX_GRID) workgroups of HOIG_GAN_THREADS threads; workgroup g
// takes the chunks g, g + G, g + 2 G, ...  in that order, and thread t of it the elements t, t + THREADS, ... of each chunk, adding
// every element's three doubles (term, logit, regulariser term) to its running sums of the element's side.  The workgroup adds its
// threads as a halving tree (thread t takes t + 128, then t + 64, ..., then t + 1: gan_tree; in the kernel the first two steps go
// through LDS and the last six are shuffles inside wave 0, which add the same pairs), stores ONE partial of six doubles, and the
// finishing step adds the G partials first to last.
constexpr int GAN_NT = HOIG_GAN_THREADS;
constexpr int GAN_CHUNK = HOIG_GAN_CHUNK;
constexpr int GAN_MAX_GRID = HOIG_GAN_MAX_GRID;      // the cap: with more chunks than this a workgroup walks several
constexpr int GAN_SUMS = 6;                          // {term, logit, regulariser} of a, then of b

struct gan_acc {
    double s[GAN_SUMS];
};

GAN_HD inline gan_acc gan_zero() {
    gan_acc z;
    for (int j = 0; j < GAN_SUMS; ++j) z.s[j] = 0.0;
    return z;
}
GAN_HD inline gan_acc gan_join(const gan_acc &x, const gan_acc &y) {
    gan_acc r;
    for (int j = 0; j < GAN_SUMS; ++j) r.s[j] = x.s[j] + y.s[j];
    return r;
}

GAN_HD inline int64_t gan_chunks(int64_t n) { return (n + GAN_CHUNK - 1) / GAN_CHUNK; }
GAN_HD inline int gan_grid(int64_t n_a, int64_t n_b) {
    const int64_t c = gan_chunks(n_a) + gan_chunks(n_b);
    return (int)(c < GAN_MAX_GRID ? c : GAN_MAX_GRID);
}

// what a launch of the head needs to know; the same struct goes to the kernel and to the twin
struct gan_args {
    const float *a, *b;       // the logits: real, fake (a may be null with n_a = 0: the G head)
    int64_t n_a, n_b;
    float *da, *db;           // the gradients, or null
    int kind_a, kind_b;       // GAN_F_*
    int form;                 // HOIG_LECAM_*
    float sa, sb;             // (float)(s / n_a), (float)(s / n_b)
    double lam_a, lam_b;      // lambda / n_a, lambda / n_b (the device multiplies by its 0 or 1 and rounds to fp32)
    const uint64_t *state;    // null: no regulariser
};

// the weight's 0 or 1, decided from the state as it stands BEFORE the step
GAN_HD inline bool gan_lecam_on(const uint64_t *state) {
    return state && (int64_t)state[LECAM_COUNT] >= (int64_t)state[LECAM_START];
}

// thread t's share of workgroup g's chunks (grid workgroups in all): writes the gradients, returns the six sums
GAN_HD inline gan_acc gan_thread(const gan_args &p, int grid, int g, int t) {
    gan_acc acc = gan_zero();
    const bool reg = p.state != nullptr;
    const bool on = gan_lecam_on(p.state);
    const float al_a = reg ? (float)gan_f64(p.state[LECAM_ALPHA_F]) : 0.f, al_b = reg ? (float)gan_f64(p.state[LECAM_ALPHA_R]) : 0.f;
    const float la = on ? (float)p.lam_a : 0.f, lb = on ? (float)p.lam_b : 0.f;
    const int64_t ca = gan_chunks(p.n_a), c_all = ca + gan_chunks(p.n_b);
    for (int64_t c = g; c < c_all; c += grid) {
        const int side = c < ca ? 0 : 1;
        const float *x = side ? p.b : p.a;
        float *dx = side ? p.db : p.da;
        const int64_t n = side ? p.n_b : p.n_a, lo = (side ? c - ca : c) * GAN_CHUNK, hi = lo + GAN_CHUNK < n ? lo + GAN_CHUNK : n;
        const int kind = side ? p.kind_b : p.kind_a;
        const float sc = side ? p.sb : p.sa, lc = side ? lb : la, al = side ? al_b : al_a;
        for (int64_t i = lo + t; i < hi; i += GAN_NT) {
            const float xi = x[i];
            float v, d, rv = 0.f, rd = 0.f;
            gan_term(kind, xi, &v, &d);
            float gi = sc * d;
            if (reg) {
                gan_lecam(p.form, side, xi, al, &rv, &rd);
                gi = gi + lc * rd;
            }
            if (dx) dx[i] = gi;
            acc.s[3 * side] += (double)v, acc.s[3 * side + 1] += (double)xi, acc.s[3 * side + 2] += (double)rv;
        }
    }
    return acc;
}

// the workgroup's tree over acc[0 .. GAN_NT), in place (the twin's form; the kernel's shuffles and its LDS step add the same pairs)
inline gan_acc gan_tree(gan_acc *acc) {
    for (int s = GAN_NT / 2; s > 0; s >>= 1)
        for (int t = 0; t < s; ++t) acc[t] = gan_join(acc[t], acc[t + s]);
    return acc[0];
}

GAN_HD inline bool gan_finite(double x) { return x - x == 0.0; }

// ---- the finishing step, one thread: the partials first to last, the slots, the tick
struct gan_finish_args {
    int grid;
    int64_t n_a, n_b;
    double s, lambda;
    float *term, *mean_a, *mean_b, *reg;      // fp32 slots that the results are ADDED to; each may be null
    uint64_t *state;                          // null: no regulariser, no tick
};

GAN_HD inline void gan_finish(const gan_finish_args &f, const double *partials) {
    gan_acc t = gan_zero();
    for (int g = 0; g < f.grid; ++g)
        for (int j = 0; j < GAN_SUMS; ++j) t.s[j] += partials[(int64_t)g * GAN_SUMS + j];
    const double na = (double)f.n_a, nb = (double)f.n_b;
    double obj = f.s * (t.s[3] / nb), ma = 0.0, reg = 0.0;
    const double mb = t.s[4] / nb;
    if (f.n_a > 0) obj = f.s * (t.s[0] / na) + obj, ma = t.s[1] / na;
    if (f.state) {
        reg = t.s[5] / nb;
        if (f.n_a > 0) reg = t.s[2] / na + reg;
        if (!gan_lecam_on(f.state)) reg = 0.0;
        obj = obj + f.lambda * reg;
    }
    if (f.term) *f.term = *f.term + (float)obj;
    if (f.mean_a) *f.mean_a = *f.mean_a + (float)ma;
    if (f.mean_b) *f.mean_b = *f.mean_b + (float)mb;
    if (f.reg) *f.reg = *f.reg + (float)reg;
    if (!f.state) return;
    // the tick: after every workgroup has read the anchors (this runs behind them in stream order)
    uint64_t *st = f.state;
    if (!gan_finite(ma) || !gan_finite(mb)) {
        st[LECAM_BAD] += 1;
        return;
    }
    if (st[LECAM_COUNT] == 0) {
        st[LECAM_ALPHA_R] = gan_u64(ma), st[LECAM_ALPHA_F] = gan_u64(mb);
    } else {
        const double g = gan_f64(st[LECAM_GAMMA]);
        st[LECAM_ALPHA_R] = gan_u64(g * gan_f64(st[LECAM_ALPHA_R]) + (1.0 - g) * ma);
        st[LECAM_ALPHA_F] = gan_u64(g * gan_f64(st[LECAM_ALPHA_F]) + (1.0 - g) * mb);
    }
    st[LECAM_COUNT] += 1;
    st[LECAM_LAST_R] = gan_u64(ma), st[LECAM_LAST_F] = gan_u64(mb);
}

// ---- argument checks and the packing of the arguments, shared by the entry points and the twins
inline bool gan_overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y ? y - x < (uintptr_t)na : x - y < (uintptr_t)nb;
}

inline bool gan_f32_ok(const void *p, bool may_be_null) { return p ? !((uintptr_t)p & 3) : may_be_null; }

// the D head's arguments -> (gan_args, gan_finish_args); false: HOIG_EINVAL
inline bool gan_d_pack(int mode, const float *a, int64_t n_a, const float *b, int64_t n_b, double s, double lambda, int form,
                       uint64_t *state, float *da, float *db, float *term, float *mean_a, float *mean_b, float *reg, gan_args *p,
                       gan_finish_args *f) {
    if (gan_kind(mode, 0) == GAN_F_NONE || (form != HOIG_LECAM_PAPER && form != HOIG_LECAM_RELU)) return false;
    const int64_t lim = (int64_t)1 << 40;
    if (n_a <= 0 || n_b <= 0 || n_a >= lim || n_b >= lim || !gan_finite(s) || !gan_finite(lambda) || lambda < 0.0) return false;
    if (!gan_f32_ok(a, false) || !gan_f32_ok(b, false) || !gan_f32_ok(da, true) || !gan_f32_ok(db, true) || !gan_f32_ok(term, true) ||
        !gan_f32_ok(mean_a, true) || !gan_f32_ok(mean_b, true) || !gan_f32_ok(reg, true) || ((uintptr_t)state & 7))
        return false;
    // a gradient may not lie over the logits of the other side, nor over the other gradient (in place over its own logits is fine)
    if (gan_overlap(da, 4 * n_a, b, 4 * n_b) || gan_overlap(db, 4 * n_b, a, 4 * n_a) || gan_overlap(da, 4 * n_a, db, 4 * n_b)) return false;
    p->a = a, p->b = b, p->n_a = n_a, p->n_b = n_b, p->da = da, p->db = db;
    p->kind_a = gan_kind(mode, 0), p->kind_b = gan_kind(mode, 1), p->form = form;
    p->sa = (float)(s / (double)n_a), p->sb = (float)(s / (double)n_b);
    p->lam_a = lambda / (double)n_a, p->lam_b = lambda / (double)n_b;
    p->state = state;
    f->grid = gan_grid(n_a, n_b), f->n_a = n_a, f->n_b = n_b, f->s = s, f->lambda = lambda;
    f->term = term, f->mean_a = mean_a, f->mean_b = mean_b, f->reg = reg, f->state = state;
    return true;
}

// the G head's: the fake logits alone, no state
inline bool gan_g_pack(int mode, const float *b, int64_t n_b, double s, float *db, float *term, gan_args *p, gan_finish_args *f) {
    if (gan_kind(mode, 2) == GAN_F_NONE || n_b <= 0 || n_b >= ((int64_t)1 << 40) || !gan_finite(s)) return false;
    if (!gan_f32_ok(b, false) || !gan_f32_ok(db, true) || !gan_f32_ok(term, true)) return false;
    p->a = nullptr, p->b = b, p->n_a = 0, p->n_b = n_b, p->da = nullptr, p->db = db;
    p->kind_a = GAN_F_NONE, p->kind_b = gan_kind(mode, 2), p->form = HOIG_LECAM_PAPER;
    p->sa = 0.f, p->sb = (float)(s / (double)n_b), p->lam_a = p->lam_b = 0.0, p->state = nullptr;
    f->grid = gan_grid(0, n_b), f->n_a = 0, f->n_b = n_b, f->s = s, f->lambda = 0.0;
    f->term = term, f->mean_a = f->mean_b = f->reg = nullptr, f->state = nullptr;
    return true;
}

inline int64_t gan_workspace_bytes(int64_t n_a, int64_t n_b) {
    if (n_a < 0 || n_b <= 0 || n_a >= ((int64_t)1 << 40) || n_b >= ((int64_t)1 << 40)) return -1;
    return (int64_t)gan_grid(n_a, n_b) * GAN_SUMS * (int64_t)sizeof(double);
}
