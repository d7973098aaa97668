// Differentiable augmentation in front of the discriminator (docs/d_augment.md): the state, the Philox draws, the per-element forward
// and backward and the layout of the two per-sample reductions, shared by the kernels of d_augment.hip and the CPU twins of
// d_augment_host.cpp.  Both files are built with -ffp-contract=off, so every fp32 operation below rounds once on either side; the
// draws and the controller are integer and double arithmetic in a fixed order.
#pragma once
#include <stdint.h>

#include "hoig_kernels.h"
#include "philox.h"

#if defined(__HIPCC__)
#define DAUG_HD __host__ __device__
#else
#define DAUG_HD
#endif

// ---- the state: HOIG_DAUG_STATE_WORDS 64-bit words (doubles are stored as their bits)
enum {
    DAUG_STEP = 0,        // uint64: steps begun (hoig_daug_tick adds one); the draws of a step use it as it stands
    DAUG_P = 1,           // double: the probability of each family
    DAUG_POS = 2,         // int64: d_real > 0 seen in the current interval
    DAUG_NEG = 3,         // int64: d_real < 0
    DAUG_TOTAL = 4,       // int64: d_real values seen
    DAUG_STEPS = 5,       // int64: hoig_daug_adapt calls in the current interval
    DAUG_SEED = 6,        // uint64: its low word is the Philox key's first word
    DAUG_RANK = 7,        // int64: the key's second word
    DAUG_TARGET = 8,      // double
    DAUG_INTERVAL = 9,    // int64
    DAUG_INCREMENT = 10,  // double: batch * interval / (kimg * 1000)
    DAUG_POLICY = 11,     // int64: HOIG_DAUG_COLOR | HOIG_DAUG_TRANSLATION | HOIG_DAUG_CUTOUT
    DAUG_RT = 12,         // double: r of the last adjustment
    DAUG_ADJUSTS = 13,    // int64: adjustments so far
};

DAUG_HD inline double daug_f64(uint64_t w) {
    union { uint64_t u; double d; } c;
    c.u = w;
    return c.d;
}
DAUG_HD inline uint64_t daug_u64(double d) {
    union { uint64_t u; double d; } c;
    c.d = d;
    return c.u;
}

// ---- Philox4x32-10 (philox.h: the routine the sliced Wasserstein distance shares)
DAUG_HD inline void daug_philox(const uint32_t ctr[4], uint32_t k0, uint32_t k1, uint32_t out[4]) {
    hoig_philox4x32_10(ctr, k0, k1, out);
}

DAUG_HD inline float daug_uniform(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-08f; }      // (w >> 8) * 2^-24, exact
DAUG_HD inline int daug_below(uint32_t w, int n) { return (int)(((uint64_t)w * (uint64_t)(uint32_t)n) >> 32); }
DAUG_HD inline int daug_shift(int n) { return (int)((double)n * 0.125 + 0.5); }      // the largest translation of an axis of n
DAUG_HD inline int daug_cut(int n) { return (int)((double)n * 0.5 + 0.5); }          // the cutout's size along it

// one record: 8 words {b, s, k (fp32 bits), ty, tx, cut_y0, cut_x0, flags}
DAUG_HD inline uint32_t daug_bits(float f) {
    union { uint32_t u; float f; } c;
    c.f = f;
    return c.u;
}
DAUG_HD inline float daug_float(uint32_t u) {
    union { uint32_t u; float f; } c;
    c.u = u;
    return c.f;
}

DAUG_HD inline void daug_draw_one(const uint64_t *state, int site, int sample, int H, int W, uint32_t *rec) {
    const uint64_t step = state[DAUG_STEP];
    const uint32_t k0 = (uint32_t)state[DAUG_SEED], k1 = (uint32_t)state[DAUG_RANK];
    const float p = (float)daug_f64(state[DAUG_P]);
    const int policy = (int)state[DAUG_POLICY];
    uint32_t w[12];
    for (int j = 0; j < 3; ++j) {
        const uint32_t ctr[4] = {(uint32_t)step, (uint32_t)(step >> 32), (uint32_t)site, (uint32_t)(3 * sample + j)};
        daug_philox(ctr, k0, k1, w + 4 * j);
    }
    const bool color = (policy & HOIG_DAUG_COLOR) && daug_uniform(w[0]) < p;
    const bool trans = (policy & HOIG_DAUG_TRANSLATION) && daug_uniform(w[1]) < p;
    const bool cut = (policy & HOIG_DAUG_CUTOUT) && daug_uniform(w[2]) < p;
    rec[0] = daug_bits(color ? daug_uniform(w[3]) - 0.5f : 0.f);
    rec[1] = daug_bits(color ? daug_uniform(w[4]) * 2.f : 1.f);
    rec[2] = daug_bits(color ? daug_uniform(w[5]) + 0.5f : 1.f);
    const int sy = daug_shift(H), sx = daug_shift(W);
    rec[3] = (uint32_t)(trans ? daug_below(w[6], 2 * sy + 1) - sy : 0);
    rec[4] = (uint32_t)(trans ? daug_below(w[7], 2 * sx + 1) - sx : 0);
    const int cy = daug_cut(H), cx = daug_cut(W);
    rec[5] = (uint32_t)(cut ? daug_below(w[8], H + 1 - cy % 2) - cy / 2 : 0);
    rec[6] = (uint32_t)(cut ? daug_below(w[9], W + 1 - cx % 2) - cx / 2 : 0);
    rec[7] = (color ? HOIG_DAUG_COLOR : 0) | (trans ? HOIG_DAUG_TRANSLATION : 0) | (cut ? HOIG_DAUG_CUTOUT : 0);
}

// ---- the controller (one thread): the counts of one D step join the interval's; every `interval` calls p moves by one increment
DAUG_HD inline void daug_adapt(uint64_t *state, int64_t pos, int64_t neg, int64_t n) {
    const int64_t P = (int64_t)state[DAUG_POS] + pos, N = (int64_t)state[DAUG_NEG] + neg, T = (int64_t)state[DAUG_TOTAL] + n;
    const int64_t steps = (int64_t)state[DAUG_STEPS] + 1;
    if (steps < (int64_t)state[DAUG_INTERVAL]) {
        state[DAUG_POS] = (uint64_t)P, state[DAUG_NEG] = (uint64_t)N, state[DAUG_TOTAL] = (uint64_t)T, state[DAUG_STEPS] = (uint64_t)steps;
        return;
    }
    const double r = (double)(P - N) / (double)T, d = r - daug_f64(state[DAUG_TARGET]);
    double p = daug_f64(state[DAUG_P]);
    const double inc = daug_f64(state[DAUG_INCREMENT]);
    if (d > 0.0) p += inc;
    else if (d < 0.0) p -= inc;
    if (p < 0.0) p = 0.0;
    if (p > 1.0) p = 1.0;
    state[DAUG_P] = daug_u64(p);
    state[DAUG_RT] = daug_u64(r);
    state[DAUG_ADJUSTS] += 1;
    state[DAUG_POS] = state[DAUG_NEG] = state[DAUG_TOTAL] = state[DAUG_STEPS] = 0;
}

// ---- the records as the kernels read them
struct DaugRec {
    float b, s, k;
    int ty, tx, cy0, cx0, flags;
};

DAUG_HD inline DaugRec daug_rec(const uint32_t *params, int i) {
    const uint32_t *r = params + 8 * (int64_t)i;
    DaugRec o;
    o.b = daug_float(r[0]), o.s = daug_float(r[1]), o.k = daug_float(r[2]);
    o.ty = (int)r[3], o.tx = (int)r[4], o.cy0 = (int)r[5], o.cx0 = (int)r[6], o.flags = (int)r[7];
    return o;
}

// does output pixel (y, x) survive, and which source pixel does it show?  (64-bit sums: a handcrafted record may hold any shift)
DAUG_HD inline bool daug_source(const DaugRec &r, int H, int W, int y, int x, int *ys, int *xs) {
    if (r.flags & HOIG_DAUG_CUTOUT) {
        const int64_t y0 = r.cy0, x0 = r.cx0;
        if (y >= y0 && y < y0 + daug_cut(H) && x >= x0 && x < x0 + daug_cut(W)) return false;
    }
    int64_t sy = y, sx = x;
    if (r.flags & HOIG_DAUG_TRANSLATION) sy += r.ty, sx += r.tx;
    if (sy < 0 || sy >= H || sx < 0 || sx >= W) return false;
    *ys = (int)sy, *xs = (int)sx;
    return true;
}

// the output pixel that shows source pixel (ys, xs), if one does
DAUG_HD inline bool daug_target(const DaugRec &r, int H, int W, int ys, int xs, int *y, int *x) {
    int64_t oy = ys, ox = xs;
    if (r.flags & HOIG_DAUG_TRANSLATION) oy -= r.ty, ox -= r.tx;
    if (oy < 0 || oy >= H || ox < 0 || ox >= W) return false;
    if (r.flags & HOIG_DAUG_CUTOUT) {
        const int64_t y0 = r.cy0, x0 = r.cx0;
        if (oy >= y0 && oy < y0 + daug_cut(H) && ox >= x0 && ox < x0 + daug_cut(W)) return false;
    }
    *y = (int)oy, *x = (int)ox;
    return true;
}

// channel c of an image pixel px[0..3) under brightness b, saturation s, contrast k about mu = M + b
DAUG_HD inline float daug_color(const float *px, int c, const DaugRec &r, float mu) {
    const float p0 = px[0] + r.b, p1 = px[1] + r.b, p2 = px[2] + r.b;
    const float m = ((p0 + p1) + p2) / 3.f;
    const float pc = c == 0 ? p0 : (c == 1 ? p1 : p2);
    const float q = (pc - m) * r.s + m;
    return (q - mu) * r.k + mu;
}

// channel c of output pixel (y, x) of sample i; `img`, `cond` are the sample's own
DAUG_HD inline float daug_fwd_at(const float *img, const float *cond, const DaugRec &r, float mu, int H, int W, int k, int y, int x, int c) {
    int ys, xs;
    if (!daug_source(r, H, W, y, x, &ys, &xs)) return 0.f;
    const int64_t src = (int64_t)ys * W + xs;
    if (c >= 3) return cond[src * k + (c - 3)];
    if (!(r.flags & HOIG_DAUG_COLOR)) return img[src * 3 + c];
    return daug_color(img + src * 3, c, r, mu);
}

// element e = (y * W + x) * (3 + k) + c of sample i's output
DAUG_HD inline float daug_fwd_elem(const float *img, const float *cond, const DaugRec &r, float mu, int H, int W, int k, int e) {
    const int C = 3 + k, pix = e / C, y = pix / W;
    return daug_fwd_at(img, cond, r, mu, H, W, k, y, pix - y * W, e - pix * C);
}

// channel c of source pixel (ys, xs) of sample i's image gradient; `g` is the sample's own [H][W][3 + k]; cmu = dmu / (3HW)
DAUG_HD inline float daug_bwd_at(const float *g, const DaugRec &r, float cmu, int H, int W, int k, int ys, int xs, int c) {
    int y, x;
    const bool live = daug_target(r, H, W, ys, xs, &y, &x);
    if (!(r.flags & HOIG_DAUG_COLOR)) return live ? g[((int64_t)y * W + x) * (3 + k) + c] : 0.f;
    if (!live) return cmu;
    const float *gp = g + ((int64_t)y * W + x) * (3 + k);
    const float d0 = r.k * gp[0], d1 = r.k * gp[1], d2 = r.k * gp[2];
    const float mean = ((d0 + d1) + d2) / 3.f;
    const float dc = c == 0 ? d0 : (c == 1 ? d1 : d2);
    const float dp = r.s * dc + (1.f - r.s) * mean;
    return dp + cmu;
}

// element e = (ys * W + xs) * 3 + c of sample i's image gradient
DAUG_HD inline float daug_bwd_elem(const float *g, const DaugRec &r, float cmu, int H, int W, int k, int e) {
    const int pix = e / 3, ys = pix / W;
    return daug_bwd_at(g, r, cmu, H, W, k, ys, pix - ys * W, e - pix * 3);
}

// ---- the two reductions.  A sample's `units` (groups of four image values; output pixels of g) are cut into `parts` equal chunks,
// one workgroup of HOIG_DAUG_THREADS each: thread t adds the units chunk_start + t, + THREADS, ... in that order, the workgroup adds its
// threads as a halving tree (t += t + 128, 64, ..., 1), and whoever needs the sum adds the `parts` partials first to last.  All of it
// follows from the sizes alone.
constexpr int DAUG_NT = HOIG_DAUG_THREADS;
constexpr int DAUG_MAX_PARTS = HOIG_DAUG_MAX_PARTS;

DAUG_HD inline int daug_parts(int64_t units) {
    const int64_t p = (units + 4 * DAUG_NT - 1) / (4 * DAUG_NT);
    return (int)(p < 1 ? 1 : (p > DAUG_MAX_PARTS ? DAUG_MAX_PARTS : p));
}
DAUG_HD inline int64_t daug_chunk(int64_t units) {
    const int parts = daug_parts(units);
    return (units + parts - 1) / parts;
}

// thread t's share of part `part` of the image sum: groups of four values, each value added in turn
DAUG_HD inline float daug_mean_thread(const float *img, int64_t n, int part, int t) {
    const int64_t groups = (n + 3) / 4, chunk = daug_chunk(groups);
    const int64_t lo = part * chunk, hi = lo + chunk < groups ? lo + chunk : groups;
    const bool vec = !((uintptr_t)img & 15);
    float acc = 0.f;
    for (int64_t gidx = lo + t; gidx < hi; gidx += DAUG_NT) {
        const int64_t e = gidx * 4;
        if (vec && e + 4 <= n) {
            const float *v = img + e;
#if defined(__HIP_DEVICE_COMPILE__)
            const float4 q = *reinterpret_cast<const float4 *>(v);
            acc += q.x, acc += q.y, acc += q.z, acc += q.w;
#else
            acc += v[0], acc += v[1], acc += v[2], acc += v[3];
#endif
        } else {
            for (int64_t j = e; j < e + 4 && j < n; ++j) acc += img[j];
        }
    }
    return acc;
}

// thread t's share of part `part` of G: the image channels of g at the surviving output pixels
DAUG_HD inline float daug_gsum_thread(const float *g, const DaugRec &r, int H, int W, int k, int part, int t) {
    const int64_t npix = (int64_t)H * W, chunk = daug_chunk(npix);
    const int64_t lo = part * chunk, hi = lo + chunk < npix ? lo + chunk : npix;
    float acc = 0.f;
    for (int64_t pix = lo + t; pix < hi; pix += DAUG_NT) {
        const int y = (int)(pix / W), x = (int)(pix - (int64_t)y * W);
        int ys, xs;
        if (!daug_source(r, H, W, y, x, &ys, &xs)) continue;
        const float *gp = g + pix * (3 + k);
        acc += gp[0], acc += gp[1], acc += gp[2];
    }
    return acc;
}

DAUG_HD inline float daug_sum_parts(const float *partials, int parts) {
    float s = partials[0];
    for (int j = 1; j < parts; ++j) s += partials[j];
    return s;
}

// mu = M + b of a colour sample from the partials of its image sum
DAUG_HD inline float daug_mu(const float *partials, int H, int W, float b) {
    const int64_t n = 3 * (int64_t)H * W;
    return daug_sum_parts(partials, daug_parts((n + 3) / 4)) / (float)n + b;
}

// dmu / (3HW) of a colour sample from the partials of G
DAUG_HD inline float daug_cmu(const float *partials, int H, int W, float k) {
    const int64_t npix = (int64_t)H * W;
    return ((1.f - k) * daug_sum_parts(partials, daug_parts(npix))) / (float)(3 * npix);
}

// ---- argument checks shared by the kernels' entry points and the twins
inline bool daug_ranges_overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y ? y - x < (uintptr_t)na : x - y < (uintptr_t)nb;
}

inline bool daug_shape_ok(int B, int H, int W, int k) {
    if (B <= 0 || H <= 0 || W <= 0 || k <= 0) return false;
    return (int64_t)H * W * (3 + (int64_t)k) < ((int64_t)1 << 31) && (int64_t)B * 8 < ((int64_t)1 << 31);
}

inline bool daug_state_ok(const uint64_t *state) { return state && !((uintptr_t)state & 7); }

inline bool daug_draw_ok(const uint64_t *state, int site, int B, int H, int W, const uint32_t *params) {
    return daug_state_ok(state) && params && !((uintptr_t)params & 15) && site >= 0 && site < HOIG_DAUG_SITES && daug_shape_ok(B, H, W, 1);
}

inline bool daug_fwd_ok(const float *img, const float *cond, const uint32_t *params, const float *out, int B, int H, int W, int k,
                        const float *ws) {
    if (!img || !cond || !params || !out || !ws || !daug_shape_ok(B, H, W, k)) return false;
    if (((uintptr_t)img | (uintptr_t)cond | (uintptr_t)out | (uintptr_t)ws) & 3 || ((uintptr_t)params & 15)) return false;
    const int64_t npix = (int64_t)B * H * W;
    const int64_t no = npix * (3 + k) * 4, nw = (int64_t)B * DAUG_MAX_PARTS * 4;
    return !daug_ranges_overlap(out, no, img, npix * 12) && !daug_ranges_overlap(out, no, cond, npix * k * 4) &&
           !daug_ranges_overlap(out, no, params, (int64_t)B * 32) && !daug_ranges_overlap(out, no, ws, nw) &&
           !daug_ranges_overlap(ws, nw, img, npix * 12) && !daug_ranges_overlap(ws, nw, cond, npix * k * 4) &&
           !daug_ranges_overlap(ws, nw, params, (int64_t)B * 32);
}

inline bool daug_bwd_ok(const float *g, const uint32_t *params, const float *dimg, int B, int H, int W, int k, const float *ws) {
    if (!g || !params || !dimg || !ws || !daug_shape_ok(B, H, W, k)) return false;
    if (((uintptr_t)g | (uintptr_t)dimg | (uintptr_t)ws) & 3 || ((uintptr_t)params & 15)) return false;
    const int64_t npix = (int64_t)B * H * W;
    const int64_t nd = npix * 12, nw = (int64_t)B * DAUG_MAX_PARTS * 4;
    return !daug_ranges_overlap(dimg, nd, g, npix * (3 + k) * 4) && !daug_ranges_overlap(dimg, nd, params, (int64_t)B * 32) &&
           !daug_ranges_overlap(dimg, nd, ws, nw) && !daug_ranges_overlap(ws, nw, g, npix * (3 + k) * 4) &&
           !daug_ranges_overlap(ws, nw, params, (int64_t)B * 32);
}
