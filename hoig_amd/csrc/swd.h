// Laplacian-pyramid sliced Wasserstein distance (docs/swd.md): the per-lane code that the kernels of swd.hip and the CPU twins of
// swd_host.cpp share, the tile sizes and the workspace layouts.  Both files are built with -ffp-contract=off: every fp32 product and
// every sum below rounds once, on either side, in the order written here.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "hoig_kernels.h"
#include "philox.h"

#if defined(__HIPCC__)
#define SWD_HD __host__ __device__
#else
#define SWD_HD
#endif

#define SWD_PATCH 7                  // a patch is 7 x 7 pixels of 3 channels
#define SWD_PLANE 49                 // values of one channel of a descriptor
#define SWD_K HOIG_SWD_K             // 147 = 3 * 49 values, flattened as (c, dy, dx)
#define SWD_MAX_LEVELS 16
#define SWD_WAVE 64
#define SWD_NT 256                   // threads of a reduction workgroup (four waves)
#define SWD_MAX_PARTS 1024           // the most partial sums of a chunked reduction
#define SWD_DOWN_TILE 16             // a workgroup of the pyramid kernel makes 16 x 16 pixels of the next level
#define SWD_PROJ_TILE 64             // rows and directions of a workgroup's tile of the projection
#define SWD_SORT_LDS_MAX HOIG_SORT_LDS_MAX
#define SWD_SORT_TILE HOIG_SORT_TILE

// ---- levels
SWD_HD inline int swd_levels(int H, int W) {
    int m = H < W ? H : W, L = 0;
    while (m >= 16) ++L, m >>= 1;
    return L;                        // floor(log2(min / 16)) + 1; 0 below 16
}
// is (H, W, L) a pyramid this library takes?
SWD_HD inline bool swd_shape_ok(int H, int W, int L) {
    if (H < 16 || W < 16 || L < 1 || L > SWD_MAX_LEVELS || L > swd_levels(H, W)) return false;
    const int mask = (1 << (L - 1)) - 1;
    return !(H & mask) && !(W & mask);
}

// scipy's mode='mirror' for an index in [-2, m + 1], m >= 3: reflection about the edge sample, which is not repeated
SWD_HD inline int swd_mirror(int i, int m) { return i < 0 ? -i : (i >= m ? 2 * m - 2 - i : i); }

// ---- the filter.  f = [1, 4, 6, 4, 1] / 16; five products and four sums, left to right
SWD_HD inline float swd_tap5(float a0, float a1, float a2, float a3, float a4) {
    float s = 0.0625f * a0;
    s = s + 0.25f * a1;
    s = s + 0.375f * a2;
    s = s + 0.25f * a3;
    s = s + 0.0625f * a4;
    return s;
}

// One value of the horizontal pass of the step down: source row ys (already mirrored) of an NHWC image of width W, filtered at
// column 2 xo, channel c.
template <class T>
SWD_HD inline float swd_down_h(const T *img, int W, int ys, int xo, int c) {
    const T *row = img + (int64_t)ys * W * 3 + c;
    const int x = 2 * xo;
    return swd_tap5((float)row[3 * swd_mirror(x - 2, W)], (float)row[3 * swd_mirror(x - 1, W)], (float)row[3 * x],
                    (float)row[3 * swd_mirror(x + 1, W)], (float)row[3 * swd_mirror(x + 2, W)]);
}

// lap[l] at (y, x, c): g[l] minus the step up of g[l + 1] (4 f (x) f on the zero-interleaved image: the taps that meet a zero are
// left out, which changes no bit).  The weights of a pass are 2 f = [1, 4, 6, 4, 1] / 8; columns first, taps left to right, then rows
// top to bottom.  next == nullptr: the last level, lap = g.
template <class T>
SWD_HD inline float swd_lap_at(const T *g, int Hl, int Wl, const float *next, int y, int x, int c) {
    const float v = (float)g[((int64_t)y * Wl + x) * 3 + c];
    if (!next) return v;
    const float w[5] = {0.125f, 0.5f, 0.75f, 0.5f, 0.125f};
    const int Wn = Wl >> 1;
    float up = 0.f;
    for (int i = 0; i < 5; ++i) {
        const int ty = swd_mirror(y + i - 2, Hl);
        if (ty & 1) continue;
        float row = 0.f;
        for (int j = 0; j < 5; ++j) {
            const int tx = swd_mirror(x + j - 2, Wl);
            if (tx & 1) continue;
            row = row + w[j] * next[((int64_t)(ty >> 1) * Wn + (tx >> 1)) * 3 + c];
        }
        up = up + w[i] * row;
    }
    return v - up;
}

// ---- positions.  Counter (set id, level, image index, patch index), key (seed low, seed high); word 0 gives y0, word 1 x0
SWD_HD inline void swd_position(uint64_t seed, int set_id, int level, int64_t image, int patch, int Hl, int Wl, int *y0, int *x0) {
    const uint32_t ctr[4] = {(uint32_t)set_id, (uint32_t)level, (uint32_t)image, (uint32_t)patch};
    uint32_t w[4];
    hoig_philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    *y0 = hoig_philox_below(w[0], Hl - SWD_PATCH + 1);
    *x0 = hoig_philox_below(w[1], Wl - SWD_PATCH + 1);
}
SWD_HD inline int swd_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ---- chunked fp64 reductions.  E elements are cut into swd_parts(E) chunks of swd_chunk(E); a workgroup of SWD_NT threads owns a
// chunk: thread t adds the elements lo + t, + SWD_NT, .. in that order, the 64 lanes of a wave meet in a butterfly (offsets 32 .. 1),
// the four wave sums are added first to last.  The partials meet in one wave: lane l adds partials l, l + 64, .., then the butterfly.
SWD_HD inline int swd_parts(int64_t E) {
    const int64_t p = (E + 8 * SWD_NT - 1) / (8 * SWD_NT);
    return (int)(p < 1 ? 1 : (p > SWD_MAX_PARTS ? SWD_MAX_PARTS : p));
}
SWD_HD inline int64_t swd_chunk(int64_t E) {
    const int parts = swd_parts(E);
    return (E + parts - 1) / parts;
}
SWD_HD inline double swd_lane_partials(const double *part, int parts, int lane) {
    double s = 0.0;
    for (int p = lane; p < parts; p += SWD_WAVE) s = s + part[p];
    return s;
}

// element e of channel c of descriptor rows [R][147]
SWD_HD inline double swd_stat_elem(const float *rows, int c, int64_t e) {
    const int64_t r = e / SWD_PLANE;
    return (double)rows[r * SWD_K + c * SWD_PLANE + (e - r * SWD_PLANE)];
}
// thread t's share of chunk `part` of sum (x - pivot)^power, power 1 or 2
SWD_HD inline double swd_stat_thread(const float *rows, int64_t E, int c, int part, int t, double pivot, bool square) {
    const int64_t chunk = swd_chunk(E), lo = part * chunk, hi = lo + chunk < E ? lo + chunk : E;
    double s = 0.0;
    for (int64_t e = lo + t; e < hi; e += SWD_NT) {
        const double d = swd_stat_elem(rows, c, e) - pivot;
        s = s + (square ? d * d : d);
    }
    return s;
}
// thread t's share of chunk `part` of sum |a - b|
SWD_HD inline double swd_l1_thread(const float *a, const float *b, int64_t N, int part, int t) {
    const int64_t chunk = swd_chunk(N), lo = part * chunk, hi = lo + chunk < N ? lo + chunk : N;
    double s = 0.0;
    for (int64_t e = lo + t; e < hi; e += SWD_NT) s = s + fabs((double)a[e] - (double)b[e]);
    return s;
}

// ---- the projection's operand: (x - mean) / std in fp64, rounded to fp32 once
SWD_HD inline float swd_normalised(float x, double mean, double stdev) { return (float)(((double)x - mean) / stdev); }

// ---- the sort's keys: the order-preserving map float -> uint32 and back
SWD_HD inline uint32_t swd_key_encode(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
SWD_HD inline uint32_t swd_key_decode(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }
SWD_HD inline bool swd_bits_nan(uint32_t bits) { return (bits & 0x7FFFFFFFu) > 0x7F800000u; }

// ---- argument checks shared by the entry points and the twins
inline int swd_next_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}
inline int64_t swd_sort_tiles(int64_t n) { return (n + SWD_SORT_TILE - 1) / SWD_SORT_TILE; }
inline bool swd_sort_ok(const void *keys, int64_t S, int64_t n) {
    if (!keys || ((uintptr_t)keys & 3) || S < 1 || n < 1 || n >= ((int64_t)1 << 31)) return false;
    return S * swd_sort_tiles(n) < ((int64_t)1 << 31) && S * n < ((int64_t)1 << 40);
}
// chain: the Gaussian levels 1 .. L - 1 of n images, NHWC fp32, level after level (level l starts at swd_chain_floats(n, H, W, l))
SWD_HD inline int64_t swd_chain_floats(int n, int H, int W, int L) {
    int64_t f = 0;
    for (int l = 1; l < L; ++l) f += (int64_t)n * (H >> l) * (W >> l) * 3;
    return f;
}
inline bool swd_desc_ok(int n, int H, int W, int L, int patches) {
    if (n < 1 || patches < 1 || !swd_shape_ok(H, W, L)) return false;
    return (int64_t)n * H * W * 3 < ((int64_t)1 << 40) && (int64_t)n * L * patches * SWD_K < ((int64_t)1 << 40) &&
           (int64_t)n * L * patches < ((int64_t)1 << 31);
}
