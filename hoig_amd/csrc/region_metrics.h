// Region scores (docs/region_metrics.md): the per-pixel sums, the box rule and the crop's two resample passes, shared by the kernels
// (region_metrics.hip) and their CPU twins (region_metrics_host.cpp), so that both run the same code.  Everything here is integer
// arithmetic on bytes: no result depends on the order in which partial sums meet.
//
// Statistics: a row is [count, sum |d|, sum d^2, x0, y0, x1, y1, 0] (HOIG_REGION_ROW int64); row 0 takes every pixel, row r the pixels
// labelled r.  region_rows<T> is the accumulator of one lane (T = uint32_t: at most REGION_LANE_PIXELS pixels, 3 * 255^2 each) or of
// the whole twin (T = int64_t).
// Crops: Pillow's fixed-point separable resample of pil_resize.h on the window (left, top, side) of a box, horizontal pass first and
// rounded to bytes, for every side up to min(H, W) from one buffer of tables (region_tables_*): [max_side, S], then (offset, ksize)
// per side, then the pil_build_table rows of every side.
#pragma once
#include <stdint.h>
#include "hoig_kernels.h"
#include "pil_resize.h"

#define REGION_NT 256
#define REGION_LANE_PIXELS 16                                  // 16 * 3 * 255^2 < 2^32
#define REGION_BLOCK_PIXELS (REGION_NT * REGION_LANE_PIXELS)
#define REGION_ROWS (HOIG_REGION_MAX + 1)
#define REGION_PER_LANE 4                                      // output bytes of a lane of the crop passes: one word

template <class T>
struct region_rows {
    T cnt[REGION_ROWS], ad[REGION_ROWS], sq[REGION_ROWS];
    int x0[REGION_ROWS], y0[REGION_ROWS], x1[REGION_ROWS], y1[REGION_ROWS];
    int bad;                                                   // the largest label above R that was read (0: none)
};

template <class T>
PIL_HD inline void region_rows_clear(region_rows<T> &a, int H, int W) {
#pragma unroll
    for (int r = 0; r < REGION_ROWS; ++r) {
        a.cnt[r] = 0, a.ad[r] = 0, a.sq[r] = 0;
        a.x0[r] = W, a.y0[r] = H, a.x1[r] = -1, a.y1[r] = -1;
    }
    a.bad = 0;
}

// one pixel at (x, y): its three byte pairs and its label
template <class T>
PIL_HD inline void region_rows_add(region_rows<T> &a, int R, const uint8_t *gen, const uint8_t *gt, int label, int x, int y) {
    int ad = 0, sq = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int d = (int)gen[c] - (int)gt[c];
        ad += d < 0 ? -d : d;
        sq += d * d;
    }
    if (label > R && label > a.bad) a.bad = label;
#pragma unroll
    for (int r = 0; r < REGION_ROWS; ++r) {
        if (r != 0 && r != label) continue;
        if (r > R) continue;
        a.cnt[r] += 1, a.ad[r] += (T)ad, a.sq[r] += (T)sq;
        if (x < a.x0[r]) a.x0[r] = x;
        if (y < a.y0[r]) a.y0[r] = y;
        if (x > a.x1[r]) a.x1[r] = x;
        if (y > a.y1[r]) a.y1[r] = y;
    }
}

PIL_HD inline int32_t region_status_word(int bad) { return bad ? (HOIG_REGION_BAD_LABEL | (bad << 8)) : 0; }

PIL_HD inline void region_row_init(int64_t *row, int H, int W) {
    row[0] = 0, row[1] = 0, row[2] = 0, row[3] = W, row[4] = H, row[5] = -1, row[6] = -1, row[7] = 0;
}

PIL_HD inline int region_floor_half(int v) { return v >= 0 ? v / 2 : -((1 - v) / 2); }

PIL_HD inline int region_clamp(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// box [left, top, side, valid] of one statistics row
PIL_HD inline void region_box(const int64_t *row, int H, int W, int min_pixels, int32_t *box) {
    const int64_t need = min_pixels > 1 ? min_pixels : 1;
    box[0] = box[1] = box[2] = box[3] = 0;
    if (row[0] < need) return;
    const int x0 = (int)row[3], y0 = (int)row[4], x1 = (int)row[5], y1 = (int)row[6];
    if (x0 < 0 || y0 < 0 || x1 >= W || y1 >= H || x1 < x0 || y1 < y0) return;        // (not a row region_rows made)
    const int w = x1 - x0 + 1, h = y1 - y0 + 1, side0 = w > h ? w : h, pad = (side0 + 3) / 4;
    int side = side0 + 2 * pad;
    if (side > H) side = H;
    if (side > W) side = W;
    box[0] = region_clamp(region_floor_half(x0 + x1 + 1 - side), W - side);
    box[1] = region_clamp(region_floor_half(y0 + y1 + 1 - side), H - side);
    box[2] = side;
    box[3] = 1;
}

// a box the crop passes may follow: valid, inside the image and inside the tables
PIL_HD inline bool region_box_usable(const int32_t *box, int H, int W, int S, const int32_t *tables) {
    const int left = box[0], top = box[1], side = box[2];
    if (!box[3] || side < 1 || left < 0 || top < 0 || side > W || side > H || left > W - side || top > H - side) return false;
    return side <= tables[0] && S == tables[1];
}

// the row [xmin, n, k[..]] of output sample xx for a source of `side` samples, its window clamped into the source
PIL_HD inline const int32_t *region_taps(const int32_t *tables, int side, int xx, int *xmin, int *n) {
    const int ksize = tables[2 * side + 1];
    const int32_t *row = tables + tables[2 * side] + (int64_t)xx * (PIL_ROW_HEAD + ksize);
    int lo = row[0], cnt = row[1] < ksize ? row[1] : ksize;
    if (lo < 0) lo = 0;
    if (lo > side) lo = side;
    if (cnt > side - lo) cnt = side - lo;
    *xmin = lo, *n = cnt;
    return row + PIL_ROW_HEAD;
}

// byte e of the horizontal pass's result [side][S][3] of one crop; img: the image the box lies in
PIL_HD inline uint8_t region_crop_h_byte(const uint8_t *img, int W, const int32_t *box, int S, const int32_t *tables, int e) {
    const int j = e % 3, xx = (e / 3) % S, y = e / (3 * S);
    int xmin, n;
    const int32_t *k = region_taps(tables, box[2], xx, &xmin, &n);
    return pil_resample_byte(img + ((int64_t)(box[1] + y) * W + box[0] + xmin) * 3 + j, 3, k, n);
}

// byte e of the crop [S][S][3] from the horizontal pass's result `mid` [side][S][3]
PIL_HD inline uint8_t region_crop_v_byte(const uint8_t *mid, const int32_t *box, int S, const int32_t *tables, int e) {
    const int row = 3 * S, j = e % row, yy = e / row;
    int ymin, n;
    const int32_t *k = region_taps(tables, box[2], yy, &ymin, &n);
    return pil_resample_byte(mid + (int64_t)ymin * row + j, row, k, n);
}

// bytes between two crops of the workspace [R][N][min(H, W)][S][3], rounded up so that every crop starts on a word
PIL_HD inline int64_t region_mid_stride(int H, int W, int S) {
    const int64_t m = (int64_t)(H < W ? H : W) * S * 3;
    return (m + 3) / 4 * 4;
}

inline bool region_stats_ok(int N, int H, int W, int R) {
    return N >= 1 && pil_side_ok(H) && pil_side_ok(W) && R >= 1 && R <= HOIG_REGION_MAX;
}

inline bool region_size_ok(int S) { return S >= HOIG_REGION_MIN_SIZE && S <= HOIG_REGION_MAX_SIZE; }

inline int64_t region_tables_words(int max_side, int S) {
    int64_t words = 2 * ((int64_t)max_side + 1);
    for (int s = 1; s <= max_side; ++s) words += (int64_t)S * (PIL_ROW_HEAD + pil_ksize(s, S));
    return words;
}

inline void region_tables_build(int max_side, int S, int32_t *tables) {
    tables[0] = max_side, tables[1] = S;
    int64_t at = 2 * ((int64_t)max_side + 1);
    for (int s = 1; s <= max_side; ++s) {
        const int ksize = pil_ksize(s, S);
        tables[2 * s] = (int32_t)at, tables[2 * s + 1] = ksize;
        pil_build_table(s, S, tables + at);
        at += (int64_t)S * (PIL_ROW_HEAD + ksize);
    }
}
