// Pillow's 8-bit Image.resize(size, BILINEAR) -- a fixed-point, separable convolution -- shared by its kernel (pil_resize.hip) and its
// CPU twin (pil_resize_host.cpp), so that both run the same code.  get_eval_loader resizes with it twice (to img_size, then to 299),
// which is what LPIPS and SSIM / MS-SSIM see; written from the algorithm's description, every byte pinned to Pillow by
// tests/test_pil_resize_cpu.py and tests/test_pil_resize_gpu.py.
//
// Per axis (in -> out samples), in double on the HOST:
//   scale = in / out, fs = max(scale, 1), support = fs (the triangle filter's support of 1, widened when shrinking), ss = 1 / fs;
//   output xx: center = (xx + 0.5) scale, xmin = max((int)(center - support + 0.5), 0), xmax = min((int)(center + support + 0.5), in),
//   n = xmax - xmin taps w[x] = max(0, 1 - |(x + xmin - center + 0.5) ss|), divided by their sum, then k[x] = (int)(0.5 + w[x] 2^22).
// One output byte = clip((2^21 + sum_x src[xmin + x] k[x]) >> 22, 0, 255) in int32 (the k of a row sum to about 2^22: < 2^31).
// The horizontal pass runs first and is rounded to bytes, the vertical pass reads that; a pass that keeps its size is skipped.
//
// A table holds one row of PIL_ROW_HEAD + ksize int32 per output sample: [xmin, n, k[0 .. ksize)], ksize = 2 ceil(support) + 1 >= n,
// unused taps zero.  The files that include this are built with -ffp-contract=off: the doubles below round step by step.
#pragma once
#include <math.h>
#include <stdint.h>
#include "hoig_kernels.h"

#if defined(__HIPCC__)
#define PIL_HD __host__ __device__
#else
#define PIL_HD
#endif

#define PIL_PRECISION_BITS 22
#define PIL_ROW_HEAD 2
#define PIL_MAX_SIDE 4096

// the one output byte: n taps k[] on bytes `stride` apart
PIL_HD inline uint8_t pil_resample_byte(const uint8_t *src, int64_t stride, const int32_t *k, int n) {
    int32_t acc = 1 << (PIL_PRECISION_BITS - 1);
    for (int x = 0; x < n; ++x) acc += (int32_t)src[x * stride] * k[x];
    acc >>= PIL_PRECISION_BITS;
    return (uint8_t)(acc < 0 ? 0 : acc > 255 ? 255 : acc);
}

inline bool pil_side_ok(int v) { return v >= 1 && v <= PIL_MAX_SIDE; }

inline double pil_support(int in, int out) {
    const double scale = (double)in / (double)out;
    return scale < 1.0 ? 1.0 : scale;
}

inline int pil_ksize(int in, int out) { return 2 * (int)ceil(pil_support(in, out)) + 1; }

// the taps' window of output xx: [xmin, xmin + n)
inline void pil_window(int in, int out, int xx, int *xmin, int *n) {
    const double scale = (double)in / (double)out, support = pil_support(in, out);
    const double center = (xx + 0.5) * scale;
    int lo = (int)(center - support + 0.5), hi = (int)(center + support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > in) hi = in;
    *xmin = lo;
    *n = hi - lo;
}

// table [out][PIL_ROW_HEAD + pil_ksize(in, out)]
inline void pil_build_table(int in, int out, int32_t *table) {
    const double scale = (double)in / (double)out, ss = 1.0 / pil_support(in, out);
    const int ksize = pil_ksize(in, out);
    double w[2 * PIL_MAX_SIDE + 1];
    for (int xx = 0; xx < out; ++xx) {
        int32_t *row = table + (int64_t)xx * (PIL_ROW_HEAD + ksize);
        const double center = (xx + 0.5) * scale;
        int xmin, n;
        pil_window(in, out, xx, &xmin, &n);
        double sum = 0.0;
        for (int x = 0; x < n; ++x) {
            const double t = fabs((x + xmin - center + 0.5) * ss);
            w[x] = t < 1.0 ? 1.0 - t : 0.0;
            sum += w[x];
        }
        row[0] = xmin;
        row[1] = n;
        for (int x = 0; x < ksize; ++x) {
            double v = x < n ? w[x] : 0.0;
            if (x < n && sum != 0.0) v /= sum;
            row[PIL_ROW_HEAD + x] = (int32_t)(0.5 + v * (double)(1 << PIL_PRECISION_BITS));
        }
    }
}

// The rows of the horizontal pass's result that the vertical pass reads: [*first, *first + *count) (the windows move monotonically)
inline void pil_rows_read(int in, int out, int *first, int *count) {
    int lo, n0, hi, n1;
    pil_window(in, out, 0, &lo, &n0);
    pil_window(in, out, out - 1, &hi, &n1);
    *first = lo;
    *count = hi + n1 - lo;
}
