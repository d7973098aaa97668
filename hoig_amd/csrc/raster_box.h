// The rasteriser's face binning, shared by raster_setup_kernel (raster.hip) and its CPU twin (raster_host.cpp): which 16 x 16-pixel
// tiles may hold a pixel that passes the reference's three edge tests for a face.  docs/raster_parity.md derives the criterion below.
//
// A pixel that passes the tests IN EXACT ARITHMETIC lies in the face, hence in the bounding box of its vertices: the box of tiles
// around it, with one pixel of slack for the roundings of the pixel <-> [-1,1] maps, holds it.  The tests run in fp32: each passes
// while the pixel is outside its edge by up to K |p - a| |e| (a: the edge's first vertex, e: the edge), K = (1 + 2^-24)^3 - 1.  For a
// face of longest edge L pixels and twice the area `den`, such a pixel leaves the vertices' bounding box by at most
// c L / (den / L^2 - c) pixels, c = 2 sqrt(2) K.  The face keeps its bounding box when den / L^2 > TAU (L + 1) with TAU = 2^-20 (1.88 c:
// at most 0.53 pixels, where the box excludes no pixel closer than 2); every other face -- a sliver, whose two long edges differ in
// direction by less than fp32 resolves, so that both tests pass along the whole line through it -- takes the whole image, the path
// of faces with non-finite vertices: there every pixel runs the reference's test, as in the reference.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RB_HD __host__ __device__
#else
#define RB_HD
#endif

constexpr int RB_TILE = 16;
constexpr unsigned RB_EMPTY_BOX = 0x00ff00ffu;        // tx0 = 255 > tx1 = 0: never overlaps
constexpr double RB_TAU = 1.0 / 1048576.0;            // 2^-20 = 16 u, u = 2^-24
constexpr double RB_MIN_EDGE2 = 8.271806125530277e-25;    // 2^-80 ([-1,1] units, squared): below it the tests' products may underflow

RB_HD inline bool raster_back_side(const float *f) {  // rasterize_cuda_kernel.cu:55,127
#pragma clang fp contract(off)
    return (f[7] - f[1]) * (f[3] - f[0]) < (f[4] - f[1]) * (f[6] - f[0]);
}

RB_HD inline unsigned raster_whole_image_box(int is) {
    const unsigned last = (unsigned)((is - 1) / RB_TILE);
    return 0u | (last << 8) | (0u << 16) | (last << 24);
}

// true when no pixel outside the vertices' bounding box (one pixel of slack) can pass the fp32 edge tests.  f: the face in [-1,1]
// units.  Doubles: the differences and products of fp32 values are then exact to 2^-53, and +, -, *, / and comparisons round the same
// way on the host and on the device.
RB_HD inline bool raster_edge_tests_stay_in_box(const float *f, int is) {
#pragma clang fp contract(off)
    const double ax = (double)f[3] - (double)f[0], ay = (double)f[4] - (double)f[1];      // A -> B
    const double bx = (double)f[6] - (double)f[3], by = (double)f[7] - (double)f[4];      // B -> C
    const double cx = (double)f[0] - (double)f[6], cy = (double)f[1] - (double)f[7];      // C -> A
    const double la = ax * ax + ay * ay, lb = bx * bx + by * by, lc = cx * cx + cy * cy;
    const double l2 = la > lb ? (la > lc ? la : lc) : (lb > lc ? lb : lc);                 // longest edge, squared
    const double den = ax * -cy - ay * -cx;                                                // (B - A) x (C - A): twice the area
    if (l2 == 0.) return true;                          // one point: every weight is 0 / 0, the face covers nothing anywhere
    if (!(l2 >= RB_MIN_EDGE2)) return false;            // (NaN and inf fall through to the comparison below, which they fail)
    const double r = den / (RB_TAU * l2) - 1.;          // den / L^2 > TAU (Lpx + 1), Lpx = sqrt(l2) is / 2, without the root
    return r > 0. && r * r > 0.25 * l2 * (double)is * (double)is;
}

// the packed tile box x0 | x1 << 8 | y0 << 16 | y1 << 24 of a front face
RB_HD inline unsigned raster_face_box(const float *f, int is) {
#pragma clang fp contract(off)
    float p[3][2];                                     // :59-63: [-1,1] -> [0, is-1]
    for (int n = 0; n < 3; ++n)
        for (int d = 0; d < 2; ++d) p[n][d] = (float)(0.5 * (f[3 * n + d] * is + is - 1));
    const bool finite = isfinite(p[0][0]) && isfinite(p[1][0]) && isfinite(p[2][0]) && isfinite(p[0][1]) && isfinite(p[1][1]) &&
                        isfinite(p[2][1]);
    if (!finite || !raster_edge_tests_stay_in_box(f, is)) return raster_whole_image_box(is);
    // bounding box in pixels (p is the pixel-space vertex), one pixel of slack, then in tiles
    const float lox = fminf(p[0][0], fminf(p[1][0], p[2][0])), hix = fmaxf(p[0][0], fmaxf(p[1][0], p[2][0]));
    const float loy = fminf(p[0][1], fminf(p[1][1], p[2][1])), hiy = fmaxf(p[0][1], fmaxf(p[1][1], p[2][1]));
    if (hix < -1.f || hiy < -1.f || lox > (float)is || loy > (float)is) return RB_EMPTY_BOX;
    const int fx = (int)floorf(fmaxf(lox, -1.f)) - 1, fy = (int)floorf(fmaxf(loy, -1.f)) - 1;
    const int cx = (int)ceilf(fminf(hix, (float)is)) + 1, cy = (int)ceilf(fminf(hiy, (float)is)) + 1;
    const int x0 = (fx > 0 ? fx : 0) / RB_TILE, y0 = (fy > 0 ? fy : 0) / RB_TILE;
    const int x1 = (cx < is - 1 ? cx : is - 1) / RB_TILE, y1 = (cy < is - 1 ? cy : is - 1) / RB_TILE;
    return (unsigned)x0 | ((unsigned)x1 << 8) | ((unsigned)y0 << 16) | ((unsigned)y1 << 24);
}
