// The serial part of a baseline / extended-sequential JPEG decode (ITU T.81 F.2.2, 8-bit samples, one interleaved Huffman scan), written
// ONCE for the device and for the host: the bit reader (removes the FF 00 stuffing), the symbol decode through an 8-bit lookahead table,
// the DC prediction and the block loop of one restart interval.  jpeg.hip runs it in lane 0 of a one-wave workgroup
// (jpeg_entropy_kernel); jpeg_host.cpp runs the same code on the CPU (hoig_jpeg_entropy_host), which is what the CPU suite pins.
//
// (jpeg_parallel.h builds the decode that is parallel inside an interval on the tables, the symbol decode and the geometry of this file.)
//
// What differs between the two is only WHERE bytes come from and where a finished block goes, and that is the `Ctx` parameter:
//   uint8_t  byte(int pos)        one byte of the scan data (pos < the interval's end: the reader never asks beyond it)
//   void     window(int pos)      called by EVERYONE between blocks: make [pos, pos + JPEG_BLOCK_MAX_BYTES) readable (device: the LDS window)
//   int16_t *stage()              called by everyone: 64 zeroed coefficients to decode into (in ZIGZAG order: the serial code looks
//                                 nothing up to place a coefficient)
//   bool     decoder()            does this caller run the serial code (device: lane 0)
//   int      share(int v)         the decoder's value, for everyone (device: a broadcast)
//   void     flush(int16_t *dst)  called by everyone: the staged block -> dst[jpeg_natural(k)] = staged[k], k = 0..63
//
// Bounds: every byte read is checked against the interval's end, a block decodes at most 64 symbols, an interval decodes exactly its
// block count, and a block that used bits past the interval's end is an error -- so a corrupt stream costs at most what a valid stream of
// its length costs, and touches nothing outside [begin, end) and its own blocks.
#pragma once
#include <stdint.h>
#include "hoig_kernels.h"

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__
#else
#define JPEG_HD
#endif

// one symbol is at most a 16-bit code + 15 magnitude bits, a block at most 64 symbols: 248 bytes, twice that with stuffing, plus the
// reader's 8 bytes of read-ahead
#define JPEG_BLOCK_MAX_BYTES 512

struct JpegHuff {
    uint16_t look[256];    // next 8 bits -> (code length << 8) | symbol; 0: the code is longer than 8 bits
    int32_t maxcode[18];   // largest code of each length (-1: none); [17] ends every search
    int32_t valoff[17];    // symbol index = code + valoff[length]
    uint8_t vals[256];
};

// zigzag position -> position in the 8 x 8 block (row-major)
JPEG_HD inline int jpeg_natural(int k) {
    const uint8_t order[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return order[k & 63];
}

// Canonical table (16 counts + values, T.81 annex C) -> decoding tables.  false: more values than `nvals_max`, or more codes of a length
// than that length has.
JPEG_HD inline bool jpeg_build_huff(const uint8_t *counts, const uint8_t *vals, int nvals_max, JpegHuff *h) {
    for (int i = 0; i < 256; ++i) h->look[i] = 0;
    for (int i = 0; i < 256; ++i) h->vals[i] = 0;
    int code = 0, p = 0;
    h->maxcode[0] = -1;
    h->valoff[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = counts[l - 1];
        h->valoff[l] = p - code;
        if (p + n > nvals_max) return false;
        for (int i = 0; i < n; ++i, ++code, ++p) {
            if (code >= (1 << l)) return false;
            h->vals[p] = vals[p];
            if (l <= 8) {
                const int first = code << (8 - l);
                for (int j = 0; j < (1 << (8 - l)); ++j) h->look[first + j] = (uint16_t)((l << 8) | vals[p]);
            }
        }
        h->maxcode[l] = n ? code - 1 : -1;
        code <<= 1;
    }
    h->maxcode[17] = 0x7fffffff;
    return true;
}

template <class Ctx>
struct JpegBits {
    Ctx *cx;
    uint64_t acc;   // the next `n` bits of the stream, right-aligned
    int n;
    int pos, end;   // next byte to read / the interval's end, both relative to the scan data
    int fake;       // zero bytes fed after the end (or in front of a marker): using one of them is an overrun

    JPEG_HD void init(Ctx *c, int begin, int end_) { cx = c; acc = 0; n = 0; pos = begin; end = end_; fake = 0; }
    JPEG_HD void fill() {
        if (n > 32) return;
        if (pos + 4 <= end) {                           // four bytes at once when none of them is an FF (four independent reads)
            const unsigned b0 = cx->byte(pos), b1 = cx->byte(pos + 1), b2 = cx->byte(pos + 2), b3 = cx->byte(pos + 3);
            if (b0 != 0xFF && b1 != 0xFF && b2 != 0xFF && b3 != 0xFF) {
                acc = (acc << 32) | (uint64_t)((b0 << 24) | (b1 << 16) | (b2 << 8) | b3);
                n += 32;
                pos += 4;
                return;
            }
        }
        while (n <= 56) {
            unsigned b = 0;
            if (pos < end) {
                b = cx->byte(pos);
                if (b == 0xFF) {
                    if (pos + 1 < end && cx->byte(pos + 1) == 0) pos += 2;      // a stuffed FF
                    else { b = 0; ++fake; }                                      // a marker (or a cut FF): the data ends here
                } else ++pos;
            } else ++fake;
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    JPEG_HD unsigned peek(int k) const { return (unsigned)(acc >> (n - k)) & ((1u << k) - 1u); }
    JPEG_HD void drop(int k) { n -= k; }
    JPEG_HD bool overran() const { return n < fake * 8; }
    // bytes of the interval nobody has read, plus whole bytes waiting in the accumulator
    JPEG_HD int unread() const { return (end - pos) + (n - fake * 8) / 8; }
};

// one Huffman symbol; -1: no code of 16 bits or fewer matches  (Bits: JpegBits, or jpeg_parallel.h's reader)
template <class Bits>
JPEG_HD inline int jpeg_symbol(Bits &br, const JpegHuff *h) {
    const unsigned e = h->look[br.peek(8)];
    if (e) {
        br.drop((int)(e >> 8));
        return (int)(e & 255u);
    }
    int l = 9;
    int code = (int)br.peek(9);
    while (l <= 16 && code > h->maxcode[l]) {
        ++l;
        code = (int)br.peek(l > 16 ? 16 : l);
    }
    if (l > 16) return -1;
    br.drop(l);
    return h->vals[(code + h->valoff[l]) & 255];
}

// T.81 F.2.2.1 EXTEND: s magnitude bits -> the signed value
JPEG_HD inline int jpeg_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// One block: its coefficients (zigzag order, NOT dequantised) into blk[64] (zeroed by the caller).  0 or a HOIG_JPEG_E* bit.
template <class Ctx>
JPEG_HD inline int jpeg_decode_block(JpegBits<Ctx> &br, const JpegHuff *dc, const JpegHuff *ac, int *pred, int16_t *blk) {
    br.fill();
    int s = jpeg_symbol(br, dc);
    if (s < 0 || s > 15) return HOIG_JPEG_ECODE;
    if (s) {
        const int v = (int)br.peek(s);
        br.drop(s);
        *pred += jpeg_extend(v, s);
    }
    blk[0] = (int16_t)*pred;
    for (int k = 1; k < 64;) {
        br.fill();
        const int rs = jpeg_symbol(br, ac);
        if (rs < 0) return HOIG_JPEG_ECODE;
        const int r = rs >> 4;
        s = rs & 15;
        if (s) {
            k += r;
            if (k > 63) return HOIG_JPEG_ECODE;
            const int v = (int)br.peek(s);
            br.drop(s);
            blk[k] = (int16_t)jpeg_extend(v, s);
            ++k;
        } else if (r == 15) {
            k += 16;
            if (k > 64) return HOIG_JPEG_ECODE;
        } else
            break;
    }
    return br.overran() ? HOIG_JPEG_EOVERRUN : 0;
}

// Geometry of a plan: MCU grid and, per component, the blocks of its padded plane and where they start in the coefficient workspace.
struct JpegGeom {
    int mcux, mcuy;
    int h[3], v[3];       // blocks of component c in an MCU
    int bw[3], bh[3];     // blocks per row / column of the padded plane
    int64_t first[3];     // index of the component's first block among the image's blocks
    int64_t blocks;
};

JPEG_HD inline JpegGeom jpeg_geometry(const hoig_jpeg_plan &P) {
    JpegGeom g;
    const int hs = P.ncomp == 1 ? 1 : P.hs, vs = P.ncomp == 1 ? 1 : P.vs;
    g.mcux = (P.width + 8 * hs - 1) / (8 * hs);
    g.mcuy = (P.height + 8 * vs - 1) / (8 * vs);
    int64_t at = 0;
    for (int c = 0; c < 3; ++c) {
        g.h[c] = c == 0 ? hs : 1;
        g.v[c] = c == 0 ? vs : 1;
        g.bw[c] = c < P.ncomp ? g.mcux * g.h[c] : 0;
        g.bh[c] = c < P.ncomp ? g.mcuy * g.v[c] : 0;
        g.first[c] = at;
        at += (int64_t)g.bw[c] * g.bh[c];
    }
    g.blocks = at;
    return g;
}

// What a caller may put into a plan (everything the kernels index with): sizes, sampling, table selectors' ranges.
JPEG_HD inline bool jpeg_plan_sane(const hoig_jpeg_plan &P) {
    if (P.width < 1 || P.height < 1 || P.width > 65535 || P.height > 65535) return false;
    if (P.ncomp != 1 && P.ncomp != 3) return false;
    if (P.ncomp == 3 && !((P.hs == 1 && P.vs == 1) || (P.hs == 2 && P.vs == 1) || (P.hs == 2 && P.vs == 2))) return false;
    if (P.data_off < 0 || P.data_len < 0 || P.restart_interval < 0 || P.n_intervals < 1 || P.interval_first < 0) return false;
    const JpegGeom g = jpeg_geometry(P);
    const int64_t mcus = (int64_t)g.mcux * g.mcuy;
    const int64_t want = P.restart_interval ? (mcus + P.restart_interval - 1) / P.restart_interval : 1;
    return P.n_intervals == want;
}

// Restart interval `iv` of one image: its blocks, in scan order, into coef (the image's coefficient blocks: [component][block row]
// [block column][64]).  `intervals` holds n_intervals + 1 offsets relative to the scan data: where each interval starts, then where the
// data ends; between two intervals sits the marker RSTm, m = iv mod 8.  Returns 0 or HOIG_JPEG_E* bits (the same value for every caller).
template <class Ctx>
JPEG_HD inline int jpeg_decode_interval(const hoig_jpeg_plan &P, const JpegHuff *dc, const JpegHuff *ac, const int32_t *intervals,
                                        int iv, int16_t *coef, Ctx &cx) {
    const JpegGeom g = jpeg_geometry(P);
    const int begin = intervals[iv], stop = intervals[iv + 1];
    const bool last = iv + 1 == P.n_intervals;
    // an interval ends in front of its RST marker (2 bytes), the last one where the data ends
    const int end = last ? stop : stop - 2;
    if (begin < 0 || end < begin || stop > P.data_len) return HOIG_JPEG_EMARKER;
    int err = 0;
    if (!last) cx.window(end);
    if (cx.decoder() && !last && (cx.byte(end) != 0xFF || cx.byte(end + 1) != (0xD0 | (iv & 7)))) err = HOIG_JPEG_EMARKER;
    err = cx.share(err);
    if (err) return err;
    const int64_t mcus = (int64_t)g.mcux * g.mcuy;
    const int64_t m0 = P.restart_interval ? (int64_t)iv * P.restart_interval : 0;
    const int64_t m1 = P.restart_interval && m0 + P.restart_interval < mcus ? m0 + P.restart_interval : mcus;
    JpegBits<Ctx> br;
    br.init(&cx, begin, end);
    int pred[3] = {0, 0, 0};
    const int ncomp = P.ncomp;
    for (int64_t m = m0; m < m1; ++m) {
        const int mx = (int)(m % g.mcux), my = (int)(m / g.mcux);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll                                          // (c a constant: g's and pred's entries stay in registers)
#endif
        for (int c = 0; c < 3; ++c) {
            if (c >= ncomp) break;
            for (int y = 0; y < g.v[c]; ++y)
                for (int x = 0; x < g.h[c]; ++x) {
                    cx.window(cx.share(br.pos));
                    int16_t *blk = cx.stage();
                    if (cx.decoder()) err = jpeg_decode_block(br, dc + c, ac + c, pred + c, blk);
                    err = cx.share(err);
                    if (err) return err;
                    cx.flush(coef + (g.first[c] + (int64_t)(my * g.v[c] + y) * g.bw[c] + (mx * g.h[c] + x)) * 64);
                }
        }
    }
    // an encoder pads the last byte with 1-bits and puts the marker right behind it: a whole byte left over means the stream and the
    // block count disagree
    if (cx.decoder() && br.unread() > 0) err = HOIG_JPEG_ETRAILING;
    return cx.share(err);
}
