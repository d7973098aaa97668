// Parallel Huffman decode INSIDE a restart interval, by self-synchronising sub-sequences (Klein & Wiseman 2003; Weissenberger & Schmidt,
// ICPP 2018 / 2021: PAPERS.md), written ONCE for the device (jpeg.hip: jpeg_entropy_par_kernel, a workgroup per image and interval)
// and for the host (jpeg_host.cpp: hoig_jpeg_entropy_par_host, which walks the lanes of that workgroup one after the other).
//
// An interval's bytes are cut into sub-sequences of S RAW bytes (stuffing included), `lanes` of them form a chunk, and a lane owns one
// sub-sequence of the chunk.  A sub-sequence's START STATE is (bit offset of the first symbol that starts in it, block within the MCU,
// zigzag position k; k = 0: a DC symbol is next).  Sub-sequence 0 of the interval starts at (0, 0, 0); every other lane guesses.
//   rounds  a lane whose state changed decodes -- writing nothing -- until a symbol would start at or behind its boundary: that is the
//           candidate state of its neighbour, which takes it if it differs and decodes again.  After round r the state of sub-sequence
//           r is final, so a chunk needs at most as many rounds as it has sub-sequences, and the fixed point is the serial decode.  A
//           bad code, a marker or the end of the data met on the way only mean "no candidate".
//   scan    exclusive prefix sums of the blocks each lane COMPLETED and of its DC differences per component: the ordinal (in scan
//           order) of the block a lane starts in, and its DC predictors.
//   write   every lane decodes once more from its final state and stores the coefficients; a lane that starts inside a block goes on
//           with the block its neighbour began, so the coefficients must have been zeroed.  The chunk's last candidate, block count
//           and predictors carry into the next chunk.
// Anything irregular in the write pass (no candidate from a final state, a block count that does not come out, whole bytes left over,
// an overrun, a restart marker that is not there) makes the interval IRREGULAR: the function returns 1 and the caller runs the serial
// jpeg_decode_interval on it, which writes every block again and produces the status word.  A regular interval is exactly one on which
// the serial code returns 0 with the same coefficients.
//
// The `Ctx` parameter (everything is called by EVERY lane, in the same order):
//   uint8_t  byte(int pos)            one byte of the scan data, pos inside the range last staged and below the interval's stop
//   void     stage(int pos0, int pos1) make [pos0, pos1) readable (device: the LDS copy of the chunk)
//   int      first(), step()          the lanes this caller runs: first(), first() + step(), ...   (host: 0, 1 -- all of them)
//   void     barrier()                everything written before it is visible to every lane after it
//   bool     any(bool v)              a barrier, and whether v held for any caller
//   JpegParTab *tab()                 the chunk's tables: one entry per lane, and `carry`
//
// Bounds: a lane reads bytes below the interval's end only (JpegRawBits checks every byte), at most 26 bytes behind its boundary (one
// symbol of 31 bits, the reader's 8 bytes of read-ahead, all of them stuffed); it decodes at most one symbol per bit of its
// sub-sequence; a chunk runs at most as many rounds as it has lanes (the driver counts them: one more makes the interval irregular); table indices are masked as in jpeg_symbol; the write pass stores
// to block ordinals below the interval's block count only, i.e. inside the image's coefficient blocks.
#pragma once
#include "jpeg_entropy.h"

#define JPEG_PAR_NONE 0xffffffffu
#define JPEG_PAR_OVER 64          // bytes staged behind a chunk (26 are needed, see above)

JPEG_HD inline bool jpeg_par_subseq_ok(int s) { return s == 32 || s == 64 || s == 128 || s == 256; }

// sub-sequences of interval `iv` (0: its offsets are not inside the data, or it is empty -- the serial code reports such an interval)
JPEG_HD inline int jpeg_par_nsub(const hoig_jpeg_plan &P, const int32_t *intervals, int iv, int S) {
    const int begin = intervals[iv], stop = intervals[iv + 1];
    const int end = iv + 1 == P.n_intervals ? stop : stop - 2;
    if (begin < 0 || end <= begin || stop > P.data_len) return 0;
    return (int)(((int64_t)(end - begin) + S - 1) / S);
}

// What the parallel decoder keeps in the workspace behind the planes: one int32 per entry of the `intervals` array, "this interval is
// irregular".  -> the first byte of that table and its entries, from plans whose coef_off / plane_off are laid out.
inline void jpeg_par_tables(const hoig_jpeg_plan *plans, int n, int64_t *off, int64_t *entries) {
    int64_t at = 0, m = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t e = plans[i].plane_off + jpeg_geometry(plans[i]).blocks * 64;
        const int64_t k = (int64_t)plans[i].interval_first + plans[i].n_intervals + 1;
        at = e > at ? e : at;
        m = k > m ? k : m;
    }
    *off = (at + 15) & ~(int64_t)15;
    *entries = m;
}

JPEG_HD inline uint32_t jpeg_par_pack(int bit, int blk, int k) { return ((uint32_t)bit << 9) | ((uint32_t)blk << 6) | (uint32_t)k; }
JPEG_HD inline int jpeg_par_bit(uint32_t st) { return (int)(st >> 9); }
JPEG_HD inline int jpeg_par_blk(uint32_t st) { return (int)(st >> 6) & 7; }
JPEG_HD inline int jpeg_par_k(uint32_t st) { return (int)st & 63; }

JPEG_HD inline int jpeg_par_popcount8(unsigned v) {
    v = (v & 0x55u) + ((v >> 1) & 0x55u);
    v = (v & 0x33u) + ((v >> 2) & 0x33u);
    return (int)((v + (v >> 4)) & 0x0fu);
}

// JpegBits with the RAW position of the next bit: beside the accumulator it keeps, per byte loaded, whether a stuffed 00 followed it.
// Bytes behind the end (or behind a marker, which ends the data) are zeros that still count as positions, so that head() > 8 * end
// says "used bits that are not there".
template <class Ctx>
struct JpegRawBits {
    Ctx *cx;
    uint64_t acc;
    int n;
    int pos, end;
    unsigned stuffed;   // bit j: the byte loaded j loads ago was an FF followed by its 00
    bool marker;        // an FF that no 00 follows was met: the interval is irregular

    JPEG_HD void init(Ctx *c, int begin, int end_) { cx = c; acc = 0; n = 0; pos = begin; end = end_; stuffed = 0; marker = false; }
    JPEG_HD void fill() {
        if (n > 32) return;
        if (pos + 4 <= end) {
            const unsigned b0 = cx->byte(pos), b1 = cx->byte(pos + 1), b2 = cx->byte(pos + 2), b3 = cx->byte(pos + 3);
            if (b0 != 0xFF && b1 != 0xFF && b2 != 0xFF && b3 != 0xFF) {
                acc = (acc << 32) | (uint64_t)((b0 << 24) | (b1 << 16) | (b2 << 8) | b3);
                n += 32;
                pos += 4;
                stuffed <<= 4;
                return;
            }
        }
        while (n <= 56) {
            unsigned b = 0, two = 0;
            if (pos < end) {
                b = cx->byte(pos);
                if (b == 0xFF) {
                    if (pos + 1 < end && cx->byte(pos + 1) == 0) two = 1;
                    else { b = 0; marker = true; end = pos; }
                }
            }
            pos += 1 + (int)two;
            acc = (acc << 8) | b;
            n += 8;
            stuffed = (stuffed << 1) | two;
        }
    }
    JPEG_HD unsigned peek(int k) const { return (unsigned)(acc >> (n - k)) & ((1u << k) - 1u); }
    JPEG_HD void drop(int k) { n -= k; }
    // raw bit position (relative to the scan data) of the next bit; fill() does not change it
    JPEG_HD int head() const {
        const int k = (n + 7) >> 3;
        return (pos - k - jpeg_par_popcount8(stuffed & ((1u << k) - 1u))) * 8 + ((8 - (n & 7)) & 7);
    }
};

struct JpegParTab {
    uint32_t *state, *cand;          // start state of the lane's sub-sequence / the candidate it found for its neighbour
    int32_t *dirty;                  // the state changed: decode again
    int32_t *nblk, *dc0, *dc1, *dc2; // completed blocks and DC sums of the last decode; after the scan: their exclusive prefix sums
    int32_t *carry;                  // [6]: block ordinal, three predictors, first state of the next chunk, "the last block ended well"
};

struct JpegParRun {
    uint32_t next;                   // the neighbour's candidate state, JPEG_PAR_NONE: none
    int nblk, dc0, dc1, dc2;
    bool bad, finished;
};

// index of a block among the image's coefficient blocks: MCU m, block `blk` of the MCU (n0 = blocks of component 0 in an MCU)
JPEG_HD inline int64_t jpeg_par_block_index(const JpegGeom &g, int64_t m, int blk, int n0) {
    const int c = blk < n0 ? 0 : blk - n0 + 1;
    const int hc = c ? 1 : g.h[0], vc = c ? 1 : g.v[0];
    const int j = c ? 0 : blk;
    const int y = j / hc, x = j - y * hc;
    const int bw = c == 0 ? g.bw[0] : (c == 1 ? g.bw[1] : g.bw[2]);
    const int64_t first = c == 0 ? g.first[0] : (c == 1 ? g.first[1] : g.first[2]);
    const int mx = (int)(m % g.mcux), my = (int)(m / g.mcux);
    return first + (int64_t)(my * vc + y) * bw + (mx * hc + x);
}

// One sub-sequence from state `st`: symbols that START in [startbit, limitbit) -- raw bit positions relative to the scan data; endbit:
// the interval's end.  WRITE: the lane's first block has ordinal `ord` within the interval (whose first MCU is m0 and which holds
// ord_end blocks), its predictors are p0..p2, and coefficients go to coef (the image's blocks).
template <bool WRITE, class Ctx>
JPEG_HD inline JpegParRun jpeg_par_subseq(Ctx &cx, const JpegHuff *dc, const JpegHuff *ac, int n0, int bpm, int startbit, int limitbit,
                                          int endbit, uint32_t st, const JpegGeom &g, int64_t m0, int64_t ord, int64_t ord_end, int p0,
                                          int p1, int p2, int16_t *coef) {
    JpegParRun r;
    r.next = JPEG_PAR_NONE;
    r.nblk = 0; r.dc0 = 0; r.dc1 = 0; r.dc2 = 0;
    r.bad = false; r.finished = false;
    int blk = jpeg_par_blk(st), k = jpeg_par_k(st);
    if (blk >= bpm) { r.bad = true; return r; }
    int16_t *dst = nullptr;
    if (WRITE) {
        if (ord >= ord_end) return r;
        if ((int)(ord % bpm) != blk) { r.bad = true; return r; }
        dst = coef + jpeg_par_block_index(g, m0 + ord / bpm, blk, n0) * 64;
    }
    JpegRawBits<Ctx> br;
    br.init(&cx, startbit >> 3, endbit >> 3);
    br.fill();
    br.drop(startbit & 7);
    br.fill();
    int at = br.head();
    for (;;) {
        if (at >= limitbit) {
            r.next = jpeg_par_pack(at - limitbit, blk, k);
            break;
        }
        const int c = blk < n0 ? 0 : blk - n0 + 1;
        const bool isdc = k == 0;
        bool done = false, store = false;
        int value = 0, where = 0;
        if (isdc) {
            const int s = jpeg_symbol(br, dc + c);
            if (s < 0 || s > 15) { r.bad = true; break; }
            if (s) {
                const int v = (int)br.peek(s);
                br.drop(s);
                value = jpeg_extend(v, s);
            }
            k = 1;
        } else {
            const int rs = jpeg_symbol(br, ac + c);
            if (rs < 0) { r.bad = true; break; }
            const int run = rs >> 4, s = rs & 15;
            if (s) {
                k += run;
                if (k > 63) { r.bad = true; break; }
                const int v = (int)br.peek(s);
                br.drop(s);
                value = jpeg_extend(v, s);
                where = k;
                store = true;
                ++k;
            } else if (run == 15) {
                k += 16;
                if (k > 64) { r.bad = true; break; }
            } else
                done = true;
            if (k == 64) done = true;
        }
        at = br.head();
        if (at > endbit || br.marker) { r.bad = true; break; }       // the symbol used bits that are not there
        if (isdc) {
            // unsigned sums: they wrap as the serial code's int predictor does on the machines this runs on, without the undefined behaviour
            if (c == 0) { r.dc0 = (int)((unsigned)r.dc0 + (unsigned)value); p0 = (int)((unsigned)p0 + (unsigned)value); }
            else if (c == 1) { r.dc1 = (int)((unsigned)r.dc1 + (unsigned)value); p1 = (int)((unsigned)p1 + (unsigned)value); }
            else { r.dc2 = (int)((unsigned)r.dc2 + (unsigned)value); p2 = (int)((unsigned)p2 + (unsigned)value); }
            if (WRITE) dst[0] = (int16_t)(c == 0 ? p0 : (c == 1 ? p1 : p2));
        } else if (WRITE && store)
            dst[jpeg_natural(where)] = (int16_t)value;
        if (done) {
            k = 0;
            blk = blk + 1 == bpm ? 0 : blk + 1;
            ++r.nblk;
            if (WRITE) {
                ++ord;
                if (ord == ord_end) {
                    // the serial code's end of an interval: no whole byte may be left in front of the marker
                    if (endbit - at >= 8) r.bad = true;
                    else r.finished = true;
                    break;
                }
                dst = coef + jpeg_par_block_index(g, m0 + ord / bpm, blk, n0) * 64;
            }
        }
        br.fill();
    }
    return r;
}

// Restart interval `iv` of one image with sub-sequences of S bytes in chunks of `lanes`; arguments as jpeg_decode_interval.  Returns 0:
// every block of the interval is in coef (which was ZERO before); 1: irregular, the caller runs jpeg_decode_interval on it.  The same
// value for every caller.  rounds (optional): the decode rounds of all chunks are added to it.  states (optional): the final table, four
// entries per sub-sequence (bit offset, block in MCU, k, completed blocks).
template <class Ctx>
JPEG_HD inline int jpeg_par_interval(const hoig_jpeg_plan &P, const JpegHuff *dc, const JpegHuff *ac, const int32_t *intervals, int iv,
                                     int16_t *coef, int S, int lanes, Ctx &cx, int32_t *rounds, int32_t *states) {
    const JpegGeom g = jpeg_geometry(P);
    const int begin = intervals[iv], stop = intervals[iv + 1];
    const bool last = iv + 1 == P.n_intervals;
    const int end = last ? stop : stop - 2;
    const int nsub = jpeg_par_nsub(P, intervals, iv, S);
    if (nsub == 0) return 1;
    const int64_t mcus = (int64_t)g.mcux * g.mcuy;
    const int64_t m0 = P.restart_interval ? (int64_t)iv * P.restart_interval : 0;
    const int64_t m1 = P.restart_interval && m0 + P.restart_interval < mcus ? m0 + P.restart_interval : mcus;
    const int n0 = g.h[0] * g.v[0], bpm = P.ncomp == 3 ? n0 + 2 : 1;
    const int64_t nblocks = (m1 - m0) * bpm;
    JpegParTab *T = cx.tab();
    if (cx.first() == 0) {
        T->carry[0] = 0; T->carry[1] = 0; T->carry[2] = 0; T->carry[3] = 0;
        T->carry[4] = (int32_t)jpeg_par_pack(0, 0, 0);
        T->carry[5] = 0;
    }
    bool irregular = false;
    for (int c0 = 0; c0 < nsub; c0 += lanes) {
        const int nl = nsub - c0 < lanes ? nsub - c0 : lanes;
        const int cb = begin + c0 * S;
        const int ce = cb + nl * S < end ? cb + nl * S : end;
        cx.stage(cb, ce + JPEG_PAR_OVER < stop ? ce + JPEG_PAR_OVER : stop);     // (stage() is a barrier: the carry is visible)
        if ((uint32_t)T->carry[4] == JPEG_PAR_NONE) return 1;                  // the previous chunk found no way into this one
        for (int l = cx.first(); l < nl; l += cx.step()) {
            const int p = cb + l * S;
            // a sub-sequence that begins with the 00 of an FF 00 pair: no symbol starts there
            T->state[l] = l == 0 ? (uint32_t)T->carry[4] : jpeg_par_pack(cx.byte(p) == 0 && cx.byte(p - 1) == 0xFF ? 8 : 0, 0, 0);
            T->dirty[l] = 1;
        }
        bool changed;
        int round = 0;
        do {
            if (round++ == nl) return 1;                                        // (cannot happen: state r is final after round r)
            for (int l = cx.first(); l < nl; l += cx.step()) {
                if (!T->dirty[l]) continue;
                const int p = cb + l * S;
                const int limit = p + S < end ? p + S : end;
                const JpegParRun r = jpeg_par_subseq<false>(cx, dc, ac, n0, bpm, p * 8 + jpeg_par_bit(T->state[l]), limit * 8, end * 8,
                                                            T->state[l], g, m0, 0, 0, 0, 0, 0, nullptr);
                T->cand[l] = r.next;
                T->nblk[l] = r.nblk; T->dc0[l] = r.dc0; T->dc1[l] = r.dc1; T->dc2[l] = r.dc2;
                T->dirty[l] = 0;
            }
            cx.barrier();
            changed = false;
            for (int l = cx.first(); l < nl; l += cx.step()) {
                if (l == 0) continue;
                const uint32_t c = T->cand[l - 1];
                if (c != JPEG_PAR_NONE && c != T->state[l]) {
                    T->state[l] = c;
                    T->dirty[l] = 1;
                    changed = true;
                }
            }
            if (rounds && cx.first() == 0) ++*rounds;
            changed = cx.any(changed);
        } while (changed);
        if (states)
            for (int l = cx.first(); l < nl; l += cx.step()) {
                int32_t *s = states + (int64_t)(c0 + l) * 4;
                s[0] = jpeg_par_bit(T->state[l]); s[1] = jpeg_par_blk(T->state[l]); s[2] = jpeg_par_k(T->state[l]); s[3] = T->nblk[l];
            }
        if (cx.first() == 0) {                                                  // the scan: a chunk has a few hundred entries
            unsigned ord = (unsigned)T->carry[0], a = (unsigned)T->carry[1], b = (unsigned)T->carry[2], c = (unsigned)T->carry[3];
            for (int l = 0; l < nl; ++l) {
                const unsigned t = (unsigned)T->nblk[l], ta = (unsigned)T->dc0[l], tb = (unsigned)T->dc1[l], tc = (unsigned)T->dc2[l];
                T->nblk[l] = (int32_t)ord; T->dc0[l] = (int32_t)a; T->dc1[l] = (int32_t)b; T->dc2[l] = (int32_t)c;
                ord += t; a += ta; b += tb; c += tc;
            }
            T->carry[0] = (int32_t)ord; T->carry[1] = (int32_t)a; T->carry[2] = (int32_t)b; T->carry[3] = (int32_t)c;
            T->carry[4] = (int32_t)T->cand[nl - 1];
        }
        cx.barrier();
        bool bad = false;
        for (int l = cx.first(); l < nl; l += cx.step()) {
            const int64_t ord = (uint32_t)T->nblk[l];
            if (ord >= nblocks) continue;
            const int p = cb + l * S;
            const int limit = p + S < end ? p + S : end;
            const JpegParRun r = jpeg_par_subseq<true>(cx, dc, ac, n0, bpm, p * 8 + jpeg_par_bit(T->state[l]), limit * 8, end * 8,
                                                       T->state[l], g, m0, ord, nblocks, T->dc0[l], T->dc1[l], T->dc2[l], coef);
            bad = bad || r.bad;
            if (r.finished) T->carry[5] = 1;
        }
        if (ce == end && !last && (cx.byte(end) != 0xFF || cx.byte(end + 1) != (0xD0 | (iv & 7)))) bad = true;
        irregular = cx.any(bad) || irregular;
        if (irregular) return 1;
    }
    return T->carry[5] ? 0 : 1;
}
