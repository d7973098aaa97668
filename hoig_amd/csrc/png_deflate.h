// The per-lane code of the PNG encoder (docs/png_encode.md), shared by its kernels (png.hip) and their CPU twins (png_host.cpp): the
// row filter, and one deflate block per segment of the filtered stream.  A workgroup of PNG_LANES lanes runs a segment as a list of
// PHASES with a barrier between two of them; a phase is a function of (context, lane).  The kernel calls it with its thread index,
// the twin walks the lanes in a loop, so both run the same statements on the same data.  Whatever lanes of one phase share is
// combined with atomicMax / atomicAdd / atomicOr only: the result never depends on the order in which lanes or workgroups ran.
//
// Integer only.  The output of a segment: [dynamic-Huffman block | stored block of the raw bytes, whichever is not larger] then an
// empty stored block (which ends on a byte boundary and carries BFINAL on the last segment).
#pragma once
#include <stdint.h>
#include "hoig_kernels.h"

#if defined(__HIPCC__)
#define PNG_HD __host__ __device__
#else
#define PNG_HD
#endif

// How lanes combine: device atomics in a kernel, plain statements in the twin (which runs one lane at a time).
#if defined(__HIP_DEVICE_COMPILE__)
#define PNG_ATOMIC_MAX(p, v) atomicMax((p), (v))
#define PNG_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#define PNG_ATOMIC_OR(p, v) atomicOr((p), (v))
// words that other lanes of the workgroup completed with atomicOr: read where the atomics landed, past this CU's vector cache
#define PNG_LOAD_SHARED_WORD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#else
#define PNG_ATOMIC_MAX(p, v) (*(p) = *(p) < (v) ? (v) : *(p))
#define PNG_ATOMIC_ADD(p, v) (*(p) += (v))
#define PNG_ATOMIC_OR(p, v) (*(p) |= (v))
#define PNG_LOAD_SHARED_WORD(p) (*(p))
#endif

#define PNG_LANES 256
#define PNG_HASH_BITS 12
#define PNG_HASH_BACK 8192        // positions in front of a segment that its hash table knows
#define PNG_MAX_DIST 32768
#define PNG_MIN_MATCH 3
#define PNG_MAX_MATCH 258
#define PNG_NLIT 286
#define PNG_NDIST 30
#define PNG_NCLC 19
#define PNG_SIG_IHDR 33           // signature + IHDR chunk
#define PNG_SEG_FRAME 12          // length, type, CRC of one chunk
#define PNG_SLOT_PAD 32           // a segment's slot: segment_bytes + this (stored block 5 + n, empty block 5, rounded to words)

PNG_HD inline bool png_segment_ok(int s) { return s == 4096 || s == 8192 || s == 16384 || s == 32768; }
PNG_HD inline int64_t png_row_stride(int W, int C) { return 1 + (int64_t)W * C; }
PNG_HD inline int64_t png_nseg(int64_t n, int S) { return n <= 0 ? 1 : (n + S - 1) / S; }
// A file is at most: signature + IHDR, per segment its frame + 10 bytes of stored-block headers + its bytes, the zlib header, the
// Adler-32 chunk and IEND
PNG_HD inline int64_t png_file_bound(int64_t n, int S) { return PNG_SIG_IHDR + n + png_nseg(n, S) * (PNG_SEG_FRAME + 10) + 2 + 16 + 12; }
PNG_HD inline int64_t png_zlib_bound(int64_t n, int S) { return 2 + n + png_nseg(n, S) * 10 + 4; }

// ---------------------------------------------------------------------------------------------------------------- the row filter

PNG_HD inline int png_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

// filter `type` of raw byte x with a = left pixel, b = above, c = above left (0 outside the image)
PNG_HD inline uint8_t png_filter_byte(int type, int x, int a, int b, int c) {
    switch (type) {
        case 0: return (uint8_t)x;
        case 1: return (uint8_t)(x - a);
        case 2: return (uint8_t)(x - b);
        case 3: return (uint8_t)(x - ((a + b) >> 1));
        default: return (uint8_t)(x - png_paeth(a, b, c));
    }
}

PNG_HD inline uint32_t png_abs_s8(uint8_t v) { return v < 128 ? v : 256u - v; }

// byte j of row y of one image (rows of `rowlen` = W * C bytes), its three neighbours
PNG_HD inline void png_neighbours(const uint8_t *img, int y, int64_t j, int64_t rowlen, int C, int *x, int *a, int *b, int *c) {
    const uint8_t *row = img + (int64_t)y * rowlen;
    *x = row[j];
    *a = j >= C ? row[j - C] : 0;
    *b = y > 0 ? row[j - rowlen] : 0;
    *c = (y > 0 && j >= C) ? row[j - rowlen - C] : 0;
}

// the smallest of the five sums wins, a tie goes to the lowest type
PNG_HD inline int png_pick_filter(const uint64_t *sums) {
    int best = 0;
    for (int t = 1; t < 5; ++t)
        if (sums[t] < sums[best]) best = t;
    return best;
}

// ------------------------------------------------------------------------------------------------- symbols of lengths and distances

PNG_HD inline int png_log2(uint32_t v) { return 31 - __builtin_clz(v); }

PNG_HD inline void png_len_symbol(int len, int *sym, int *ebits, int *extra) {
    const int l = len - 3;
    if (len == 258) {
        *sym = 285, *ebits = 0, *extra = 0;
    } else if (l < 8) {
        *sym = 257 + l, *ebits = 0, *extra = 0;
    } else {
        const int eb = png_log2((uint32_t)l) - 2;
        *sym = 261 + 4 * eb + ((l >> eb) & 3), *ebits = eb, *extra = l & ((1 << eb) - 1);
    }
}

PNG_HD inline void png_dist_symbol(int dist, int *sym, int *ebits, int *extra) {
    const int d = dist - 1;
    if (d < 4) {
        *sym = d, *ebits = 0, *extra = 0;
    } else {
        const int k = png_log2((uint32_t)d);
        *sym = 2 * k + ((d >> (k - 1)) & 1), *ebits = k - 1, *extra = d & ((1 << (k - 1)) - 1);
    }
}

PNG_HD inline uint32_t png_reverse_bits(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// ------------------------------------------------------------------------------------------------------------------ checksums

PNG_HD inline uint32_t png_crc_entry(uint32_t i) {
    for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ 0xEDB88320u : i >> 1;
    return i;
}

// a * b in GF(2)[x] / CRC-32's polynomial, both bit-reflected (bit 31 is x^0)
PNG_HD inline uint32_t png_gf2_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        if ((a >> i) & 1u) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}

// a small message's standard CRC-32, bit by bit (chunk headers of a few bytes)
PNG_HD inline uint32_t png_crc_small(const uint8_t *p, int n) {
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 0; i < n; ++i) c = png_crc_entry((c ^ p[i]) & 0xFFu) ^ (c >> 8);
    return ~c;
}

#define PNG_ADLER 65521u

// -------------------------------------------------------------------------------------------------------- one segment's working set

struct PngSegShared {                   // LDS in the kernel
    uint32_t crc_tab[256];
    uint32_t hash[1 << PNG_HASH_BITS];  // position + 1 of the latest 3-byte string with this hash (0: none)
    uint32_t lfreq[288], dfreq[32], cfreq[20];
    uint16_t lsorted[288], dsorted[32], csorted[20];   // used symbols, ascending (frequency, symbol)
    uint8_t llen[288], dlen[32], clen[20];
    uint16_t lcode[288], dcode[32], ccode[20];         // bit-reversed: ready to go out LSB first
    uint32_t nfreq[576];                // the Huffman tree being merged: leaves then internal nodes
    uint16_t nparent[576], ndepth[576];
    uint8_t hdr_sym[320], hdr_extra[320];              // the code-length sequence of the block header, zero runs as 17 / 18
    uint32_t lane_bits[PNG_LANES];      // bits of each lane's tokens, then their exclusive prefix sum
    uint32_t lane_crc[PNG_LANES];
    uint16_t lit_cost[256];             // what a literal of each byte value is expected to cost, in 1/8 bit
    uint32_t lused, dused, cused;
    uint32_t ntok, hdr_n, hlit, hdist, hclen, hdr_bits, body_bits, stored, out_bytes;
    uint32_t adler_a, adler_b, crc_len, crc_chunk;
};

struct PngSegRecord {                   // what the assemble stage reads of a segment
    uint32_t bytes, crc, adler_a, adler_b;
};

struct PngSegCtx {
    PngSegShared *sh;
    uint16_t *mlen;            // [n] match length at each position, 0: none (LDS in the kernel)
    uint16_t *mdist;           // [n] its distance - 1
    uint16_t *tl;              // [n] the positions the greedy parse visits
    uint32_t *out;             // the segment's slot, whole words
    uint32_t out_words;
    const uint8_t *stream;     // the whole stream (matches reach back across segments)
    int64_t total, start;      // its length; where the segment starts
    int n;                     // the segment's bytes
    int dist_c, dist_row;      // PNG's own match distances (a pixel, a row); 0: none.  dist_c < 0: no matches at all, literals only
    int first, last;           // the first segment's chunk carries the zlib header; the last one BFINAL
    PngSegRecord *rec;
};

PNG_HD inline uint32_t png_hash3(const uint8_t *p) {
    return (((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16) * 0x9E3779B1u) >> (32 - PNG_HASH_BITS);
}

// bits [pos, pos + nbits) of the slot |= v, LSB first (nbits <= 16)
PNG_HD inline void png_put(const PngSegCtx &c, uint32_t pos, uint32_t v, int nbits) {
    if (nbits == 0) return;
    const uint32_t w = pos >> 5, s = pos & 31;
    PNG_ATOMIC_OR(c.out + w, v << s);
    if (s + nbits > 32) PNG_ATOMIC_OR(c.out + w + 1, v >> (32 - s));
}

PNG_HD inline uint8_t png_out_byte(const PngSegCtx &c, uint32_t i) { return (uint8_t)(PNG_LOAD_SHARED_WORD(c.out + (i >> 2)) >> (8 * (i & 3))); }

// phase: clear
PNG_HD inline void png_phase_init(const PngSegCtx &c, int lane) {
    PngSegShared &s = *c.sh;
    s.crc_tab[lane] = png_crc_entry((uint32_t)lane);
    for (int i = lane; i < (1 << PNG_HASH_BITS); i += PNG_LANES) s.hash[i] = 0;
    for (int i = lane; i < 288; i += PNG_LANES) s.lfreq[i] = i == 256 ? 1u : 0u, s.llen[i] = 0, s.lcode[i] = 0;
    if (lane < 32) s.dfreq[lane] = 0, s.dlen[lane] = 0, s.dcode[lane] = 0;
    if (lane < 20) s.cfreq[lane] = 0, s.clen[lane] = 0, s.ccode[lane] = 0;
    for (uint32_t i = lane; i < c.out_words; i += PNG_LANES) c.out[i] = 0;
    if (lane == 0) s.lused = s.dused = s.cused = 0, s.adler_a = s.adler_b = 0;
}

// phase: the table learns the PNG_HASH_BACK positions in front of the segment
PNG_HD inline void png_phase_prefill(const PngSegCtx &c, int lane) {
    const int64_t lo = c.start > PNG_HASH_BACK ? c.start - PNG_HASH_BACK : 0;
    for (int64_t q = lo + lane; q < c.start; q += PNG_LANES)
        if (q + 3 <= c.total) PNG_ATOMIC_MAX(c.sh->hash + png_hash3(c.stream + q), (uint32_t)(q + 1));
}

// 8 log2(v) for v >= 8, the mantissa read as the fraction (within 0.7 of the 8 log2 it stands for)
PNG_HD inline int png_log2_fx(uint32_t v) {
    const int k = png_log2(v);
    return (k << 3) | (int)((v >> (k - 3)) & 7u);
}

// phase: count the segment's bytes (into the literal histogram, which the next phase clears again)
PNG_HD inline void png_phase_count(const PngSegCtx &c, int lane) {
    for (int i = lane; i < c.n; i += PNG_LANES) PNG_ATOMIC_ADD(c.sh->lfreq + c.stream[c.start + i], 1u);
}

// phase: a lane per byte value.  The price of a literal, from the segment's byte histogram alone: 8 log2(n / count), at least one bit.
// A match is taken only where it is cheaper than the literals it replaces -- on low-noise content most short matches are not.
PNG_HD inline void png_phase_cost(const PngSegCtx &c, int lane) {
    const uint32_t f = c.sh->lfreq[lane];
    int cost = 8 * 15;
    if (f) cost = png_log2_fx((uint32_t)c.n << 4) - png_log2_fx(f << 4);
    c.sh->lit_cost[lane] = (uint16_t)(cost < 8 ? 8 : cost);
    c.sh->lfreq[lane] = 0;
}

// the price a match is charged, in 1/8 bit: 8 bits for its length symbol, 5 for its distance symbol, and their extra bits
PNG_HD inline int png_match_cost(int len, int dist) {
    int sym, le, de, ex;
    png_len_symbol(len, &sym, &le, &ex);
    png_dist_symbol(dist, &sym, &de, &ex);
    return 8 * (8 + le + 5 + de);
}

PNG_HD inline int png_match_len(const uint8_t *at, int64_t dist, int maxlen) {
    const uint8_t *from = at - dist;
    int l = 0;
    while (l < maxlen && at[l] == from[l]) ++l;
    return l;
}

// phase, once per round r: position r * PNG_LANES + lane reads the table (which holds earlier rounds only) and takes the longest of
// the matches at distance 1, a pixel, a row and the table's (of equal lengths the first in that order), if that one pays
PNG_HD inline void png_phase_match(const PngSegCtx &c, int r, int lane) {
    const int p = r * PNG_LANES + lane;
    if (p >= c.n) return;
    const int64_t a = c.start + p;
    const uint8_t *at = c.stream + a;
    const int maxlen = c.n - p < PNG_MAX_MATCH ? c.n - p : PNG_MAX_MATCH;
    int64_t cand[4] = {1, c.dist_c, c.dist_row, 0};
    if (a + 3 <= c.total) {
        const uint32_t h = c.sh->hash[png_hash3(at)];
        if (h) cand[3] = a - (int64_t)(h - 1);
    }
    int best = 0;
    int64_t bdist = 0;
    if (maxlen >= PNG_MIN_MATCH && c.dist_c >= 0)
        for (int k = 0; k < 4 && best < maxlen; ++k) {
            const int64_t d = cand[k];
            if (d <= 0 || d > a || d > PNG_MAX_DIST) continue;
            bool seen = false;
            for (int j = 0; j < k; ++j) seen = seen || cand[j] == d;
            if (seen) continue;
            const int l = png_match_len(at, d, maxlen);
            if (l > best) best = l, bdist = d;
        }
    if (best >= PNG_MIN_MATCH) {
        int lits = 0;
        for (int i = 0; i < best; ++i) lits += c.sh->lit_cost[at[i]];
        if (lits <= png_match_cost(best, (int)bdist)) best = 0;
    }
    if (best < PNG_MIN_MATCH) best = 0, bdist = 1;
    c.mlen[p] = (uint16_t)best;
    c.mdist[p] = (uint16_t)(bdist - 1);
}

// phase, once per round after a barrier: the round's positions enter the table; the largest position stays, whoever came first
PNG_HD inline void png_phase_insert(const PngSegCtx &c, int r, int lane) {
    const int p = r * PNG_LANES + lane;
    const int64_t a = c.start + p;
    if (p < c.n && a + 3 <= c.total) PNG_ATOMIC_MAX(c.sh->hash + png_hash3(c.stream + a), (uint32_t)(a + 1));
}

// phase, lane 0: the greedy parse, a walk over next(p) = p + max(1, len(p))
PNG_HD inline void png_phase_parse(const PngSegCtx &c, int lane) {
    if (lane) return;
    uint32_t t = 0;
    for (int p = 0; p < c.n;) {
        c.tl[t++] = (uint16_t)p;
        const int l = c.mlen[p];
        p += l ? l : 1;
    }
    c.sh->ntok = t;
}

// the tokens of `lane`: a contiguous run, so that its bits are too
PNG_HD inline void png_lane_tokens(const PngSegCtx &c, int lane, uint32_t *t0, uint32_t *t1) {
    const uint32_t per = (c.sh->ntok + PNG_LANES - 1) / PNG_LANES;
    *t0 = (uint32_t)lane * per < c.sh->ntok ? (uint32_t)lane * per : c.sh->ntok;
    *t1 = *t0 + per < c.sh->ntok ? *t0 + per : c.sh->ntok;
}

// phase: the histograms of the 286 + 30 symbols
PNG_HD inline void png_phase_hist(const PngSegCtx &c, int lane) {
    uint32_t t0, t1;
    png_lane_tokens(c, lane, &t0, &t1);
    for (uint32_t t = t0; t < t1; ++t) {
        const int p = c.tl[t], l = c.mlen[p];
        if (!l) {
            PNG_ATOMIC_ADD(c.sh->lfreq + c.stream[c.start + p], 1u);
        } else {
            int sym, eb, ex;
            png_len_symbol(l, &sym, &eb, &ex);
            PNG_ATOMIC_ADD(c.sh->lfreq + sym, 1u);
            png_dist_symbol(c.mdist[p] + 1, &sym, &eb, &ex);
            PNG_ATOMIC_ADD(c.sh->dfreq + sym, 1u);
        }
    }
}

// where symbol i stands among the used ones in ascending (frequency, symbol) order; -1: unused
PNG_HD inline int png_rank(const uint32_t *freq, int nsym, int i) {
    if (!freq[i]) return -1;
    int r = 0;
    for (int j = 0; j < nsym; ++j) r += freq[j] && (freq[j] < freq[i] || (freq[j] == freq[i] && j < i));
    return r;
}

// phase: sort the used symbols of both alphabets (a rank per lane)
PNG_HD inline void png_phase_rank(const PngSegCtx &c, int lane) {
    PngSegShared &s = *c.sh;
    for (int i = lane; i < PNG_NLIT; i += PNG_LANES) {
        const int r = png_rank(s.lfreq, PNG_NLIT, i);
        if (r >= 0) s.lsorted[r] = (uint16_t)i, PNG_ATOMIC_ADD(&s.lused, 1u);
    }
    if (lane < PNG_NDIST) {
        const int r = png_rank(s.dfreq, PNG_NDIST, lane);
        if (r >= 0) s.dsorted[r] = (uint16_t)lane, PNG_ATOMIC_ADD(&s.dused, 1u);
    }
}

// Code lengths of at most `maxbits` for the `nused` symbols of sorted[] (one lane).  Fewer than two used symbols are padded to two
// codes of one bit, as zlib does, so that every code is complete: a block without a match, with one distance code, with one literal.
PNG_HD inline void png_code_lengths(PngSegShared &s, const uint32_t *freq, const uint16_t *sorted, int nused, int maxbits, uint8_t *lens) {
    if (nused < 2) {
        const int only = nused ? sorted[0] : 0;
        lens[only] = 1;
        lens[only == 0 ? 1 : 0] = 1;
        return;
    }
    // two queues: the sorted leaves [0, nused) and the internal nodes [nused, ..) in the order they are made (ascending too)
    for (int i = 0; i < nused; ++i) s.nfreq[i] = freq[sorted[i]];
    int leaf = 0, inner = nused, made = nused;
    while (made < 2 * nused - 1) {
        int pick[2];
        for (int k = 0; k < 2; ++k) {
            if (leaf < nused && (inner >= made || s.nfreq[leaf] <= s.nfreq[inner])) pick[k] = leaf++;
            else pick[k] = inner++;
        }
        s.nfreq[made] = s.nfreq[pick[0]] + s.nfreq[pick[1]];
        s.nparent[pick[0]] = s.nparent[pick[1]] = (uint16_t)made;
        ++made;
    }
    s.ndepth[made - 1] = 0;
    for (int i = made - 2; i >= 0; --i) s.ndepth[i] = (uint16_t)(s.ndepth[s.nparent[i]] + 1);
    // the limiter: count the codes of each length with the too long ones at maxbits, then, while the Kraft sum is over, take one
    // code off maxbits and turn the deepest shorter code into two codes one bit longer (each step lowers the sum by one unit)
    uint32_t count[16];
    for (int l = 0; l <= maxbits; ++l) count[l] = 0;
    for (int i = 0; i < nused; ++i) ++count[s.ndepth[i] > maxbits ? maxbits : s.ndepth[i]];
    uint32_t kraft = 0;
    for (int l = 1; l <= maxbits; ++l) kraft += count[l] << (maxbits - l);
    while (kraft > (1u << maxbits)) {
        --count[maxbits];
        for (int l = maxbits - 1; l >= 1; --l)
            if (count[l]) {
                --count[l];
                count[l + 1] += 2;
                break;
            }
        --kraft;
    }
    // the rarest symbols take the longest codes
    int at = 0;
    for (int l = maxbits; l >= 1; --l)
        for (uint32_t k = 0; k < count[l]; ++k) lens[sorted[at++]] = (uint8_t)l;
}

// canonical codes of lens[], stored bit-reversed
PNG_HD inline void png_assign_codes(const uint8_t *lens, int nsym, uint16_t *codes) {
    uint32_t count[16] = {0}, next[16];
    for (int i = 0; i < nsym; ++i) ++count[lens[i]];
    count[0] = 0;
    uint32_t code = 0;
    for (int l = 1; l < 16; ++l) {
        code = (code + count[l - 1]) << 1;
        next[l] = code;
    }
    for (int i = 0; i < nsym; ++i)
        if (lens[i]) codes[i] = (uint16_t)png_reverse_bits(next[lens[i]]++, lens[i]);
}

// the order in which a block header lists the code-length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
PNG_HD inline int png_clc_order(int i) {
    if (i < 3) return 16 + i;
    const int j = i - 3;
    return j == 0 ? 0 : (j & 1) ? 8 + (j - 1) / 2 : 8 - j / 2;
}

// phase, lane 0: the three codes and the block header's code-length sequence
PNG_HD inline void png_phase_codes(const PngSegCtx &c, int lane) {
    if (lane) return;
    PngSegShared &s = *c.sh;
    png_code_lengths(s, s.lfreq, s.lsorted, (int)s.lused, 15, s.llen);
    png_code_lengths(s, s.dfreq, s.dsorted, (int)s.dused, 15, s.dlen);
    png_assign_codes(s.llen, PNG_NLIT, s.lcode);
    png_assign_codes(s.dlen, PNG_NDIST, s.dcode);
    int hlit = PNG_NLIT, hdist = PNG_NDIST;
    while (hlit > 257 && !s.llen[hlit - 1]) --hlit;
    while (hdist > 1 && !s.dlen[hdist - 1]) --hdist;
    s.hlit = (uint32_t)hlit, s.hdist = (uint32_t)hdist;
    // the hlit + hdist lengths as one sequence; runs of 3 .. 138 zeros go out as symbol 17 or 18, everything else as itself
    const int total = hlit + hdist;
    uint32_t n = 0;
    for (int i = 0; i < total;) {
        const int v = i < hlit ? s.llen[i] : s.dlen[i - hlit];
        int run = 1;
        if (v == 0)
            while (i + run < total && run < 138 && (i + run < hlit ? s.llen[i + run] : s.dlen[i + run - hlit]) == 0) ++run;
        if (v == 0 && run >= 3) {
            s.hdr_sym[n] = run <= 10 ? 17 : 18;
            s.hdr_extra[n] = (uint8_t)(run <= 10 ? run - 3 : run - 11);
            i += run;
        } else {
            s.hdr_sym[n] = (uint8_t)v;
            s.hdr_extra[n] = 0;
            i += 1;
        }
        ++s.cfreq[s.hdr_sym[n]];
        ++n;
    }
    s.hdr_n = n;
    uint32_t cused = 0;
    for (int i = 0; i < PNG_NCLC; ++i) {
        const int r = png_rank(s.cfreq, PNG_NCLC, i);
        if (r >= 0) s.csorted[r] = (uint16_t)i, ++cused;
    }
    s.cused = cused;
    png_code_lengths(s, s.cfreq, s.csorted, (int)cused, 7, s.clen);
    png_assign_codes(s.clen, PNG_NCLC, s.ccode);
    int hclen = PNG_NCLC;
    while (hclen > 4 && !s.clen[png_clc_order(hclen - 1)]) --hclen;
    s.hclen = (uint32_t)hclen;
    uint32_t bits = 5 + 5 + 4 + 3 * (uint32_t)hclen;
    for (uint32_t i = 0; i < n; ++i) bits += s.clen[s.hdr_sym[i]] + (s.hdr_sym[i] == 17 ? 3 : s.hdr_sym[i] == 18 ? 7 : 0);
    s.hdr_bits = bits;
}

PNG_HD inline uint32_t png_token_bits(const PngSegCtx &c, uint32_t t) {
    const int p = c.tl[t], l = c.mlen[p];
    if (!l) return c.sh->llen[c.stream[c.start + p]];
    int ls, le, lx, ds, de, dx;
    png_len_symbol(l, &ls, &le, &lx);
    png_dist_symbol(c.mdist[p] + 1, &ds, &de, &dx);
    return (uint32_t)(c.sh->llen[ls] + le + c.sh->dlen[ds] + de);
}

// phase: the bits of each lane's tokens
PNG_HD inline void png_phase_bits(const PngSegCtx &c, int lane) {
    uint32_t t0, t1, bits = 0;
    png_lane_tokens(c, lane, &t0, &t1);
    for (uint32_t t = t0; t < t1; ++t) bits += png_token_bits(c, t);
    c.sh->lane_bits[lane] = bits;
}

// phase, lane 0: where each lane's bits start; dynamic or stored
PNG_HD inline void png_phase_scan(const PngSegCtx &c, int lane) {
    if (lane) return;
    PngSegShared &s = *c.sh;
    uint32_t at = 0;
    for (int i = 0; i < PNG_LANES; ++i) {
        const uint32_t b = s.lane_bits[i];
        s.lane_bits[i] = at;
        at += b;
    }
    s.body_bits = at + s.llen[256];
    const uint32_t dyn_bytes = (3 + s.hdr_bits + s.body_bits + 7) / 8, stored_bytes = 5 + (uint32_t)c.n;
    s.stored = stored_bytes <= dyn_bytes;
    const uint32_t end_bits = s.stored ? stored_bytes * 8 : 3 + s.hdr_bits + s.body_bits;
    s.out_bytes = (end_bits + 3 + 7) / 8 + 4;          // the empty stored block: 3 bits, to the byte, 00 00 FF FF
    // the chunk that the CRC covers: "IDAT", the zlib header on the first segment, the bytes
    s.crc_len = 4 + (c.first ? 2 : 0) + s.out_bytes;
    s.crc_chunk = (s.crc_len + PNG_LANES - 1) / PNG_LANES;
}

// phase: every lane writes its tokens' bits (or its share of the raw bytes); lane 0 the headers, the end-of-block and the empty block
PNG_HD inline void png_phase_emit(const PngSegCtx &c, int lane) {
    PngSegShared &s = *c.sh;
    uint32_t end_bits;
    if (s.stored) {
        for (int i = lane; i < c.n; i += PNG_LANES) png_put(c, (5 + (uint32_t)i) * 8, c.stream[c.start + i], 8);
        end_bits = (5 + (uint32_t)c.n) * 8;
        if (lane == 0) {                                // BFINAL 0, BTYPE 0 and the padding: byte 0 stays zero
            png_put(c, 8, (uint32_t)c.n & 0xFFFFu, 16);
            png_put(c, 24, ~(uint32_t)c.n & 0xFFFFu, 16);
        }
    } else {
        const uint32_t body = 3 + s.hdr_bits;
        end_bits = body + s.body_bits;
        uint32_t t0, t1, at = body + s.lane_bits[lane];
        png_lane_tokens(c, lane, &t0, &t1);
        for (uint32_t t = t0; t < t1; ++t) {
            const int p = c.tl[t], l = c.mlen[p];
            if (!l) {
                const int b = c.stream[c.start + p];
                png_put(c, at, s.lcode[b], s.llen[b]), at += s.llen[b];
            } else {
                int sym, eb, ex;
                png_len_symbol(l, &sym, &eb, &ex);
                png_put(c, at, s.lcode[sym], s.llen[sym]), at += s.llen[sym];
                png_put(c, at, (uint32_t)ex, eb), at += eb;
                png_dist_symbol(c.mdist[p] + 1, &sym, &eb, &ex);
                png_put(c, at, s.dcode[sym], s.dlen[sym]), at += s.dlen[sym];
                png_put(c, at, (uint32_t)ex, eb), at += eb;
            }
        }
        if (lane == 0) {
            uint32_t h = 0;
            png_put(c, h, 4u, 3), h += 3;               // BFINAL 0, BTYPE 2
            png_put(c, h, s.hlit - 257, 5), h += 5;
            png_put(c, h, s.hdist - 1, 5), h += 5;
            png_put(c, h, s.hclen - 4, 4), h += 4;
                    for (uint32_t i = 0; i < s.hclen; ++i) png_put(c, h, s.clen[png_clc_order((int)i)], 3), h += 3;
            for (uint32_t i = 0; i < s.hdr_n; ++i) {
                const int sym = s.hdr_sym[i];
                png_put(c, h, s.ccode[sym], s.clen[sym]), h += s.clen[sym];
                if (sym == 17) png_put(c, h, s.hdr_extra[i], 3), h += 3;
                if (sym == 18) png_put(c, h, s.hdr_extra[i], 7), h += 7;
            }
            png_put(c, end_bits - s.llen[256], s.lcode[256], s.llen[256]);
        }
    }
    if (lane == 0) {
        png_put(c, end_bits, c.last ? 1u : 0u, 3);      // BFINAL, BTYPE 0
        const uint32_t len_at = (end_bits + 3 + 7) / 8 * 8;
        png_put(c, len_at + 16, 0xFFFFu, 16);           // LEN 0, NLEN FFFF
    }
}

// byte i of the chunk the CRC covers, its first four bytes complemented: a CRC register that starts at zero over this message is the
// standard one (which starts at all ones) before its final complement -- and leading zero bytes do not move a zero register
PNG_HD inline uint8_t png_crc_msg(const PngSegCtx &c, uint32_t i) {
    const uint8_t idat[4] = {'I', 'D', 'A', 'T'}, zhdr[2] = {0x78, 0x01};
    uint8_t v;
    if (i < 4) v = idat[i];
    else if (c.first && i < 6) v = zhdr[i - 4];
    else v = png_out_byte(c, i - (c.first ? 6 : 4));
    return i < 4 ? (uint8_t)~v : v;
}

// phase: the chunk's CRC in PNG_LANES pieces of crc_chunk bytes that END together with the message (the front piece is short), and
// the Adler sums of the segment's stream bytes: a = sum d_i, b = sum (n - i) d_i
PNG_HD inline void png_phase_sums(const PngSegCtx &c, int lane) {
    PngSegShared &s = *c.sh;
    const int64_t pad = (int64_t)s.crc_chunk * PNG_LANES - s.crc_len;
    uint32_t r = 0;
    for (uint32_t k = 0; k < s.crc_chunk; ++k) {
        const int64_t i = (int64_t)lane * s.crc_chunk + k - pad;
        if (i >= 0) r = s.crc_tab[(r ^ png_crc_msg(c, (uint32_t)i)) & 0xFFu] ^ (r >> 8);
    }
    s.lane_crc[lane] = r;
    uint64_t a = 0, b = 0;
    for (int i = lane; i < c.n; i += PNG_LANES) {
        const uint32_t d = c.stream[c.start + i];
        a += d;
        b += (uint64_t)(c.n - i) * d;
    }
    PNG_ATOMIC_ADD(&s.adler_a, (uint32_t)(a % PNG_ADLER));
    PNG_ATOMIC_ADD(&s.adler_b, (uint32_t)(b % PNG_ADLER));
}

// phase, lane 0: crc = sum_j piece_j x^(8 crc_chunk (LANES - 1 - j)), by Horner; the record
PNG_HD inline void png_phase_record(const PngSegCtx &c, int lane) {
    if (lane) return;
    PngSegShared &s = *c.sh;
    uint32_t x = 0x80000000u;                           // x^0, then times x^8 per byte of a piece
    for (uint32_t k = 0; k < s.crc_chunk; ++k) x = s.crc_tab[x & 0xFFu] ^ (x >> 8);
    uint32_t acc = 0;
    for (int j = 0; j < PNG_LANES; ++j) acc = png_gf2_mul(acc, x) ^ s.lane_crc[j];
    c.rec->bytes = s.out_bytes;
    c.rec->crc = ~acc;
    c.rec->adler_a = s.adler_a % PNG_ADLER;
    c.rec->adler_b = s.adler_b % PNG_ADLER;
}

// A workgroup's run of one segment; `SYNC` is the barrier between phases, `FOR_LANES(body)` runs body for every value of `lane`.
#define PNG_RUN_SEGMENT(c, FOR_LANES, SYNC)                              \
    do {                                                                 \
        FOR_LANES(png_phase_init(c, lane)) SYNC;                         \
        FOR_LANES(png_phase_count(c, lane)) SYNC;                        \
        FOR_LANES(png_phase_cost(c, lane)) SYNC;                         \
        FOR_LANES(png_phase_prefill(c, lane)) SYNC;                      \
        for (int r__ = 0; r__ * PNG_LANES < (c).n; ++r__) {              \
            FOR_LANES(png_phase_match(c, r__, lane)) SYNC;               \
            FOR_LANES(png_phase_insert(c, r__, lane)) SYNC;              \
        }                                                                \
        FOR_LANES(png_phase_parse(c, lane)) SYNC;                        \
        FOR_LANES(png_phase_hist(c, lane)) SYNC;                         \
        FOR_LANES(png_phase_rank(c, lane)) SYNC;                         \
        FOR_LANES(png_phase_codes(c, lane)) SYNC;                        \
        FOR_LANES(png_phase_bits(c, lane)) SYNC;                         \
        FOR_LANES(png_phase_scan(c, lane)) SYNC;                         \
        FOR_LANES(png_phase_emit(c, lane)) SYNC;                         \
        FOR_LANES(png_phase_sums(c, lane)) SYNC;                         \
        FOR_LANES(png_phase_record(c, lane)) SYNC;                       \
    } while (0)

// ------------------------------------------------------------------------------------------------------------------ framing

PNG_HD inline void png_be32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v; }

struct PngHead {
    uint8_t bytes[PNG_SIG_IHDR];
};

// the signature and IHDR: 8 bit, colour type 2 (C = 3) or 0 (C = 1), no interlace
inline PngHead png_make_head(int H, int W, int C) {
    PngHead h;
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    for (int i = 0; i < 8; ++i) h.bytes[i] = sig[i];
    uint8_t *p = h.bytes + 8;
    png_be32(p, 13);
    p[4] = 'I', p[5] = 'H', p[6] = 'D', p[7] = 'R';
    png_be32(p + 8, (uint32_t)W);
    png_be32(p + 12, (uint32_t)H);
    p[16] = 8, p[17] = C == 3 ? 2 : 0, p[18] = 0, p[19] = 0, p[20] = 0;
    png_be32(p + 21, png_crc_small(p + 4, 17));
    return h;
}

// The Adler-32 of the whole stream from the segments' partial sums; where the zlib stream's and the file's bytes of segment k start.
// One lane: a loop over the records.
PNG_HD inline uint32_t png_combine_adler(const PngSegRecord *rec, int64_t nseg, int64_t n, int S) {
    uint32_t a = 1, b = 0;
    for (int64_t k = 0; k < nseg; ++k) {
        const int64_t len = n - k * S < S ? n - k * S : S;
        b = (uint32_t)((b + (uint64_t)a * (uint64_t)(len > 0 ? len : 0) + rec[k].adler_b) % PNG_ADLER);
        a = (a + rec[k].adler_a) % PNG_ADLER;
    }
    return b << 16 | a;
}

// the tail of a file behind its last segment chunk: the Adler-32 in a chunk of its own, then IEND (28 bytes)
PNG_HD inline void png_write_tail(uint8_t *p, uint32_t adler) {
    png_be32(p, 4);
    p[4] = 'I', p[5] = 'D', p[6] = 'A', p[7] = 'T';
    png_be32(p + 8, adler);
    png_be32(p + 12, png_crc_small(p + 4, 8));
    png_be32(p + 16, 0);
    p[20] = 'I', p[21] = 'E', p[22] = 'N', p[23] = 'D';
    png_be32(p + 24, png_crc_small(p + 20, 4));
}

// ------------------------------------------------------------------------------------------------- sizes and the device workspace

struct PngLayout {
    int64_t n;                  // the filtered stream of one image: H (1 + W C) bytes
    int64_t nseg;
    int S, cap;                 // segment bytes; positions a segment can hold (min(S, n) rounded up to 16)
    int64_t slot_bytes;         // one segment's output slot
    int64_t filt_off, rec_off, slot_off, mdist_off, tl_off, per_image;   // offsets inside one image's part of the workspace
};

// HOIG_OK, or why this image / segment size cannot be encoded
inline int png_layout(int H, int W, int C, int segment_bytes, PngLayout *L) {
    const int S = segment_bytes ? segment_bytes : HOIG_PNG_SEGMENT_BYTES;
    if (!png_segment_ok(S)) return HOIG_EINVAL;
    if ((C != 1 && C != 3) || H < 1 || W < 1) return HOIG_EUNSUPPORTED;
    if ((int64_t)W * C >= ((int64_t)1 << 31) || (int64_t)H * png_row_stride(W, C) >= ((int64_t)1 << 31)) return HOIG_EUNSUPPORTED;
    L->n = (int64_t)H * png_row_stride(W, C);
    L->S = S;
    L->nseg = png_nseg(L->n, S);
    L->cap = (int)((L->n < S ? L->n : S) + 15) / 16 * 16;
    L->slot_bytes = L->cap + PNG_SLOT_PAD;
    L->filt_off = 0;
    L->rec_off = (L->n + 15) / 16 * 16;
    L->slot_off = L->rec_off + L->nseg * (int64_t)sizeof(PngSegRecord);
    L->mdist_off = L->slot_off + L->nseg * L->slot_bytes;
    L->tl_off = L->mdist_off + L->nseg * L->cap * 2;
    L->per_image = L->tl_off + L->nseg * L->cap * 2;
    return HOIG_OK;
}

// the file's byte at which segment k's chunk starts, given the bytes of the segments in front of it
PNG_HD inline int64_t png_chunk_start(int64_t k, int64_t bytes_before) { return PNG_SIG_IHDR + k * PNG_SEG_FRAME + (k > 0 ? 2 : 0) + bytes_before; }
