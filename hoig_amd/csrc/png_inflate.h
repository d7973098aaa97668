// PNG files decoded on the device: the per-lane code of png_decode.hip's two kernels, compiled for the device there and for the host
// in png_decode_host.cpp (the CPU twins walk a workgroup lane by lane through the same functions).  docs/png_decode.md.
//
// INFLATE, one 64-lane workgroup (a wave) per image.  All state is in PngdShared (LDS on the device):
//   buf      1 KiB of the zlib stream, reloaded by the wave (16 bytes a lane) before every phase in which lane 0 reads bits; such a
//            phase reads at most PNGD_PHASE_BYTES of it (all code lengths of a dynamic header: 316 x 14 bits; a round of tokens:
//            64 x 48 bits)
//   lit/dist the current block's codes: a 9-bit table (symbol << 4 | length) and, for longer codes, the canonical counts and the
//            symbols in code order.  Built by the wave from the code lengths in four phases (count per length | first code and
//            index per length, the over-subscribed / incomplete test | symbols placed in order, a lane per length | table entries,
//            a lane per symbol).  The code-length code goes through the same builder, in `dist`.
//   tok      a round's tokens (at most 64): lane 0 decodes symbols into them, then the wave executes them.  Literals are stored a lane
//            each; matches run in order, each copied by the whole wave (byte i from i mod distance where the distance is below the
//            length).
//   window   the last 32 KiB of output as a ring; every byte also goes to the filtered stream in the workspace, which is never read
//            back while the image decodes (it is read once at the end, for the Adler-32).  A literal stored before an earlier match of
//            its round has run may only overwrite ring bytes that match does not read: lane 0 ends a round after a match whose
//            distance is above PNGD_FAR, so that no literal of the round follows it (a round writes at most 64 x 258 bytes).
// A bad stream sets bits of HOIG_PNG_E* and stops; every read of the stream and every write is checked against the image's extent.
//
// UNFILTER + CONVERT, one 256-lane workgroup per image: lane r owns row band + r and is at filter unit t - r in step t, so the row
// above is always one unit ahead; a lane hands its unit to the lane below through LDS (two slots by step parity).  The last row of a
// band is written back in place for the first row of the next.
#pragma once
#include <stdint.h>
#include <string.h>
#include "hoig_kernels.h"

#if defined(__HIPCC__)
#define PNGD_HD __host__ __device__
#else
#define PNGD_HD
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define PNGD_ATOMIC_OR(p, v) atomicOr((p), (v))
#else
#define PNGD_ATOMIC_OR(p, v) (*(p) |= (v))
#endif

#define PNGD_LANES 64
#define PNGD_WINDOW 32768
#define PNGD_BUF 1024
#define PNGD_PHASE_BYTES 600       // the most a serial phase reads of buf
#define PNGD_TOKENS 64
#define PNGD_FAR (PNGD_WINDOW - PNGD_TOKENS * 258)
#define PNGD_FAST 9
#define PNGD_MAXSYM 288
#define PNGD_ADLER 65521u
#define PNGD_ROWS 256
// a dynamic header (17 + 19 x 3 bits, then 316 lengths of at most 7 + 7 bits) and a round of tokens (15 + 5 + 15 + 13 bits each) fit, behind
// up to 15 bytes of alignment and in front of the bit reader's 8 bytes of look-ahead
static_assert((17 + 19 * 3 + 316 * 14 + 7) / 8 <= PNGD_PHASE_BYTES && PNGD_TOKENS * 48 / 8 <= PNGD_PHASE_BYTES, "a phase outruns buf");
static_assert(15 + PNGD_PHASE_BYTES + 8 <= PNGD_BUF && PNGD_FAR > 0, "a phase outruns buf");

struct PngdHuff {
    uint16_t fast[1 << PNGD_FAST];     // symbol << 4 | length; 0: a longer code, or none
    uint16_t count[16], offs[16], first[16];
    uint16_t sym[PNGD_MAXSYM];
    int32_t bad;                       // 1 over-subscribed, 2 incomplete (allowed for a single 1-bit code), 0 fine
    int32_t ncodes, maxlen;
};

enum { PNGD_STORED = 0, PNGD_FIXED = 1, PNGD_DYNAMIC = 2 };

struct PngdShared {
    uint32_t buf[PNGD_BUF / 4 + 4];    // 16 zero bytes behind the data
    uint8_t window[PNGD_WINDOW];
    PngdHuff lit, dist;
    uint8_t lens[PNGD_MAXSYM + 32];
    uint32_t tok_pos[PNGD_TOKENS], tok[PNGD_TOKENS];   // token: a literal's byte, or length | distance << 9
    uint64_t sum1[PNGD_LANES], sum2[PNGD_LANES];
    int64_t bitpos, buf_base, pos;
    int32_t ntok, nlit, ndist, mode, last, block_done, stop, status, stored_len;
};

struct PngdCtx {
    PngdShared *sh;
    const uint8_t *data;               // the zlib stream
    int64_t data_len;
    uint8_t *out;                      // the filtered stream
    int64_t expect;
    int32_t *status;
    int32_t ws_window;                 // matches read the filtered stream itself instead of the ring (the "png_window" key)
};

PNGD_HD inline void pngd_fail(PngdShared *s, int bit) { s->status |= bit, s->stop = 1; }

// ---- the stream window

PNGD_HD inline void pngd_phase_init(const PngdCtx &c, int lane) {
    PngdShared *s = c.sh;
    if (lane < 4) s->buf[PNGD_BUF / 4 + lane] = 0;
    if (lane == 0) {
        s->bitpos = 16, s->pos = 0, s->buf_base = 0;         // the two bytes of the zlib header were checked on the host
        s->ntok = 0, s->last = 0, s->block_done = 0, s->stop = 0, s->status = 0, s->stored_len = 0, s->mode = 0;
        if (c.data_len < 2) pngd_fail(s, HOIG_PNG_EEARLY);
    }
}

PNGD_HD inline void pngd_phase_fill(const PngdCtx &c, int lane) {
    PngdShared *s = c.sh;
    const int64_t base = (s->bitpos >> 3) & ~(int64_t)15, at = base + 16 * lane;
    uint32_t w[4] = {0, 0, 0, 0};
    if (at + 16 <= c.data_len) {
#if defined(__HIP_DEVICE_COMPILE__)
        __builtin_memcpy(w, __builtin_assume_aligned(c.data + at, 16), 16);
#else
        memcpy(w, c.data + at, 16);
#endif
    } else {
        for (int k = 0; k < 16; ++k)
            if (at + k < c.data_len) w[k >> 2] |= (uint32_t)c.data[at + k] << (8 * (k & 3));
    }
    for (int k = 0; k < 4; ++k) s->buf[4 * lane + k] = w[k];
}
// lane 0, after the fill and its barrier
PNGD_HD inline void pngd_fill_done(PngdShared *s) { s->buf_base = (s->bitpos >> 3) & ~(int64_t)15; }

// 32 bits at `bitpos` (zeros behind the window)
PNGD_HD inline uint32_t pngd_peek(const PngdShared *s, int64_t bitpos) {
    const uint32_t b = (uint32_t)((bitpos >> 3) - s->buf_base);
    uint32_t w = b >> 2;
    if (w > PNGD_BUF / 4 + 2) w = PNGD_BUF / 4 + 2;
    const uint64_t v = (uint64_t)s->buf[w] | ((uint64_t)s->buf[w + 1] << 32);
    return (uint32_t)(v >> ((b & 3) * 8 + (uint32_t)(bitpos & 7)));
}

// the bit reader of the token loop: the next bits in a register, refilled a word at a time
struct PngdBits {
    uint64_t hold;
    int cnt;
    uint32_t nw;                       // the next word of buf
};
PNGD_HD inline void pngd_bits_open(const PngdShared *s, PngdBits *r) {
    const uint32_t b = (uint32_t)((s->bitpos >> 3) - s->buf_base), sh = (b & 3) * 8 + (uint32_t)(s->bitpos & 7);
    r->nw = (b >> 2) + 1;
    r->hold = (uint64_t)s->buf[b >> 2] >> sh;
    r->cnt = 32 - (int)sh;
}
PNGD_HD inline void pngd_bits_refill(const PngdShared *s, PngdBits *r) {
    if (r->cnt < 32) {
        const uint32_t w = r->nw < PNGD_BUF / 4 + 3 ? r->nw : PNGD_BUF / 4 + 3;
        r->hold |= (uint64_t)s->buf[w] << r->cnt;
        r->cnt += 32, r->nw += 1;
    }
}
PNGD_HD inline int64_t pngd_bits_pos(const PngdShared *s, const PngdBits *r) { return (s->buf_base + 4 * (int64_t)r->nw) * 8 - r->cnt; }
PNGD_HD inline uint32_t pngd_bits_take(PngdBits *r, int n) {
    const uint32_t v = (uint32_t)r->hold & ((1u << n) - 1);
    r->hold >>= n, r->cnt -= n;
    return v;
}

// ---- codes

PNGD_HD inline uint32_t pngd_reverse(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// the four phases of a table over lens[0 .. n)
PNGD_HD inline void pngd_build_count(PngdHuff *h, const uint8_t *lens, int n, int lane) {
    for (int i = lane; i < (1 << PNGD_FAST); i += PNGD_LANES) h->fast[i] = 0;
    if (lane < 16) {
        int k = 0;
        for (int s = 0; s < n; ++s) k += lens[s] == lane;
        h->count[lane] = (uint16_t)k;
    }
}
PNGD_HD inline void pngd_build_first(PngdHuff *h, int lane) {
    if (lane != 0) return;
    int left = 1, code = 0, index = 0, maxlen = 0;
    h->bad = 0;
    h->count[0] = 0, h->offs[0] = 0, h->first[0] = 0;
    for (int l = 1; l <= 15; ++l) {
        left = 2 * left - h->count[l];
        if (left < 0) {
            h->bad = 1;
            break;
        }
        h->first[l] = (uint16_t)code, h->offs[l] = (uint16_t)index;
        code = (code + h->count[l]) << 1, index += h->count[l];
        if (h->count[l]) maxlen = l;
    }
    if (!h->bad && left > 0) h->bad = 2;
    h->ncodes = h->bad == 1 ? 0 : index, h->maxlen = maxlen;
}
PNGD_HD inline void pngd_build_place(PngdHuff *h, const uint8_t *lens, int n, int lane) {
    if (lane < 1 || lane > 15 || h->bad == 1) return;
    int at = h->offs[lane];
    for (int s = 0; s < n; ++s)
        if (lens[s] == lane) h->sym[at++] = (uint16_t)s;
}
PNGD_HD inline void pngd_build_fast(PngdHuff *h, const uint8_t *lens, int lane) {
    for (int i = lane; i < h->ncodes; i += PNGD_LANES) {
        const int s = h->sym[i], l = lens[s];
        if (l > PNGD_FAST) continue;
        const uint32_t code = h->first[l] + (uint32_t)(i - h->offs[l]);
        for (uint32_t j = pngd_reverse(code, l); j < (1u << PNGD_FAST); j += 1u << l) h->fast[j] = (uint16_t)(s << 4 | l);
    }
}

// the symbol at the low end of `bits` and its length; -1: no code matches
PNGD_HD inline int pngd_symbol(const PngdHuff *h, uint32_t bits, int *len) {
    const uint32_t e = h->fast[bits & ((1u << PNGD_FAST) - 1)];
    if (e) {
        *len = (int)(e & 15);
        return (int)(e >> 4);
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; ++l) {
        code |= (int)((bits >> (l - 1)) & 1);
        const int count = h->count[l];
        if (code - count < first) {
            *len = l;
            return h->sym[index + (code - first)];
        }
        index += count, first = (first + count) << 1, code <<= 1;
    }
    *len = 0;
    return -1;
}

// ---- block headers (lane 0)

PNGD_HD inline bool pngd_overrun(const PngdCtx &c, int64_t bitpos) { return bitpos > c.data_len * 8; }

PNGD_HD inline void pngd_block_header(const PngdCtx &c) {
    PngdShared *s = c.sh;
    pngd_fill_done(s);
    int64_t at = s->bitpos;
    const uint32_t h = pngd_peek(s, at);
    at += 3;
    if (pngd_overrun(c, at)) return pngd_fail(s, HOIG_PNG_EEARLY);
    s->last = (int)(h & 1), s->block_done = 0;
    const int type = (int)((h >> 1) & 3);
    s->mode = type;
    if (type == 3) return pngd_fail(s, HOIG_PNG_EBTYPE);
    if (type == PNGD_STORED) {
        at = (at + 7) & ~(int64_t)7;
        const uint32_t v = pngd_peek(s, at);
        at += 32;
        if (pngd_overrun(c, at)) return pngd_fail(s, HOIG_PNG_EEARLY);
        const uint32_t len = v & 0xffff, nlen = v >> 16;
        if ((len ^ 0xffff) != nlen) return pngd_fail(s, HOIG_PNG_ESTORED);
        s->bitpos = at;
        if ((at >> 3) + len > c.data_len) return pngd_fail(s, HOIG_PNG_EEARLY);
        if (s->pos + len > c.expect) return pngd_fail(s, HOIG_PNG_EMORE);
        s->stored_len = (int32_t)len;
        return;
    }
    if (type == PNGD_FIXED) {
        for (int i = 0; i < 288; ++i) s->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
        for (int i = 0; i < 32; ++i) s->lens[288 + i] = 5;
        s->nlit = 288, s->ndist = 32, s->bitpos = at;
        return;
    }
    const uint32_t v = pngd_peek(s, at);
    at += 14;
    if (pngd_overrun(c, at)) return pngd_fail(s, HOIG_PNG_EEARLY);
    const int nlit = (int)(v & 31) + 257, ndist = (int)((v >> 5) & 31) + 1, nclc = (int)((v >> 10) & 15) + 4;
    if (nlit > 286 || ndist > 30) return pngd_fail(s, HOIG_PNG_ECODE);
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int i = 0; i < 19; ++i) s->lens[i] = 0;
    for (int i = 0; i < nclc; ++i) {
        s->lens[order[i]] = (uint8_t)(pngd_peek(s, at) & 7);
        at += 3;
    }
    if (pngd_overrun(c, at)) return pngd_fail(s, HOIG_PNG_EEARLY);
    s->nlit = nlit, s->ndist = ndist, s->bitpos = at;
}

// the nlit + ndist code lengths through the code-length code (in s->dist); they replace lens[0 ..)
PNGD_HD inline void pngd_read_lengths(const PngdCtx &c) {
    PngdShared *s = c.sh;
    if (s->dist.bad) return pngd_fail(s, HOIG_PNG_ECODE);        // zlib: the code-length code must be complete
    uint8_t *lens = s->lens;
    const int total = s->nlit + s->ndist;
    int64_t at = s->bitpos;
    // the code-length code's own lengths sit in lens[0 .. 19) and are overwritten below: the built table no longer reads them
    int n = 0, prev = 0;
    while (n < total) {
        int l;
        const uint32_t bits = pngd_peek(s, at);
        const int sym = pngd_symbol(&s->dist, bits, &l);
        if (sym < 0) return pngd_fail(s, pngd_overrun(c, at + 7) ? HOIG_PNG_EEARLY : HOIG_PNG_ECODE);
        at += l;
        if (pngd_overrun(c, at)) return pngd_fail(s, HOIG_PNG_EEARLY);
        if (sym < 16) {
            lens[n++] = (uint8_t)sym, prev = sym;
            continue;
        }
        const int ebits = sym == 16 ? 2 : sym == 17 ? 3 : 7;
        const int rep = (sym == 16 ? 3 : sym == 17 ? 3 : 11) + (int)((bits >> l) & ((1u << ebits) - 1));
        at += ebits;
        if (pngd_overrun(c, at)) return pngd_fail(s, HOIG_PNG_EEARLY);
        if (sym == 16 && n == 0) return pngd_fail(s, HOIG_PNG_ECODE);
        if (n + rep > total) return pngd_fail(s, HOIG_PNG_ECODE);
        const int fill = sym == 16 ? prev : 0;
        for (int k = 0; k < rep; ++k) lens[n++] = (uint8_t)fill;
        if (sym != 16) prev = 0;
    }
    s->bitpos = at;
    if (lens[256] == 0) return pngd_fail(s, HOIG_PNG_ECODE);     // no end-of-block code
}

// lane 0, after both tables are built: zlib's rule for an incomplete code
PNGD_HD inline void pngd_check_tables(const PngdCtx &c) {
    PngdShared *s = c.sh;
    const PngdHuff *t[2] = {&s->lit, &s->dist};
    for (int k = 0; k < 2; ++k)
        if (t[k]->bad == 1 || (t[k]->bad == 2 && t[k]->maxlen > 1)) return pngd_fail(s, HOIG_PNG_ECODE);
}

// ---- a round of tokens (lane 0), and its execution (the wave)

PNGD_HD inline void pngd_phase_tokens(const PngdCtx &c) {
    const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                                8193, 12289, 16385, 24577};
    const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    PngdShared *s = c.sh;
    pngd_fill_done(s);
    PngdBits r;
    pngd_bits_open(s, &r);
    // positions in 32 bits inside the loop: the stream's end relative to buf (a round reads less than 1 KiB), the output below 2^31
    const int64_t left = (c.data_len - s->buf_base) * 8;
    const int32_t limit = left < (1 << 20) ? (int32_t)left : (1 << 20);
#define PNGD_REL() ((int32_t)(32 * r.nw) - r.cnt)
    const uint32_t expect = (uint32_t)c.expect;
    uint32_t pos = (uint32_t)s->pos;
    int n = 0, l;
    while (n < PNGD_TOKENS) {
        pngd_bits_refill(s, &r);
        const int sym = pngd_symbol(&s->lit, (uint32_t)r.hold, &l);
        if (sym < 0) {
            pngd_fail(s, PNGD_REL() + 15 > limit ? HOIG_PNG_EEARLY : HOIG_PNG_ECODE);
            break;
        }
        pngd_bits_take(&r, l);
        if (PNGD_REL() > limit) {
            pngd_fail(s, HOIG_PNG_EEARLY);
            break;
        }
        if (sym < 256) {
            if (pos >= expect) {
                pngd_fail(s, HOIG_PNG_EMORE);
                break;
            }
            s->tok_pos[n] = pos, s->tok[n] = (uint32_t)sym;
            ++n, ++pos;
            continue;
        }
        if (sym == 256) {
            s->block_done = 1;
            break;
        }
        if (sym >= 286) {
            pngd_fail(s, HOIG_PNG_ECODE);
            break;
        }
        const uint32_t len = lbase[sym - 257] + pngd_bits_take(&r, lext[sym - 257]);
        pngd_bits_refill(s, &r);
        const int dsym = pngd_symbol(&s->dist, (uint32_t)r.hold, &l);
        if (dsym < 0 || dsym >= 30) {
            pngd_fail(s, dsym < 0 && PNGD_REL() + 15 > limit ? HOIG_PNG_EEARLY : HOIG_PNG_ECODE);
            break;
        }
        pngd_bits_take(&r, l);
        const uint32_t dist = dbase[dsym] + pngd_bits_take(&r, dext[dsym]);
        if (PNGD_REL() > limit) {
            pngd_fail(s, HOIG_PNG_EEARLY);
            break;
        }
        if (dist > pos) {
            pngd_fail(s, HOIG_PNG_EDIST);
            break;
        }
        if (len > expect - pos) {
            pngd_fail(s, HOIG_PNG_EMORE);
            break;
        }
        s->tok_pos[n] = pos, s->tok[n] = len | dist << 9;
        ++n, pos += len;
        if (dist > PNGD_FAR) break;
    }
#undef PNGD_REL
    s->ntok = n, s->pos = pos;
    s->bitpos = pngd_bits_pos(s, &r);
}

PNGD_HD inline void pngd_phase_literals(const PngdCtx &c, int lane) {
    PngdShared *s = c.sh;
    if (lane >= s->ntok || s->tok[lane] >> 9) return;
    const uint32_t pos = s->tok_pos[lane];
    const uint8_t b = (uint8_t)s->tok[lane];
    s->window[pos & (PNGD_WINDOW - 1)] = b;
    c.out[pos] = b;
}

// bytes base + lane of match t
PNGD_HD inline void pngd_phase_copy(const PngdCtx &c, int t, int base, int lane) {
    PngdShared *s = c.sh;
    const uint32_t pos = s->tok_pos[t], len = s->tok[t] & 511, dist = s->tok[t] >> 9, i = (uint32_t)(base + lane);
    if (i >= len) return;
    const uint32_t src = pos - dist + (dist < len ? i % dist : i);
    const uint8_t b = c.ws_window ? c.out[src] : s->window[src & (PNGD_WINDOW - 1)];
    s->window[(pos + i) & (PNGD_WINDOW - 1)] = b;
    c.out[pos + i] = b;
}

PNGD_HD inline void pngd_phase_stored(const PngdCtx &c, int lane) {
    PngdShared *s = c.sh;
    const int64_t from = s->bitpos >> 3, pos = s->pos;
    for (int i = lane; i < s->stored_len; i += PNGD_LANES) {
        const uint8_t b = c.data[from + i];
        s->window[(pos + i) & (PNGD_WINDOW - 1)] = b;
        c.out[pos + i] = b;
    }
}
PNGD_HD inline void pngd_stored_done(PngdShared *s) {
    s->bitpos += 8 * (int64_t)s->stored_len, s->pos += s->stored_len;
    s->stored_len = 0, s->block_done = 1;
}

// ---- the end: the size, the Adler-32 of what was written against the stored one

PNGD_HD inline void pngd_phase_adler(const PngdCtx &c, int lane) {
    PngdShared *s = c.sh;
    uint64_t a = 0, b = 0;
    if (s->status == 0 && s->pos == c.expect)
        for (int64_t i = lane; i < c.expect; i += PNGD_LANES) {
            const uint32_t v = c.out[i];
            a += v, b += (uint64_t)((uint32_t)(c.expect - i) % PNGD_ADLER) * v;
        }
    s->sum1[lane] = a, s->sum2[lane] = b;
}
PNGD_HD inline void pngd_phase_finish(const PngdCtx &c, int lane) {
    PngdShared *s = c.sh;
    if (lane != 0) return;
    if (s->status == 0 && s->pos < c.expect) s->status |= HOIG_PNG_ELESS;
    if (s->status == 0) {
        const int64_t at = (s->bitpos + 7) >> 3;
        if (at + 4 > c.data_len) {
            s->status |= HOIG_PNG_EEARLY;
        } else {
            uint64_t a = 1, b = (uint64_t)(c.expect % PNGD_ADLER);
            for (int k = 0; k < PNGD_LANES; ++k) a += s->sum1[k] % PNGD_ADLER, b += s->sum2[k] % PNGD_ADLER;
            const uint32_t mine = (uint32_t)(b % PNGD_ADLER) << 16 | (uint32_t)(a % PNGD_ADLER);
            const uint32_t theirs = (uint32_t)c.data[at] << 24 | (uint32_t)c.data[at + 1] << 16 | (uint32_t)c.data[at + 2] << 8 | c.data[at + 3];
            if (mine != theirs) s->status |= HOIG_PNG_EADLER;
        }
    }
    *c.status = s->status;
}

// The kernel and its twin.  LANES(body) runs `body` with `lane` = 0 .. 63; SYNC orders the workgroup's LDS and global accesses, LSYNC
// its LDS accesses alone.  Every loop condition is read from LDS behind a barrier, so it is uniform.
#define PNGD_BUILD(c, LANES, SYNC, table, lens_, n_)                   \
    LANES(pngd_build_count(&(c).sh->table, (lens_), (n_), lane));      \
    SYNC;                                                              \
    LANES(pngd_build_first(&(c).sh->table, lane));                     \
    SYNC;                                                              \
    LANES(pngd_build_place(&(c).sh->table, (lens_), (n_), lane));      \
    SYNC;                                                              \
    LANES(pngd_build_fast(&(c).sh->table, (lens_), lane));             \
    SYNC;

#define PNGD_RUN_INFLATE(c, LANES, SYNC, LSYNC)                                                         \
    LANES(pngd_phase_init(c, lane));                                                                    \
    LSYNC;                                                                                              \
    while (!(c).sh->stop) {                                                                             \
        LANES(pngd_phase_fill(c, lane));                                                                \
        LSYNC;                                                                                          \
        LANES(if (lane == 0) pngd_block_header(c));                                                     \
        LSYNC;                                                                                          \
        if ((c).sh->stop) break;                                                                        \
        if ((c).sh->mode == PNGD_STORED) {                                                              \
            LANES(pngd_phase_stored(c, lane));                                                          \
            LSYNC;                                                                                      \
            LANES(if (lane == 0) pngd_stored_done((c).sh));                                             \
            LSYNC;                                                                                      \
        } else {                                                                                        \
            if ((c).sh->mode == PNGD_DYNAMIC) {                                                         \
                PNGD_BUILD(c, LANES, LSYNC, dist, (c).sh->lens, 19)                                     \
                LANES(if (lane == 0) pngd_read_lengths(c));                                             \
                LSYNC;                                                                                  \
                if ((c).sh->stop) break;                                                                \
            }                                                                                           \
            PNGD_BUILD(c, LANES, LSYNC, lit, (c).sh->lens, (c).sh->nlit)                                \
            PNGD_BUILD(c, LANES, LSYNC, dist, (c).sh->lens + (c).sh->nlit, (c).sh->ndist)               \
            LANES(if (lane == 0) pngd_check_tables(c));                                                 \
            LSYNC;                                                                                      \
            while (!(c).sh->stop && !(c).sh->block_done) {                                              \
                LANES(pngd_phase_fill(c, lane));                                                        \
                LSYNC;                                                                                  \
                LANES(if (lane == 0) pngd_phase_tokens(c));                                             \
                LSYNC;                                                                                  \
                LANES(pngd_phase_literals(c, lane));                                                    \
                LSYNC;                                                                                  \
                for (int t_ = 0; t_ < (c).sh->ntok; ++t_) {                                             \
                    if (((c).sh->tok[t_] >> 9) == 0) continue;                                          \
                    for (int base_ = 0; base_ < (int)((c).sh->tok[t_] & 511); base_ += PNGD_LANES) {    \
                        LANES(pngd_phase_copy(c, t_, base_, lane));                                     \
                        LSYNC;                                                                          \
                    }                                                                                   \
                }                                                                                       \
                LSYNC;                                                                                  \
            }                                                                                           \
        }                                                                                               \
        if ((c).sh->last && (c).sh->block_done) break;                                                  \
    }                                                                                                   \
    SYNC;                                                                                               \
    LANES(pngd_phase_adler(c, lane));                                                                   \
    LSYNC;                                                                                              \
    LANES(pngd_phase_finish(c, lane));

// ---- unfilter + convert

struct PngdRowShared {
    uint32_t pub[2][PNGD_ROWS];
    int32_t skip;
};
struct PngdLane {
    uint32_t a, c;                     // the unit to the left, and the one above it
    int32_t type;
};
struct PngdRowCtx {
    PngdRowShared *sh;
    uint8_t *filt;                     // the filtered stream (a band's last row is reconstructed in place)
    uint8_t *out;
    const uint8_t *pal;
    int32_t *status;
    int32_t W, H, ctype, depth, bpp, rowbytes, units, pal_entries, bgr;
};

PNGD_HD inline int pngd_channels(int ctype) { return ctype == 2 ? 3 : ctype == 4 ? 2 : ctype == 6 ? 4 : 1; }
PNGD_HD inline int64_t pngd_rowbytes(int W, int ctype, int depth) { return ((int64_t)W * pngd_channels(ctype) * depth + 7) / 8; }
PNGD_HD inline int pngd_bpp(int ctype, int depth) { return depth < 8 ? 1 : pngd_channels(ctype); }
// 0, or the HOIG_E* code of a plan outside the supported set
PNGD_HD inline int pngd_plan_check(const hoig_png_decode_plan *p) {
    if (p->width < 1 || p->height < 1 || p->data_len < 0 || p->data_off < 0 || (p->data_off & 15) || p->out_off < 0) return HOIG_EINVAL;
    const int t = p->color_type, d = p->bit_depth;
    if (!(t == 0 || t == 2 || t == 3 || t == 4 || t == 6)) return HOIG_EUNSUPPORTED;
    if (!(d == 8 || ((t == 0 || t == 3) && (d == 1 || d == 2 || d == 4)))) return HOIG_EUNSUPPORTED;
    if (t == 3 && (p->pal_off < 0 || p->pal_entries < 1 || p->pal_entries > 256)) return HOIG_EUNSUPPORTED;
    const int64_t rb = pngd_rowbytes(p->width, t, d);
    if (rb >= ((int64_t)1 << 31) || (1 + rb) * p->height >= ((int64_t)1 << 31)) return HOIG_EUNSUPPORTED;
    if ((int64_t)p->width * p->height * 3 >= ((int64_t)1 << 40)) return HOIG_EUNSUPPORTED;
    return HOIG_OK;
}
PNGD_HD inline int64_t pngd_expect(const hoig_png_decode_plan *p) {
    return (1 + pngd_rowbytes(p->width, p->color_type, p->bit_depth)) * p->height;
}

// png_decode_host.cpp: every plan supported, every offset and size inside its buffer (HOIG_OK, or the code to return before any launch)
int pngd_check_batch(const hoig_png_decode_plan *plans, int n, int64_t nbytes, int64_t out_bytes, int64_t workspace_bytes);

PNGD_HD inline int pngd_paeth(int a, int b, int c) {
    const int p = a + b - c, pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

PNGD_HD inline void pngd_store_px(const PngdRowCtx &c, int64_t px, int r, int g, int b) {
    uint8_t *o = c.out + px * 3;
    o[0] = (uint8_t)(c.bgr ? b : r), o[1] = (uint8_t)g, o[2] = (uint8_t)(c.bgr ? r : b);
}
PNGD_HD inline void pngd_store_index(const PngdRowCtx &c, int64_t px, int v) {
    if (v < c.pal_entries) pngd_store_px(c, px, c.pal[3 * v], c.pal[3 * v + 1], c.pal[3 * v + 2]);
    else pngd_store_px(c, px, 0, 0, 0);
}
// the pixels of reconstructed unit `col` of row y
PNGD_HD inline void pngd_convert(const PngdRowCtx &c, int y, int col, uint32_t x) {
    const int64_t row = (int64_t)y * c.W;
    if (c.depth == 8) {
        const int v0 = (int)(x & 255), v1 = (int)((x >> 8) & 255), v2 = (int)((x >> 16) & 255);
        if (c.ctype == 2 || c.ctype == 6) pngd_store_px(c, row + col, v0, v1, v2);
        else if (c.ctype == 3) pngd_store_index(c, row + col, v0);
        else pngd_store_px(c, row + col, v0, v0, v0);
        return;
    }
    const int per = 8 / c.depth, mask = (1 << c.depth) - 1, scale = 255 / mask;
    for (int k = 0; k < per; ++k) {
        const int px = col * per + k;
        if (px >= c.W) break;
        const int v = (int)(x >> (8 - c.depth * (k + 1))) & mask;
        if (c.ctype == 3) pngd_store_index(c, row + px, v);
        else pngd_store_px(c, row + px, v * scale, v * scale, v * scale);
    }
}

PNGD_HD inline void pngd_row_init(const PngdRowCtx &c, int lane) {
    if (lane == 0) c.sh->skip = *c.status != 0;
}
PNGD_HD inline void pngd_row_band(const PngdRowCtx &c, PngdLane &st, int band, int lane) {
    st.a = 0, st.c = 0, st.type = 0;
    const int y = band + lane;
    if (y >= c.H) return;
    const int type = c.filt[(int64_t)y * (1 + c.rowbytes)];
    if (type > 4) PNGD_ATOMIC_OR(c.status, (int32_t)HOIG_PNG_EFILTER);
    else st.type = type;
}
PNGD_HD inline void pngd_row_step(const PngdRowCtx &c, PngdLane &st, int band, int t, int lane) {
    const int y = band + lane, col = t - lane;
    if (y >= c.H || col < 0 || col >= c.units) return;
    uint8_t *p = c.filt + (int64_t)y * (1 + c.rowbytes) + 1 + (int64_t)col * c.bpp;
    uint32_t above = 0;
    if (y > 0) {
        if (lane > 0) {
            above = c.sh->pub[(t - 1) & 1][lane - 1];
        } else {
            const uint8_t *q = p - (1 + c.rowbytes);
            for (int k = 0; k < c.bpp; ++k) above |= (uint32_t)q[k] << (8 * k);
        }
    }
    uint32_t x = 0;
    for (int k = 0; k < c.bpp; ++k) {
        const int f = p[k], a = (int)((st.a >> (8 * k)) & 255), b = (int)((above >> (8 * k)) & 255), cc = (int)((st.c >> (8 * k)) & 255);
        const int pred = st.type == 0 ? 0 : st.type == 1 ? a : st.type == 2 ? b : st.type == 3 ? (a + b) >> 1 : pngd_paeth(a, b, cc);
        x |= (uint32_t)((f + pred) & 255) << (8 * k);
    }
    st.a = x, st.c = above;
    c.sh->pub[t & 1][lane] = x;
    if (lane == PNGD_ROWS - 1 && y + 1 < c.H)
        for (int k = 0; k < c.bpp; ++k) p[k] = (uint8_t)(x >> (8 * k));
    pngd_convert(c, y, col, x);
}

// ST(lane): the lane's PngdLane (a register on the device, an array entry in the twin)
#define PNGD_RUN_ROWS(c, LANES, SYNC, LSYNC, ST)                                               \
    LANES(pngd_row_init(c, lane));                                                             \
    SYNC;                                                                                      \
    if (!(c).sh->skip)                                                                         \
        for (int band_ = 0; band_ < (c).H; band_ += PNGD_ROWS) {                               \
            LANES(pngd_row_band(c, ST(lane), band_, lane));                                    \
            const int rows_ = (c).H - band_ < PNGD_ROWS ? (c).H - band_ : PNGD_ROWS;           \
            for (int t_ = 0; t_ < (c).units + rows_ - 1; ++t_) {                               \
                LANES(pngd_row_step(c, ST(lane), band_, t_, lane));                            \
                LSYNC;                                                                         \
            }                                                                                  \
            SYNC;                                                                              \
        }
