// Host half of the PNG encoder (png_deflate.h): the sizes, and the CPU twins of the three kernels of png.hip -- the same per-lane code,
// a workgroup walked lane by lane and phase by phase.  Plain C++ with no HIP call (it also builds on its own under a host sanitizer).
#include <string.h>
#include <vector>

#include "png_deflate.h"

extern "C" int64_t hoig_png_encode_bound(int H, int W, int C, int segment_bytes) {
    PngLayout L;
    const int rc = png_layout(H, W, C, segment_bytes, &L);
    if (rc != HOIG_OK) return rc;
    return (png_file_bound(L.n, L.S) + 15) / 16 * 16;
}

extern "C" int64_t hoig_png_encode_workspace_bytes(int B, int H, int W, int C, int segment_bytes) {
    PngLayout L;
    const int rc = png_layout(H, W, C, segment_bytes, &L);
    if (rc != HOIG_OK) return rc;
    if (B < 1) return HOIG_EINVAL;
    return (int64_t)B * L.per_image;
}

namespace {

void filter_image(const uint8_t *img, int H, int W, int C, uint8_t *filtered) {
    const int64_t rowlen = (int64_t)W * C, stride = png_row_stride(W, C);
    for (int y = 0; y < H; ++y) {
        uint64_t sums[5] = {0, 0, 0, 0, 0};
        int x, a, b, c;
        for (int64_t j = 0; j < rowlen; ++j) {
            png_neighbours(img, y, j, rowlen, C, &x, &a, &b, &c);
            for (int t = 0; t < 5; ++t) sums[t] += png_abs_s8(png_filter_byte(t, x, a, b, c));
        }
        const int type = png_pick_filter(sums);
        uint8_t *out = filtered + y * stride;
        out[0] = (uint8_t)type;
        for (int64_t j = 0; j < rowlen; ++j) {
            png_neighbours(img, y, j, rowlen, C, &x, &a, &b, &c);
            out[1 + j] = png_filter_byte(type, x, a, b, c);
        }
    }
}

// one workgroup's memory, every block of exactly the size the kernel has
struct HostSegment {
    PngSegShared *sh;
    std::vector<uint16_t> mlen, mdist, tl;
    std::vector<uint32_t> out;
    PngSegRecord rec;

    explicit HostSegment(int cap) : sh(new PngSegShared), mlen(cap), mdist(cap), tl(cap), out((cap + PNG_SLOT_PAD) / 4) {}
    ~HostSegment() { delete sh; }
    HostSegment(const HostSegment &) = delete;

    // segment k of the stream; afterwards rec and byte(i) hold its result
    void run(const uint8_t *stream, int64_t n, int S, int64_t k, int64_t nseg, int dist_c, int dist_row) {
        PngSegCtx c;
        c.sh = sh;
        c.mlen = mlen.data(), c.mdist = mdist.data(), c.tl = tl.data();
        c.out = out.data(), c.out_words = (uint32_t)out.size();
        c.stream = stream, c.total = n, c.start = k * S;
        c.n = (int)(n - c.start < S ? n - c.start : S);
        if (c.n < 0) c.n = 0;
        c.dist_c = dist_c, c.dist_row = dist_row;
        c.first = k == 0, c.last = k == nseg - 1;
        c.rec = &rec;
#define PNG_HOST_LANES(body) \
    for (int lane = 0; lane < PNG_LANES; ++lane) { body; }
        PNG_RUN_SEGMENT(c, PNG_HOST_LANES, (void)0);
#undef PNG_HOST_LANES
    }
    uint8_t byte(uint32_t i) const { return (uint8_t)(out[i >> 2] >> (8 * (i & 3))); }
};

int segment_cap(int64_t n, int S) { return (int)((n < S ? n : S) + 15) / 16 * 16; }

}  // namespace

extern "C" int hoig_png_filter_host(const uint8_t *src, int H, int W, int C, uint8_t *filtered) {
    PngLayout L;
    if (!src || !filtered) return HOIG_EINVAL;
    const int rc = png_layout(H, W, C, 0, &L);
    if (rc != HOIG_OK) return rc;
    filter_image(src, H, W, C, filtered);
    return HOIG_OK;
}

extern "C" int hoig_png_deflate_host(const uint8_t *stream, int64_t n, int segment_bytes, int dist_c, int dist_row, uint8_t *out,
                                     int64_t out_bytes, int64_t *out_size, int32_t *seg_sizes) {
    const int S = segment_bytes ? segment_bytes : HOIG_PNG_SEGMENT_BYTES;
    if (!png_segment_ok(S) || !out || !out_size || n < 0 || (n > 0 && !stream) || dist_c < -1 || dist_row < 0) return HOIG_EINVAL;
    if (n >= ((int64_t)1 << 31)) return HOIG_EUNSUPPORTED;
    if (out_bytes < png_zlib_bound(n, S)) return HOIG_EINVAL;
    const int64_t nseg = png_nseg(n, S);
    HostSegment seg(segment_cap(n, S));
    std::vector<PngSegRecord> recs((size_t)nseg);
    int64_t at = 0;
    out[at++] = 0x78, out[at++] = 0x01;
    for (int64_t k = 0; k < nseg; ++k) {
        seg.run(stream, n, S, k, nseg, dist_c, dist_row);
        recs[(size_t)k] = seg.rec;
        for (uint32_t i = 0; i < seg.rec.bytes; ++i) out[at++] = seg.byte(i);
        if (seg_sizes) seg_sizes[k] = (int32_t)seg.rec.bytes;
    }
    png_be32(out + at, png_combine_adler(recs.data(), nseg, n, S));
    *out_size = at + 4;
    return HOIG_OK;
}

extern "C" int hoig_png_encode_host(const uint8_t *src, int B, int H, int W, int C, uint8_t *out, int64_t out_stride, int32_t *sizes,
                                    int segment_bytes) {
    PngLayout L;
    const int rc = png_layout(H, W, C, segment_bytes, &L);
    if (rc != HOIG_OK) return rc;
    if (!src || !out || !sizes || B < 1 || out_stride < png_file_bound(L.n, L.S)) return HOIG_EINVAL;
    const PngHead head = png_make_head(H, W, C);
    std::vector<uint8_t> filtered((size_t)L.n);
    std::vector<PngSegRecord> recs((size_t)L.nseg);
    HostSegment seg(L.cap);
    for (int i = 0; i < B; ++i) {
        filter_image(src + (int64_t)i * H * W * C, H, W, C, filtered.data());
        uint8_t *file = out + (int64_t)i * out_stride;
        memcpy(file, head.bytes, PNG_SIG_IHDR);
        int64_t before = 0;
        for (int64_t k = 0; k < L.nseg; ++k) {
            seg.run(filtered.data(), L.n, L.S, k, L.nseg, C, (int)png_row_stride(W, C));
            recs[(size_t)k] = seg.rec;
            uint8_t *p = file + png_chunk_start(k, before);
            png_be32(p, seg.rec.bytes + (k == 0 ? 2 : 0));
            p[4] = 'I', p[5] = 'D', p[6] = 'A', p[7] = 'T';
            p += 8;
            if (k == 0) *p++ = 0x78, *p++ = 0x01;
            for (uint32_t j = 0; j < seg.rec.bytes; ++j) p[j] = seg.byte(j);
            png_be32(p + seg.rec.bytes, seg.rec.crc);
            before += seg.rec.bytes;
        }
        uint8_t *tail = file + png_chunk_start(L.nseg, before);
        png_write_tail(tail, png_combine_adler(recs.data(), L.nseg, L.n, L.S));
        sizes[i] = (int32_t)(tail + 28 - file);
    }
    return HOIG_OK;
}
