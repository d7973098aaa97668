// PNG files encoded on the device (the format, the per-lane code and the phases: png_deflate.h; docs/png_encode.md): eval.py's output
// images leave the device as finished files instead of raw pixels for zlib on the host.  Integer-only; three launches for a batch:
//
//   filter    a wave per row, four rows per workgroup: the five candidate filters' sums of absolute values by wave reduction, then
//             the chosen row and its type byte into the workspace.  Row y reads raw rows y and y - 1 only.
//   segment   a workgroup per (segment, image) runs PNG_RUN_SEGMENT: match lengths per position (distance 1, a pixel, a row, one
//             candidate from a hash table in LDS that is filled round by round with atomicMax), a greedy parse walked by one lane over
//             the lengths in LDS, histograms, length-limited codes, bit offsets by prefix sum, then every lane ORs its tokens' bits
//             into the segment's slot; the chunk's CRC-32 and the Adler partial sums go into the segment's record.
//   assemble  a workgroup per (segment, image): the sizes in front of it summed, its IDAT chunk copied into the file; the first also
//             writes the signature and IHDR, the last the Adler-32 chunk, IEND and sizes[i].
#include "common.h"
#include "png_deflate.h"

namespace {

constexpr int FILTER_ROWS = 4;

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
    return v;
}

__global__ __launch_bounds__(64 * FILTER_ROWS) void png_filter_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ ws,
                                                                      int64_t per_image, int H, int W, int C) {
    const int y = blockIdx.x * FILTER_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (y >= H) return;                                  // a whole wave leaves: no barrier follows
    const int64_t rowlen = (int64_t)W * C;
    const uint8_t *img = src + (int64_t)blockIdx.y * H * rowlen;
    uint8_t *out = ws + (int64_t)blockIdx.y * per_image + (int64_t)y * png_row_stride(W, C);
    uint64_t sums[5] = {0, 0, 0, 0, 0};
    int x, a, b, c;
    for (int64_t j = lane; j < rowlen; j += 64) {
        png_neighbours(img, y, j, rowlen, C, &x, &a, &b, &c);
#pragma unroll
        for (int t = 0; t < 5; ++t) sums[t] += png_abs_s8(png_filter_byte(t, x, a, b, c));
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) sums[t] = wave_sum_u64(sums[t]);
    const int type = png_pick_filter(sums);
    if (lane == 0) out[0] = (uint8_t)type;
    for (int64_t j = lane; j < rowlen; j += 64) {
        png_neighbours(img, y, j, rowlen, C, &x, &a, &b, &c);
        out[1 + j] = png_filter_byte(type, x, a, b, c);
    }
}

__global__ __launch_bounds__(PNG_LANES) void png_segment_kernel(uint8_t *__restrict__ ws, PngLayout L, int dist_c, int dist_row) {
    extern __shared__ __align__(16) uint8_t lds[];
    uint8_t *base = ws + (int64_t)blockIdx.y * L.per_image;
    const int64_t k = blockIdx.x;
    PngSegCtx c;
    c.sh = reinterpret_cast<PngSegShared *>(lds);
    c.mlen = reinterpret_cast<uint16_t *>(lds + sizeof(PngSegShared));
    c.mdist = reinterpret_cast<uint16_t *>(base + L.mdist_off) + k * L.cap;
    c.tl = reinterpret_cast<uint16_t *>(base + L.tl_off) + k * L.cap;
    c.out = reinterpret_cast<uint32_t *>(base + L.slot_off + k * L.slot_bytes);
    c.out_words = (uint32_t)(L.slot_bytes / 4);
    c.stream = base + L.filt_off;
    c.total = L.n;
    c.start = k * L.S;
    c.n = (int)(L.n - c.start < L.S ? L.n - c.start : L.S);
    c.dist_c = dist_c, c.dist_row = dist_row;
    c.first = k == 0, c.last = k == L.nseg - 1;
    c.rec = reinterpret_cast<PngSegRecord *>(base + L.rec_off) + k;
#define PNG_DEVICE_LANES(body) \
    {                          \
        const int lane = threadIdx.x; \
        body;                  \
    }
    PNG_RUN_SEGMENT(c, PNG_DEVICE_LANES, __syncthreads());
#undef PNG_DEVICE_LANES
}

__global__ __launch_bounds__(PNG_LANES) void png_assemble_kernel(const uint8_t *__restrict__ ws, PngLayout L, PngHead head,
                                                                 uint8_t *__restrict__ out, int64_t out_stride,
                                                                 int32_t *__restrict__ sizes) {
    __shared__ uint32_t before_sh;
    const uint8_t *base = ws + (int64_t)blockIdx.y * L.per_image;
    const PngSegRecord *rec = reinterpret_cast<const PngSegRecord *>(base + L.rec_off);
    uint8_t *file = out + (int64_t)blockIdx.y * out_stride;
    const int64_t k = blockIdx.x;
    const int lane = threadIdx.x;
    if (lane == 0) before_sh = 0;
    __syncthreads();
    uint32_t part = 0;
    for (int64_t j = lane; j < k; j += PNG_LANES) part += rec[j].bytes;
    if (part) atomicAdd(&before_sh, part);
    __syncthreads();
    const int64_t before = before_sh;
    const uint32_t bytes = rec[k].bytes;
    uint8_t *p = file + png_chunk_start(k, before);
    if (k == 0 && lane < PNG_SIG_IHDR) file[lane] = head.bytes[lane];
    if (lane == 0) {
        png_be32(p, bytes + (k == 0 ? 2 : 0));
        p[4] = 'I', p[5] = 'D', p[6] = 'A', p[7] = 'T';
        if (k == 0) p[8] = 0x78, p[9] = 0x01;
    }
    p += k == 0 ? 10 : 8;
    const uint8_t *slot = base + L.slot_off + k * L.slot_bytes;
    for (uint32_t i = lane; i < bytes; i += PNG_LANES) p[i] = slot[i];
    if (lane == 0) png_be32(p + bytes, rec[k].crc);
    if (k == L.nseg - 1 && lane == 0) {
        uint8_t *tail = file + png_chunk_start(L.nseg, before + bytes);
        png_write_tail(tail, png_combine_adler(rec, L.nseg, L.n, L.S));
        sizes[blockIdx.y] = (int32_t)(tail + 28 - file);
    }
}

}  // namespace

extern "C" int hoig_png_encode_u8(const uint8_t *src, int B, int H, int W, int C, uint8_t *out, int64_t out_stride, int32_t *sizes,
                                  void *workspace, int64_t workspace_bytes, int segment_bytes, hoig_stream_t stream) {
    PngLayout L;
    const int rc = png_layout(H, W, C, segment_bytes, &L);
    if (rc != HOIG_OK) return rc;
    if (!src || !out || !sizes || !workspace || B < 1 || ((uintptr_t)workspace & 15)) return HOIG_EINVAL;
    if (out_stride < png_file_bound(L.n, L.S) || workspace_bytes < (int64_t)B * L.per_image) return HOIG_EINVAL;
    if (B > 65535 || hoig_cdiv(H, FILTER_ROWS) > 0x7fffffff) return HOIG_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    const size_t lds = sizeof(PngSegShared) + (size_t)L.cap * sizeof(uint16_t);
    png_filter_kernel<<<dim3((unsigned)hoig_cdiv(H, FILTER_ROWS), B), 64 * FILTER_ROWS, 0, st>>>(src, ws, L.per_image, H, W, C);
    HOIG_LAUNCH_CHECK();
    constexpr int LDS_MAX = (int)(sizeof(PngSegShared) + 32768 * sizeof(uint16_t));
    const int rc_seg = hoig_launch<png_segment_kernel, LDS_MAX>(dim3((unsigned)L.nseg, B), PNG_LANES, lds, st,
                                                                ws, L, C, (int)png_row_stride(W, C));
    if (rc_seg != HOIG_OK) return rc_seg;
    png_assemble_kernel<<<dim3((unsigned)L.nseg, B), PNG_LANES, 0, st>>>(ws, L, png_make_head(H, W, C), out, out_stride, sizes);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}
