// Region scores on the device (docs/region_metrics.md; the shared per-lane code and the table layout: region_metrics.h).
//
// stats_init_kernel: the rows of `stats` to (0, 0, 0, W, H, -1, -1, 0) and *status to 0.
// stats_kernel: a workgroup takes REGION_BLOCK_PIXELS consecutive pixels of one image, a lane REGION_LANE_PIXELS of them, NT apart,
//   so that a wave's byte loads of one turn are 192 + 192 + 64 consecutive bytes (3 W is in general no multiple of 4: no word loads).
//   A lane keeps the R + 1 rows in registers (32-bit: region_metrics.h has the bound), the waves meet through shuffles and LDS, and
//   one lane per value adds the workgroup's row to `stats` with 64-bit integer atomics (add / min / max) -- rows the workgroup did
//   not touch are skipped, which is most of them.  Integer sums: the order of arrival changes nothing.  No workgroup waits for
//   another.
// boxes_kernel: one lane per (image, region).
// crop_h_kernel: the horizontal pass of crop (r, n) into the workspace [R][N][min(H, W)][S][3].  The grid holds enough workgroups
//   per crop for side = min(H, W); each reads its box from device memory and leaves at once when the box is invalid or its share of
//   the [side][S][3] bytes is empty.  A lane makes 4 consecutive bytes and stores one word.
// crop_v_kernel: the vertical pass over the whole of dst [R][N][S][S][3], 4 bytes per lane; invalid crops become zeros here.
#include "common.h"
#include "region_metrics.h"

namespace {

constexpr int NT = REGION_NT;
constexpr int VALUES = REGION_ROWS * 7;     // the seven live values of every row

__global__ __launch_bounds__(NT) void stats_init_kernel(int64_t *stats, int64_t rows, int H, int W, int32_t *status) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i == 0) *status = 0;
    if (i < rows) region_row_init(stats + i * HOIG_REGION_ROW, H, W);
}

__device__ __forceinline__ uint32_t wave_add(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

__global__ __launch_bounds__(NT) void stats_kernel(const uint8_t *__restrict__ gen, const uint8_t *__restrict__ gt,
                                                   const uint8_t *__restrict__ labels, int H, int W, int R, int chunks,
                                                   int64_t *stats, int32_t *status) {
    __shared__ uint32_t part[NT / 64][VALUES];
    __shared__ int bad_part[NT / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int img = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const int npix = H * W;                                         // <= 4096^2
    const int lo = chunk * REGION_BLOCK_PIXELS, hi = lo + REGION_BLOCK_PIXELS < npix ? lo + REGION_BLOCK_PIXELS : npix;
    const uint8_t *g = gen + (int64_t)img * npix * 3, *r = gt + (int64_t)img * npix * 3, *lab = labels + (int64_t)img * npix;
    region_rows<uint32_t> a;
    region_rows_clear(a, H, W);
    for (int i = lo + t; i < hi; i += NT) region_rows_add(a, R, g + (int64_t)i * 3, r + (int64_t)i * 3, lab[i], i % W, i / W);
#pragma unroll
    for (int row = 0; row < REGION_ROWS; ++row) {
        const uint32_t cnt = wave_add(a.cnt[row]), ad = wave_add(a.ad[row]), sq = wave_add(a.sq[row]);
        const int x0 = wave_min(a.x0[row]), y0 = wave_min(a.y0[row]), x1 = wave_max(a.x1[row]), y1 = wave_max(a.y1[row]);
        if (lane == 0) {
            uint32_t *p = part[wave] + row * 7;
            p[0] = cnt, p[1] = ad, p[2] = sq;
            p[3] = (uint32_t)x0, p[4] = (uint32_t)y0, p[5] = (uint32_t)x1, p[6] = (uint32_t)y1;
        }
    }
    const int bad = wave_max(a.bad);
    if (lane == 0) bad_part[wave] = bad;
    __syncthreads();
    if (t == 0) {
        int b = bad_part[0];
        for (int w = 1; w < NT / 64; ++w) b = bad_part[w] > b ? bad_part[w] : b;
        if (b) atomicMax(status, region_status_word(b));
    }
    if (t >= VALUES) return;
    const int row = t / 7, v = t % 7;
    if (row > R) return;
    uint32_t cnt = 0;
    for (int w = 0; w < NT / 64; ++w) cnt += part[w][row * 7];
    if (cnt == 0) return;                                           // the workgroup saw no pixel of this row
    int64_t *out = stats + ((int64_t)img * (R + 1) + row) * HOIG_REGION_ROW + v;
    if (v < 3) {
        // at most 4096 pixels * 3 * 255^2 per workgroup: the sum of the four waves stays below 2^32
        uint32_t s = 0;
        for (int w = 0; w < NT / 64; ++w) s += part[w][t];
        atomicAdd(reinterpret_cast<unsigned long long *>(out), (unsigned long long)s);
    } else {
        int m = (int)part[0][t];
        for (int w = 1; w < NT / 64; ++w) {
            const int u = (int)part[w][t];
            m = v < 5 ? (u < m ? u : m) : (u > m ? u : m);
        }
        if (v < 5)
            atomicMin(reinterpret_cast<long long *>(out), (long long)m);
        else
            atomicMax(reinterpret_cast<long long *>(out), (long long)m);
    }
}

__global__ __launch_bounds__(NT) void boxes_kernel(const int64_t *__restrict__ stats, int N, int H, int W, int R, int min_pixels,
                                                   int32_t *boxes) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= N * R) return;
    const int n = i / R, r = i % R;
    region_box(stats + ((int64_t)n * (R + 1) + r + 1) * HOIG_REGION_ROW, H, W, min_pixels, boxes + (int64_t)i * 4);
}

__global__ __launch_bounds__(NT) void crop_h_kernel(const uint8_t *__restrict__ src, int N, int H, int W,
                                                    const int32_t *__restrict__ boxes, int R, int S,
                                                    const int32_t *__restrict__ tables, uint8_t *__restrict__ mid, int blocks_per_crop) {
    const int crop = blockIdx.x / blocks_per_crop, part = blockIdx.x % blocks_per_crop;     // crop = r * N + n
    const int r = crop / N, n = crop % N;
    int32_t box[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) box[v] = boxes[((int64_t)n * R + r) * 4 + v];
    if (!region_box_usable(box, H, W, S, tables)) return;
    const int total = box[2] * S * 3;                               // <= 4096 * 512 * 3
    const int e0 = (part * NT + threadIdx.x) * REGION_PER_LANE;
    if (e0 >= total) return;
    const uint8_t *img = src + (int64_t)n * H * W * 3;
    uint8_t *out = mid + (int64_t)crop * region_mid_stride(H, W, S);
    const int cnt = total - e0 < REGION_PER_LANE ? total - e0 : REGION_PER_LANE;
    uint32_t word = 0;
    for (int e = 0; e < cnt; ++e) word |= (uint32_t)region_crop_h_byte(img, W, box, S, tables, e0 + e) << (8 * e);
    if (cnt == REGION_PER_LANE) {
        *reinterpret_cast<uint32_t *>(out + e0) = word;             // e0 % 4 == 0, the crop's stride too, and mid is 4-byte aligned
    } else {
        for (int e = 0; e < cnt; ++e) out[e0 + e] = (uint8_t)(word >> (8 * e));
    }
}

__global__ __launch_bounds__(NT) void crop_v_kernel(const uint8_t *__restrict__ mid, int N, int H, int W,
                                                    const int32_t *__restrict__ boxes, int R, int S,
                                                    const int32_t *__restrict__ tables, uint8_t *__restrict__ dst, int64_t total) {
    const int per_crop = S * S * 3;
    const int64_t stride = region_mid_stride(H, W, S);
    for (int64_t i0 = ((int64_t)blockIdx.x * NT + threadIdx.x) * REGION_PER_LANE; i0 < total;
         i0 += (int64_t)gridDim.x * NT * REGION_PER_LANE) {
        const int cnt = total - i0 < REGION_PER_LANE ? (int)(total - i0) : REGION_PER_LANE;
        uint32_t word = 0;
        for (int e = 0; e < cnt; ++e) {
            const int64_t crop = (i0 + e) / per_crop;
            const int at = (int)((i0 + e) % per_crop), r = (int)(crop / N), n = (int)(crop % N);
            int32_t box[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) box[v] = boxes[((int64_t)n * R + r) * 4 + v];
            if (!region_box_usable(box, H, W, S, tables)) continue;
            word |= (uint32_t)region_crop_v_byte(mid + crop * stride, box, S, tables, at) << (8 * e);
        }
        if (cnt == REGION_PER_LANE) {
            *reinterpret_cast<uint32_t *>(dst + i0) = word;         // i0 % 4 == 0 and dst is 4-byte aligned (checked by the entry)
        } else {
            for (int e = 0; e < cnt; ++e) dst[i0 + e] = (uint8_t)(word >> (8 * e));
        }
    }
}

}  // namespace

extern "C" int hoig_region_stats_u8(const uint8_t *gen, const uint8_t *gt, const uint8_t *labels, int N, int H, int W, int R,
                                    int64_t *stats, int32_t *status, hoig_stream_t stream) {
    if (!gen || !gt || !labels || !stats || !status || !region_stats_ok(N, H, W, R)) return HOIG_EINVAL;
    if (((uintptr_t)stats & 7) || ((uintptr_t)status & 3)) return HOIG_EINVAL;
    const int chunks = (int)hoig_cdiv((int64_t)H * W, REGION_BLOCK_PIXELS);
    const int64_t blocks = (int64_t)N * chunks, rows = (int64_t)N * (R + 1);
    if (blocks >= ((int64_t)1 << 31)) return HOIG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int rc = hoig_launch<stats_init_kernel>(dim3((unsigned)hoig_cdiv(rows, NT)), dim3(NT), 0, st, stats, rows, H, W, status);
    if (rc != HOIG_OK) return rc;
    return hoig_launch<stats_kernel>(dim3((unsigned)blocks), dim3(NT), 0, st, gen, gt, labels, H, W, R, chunks, stats, status);
}

extern "C" int hoig_region_boxes(const int64_t *stats, int N, int H, int W, int R, int min_pixels, int32_t *boxes, hoig_stream_t stream) {
    if (!stats || !boxes || !region_stats_ok(N, H, W, R) || min_pixels < 0) return HOIG_EINVAL;
    if (((uintptr_t)stats & 7) || ((uintptr_t)boxes & 3) || (int64_t)N * R >= ((int64_t)1 << 31)) return HOIG_EINVAL;
    return hoig_launch<boxes_kernel>(dim3((unsigned)hoig_cdiv((int64_t)N * R, NT)), dim3(NT), 0, (hipStream_t)stream, stats, N, H, W, R,
                                     min_pixels, boxes);
}

extern "C" int hoig_region_crop_resize_u8(const uint8_t *src, int N, int H, int W, const int32_t *boxes, int R, int S,
                                          const int32_t *tables, uint8_t *dst, void *workspace, hoig_stream_t stream) {
    if (!src || !boxes || !tables || !dst || !workspace || !region_stats_ok(N, H, W, R) || !region_size_ok(S)) return HOIG_EINVAL;
    if (((uintptr_t)boxes & 3) || ((uintptr_t)tables & 3) || ((uintptr_t)dst & 3) || ((uintptr_t)workspace & 3)) return HOIG_EINVAL;
    const int max_side = H < W ? H : W;
    const int bpc = (int)hoig_cdiv((int64_t)max_side * S * 3, NT * REGION_PER_LANE);
    const int64_t blocks = (int64_t)R * N * bpc, total = (int64_t)R * N * S * S * 3;
    if (blocks >= ((int64_t)1 << 31)) return HOIG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *mid = static_cast<uint8_t *>(workspace);
    const int rc = hoig_launch<crop_h_kernel>(dim3((unsigned)blocks), dim3(NT), 0, st, src, N, H, W, boxes, R, S, tables, mid, bpc);
    if (rc != HOIG_OK) return rc;
    return hoig_launch<crop_v_kernel>(dim3((unsigned)hoig_stream_grid(hoig_cdiv(total, REGION_PER_LANE), NT)), dim3(NT), 0, st,
                                      (const uint8_t *)mid, N, H, W, boxes, R, S, tables, dst, total);
}
