// Laplacian-pyramid sliced Wasserstein distance on the device (docs/swd.md; the shared per-lane code, the tile sizes and the
// workspace layouts: swd.h).
//
// down_kernel: one step down the Gaussian chain.  A workgroup makes a 16 x 16 x 3 tile of g[l+1]: the horizontal pass of the 35
//   source rows it needs goes to LDS (swd_down_h, one value per thread and turn), the vertical pass reads five LDS rows (swd_tap5).
//   Level 0 is the uint8 input itself; the other levels are NHWC fp32 in the workspace.
// gather_kernel: one thread per descriptor value.  lap[l] is never stored: swd_lap_at takes g[l] at the pixel and the at most 3 x 3
//   values of g[l+1] that the step up reads there.
// stat_kernel / stat_finish_kernel: the chunked fp64 reductions of swd.h -- the sum, then sum (x - mean)^2 with the mean taken from
//   the first pass's partials by every workgroup in the same order.
// proj_kernel: a 64 x 64 tile of [rows, 147] x [147, dirs], K staged through LDS one channel (49 values) at a time, the operand
//   normalised on load; thread (rx, dy) owns rows 4 rx .. + 3 and directions 4 dy .. + 3 and walks k in order with fmaf -- plain fp32
//   FMA tiles: K = 147 is too thin for the MFMA's fill to pay and the order stays the twin's.  The output is direction-major.
// sort_lds_kernel: one workgroup per segment of at most SWD_SORT_LDS_MAX keys, a bitonic network over the next power of two in LDS.
// sort_hist / sort_scan / sort_scatter: an 8-bit LSD radix pass for longer segments.  Tiles of SWD_SORT_TILE keys; counts
//   [segment][digit][tile]; the scan gives every (digit, tile) its first output position; the scatter is one wave per tile that walks
//   its keys 64 at a time in order, ranks equal digits by ballots and keeps the running positions in LDS: equal digits keep their
//   order, which is what the next pass relies on.  Integer LDS atomics only (the counts).  No pass waits on another workgroup.
// l1_kernel / l1_finish_kernel: sum |a - b| in fp64, a partial per workgroup and a finishing wave.
// Built with -ffp-contract=off.
#include "common.h"
#include "swd.h"

namespace {

constexpr int NT = SWD_NT;
constexpr int DT = SWD_DOWN_TILE;
constexpr int DROWS = 2 * DT + 3;
constexpr int PT = SWD_PROJ_TILE;
constexpr int PLDA = PT + 4;                 // floats of a row of the A panel (16-byte aligned rows)

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, SWD_WAVE);
    return v;
}

// every thread of the workgroup calls it; every thread gets the sum
__device__ __forceinline__ double block_sum(double v, double *wsum) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// ---------------------------------------------------------------- positions
__global__ __launch_bounds__(NT) void positions_kernel(uint64_t seed, int set_id, int64_t first, int n, int H, int W, int L, int patches,
                                                       int32_t *pos) {
    const int64_t total = (int64_t)n * L * patches, i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const int p = (int)(i % patches), l = (int)((i / patches) % L), img = (int)(i / ((int64_t)patches * L));
    int y0, x0;
    swd_position(seed, set_id, l, first + img, p, H >> l, W >> l, &y0, &x0);
    pos[2 * i] = y0, pos[2 * i + 1] = x0;
}

// ---------------------------------------------------------------- the Gaussian chain
template <class T>
__global__ __launch_bounds__(NT) void down_kernel(const T *__restrict__ in, int H, int W, float *__restrict__ out, int tiles_x,
                                                  int tiles_y) {
    __shared__ float hbuf[DROWS][DT][3];
    const int Ho = H >> 1, Wo = W >> 1;
    const int b = blockIdx.x, tx = b % tiles_x, ty = (b / tiles_x) % tiles_y, img = b / (tiles_x * tiles_y);
    const int y0 = ty * DT, x0 = tx * DT, t = threadIdx.x;
    const T *src = in + (int64_t)img * H * W * 3;
    for (int e = t; e < DROWS * DT * 3; e += NT) {
        const int c = e % 3, xx = (e / 3) % DT, r = e / (3 * DT);
        const int s = 2 * y0 + r - 2, xo = x0 + xx;
        if (xo < Wo && s <= H + 1) hbuf[r][xx][c] = swd_down_h(src, W, swd_mirror(s, H), xo, c);
    }
    __syncthreads();
    float *dst = out + (int64_t)img * Ho * Wo * 3;
    for (int e = t; e < DT * DT * 3; e += NT) {
        const int c = e % 3, xx = (e / 3) % DT, yy = e / (3 * DT);
        const int yo = y0 + yy, xo = x0 + xx;
        if (yo < Ho && xo < Wo)
            dst[((int64_t)yo * Wo + xo) * 3 + c] = swd_tap5(hbuf[2 * yy][xx][c], hbuf[2 * yy + 1][xx][c], hbuf[2 * yy + 2][xx][c],
                                                            hbuf[2 * yy + 3][xx][c], hbuf[2 * yy + 4][xx][c]);
    }
}

// ---------------------------------------------------------------- the patches of the Laplacian levels
__global__ __launch_bounds__(NT) void gather_kernel(const uint8_t *__restrict__ u8, const float *__restrict__ chain, int n, int H, int W,
                                                    int L, int patches, const int32_t *__restrict__ pos, float *__restrict__ out,
                                                    int64_t total) {
    for (int64_t v = (int64_t)blockIdx.x * NT + threadIdx.x; v < total; v += (int64_t)gridDim.x * NT) {
        const int e = (int)(v % SWD_K);
        const int64_t q = v / SWD_K;
        const int p = (int)(q % patches), img = (int)((q / patches) % n), l = (int)(q / ((int64_t)patches * n));
        const int Hl = H >> l, Wl = W >> l;
        const int32_t *at = pos + (((int64_t)img * L + l) * patches + p) * 2;
        const int y = swd_clamp(at[0], Hl - SWD_PATCH) + (e % SWD_PLANE) / SWD_PATCH, x = swd_clamp(at[1], Wl - SWD_PATCH) + e % SWD_PATCH;
        const int c = e / SWD_PLANE;
        const float *next = nullptr;
        if (l + 1 < L) next = chain + swd_chain_floats(n, H, W, l + 1) + (int64_t)img * (Hl >> 1) * (Wl >> 1) * 3;
        if (l == 0)
            out[v] = swd_lap_at(u8 + (int64_t)img * H * W * 3, Hl, Wl, next, y, x, c);
        else
            out[v] = swd_lap_at(chain + swd_chain_floats(n, H, W, l) + (int64_t)img * Hl * Wl * 3, Hl, Wl, next, y, x, c);
    }
}

// ---------------------------------------------------------------- channel statistics
// partials: [2 passes][3 channels][SWD_MAX_PARTS] doubles
template <bool SQUARE>
__global__ __launch_bounds__(NT) void stat_kernel(const float *__restrict__ desc, int64_t E, int parts, double *partials) {
    __shared__ double wsum[4];
    const int part = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
    double pivot = 0.0;
    if (SQUARE) pivot = wave_sum(swd_lane_partials(partials + c * SWD_MAX_PARTS, parts, t & 63)) / (double)E;
    const double s = block_sum(swd_stat_thread(desc, E, c, part, t, pivot, SQUARE), wsum);
    if (t == 0) partials[((SQUARE ? 3 : 0) + c) * SWD_MAX_PARTS + part] = s;
}

__global__ __launch_bounds__(SWD_WAVE) void stat_finish_kernel(const double *__restrict__ partials, int64_t E, int parts, double *stats,
                                                               int32_t *status) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const double sum = wave_sum(swd_lane_partials(partials + c * SWD_MAX_PARTS, parts, lane));
    const double sq = wave_sum(swd_lane_partials(partials + (3 + c) * SWD_MAX_PARTS, parts, lane));
    if (lane != 0) return;
    const double sd = sqrt(sq / (double)E);
    stats[2 * c] = sum / (double)E;
    stats[2 * c + 1] = sd;
    if (!(sd > 0.0)) atomicOr(status, 1 << c);
}

// ---------------------------------------------------------------- projection
__global__ __launch_bounds__(NT) void proj_kernel(const float *__restrict__ desc, int64_t rows, const double *__restrict__ stats,
                                                  const float *__restrict__ dirs, int D, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float As[SWD_PLANE][PLDA];
    __shared__ __attribute__((aligned(16))) float Bs[SWD_PLANE][PT];
    const int64_t r0 = (int64_t)blockIdx.x * PT;
    const int d0 = blockIdx.y * PT, t = threadIdx.x, rx = t & 15, dy = t >> 4;
    float acc[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = 0.f;
    for (int c = 0; c < 3; ++c) {
        const double mean = stats[2 * c], sd = stats[2 * c + 1];
        __syncthreads();                                  // the previous panel has been read
        for (int e = t; e < PT * SWD_PLANE; e += NT) {
            const int row = e / SWD_PLANE, kk = e - row * SWD_PLANE;
            const int64_t r = r0 + row;
            As[kk][row] = r < rows ? swd_normalised(desc[r * SWD_K + c * SWD_PLANE + kk], mean, sd) : 0.f;
        }
        for (int e = t; e < PT * SWD_PLANE; e += NT) {
            const int kk = e / PT, d = e - kk * PT;
            Bs[kk][d] = d0 + d < D ? dirs[(int64_t)(c * SWD_PLANE + kk) * D + d0 + d] : 0.f;
        }
        __syncthreads();
        for (int kk = 0; kk < SWD_PLANE; ++kk) {
            const float4 a4 = *reinterpret_cast<const float4 *>(&As[kk][4 * rx]);
            const float4 b4 = *reinterpret_cast<const float4 *>(&Bs[kk][4 * dy]);
            const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[j][i] = fmaf(a[i], b[j], acc[j][i]);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = d0 + 4 * dy + j;
        if (d >= D) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t r = r0 + 4 * rx + i;
            if (r < rows) out[(int64_t)d * rows + r] = acc[j][i];
        }
    }
}

// ---------------------------------------------------------------- the sort: short segments
__global__ __launch_bounds__(NT) void sort_lds_kernel(float *keys, int n, int p2, int32_t *status) {
    __shared__ uint32_t s[SWD_SORT_LDS_MAX];
    uint32_t *seg = reinterpret_cast<uint32_t *>(keys) + (int64_t)blockIdx.x * n;
    const int t = threadIdx.x;
    bool nan = false;
    for (int i = t; i < p2; i += NT) {
        uint32_t k = 0xFFFFFFFFu;
        if (i < n) {
            const uint32_t bits = seg[i];
            nan |= swd_bits_nan(bits);
            k = swd_key_encode(bits);
        }
        s[i] = k;
    }
    if (nan) atomicOr(status, HOIG_SORT_NAN);
    __syncthreads();
    for (int k = 2; k <= p2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < p2; i += NT) {
                const int o = i ^ j;
                if (o > i) {
                    const uint32_t a = s[i], b = s[o];
                    if ((a > b) == ((i & k) == 0)) s[i] = b, s[o] = a;
                }
            }
            __syncthreads();
        }
    for (int i = t; i < n; i += NT) seg[i] = swd_key_decode(s[i]);
}

// ---------------------------------------------------------------- the sort: one radix pass
// hist: [S][256][nb] uint32
template <bool FIRST>
__global__ __launch_bounds__(NT) void sort_hist_kernel(const uint32_t *__restrict__ in, int64_t n, int nb, int shift, uint32_t *hist,
                                                       int32_t *status) {
    __shared__ uint32_t cnt[256];
    const int t = threadIdx.x;
    const int64_t seg = blockIdx.x / nb, blk = blockIdx.x % nb;
    cnt[t] = 0;
    __syncthreads();
    const uint32_t *src = in + seg * n;
    const int64_t lo = blk * SWD_SORT_TILE, hi = lo + SWD_SORT_TILE < n ? lo + SWD_SORT_TILE : n;
    bool nan = false;
    for (int64_t i = lo + t; i < hi; i += NT) {
        uint32_t k = src[i];
        if (FIRST) nan |= swd_bits_nan(k), k = swd_key_encode(k);
        atomicAdd(&cnt[(k >> shift) & 255u], 1u);
    }
    if (FIRST && nan) atomicOr(status, HOIG_SORT_NAN);
    __syncthreads();
    hist[(seg * 256 + t) * nb + blk] = cnt[t];
}

// one workgroup per segment; thread d owns digit d: its tiles' counts become their first output positions
__global__ __launch_bounds__(NT) void sort_scan_kernel(uint32_t *hist, int nb) {
    __shared__ uint32_t tot[256];
    const int d = threadIdx.x;
    uint32_t *mine = hist + ((int64_t)blockIdx.x * 256 + d) * nb;
    uint32_t sum = 0;
    for (int b = 0; b < nb; ++b) sum += mine[b];
    tot[d] = sum;
    __syncthreads();
    uint32_t run = 0;
    for (int e = 0; e < d; ++e) run += tot[e];
    for (int b = 0; b < nb; ++b) {
        const uint32_t c = mine[b];
        mine[b] = run;
        run += c;
    }
}

// one wave per tile
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(SWD_WAVE) void sort_scatter_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, int64_t n,
                                                                int nb, int shift, const uint32_t *__restrict__ hist) {
    __shared__ uint32_t base[256];
    const int lane = threadIdx.x;
    const int64_t seg = blockIdx.x / nb, blk = blockIdx.x % nb;
    for (int d = lane; d < 256; d += SWD_WAVE) base[d] = hist[(seg * 256 + d) * nb + blk];
    __syncthreads();
    const uint32_t *src = in + seg * n;
    uint32_t *dst = out + seg * n;
    const int64_t lo = blk * SWD_SORT_TILE, hi = lo + SWD_SORT_TILE < n ? lo + SWD_SORT_TILE : n;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t i0 = lo; i0 < hi; i0 += SWD_WAVE) {
        const int64_t i = i0 + lane;
        const bool live = i < hi;
        uint32_t k = live ? src[i] : 0u;
        if (FIRST) k = swd_key_encode(k);
        const uint32_t digit = (k >> shift) & 255u;
        unsigned long long same = __ballot(live);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (digit >> b) & 1u;
            const unsigned long long votes = __ballot(bit);
            same &= bit ? votes : ~votes;
        }
        const int rank = __popcll(same & below);
        const uint32_t first = live ? base[digit] : 0u;
        __syncthreads();                                  // every lane has read the position before a leader moves it
        if (live && rank == 0) base[digit] = first + (uint32_t)__popcll(same);
        __syncthreads();
        const int64_t to = (int64_t)first + rank;
        if (live && to < n) dst[to] = LAST ? swd_key_decode(k) : k;
    }
}

// ---------------------------------------------------------------- sorted L1
__global__ __launch_bounds__(NT) void l1_kernel(const float *__restrict__ a, const float *__restrict__ b, int64_t N, double *partials) {
    __shared__ double wsum[4];
    const double s = block_sum(swd_l1_thread(a, b, N, blockIdx.x, threadIdx.x), wsum);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(SWD_WAVE) void l1_finish_kernel(const double *__restrict__ partials, int parts, double *out) {
    const double s = wave_sum(swd_lane_partials(partials, parts, threadIdx.x));
    if (threadIdx.x == 0) out[0] = s;
}

template <bool FIRST, bool LAST>
int radix_pass(const uint32_t *in, uint32_t *out, int64_t S, int64_t n, int nb, int shift, uint32_t *hist, int32_t *status, hipStream_t st) {
    const dim3 grid((unsigned)(S * nb));
    int rc = hoig_launch<sort_hist_kernel<FIRST>>(grid, dim3(NT), 0, st, in, n, nb, shift, hist, status);
    if (rc != HOIG_OK) return rc;
    rc = hoig_launch<sort_scan_kernel>(dim3((unsigned)S), dim3(NT), 0, st, hist, nb);
    if (rc != HOIG_OK) return rc;
    return hoig_launch<sort_scatter_kernel<FIRST, LAST>>(grid, dim3(SWD_WAVE), 0, st, in, out, n, nb, shift, (const uint32_t *)hist);
}

}  // namespace

extern "C" int hoig_swd_positions(uint64_t seed, int set_id, int64_t first_index, int n, int H, int W, int L, int patches,
                                  int32_t *positions, hoig_stream_t stream) {
    if (!positions || ((uintptr_t)positions & 3) || first_index < 0 || !swd_desc_ok(n, H, W, L, patches)) return HOIG_EINVAL;
    const int64_t total = (int64_t)n * L * patches;
    return hoig_launch<positions_kernel>(dim3((unsigned)hoig_cdiv(total, NT)), dim3(NT), 0, (hipStream_t)stream, seed, set_id, first_index,
                                         n, H, W, L, patches, positions);
}

extern "C" int hoig_swd_descriptors_u8(const uint8_t *u8, int n, int H, int W, int L, int patches, const int32_t *positions, float *out,
                                       void *workspace, int64_t workspace_bytes, hoig_stream_t stream) {
    if (!u8 || !positions || !out || !workspace || !swd_desc_ok(n, H, W, L, patches)) return HOIG_EINVAL;
    if (((uintptr_t)positions & 3) || ((uintptr_t)out & 3) || ((uintptr_t)workspace & 7)) return HOIG_EINVAL;
    if (workspace_bytes < hoig_swd_descriptors_workspace_bytes(n, H, W, L)) return HOIG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    float *chain = static_cast<float *>(workspace);
    for (int l = 0; l + 1 < L; ++l) {
        const int Hl = H >> l, Wl = W >> l;
        const int tx = (int)hoig_cdiv(Wl >> 1, DT), ty = (int)hoig_cdiv(Hl >> 1, DT);
        const int64_t blocks = (int64_t)n * tx * ty;
        if (blocks >= ((int64_t)1 << 31)) return HOIG_EINVAL;
        float *dst = chain + swd_chain_floats(n, H, W, l + 1);
        const int rc = l == 0 ? hoig_launch<down_kernel<uint8_t>>(dim3((unsigned)blocks), dim3(NT), 0, st, u8, Hl, Wl, dst, tx, ty)
                              : hoig_launch<down_kernel<float>>(dim3((unsigned)blocks), dim3(NT), 0, st,
                                                                (const float *)(chain + swd_chain_floats(n, H, W, l)), Hl, Wl, dst, tx, ty);
        if (rc != HOIG_OK) return rc;
    }
    const int64_t total = (int64_t)n * L * patches * SWD_K;
    return hoig_launch<gather_kernel>(dim3((unsigned)hoig_stream_grid(total, NT)), dim3(NT), 0, st, u8, (const float *)chain, n, H, W, L,
                                      patches, positions, out, total);
}

extern "C" int hoig_swd_channel_stats_f64(const float *desc, int64_t rows, double *stats, int32_t *status, void *workspace,
                                          int64_t workspace_bytes, hoig_stream_t stream) {
    if (!desc || !stats || !status || !workspace || rows < 1 || rows >= ((int64_t)1 << 32)) return HOIG_EINVAL;
    if (((uintptr_t)desc & 3) || ((uintptr_t)stats & 7) || ((uintptr_t)workspace & 7)) return HOIG_EINVAL;
    if (workspace_bytes < hoig_swd_channel_stats_workspace_bytes(rows)) return HOIG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int64_t E = rows * SWD_PLANE;
    const int parts = swd_parts(E);
    double *partials = static_cast<double *>(workspace);
    if (hipMemsetAsync(status, 0, sizeof(int32_t), st) != hipSuccess) return HOIG_ELAUNCH;
    int rc = hoig_launch<stat_kernel<false>>(dim3((unsigned)parts, 3), dim3(NT), 0, st, desc, E, parts, partials);
    if (rc != HOIG_OK) return rc;
    rc = hoig_launch<stat_kernel<true>>(dim3((unsigned)parts, 3), dim3(NT), 0, st, desc, E, parts, partials);
    if (rc != HOIG_OK) return rc;
    return hoig_launch<stat_finish_kernel>(dim3(3), dim3(SWD_WAVE), 0, st, (const double *)partials, E, parts, stats, status);
}

extern "C" int hoig_swd_project_f32(const float *desc, int64_t rows, const double *stats, const float *dirs, int D, float *out,
                                    hoig_stream_t stream) {
    if (!desc || !stats || !dirs || !out || rows < 1 || D < 1 || D > 65535 * PT) return HOIG_EINVAL;
    if (((uintptr_t)desc & 3) || ((uintptr_t)stats & 7) || ((uintptr_t)dirs & 3) || ((uintptr_t)out & 3)) return HOIG_EINVAL;
    const int64_t tiles = hoig_cdiv(rows, PT);
    if (tiles >= ((int64_t)1 << 31) || rows * D >= ((int64_t)1 << 40)) return HOIG_EINVAL;
    return hoig_launch<proj_kernel>(dim3((unsigned)tiles, (unsigned)hoig_cdiv(D, PT)), dim3(NT), 0, (hipStream_t)stream, desc, rows, stats,
                                    dirs, D, out);
}

extern "C" int hoig_sort_segments_f32(float *keys, int64_t S, int64_t n, void *workspace, int32_t *status, hoig_stream_t stream) {
    if (!swd_sort_ok(keys, S, n) || !status || !workspace || ((uintptr_t)workspace & 7)) return HOIG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int32_t), st) != hipSuccess) return HOIG_ELAUNCH;
    if (n <= SWD_SORT_LDS_MAX) {
        if (S >= ((int64_t)1 << 31)) return HOIG_EINVAL;
        return hoig_launch<sort_lds_kernel>(dim3((unsigned)S), dim3(NT), 0, st, keys, (int)n, swd_next_pow2((int)n), status);
    }
    const int nb = (int)swd_sort_tiles(n);
    uint32_t *a = reinterpret_cast<uint32_t *>(keys), *b = static_cast<uint32_t *>(workspace), *hist = b + S * n;
    int rc = radix_pass<true, false>(a, b, S, n, nb, 0, hist, status, st);
    if (rc != HOIG_OK) return rc;
    rc = radix_pass<false, false>(b, a, S, n, nb, 8, hist, status, st);
    if (rc != HOIG_OK) return rc;
    rc = radix_pass<false, false>(a, b, S, n, nb, 16, hist, status, st);
    if (rc != HOIG_OK) return rc;
    return radix_pass<false, true>(b, a, S, n, nb, 24, hist, status, st);
}

extern "C" int hoig_swd_sorted_l1_f64(const float *a, const float *b, int64_t N, double *out, void *workspace, int64_t workspace_bytes,
                                      hoig_stream_t stream) {
    if (!a || !b || !out || !workspace || N < 1 || N >= ((int64_t)1 << 40)) return HOIG_EINVAL;
    if (((uintptr_t)a & 3) || ((uintptr_t)b & 3) || ((uintptr_t)out & 7) || ((uintptr_t)workspace & 7)) return HOIG_EINVAL;
    if (workspace_bytes < hoig_swd_sorted_l1_workspace_bytes(N)) return HOIG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int parts = swd_parts(N);
    double *partials = static_cast<double *>(workspace);
    const int rc = hoig_launch<l1_kernel>(dim3((unsigned)parts), dim3(NT), 0, st, a, b, N, partials);
    if (rc != HOIG_OK) return rc;
    return hoig_launch<l1_finish_kernel>(dim3(1), dim3(SWD_WAVE), 0, st, (const double *)partials, parts, out);
}
