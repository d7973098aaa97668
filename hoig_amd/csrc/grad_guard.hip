// Gradient guard on the device (docs/grad_guard.md; the shared per-lane code, the summation order and the workspace layout:
// grad_guard.h).  hoig_grad_stats is two launches -- per-chunk partials, then one workgroup per result that joins them in a fixed
// order -- and hoig_guard_decide one thread.  Nothing here synchronises, allocates or waits for another workgroup; there are no
// floating-point atomics.  Built with -ffp-contract=off.
#include "common.h"
#include "grad_guard.h"

namespace {

__device__ __forceinline__ gg_acc wave_join(gg_acc a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        gg_acc b;
        b.s = __shfl_xor(a.s, o, GG_WAVE);
        b.mx = __shfl_xor(a.mx, o, GG_WAVE);
        b.nf = __shfl_xor(a.nf, o, GG_WAVE);
        a = gg_join(a, b);
    }
    return a;
}

__device__ __forceinline__ void store3(double *p, const gg_acc &a) { p[0] = a.s, p[1] = a.mx, p[2] = a.nf; }

// stage 1: workgroups walk the chunks; `vec`: x is 16-byte aligned, so a whole chunk is read as four 16-byte loads per thread, all in
// flight before the first is used (the order of the additions is gg_thread_chunk's either way)
__global__ __launch_bounds__(GG_NT) void stats_chunks_kernel(const float *__restrict__ x, int64_t n, const int64_t *__restrict__ segs,
                                                             int nseg, int64_t nchunk, double *__restrict__ chunk_part,
                                                             double *__restrict__ piece_part, int vec) {
    __shared__ gg_acc sh[GG_NT / GG_WAVE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int64_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
        const int64_t base = c * GG_CHUNK;
        const int cnt = (int)(n - base < GG_CHUNK ? n - base : GG_CHUNK);
        gg_acc a;
        if (vec && cnt == GG_CHUNK) {
            float4 q[GG_SLOTS];
#pragma unroll
            for (int j = 0; j < GG_SLOTS; ++j) q[j] = *reinterpret_cast<const float4 *>(x + base + 4 * (t + GG_NT * j));
            a = gg_zero();
#pragma unroll
            for (int j = 0; j < GG_SLOTS; ++j) {
                gg_take(a, q[j].x);
                gg_take(a, q[j].y);
                gg_take(a, q[j].z);
                gg_take(a, q[j].w);
            }
        } else {
            a = gg_thread_chunk(x, base, cnt, t);
        }
        a = wave_join(a);
        if (lane == 0) sh[wave] = a;
        __syncthreads();
        const gg_acc tot = gg_join(gg_join(gg_join(sh[0], sh[1]), sh[2]), sh[3]);
        if (t == 0) store3(chunk_part + 3 * c, tot);
        if (nseg > 0) {
            const int64_t end = base + cnt;
            int i = 0;
            for (int s = gg_first_row(segs, nseg, base); s < nseg; ++s, ++i) {
                const int64_t f = segs[2 * s];
                if (f >= end) break;
                const int64_t b = f > base ? f : base, e = f + segs[2 * s + 1] < end ? f + segs[2 * s + 1] : end;
                if (e <= b) continue;
                if (b == base && e == end) {
                    if (t == 0) store3(piece_part + 3 * (c + s), tot);
                } else if ((i & 3) == wave) {                 // (wave-uniform)
                    const gg_acc p = wave_join(gg_lane_piece(x, b, e, lane));
                    if (lane == 0) store3(piece_part + 3 * (c + s), p);
                }
            }
        }
        __syncthreads();                                      // (sh is written again by the next chunk)
    }
}

// stage 2: workgroup 0 joins the chunk partials into `total`, workgroup 1 + s the pieces of row s into seg_out[s]
__global__ __launch_bounds__(GG_NT2) void stats_join_kernel(const int64_t *__restrict__ segs, int64_t nchunk,
                                                            const double *__restrict__ chunk_part, const double *__restrict__ piece_part,
                                                            double *__restrict__ seg_out, double *__restrict__ total) {
    __shared__ gg_acc sh[GG_NT2 / GG_WAVE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const double *parts = chunk_part;
    double *out = total;
    int64_t first = 0, last = nchunk;
    if (blockIdx.x > 0) {
        const int s = (int)blockIdx.x - 1;
        gg_row_slots(segs, s, nchunk, &first, &last);
        parts = piece_part, out = seg_out + 3 * (int64_t)s;
    }
    const gg_acc a = wave_join(gg_thread_parts(parts, first, last, t));
    if (lane == 0) sh[wave] = a;
    __syncthreads();
    if (t == 0) {
        gg_acc r = sh[0];
        for (int w = 1; w < GG_NT2 / GG_WAVE; ++w) r = gg_join(r, sh[w]);
        store3(out, r);
    }
}

__global__ void decide_kernel(const double *__restrict__ total, double pre_scale, double max_norm, int flags, float *__restrict__ guard,
                              double *__restrict__ record) {
    if (threadIdx.x == 0 && blockIdx.x == 0) gg_decide(total, pre_scale, max_norm, flags, guard, record);
}

}  // namespace

extern "C" int hoig_grad_stats(const float *x, int64_t n, const int64_t *segs_host, const int64_t *segs_dev, int nseg, double *seg_out,
                               double *total, void *workspace, hoig_stream_t stream) {
    if (!x || !total || !workspace || ((uintptr_t)x & 3) || ((uintptr_t)workspace & 7) || !gg_table_ok(n, segs_host, nseg) ||
        (nseg > 0 && (!segs_dev || !seg_out)))
        return HOIG_EINVAL;
    const int64_t nchunk = gg_chunks(n);
    double *chunk_part = static_cast<double *>(workspace), *piece_part = chunk_part + 3 * nchunk;
    const unsigned grid = (unsigned)(nchunk < GG_MAX_GRID ? nchunk : GG_MAX_GRID);
    stats_chunks_kernel<<<grid, GG_NT, 0, (hipStream_t)stream>>>(x, n, segs_dev, nseg, nchunk, chunk_part, piece_part,
                                                                 ((uintptr_t)x & 15) == 0);
    HOIG_LAUNCH_CHECK();
    stats_join_kernel<<<(unsigned)(1 + nseg), GG_NT2, 0, (hipStream_t)stream>>>(segs_dev, nchunk, chunk_part, piece_part, seg_out, total);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}

extern "C" int hoig_guard_decide(const double *total, double pre_scale, double max_norm, int flags, float *guard, double *record,
                                 hoig_stream_t stream) {
    if (!total || !guard || !record || (flags & ~HOIG_GUARD_SKIP) || !(pre_scale > 0.0) || !(max_norm >= 0.0)) return HOIG_EINVAL;
    decide_kernel<<<1, 64, 0, (hipStream_t)stream>>>(total, pre_scale, max_norm, flags, guard, record);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}
