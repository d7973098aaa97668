// The packed weight planes of the 16-bit convolution kernels (layout: plane_index of conv_bf16_common.h) and the optimiser step that
// writes them: the packers of one weight and of every weight of a flat parameter buffer, and Adam fused with the pack
// (docs/optimizer_parity.md; the guarded form: docs/grad_guard.md).
#include "conv_bf16_common.h"

namespace {
using namespace hoig_detail;

// forward planes: fp16 split of w * 2^8;   data-gradient planes: bf16 split of w
__device__ __forceinline__ void split_weight(float x, bool f16, unsigned short &h, unsigned short &l) {
    if (f16) {
        const float xs = x * W_SCALE_F16;
        // (the compiler folds product and conversion into one fma(x, 256, +0) -> fp16, which turns x = -0 into +0: hi takes the sign
        //  of x back -- every other result has it already -- so that hi is fp16(256 x) to the bit and lo = +0 for either zero)
        h = __builtin_bit_cast(unsigned short, (_Float16)xs) | (unsigned short)((__float_as_uint(x) >> 16) & 0x8000u);
        const _Float16 hh = __builtin_bit_cast(_Float16, h);
        const _Float16 ll = (_Float16)(xs - (float)hh);
        l = __builtin_bit_cast(unsigned short, ll);
    } else {
        h = hoig_f2bf(x);
        l = hoig_f2bf(x - hoig_bf2f(h));
    }
}

// w: fp32 [Co][RS][Ci].  mode 0 -> plane rows n = co, k = (rs, ci) (forward); mode 1 -> rows n = ci, k = (rs, co) (data
// gradient); both in the blocked plane layout (plane_index)
__global__ void pack_weight_kernel(const float *__restrict__ w, int Co, int RS, int Ci, int mode,
                                   unsigned short *__restrict__ hi, unsigned short *__restrict__ lo) {
    const int64_t n = (int64_t)Co * RS * Ci;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int ci = (int)(i % Ci);
        const int64_t t = i / Ci;
        const int rs = (int)(t % RS), co = (int)(t / RS);
        const size_t dst = mode == 1 ? plane_index(ci, rs * Co + co, RS * Co) : plane_index(co, rs * Ci + ci, RS * Ci);
        unsigned short h, l;
        split_weight(w[i], mode == 0, h, l);
        hi[dst] = h;
        if (lo) lo[dst] = l;
    }
}

// Every conv weight of a network in ONE launch: `segs` holds (offset, Co, RS, Ci, flags, first tile) per weight of the
// flat parameter buffer; the planes of a weight land at the weight's own offset in the plane buffers.  A workgroup owns one
// 32(co) x 32(ci) tile of one weight (binary search over the tile prefix) and walks its RS taps: rows are read coalesced
// along ci, the forward planes written in place, the data-gradient planes ([Ci][RS][Co]) written coalesced along co after a
// transpose through LDS.
__global__ __launch_bounds__(256) void pack_all_kernel(const float *__restrict__ flat, const int64_t *__restrict__ segs,
                                                       int nseg, unsigned short *__restrict__ hi_f,
                                                       unsigned short *__restrict__ lo_f,
                                                       unsigned short *__restrict__ hi_d,
                                                       unsigned short *__restrict__ lo_d) {
    int lo_s = 0, hi_s = nseg - 1;
    while (lo_s < hi_s) {                 // last segment whose first tile <= blockIdx.x
        const int mid = (lo_s + hi_s + 1) >> 1;
        if (segs[(int64_t)mid * 6 + 5] <= (int64_t)blockIdx.x) lo_s = mid; else hi_s = mid - 1;
    }
    const int64_t *sg = segs + (int64_t)lo_s * 6;
    const int64_t off = sg[0];
    const int Co = (int)sg[1], RS = (int)sg[2], Ci = (int)sg[3], flags = (int)sg[4];
    const int t = (int)((int64_t)blockIdx.x - sg[5]);
    const int tiles_ci = (Ci + 31) >> 5;
    const int co0 = (t / tiles_ci) * 32, ci0 = (t % tiles_ci) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    __shared__ unsigned int tile[32][33];
    const float *w = flat + off;
    for (int rs = 0; rs < RS; ++rs) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int co = co0 + ty + 8 * k, ci = ci0 + tx;
            unsigned int pk = 0;
            if (co < Co && ci < Ci) {
                const int64_t i = ((int64_t)co * RS + rs) * Ci + ci;
                const float x = w[i];
                unsigned short h, l;
                if (flags & 1) {
                    split_weight(x, true, h, l);
                    const size_t o = off + plane_index(co, rs * Ci + ci, RS * Ci);
                    hi_f[o] = h;
                    lo_f[o] = l;
                }
                split_weight(x, false, h, l);
                pk = (unsigned int)h | ((unsigned int)l << 16);
            }
            tile[ty + 8 * k][tx] = pk;
        }
        if (flags & 2) {
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ci = ci0 + ty + 8 * k, co = co0 + tx;
                if (co < Co && ci < Ci) {
                    const unsigned int pk = tile[tx][ty + 8 * k];
                    const size_t o = off + plane_index(ci, rs * Co + co, RS * Co);
                    hi_d[o] = (unsigned short)(pk & 0xffffu);
                    lo_d[o] = (unsigned short)(pk >> 16);
                }
            }
            __syncthreads();
        }
    }
}

// Adam and the operand split in ONE pass over the weights (hoig_adam_pack_step): the update of a convolution weight and its
// four 16-bit planes used to be two launches -- Adam over the flat buffer (28 B per parameter), then pack_all_kernel re-reading
// every updated weight (4 B) and writing the planes with 2-byte stores -- at the END of a step, where nothing runs beside them.
// Here a workgroup owns one 32(co) x 32(ci) tile of one weight as in pack_all_kernel; a thread updates FOUR consecutive input
// channels (float4 of p, g, m, v; the arithmetic of adam_dev_kernel, expression for expression) and writes their forward planes
// as 8-byte stores; the data-gradient planes go through the same LDS transpose, four output channels per thread.  Workgroups
// past the tile count do the plain update of the parameters that have no planes (`plain`: 1024-element chunks).
// GUARD (hoig_adam_pack_step_guarded, docs/grad_guard.md): `guard` = {scale, skip}; a skipped step returns before the first load (the
// whole workgroup does: no barrier is left waiting), otherwise the gradient's factor is gscale * guard[0].
template <bool GUARD>
__global__ __launch_bounds__(256) void adam_pack_kernel(float *__restrict__ flat, const float *__restrict__ grad, float *__restrict__ m_,
                                                        float *__restrict__ v_, const float *__restrict__ derived, float gscale,
                                                        const int64_t *__restrict__ segs, int nseg, int64_t ntiles,
                                                        const int64_t *__restrict__ plain, unsigned short *__restrict__ hi_f,
                                                        unsigned short *__restrict__ lo_f, unsigned short *__restrict__ hi_d,
                                                        unsigned short *__restrict__ lo_d, const float *__restrict__ guard) {
    if constexpr (GUARD) {
        if (guard[1] != 0.f) return;
        gscale = gscale * guard[0];
    }
    const float step_size = derived[0], omb1 = derived[1], b2 = derived[2], omb2 = derived[3], eps = derived[4], bc2_sqrt = derived[5];
    struct Q { float4 p, g, m, v; };
    auto load4 = [&](int64_t i) -> Q {
        Q q;
        q.p = *reinterpret_cast<const float4 *>(flat + i);
        q.g = *reinterpret_cast<const float4 *>(grad + i);
        q.m = *reinterpret_cast<const float4 *>(m_ + i);
        q.v = *reinterpret_cast<const float4 *>(v_ + i);
        return q;
    };
    auto update4 = [&](Q q, int64_t i) -> float4 {
        float *pe = &q.p.x, *me = &q.m.x, *ve = &q.v.x;
        const float *ge = &q.g.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gk = ge[k] * gscale;
            me[k] = me[k] + (gk - me[k]) * omb1;
            ve[k] = ve[k] * b2 + omb2 * (gk * gk);
            const float denom = sqrtf(ve[k]) / bc2_sqrt + eps;
            pe[k] = pe[k] - step_size * (me[k] / denom);
        }
        *reinterpret_cast<float4 *>(flat + i) = q.p;
        *reinterpret_cast<float4 *>(m_ + i) = q.m;
        *reinterpret_cast<float4 *>(v_ + i) = q.v;
        return q.p;
    };
    if ((int64_t)blockIdx.x >= ntiles) {
        const int64_t *c = plain + 2 * ((int64_t)blockIdx.x - ntiles);
        const int e = 4 * (int)threadIdx.x;
        if (e < (int)c[1]) update4(load4(c[0] + e), c[0] + e);
        return;
    }
    int lo_s = 0, hi_s = nseg - 1;
    while (lo_s < hi_s) {                 // last segment whose first tile <= blockIdx.x
        const int mid = (lo_s + hi_s + 1) >> 1;
        if (segs[(int64_t)mid * 6 + 5] <= (int64_t)blockIdx.x) lo_s = mid; else hi_s = mid - 1;
    }
    const int64_t *sg = segs + (int64_t)lo_s * 6;
    const int64_t off = sg[0];
    const int Co = (int)sg[1], RS = (int)sg[2], Ci = (int)sg[3], flags = (int)sg[4];
    const int t = (int)((int64_t)blockIdx.x - sg[5]);
    const int tiles_ci = Ci >> 5;
    const int co0 = (t / tiles_ci) * 32, ci0 = (t % tiles_ci) * 32;
    const int row = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
    __shared__ unsigned int tile[32][33];
    const int co = co0 + row, ci = ci0 + c4;
    const int64_t e0 = off + (int64_t)co * RS * Ci + ci;
    Q nxt = load4(e0);
    for (int rs = 0; rs < RS; ++rs) {
        const Q cur = nxt;
        if (rs + 1 < RS) nxt = load4(e0 + (int64_t)(rs + 1) * Ci);          // the next tap's rows are in flight while this one is split
        const float4 w4 = update4(cur, e0 + (int64_t)rs * Ci);
        const float we[4] = {w4.x, w4.y, w4.z, w4.w};
        unsigned short h[4], l[4];
        if (flags & 1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) split_weight(we[k], true, h[k], l[k]);
            const size_t o = off + plane_index(co, rs * Ci + ci, RS * Ci);
            *reinterpret_cast<uint2 *>(hi_f + o) = make_uint2(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16));
            *reinterpret_cast<uint2 *>(lo_f + o) = make_uint2(l[0] | ((unsigned)l[1] << 16), l[2] | ((unsigned)l[3] << 16));
        }
        if (flags & 2) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                split_weight(we[k], false, h[k], l[k]);
                tile[row][c4 + k] = (unsigned int)h[k] | ((unsigned int)l[k] << 16);
            }
            __syncthreads();
            unsigned int pk[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) pk[k] = tile[c4 + k][row];          // (ci = ci0 + row, co = co0 + c4 + k)
            const size_t o = off + plane_index(ci0 + row, rs * Co + co0 + c4, RS * Co);
            *reinterpret_cast<uint2 *>(hi_d + o) = make_uint2((pk[0] & 0xffffu) | (pk[1] << 16), (pk[2] & 0xffffu) | (pk[3] << 16));
            *reinterpret_cast<uint2 *>(lo_d + o) = make_uint2((pk[0] >> 16) | (pk[1] & 0xffff0000u), (pk[2] >> 16) | (pk[3] & 0xffff0000u));
            __syncthreads();
        }
    }
}

}  // namespace

extern "C" int hoig_pack_conv_weight_bf16(const float *w, int Co, int RS, int Ci, int for_dgrad, uint16_t *hi,
                                          uint16_t *lo, hoig_stream_t stream) {
    if (!w || !hi || Co <= 0 || RS <= 0 || Ci <= 0) return HOIG_EINVAL;
    if ((Co & 31) || (Ci & 31)) return HOIG_EUNSUPPORTED;      // the blocked plane layout needs whole 32x32 blocks
    const int64_t n = (int64_t)Co * RS * Ci;
    return hoig_launch<pack_weight_kernel>(hoig_stream_grid(n, 256), 256, 0, (hipStream_t)stream, w, Co, RS, Ci, for_dgrad ? 1 : 0, hi, lo);
}

extern "C" int hoig_pack_conv_weights_bf16_all(const float *flat, const int64_t *segs, int nseg, int64_t ntiles,
                                               uint16_t *hi_f, uint16_t *lo_f, uint16_t *hi_d, uint16_t *lo_d,
                                               hoig_stream_t stream) {
    if (!flat || !segs || nseg <= 0 || ntiles <= 0 || !hi_f || !lo_f || !hi_d || !lo_d) return HOIG_EINVAL;
    return hoig_launch<pack_all_kernel>((unsigned)ntiles, 256, 0, (hipStream_t)stream, flat, segs, nseg, hi_f, lo_f, hi_d, lo_d);
}

extern "C" int hoig_adam_pack_step(float *flat, const float *grad, float *exp_avg, float *exp_avg_sq, const float *derived,
                                   float grad_scale, const int64_t *segs, int nseg, int64_t ntiles, const int64_t *plain,
                                   int64_t nplain, uint16_t *hi_f, uint16_t *lo_f, uint16_t *hi_d, uint16_t *lo_d,
                                   hoig_stream_t stream) {
    if (!flat || !grad || !exp_avg || !exp_avg_sq || !derived || !segs || nseg <= 0 || ntiles <= 0 || nplain < 0 || (nplain && !plain) ||
        !hi_f || !lo_f || !hi_d || !lo_d)
        return HOIG_EINVAL;
    const float *no_guard = nullptr;
    return hoig_launch<adam_pack_kernel<false>>((unsigned)(ntiles + nplain), 256, 0, (hipStream_t)stream, flat, grad, exp_avg, exp_avg_sq,
                                                derived, grad_scale, segs, nseg, ntiles, plain, hi_f, lo_f, hi_d, lo_d, no_guard);
}

extern "C" int hoig_adam_pack_step_guarded(float *flat, const float *grad, float *exp_avg, float *exp_avg_sq, const float *derived,
                                           float grad_scale, const int64_t *segs, int nseg, int64_t ntiles, const int64_t *plain,
                                           int64_t nplain, uint16_t *hi_f, uint16_t *lo_f, uint16_t *hi_d, uint16_t *lo_d,
                                           const float *guard, hoig_stream_t stream) {
    if (!flat || !grad || !exp_avg || !exp_avg_sq || !derived || !segs || nseg <= 0 || ntiles <= 0 || nplain < 0 || (nplain && !plain) ||
        !hi_f || !lo_f || !hi_d || !lo_d || !guard)
        return HOIG_EINVAL;
    return hoig_launch<adam_pack_kernel<true>>((unsigned)(ntiles + nplain), 256, 0, (hipStream_t)stream, flat, grad, exp_avg, exp_avg_sq,
                                               derived, grad_scale, segs, nseg, ntiles, plain, hi_f, lo_f, hi_d, lo_d, guard);
}
