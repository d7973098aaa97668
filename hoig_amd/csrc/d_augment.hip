// Differentiable augmentation in front of the discriminator, on the device (docs/d_augment.md; the shared code: d_augment.h).
// hoig_daug_tick and the tail of hoig_daug_adapt are one thread; hoig_daug_draw is one thread per sample; the forward and the backward
// are grid-stride bodies that make four consecutive output floats per thread (one 16-byte store where the pointer allows, scalar stores
// for the rest), each behind a per-sample reduction whose partials are added in an order the sizes fix: no atomics, no grid-wide wait.
// Nothing here synchronises or allocates, so the launches sit in a captured step.  Built with -ffp-contract=off.
#include "common.h"
#include "d_augment.h"

namespace {

constexpr int NT = DAUG_NT;

__global__ void daug_tick_kernel(uint64_t *__restrict__ state) {
    if (threadIdx.x == 0 && blockIdx.x == 0) state[DAUG_STEP] += 1;
}

__global__ __launch_bounds__(NT) void daug_draw_kernel(const uint64_t *__restrict__ state, int site, int B, int H, int W,
                                                       uint32_t *__restrict__ params) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= B) return;
    uint32_t rec[8];
    daug_draw_one(state, site, i, H, W, rec);
    uint4 *dst = reinterpret_cast<uint4 *>(params + 8 * (int64_t)i);
    dst[0] = make_uint4(rec[0], rec[1], rec[2], rec[3]);
    dst[1] = make_uint4(rec[4], rec[5], rec[6], rec[7]);
}

// one workgroup: integer counts, a halving tree in LDS, then thread 0 runs the controller
__global__ __launch_bounds__(NT) void daug_adapt_kernel(uint64_t *__restrict__ state, const float *__restrict__ d_real, int64_t n) {
    __shared__ int pos_s[NT], neg_s[NT];
    const int t = threadIdx.x;
    int pos = 0, neg = 0;
    for (int64_t i = t; i < n; i += NT) {
        const float v = d_real[i];
        pos += v > 0.f, neg += v < 0.f;
    }
    pos_s[t] = pos, neg_s[t] = neg;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (t < s) pos_s[t] += pos_s[t + s], neg_s[t] += neg_s[t + s];
        __syncthreads();
    }
    if (t == 0) daug_adapt(state, pos_s[0], neg_s[0], n);
}

__device__ __forceinline__ float block_tree(float acc, float *lds) {
    const int t = threadIdx.x;
    lds[t] = acc;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (t < s) lds[t] = lds[t] + lds[t + s];
        __syncthreads();
    }
    return lds[0];
}

// grid (DAUG_MAX_PARTS, B): part blockIdx.x of sample blockIdx.y's image sum -> ws[sample][part]; a sample without the colour flag is
// left alone (its partials are never read)
__global__ __launch_bounds__(NT) void daug_mean_kernel(const float *__restrict__ img, const uint32_t *__restrict__ params, int H, int W,
                                                       float *__restrict__ ws) {
    __shared__ float lds[NT];
    const int i = blockIdx.y, part = blockIdx.x;
    if (!(params[8 * (int64_t)i + 7] & HOIG_DAUG_COLOR)) return;
    const int64_t n = 3 * (int64_t)H * W;
    if (part >= daug_parts((n + 3) / 4)) return;
    const float sum = block_tree(daug_mean_thread(img + i * n, n, part, threadIdx.x), lds);
    if (threadIdx.x == 0) ws[(int64_t)i * DAUG_MAX_PARTS + part] = sum;
}

__global__ __launch_bounds__(NT) void daug_gsum_kernel(const float *__restrict__ g, const uint32_t *__restrict__ params, int H, int W, int k,
                                                       float *__restrict__ ws) {
    __shared__ float lds[NT];
    const int i = blockIdx.y, part = blockIdx.x;
    const DaugRec r = daug_rec(params, i);
    if (!(r.flags & HOIG_DAUG_COLOR)) return;
    const int64_t npix = (int64_t)H * W;
    if (part >= daug_parts(npix)) return;
    const float sum = block_tree(daug_gsum_thread(g + i * npix * (3 + k), r, H, W, k, part, threadIdx.x), lds);
    if (threadIdx.x == 0) ws[(int64_t)i * DAUG_MAX_PARTS + part] = sum;
}

// Four consecutive floats of the [B][per] output per thread.  FWD: per = HW(3 + k), the augmented concatenation; else per = 3HW, dimg.
template <bool FWD>
__global__ __launch_bounds__(NT) void daug_apply_kernel(const float *__restrict__ a, const float *__restrict__ cond,
                                                        const uint32_t *__restrict__ params, const float *__restrict__ ws,
                                                        float *__restrict__ out, int B, int H, int W, int k) {
    const int64_t per = (int64_t)H * W * (FWD ? 3 + k : 3), total = (int64_t)B * per;
    const int64_t per_in = (int64_t)H * W * (FWD ? 3 : 3 + k);
    const bool vec = !((uintptr_t)out & 15);
    for (int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x; q * 4 < total; q += (int64_t)gridDim.x * NT) {
        float v[4];
        const int64_t e0 = q * 4;
        // the first float's sample, pixel and channel by division; the other three by stepping (they may straddle two samples)
        const int C = FWD ? 3 + k : 3;
        int i = (int)(e0 / per);
        const int e = (int)(e0 - (int64_t)i * per), pix = e / C;
        int c = e - pix * C, y = pix / W, x = pix - y * W;
        int have = -1;
        DaugRec r;
        float m = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (e0 + j >= total) {
                v[j] = 0.f;
                continue;
            }
            if (have != i) {
                r = daug_rec(params, i);
                if (r.flags & HOIG_DAUG_COLOR)
                    m = FWD ? daug_mu(ws + (int64_t)i * DAUG_MAX_PARTS, H, W, r.b) : daug_cmu(ws + (int64_t)i * DAUG_MAX_PARTS, H, W, r.k);
                have = i;
            }
            if (FWD)
                v[j] = daug_fwd_at(a + i * per_in, cond + (int64_t)i * H * W * k, r, m, H, W, k, y, x, c);
            else
                v[j] = daug_bwd_at(a + i * per_in, r, m, H, W, k, y, x, c);
            if (++c == C) {
                c = 0;
                if (++x == W) {
                    x = 0;
                    if (++y == H) y = 0, ++i;
                }
            }
        }
        if (vec && e0 + 4 <= total) {
            *reinterpret_cast<float4 *>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int j = 0; j < 4 && e0 + j < total; ++j) out[e0 + j] = v[j];
        }
    }
}

}  // namespace

extern "C" int hoig_daug_ws_floats(int B) { return B > 0 && (int64_t)B * DAUG_MAX_PARTS < ((int64_t)1 << 31) ? B * DAUG_MAX_PARTS : HOIG_EINVAL; }

extern "C" int hoig_daug_tick(uint64_t *state, hoig_stream_t stream) {
    if (!daug_state_ok(state)) return HOIG_EINVAL;
    daug_tick_kernel<<<1, 64, 0, (hipStream_t)stream>>>(state);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}

extern "C" int hoig_daug_draw(const uint64_t *state, int site, int B, int H, int W, uint32_t *params, hoig_stream_t stream) {
    if (!daug_draw_ok(state, site, B, H, W, params)) return HOIG_EINVAL;
    daug_draw_kernel<<<(B + NT - 1) / NT, NT, 0, (hipStream_t)stream>>>(state, site, B, H, W, params);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}

extern "C" int hoig_daug_adapt(uint64_t *state, const float *d_real, int64_t n, hoig_stream_t stream) {
    if (!daug_state_ok(state) || !d_real || ((uintptr_t)d_real & 3) || n <= 0) return HOIG_EINVAL;
    daug_adapt_kernel<<<1, NT, 0, (hipStream_t)stream>>>(state, d_real, n);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}

extern "C" int hoig_daug_fwd(const float *img, const float *cond, const uint32_t *params, float *out, int B, int H, int W, int k, float *ws,
                             hoig_stream_t stream) {
    if (!daug_fwd_ok(img, cond, params, out, B, H, W, k, ws)) return HOIG_EINVAL;
    if (B > 65535) return HOIG_EUNSUPPORTED;
    const int parts = daug_parts((3 * (int64_t)H * W + 3) / 4);
    daug_mean_kernel<<<dim3(parts, B), NT, 0, (hipStream_t)stream>>>(img, params, H, W, ws);
    HOIG_LAUNCH_CHECK();
    const int64_t total = (int64_t)B * H * W * (3 + k);
    daug_apply_kernel<true><<<hoig_stream_grid(total / 4 + 1, NT), NT, 0, (hipStream_t)stream>>>(img, cond, params, ws, out, B, H, W, k);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}

extern "C" int hoig_daug_bwd(const float *g, const uint32_t *params, float *dimg, int B, int H, int W, int k, float *ws,
                             hoig_stream_t stream) {
    if (!daug_bwd_ok(g, params, dimg, B, H, W, k, ws)) return HOIG_EINVAL;
    if (B > 65535) return HOIG_EUNSUPPORTED;
    daug_gsum_kernel<<<dim3(daug_parts((int64_t)H * W), B), NT, 0, (hipStream_t)stream>>>(g, params, H, W, k, ws);
    HOIG_LAUNCH_CHECK();
    const int64_t total = (int64_t)B * H * W * 3;
    daug_apply_kernel<false><<<hoig_stream_grid(total / 4 + 1, NT), NT, 0, (hipStream_t)stream>>>(g, nullptr, params, ws, dimg, B, H, W, k);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}
