// EMA of a network's weights on the device (docs/ema.md; the shared per-element code and the schedule: ema.h).  hoig_ema_tick is one
// thread, hoig_ema_update and hoig_swap_f32 are grid-stride float4 bodies with a scalar tail, sized as adam_dev_kernel is.  Nothing
// here synchronises or allocates, so the launches sit in a captured step like the optimiser's.  Built with -ffp-contract=off.
#include "common.h"
#include "ema.h"

namespace {

constexpr int NT = 256;

// `guard` = {scale, skip} as hoig_guard_decide left it (nullptr: none): a skipped step leaves the count and `derived` as they are, as
// adam_tick_kernel<true> does
__global__ void ema_tick_kernel(double *__restrict__ state, float *__restrict__ derived, const float *__restrict__ guard) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (guard && guard[1] != 0.f) return;
    ema_tick(state, derived);
}

// a skipped step returns before the first load; `p` is only ever read
__global__ __launch_bounds__(NT) void ema_update_kernel(float *__restrict__ e, const float *__restrict__ p, int64_t n,
                                                        const float *__restrict__ derived, const float *__restrict__ guard) {
    if (guard && guard[1] != 0.f) return;
    const float w = derived[0];
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (int64_t)gridDim.x * NT) {
        float4 ee = reinterpret_cast<float4 *>(e)[i];
        const float4 pp = reinterpret_cast<const float4 *>(p)[i];
        ee.x = ema_lerp(ee.x, pp.x, w);
        ee.y = ema_lerp(ee.y, pp.y, w);
        ee.z = ema_lerp(ee.z, pp.z, w);
        ee.w = ema_lerp(ee.w, pp.w, w);
        reinterpret_cast<float4 *>(e)[i] = ee;
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) e[i] = ema_lerp(e[i], p[i], w);
}

__global__ __launch_bounds__(NT) void swap_kernel(float *__restrict__ a, float *__restrict__ b, int64_t n) {
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (int64_t)gridDim.x * NT) {
        const float4 aa = reinterpret_cast<float4 *>(a)[i], bb = reinterpret_cast<float4 *>(b)[i];
        reinterpret_cast<float4 *>(a)[i] = bb;
        reinterpret_cast<float4 *>(b)[i] = aa;
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const float av = a[i], bv = b[i];
        a[i] = bv;
        b[i] = av;
    }
}

}  // namespace

extern "C" int hoig_ema_tick(double *state, float *derived, const float *guard, hoig_stream_t stream) {
    if (!state || !derived) return HOIG_EINVAL;
    ema_tick_kernel<<<1, 64, 0, (hipStream_t)stream>>>(state, derived, guard);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}

extern "C" int hoig_ema_update(float *ema, const float *param, int64_t n, const float *derived, const float *guard, hoig_stream_t stream) {
    if (!ema_update_ok(ema, param, n, derived)) return HOIG_EINVAL;
    ema_update_kernel<<<hoig_stream_grid(n / 4 + 1, NT), NT, 0, (hipStream_t)stream>>>(ema, param, n, derived, guard);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}

extern "C" int hoig_swap_f32(float *a, float *b, int64_t n, hoig_stream_t stream) {
    if (!a || !b || n <= 0 || (((uintptr_t)a | (uintptr_t)b) & 15) || ema_overlap(a, b, n)) return HOIG_EINVAL;
    swap_kernel<<<hoig_stream_grid(n / 4 + 1, NT), NT, 0, (hipStream_t)stream>>>(a, b, n);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}
