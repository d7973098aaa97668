// Shared device helpers for the gfx950 kernels (wave64, 256 CUs in 8 XCDs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "hoig_kernels.h"
#include "conv_route.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));

#define HOIG_LAUNCH_CHECK()                                   \
    do {                                                      \
        hipError_t e__ = hipGetLastError();                   \
        if (e__ != hipSuccess) return HOIG_ELAUNCH;           \
    } while (0)

// hipFuncSetAttribute applies to the CURRENT device: a kernel's "attribute already set" flag remembers WHICH device ordinals have it
// (a process-wide bool left every second GPU of a multi-device process without its > 64 KB of dynamic LDS).
struct hoig_once {
    std::atomic<unsigned long long> mask{0};
    static int dev() {
        int d = 0;
        (void)hipGetDevice(&d);
        return d & 63;
    }
    bool done() const { return (mask.load(std::memory_order_acquire) >> dev()) & 1ull; }
    void set() { mask.fetch_or(1ull << dev(), std::memory_order_release); }
};

// One launch: Kernel<<<grid, block, lds, st>>>(args...) and its check.  A kernel that needs more than the default 64 KB of dynamic LDS
// names its opt-in LDS_OPT_IN (bytes, a compile-time constant); it is set on that kernel's first launch on each device, from one flag
// per instantiation -- per kernel -- so the kernel launched and the kernel opted in cannot differ.
template <auto Kernel, int LDS_OPT_IN = 0, class... A>
int hoig_launch(dim3 grid, dim3 block, size_t lds, hipStream_t st, const A &...args) {
    if constexpr (LDS_OPT_IN > 0) {
        static hoig_once once;
        if (!once.done()) {
            if (hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_OPT_IN) !=
                hipSuccess)
                return HOIG_ELAUNCH;
            once.set();
        }
    }
    Kernel<<<grid, block, lds, st>>>(args...);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}

static inline int64_t hoig_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Launchers that one .hip file defines and another calls (the dispatchers of conv_igemm.hip walk them in turn): each takes the layers it
// has a kernel for and returns HOIG_EUNSUPPORTED for the rest.  Declared here, where the defining file sees them too.
// conv_small.hip: direct fp32 kernels for <= 4 / 5 output channels, the 7x7 stems with <= 8 input channels, long dot products
int hoig_conv_small_fwd(const hoig_conv_desc *d, const float *x, const float *w, const float *bias, float *y, hipStream_t st);
int hoig_conv_small_fwd_acts(const hoig_conv_desc *d, const float *x, const float *w, const float *bias, float *y,
                             unsigned long long acts, hipStream_t st);
int hoig_conv_small_ci_fwd(const hoig_conv_desc *d, const float *x, const float *w, const float *bias, float *y, hipStream_t st);
int hoig_conv_small_dgrad(const hoig_conv_desc *d, const float *dy, const float *w, float *dx, hipStream_t st);
int hoig_conv_small_wgrad(const hoig_conv_desc *d, const float *x, const float *dy, float *dw, hipStream_t st);
int hoig_conv_dot_fwd(const hoig_conv_desc *d, const float *x, const float *w, const float *bias, float *y, hipStream_t st);
// conv_head16.hip: the 7x7 heads on MFMA
int hoig_conv_head7_m16(const hoig_conv_desc *d, const float *x, const float *w, const float *bias, float *y, unsigned long long acts,
                        hipStream_t st);
// conv_thin.hip: stride-1 'same' convolutions with <= 8 (3x3: 16) channels on one side, taps in place of the missing channels
int hoig_conv_thin_fwd(const hoig_conv_desc *d, const float *x, const float *w, const float *bias, float *y, hipStream_t st,
                       double *stats = nullptr);
int hoig_conv_thin_dgrad(const hoig_conv_desc *d, const float *dy, const float *w, float *dx, int accumulate, hipStream_t st);
int hoig_conv_thin_wgrad(const hoig_conv_desc *d, const float *x, const float *dy, float *dw, hipStream_t st);
bool hoig_conv_thin_wgrad_applies(const hoig_conv_desc *d);
int hoig_conv_thin_out(const hoig_conv_desc *d, const float *x, const float *w, const float *bias, float *y, unsigned long long acts,
                       int dgrad, hipStream_t st);
// wgrad_igemm_bf16.hip: the 16-bit weight gradients
int hoig_conv_bf16_wgrad(const hoig_conv_desc *d, const float *x, const float *dy, float *dw, float *dbias, hipStream_t st);
bool hoig_conv_bf16_wgrad_fuses_bias(const hoig_conv_desc *d);
// pointwise.hip: the block registered for `st` by hoig_stream_scratch_set (nullptr: none of that size)
namespace hoig_detail { void *stream_scratch(hipStream_t st, size_t bytes); }

// Grid for HBM-bound streaming kernels: cap at 256 CUs x 8 blocks and grid-stride the rest.
static inline int hoig_stream_grid(int64_t work_items, int block) {
    int64_t g = hoig_cdiv(work_items, block);
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return (int)g;
}

__device__ __forceinline__ float hoig_act(float v, int act, float slope) {
    switch (act) {
        case HOIG_ACT_RELU: return v > 0.f ? v : 0.f;
        case HOIG_ACT_LRELU: return v > 0.f ? v : v * slope;
        case HOIG_ACT_TANH: return tanhf(v);
        case HOIG_ACT_SIGMOID: return 1.f / (1.f + expf(-v));
        default: return v;
    }
}

// epilogue form: none / ReLU / LeakyReLU are one select + one fma (negative slope 1 / 0 / slope; "+ 0" turns ReLU's -0
// into +0), tanh / sigmoid take the (wave-uniform) slow branch
__device__ __forceinline__ float fast_act(float v, float nslope, bool special, int act, float slope) {
    if (special) return hoig_act(v, act, slope);
    return v > 0.f ? v : fmaf(v, nslope, 0.f);
}

// derivative of the activation expressed through its OUTPUT y
__device__ __forceinline__ float hoig_act_grad_from_y(float y, int act, float slope) {
    switch (act) {
        case HOIG_ACT_RELU: return y > 0.f ? 1.f : 0.f;
        case HOIG_ACT_LRELU: return y > 0.f ? 1.f : slope;
        case HOIG_ACT_TANH: return 1.f - y * y;
        case HOIG_ACT_SIGMOID: return y * (1.f - y);
        default: return 1.f;
    }
}

// The sums a convolution's epilogue leaves for the instance norm that reads its output (hoig_conv2d_fwd_packed_stats and its kin,
// consumed by hoig_inorm_stats_from_sums): accumulators [b][moment 0 / 1][N] of DOUBLES inside the norm workspace's pool of fp32
// accumulators (all-zero bits are zero in both formats, so the pool's contract -- zero on entry, zero on return -- covers them).
// Several hundred fp32 atomics per address left about 1e-6 of relative error in sum y at 65536 pixels; in fp64 what remains is the
// rounding of each workgroup's own fp32 partial.
__device__ __forceinline__ void hoig_stats_add(double *stats, int b, int N, int mom, int n, float v) {
    atomicAdd(stats + ((size_t)b * 2 + mom) * N + n, (double)v);
}

// XCD-aware remap of a 1-D block id: blocks b and b+8 share an XCD (round-robin dispatch), so give each
// XCD a contiguous chunk of the logical tile order; bijective for any grid size (guide §5, T1).
__device__ __forceinline__ int hoig_xcd_remap(int bid, int nblk) {
    const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7, idx = bid >> 3;
    const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

__device__ __forceinline__ float hoig_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// fp32 -> bf16 (round to nearest even) as raw bits; NaN handling not needed on this path's operands
__device__ __forceinline__ unsigned short hoig_f2bf(float f) {
    unsigned int u = __float_as_uint(f);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
__device__ __forceinline__ float hoig_bf2f(unsigned short h) { return __uint_as_float(((unsigned int)h) << 16); }
