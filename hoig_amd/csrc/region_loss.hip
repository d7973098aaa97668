// The opt-in region reconstruction term of G on the device (docs/region_loss.md; the per-lane code, the scales, the finishing sums and
// the layout of the workspace: region_loss.h).  A head is one memset node, which zeroes the counts, and three launches on the caller's
// stream:
//   rl_count_kernel    one pass over the labels: integer counts per (image, region), added with integer atomics; the workgroup that
//                      arrives last writes V_r, the fp32 gradient scale of every row, counts_out and the status word;
//   rl_value_kernel    one pass over pred, target and labels in whole 16-byte vectors of the flat float stream: |d| into running
//                      doubles per region and for the frame, dpred from the sign and the row's scale, the workgroup's fixed halving
//                      tree, one partial of R + 2 doubles per workgroup;
//   rl_finish_kernel   one wave: lane rho adds row rho's partials in workgroup order; then one thread forms L_r, L_all and the term.
// Stream order is the only synchronisation between the launches.  Nothing here allocates, synchronises, spins, waits for another
// workgroup or uses a floating-point atomic.  Built with -ffp-contract=off.
#include "common.h"
#include "region_loss.h"

namespace {

// Every workgroup has added its counts; the last one to arrive returns true (on thread 0 only) and may then read all of them.
// Agent-scope release before the ticket, acquire after it (metrics.hip's last_arrival): no workgroup waits for another.
__device__ bool rl_last_arrival(unsigned *ticket, unsigned expected) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x != 0) return false;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t != expected - 1) return false;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return true;
}

// grid (ctiles, N): workgroup (c, i) counts the labels [c RL_CTILE, (c + 1) RL_CTILE) of image i, 16 consecutive bytes per thread
template <int RT>
__global__ __launch_bounds__(RL_NT) void rl_count_kernel(rl_args a, int32_t *head, float *scales, int32_t *V) {
    const int i = blockIdx.y, t = threadIdx.x;
    const uint8_t *lb = a.labels + (int64_t)i * a.HW;
    const int p0 = (int)blockIdx.x * RL_CTILE + 16 * t;
    int c[RT + 1], bad = 0;
#pragma unroll
    for (int r = 0; r <= RT; ++r) c[r] = 0;
    if (p0 < a.HW) {
        const int nv = a.HW - p0 < 16 ? a.HW - p0 : 16;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (nv == 16 && (((uintptr_t)(lb + p0)) & 15) == 0) {
            const uint4 x = *reinterpret_cast<const uint4 *>(lb + p0);
            w[0] = x.x, w[1] = x.y, w[2] = x.z, w[3] = x.w;
        } else {
            for (int j = 0; j < nv; ++j) w[j >> 2] |= (uint32_t)lb[p0 + j] << (8 * (j & 3));
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int l = (int)((w[j >> 2] >> (8 * (j & 3))) & 255u);
            if (j < nv) {
#pragma unroll
                for (int r = 0; r <= RT; ++r) c[r] += (l == r && l <= a.R) ? 1 : 0;
                bad = l > a.R && l > bad ? l : bad;
            }
        }
    }
    // the wave's sums by shuffles, then one integer atomic per wave and region that has something to add
    int32_t *counts = head;
    const int R1 = a.R + 1;
#pragma unroll
    for (int r = 0; r <= RT; ++r) {
        int v = c[r];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((t & 63) == 0 && r <= a.R && v != 0) atomicAdd(counts + i * R1 + r, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int b = __shfl_xor(bad, o, 64);
        bad = b > bad ? b : bad;
    }
    const int64_t rows = (int64_t)a.N * R1;
    if ((t & 63) == 0 && bad != 0) atomicMax(head + rows + 1, bad);
    if (!rl_last_arrival(reinterpret_cast<unsigned *>(head + rows), gridDim.x * gridDim.y)) return;
    auto count = [&](int k) { return __hip_atomic_load(counts + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    rl_scales(a, count, __hip_atomic_load(head + rows + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), scales, V);
}

// grid (tiles, N): workgroup (w, i) takes the floats [w RL_TILE, (w + 1) RL_TILE) of image i
template <int RT>
__global__ __launch_bounds__(RL_NT) void rl_value_kernel(rl_args a, const float *__restrict__ scales, double *__restrict__ partials) {
    __shared__ double sh[RL_NT][RT + 2];
    const int i = blockIdx.y, w = blockIdx.x, t = threadIdx.x;
    float sc[RT + 1];
    double acc[RT + 2];
#pragma unroll
    for (int r = 0; r <= RT; ++r) sc[r] = r <= a.R ? scales[i * (a.R + 1) + r] : 0.f;
#pragma unroll
    for (int j = 0; j < RT + 2; ++j) acc[j] = 0.0;
    const int64_t base = (int64_t)i * a.E;
    const bool vec = ((((uintptr_t)(a.pred + base)) | ((uintptr_t)(a.target + base)) | ((uintptr_t)(a.dpred ? a.dpred + base : nullptr))) & 15) == 0;
    rl_lane<RT>(a, i, w, t, vec, sc, acc);
#pragma unroll
    for (int j = 0; j < RT + 2; ++j) sh[t][j] = acc[j];
    __syncthreads();
    if (t >= 64) return;                                    // (wave 0 goes on alone: no barrier below)
    // the halving tree's steps 128 and 64 ...
#pragma unroll
    for (int j = 0; j < RT + 2; ++j) acc[j] = (sh[t][j] + sh[t + 128][j]) + (sh[t + 64][j] + sh[t + 192][j]);
    // ... and its steps 32 .. 1: lane t < o holds acc[t] + acc[t + o], as the tree does (the other lanes' sums are not used)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int j = 0; j < RT + 2; ++j) acc[j] = acc[j] + __shfl_xor(acc[j], o, 64);
    }
    if (t == 0) {
        double *out = partials + ((int64_t)i * a.tiles + w) * (a.R + 2);
#pragma unroll
        for (int j = 0; j <= RT; ++j)
            if (j <= a.R) out[j] = acc[j];
        out[a.R + 1] = acc[RT + 1];
    }
}

__global__ __launch_bounds__(64) void rl_finish_kernel(rl_args a, const int32_t *__restrict__ counts, const int32_t *__restrict__ V,
                                                       const double *__restrict__ partials, double *rows) {
    const int n = a.N * (a.R + 2);
    for (int rho = threadIdx.x; rho < n; rho += 64) rows[rho] = rl_row(a, partials, rho);
    __syncthreads();                                        // (the rows are this workgroup's own stores)
    if (threadIdx.x == 0) rl_finish(a, counts, V, rows);
}

template <int RT>
int launch(const rl_args &a, char *ws, const rl_layout &l, hipStream_t st) {
    int32_t *head = reinterpret_cast<int32_t *>(ws);
    float *scales = reinterpret_cast<float *>(ws + l.off_scales);
    int32_t *V = reinterpret_cast<int32_t *>(ws + l.off_v);
    double *rows = reinterpret_cast<double *>(ws + l.off_rows), *partials = reinterpret_cast<double *>(ws + l.off_partials);
    if (hipMemsetAsync(head, 0, (size_t)l.head_bytes, st) != hipSuccess) return HOIG_ELAUNCH;
    int rc = hoig_launch<rl_count_kernel<RT>>(dim3((unsigned)a.ctiles, (unsigned)a.N), dim3(RL_NT), 0, st, a, head, scales, V);
    if (rc != HOIG_OK) return rc;
    rc = hoig_launch<rl_value_kernel<RT>>(dim3((unsigned)a.tiles, (unsigned)a.N), dim3(RL_NT), 0, st, a, (const float *)scales, partials);
    if (rc != HOIG_OK) return rc;
    return hoig_launch<rl_finish_kernel>(dim3(1), dim3(64), 0, st, a, (const int32_t *)head, (const int32_t *)V, (const double *)partials,
                                         rows);
}

}  // namespace

extern "C" int64_t hoig_region_loss_workspace_bytes(int N, int H, int W, int C, int R) { return rl_workspace_bytes(N, H, W, C, R); }

extern "C" int hoig_region_loss(const float *pred, const float *target, const uint8_t *labels, int N, int H, int W, int C, int R,
                                const double *lambda, double lambda_all, int min_pixels, float *dpred, float *term, float *terms_r,
                                float *term_all, int32_t *counts_out, int32_t *status, void *workspace, int64_t workspace_bytes,
                                hoig_stream_t stream) {
    rl_args a;
    if (!rl_pack(pred, target, labels, N, H, W, C, R, lambda, lambda_all, min_pixels, dpred, term, terms_r, term_all, counts_out, status, &a))
        return HOIG_EINVAL;
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < rl_workspace_bytes(N, H, W, C, R)) return HOIG_EINVAL;
    const rl_layout l = rl_make_layout(N, R, a.tiles);
    char *ws = static_cast<char *>(workspace);
    return R <= 2 ? launch<2>(a, ws, l, (hipStream_t)stream) : launch<RL_MAXR>(a, ws, l, (hipStream_t)stream);
}
