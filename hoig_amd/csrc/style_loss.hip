// The opt-in style (Gram-matrix) term of G on the device (docs/style_loss.md; the checks, the workspace, the per-entry code of the finish
// and the last sums: style_loss.h).  hoig_style_gram is three launches on the caller's stream:
//   st_gram_kernel     one workgroup per (image of the 2N, tile pair tj >= ti, pixel chunk): four waves, each a 32 x 32 block of the
//                      ST_T x ST_T tile on v_mfma_f32_32x32x2_f32 from a zero accumulator over the chunk's pixels in ascending order;
//                      both operands are coalesced reads of the same rows of F.  The raw partial tile goes to the workspace;
//   st_finish_kernel   one workgroup per (image of the N, tile pair): chunk partials in index order in double, / (C P), d = Gx - Gy, S
//                      (and its mirror image), |d| through the workgroup's fixed halving tree, one sum per workgroup;
//   st_last_kernel     one wave: the workgroups' sums in a fixed order, L, the two slots.
// hoig_style_dfeat is one launch: dFx = Fx S in tiles of ST_ROWS pixels x ST_T columns, k over the channels in ascending order on the
// same MFMA; the tile of Fx goes through LDS (its k index is the contiguous one), S is read as it lies.
// Stream order is the only synchronisation between the launches.  Nothing here allocates, synchronises, spins, waits for another
// workgroup or uses an atomic.  Built with -ffp-contract=off.
#include "common.h"
#include "style_loss.h"

namespace {

constexpr int ST_U = 8;          // MFMA steps (of two pixels) whose loads are issued together

// grid (chunks, pairs, 2N)
__global__ __launch_bounds__(ST_NT) void st_gram_kernel(st_args a, float *__restrict__ partials) {
    const int chunk = blockIdx.x, pair = blockIdx.y, img = blockIdx.z;
    int ti, tj;
    st_pair(a.tiles, pair, &ti, &tj);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, li = l & 31, lk = l >> 5;
    const int bi = (w >> 1) * 32, bj = (w & 1) * 32;          // this wave's block of the tile
    const int ci = ti * ST_T + bi, cj = tj * ST_T + bj;
    if (ci >= a.C || cj >= a.C) return;                       // (wave-uniform; the kernel has no barrier; the finish never reads it)
    const float *F = st_image(a, img);
    const bool va = ci + li < a.C, vb = cj + li < a.C;        // C is a multiple of 16, the block is 32 wide
    const int p0 = chunk * ST_K, p1 = p0 + ST_K < a.P ? p0 + ST_K : a.P;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // lane l holds A[i = l & 31][k = l >> 5] = F[p + k][ci + i] and B[k][j = l & 31] = F[p + k][cj + j]
    for (int p = p0; p < p1; p += 2 * ST_U) {
        float av[ST_U], bv[ST_U];
#pragma unroll
        for (int u = 0; u < ST_U; ++u) {
            const int pp = p + 2 * u + lk;
            const bool ok = pp < p1;
            const int64_t row = (int64_t)(ok ? pp : p0) * a.C;
            av[u] = ok && va ? F[row + ci + li] : 0.f;
            bv[u] = ok && vb ? F[row + cj + li] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < ST_U; ++u)
            if (p + 2 * u < p1) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
    }
    float *out = partials + (((int64_t)img * a.pairs + pair) * a.chunks + chunk) * (ST_T * ST_T);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = bi + (r & 3) + 8 * (r >> 2) + 4 * lk;
        out[row * ST_T + bj + li] = acc[r];
    }
}

// the workgroup's halving tree over the threads' sums: steps 128 and 64 through LDS, 32 .. 1 by shuffles; lane 0 of wave 0 holds it
__device__ double st_wg_tree(double v, double *sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    if (t >= 64) return 0.0;
    double x = (sh[t] + sh[t + 128]) + (sh[t + 64] + sh[t + 192]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = x + __shfl_xor(x, o, 64);
    return x;
}

// grid (pairs, N)
__global__ __launch_bounds__(ST_NT) void st_finish_kernel(st_args a, const float *partials, double *__restrict__ sums) {
    __shared__ double sh[ST_NT];
    const int pair = blockIdx.x, n = blockIdx.y;
    int ti, tj;
    st_pair(a.tiles, pair, &ti, &tj);
    const double x = st_wg_tree(st_finish_lane(a, partials, n, pair, ti, tj, threadIdx.x), sh);
    if (threadIdx.x == 0) sums[n * a.pairs + pair] = st_tile_sum(x, ti, tj);
}

__global__ __launch_bounds__(64) void st_last_kernel(st_args a, const double *__restrict__ sums) {
    double x = st_last_lane(a, sums, threadIdx.x);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = x + __shfl_xor(x, o, 64);
    if (threadIdx.x == 0) st_last(a, x);
}

// grid (ceil(P / ST_ROWS), tiles, N)
__global__ __launch_bounds__(ST_NT) void st_dfeat_kernel(const float *__restrict__ fx, const float *__restrict__ S, int P, int C,
                                                         float *__restrict__ dfx) {
    __shared__ float sh[ST_ROWS][33];
    const int p0 = blockIdx.x * ST_ROWS, n = blockIdx.z;
    const int t = threadIdx.x, w = t >> 6, l = t & 63, li = l & 31, lk = l >> 5;
    const int bp = (w >> 1) * 32, cj = blockIdx.y * ST_T + (w & 1) * 32;
    const float *F = fx + (int64_t)n * P * C, *Sn = S + (int64_t)n * C * C;
    const bool vb = cj + li < C;
    const int lrow = t >> 2, lseg = (t & 3) * 8;             // this thread's eight floats of the Fx tile
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < C; k0 += 32) {
        const int kc = C - k0 < 32 ? C - k0 : 32;             // 16 or 32
        float4 u0 = make_float4(0.f, 0.f, 0.f, 0.f), u1 = u0;
        if (p0 + lrow < P && lseg < kc) {
            const float4 *src = reinterpret_cast<const float4 *>(F + (int64_t)(p0 + lrow) * C + k0 + lseg);
            u0 = src[0], u1 = src[1];
        }
        float *d = &sh[lrow][lseg];
        d[0] = u0.x, d[1] = u0.y, d[2] = u0.z, d[3] = u0.w, d[4] = u1.x, d[5] = u1.y, d[6] = u1.z, d[7] = u1.w;
        // lane l holds B[k = l >> 5][j = l & 31] = S[k0 + 2 s + k][cj + j]
        float bv[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) bv[s] = vb && 2 * s < kc ? Sn[(int64_t)(k0 + 2 * s + lk) * C + cj + li] : 0.f;
        __syncthreads();
        // ... and A[i = l & 31][k] = Fx[p0 + bp + i][k0 + 2 s + k]
#pragma unroll
        for (int s = 0; s < 16; ++s)
            if (2 * s < kc) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sh[bp + li][2 * s + lk], bv[s], acc, 0, 0, 0);
        __syncthreads();
    }
    if (!vb) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int p = p0 + bp + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (p < P) dfx[((int64_t)n * P + p) * C + cj + li] = acc[r];
    }
}

}  // namespace

extern "C" int64_t hoig_style_workspace_bytes(int N, int P, int C) { return st_workspace_bytes(N, P, C); }

extern "C" int hoig_style_gram(const float *fx, const float *fy, int N, int P, int C, double scale, float *S, float *term, float *report,
                               double *gram, void *workspace, int64_t workspace_bytes, hoig_stream_t stream) {
    st_args a;
    int rc = st_pack(fx, fy, N, P, C, scale, S, term, report, gram, &a);
    if (rc != HOIG_OK) return rc;
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < st_workspace_bytes(N, P, C)) return HOIG_EINVAL;
    float *partials = static_cast<float *>(workspace);
    double *sums = reinterpret_cast<double *>(static_cast<char *>(workspace) + st_off_sums(N, P, C));
    hipStream_t st = (hipStream_t)stream;
    rc = hoig_launch<st_gram_kernel>(dim3((unsigned)a.chunks, (unsigned)a.pairs, (unsigned)(2 * N)), dim3(ST_NT), 0, st, a, partials);
    if (rc != HOIG_OK) return rc;
    rc = hoig_launch<st_finish_kernel>(dim3((unsigned)a.pairs, (unsigned)N), dim3(ST_NT), 0, st, a, (const float *)partials, sums);
    if (rc != HOIG_OK) return rc;
    return hoig_launch<st_last_kernel>(dim3(1), dim3(64), 0, st, a, (const double *)sums);
}

extern "C" int hoig_style_dfeat(const float *fx, const float *S, int N, int P, int C, float *dfx, hoig_stream_t stream) {
    const int rc = st_check_dfeat(fx, S, N, P, C, dfx);
    if (rc != HOIG_OK) return rc;
    return hoig_launch<st_dfeat_kernel>(dim3((unsigned)((P + ST_ROWS - 1) / ST_ROWS), (unsigned)st_tiles(C), (unsigned)N), dim3(ST_NT), 0,
                                        (hipStream_t)stream, fx, S, P, C, dfx);
}
