// Streaming FID statistics and the Frechet distance on the device, in fp64 (docs/fid_device.md; the shared per-lane code and the
// workspace layouts: fid_stats.h).
//
// hoig_gemm_tn_f64: C (+)= A^T B on v_mfma_f64_16x16x4_f64.  A workgroup of four waves owns a 64 x 64 tile of C, a wave a 32 x 32
//   quarter of it as 2 x 2 MFMA tiles; operands come straight from global memory (a k-step's 16 consecutive columns of a row are one
//   128-byte line, and the operands of the shapes this serves stay in L2), out-of-range elements are zeros.  Lane maps: lane l holds
//   A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; result register r of lane l is C[row (l >> 4) + 4 r][col l & 15] -- the
//   fp64 map, not the fp32 one.  Every element of C has one owner and K is walked in order: no atomics, the bits do not depend on
//   scheduling.  Symmetric mode: only the tiles on and above the diagonal run, and each element is also stored at its mirror place.
// hoig_pchol_f64: one launch per step; a wave owns FID_ROWS_PER_WAVE rows, finds the pivot itself (every wave reads the same remaining
//   diagonal and finds the same one) and makes its rows' entries of the new column, one dot product each.
// hoig_sym_eigvals_f64: Householder tridiagonalisation, three launches per step (reflector; symmetric matrix-vector product, a row per
//   wave; rank-2 update), then bisection with one lane per eigenvalue.
// No launch waits for another workgroup; a finished or refused factorisation makes the remaining launches return at once.
// Built with -ffp-contract=off (fid_stats.h).
#include "common.h"
#include "fid_stats.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int NT = 256;                                  // four waves
constexpr int WAVES = NT / FID_WAVE;
constexpr int ROWS_PER_BLOCK = WAVES * FID_ROWS_PER_WAVE;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, FID_WAVE);
    return v;
}

__device__ __forceinline__ double wave_dot(const double *a, int64_t sa, const double *b, int64_t sb, int n, int lane) {
    return wave_sum(fid_lane_dot(a, sa, b, sb, n, lane));
}

// the largest of v[0 .. n) and its lowest index, in every lane
__device__ __forceinline__ void wave_argmax(const double *v, int n, int lane, double *best, int *at) {
    double bv = -HUGE_VAL;
    int bi = 0x7fffffff;
    for (int i = lane; i < n; i += FID_WAVE)
        if (fid_better(v[i], i, bv, bi)) bv = v[i], bi = i;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, FID_WAVE);
        const int oi = __shfl_xor(bi, o, FID_WAVE);
        if (fid_better(ov, oi, bv, bi)) bv = ov, bi = oi;
    }
    *best = bv, *at = bi;
}

// ---------------------------------------------------------------- C (+)= A^T B
template <int F32>
__global__ __launch_bounds__(NT) void gemm_tn_kernel(const void *__restrict__ A, int64_t lda, const void *__restrict__ B, int64_t ldb,
                                                     const double *__restrict__ pivot, double *C, int64_t ldc, int M, int N, int K,
                                                     int accumulate, int symmetric) {
    if (symmetric && blockIdx.x < blockIdx.y) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int wm = blockIdx.y * 64 + (wave >> 1) * 32, wn = blockIdx.x * 64 + (wave & 1) * 32;
    if (wm >= M || wn >= N || (symmetric && wn + 31 < wm)) return;             // (wave-uniform)
    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + q;
        double a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = wm + 16 * i + r, n = wn + 16 * i + r;
            a[i] = (k < K && m < M) ? fid_operand(A, (int64_t)k * lda + m, F32, pivot, m) : 0.0;
            b[i] = (k < K && n < N) ? fid_operand(B, (int64_t)k * ldb + n, F32, pivot, n) : 0.0;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = wm + 16 * i + q + 4 * reg, col = wn + 16 * j + r;
                if (row >= M || col >= N || (symmetric && col < row)) continue;
                double v = acc[i][j][reg];
                if (accumulate) v = C[(int64_t)row * ldc + col] + v;
                C[(int64_t)row * ldc + col] = v;
                if (symmetric && col != row) C[(int64_t)col * ldc + row] = v;
            }
}

// ---------------------------------------------------------------- pivoted Cholesky
__global__ __launch_bounds__(NT) void pchol_scan_kernel(const double *__restrict__ S, int64_t lds, int D, fid_pchol_head *head,
                                                        double *diag) {
    const int64_t total = (int64_t)D * D;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
        const int row = (int)(i / D), col = (int)(i % D);
        const double v = S[row * lds + col];
        bad |= !fid_finite(v);
        if (row == col) diag[row] = v;
    }
    if (bad) head->status = HOIG_EINVAL;            // (every lane that stores here stores the same value)
}

__global__ __launch_bounds__(FID_WAVE) void pchol_init_kernel(int D, fid_pchol_head *head, const double *diag, int32_t *info) {
    const int lane = threadIdx.x;
    double d0;
    int at;
    wave_argmax(diag, D, lane, &d0, &at);
    if (lane != 0) return;
    info[1] = head->status;
    if (head->status != 0) {
        head->done = 1;
        return;
    }
    info[0] = 0;
    head->tol = (double)D * FID_EPS * d0;
    if (!(d0 > 0.0)) head->done = 1;
}

__global__ __launch_bounds__(NT) void pchol_step_kernel(const double *__restrict__ S, int64_t lds, int D, int j, double *L, int64_t ldl,
                                                        int32_t *piv, int32_t *info, fid_pchol_head *head, double *diag) {
    if (head->done) return;
    const int lane = threadIdx.x & 63, wave = blockIdx.x * WAVES + (threadIdx.x >> 6);
    const double *cur = diag + (int64_t)(j & 1) * D;
    double *nxt = diag + (int64_t)((j + 1) & 1) * D;
    double dmax;
    int p;
    wave_argmax(cur, D, lane, &dmax, &p);
    // the stop rule.  Every wave of this launch decides the same from the same diagonal, whether it has seen `done` or not.
    if (!(dmax > head->tol)) {
        if (wave == 0 && lane == 0) head->done = 1;
        return;
    }
    if (wave == 0 && lane == 0) piv[j] = p, info[0] = j + 1;
    const double root = sqrt(dmax);
    for (int t = 0; t < FID_ROWS_PER_WAVE; ++t) {
        const int i = wave * FID_ROWS_PER_WAVE + t;
        if (i >= D) return;
        const double dcur = cur[i];
        double val, left;
        if (dcur == FID_PIVOTED) {
            val = 0.0, left = FID_PIVOTED;
        } else if (i == p) {
            val = root, left = FID_PIVOTED;
        } else {
            const double dot = wave_dot(L + (int64_t)i * ldl, 1, L + (int64_t)p * ldl, 1, j, lane);
            val = (S[(int64_t)i * lds + p] - dot) / root;
            left = dcur - val * val;
        }
        if (lane == 0) L[(int64_t)i * ldl + j] = val, nxt[i] = left;
    }
}

// ---------------------------------------------------------------- eigenvalues of a symmetric matrix
__global__ __launch_bounds__(NT) void eig_copy_kernel(const double *__restrict__ A, int64_t lda, int n, fid_eig_head *head, double *W) {
    const int64_t total = (int64_t)n * n;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
        const double v = A[(i / n) * lda + i % n];
        bad |= !fid_finite(v);
        W[i] = v;
    }
    if (bad) head->status = HOIG_EINVAL;
}

// step k: d[k], and the reflector that clears W[k + 2 .., k]: v (indexed by row; v[k + 1] = 1), tau, e[k]
__global__ __launch_bounds__(FID_WAVE) void eig_reflector_kernel(int n, int k, fid_eig_head *head, const double *W, double *d, double *e,
                                                                 double *v, int32_t *info) {
    const int lane = threadIdx.x;
    if (k == 0 && lane == 0) {
        info[0] = head->status;
        if (head->status != 0) head->done = 1;
    }
    if (head->status != 0) return;
    const double *x = W + (int64_t)(k + 1) * n + k;             // the column below the diagonal, n apart
    const int m = n - k - 1;
    if (m < 1) {
        if (lane == 0) d[k] = W[(int64_t)k * n + k], head->tau = 0.0;
        return;
    }
    const double sigma = wave_dot(x + n, n, x + n, n, m - 1, lane);
    double tau, beta, scale;
    fid_reflector(x[0], sigma, &tau, &beta, &scale);
    for (int t = lane; t < m; t += FID_WAVE) v[k + 1 + t] = t == 0 ? 1.0 : x[(int64_t)t * n] * scale;
    if (lane == 0) d[k] = W[(int64_t)k * n + k], e[k] = beta, head->tau = tau;
}

// p = tau W22 v
__global__ __launch_bounds__(NT) void eig_symv_kernel(int n, int k, const fid_eig_head *head, const double *W, const double *v, double *p) {
    const double tau = head->tau;
    if (head->done || tau == 0.0) return;
    const int lane = threadIdx.x & 63, wave = blockIdx.x * WAVES + (threadIdx.x >> 6), m = n - k - 1;
    for (int t = 0; t < FID_ROWS_PER_WAVE; ++t) {
        const int i = k + 1 + wave * FID_ROWS_PER_WAVE + t;
        if (i >= n) return;
        const double dot = wave_dot(W + (int64_t)i * n + k + 1, 1, v + k + 1, 1, m, lane);
        if (lane == 0) p[i] = tau * dot;
    }
}

// W22 -= v w^T + w v^T with w = p - (tau / 2) (p^T v) v
__global__ __launch_bounds__(NT) void eig_rank2_kernel(int n, int k, const fid_eig_head *head, double *W, const double *v, const double *p) {
    const double tau = head->tau;
    if (head->done || tau == 0.0) return;
    const int lane = threadIdx.x & 63, wave = blockIdx.x * WAVES + (threadIdx.x >> 6), m = n - k - 1;
    const double c = (0.5 * tau) * wave_dot(p + k + 1, 1, v + k + 1, 1, m, lane);
    for (int t = 0; t < FID_ROWS_PER_WAVE; ++t) {
        const int i = k + 1 + wave * FID_ROWS_PER_WAVE + t;
        if (i >= n) return;
        const double vi = v[i], wi = p[i] - c * vi;
        double *row = W + (int64_t)i * n;
        for (int jj = k + 1 + lane; jj < n; jj += FID_WAVE) {
            const double vj = v[jj], wj = p[jj] - c * vj;
            row[jj] = row[jj] - (vi * wj + wi * vj);
        }
    }
}

__global__ __launch_bounds__(FID_WAVE) void eig_bisect_kernel(int n, const int32_t *done, const double *d, const double *e, double *lambda) {
    if (done && *done) return;
    const int idx = blockIdx.x * FID_WAVE + threadIdx.x;
    if (idx >= n) return;
    double gl, gu, pivmin;
    fid_gershgorin(d, e, n, &gl, &gu, &pivmin);
    lambda[idx] = fid_bisect(d, e, n, idx, gl, gu, pivmin);
}

int row_grid(int rows) { return (int)hoig_cdiv(rows, ROWS_PER_BLOCK); }

}  // namespace

extern "C" int hoig_gemm_tn_f64(const void *A, int64_t lda, const void *B, int64_t ldb, const double *pivot, double *C, int64_t ldc, int M,
                                int N, int K, int flags, hoig_stream_t stream) {
    if (((!A || !B) && K > 0) || !C || M < 1 || N < 1 || K < 0 || lda < M || ldb < N || ldc < N) return HOIG_EINVAL;
    if (flags & ~(HOIG_GEMM_ACCUMULATE | HOIG_GEMM_SYMMETRIC | HOIG_GEMM_F32)) return HOIG_EINVAL;
    const int sym = (flags & HOIG_GEMM_SYMMETRIC) != 0, acc = (flags & HOIG_GEMM_ACCUMULATE) != 0;
    if (sym && (A != B || M != N || lda != ldb)) return HOIG_EINVAL;
    if (pivot && !(flags & HOIG_GEMM_F32)) return HOIG_EINVAL;
    const dim3 grid((unsigned)hoig_cdiv(N, 64), (unsigned)hoig_cdiv(M, 64));
    hipStream_t st = (hipStream_t)stream;
    if (flags & HOIG_GEMM_F32)
        gemm_tn_kernel<1><<<grid, NT, 0, st>>>(A, lda, B, ldb, pivot, C, ldc, M, N, K, acc, sym);
    else
        gemm_tn_kernel<0><<<grid, NT, 0, st>>>(A, lda, B, ldb, pivot, C, ldc, M, N, K, acc, sym);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}

extern "C" int hoig_pchol_f64(const double *S, int64_t lds, int D, double *L, int64_t ldl, int32_t *piv, int32_t *info, void *workspace,
                              int64_t workspace_bytes, hoig_stream_t stream) {
    if (!S || !L || !piv || !info || !workspace || D < 1 || lds < D || ldl < D) return HOIG_EINVAL;
    if (((uintptr_t)workspace & 7) || workspace_bytes < hoig_pchol_f64_workspace_bytes(D)) return HOIG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    fid_pchol_head *head = static_cast<fid_pchol_head *>(workspace);
    double *diag = reinterpret_cast<double *>(head + 1);
    if (hipMemsetAsync(head, 0, sizeof(fid_pchol_head), st) != hipSuccess) return HOIG_ELAUNCH;
    pchol_scan_kernel<<<hoig_stream_grid((int64_t)D * D, NT), NT, 0, st>>>(S, lds, D, head, diag);
    HOIG_LAUNCH_CHECK();
    pchol_init_kernel<<<1, FID_WAVE, 0, st>>>(D, head, diag, info);
    HOIG_LAUNCH_CHECK();
    for (int j = 0; j < D; ++j) {
        pchol_step_kernel<<<row_grid(D), NT, 0, st>>>(S, lds, D, j, L, ldl, piv, info, head, diag);
        HOIG_LAUNCH_CHECK();
    }
    return HOIG_OK;
}

extern "C" int hoig_tridiag_eigvals_f64(const double *d, const double *e, int n, double *lambda, hoig_stream_t stream) {
    if (!d || !lambda || n < 1 || (n > 1 && !e)) return HOIG_EINVAL;
    eig_bisect_kernel<<<(unsigned)hoig_cdiv(n, FID_WAVE), FID_WAVE, 0, (hipStream_t)stream>>>(n, nullptr, d, e, lambda);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}

extern "C" int hoig_sym_eigvals_f64(const double *A, int64_t lda, int n, double *lambda, int32_t *info, void *workspace,
                                    int64_t workspace_bytes, hoig_stream_t stream) {
    if (!A || !lambda || !info || !workspace || n < 1 || lda < n) return HOIG_EINVAL;
    if (((uintptr_t)workspace & 7) || workspace_bytes < hoig_sym_eigvals_f64_workspace_bytes(n)) return HOIG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    fid_eig_head *head = static_cast<fid_eig_head *>(workspace);
    double *W = reinterpret_cast<double *>(head + 1), *d = W + (int64_t)n * n, *e = d + n, *v = e + n, *p = v + n;
    if (hipMemsetAsync(head, 0, sizeof(fid_eig_head), st) != hipSuccess) return HOIG_ELAUNCH;
    eig_copy_kernel<<<hoig_stream_grid((int64_t)n * n, NT), NT, 0, st>>>(A, lda, n, head, W);
    HOIG_LAUNCH_CHECK();
    for (int k = 0; k < n; ++k) {
        eig_reflector_kernel<<<1, FID_WAVE, 0, st>>>(n, k, head, W, d, e, v, info);
        HOIG_LAUNCH_CHECK();
        if (k + 2 < n) {
            eig_symv_kernel<<<row_grid(n - k - 1), NT, 0, st>>>(n, k, head, W, v, p);
            HOIG_LAUNCH_CHECK();
            eig_rank2_kernel<<<row_grid(n - k - 1), NT, 0, st>>>(n, k, head, W, v, p);
            HOIG_LAUNCH_CHECK();
        }
    }
    eig_bisect_kernel<<<(unsigned)hoig_cdiv(n, FID_WAVE), FID_WAVE, 0, st>>>(n, &head->done, d, e, lambda);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}
