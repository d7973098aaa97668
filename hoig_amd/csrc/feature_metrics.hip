// Feature-space metrics on the device, in fp64 (docs/feature_metrics.md; the shared per-lane code, the tile geometry and the workspace
// layouts: feature_metrics.h).
//
// fm_tile: a workgroup's 64 x 64 tile of P Q^T for 64 rows of P and 64 rows of Q, each a (gathered or contiguous) row of a row-major
//   fp32 [n][D] matrix -- the NT form: K is contiguous in both operands.  A k-step of the MFMA touches 16 different rows, so the rows
//   are staged through LDS in panels of FM_KP columns: eight lanes read one 128-byte line of a row (one 16-byte load each when D is a
//   multiple of 4 and the base is aligned, scalar loads otherwise), widen to fp64 (exact), take the pivot off, and store doubles.  The
//   next panel's loads are in flight while this one is multiplied.  A panel row is FM_KP + 2 doubles long: the 32 lanes of a
//   ds_read_b64 group (16 rows x 2 k) then fall into 32 different bank pairs.  v_mfma_f64_16x16x4_f64 with the fp64 lane maps
//   (fid_stats.hip): lane l gives P[row l & 15][k = l >> 4] and Q[row l & 15][k = l >> 4], result register r is the element at row
//   (l >> 4) + 4 r, column l & 15.  Rows and columns out of range are zeros.  The tile is never stored to global memory.
// hoig_kid_poly_f64: grid (tile slot, term, subset); the epilogue is fm_kid_lane, the wave butterfly and the four wave sums in wave
//   order, one partial per workgroup at its own slot; kid_finish_kernel, one wave per subset, adds the slots in slot order.
// hoig_knn_radius_f64: grid (row tile, column chunk); the tile of squared distances goes through LDS to one thread per (row, 16
//   columns), which keeps its FM_KMAX smallest in registers (fm_insert has static indices only); the four lists of a row meet in LDS,
//   the chunks' lists in knn_merge_kernel.
// hoig_manifold_hits_f64: grid (probe tile, row chunk); integer counts per probe column, added over lanes, waves and chunks.
// No floating-point atomics and no launch that waits for another workgroup: every sum has one owner and a fixed order.  The status word
// is an integer OR.  Built with -ffp-contract=off.
#include "common.h"
#include "feature_metrics.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int NT = 256;                      // four waves
constexpr int FM_KP = 32;                    // columns of a panel: 32 floats are one 128-byte line
constexpr int FM_LDP = FM_KP + 2;            // doubles of a panel row
constexpr int FM_PANEL = 2 * FM_TILE * FM_LDP;   // doubles of a panel: 64 rows of P, then 64 rows of Q
constexpr int FM_LDT = FM_TILE + 1;          // doubles of a row of the distance tile kept in the same LDS
static_assert(FM_TILE * FM_LDT <= FM_PANEL, "the distance tile reuses the panel");

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, FID_WAVE);
    return v;
}

// this thread's part of one panel: columns k0 + 4 (t & 7) .. + 3 of panel rows (t >> 3) + 32 q
template <bool VEC>
__device__ __forceinline__ void fm_load(const float *(&rowp)[4], int D, int k0, int c4, float (&stage)[4][4]) {
    const int col = k0 + 4 * c4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (VEC) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (rowp[q] && col < D) v = *reinterpret_cast<const float4 *>(rowp[q] + col);      // (D % 4 == 0: col + 3 < D)
            stage[q][0] = v.x, stage[q][1] = v.y, stage[q][2] = v.z, stage[q][3] = v.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) stage[q][e] = (rowp[q] && col + e < D) ? rowp[q][col + e] : 0.f;
        }
    }
}

// acc += P Q^T over all of K.  rowp: this thread's four staging rows (panel rows (t >> 3) + 32 q; nullptr: a row of zeros).
// Returns whether this thread read a non-finite feature.  Every thread of the workgroup calls it (it synchronises).
template <bool VEC>
__device__ __forceinline__ bool fm_tile(const float *(&rowp)[4], int D, const double *__restrict__ pivot, double *panel,
                                        f64x4 (&acc)[2][2]) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 15, kq = lane >> 4;
    const int srow = t >> 3, c4 = t & 7;
    const double *pa = panel + (32 * (wave >> 1) + r) * FM_LDP + kq;
    const double *pb = panel + (FM_TILE + 32 * (wave & 1) + r) * FM_LDP + kq;
    bool bad = false;
    float stage[4][4];
    fm_load<VEC>(rowp, D, 0, c4, stage);
    for (int k0 = 0; k0 < D; k0 += FM_KP) {
        __syncthreads();                                  // the panel (or the distance tile in its place) has been read
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int col = k0 + 4 * c4 + e;
                double v = 0.0;
                if (rowp[q] && col < D) {
                    v = (double)stage[q][e];
                    bad |= !fid_finite(v);
                    if (pivot) v = v - pivot[col];
                }
                panel[(srow + 32 * q) * FM_LDP + 4 * c4 + e] = v;
            }
        __syncthreads();
        if (k0 + FM_KP < D) fm_load<VEC>(rowp, D, k0 + FM_KP, c4, stage);
        const int steps = D - k0 < FM_KP ? (D - k0 + 3) >> 2 : FM_KP / 4;
        for (int kk = 0; kk < steps; ++kk) {
            double a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = pa[16 * i * FM_LDP + 4 * kk], b[i] = pb[16 * i * FM_LDP + 4 * kk];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    return bad;
}

__device__ __forceinline__ void fm_zero(f64x4 (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
}

// contiguous rows: panel rows 0 .. 63 are rows p0 .. of P [np][D], rows 64 .. 127 rows q0 .. of Q [nq][D]
__device__ __forceinline__ void fm_rows(const float *P, int np, int p0, const float *Q, int nq, int q0, int D, const float *(&rowp)[4]) {
    const int srow = threadIdx.x >> 3;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int lrow = (srow + 32 * q) & (FM_TILE - 1);
        const bool isp = q < 2;
        const int row = (isp ? p0 : q0) + lrow;
        rowp[q] = row < (isp ? np : nq) ? (isp ? P : Q) + (int64_t)row * D : nullptr;
    }
}

// ---------------------------------------------------------------- KID
template <bool VEC>
__global__ __launch_bounds__(NT) void kid_kernel(const float *__restrict__ X, int nx, const float *__restrict__ Y, int ny, int D,
                                                 const int32_t *__restrict__ ix, const int32_t *__restrict__ iy, int m, int nt,
                                                 double gamma, double coef0, int degree, double *partials, int32_t *status) {
    __shared__ double panel[FM_PANEL];
    __shared__ double wsum[FM_WAVES];
    const int e = blockIdx.x, ti = e / nt, tj = e % nt, term = blockIdx.y, s = blockIdx.z;
    if (!fm_kid_slot_runs(term, ti, tj)) return;
    const float *P = term == FM_TERM_YY ? Y : X, *Q = term == FM_TERM_XX ? X : Y;
    const int np = term == FM_TERM_YY ? ny : nx, nq = term == FM_TERM_XX ? nx : ny;
    const int32_t *tp = (term == FM_TERM_YY ? iy : ix) + (int64_t)s * m, *tq = (term == FM_TERM_XX ? ix : iy) + (int64_t)s * m;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, srow = t >> 3;
    int clamped = 0;
    const float *rowp[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int lrow = (srow + 32 * q) & (FM_TILE - 1);
        const bool isp = q < 2;
        const int pos = (isp ? ti : tj) * FM_TILE + lrow;
        rowp[q] = nullptr;
        if (pos < m) rowp[q] = (isp ? P : Q) + (int64_t)fm_clamp_index((isp ? tp : tq)[pos], isp ? np : nq, &clamped) * D;
    }
    f64x4 acc[2][2];
    fm_zero(acc);
    const bool bad = fm_tile<VEC>(rowp, D, nullptr, panel, acc);
    const int flags = (bad ? FM_STATUS_NONFINITE : 0) | (clamped ? FM_STATUS_CLAMPED : 0);
    if (flags) atomicOr(status, flags);
    double v[16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) v[(i * 2 + j) * 4 + reg] = acc[i][j][reg];
    const double mine = wave_sum(fm_kid_lane(v, wave, lane, ti, tj, term, m, gamma, coef0, degree));
    if (lane == 0) wsum[wave] = mine;
    __syncthreads();
    if (t == 0) partials[((int64_t)s * 3 + term) * nt * nt + e] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ __launch_bounds__(FID_WAVE) void kid_finish_kernel(const double *__restrict__ partials, int m, int nt,
                                                              const int32_t *__restrict__ status, double *out) {
    const int s = blockIdx.x, lane = threadIdx.x;
    double sums[3];
#pragma unroll
    for (int term = 0; term < 3; ++term)
        sums[term] = wave_sum(fm_kid_lane_finish(partials + ((int64_t)s * 3 + term) * nt * nt, term, nt, lane));
    if (lane != 0) return;
    const bool refused = status && *status != 0;
    const double nan = __builtin_nan("");
    out[4 * s + 0] = refused ? nan : sums[0];
    out[4 * s + 1] = refused ? nan : sums[1];
    out[4 * s + 2] = refused ? nan : sums[2];
    out[4 * s + 3] = refused ? nan : fm_mmd2(sums[0], sums[1], sums[2], m);
}

// ---------------------------------------------------------------- squared norms of the pivoted rows: a wave per row
__global__ __launch_bounds__(NT) void sqnorm_kernel(const float *__restrict__ X, int n, int D, const double *__restrict__ pivot,
                                                    double *norms) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * FM_WAVES + (threadIdx.x >> 6);
    if (row >= n) return;
    const double v = wave_sum(fm_lane_sqnorm(X + (int64_t)row * D, D, pivot, lane));
    if (lane == 0) norms[row] = v;
}

// ---------------------------------------------------------------- the k-th nearest neighbour's squared distance
template <bool VEC>
__global__ __launch_bounds__(NT) void knn_kernel(const float *__restrict__ X, int n, int D, const double *__restrict__ pivot,
                                                 const double *__restrict__ norms, int chunk_tiles, double *cand, int32_t *status) {
    __shared__ double panel[FM_PANEL];
    __shared__ double lists[FM_WAVES * FM_KMAX * FM_TILE];
    const int ti = blockIdx.x, chunk = blockIdx.y, nt = fm_tiles(n);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lrow = t & 63, part = t >> 6;
    double best[FM_KMAX];
#pragma unroll
    for (int s = 0; s < FM_KMAX; ++s) best[s] = HUGE_VAL;
    bool bad = false;
    const int last = min(nt, (chunk + 1) * chunk_tiles);
    for (int tj = chunk * chunk_tiles; tj < last; ++tj) {
        const float *rowp[4];
        fm_rows(X, n, ti * FM_TILE, X, n, tj * FM_TILE, D, rowp);
        f64x4 acc[2][2];
        fm_zero(acc);
        bad |= fm_tile<VEC>(rowp, D, pivot, panel, acc);
        __syncthreads();                                  // the last panel has been read: the distance tile takes its place
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = fm_lane_col(wave, lane, j), gj = tj * FM_TILE + col;
            const double nj = gj < n ? norms[gj] : 0.0;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int row = fm_lane_row(wave, lane, i, reg), gi = ti * FM_TILE + row;
                    double d = HUGE_VAL;                  // out of range, or the row itself (left out by index, not by value)
                    if (gi < n && gj < n && gi != gj) d = fm_dist2(norms[gi], nj, acc[i][j][reg]);
                    panel[row * FM_LDT + col] = d;
                }
        }
        __syncthreads();
        for (int c = 0; c < 16; ++c) fm_insert(best, panel[lrow * FM_LDT + 16 * part + c]);
    }
    if (bad) atomicOr(status, FM_STATUS_NONFINITE);
#pragma unroll
    for (int s = 0; s < FM_KMAX; ++s) lists[(part * FM_KMAX + s) * FM_TILE + lrow] = best[s];
    __syncthreads();
    const int gi = ti * FM_TILE + lrow;
    if (part != 0 || gi >= n) return;
    for (int e = FM_KMAX; e < FM_WAVES * FM_KMAX; ++e) fm_insert(best, lists[e * FM_TILE + lrow]);
#pragma unroll
    for (int s = 0; s < FM_KMAX; ++s) cand[((int64_t)chunk * n + gi) * FM_KMAX + s] = best[s];
}

__global__ __launch_bounds__(NT) void knn_merge_kernel(const double *__restrict__ cand, int n, int chunks, int k,
                                                       const int32_t *__restrict__ status, double *radius) {
    const int gi = blockIdx.x * NT + threadIdx.x;
    if (gi >= n) return;
    double best[FM_KMAX];
#pragma unroll
    for (int s = 0; s < FM_KMAX; ++s) best[s] = HUGE_VAL;
    for (int c = 0; c < chunks; ++c)
        for (int s = 0; s < FM_KMAX; ++s) fm_insert(best, cand[((int64_t)c * n + gi) * FM_KMAX + s]);
    radius[gi] = *status != 0 ? __builtin_nan("") : fm_pick(best, k);
}

// ---------------------------------------------------------------- ball memberships
template <bool VEC>
__global__ __launch_bounds__(NT) void hits_kernel(const float *__restrict__ X, int nx, const double *__restrict__ radius,
                                                  const float *__restrict__ Y, int ny, int D, const double *__restrict__ pivot,
                                                  const double *__restrict__ xnorm, const double *__restrict__ ynorm, int chunk_tiles,
                                                  int32_t *counts, int32_t *status) {
    __shared__ double panel[FM_PANEL];
    __shared__ int32_t colcnt[2][FM_TILE];
    const int tj = blockIdx.x, chunk = blockIdx.y, nt = fm_tiles(nx);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int cnt[2] = {0, 0};
    bool bad = false;
    const int last = min(nt, (chunk + 1) * chunk_tiles);
    for (int ti = chunk * chunk_tiles; ti < last; ++ti) {
        const float *rowp[4];
        fm_rows(X, nx, ti * FM_TILE, Y, ny, tj * FM_TILE, D, rowp);
        f64x4 acc[2][2];
        fm_zero(acc);
        bad |= fm_tile<VEC>(rowp, D, pivot, panel, acc);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int gi = ti * FM_TILE + fm_lane_row(wave, lane, i, reg);
                if (gi >= nx) continue;
                const double ni = xnorm[gi], ri = radius[gi];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int gj = tj * FM_TILE + fm_lane_col(wave, lane, j);
                    if (gj < ny && fm_dist2(ni, ynorm[gj], acc[i][j][reg]) <= ri) ++cnt[j];
                }
            }
    }
    if (bad) atomicOr(status, FM_STATUS_NONFINITE);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        cnt[j] += __shfl_xor(cnt[j], 16, FID_WAVE);
        cnt[j] += __shfl_xor(cnt[j], 32, FID_WAVE);
        if (lane < 16) colcnt[wave >> 1][fm_lane_col(wave, lane, j)] = cnt[j];
    }
    __syncthreads();
    const int gj = tj * FM_TILE + t;
    if (t < FM_TILE && gj < ny) counts[(int64_t)chunk * ny + gj] = colcnt[0][t] + colcnt[1][t];
}

__global__ __launch_bounds__(NT) void hits_sum_kernel(const int32_t *__restrict__ counts, int ny, int chunks, int32_t *hits) {
    const int gj = blockIdx.x * NT + threadIdx.x;
    if (gj >= ny) return;
    int total = 0;
    for (int c = 0; c < chunks; ++c) total += counts[(int64_t)c * ny + gj];
    hits[gj] = total;
}

// 16-byte loads need rows that start on 16 bytes
bool fm_vec(const void *a, const void *b, int D) { return (D & 3) == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

}  // namespace

extern "C" int hoig_kid_finish_f64(const double *partials, int S, int m, const int32_t *status, double *out, hoig_stream_t stream) {
    if (!partials || !out || S < 1 || S > 65535 || m < 2) return HOIG_EINVAL;
    return hoig_launch<kid_finish_kernel>(dim3((unsigned)S), dim3(FID_WAVE), 0, (hipStream_t)stream, partials, m, fm_tiles(m), status, out);
}

extern "C" int hoig_kid_poly_f64(const float *X, int nx, const float *Y, int ny, int D, const int32_t *ix, const int32_t *iy, int S, int m,
                                 double gamma, double coef0, int degree, double *out, int32_t *status, void *workspace,
                                 int64_t workspace_bytes, hoig_stream_t stream) {
    if (!X || !Y || !ix || !iy || !out || !status || !workspace || nx < 1 || ny < 1 || D < 1 || degree < 1 || degree > 4)
        return HOIG_EINVAL;
    if (S < 1 || S > 65535 || m < 2) return HOIG_EINVAL;
    if (((uintptr_t)workspace & 7) || workspace_bytes < hoig_kid_workspace_bytes(S, m)) return HOIG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int nt = fm_tiles(m);
    double *partials = static_cast<double *>(workspace);
    if (hipMemsetAsync(status, 0, sizeof(int32_t), st) != hipSuccess) return HOIG_ELAUNCH;
    const dim3 grid((unsigned)(nt * nt), 3, (unsigned)S);
    const int rc = fm_vec(X, Y, D)
                       ? hoig_launch<kid_kernel<true>>(grid, dim3(NT), 0, st, X, nx, Y, ny, D, ix, iy, m, nt, gamma, coef0, degree, partials, status)
                       : hoig_launch<kid_kernel<false>>(grid, dim3(NT), 0, st, X, nx, Y, ny, D, ix, iy, m, nt, gamma, coef0, degree, partials, status);
    if (rc != HOIG_OK) return rc;
    return hoig_kid_finish_f64(partials, S, m, status, out, stream);
}

extern "C" int hoig_knn_radius_f64(const float *X, int n, int D, const double *pivot, int k, double *radius, int32_t *status,
                                   void *workspace, int64_t workspace_bytes, hoig_stream_t stream) {
    if (!X || !radius || !status || !workspace || n < 2 || D < 1 || k < 1 || k > FM_KMAX || k > n - 1) return HOIG_EINVAL;
    if (((uintptr_t)workspace & 7) || workspace_bytes < hoig_knn_workspace_bytes(n)) return HOIG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int nt = fm_tiles(n), chunk_tiles = fm_chunk_tiles(nt), chunks = fm_chunks(nt);
    double *norms = static_cast<double *>(workspace), *cand = norms + n;
    if (hipMemsetAsync(status, 0, sizeof(int32_t), st) != hipSuccess) return HOIG_ELAUNCH;
    int rc = hoig_launch<sqnorm_kernel>(dim3((unsigned)hoig_cdiv(n, FM_WAVES)), dim3(NT), 0, st, X, n, D, pivot, norms);
    if (rc != HOIG_OK) return rc;
    const dim3 grid((unsigned)nt, (unsigned)chunks);
    rc = fm_vec(X, X, D) ? hoig_launch<knn_kernel<true>>(grid, dim3(NT), 0, st, X, n, D, pivot, norms, chunk_tiles, cand, status)
                         : hoig_launch<knn_kernel<false>>(grid, dim3(NT), 0, st, X, n, D, pivot, norms, chunk_tiles, cand, status);
    if (rc != HOIG_OK) return rc;
    return hoig_launch<knn_merge_kernel>(dim3((unsigned)hoig_cdiv(n, NT)), dim3(NT), 0, st, cand, n, chunks, k, status, radius);
}

extern "C" int hoig_manifold_hits_f64(const float *X, int nx, const double *radius, const float *Y, int ny, int D, const double *pivot,
                                      int32_t *hits, int32_t *status, void *workspace, int64_t workspace_bytes, hoig_stream_t stream) {
    if (!X || !radius || !Y || !hits || !status || !workspace || nx < 1 || ny < 1 || D < 1) return HOIG_EINVAL;
    if (((uintptr_t)workspace & 7) || workspace_bytes < hoig_manifold_hits_workspace_bytes(nx, ny)) return HOIG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int nt = fm_tiles(nx), chunk_tiles = fm_chunk_tiles(nt), chunks = fm_chunks(nt);
    double *xnorm = static_cast<double *>(workspace), *ynorm = xnorm + nx;
    int32_t *counts = reinterpret_cast<int32_t *>(ynorm + ny);
    if (hipMemsetAsync(status, 0, sizeof(int32_t), st) != hipSuccess) return HOIG_ELAUNCH;
    int rc = hoig_launch<sqnorm_kernel>(dim3((unsigned)hoig_cdiv(nx, FM_WAVES)), dim3(NT), 0, st, X, nx, D, pivot, xnorm);
    if (rc != HOIG_OK) return rc;
    rc = hoig_launch<sqnorm_kernel>(dim3((unsigned)hoig_cdiv(ny, FM_WAVES)), dim3(NT), 0, st, Y, ny, D, pivot, ynorm);
    if (rc != HOIG_OK) return rc;
    const dim3 grid((unsigned)fm_tiles(ny), (unsigned)chunks);
    rc = fm_vec(X, Y, D)
             ? hoig_launch<hits_kernel<true>>(grid, dim3(NT), 0, st, X, nx, radius, Y, ny, D, pivot, xnorm, ynorm, chunk_tiles, counts, status)
             : hoig_launch<hits_kernel<false>>(grid, dim3(NT), 0, st, X, nx, radius, Y, ny, D, pivot, xnorm, ynorm, chunk_tiles, counts, status);
    if (rc != HOIG_OK) return rc;
    return hoig_launch<hits_sum_kernel>(dim3((unsigned)hoig_cdiv(ny, NT)), dim3(NT), 0, st, counts, ny, chunks, hits);
}
