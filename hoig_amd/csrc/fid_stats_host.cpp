// The host half of the fp64 FID statistics (fid_stats.h, docs/fid_device.md): the workspace sizes, and CPU twins that run the shared
// per-lane code with a wave walked lane by lane -- the same pivots, the same order in every sum.  No HIP call; host memory only.
// Built with -ffp-contract=off.
#include <string.h>

#include <vector>

#include "fid_stats.h"

namespace {

// the butterfly of the device's wave sum: afterwards every entry holds what every lane holds there
double fid_butterfly(double *v) {
    double t[FID_WAVE];
    for (int o = 32; o > 0; o >>= 1) {
        for (int l = 0; l < FID_WAVE; ++l) t[l] = v[l] + v[l ^ o];
        memcpy(v, t, sizeof(t));
    }
    return v[0];
}

// sum a[k * sa] b[k * sb] as a wave makes it: lane l takes k = l, l + 64, .. (fid_lane_dot), walked here 64 lanes at a time
double wave_dot(const double *a, int64_t sa, const double *b, int64_t sb, int n) {
    double part[FID_WAVE] = {0.0};
    for (int k0 = 0; k0 < n; k0 += FID_WAVE) {
        const int lanes = n - k0 < FID_WAVE ? n - k0 : FID_WAVE;
        for (int l = 0; l < lanes; ++l) part[l] = part[l] + a[(k0 + l) * sa] * b[(k0 + l) * sb];
    }
    return fid_butterfly(part);
}

void argmax(const double *v, int n, double *best, int *at) {
    double bv = -HUGE_VAL;
    int bi = 0x7fffffff;
    for (int i = 0; i < n; ++i)
        if (fid_better(v[i], i, bv, bi)) bv = v[i], bi = i;
    *best = bv, *at = bi;
}

bool all_finite(const double *a, int64_t ld, int rows, int cols) {
    for (int i = 0; i < rows; ++i)
        for (int j = 0; j < cols; ++j)
            if (!fid_finite(a[i * ld + j])) return false;
    return true;
}

}  // namespace

extern "C" int64_t hoig_pchol_f64_workspace_bytes(int D) {
    if (D < 1) return HOIG_EINVAL;
    return (int64_t)sizeof(fid_pchol_head) + 2 * (int64_t)D * (int64_t)sizeof(double);
}

extern "C" int64_t hoig_sym_eigvals_f64_workspace_bytes(int n) {
    if (n < 1) return HOIG_EINVAL;
    return (int64_t)sizeof(fid_eig_head) + ((int64_t)n * n + 4 * (int64_t)n) * (int64_t)sizeof(double);
}

extern "C" int hoig_gemm_tn_f64_host(const void *A, int64_t lda, const void *B, int64_t ldb, const double *pivot, double *C, int64_t ldc,
                                     int M, int N, int K, int flags) {
    if (((!A || !B) && K > 0) || !C || M < 1 || N < 1 || K < 0 || lda < M || ldb < N || ldc < N) return HOIG_EINVAL;
    if (flags & ~(HOIG_GEMM_ACCUMULATE | HOIG_GEMM_SYMMETRIC | HOIG_GEMM_F32)) return HOIG_EINVAL;
    const int sym = (flags & HOIG_GEMM_SYMMETRIC) != 0, acc = (flags & HOIG_GEMM_ACCUMULATE) != 0, f32 = (flags & HOIG_GEMM_F32) != 0;
    if (sym && (A != B || M != N || lda != ldb)) return HOIG_EINVAL;
    if (pivot && !f32) return HOIG_EINVAL;
    // the products of one k at a time into a row of sums: K additions per element, in order of k, as the MFMA chain walks them
    std::vector<double> arow((size_t)M), brow((size_t)N);
    std::vector<double> out((size_t)M * N, 0.0);
    for (int k = 0; k < K; ++k) {
        for (int m = 0; m < M; ++m) arow[m] = fid_operand(A, (int64_t)k * lda + m, f32, pivot, m);
        for (int n = 0; n < N; ++n) brow[n] = fid_operand(B, (int64_t)k * ldb + n, f32, pivot, n);
        for (int m = 0; m < M; ++m) {
            double *o = out.data() + (size_t)m * N;
            const double a = arow[m];
            for (int n = sym ? m : 0; n < N; ++n) o[n] = o[n] + a * brow[n];
        }
    }
    for (int m = 0; m < M; ++m)
        for (int n = sym ? m : 0; n < N; ++n) {
            double v = out[(size_t)m * N + n];
            if (acc) v = C[(int64_t)m * ldc + n] + v;
            C[(int64_t)m * ldc + n] = v;
            if (sym && n != m) C[(int64_t)n * ldc + m] = v;
        }
    return HOIG_OK;
}

extern "C" int hoig_pchol_f64_host(const double *S, int64_t lds, int D, double *L, int64_t ldl, int32_t *piv, int32_t *info) {
    if (!S || !L || !piv || !info || D < 1 || lds < D || ldl < D) return HOIG_EINVAL;
    if (!all_finite(S, lds, D, D)) {
        info[1] = HOIG_EINVAL;
        return HOIG_EINVAL;
    }
    info[0] = 0, info[1] = 0;
    std::vector<double> cur((size_t)D), nxt((size_t)D);
    for (int i = 0; i < D; ++i) cur[i] = S[i * lds + i];
    double d0;
    int p;
    argmax(cur.data(), D, &d0, &p);
    if (!(d0 > 0.0)) return HOIG_OK;
    const double tol = (double)D * FID_EPS * d0;
    for (int j = 0; j < D; ++j) {
        double dmax;
        argmax(cur.data(), D, &dmax, &p);
        if (!(dmax > tol)) break;
        piv[j] = p, info[0] = j + 1;
        const double root = sqrt(dmax);
        for (int i = 0; i < D; ++i) {
            double val, left;
            if (cur[i] == FID_PIVOTED) {
                val = 0.0, left = FID_PIVOTED;
            } else if (i == p) {
                val = root, left = FID_PIVOTED;
            } else {
                const double dot = wave_dot(L + (int64_t)i * ldl, 1, L + (int64_t)p * ldl, 1, j);
                val = (S[(int64_t)i * lds + p] - dot) / root;
                left = cur[i] - val * val;
            }
            L[(int64_t)i * ldl + j] = val, nxt[i] = left;
        }
        cur.swap(nxt);
    }
    return HOIG_OK;
}

extern "C" int hoig_tridiag_eigvals_f64_host(const double *d, const double *e, int n, double *lambda) {
    if (!d || !lambda || n < 1 || (n > 1 && !e)) return HOIG_EINVAL;
    double gl, gu, pivmin;
    fid_gershgorin(d, e, n, &gl, &gu, &pivmin);
    for (int idx = 0; idx < n; ++idx) lambda[idx] = fid_bisect(d, e, n, idx, gl, gu, pivmin);
    return HOIG_OK;
}

extern "C" int hoig_sym_tridiag_f64_host(const double *A, int64_t lda, int n, double *d, double *e) {
    if (!A || !d || n < 1 || lda < n || (n > 1 && !e)) return HOIG_EINVAL;
    if (!all_finite(A, lda, n, n)) return HOIG_EINVAL;
    std::vector<double> Wv((size_t)n * n), v((size_t)n), p((size_t)n);
    double *W = Wv.data();
    for (int i = 0; i < n; ++i) memcpy(W + (size_t)i * n, A + i * lda, sizeof(double) * n);
    for (int k = 0; k < n; ++k) {
        d[k] = W[(int64_t)k * n + k];
        const int m = n - k - 1;
        if (m < 1) break;
        const double *x = W + (int64_t)(k + 1) * n + k;
        const double sigma = m > 1 ? wave_dot(x + n, n, x + n, n, m - 1) : wave_dot(x, n, x, n, 0);
        double tau, beta, scale;
        fid_reflector(x[0], sigma, &tau, &beta, &scale);
        for (int t = 0; t < m; ++t) v[k + 1 + t] = t == 0 ? 1.0 : x[(int64_t)t * n] * scale;
        e[k] = beta;
        if (k + 2 >= n || tau == 0.0) continue;
        for (int i = k + 1; i < n; ++i) p[i] = tau * wave_dot(W + (int64_t)i * n + k + 1, 1, v.data() + k + 1, 1, m);
        const double c = (0.5 * tau) * wave_dot(p.data() + k + 1, 1, v.data() + k + 1, 1, m);
        for (int i = k + 1; i < n; ++i) {
            const double vi = v[i], wi = p[i] - c * vi;
            double *row = W + (int64_t)i * n;
            for (int jj = k + 1; jj < n; ++jj) {
                const double vj = v[jj], wj = p[jj] - c * vj;
                row[jj] = row[jj] - (vi * wj + wi * vj);
            }
        }
    }
    return HOIG_OK;
}

extern "C" int hoig_sym_eigvals_f64_host(const double *A, int64_t lda, int n, double *lambda, int32_t *info) {
    if (!A || !lambda || !info || n < 1 || lda < n) return HOIG_EINVAL;
    std::vector<double> d((size_t)n), e((size_t)n);
    const int rc = hoig_sym_tridiag_f64_host(A, lda, n, d.data(), e.data());
    info[0] = rc;
    if (rc != HOIG_OK) return rc;
    return hoig_tridiag_eigvals_f64_host(d.data(), e.data(), n, lambda);
}
