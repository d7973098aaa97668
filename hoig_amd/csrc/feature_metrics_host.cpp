// The host half of the feature-space metrics (feature_metrics.h, docs/feature_metrics.md): the workspace sizes, and CPU twins that
// walk the device's tiles, lanes and reductions with the shared per-lane code.  A dot product is summed in order of k here; the MFMA's
// order inside a k-step of four is not reproduced, so a tile value is close to the device's, not equal -- every reduction of tile
// values is the device's own.  No HIP call; host memory only.  Built with -ffp-contract=off.
#include <string.h>

#include <vector>

#include "feature_metrics.h"

namespace {

double fm_butterfly(double *v) {
    double t[FID_WAVE];
    for (int o = 32; o > 0; o >>= 1) {
        for (int l = 0; l < FID_WAVE; ++l) t[l] = v[l] + v[l ^ o];
        memcpy(v, t, sizeof(t));
    }
    return v[0];
}

// rows of fp32 [n][D] as doubles, minus the pivot; the status of a non-finite feature
void widen(const float *X, int n, int D, const double *pivot, std::vector<double> *out, int *status) {
    out->resize((size_t)n * D);
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < D; ++c) {
            if (!fid_finite((double)X[(size_t)i * D + c])) *status |= FM_STATUS_NONFINITE;
            (*out)[(size_t)i * D + c] = fid_operand(X, (int64_t)i * D + c, 1, pivot, c);
        }
}

double dot(const double *a, const double *b, int D) {
    double s = 0.0;
    for (int k = 0; k < D; ++k) s = s + a[k] * b[k];
    return s;
}

void sqnorms(const float *X, int n, int D, const double *pivot, std::vector<double> *out) {
    out->resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        double part[FID_WAVE];
        for (int l = 0; l < FID_WAVE; ++l) part[l] = fm_lane_sqnorm(X + (size_t)i * D, D, pivot, l);
        (*out)[i] = fm_butterfly(part);
    }
}

// the 64 x 64 tile of dot products of the rows prow[0 .. 64) and qrow[0 .. 64) (nullptr: zeros), then one workgroup's reduction of it
double kid_tile(const double *const *prow, const double *const *qrow, int D, int ti, int tj, int term, int m, double gamma, double coef0,
                int degree) {
    static thread_local double tile[FM_TILE][FM_TILE];
    for (int r = 0; r < FM_TILE; ++r)
        for (int c = 0; c < FM_TILE; ++c) tile[r][c] = (prow[r] && qrow[c]) ? dot(prow[r], qrow[c], D) : 0.0;
    double wsum[FM_WAVES];
    for (int wave = 0; wave < FM_WAVES; ++wave) {
        double part[FID_WAVE];
        for (int lane = 0; lane < FID_WAVE; ++lane) {
            double v[16];
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j)
                    for (int reg = 0; reg < 4; ++reg)
                        v[(i * 2 + j) * 4 + reg] = tile[fm_lane_row(wave, lane, i, reg)][fm_lane_col(wave, lane, j)];
            part[lane] = fm_kid_lane(v, wave, lane, ti, tj, term, m, gamma, coef0, degree);
        }
        wsum[wave] = fm_butterfly(part);
    }
    return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

}  // namespace

extern "C" int64_t hoig_kid_workspace_bytes(int S, int m) {
    if (S < 1 || S > 65535 || m < 2) return HOIG_EINVAL;
    const int64_t nt = fm_tiles(m);
    return (int64_t)S * 3 * nt * nt * (int64_t)sizeof(double);
}

extern "C" int64_t hoig_knn_workspace_bytes(int n) {
    if (n < 2) return HOIG_EINVAL;
    return ((int64_t)n + (int64_t)fm_chunks(fm_tiles(n)) * n * FM_KMAX) * (int64_t)sizeof(double);
}

extern "C" int64_t hoig_manifold_hits_workspace_bytes(int nx, int ny) {
    if (nx < 1 || ny < 1) return HOIG_EINVAL;
    return ((int64_t)nx + ny) * (int64_t)sizeof(double) + (int64_t)fm_chunks(fm_tiles(nx)) * ny * (int64_t)sizeof(int32_t);
}

extern "C" int hoig_kid_finish_f64_host(const double *partials, int S, int m, const int32_t *status, double *out) {
    if (!partials || !out || S < 1 || S > 65535 || m < 2) return HOIG_EINVAL;
    const int nt = fm_tiles(m);
    const bool refused = status && *status != 0;
    for (int s = 0; s < S; ++s) {
        double sums[3];
        for (int term = 0; term < 3; ++term) {
            double part[FID_WAVE];
            for (int l = 0; l < FID_WAVE; ++l) part[l] = fm_kid_lane_finish(partials + ((int64_t)s * 3 + term) * nt * nt, term, nt, l);
            sums[term] = fm_butterfly(part);
        }
        out[4 * s + 0] = refused ? NAN : sums[0];
        out[4 * s + 1] = refused ? NAN : sums[1];
        out[4 * s + 2] = refused ? NAN : sums[2];
        out[4 * s + 3] = refused ? NAN : fm_mmd2(sums[0], sums[1], sums[2], m);
    }
    return HOIG_OK;
}

extern "C" int hoig_kid_poly_f64_host(const float *X, int nx, const float *Y, int ny, int D, const int32_t *ix, const int32_t *iy, int S,
                                      int m, double gamma, double coef0, int degree, double *out, int32_t *status) {
    if (!X || !Y || !ix || !iy || !out || !status || nx < 1 || ny < 1 || D < 1 || degree < 1 || degree > 4) return HOIG_EINVAL;
    if (S < 1 || S > 65535 || m < 2) return HOIG_EINVAL;
    int st = 0, clamped = 0;
    std::vector<double> xd, yd;
    widen(X, nx, D, nullptr, &xd, &st);
    widen(Y, ny, D, nullptr, &yd, &st);
    const int nt = fm_tiles(m);
    std::vector<double> partials((size_t)S * 3 * nt * nt, 0.0);
    const double *prow[FM_TILE], *qrow[FM_TILE];
    for (int s = 0; s < S; ++s)
        for (int term = 0; term < 3; ++term) {
            const std::vector<double> &P = term == FM_TERM_YY ? yd : xd, &Q = term == FM_TERM_XX ? xd : yd;
            const int np = term == FM_TERM_YY ? ny : nx, nq = term == FM_TERM_XX ? nx : ny;
            const int32_t *tp = (term == FM_TERM_YY ? iy : ix) + (int64_t)s * m, *tq = (term == FM_TERM_XX ? ix : iy) + (int64_t)s * m;
            for (int ti = 0; ti < nt; ++ti)
                for (int tj = 0; tj < nt; ++tj) {
                    if (!fm_kid_slot_runs(term, ti, tj)) continue;
                    for (int r = 0; r < FM_TILE; ++r) {
                        const int pi = ti * FM_TILE + r, pj = tj * FM_TILE + r;
                        prow[r] = pi < m ? P.data() + (size_t)fm_clamp_index(tp[pi], np, &clamped) * D : nullptr;
                        qrow[r] = pj < m ? Q.data() + (size_t)fm_clamp_index(tq[pj], nq, &clamped) * D : nullptr;
                    }
                    partials[((size_t)s * 3 + term) * nt * nt + ti * nt + tj] = kid_tile(prow, qrow, D, ti, tj, term, m, gamma, coef0, degree);
                }
        }
    *status = st | (clamped ? FM_STATUS_CLAMPED : 0);
    return hoig_kid_finish_f64_host(partials.data(), S, m, status, out);
}

extern "C" int hoig_knn_radius_f64_host(const float *X, int n, int D, const double *pivot, int k, double *radius, int32_t *status) {
    if (!X || !radius || !status || n < 2 || D < 1 || k < 1 || k > FM_KMAX || k > n - 1) return HOIG_EINVAL;
    int st = 0;
    std::vector<double> xd, norms;
    widen(X, n, D, pivot, &xd, &st);
    sqnorms(X, n, D, pivot, &norms);
    *status = st;
    for (int i = 0; i < n; ++i) {
        double best[FM_KMAX];
        for (int s = 0; s < FM_KMAX; ++s) best[s] = HUGE_VAL;
        for (int j = 0; j < n; ++j)
            if (j != i) fm_insert(best, fm_dist2(norms[i], norms[j], dot(xd.data() + (size_t)i * D, xd.data() + (size_t)j * D, D)));
        radius[i] = st != 0 ? NAN : fm_pick(best, k);
    }
    return HOIG_OK;
}

extern "C" int hoig_manifold_hits_f64_host(const float *X, int nx, const double *radius, const float *Y, int ny, int D,
                                           const double *pivot, int32_t *hits, int32_t *status) {
    if (!X || !radius || !Y || !hits || !status || nx < 1 || ny < 1 || D < 1) return HOIG_EINVAL;
    int st = 0;
    std::vector<double> xd, yd, xn, yn;
    widen(X, nx, D, pivot, &xd, &st);
    widen(Y, ny, D, pivot, &yd, &st);
    sqnorms(X, nx, D, pivot, &xn);
    sqnorms(Y, ny, D, pivot, &yn);
    *status = st;
    for (int j = 0; j < ny; ++j) {
        int total = 0;
        for (int i = 0; i < nx; ++i)
            if (fm_dist2(xn[i], yn[j], dot(xd.data() + (size_t)i * D, yd.data() + (size_t)j * D, D)) <= radius[i]) ++total;
        hits[j] = total;
    }
    return HOIG_OK;
}
