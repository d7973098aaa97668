// The host half of the opt-in style term (style_loss.h, docs/style_loss.md): the CPU twin.  It walks the images, tile pairs and pixel
// chunks of the Gram pass in the kernel's order -- every entry of a partial tile a std::fmaf chain from +0 over the chunk's pixels in
// ascending order, which is what the fp32 MFMA computes --, finishes every (image, tile pair) through the shared st_finish_lane, adds the
// lanes as the shared tree and ends through st_last_lane / st_last: the same roundings in the same order, so the same bits.  The feature
// gradient is a std::fmaf chain from +0 over the channels in ascending order.  No HIP call; host memory only.  Built with
// -ffp-contract=off.
#include <cmath>
#include <vector>

#include "style_loss.h"

extern "C" int hoig_style_gram_host(const float *fx, const float *fy, int N, int P, int C, double scale, float *S, float *term,
                                    float *report, double *gram) {
    st_args a;
    const int rc = st_pack(fx, fy, N, P, C, scale, S, term, report, gram, &a);
    if (rc != HOIG_OK) return rc;
    std::vector<float> partials((size_t)2 * N * a.pairs * a.chunks * (ST_T * ST_T), 0.f);
    std::vector<float> acc((size_t)ST_T * ST_T);
    for (int img = 0; img < 2 * N; ++img) {
        const float *F = st_image(a, img);
        for (int pair = 0; pair < a.pairs; ++pair) {
            int ti, tj;
            st_pair(a.tiles, pair, &ti, &tj);
            const int ci = ti * ST_T, cj = tj * ST_T;
            const int ni = C - ci < ST_T ? C - ci : ST_T, nj = C - cj < ST_T ? C - cj : ST_T;
            for (int chunk = 0; chunk < a.chunks; ++chunk) {
                const int p0 = chunk * ST_K, p1 = p0 + ST_K < P ? p0 + ST_K : P;
                for (size_t k = 0; k < acc.size(); ++k) acc[k] = 0.f;
                for (int p = p0; p < p1; ++p) {
                    const float *row = F + (int64_t)p * C;
                    for (int i = 0; i < ni; ++i) {
                        const float x = row[ci + i];
                        float *ai = acc.data() + i * ST_T;
                        for (int j = 0; j < nj; ++j) ai[j] = std::fmaf(x, row[cj + j], ai[j]);
                    }
                }
                float *out = partials.data() + (((size_t)img * a.pairs + pair) * a.chunks + chunk) * (ST_T * ST_T);
                for (size_t k = 0; k < acc.size(); ++k) out[k] = acc[k];
            }
        }
    }
    std::vector<double> sums((size_t)N * a.pairs, 0.0), lanes(ST_NT);
    for (int n = 0; n < N; ++n)
        for (int pair = 0; pair < a.pairs; ++pair) {
            int ti, tj;
            st_pair(a.tiles, pair, &ti, &tj);
            for (int t = 0; t < ST_NT; ++t) lanes[t] = st_finish_lane(a, partials.data(), n, pair, ti, tj, t);
            sums[(size_t)n * a.pairs + pair] = st_tile_sum(st_tree(lanes.data(), ST_NT), ti, tj);
        }
    for (int t = 0; t < 64; ++t) lanes[t] = st_last_lane(a, sums.data(), t);
    st_last(a, st_tree(lanes.data(), 64));
    return HOIG_OK;
}

extern "C" int hoig_style_dfeat_host(const float *fx, const float *S, int N, int P, int C, float *dfx) {
    const int rc = st_check_dfeat(fx, S, N, P, C, dfx);
    if (rc != HOIG_OK) return rc;
    for (int n = 0; n < N; ++n) {
        const float *Sn = S + (int64_t)n * C * C;
        for (int p = 0; p < P; ++p) {
            const float *row = fx + ((int64_t)n * P + p) * C;
            float *out = dfx + ((int64_t)n * P + p) * C;
            for (int j = 0; j < C; ++j) out[j] = 0.f;
            for (int k = 0; k < C; ++k) {
                const float x = row[k];
                const float *sk = Sn + (int64_t)k * C;
                for (int j = 0; j < C; ++j) out[j] = std::fmaf(x, sk[j], out[j]);
            }
        }
    }
    return HOIG_OK;
}
