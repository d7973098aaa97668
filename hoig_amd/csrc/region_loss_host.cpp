// The host half of the opt-in region reconstruction term (region_loss.h, docs/region_loss.md): the CPU twin.  It counts the labels (integer
// sums: any order gives the kernel's), takes V_r and the scales through the shared rl_scales, walks the images, tiles and lanes of the
// value-and-gradient pass in the kernel's order through the shared rl_lane, adds every workgroup's lanes as the shared tree, and
// finishes through rl_row / rl_finish: the same roundings in the same order, so the same bits.  No HIP call; host memory only.  Built
// with -ffp-contract=off.
#include <vector>

#include "region_loss.h"

namespace {

template <int RT>
void run(const rl_args &a) {
    const int R1 = a.R + 1, R2 = a.R + 2;
    std::vector<int32_t> counts((size_t)a.N * R1, 0), V(R1, 0);
    int badmax = 0;
    for (int i = 0; i < a.N; ++i)
        for (int p = 0; p < a.HW; ++p) {
            const int l = a.labels[(int64_t)i * a.HW + p];
            if (l <= a.R)
                counts[(size_t)i * R1 + l] += 1;
            else if (l > badmax)
                badmax = l;
        }
    std::vector<float> scales((size_t)a.N * R1, 0.f);
    rl_scales(a, [&](int k) { return counts[k]; }, badmax, scales.data(), V.data());

    std::vector<double> partials((size_t)a.N * a.tiles * R2, 0.0), rows((size_t)a.N * R2, 0.0);
    std::vector<double> lanes((size_t)RL_NT * (RT + 2));
    double(*acc)[RT + 2] = reinterpret_cast<double(*)[RT + 2]>(lanes.data());
    for (int i = 0; i < a.N; ++i) {
        float sc[RT + 1];
        for (int r = 0; r <= RT; ++r) sc[r] = r <= a.R ? scales[(size_t)i * R1 + r] : 0.f;
        for (int w = 0; w < a.tiles; ++w) {
            for (int t = 0; t < RL_NT; ++t) {
                for (int j = 0; j < RT + 2; ++j) acc[t][j] = 0.0;
                rl_lane<RT>(a, i, w, t, false, sc, acc[t]);
            }
            rl_tree<RT>(acc);
            double *out = partials.data() + ((size_t)i * a.tiles + w) * R2;
            for (int j = 0; j <= a.R; ++j) out[j] = acc[0][j];
            out[R1] = acc[0][RT + 1];
        }
    }
    for (int rho = 0; rho < a.N * R2; ++rho) rows[rho] = rl_row(a, partials.data(), rho);
    rl_finish(a, counts.data(), V.data(), rows.data());
}

}  // namespace

extern "C" int hoig_region_loss_host(const float *pred, const float *target, const uint8_t *labels, int N, int H, int W, int C, int R,
                                     const double *lambda, double lambda_all, int min_pixels, float *dpred, float *term, float *terms_r,
                                     float *term_all, int32_t *counts_out, int32_t *status) {
    rl_args a;
    if (!rl_pack(pred, target, labels, N, H, W, C, R, lambda, lambda_all, min_pixels, dpred, term, terms_r, term_all, counts_out, status, &a))
        return HOIG_EINVAL;
    if (R <= 2)
        run<2>(a);
    else
        run<RL_MAXR>(a);
    return HOIG_OK;
}
