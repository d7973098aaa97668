// The host half of the discriminator augmentation (d_augment.h, docs/d_augment.md): CPU twins that run the shared inline functions in
// the order the kernels run them -- the same integer draws, the same doubles in the controller, the same fp32 roundings per element and
// the same order of additions in the two reductions, so the same bits.  No HIP call; host memory only.  Built with -ffp-contract=off.
#include "d_augment.h"

namespace {

// a workgroup's halving tree over its threads' sums
float tree(float *acc) {
    for (int s = DAUG_NT / 2; s > 0; s >>= 1)
        for (int t = 0; t < s; ++t) acc[t] = acc[t] + acc[t + s];
    return acc[0];
}

}  // namespace

extern "C" int hoig_daug_tick_host(uint64_t *state) {
    if (!daug_state_ok(state)) return HOIG_EINVAL;
    state[DAUG_STEP] += 1;
    return HOIG_OK;
}

extern "C" int hoig_daug_draw_host(const uint64_t *state, int site, int B, int H, int W, uint32_t *params) {
    if (!daug_draw_ok(state, site, B, H, W, params)) return HOIG_EINVAL;
    for (int i = 0; i < B; ++i) daug_draw_one(state, site, i, H, W, params + 8 * (int64_t)i);
    return HOIG_OK;
}

extern "C" int hoig_daug_adapt_host(uint64_t *state, const float *d_real, int64_t n) {
    if (!daug_state_ok(state) || !d_real || ((uintptr_t)d_real & 3) || n <= 0) return HOIG_EINVAL;
    int64_t pos = 0, neg = 0;
    for (int64_t i = 0; i < n; ++i) pos += d_real[i] > 0.f, neg += d_real[i] < 0.f;
    daug_adapt(state, pos, neg, n);
    return HOIG_OK;
}

extern "C" int hoig_daug_fwd_host(const float *img, const float *cond, const uint32_t *params, float *out, int B, int H, int W, int k,
                                  float *ws) {
    if (!daug_fwd_ok(img, cond, params, out, B, H, W, k, ws)) return HOIG_EINVAL;
    const int64_t npix = (int64_t)H * W, n = 3 * npix;
    const int parts = daug_parts((n + 3) / 4);
    float acc[DAUG_NT];
    for (int i = 0; i < B; ++i) {
        const DaugRec r = daug_rec(params, i);
        float mu = 0.f;
        if (r.flags & HOIG_DAUG_COLOR) {
            for (int part = 0; part < parts; ++part) {
                for (int t = 0; t < DAUG_NT; ++t) acc[t] = daug_mean_thread(img + i * n, n, part, t);
                ws[(int64_t)i * DAUG_MAX_PARTS + part] = tree(acc);
            }
            mu = daug_mu(ws + (int64_t)i * DAUG_MAX_PARTS, H, W, r.b);
        }
        float *o = out + i * npix * (3 + k);
        for (int64_t e = 0; e < npix * (3 + k); ++e) o[e] = daug_fwd_elem(img + i * n, cond + i * npix * k, r, mu, H, W, k, (int)e);
    }
    return HOIG_OK;
}

extern "C" int hoig_daug_bwd_host(const float *g, const uint32_t *params, float *dimg, int B, int H, int W, int k, float *ws) {
    if (!daug_bwd_ok(g, params, dimg, B, H, W, k, ws)) return HOIG_EINVAL;
    const int64_t npix = (int64_t)H * W;
    const int parts = daug_parts(npix);
    float acc[DAUG_NT];
    for (int i = 0; i < B; ++i) {
        const DaugRec r = daug_rec(params, i);
        const float *gs = g + i * npix * (3 + k);
        float cmu = 0.f;
        if (r.flags & HOIG_DAUG_COLOR) {
            for (int part = 0; part < parts; ++part) {
                for (int t = 0; t < DAUG_NT; ++t) acc[t] = daug_gsum_thread(gs, r, H, W, k, part, t);
                ws[(int64_t)i * DAUG_MAX_PARTS + part] = tree(acc);
            }
            cmu = daug_cmu(ws + (int64_t)i * DAUG_MAX_PARTS, H, W, r.k);
        }
        float *d = dimg + i * npix * 3;
        for (int64_t e = 0; e < npix * 3; ++e) d[e] = daug_bwd_elem(gs, r, cmu, H, W, k, (int)e);
    }
    return HOIG_OK;
}
