// The host half of the sliced Wasserstein distance (swd.h, docs/swd.md): the workspace sizes, and CPU twins that run the inline
// functions of swd.h in the device's order -- every result is the device's, bit for bit (the sort is keys-only: any correct sort of
// the same integers gives the same bytes).  No HIP call; host memory only.  Built with -ffp-contract=off.
#include <algorithm>
#include <vector>

#include "swd.h"

namespace {

double butterfly(double *v) {
    double t[SWD_WAVE];
    for (int o = 32; o > 0; o >>= 1) {
        for (int l = 0; l < SWD_WAVE; ++l) t[l] = v[l] + v[l ^ o];
        memcpy(v, t, sizeof(t));
    }
    return v[0];
}

// a workgroup's sum of its threads' shares: four wave butterflies, then the wave sums first to last
template <class F>
double block_sum(F share) {
    double w[4];
    for (int wave = 0; wave < 4; ++wave) {
        double lane[SWD_WAVE];
        for (int l = 0; l < SWD_WAVE; ++l) lane[l] = share(wave * SWD_WAVE + l);
        w[wave] = butterfly(lane);
    }
    return ((w[0] + w[1]) + w[2]) + w[3];
}

double finish(const double *partials, int parts) {
    double lane[SWD_WAVE];
    for (int l = 0; l < SWD_WAVE; ++l) lane[l] = swd_lane_partials(partials, parts, l);
    return butterfly(lane);
}

template <class T>
void down(const T *in, int n, int H, int W, float *out) {
    const int Ho = H >> 1, Wo = W >> 1;
    for (int img = 0; img < n; ++img) {
        const T *src = in + (int64_t)img * H * W * 3;
        float *dst = out + (int64_t)img * Ho * Wo * 3;
        for (int yo = 0; yo < Ho; ++yo)
            for (int xo = 0; xo < Wo; ++xo)
                for (int c = 0; c < 3; ++c) {
                    float h[5];
                    for (int i = 0; i < 5; ++i) h[i] = swd_down_h(src, W, swd_mirror(2 * yo + i - 2, H), xo, c);
                    dst[((int64_t)yo * Wo + xo) * 3 + c] = swd_tap5(h[0], h[1], h[2], h[3], h[4]);
                }
    }
}

}  // namespace

extern "C" int hoig_swd_levels(int H, int W) { return swd_levels(H, W); }
extern "C" int hoig_sort_segments_lds_max(void) { return SWD_SORT_LDS_MAX; }
extern "C" int hoig_sort_segments_tile(void) { return SWD_SORT_TILE; }

extern "C" int64_t hoig_swd_descriptors_workspace_bytes(int n, int H, int W, int L) {
    if (n < 1 || !swd_shape_ok(H, W, L)) return HOIG_EINVAL;
    const int64_t bytes = swd_chain_floats(n, H, W, L) * (int64_t)sizeof(float);
    return bytes < 8 ? 8 : bytes;
}

extern "C" int64_t hoig_swd_channel_stats_workspace_bytes(int64_t rows) {
    if (rows < 1) return HOIG_EINVAL;
    return 6 * (int64_t)SWD_MAX_PARTS * (int64_t)sizeof(double);
}

extern "C" int64_t hoig_sort_segments_workspace_bytes(int64_t S, int64_t n) {
    if (S < 1 || n < 1 || n >= ((int64_t)1 << 31) || S * swd_sort_tiles(n) >= ((int64_t)1 << 31) || S * n >= ((int64_t)1 << 40))
        return HOIG_EINVAL;
    if (n <= SWD_SORT_LDS_MAX) return 8;
    return (S * n + S * 256 * swd_sort_tiles(n)) * (int64_t)sizeof(uint32_t);
}

extern "C" int64_t hoig_swd_sorted_l1_workspace_bytes(int64_t N) {
    if (N < 1) return HOIG_EINVAL;
    return (int64_t)swd_parts(N) * (int64_t)sizeof(double);
}

extern "C" int hoig_swd_positions_host(uint64_t seed, int set_id, int64_t first_index, int n, int H, int W, int L, int patches,
                                       int32_t *positions) {
    if (!positions || ((uintptr_t)positions & 3) || first_index < 0 || !swd_desc_ok(n, H, W, L, patches)) return HOIG_EINVAL;
    for (int img = 0; img < n; ++img)
        for (int l = 0; l < L; ++l)
            for (int p = 0; p < patches; ++p) {
                int y0, x0;
                swd_position(seed, set_id, l, first_index + img, p, H >> l, W >> l, &y0, &x0);
                int32_t *at = positions + (((int64_t)img * L + l) * patches + p) * 2;
                at[0] = y0, at[1] = x0;
            }
    return HOIG_OK;
}

extern "C" int hoig_swd_descriptors_u8_host(const uint8_t *u8, int n, int H, int W, int L, int patches, const int32_t *positions,
                                            float *out) {
    if (!u8 || !positions || !out || !swd_desc_ok(n, H, W, L, patches)) return HOIG_EINVAL;
    if (((uintptr_t)positions & 3) || ((uintptr_t)out & 3)) return HOIG_EINVAL;
    std::vector<float> chain((size_t)swd_chain_floats(n, H, W, L) + 1);
    for (int l = 0; l + 1 < L; ++l) {
        float *dst = chain.data() + swd_chain_floats(n, H, W, l + 1);
        if (l == 0)
            down(u8, n, H, W, dst);
        else
            down((const float *)(chain.data() + swd_chain_floats(n, H, W, l)), n, H >> l, W >> l, dst);
    }
    for (int l = 0; l < L; ++l) {
        const int Hl = H >> l, Wl = W >> l;
        for (int img = 0; img < n; ++img) {
            const float *next = l + 1 < L ? chain.data() + swd_chain_floats(n, H, W, l + 1) + (int64_t)img * (Hl >> 1) * (Wl >> 1) * 3 : nullptr;
            for (int p = 0; p < patches; ++p) {
                const int32_t *at = positions + (((int64_t)img * L + l) * patches + p) * 2;
                const int y0 = swd_clamp(at[0], Hl - SWD_PATCH), x0 = swd_clamp(at[1], Wl - SWD_PATCH);
                float *row = out + (((int64_t)l * n + img) * patches + p) * SWD_K;
                for (int e = 0; e < SWD_K; ++e) {
                    const int c = e / SWD_PLANE, y = y0 + (e % SWD_PLANE) / SWD_PATCH, x = x0 + e % SWD_PATCH;
                    row[e] = l == 0 ? swd_lap_at(u8 + (int64_t)img * H * W * 3, Hl, Wl, next, y, x, c)
                                    : swd_lap_at((const float *)(chain.data() + swd_chain_floats(n, H, W, l) + (int64_t)img * Hl * Wl * 3),
                                                 Hl, Wl, next, y, x, c);
                }
            }
        }
    }
    return HOIG_OK;
}

extern "C" int hoig_swd_channel_stats_f64_host(const float *desc, int64_t rows, double *stats, int32_t *status) {
    if (!desc || !stats || !status || rows < 1 || rows >= ((int64_t)1 << 32)) return HOIG_EINVAL;
    if (((uintptr_t)desc & 3) || ((uintptr_t)stats & 7)) return HOIG_EINVAL;
    const int64_t E = rows * SWD_PLANE;
    const int parts = swd_parts(E);
    int st = 0;
    std::vector<double> partials((size_t)parts);
    for (int c = 0; c < 3; ++c) {
        for (int part = 0; part < parts; ++part)
            partials[part] = block_sum([&](int t) { return swd_stat_thread(desc, E, c, part, t, 0.0, false); });
        const double sum = finish(partials.data(), parts);
        const double mean = sum / (double)E;
        for (int part = 0; part < parts; ++part)
            partials[part] = block_sum([&](int t) { return swd_stat_thread(desc, E, c, part, t, mean, true); });
        const double sd = sqrt(finish(partials.data(), parts) / (double)E);
        stats[2 * c] = mean, stats[2 * c + 1] = sd;
        if (!(sd > 0.0)) st |= 1 << c;
    }
    *status = st;
    return HOIG_OK;
}

extern "C" int hoig_swd_project_f32_host(const float *desc, int64_t rows, const double *stats, const float *dirs, int D, float *out) {
    if (!desc || !stats || !dirs || !out || rows < 1 || D < 1 || D > 65535 * SWD_PROJ_TILE) return HOIG_EINVAL;
    if (((uintptr_t)desc & 3) || ((uintptr_t)stats & 7) || ((uintptr_t)dirs & 3) || ((uintptr_t)out & 3)) return HOIG_EINVAL;
    if (rows * D >= ((int64_t)1 << 40)) return HOIG_EINVAL;
    std::vector<float> x(SWD_K), acc((size_t)D);
    for (int64_t r = 0; r < rows; ++r) {
        for (int k = 0; k < SWD_K; ++k) x[k] = swd_normalised(desc[r * SWD_K + k], stats[2 * (k / SWD_PLANE)], stats[2 * (k / SWD_PLANE) + 1]);
        std::fill(acc.begin(), acc.end(), 0.f);
        for (int k = 0; k < SWD_K; ++k) {
            const float *w = dirs + (int64_t)k * D;
            for (int d = 0; d < D; ++d) acc[d] = fmaf(x[k], w[d], acc[d]);
        }
        for (int d = 0; d < D; ++d) out[(int64_t)d * rows + r] = acc[d];
    }
    return HOIG_OK;
}

extern "C" int hoig_sort_segments_f32_host(float *keys, int64_t S, int64_t n, int32_t *status) {
    if (!swd_sort_ok(keys, S, n) || !status) return HOIG_EINVAL;
    int st = 0;
    std::vector<uint32_t> k((size_t)n);
    for (int64_t s = 0; s < S; ++s) {
        float *seg = keys + s * n;
        memcpy(k.data(), seg, (size_t)n * sizeof(uint32_t));
        for (int64_t i = 0; i < n; ++i) {
            if (swd_bits_nan(k[i])) st |= HOIG_SORT_NAN;
            k[i] = swd_key_encode(k[i]);
        }
        std::sort(k.begin(), k.end());
        for (int64_t i = 0; i < n; ++i) k[i] = swd_key_decode(k[i]);
        memcpy(seg, k.data(), (size_t)n * sizeof(uint32_t));
    }
    *status = st;
    return HOIG_OK;
}

extern "C" int hoig_swd_sorted_l1_f64_host(const float *a, const float *b, int64_t N, double *out) {
    if (!a || !b || !out || N < 1 || N >= ((int64_t)1 << 40)) return HOIG_EINVAL;
    if (((uintptr_t)a & 3) || ((uintptr_t)b & 3) || ((uintptr_t)out & 7)) return HOIG_EINVAL;
    const int parts = swd_parts(N);
    std::vector<double> partials((size_t)parts);
    for (int part = 0; part < parts; ++part) partials[part] = block_sum([&](int t) { return swd_l1_thread(a, b, N, part, t); });
    out[0] = finish(partials.data(), parts);
    return HOIG_OK;
}
