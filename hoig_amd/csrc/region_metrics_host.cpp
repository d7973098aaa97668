// Host half of the region scores (region_metrics.h): the tap tables of every source side, the workspace size and the CPU twins of
// the kernels.  Plain C++ with no HIP call (it also builds on its own under a host sanitizer).
#include <string.h>
#include <vector>

#include "region_metrics.h"

extern "C" int hoig_region_stats_u8_host(const uint8_t *gen, const uint8_t *gt, const uint8_t *labels, int N, int H, int W, int R,
                                         int64_t *stats, int32_t *status) {
    if (!gen || !gt || !labels || !stats || !status || !region_stats_ok(N, H, W, R)) return HOIG_EINVAL;
    int bad = 0;
    for (int n = 0; n < N; ++n) {
        const int64_t base = (int64_t)n * H * W;
        region_rows<int64_t> a;
        region_rows_clear(a, H, W);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const int64_t i = base + (int64_t)y * W + x;
                region_rows_add(a, R, gen + i * 3, gt + i * 3, labels[i], x, y);
            }
        for (int r = 0; r <= R; ++r) {
            int64_t *row = stats + ((int64_t)n * (R + 1) + r) * HOIG_REGION_ROW;
            row[0] = a.cnt[r], row[1] = a.ad[r], row[2] = a.sq[r];
            row[3] = a.x0[r], row[4] = a.y0[r], row[5] = a.x1[r], row[6] = a.y1[r], row[7] = 0;
        }
        if (a.bad > bad) bad = a.bad;
    }
    *status = region_status_word(bad);
    return HOIG_OK;
}

extern "C" int hoig_region_boxes_host(const int64_t *stats, int N, int H, int W, int R, int min_pixels, int32_t *boxes) {
    if (!stats || !boxes || !region_stats_ok(N, H, W, R) || min_pixels < 0) return HOIG_EINVAL;
    for (int n = 0; n < N; ++n)
        for (int r = 0; r < R; ++r)
            region_box(stats + ((int64_t)n * (R + 1) + r + 1) * HOIG_REGION_ROW, H, W, min_pixels, boxes + ((int64_t)n * R + r) * 4);
    return HOIG_OK;
}

extern "C" int64_t hoig_region_tables_bytes(int max_side, int S) {
    if (!pil_side_ok(max_side) || !region_size_ok(S)) return HOIG_EINVAL;
    return region_tables_words(max_side, S) * (int64_t)sizeof(int32_t);
}

extern "C" int hoig_region_tables(int max_side, int S, int32_t *tables) {
    if (!tables || !pil_side_ok(max_side) || !region_size_ok(S)) return HOIG_EINVAL;
    region_tables_build(max_side, S, tables);
    return HOIG_OK;
}

extern "C" int64_t hoig_region_crop_workspace_bytes(int N, int H, int W, int R, int S) {
    if (!region_stats_ok(N, H, W, R) || !region_size_ok(S)) return HOIG_EINVAL;
    return (int64_t)R * N * region_mid_stride(H, W, S);
}

extern "C" int hoig_region_crop_resize_u8_host(const uint8_t *src, int N, int H, int W, const int32_t *boxes, int R, int S, uint8_t *dst) {
    if (!src || !boxes || !dst || !region_stats_ok(N, H, W, R) || !region_size_ok(S)) return HOIG_EINVAL;
    const int max_side = H < W ? H : W;
    const int64_t per_crop = (int64_t)S * S * 3;
    // the tables of one side at a time, in the layout the kernels read: a header up to that side, then its rows
    std::vector<int32_t> tables;
    std::vector<uint8_t> mid;
    for (int r = 0; r < R; ++r)
        for (int n = 0; n < N; ++n) {
            const int32_t *box = boxes + ((int64_t)n * R + r) * 4;
            uint8_t *out = dst + ((int64_t)r * N + n) * per_crop;
            memset(out, 0, (size_t)per_crop);
            const int side = box[2];
            if (side < 1 || side > max_side) continue;
            const int ksize = pil_ksize(side, S);
            const int64_t head = 2 * ((int64_t)side + 1);
            tables.assign((size_t)(head + (int64_t)S * (PIL_ROW_HEAD + ksize)), 0);
            tables[0] = side, tables[1] = S;
            tables[2 * side] = (int32_t)head, tables[2 * side + 1] = ksize;
            pil_build_table(side, S, tables.data() + head);
            if (!region_box_usable(box, H, W, S, tables.data())) continue;
            const int total = side * S * 3;
            mid.resize((size_t)total);
            const uint8_t *img = src + (int64_t)n * H * W * 3;
            for (int e = 0; e < total; ++e) mid[e] = region_crop_h_byte(img, W, box, S, tables.data(), e);
            for (int e = 0; e < (int)per_crop; ++e) out[e] = region_crop_v_byte(mid.data(), box, S, tables.data(), e);
        }
    return HOIG_OK;
}
