// Runs the CPU twins of the region scores (hoig_amd/csrc/region_metrics_host.cpp) -- statistics, boxes, the tap tables and the crops --
// on the cases given on the command line, every buffer in a heap block of exactly its size: built with -fsanitize=address by
// tests/test_region_metrics_cpu.py, so that a read or write one byte outside a buffer aborts the run.  Arguments: N H W S per case.
// Content: byte i of gen = (i * 2654435761 + H * 31 + W) >> 24, of gt the same with + 7 (uint32 arithmetic); image n is labelled 1 on
// x in [W / 8 + n, W / 2), y in [H / 8, H / 2 + n) and 2 on x in [W / 2, W - n), y in [H / 2, H); two regions, min_pixels 1.
// Prints one line per case: "<the four return codes and the status> <FNV-1a of stats> <of boxes> <of the tables> <of gen's crops>".
#include <stdio.h>
#include <stdlib.h>

#include "hoig_kernels.h"

static uint32_t fnv(const void *p, size_t n) {
    const uint8_t *b = (const uint8_t *)p;
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 16777619u;
    return h;
}

int main(int argc, char **argv) {
    if (argc < 5 || (argc - 1) % 4) return 2;
    const int R = 2;
    for (int a = 1; a + 3 < argc; a += 4) {
        const int N = atoi(argv[a]), H = atoi(argv[a + 1]), W = atoi(argv[a + 2]), S = atoi(argv[a + 3]);
        const size_t npix = (size_t)N * H * W, nbytes = npix * 3;
        uint8_t *gen = (uint8_t *)malloc(nbytes), *gt = (uint8_t *)malloc(nbytes), *lab = (uint8_t *)malloc(npix);
        for (size_t i = 0; i < nbytes; ++i) {
            gen[i] = (uint8_t)(((uint32_t)i * 2654435761u + (uint32_t)(H * 31 + W)) >> 24);
            gt[i] = (uint8_t)(((uint32_t)i * 2654435761u + (uint32_t)(H * 31 + W + 7)) >> 24);
        }
        for (int n = 0; n < N; ++n)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    uint8_t v = 0;
                    if (x >= W / 8 + n && x < W / 2 && y >= H / 8 && y < H / 2 + n) v = 1;
                    else if (x >= W / 2 && x < W - n && y >= H / 2) v = 2;
                    lab[((size_t)n * H + y) * W + x] = v;
                }
        const size_t stats_bytes = sizeof(int64_t) * (size_t)N * (R + 1) * 8, boxes_bytes = sizeof(int32_t) * (size_t)N * R * 4;
        const size_t dst_bytes = (size_t)R * N * S * S * 3;
        int64_t *stats = (int64_t *)malloc(stats_bytes);
        int32_t *status = (int32_t *)malloc(sizeof(int32_t)), *boxes = (int32_t *)malloc(boxes_bytes);
        uint8_t *dst = (uint8_t *)malloc(dst_bytes);
        const int rc0 = hoig_region_stats_u8_host(gen, gt, lab, N, H, W, R, stats, status);
        const int rc1 = hoig_region_boxes_host(stats, N, H, W, R, 1, boxes);
        const int64_t tb = hoig_region_tables_bytes(H < W ? H : W, S);
        if (tb < 0) return 3;
        int32_t *tables = (int32_t *)malloc((size_t)tb);
        const int rc2 = hoig_region_tables(H < W ? H : W, S, tables);
        const uint32_t ht = fnv(tables, (size_t)tb);
        free(tables);
        const int rc3 = hoig_region_crop_resize_u8_host(gen, N, H, W, boxes, R, S, dst);
        printf("%d%d%d%d%d %u %u %u %u\n", rc0, rc1, rc2, rc3, status[0], fnv(stats, stats_bytes), fnv(boxes, boxes_bytes), ht,
               fnv(dst, dst_bytes));
        free(dst), free(boxes), free(status), free(stats), free(lab), free(gt), free(gen);
    }
    return 0;
}
