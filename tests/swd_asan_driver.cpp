// The *_host twins of the sliced Wasserstein distance (hoig_amd/csrc/swd_host.cpp) in a program of its own, for a host
// AddressSanitizer / UBSan build (tests/test_swd_cpu.py): every buffer is a heap block of exactly its size, so a read or write past an
// end is a report.
//   swd_asan_driver H W L n1 n2 ..  ->  "rc"; then as hex doubles: the sum of every level's descriptor rows, the six statistics of the
//   last level, sum |a - b| of its two sorted projections, their first and last value; then one 0 / 1 per sort size n (two segments of
//   n keys against std::sort).
// Two images, three patches, seed 11, set 1, first image index 4; pixel (i, y, x, c) = (53 i + 31 y + 17 x + 101 c + 9 ((x y) % 7)) % 256;
// direction j of component k: ((7 k + 3 j) % 11 - 5) / 8 (the test restates all of it in numpy).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "hoig_kernels.h"

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    const int H = atoi(argv[1]), W = atoi(argv[2]), L = atoi(argv[3]), n = 2, patches = 3, D = 2;
    std::vector<uint8_t> u8((size_t)n * H * W * 3);
    for (int i = 0; i < n; ++i)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                for (int c = 0; c < 3; ++c) u8[(((size_t)i * H + y) * W + x) * 3 + c] = (uint8_t)((i * 53 + y * 31 + x * 17 + c * 101 + ((x * y) % 7) * 9) % 256);
    const int64_t rows = (int64_t)n * patches;
    std::vector<int32_t> pos((size_t)n * L * patches * 2), status(1, -1);
    std::vector<float> desc((size_t)L * rows * HOIG_SWD_K), dirs((size_t)HOIG_SWD_K * D), proj((size_t)D * rows);
    std::vector<double> stats(6), l1(1);
    for (int k = 0; k < HOIG_SWD_K; ++k)
        for (int j = 0; j < D; ++j) dirs[(size_t)k * D + j] = (float)((k * 7 + j * 3) % 11 - 5) * 0.125f;
    int rc = hoig_swd_positions_host(11, 1, 4, n, H, W, L, patches, pos.data());
    if (rc == 0) rc = hoig_swd_descriptors_u8_host(u8.data(), n, H, W, L, patches, pos.data(), desc.data());
    const float *last = desc.data() + (size_t)(L - 1) * rows * HOIG_SWD_K;
    if (rc == 0) rc = hoig_swd_channel_stats_f64_host(last, rows, stats.data(), status.data());
    if (rc == 0) rc = hoig_swd_project_f32_host(last, rows, stats.data(), dirs.data(), D, proj.data());
    if (rc == 0) rc = hoig_sort_segments_f32_host(proj.data(), D, rows, status.data());
    if (rc == 0) rc = hoig_swd_sorted_l1_f64_host(proj.data(), proj.data() + rows, rows, l1.data());
    printf("%d\n", rc);
    for (int l = 0; l < L; ++l) {
        double s = 0.0;
        for (int64_t e = 0; e < rows * HOIG_SWD_K; ++e) s += (double)desc[(size_t)l * rows * HOIG_SWD_K + e];
        printf("%a ", s);
    }
    for (int e = 0; e < 6; ++e) printf("%a ", stats[e]);
    printf("%a %a %a\n", l1[0], (double)proj[0], (double)proj[(size_t)D * rows - 1]);
    for (int a = 4; a < argc; ++a) {
        const int64_t m = atoll(argv[a]);
        float *keys = (float *)malloc((size_t)(2 * m) * sizeof(float));      // exactly 2 m floats
        if (!keys) return 3;
        uint32_t lcg = 12345u + (uint32_t)m;
        for (int64_t i = 0; i < 2 * m; ++i) {
            lcg = lcg * 1664525u + 1013904223u;
            keys[i] = (float)(int32_t)(lcg >> 8) * 0.001f - 8000.f;
        }
        std::vector<float> want(keys, keys + 2 * m);
        std::sort(want.begin(), want.begin() + m);
        std::sort(want.begin() + m, want.end());
        int ok = hoig_sort_segments_f32_host(keys, 2, m, status.data()) == 0 && status[0] == 0;
        for (int64_t i = 0; i < 2 * m; ++i) ok = ok && keys[i] == want[(size_t)i];
        printf("%d ", ok);
        free(keys);
    }
    printf("\n");
    return 0;
}
