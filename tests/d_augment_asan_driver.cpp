// The hoig_daug_*_host twins (hoig_amd/csrc/d_augment_host.cpp) in a program of its own, for a host AddressSanitizer / UBSan build
// (tests/test_d_augment_cpu.py): every buffer is a heap block of exactly its size, so a read or write past an end is a report.
//   d_augment_asan_driver B H W k  ->  "rc", then the 8 B record words (hex), the B H W (3 + k) outputs and the 3 B H W image gradients
//   as hex doubles, then the state's step, its p (hex double) and its three counters after one tick and three adapt calls
// img[i] = (((i * 17 + 3) % 29) - 14) / 16, cond[i] = (((i * 37 + 11) % 41) - 20) / 32, g[i] = (((i * 13 + 5) % 23) - 11) / 16 (the test
// restates them in numpy).  The records are drawn at step 5, site 1, p = 1, every family, seed 1, rank 2.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hoig_kernels.h"

template <typename T>
static T *block(size_t n) {
    void *p = nullptr;
    if (posix_memalign(&p, 16, n ? n * sizeof(T) : 1)) exit(3);
    return (T *)p;
}

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const int B = atoi(argv[1]), H = atoi(argv[2]), W = atoi(argv[3]), k = atoi(argv[4]);
    const bool ok = B > 0 && H > 0 && W > 0 && k > 0;
    const size_t npix = ok ? (size_t)B * H * W : 0;
    uint64_t *state = block<uint64_t>(HOIG_DAUG_STATE_WORDS);
    memset(state, 0, HOIG_DAUG_STATE_WORDS * sizeof(uint64_t));
    const double one = 1.0, target = 0.6, inc = 0.25;
    state[0] = 4;
    memcpy(&state[1], &one, 8);
    state[6] = 1, state[7] = 2;
    memcpy(&state[8], &target, 8);
    state[9] = 2;
    memcpy(&state[10], &inc, 8);
    state[11] = HOIG_DAUG_COLOR | HOIG_DAUG_TRANSLATION | HOIG_DAUG_CUTOUT;
    float *img = block<float>(npix * 3), *cond = block<float>(npix * k), *out = block<float>(npix * (3 + k));
    float *g = block<float>(npix * (3 + k)), *dimg = block<float>(npix * 3), *ws = block<float>((size_t)(ok ? B : 0) * HOIG_DAUG_MAX_PARTS);
    uint32_t *params = block<uint32_t>((size_t)(ok ? B : 0) * 8);
    for (size_t i = 0; i < npix * 3; ++i) img[i] = (float)((int)((i * 17 + 3) % 29) - 14) * 0.0625f;
    for (size_t i = 0; i < npix * k; ++i) cond[i] = (float)((int)((i * 37 + 11) % 41) - 20) * 0.03125f;
    for (size_t i = 0; i < npix * (3 + k); ++i) g[i] = (float)((int)((i * 13 + 5) % 23) - 11) * 0.0625f;
    int rc = hoig_daug_tick_host(state);
    if (rc == 0) rc = hoig_daug_draw_host(state, 1, B, H, W, params);
    if (rc == 0) rc = hoig_daug_fwd_host(img, cond, params, out, B, H, W, k, ws);
    if (rc == 0) rc = hoig_daug_bwd_host(g, params, dimg, B, H, W, k, ws);
    for (int j = 0; j < 3 && rc == 0; ++j) rc = hoig_daug_adapt_host(state, g, (int64_t)(npix * (3 + k)));
    printf("%d\n", rc);
    if (rc == 0) {
        for (int i = 0; i < B * 8; ++i) printf("%x\n", params[i]);
        for (size_t i = 0; i < npix * (3 + k); ++i) printf("%a\n", (double)out[i]);
        for (size_t i = 0; i < npix * 3; ++i) printf("%a\n", (double)dimg[i]);
        double p;
        memcpy(&p, &state[1], 8);
        printf("%llu %a %lld %lld %lld\n", (unsigned long long)state[0], p, (long long)state[2], (long long)state[3], (long long)state[5]);
    }
    free(state), free(img), free(cond), free(out), free(g), free(dimg), free(ws), free(params);
    return 0;
}
