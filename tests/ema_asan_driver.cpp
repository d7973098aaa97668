// hoig_ema_tick_host / hoig_ema_update_host (hoig_amd/csrc/ema_host.cpp) in a program of its own, for a host AddressSanitizer / UBSan
// build (tests/test_ema_cpu.py): every buffer is a heap block of exactly its size, so a read or write past an end is a report.
//   ema_asan_driver n K  ->  "rc", then the count and the last weight as hex doubles, then the n averages as hex doubles
// ema[i] = (((i * 17 + 3) % 29) - 14) / 16; the weights of update k: (((i * 37 + 11 + 13 * k) % 41) - 20) / 32 (the test restates both
// in numpy).  Decay 0.999 with warm-up.  After the K updates one more call under a guard with skip = 1, which must change nothing.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "hoig_kernels.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const int64_t n = atoll(argv[1]);
    const int K = atoi(argv[2]);
    const size_t len = (size_t)(n > 0 ? n : 0);
    // (16-byte aligned blocks of exactly n floats: the entry points refuse any other alignment)
    float *ema = nullptr, *param = nullptr;
    if (posix_memalign((void **)&ema, 16, len ? len * sizeof(float) : 1) || posix_memalign((void **)&param, 16, len ? len * sizeof(float) : 1)) return 3;
    std::vector<float> derived(1, 0.f), guard(2);
    std::vector<double> state{0.999, 1.0, 0.0};
    for (int64_t i = 0; i < n; ++i) ema[i] = (float)(((i * 17 + 3) % 29) - 14) * 0.0625f;
    int rc = 0;
    guard[0] = 1.f, guard[1] = 0.f;
    for (int k = 0; k < K && rc == 0; ++k) {
        for (int64_t i = 0; i < n; ++i) param[i] = (float)(((i * 37 + 11 + 13 * k) % 41) - 20) * 0.03125f;
        rc = hoig_ema_tick_host(state.data(), derived.data(), k & 1 ? guard.data() : nullptr);
        if (rc == 0) rc = hoig_ema_update_host(ema, param, n, derived.data(), k & 1 ? guard.data() : nullptr);
    }
    guard[1] = 1.f;
    if (rc == 0) rc = hoig_ema_tick_host(state.data(), derived.data(), guard.data());
    if (rc == 0) rc = hoig_ema_update_host(ema, param, n, derived.data(), guard.data());
    printf("%d\n%a %a\n", rc, state[2], (double)derived[0]);
    for (int64_t i = 0; i < n; ++i) printf("%a\n", (double)ema[i]);
    free(ema);
    free(param);
    return 0;
}
