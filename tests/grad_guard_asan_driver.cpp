// hoig_grad_stats_host (hoig_amd/csrc/grad_guard_host.cpp) in a program of its own, for a host AddressSanitizer / UBSan build
// (tests/test_grad_guard_cpu.py): every buffer is a heap block of exactly its size, so a read or write past an end is a report.
//   grad_guard_asan_driver n first0 count0 first1 count1 ..   ->  "rc", then total and every row as three hex doubles
// x[i] = (((i * 37 + 11) % 41) - 20) / 8, +Inf where i % 97 == 5, NaN where i % 101 == 3 (the test restates it in numpy).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "hoig_kernels.h"

int main(int argc, char **argv) {
    if (argc < 2 || (argc - 2) % 2) return 2;
    const int64_t n = atoll(argv[1]);
    const int nseg = (argc - 2) / 2;
    std::vector<int64_t> segs(2 * (size_t)nseg);
    for (size_t i = 0; i < segs.size(); ++i) segs[i] = atoll(argv[2 + i]);
    std::vector<float> x((size_t)(n > 0 ? n : 0));
    for (int64_t i = 0; i < n; ++i) {
        x[i] = (float)(((i * 37 + 11) % 41) - 20) * 0.125f;
        if (i % 97 == 5) x[i] = INFINITY;
        if (i % 101 == 3) x[i] = NAN;
    }
    const int64_t bytes = hoig_grad_stats_workspace_bytes(n > 0 ? n : 1, nseg);
    if (bytes < 0) return 3;
    std::vector<double> ws((size_t)bytes / 8), total(3, -7.25), seg(3 * (size_t)nseg, -7.25);
    const int rc = hoig_grad_stats_host(x.data(), n, segs.data(), nseg, seg.data(), total.data(), ws.data());
    printf("%d\n%a %a %a\n", rc, total[0], total[1], total[2]);
    for (int s = 0; s < nseg; ++s) printf("%a %a %a\n", seg[3 * s], seg[3 * s + 1], seg[3 * s + 2]);
    float guard[2] = {0.f, 0.f};
    std::vector<double> record(7, 0.0);
    if (rc == 0 && hoig_guard_decide_host(total.data(), 0.5, 1.0, HOIG_GUARD_SKIP, guard, record.data()) != 0) return 4;
    printf("%a %a %a\n", (double)guard[0], (double)guard[1], record[3]);
    return 0;
}
