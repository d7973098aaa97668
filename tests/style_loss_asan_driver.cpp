// style_loss_host.cpp in a program of its own, every buffer a heap block of exactly its size -- built with -fsanitize=address,undefined by
// tests/test_style_loss_cpu.py, so that a read or write one element outside a buffer aborts the run.
//   style_loss_asan_driver N P C  ->  "rc term report sum(S) sum(|S|) sum(gram) rc sum(dfx)" (floats as hex), then the Gram call with
//   every optional pointer null: "rc sum(S)"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "hoig_kernels.h"

namespace {

// fixed patterns of ReLU-like values: about half of them exactly 0
float value(int64_t k, int side) {
    const int v = side ? (int)((k * 29 + 7) % 43) - 21 : (int)((k * 37) % 41) - 20;
    return v > 0 ? (float)v * 0.046875f : 0.f;
}

void *block(size_t bytes) {
    void *p = nullptr;
    if (posix_memalign(&p, 16, bytes) != 0) exit(3);
    return p;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const int N = atoi(argv[1]), P = atoi(argv[2]), C = atoi(argv[3]);
    const int64_t n = (int64_t)N * P * C, ns = (int64_t)N * C * C;
    float *fx = (float *)block(sizeof(float) * n), *fy = (float *)block(sizeof(float) * n), *dfx = (float *)block(sizeof(float) * n);
    float *S = (float *)block(sizeof(float) * ns);
    double *gram = (double *)block(sizeof(double) * 2 * ns);
    float *term = (float *)malloc(sizeof(float)), *report = (float *)malloc(sizeof(float));
    for (int64_t k = 0; k < n; ++k) fx[k] = value(k, 0), fy[k] = value(k, 1);
    *term = 0.5f, *report = 0.25f;
    int rc = hoig_style_gram_host(fx, fy, N, P, C, 10.0, S, term, report, gram);
    double s = 0.0, sa = 0.0, sg = 0.0, sd = 0.0;
    for (int64_t k = 0; k < ns; ++k) s += S[k], sa += S[k] < 0 ? -S[k] : S[k];
    for (int64_t k = 0; k < 2 * ns; ++k) sg += gram[k];
    const int rc2 = hoig_style_dfeat_host(fx, S, N, P, C, dfx);
    for (int64_t k = 0; k < n; ++k) sd += dfx[k];
    printf("%d %a %a %a %a %a %d %a\n", rc, *term, *report, s, sa, sg, rc2, sd);
    rc = hoig_style_gram_host(fx, fy, N, P, C, 2.5, S, nullptr, nullptr, nullptr);
    s = 0.0;
    for (int64_t k = 0; k < ns; ++k) s += S[k];
    printf("%d %a\n", rc, s);
    free(fx), free(fy), free(dfx), free(S), free(gram), free(term), free(report);
    return 0;
}
