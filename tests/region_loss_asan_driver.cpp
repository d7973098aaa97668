// region_loss_host.cpp in a program of its own, every buffer a heap block of exactly its size -- built with -fsanitize=address,undefined by
// tests/test_region_loss_cpu.py, so that a read or write one element outside a buffer aborts the run.
//   region_loss_asan_driver N H W C  ->  "rc term term_all L_0 L_1 L_2 sum(dpred) status counts..." (floats as hex), then the call with
//   every optional pointer null: "rc term status"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "hoig_kernels.h"

namespace {

// fixed patterns with exact zeros of the difference in them, and a label above R now and then
float value(int64_t k, int side) {
    return side ? (float)((k * 29 + 7) % 43 - 21) * 0.046875f : (float)((k * 37) % 41 - 20) * 0.046875f;
}
uint8_t label(int64_t q) { return q % 97 == 96 ? 7 : (uint8_t)((q * 5 + q / 3) % 3); }

}  // namespace

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const int N = atoi(argv[1]), H = atoi(argv[2]), W = atoi(argv[3]), C = atoi(argv[4]), R = 2;
    const int64_t px = (int64_t)N * H * W, n = px * C;
    float *pred = (float *)malloc(sizeof(float) * n), *target = (float *)malloc(sizeof(float) * n), *dpred = (float *)malloc(sizeof(float) * n);
    uint8_t *labels = (uint8_t *)malloc(px);
    for (int64_t k = 0; k < n; ++k) pred[k] = value(k, 0), target[k] = value(k, 1);
    for (int64_t q = 0; q < px; ++q) labels[q] = label(q);
    double *lambda = (double *)malloc(sizeof(double) * (R + 1));
    lambda[0] = 0.25, lambda[1] = 10.0, lambda[2] = 2.5;
    float *term = (float *)malloc(sizeof(float)), *term_all = (float *)malloc(sizeof(float)), *terms_r = (float *)malloc(sizeof(float) * (R + 1));
    int32_t *counts = (int32_t *)malloc(sizeof(int32_t) * N * (R + 1)), *status = (int32_t *)malloc(sizeof(int32_t));
    *term = *term_all = 0.f;
    for (int r = 0; r <= R; ++r) terms_r[r] = 0.f;
    int rc = hoig_region_loss_host(pred, target, labels, N, H, W, C, R, lambda, 30.0, 2, dpred, term, terms_r, term_all, counts, status);
    double s = 0.0;
    for (int64_t k = 0; k < n; ++k) s += dpred[k];
    printf("%d %a %a %a %a %a %a %d", rc, *term, *term_all, terms_r[0], terms_r[1], terms_r[2], s, *status);
    for (int k = 0; k < N * (R + 1); ++k) printf(" %d", counts[k]);
    printf("\n");
    *term = 0.f;
    rc = hoig_region_loss_host(pred, target, labels, N, H, W, C, R, lambda, 30.0, 2, nullptr, term, nullptr, nullptr, nullptr, status);
    printf("%d %a %d\n", rc, *term, *status);
    free(pred), free(target), free(dpred), free(labels), free(lambda), free(term), free(term_all), free(terms_r), free(counts), free(status);
    return 0;
}
