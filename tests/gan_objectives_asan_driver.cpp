// gan_loss_host.cpp in a program of its own, every buffer a heap block of exactly its size -- built with -fsanitize=address,undefined by
// tests/test_gan_objectives_cpu.py, so that a read or write one element outside a buffer aborts the run.
//   gan_objectives_asan_driver n_a n_b  ->  per mode, form and start (before / after): "rc" and, as hex, the four slots, the sums of
//   the two gradients, and the state's words; then the G head's term and gradient sum per mode
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "hoig_kernels.h"

namespace {

// logit i of a side: a fixed pattern with exact zeros and the hinge's kinks in it
float logit(int64_t i, int side) {
    const int k = (int)((i * 37 + side * 11) % 41);
    if (k == 0) return 0.f;
    if (k == 1) return 1.f;
    if (k == 2) return -1.f;
    return (float)(k - 20) * 0.171875f + (side ? 0.25f : -0.125f);
}

double sum(const float *x, int64_t n) {
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s += x[i];
    return s;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const int64_t n_a = atoll(argv[1]), n_b = atoll(argv[2]);
    float *a = (float *)malloc(sizeof(float) * n_a), *b = (float *)malloc(sizeof(float) * n_b);
    float *da = (float *)malloc(sizeof(float) * n_a), *db = (float *)malloc(sizeof(float) * n_b);
    for (int64_t i = 0; i < n_a; ++i) a[i] = logit(i, 0);
    for (int64_t i = 0; i < n_b; ++i) b[i] = logit(i, 1);
    float *slots = (float *)malloc(sizeof(float) * 4);
    uint64_t *state = (uint64_t *)malloc(sizeof(uint64_t) * HOIG_LECAM_STATE_WORDS);
    union { double d; uint64_t u; } g;
    g.d = 0.9;
    for (int mode = HOIG_GAN_LSGAN; mode <= HOIG_GAN_LOGISTIC; ++mode) {
        for (int form = HOIG_LECAM_PAPER; form <= HOIG_LECAM_RELU; ++form) {
            for (int64_t i = 0; i < HOIG_LECAM_STATE_WORDS; ++i) state[i] = 0;
            state[3] = g.u, state[4] = 1;
            for (int step = 0; step < 2; ++step) {      // the first tick sets the anchors: the second step has the regulariser
                for (int j = 0; j < 4; ++j) slots[j] = 0.f;
                const int rc = hoig_gan_d_loss_host(mode, a, n_a, b, n_b, 0.5, 0.3, form, state, da, db, slots, slots + 1, slots + 2, slots + 3);
                printf("%d %a %a %a %a %a %a", rc, slots[0], slots[1], slots[2], slots[3], sum(da, n_a), sum(db, n_b));
                for (int64_t i = 0; i < HOIG_LECAM_STATE_WORDS; ++i) printf(" %llx", (unsigned long long)state[i]);
                printf("\n");
            }
        }
        // null gradients, no state, no report slots
        slots[0] = 0.f;
        const int rc0 = hoig_gan_d_loss_host(mode, a, n_a, b, n_b, 0.5, 0.0, HOIG_LECAM_PAPER, nullptr, nullptr, nullptr, slots, nullptr,
                                             nullptr, nullptr);
        printf("%d %a\n", rc0, slots[0]);
        slots[0] = 0.f;
        const int rc1 = hoig_gan_g_loss_host(mode, b, n_b, 0.5, db, slots);
        printf("%d %a %a\n", rc1, slots[0], sum(db, n_b));
    }
    free(a), free(b), free(da), free(db), free(slots), free(state);
    return 0;
}
