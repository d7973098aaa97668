// Runs hoig_jpeg_entropy_par_host (hoig_amd/csrc/jpeg_host.cpp) on the cases of a file written by tests/test_jpeg_par_cpu.py, every buffer
// in a heap block of exactly its size -- built with -fsanitize=address by that test, so that a read or write one byte outside a buffer
// aborts the run.  File: int32 count, then per case int64 nbytes, n_entries, coef_bytes, subseq_bytes, lanes, n_states | hoig_jpeg_plan |
// bytes | int32 intervals.  Prints one line per case: "<return code> <status word>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hoig_kernels.h"

static void *take(FILE *f, size_t n) {
    void *p = malloc(n ? n : 1);
    if (n && fread(p, 1, n, f) != n) exit(2);
    return p;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t count = 0;
    if (fread(&count, sizeof count, 1, f) != 1) return 2;
    for (int32_t k = 0; k < count; ++k) {
        int64_t head[6];
        if (fread(head, sizeof head, 1, f) != 1) return 2;
        hoig_jpeg_plan *plan = (hoig_jpeg_plan *)take(f, sizeof(hoig_jpeg_plan));
        uint8_t *bytes = (uint8_t *)take(f, (size_t)head[0]);
        int32_t *intervals = (int32_t *)take(f, (size_t)head[1] * sizeof(int32_t));
        void *coef = malloc((size_t)head[2]);
        int32_t *status = (int32_t *)malloc(sizeof(int32_t));
        int32_t *rounds = (int32_t *)malloc(sizeof(int32_t));
        int32_t *states = (int32_t *)malloc((size_t)(head[5] ? head[5] : 1) * 4 * sizeof(int32_t));
        *status = -1;
        const int rc = hoig_jpeg_entropy_par_host(bytes, head[0], plan, 1, intervals, head[1], (int)head[3], (int)head[4], coef, head[2],
                                                  status, rounds, states, head[5]);
        printf("%d %d\n", rc, (int)*status);
        free(states); free(rounds); free(status); free(coef); free(intervals); free(bytes); free(plan);
    }
    fclose(f);
    return 0;
}
