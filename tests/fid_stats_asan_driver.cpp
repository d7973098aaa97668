// Runs the CPU twins of the fp64 FID statistics (hoig_amd/csrc/fid_stats_host.cpp) with every buffer in a heap block of exactly its
// size -- built with -fsanitize=address by tests/test_fid_device_cpu.py, so that a read or write one element outside a buffer aborts the
// run.  Arguments: K M N.  A [K][M] and B [K][N] hold x[k][c] = ((k * 31 + c * 17) % 23 - 11) / 8; the program makes C = A^T B, the
// symmetric Gram matrix G = C^T C, the pivoted Cholesky factor and the eigenvalues of G, then both of the rank-1 matrix
// (i + 1)(j + 1), 5 x 5.  One line per result: "<name> <return code> [<rank>] <FNV-1a of the result's bytes>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hoig_kernels.h"

static uint32_t fnv(const void *p, size_t n) {
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const uint8_t *>(p)[i]) * 16777619u;
    return h;
}

static double *block(size_t n) {
    double *p = (double *)malloc(sizeof(double) * n);
    memset(p, 0, sizeof(double) * n);
    return p;
}

static double *operand(int rows, int cols) {
    double *p = block((size_t)rows * cols);
    for (int k = 0; k < rows; ++k)
        for (int c = 0; c < cols; ++c) p[(size_t)k * cols + c] = ((k * 31 + c * 17) % 23 - 11) / 8.0;
    return p;
}

static void factor_and_eigenvalues(const char *suffix, const double *g, int n) {
    double *fac = block((size_t)n * n), *lam = block(n);
    int32_t *piv = (int32_t *)malloc(sizeof(int32_t) * n), info[2] = {0, 0}, einfo[1] = {0};
    memset(piv, 0, sizeof(int32_t) * n);
    int rc = hoig_pchol_f64_host(g, n, n, fac, n, piv, info);
    printf("pchol%s %d %d %u\n", suffix, rc, info[0], fnv(fac, sizeof(double) * n * n));
    rc = hoig_sym_eigvals_f64_host(g, n, n, lam, einfo);
    printf("eig%s %d %u\n", suffix, rc, fnv(lam, sizeof(double) * n));
    free(piv);
    free(lam);
    free(fac);
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const int K = atoi(argv[1]), M = atoi(argv[2]), N = atoi(argv[3]);
    if (K < 1 || M < 1 || N < 1) return 2;
    double *a = operand(K, M), *b = operand(K, N), *c = block((size_t)M * N), *g = block((size_t)N * N);
    int rc = hoig_gemm_tn_f64_host(a, M, b, N, NULL, c, N, M, N, K, 0);
    printf("gemm %d %u\n", rc, fnv(c, sizeof(double) * M * N));
    rc = hoig_gemm_tn_f64_host(c, N, c, N, NULL, g, N, N, N, M, HOIG_GEMM_SYMMETRIC);
    printf("gram %d %u\n", rc, fnv(g, sizeof(double) * N * N));
    factor_and_eigenvalues("", g, N);
    double *one = block(25);
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 5; ++j) one[i * 5 + j] = (i + 1.0) * (j + 1.0);
    factor_and_eigenvalues("1", one, 5);
    free(one);
    free(g);
    free(c);
    free(b);
    free(a);
    return 0;
}
