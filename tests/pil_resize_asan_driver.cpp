// Runs hoig_pil_bilinear_table and hoig_resize_pil_bilinear_u8_host (hoig_amd/csrc/pil_resize_host.cpp) on the cases given on the
// command line, every buffer in a heap block of exactly its size -- built with -fsanitize=address by tests/test_pil_resize_cpu.py, so
// that a read or write one byte outside a buffer aborts the run.  Arguments: B, then H W Ho Wo per case.  The content of a case is
// byte i = (i * 2654435761 + H * 31 + W) >> 24 (uint32 arithmetic); prints one line per case: "<return code> <FNV-1a of dst>".
#include <stdio.h>
#include <stdlib.h>

#include "hoig_kernels.h"

int main(int argc, char **argv) {
    if (argc < 6 || (argc - 2) % 4) return 2;
    const int B = atoi(argv[1]);
    for (int a = 2; a + 3 < argc; a += 4) {
        const int H = atoi(argv[a]), W = atoi(argv[a + 1]), Ho = atoi(argv[a + 2]), Wo = atoi(argv[a + 3]);
        const size_t n = (size_t)B * H * W * 3, m = (size_t)B * Ho * Wo * 3;
        uint8_t *src = (uint8_t *)malloc(n), *dst = (uint8_t *)malloc(m);
        for (size_t i = 0; i < n; ++i) src[i] = (uint8_t)(((uint32_t)i * 2654435761u + (uint32_t)(H * 31 + W)) >> 24);
        const int dims[2][2] = {{W, Wo}, {H, Ho}};
        for (int k = 0; k < 2; ++k) {     // the tables on their own, each in a block of its exact size
            const int ksize = hoig_pil_bilinear_ksize(dims[k][0], dims[k][1]);
            if (ksize < 0) return 3;
            int32_t *table = (int32_t *)malloc(sizeof(int32_t) * (size_t)dims[k][1] * (2 + ksize));
            if (hoig_pil_bilinear_table(dims[k][0], dims[k][1], table) != HOIG_OK) return 3;
            free(table);
        }
        const int rc = hoig_resize_pil_bilinear_u8_host(src, B, H, W, 3, dst, Ho, Wo);
        uint32_t h = 2166136261u;
        for (size_t i = 0; i < m; ++i) h = (h ^ dst[i]) * 16777619u;
        printf("%d %u\n", rc, h);
        free(dst);
        free(src);
    }
    return 0;
}
