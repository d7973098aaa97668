// Runs hoig_png_encode_bound and hoig_png_encode_host (hoig_amd/csrc/png_host.cpp) on the cases given on the command line, every
// buffer in a heap block of exactly its size -- built with -fsanitize=address by tests/test_png_cpu.py, so that a read or write one
// byte outside a buffer aborts the run.  Arguments: B, then H W C segment_bytes mode per case.  The content of a case is, by mode,
// 0: byte i = (i * 2654435761 + H * 31 + W) >> 24 (uint32 arithmetic), 1: zeros, 2: byte i = i >> 4; prints one line per case:
// "<return code> <FNV-1a of the B files one after the other>".
#include <stdio.h>
#include <stdlib.h>

#include "hoig_kernels.h"

int main(int argc, char **argv) {
    if (argc < 7 || (argc - 2) % 5) return 2;
    const int B = atoi(argv[1]);
    for (int a = 2; a + 4 < argc; a += 5) {
        const int H = atoi(argv[a]), W = atoi(argv[a + 1]), C = atoi(argv[a + 2]), seg = atoi(argv[a + 3]), mode = atoi(argv[a + 4]);
        const int64_t stride = hoig_png_encode_bound(H, W, C, seg);
        if (stride < 0) return 3;
        const size_t n = (size_t)B * H * W * C;
        uint8_t *src = (uint8_t *)malloc(n), *out = (uint8_t *)malloc((size_t)B * stride);
        int32_t *sizes = (int32_t *)malloc(sizeof(int32_t) * B);
        for (size_t i = 0; i < n; ++i)
            src[i] = mode == 0 ? (uint8_t)(((uint32_t)i * 2654435761u + (uint32_t)(H * 31 + W)) >> 24) : mode == 1 ? 0 : (uint8_t)(i >> 4);
        const int rc = hoig_png_encode_host(src, B, H, W, C, out, stride, sizes, seg);
        uint32_t h = 2166136261u;
        for (int b = 0; b < B; ++b)
            for (int32_t i = 0; i < sizes[b]; ++i) h = (h ^ out[(size_t)b * stride + i]) * 16777619u;
        printf("%d %u\n", rc, h);
        free(sizes);
        free(out);
        free(src);
    }
    return 0;
}
