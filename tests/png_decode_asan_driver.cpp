// A program of its own around png_decode_host.cpp for a host AddressSanitizer build (tests/test_png_decode_cpu.py): it reads a file of
// cases (int32 count; per case width, height, colour type, bit depth, stream bytes, palette bytes, bgr, then the stream and the
// palette), decodes each through hoig_png_decode_host with every buffer a heap block of exactly its size, and prints one line per case:
// the status and the FNV-1a hash of the pixels (0 with a status).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hoig_kernels.h"

static int32_t read_i32(FILE *f) {
    int32_t v = 0;
    if (fread(&v, 4, 1, f) != 1) exit(3);
    return v;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int n = read_i32(f);
    for (int i = 0; i < n; ++i) {
        hoig_png_decode_plan p;
        memset(&p, 0, sizeof p);
        p.width = read_i32(f), p.height = read_i32(f), p.color_type = read_i32(f), p.bit_depth = read_i32(f);
        p.data_len = read_i32(f);
        const int pal = read_i32(f), bgr = read_i32(f);
        p.pal_entries = pal / 3;
        p.pal_off = pal ? (p.data_len + 15) / 16 * 16 : 0;
        const int64_t nbytes = pal ? p.pal_off + pal : p.data_len;
        uint8_t *bytes = (uint8_t *)malloc((size_t)(nbytes > 0 ? nbytes : 1));
        memset(bytes, 0, (size_t)nbytes);
        if (p.data_len && fread(bytes, (size_t)p.data_len, 1, f) != 1) return 3;
        if (pal && fread(bytes + p.pal_off, (size_t)pal, 1, f) != 1) return 3;
        const int64_t ws_bytes = hoig_png_decode_workspace_bytes(&p, 1);
        if (ws_bytes < 0) return 4;
        const int64_t out_bytes = (int64_t)p.width * p.height * 3;
        uint8_t *out = (uint8_t *)malloc((size_t)out_bytes), *ws = (uint8_t *)malloc((size_t)ws_bytes);
        int32_t *status = (int32_t *)malloc(sizeof(int32_t));
        *status = -1;
        memset(out, 0, (size_t)out_bytes);
        const int rc = hoig_png_decode_host(bytes, nbytes, &p, 1, out, out_bytes, status, ws, ws_bytes, bgr);
        if (rc != HOIG_OK) return 5;
        uint32_t h = 2166136261u;
        if (*status == 0)
            for (int64_t k = 0; k < out_bytes; ++k) h = (h ^ out[k]) * 16777619u;
        printf("%d %u\n", *status, *status == 0 ? h : 0u);
        free(bytes), free(out), free(ws), free(status);
    }
    fclose(f);
    return 0;
}
