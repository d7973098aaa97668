// raster_host.cpp in a program of its own, every buffer a heap block of exactly its size -- built with -fsanitize=address,undefined by
// tests/test_raster_box_cpu.py, so that a read or write one element outside a buffer aborts the run.
//   raster_box_asan_driver n_faces image_size  ->  "rc box_0 box_1 ..." (boxes as hex)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "hoig_kernels.h"

namespace {

// a fixed pattern on a grid of 1/32: equal vertices, collinear faces, back faces and faces off the image are in it; an inf now and then
float coord(int64_t k) {
    if (k % 173 == 172) return INFINITY;
    const float v = (float)((k * 37 + (k / 9) * 11) % 83 - 41) * 0.03125f;
    return k % 9 % 3 == 2 ? v + 3.0f : v;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const int n = atoi(argv[1]), S = atoi(argv[2]);
    float *faces = (float *)malloc(sizeof(float) * 9 * n);
    uint32_t *boxes = (uint32_t *)malloc(sizeof(uint32_t) * n);
    for (int64_t k = 0; k < (int64_t)n * 9; ++k) faces[k] = coord(k);
    const int rc = hoig_raster_face_boxes_host(faces, n, S, boxes);
    printf("%d", rc);
    for (int i = 0; i < n; ++i) printf(" %x", boxes[i]);
    printf("\n");
    free(faces), free(boxes);
    return 0;
}
