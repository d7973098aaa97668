// The host half of the rasteriser's setup stage (raster_box.h, docs/raster_parity.md): the CPU twin of the tile boxes that
// raster_setup_kernel writes, through the same inline functions -- EMPTY for a back face, else the face's box.  No HIP call; host memory
// only.  Built with -ffp-contract=off, like the kernel.
#include "hoig_kernels.h"
#include "raster_box.h"

extern "C" int hoig_raster_face_boxes_host(const float *faces, int n_faces, int image_size, uint32_t *boxes_out) {
    if (!faces || !boxes_out || n_faces <= 0 || image_size <= 0 || image_size > 4096) return HOIG_EINVAL;
    for (int i = 0; i < n_faces; ++i) {
        const float *f = faces + (size_t)i * 9;
        boxes_out[i] = raster_back_side(f) ? RB_EMPTY_BOX : raster_face_box(f, image_size);
    }
    return HOIG_OK;
}
