// Host half of the Pillow-exact 8-bit bilinear resize (pil_resize.h): the coefficient tables and the CPU twin of the kernel.  Plain
// C++ with no HIP call (it also builds on its own under a host sanitizer).
#include <string.h>
#include <vector>

#include "pil_resize.h"

extern "C" int hoig_pil_bilinear_ksize(int in, int out) {
    if (!pil_side_ok(in) || !pil_side_ok(out)) return HOIG_EINVAL;
    return pil_ksize(in, out);
}

extern "C" int hoig_pil_bilinear_table(int in, int out, int32_t *table) {
    if (!table || !pil_side_ok(in) || !pil_side_ok(out)) return HOIG_EINVAL;
    pil_build_table(in, out, table);
    return HOIG_OK;
}

extern "C" int64_t hoig_resize_pil_bilinear_u8_workspace_bytes(int B, int H, int W, int C, int Ho, int Wo) {
    if (B < 1 || C != 3 || !pil_side_ok(H) || !pil_side_ok(W) || !pil_side_ok(Ho) || !pil_side_ok(Wo)) return HOIG_EINVAL;
    if (W == Wo || H == Ho) return 0;
    int first, rows;
    pil_rows_read(H, Ho, &first, &rows);
    return (int64_t)B * rows * Wo * C;
}

namespace {

// dst [outer][n_out][inner] from src [outer][..][inner]: one 1-D resample along the axis whose samples lie `inner` bytes apart.
// src_outer: bytes between two outer slices of src; shift: the axis index src starts at (subtracted from every xmin)
void resample_axis(const uint8_t *src, uint8_t *dst, const int32_t *table, int ksize, int64_t outer, int n_out, int64_t inner,
                   int64_t src_outer, int shift) {
    for (int64_t o = 0; o < outer; ++o)
        for (int xx = 0; xx < n_out; ++xx) {
            const int32_t *row = table + (int64_t)xx * (PIL_ROW_HEAD + ksize);
            const uint8_t *s = src + o * src_outer + (int64_t)(row[0] - shift) * inner;
            uint8_t *d = dst + (o * n_out + xx) * inner;
            for (int64_t j = 0; j < inner; ++j) d[j] = pil_resample_byte(s + j, inner, row + PIL_ROW_HEAD, row[1]);
        }
}

}  // namespace

extern "C" int hoig_resize_pil_bilinear_u8_host(const uint8_t *src, int B, int H, int W, int C, uint8_t *dst, int Ho, int Wo) {
    if (!src || !dst || B < 1 || C != 3 || !pil_side_ok(H) || !pil_side_ok(W) || !pil_side_ok(Ho) || !pil_side_ok(Wo)) return HOIG_EINVAL;
    const bool horiz = W != Wo, vert = H != Ho;
    if (!horiz && !vert) {
        memcpy(dst, src, (size_t)B * H * W * C);
        return HOIG_OK;
    }
    std::vector<int32_t> th, tv;
    int kh = 0, kv = 0, first = 0, rows = H;
    if (horiz) {
        kh = pil_ksize(W, Wo);
        th.resize((size_t)Wo * (PIL_ROW_HEAD + kh));
        pil_build_table(W, Wo, th.data());
    }
    if (vert) {
        kv = pil_ksize(H, Ho);
        tv.resize((size_t)Ho * (PIL_ROW_HEAD + kv));
        pil_build_table(H, Ho, tv.data());
        pil_rows_read(H, Ho, &first, &rows);
    }
    const int64_t in_row = (int64_t)W * C, out_row = (int64_t)Wo * C;
    if (!vert) {
        resample_axis(src, dst, th.data(), kh, (int64_t)B * H, Wo, C, in_row, 0);
        return HOIG_OK;
    }
    if (!horiz) {
        resample_axis(src, dst, tv.data(), kv, B, Ho, out_row, (int64_t)H * in_row, 0);
        return HOIG_OK;
    }
    // the intermediate holds the rows [first, first + rows) of every image
    std::vector<uint8_t> mid((size_t)B * rows * out_row);
    for (int b = 0; b < B; ++b)
        resample_axis(src + ((int64_t)b * H + first) * in_row, mid.data() + (int64_t)b * rows * out_row, th.data(), kh, rows, Wo, C,
                      in_row, 0);
    resample_axis(mid.data(), dst, tv.data(), kv, B, Ho, out_row, (int64_t)rows * out_row, first);
    return HOIG_OK;
}
