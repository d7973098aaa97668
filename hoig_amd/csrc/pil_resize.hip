// Pillow's 8-bit Image.resize(size, BILINEAR) for a batch on the device (the algorithm and the table layout: pil_resize.h): what
// get_eval_loader does to every image before LPIPS and SSIM / MS-SSIM see it, so that eval output can be scored from device memory
// with the bytes the PNG path would have produced.
//
// One kernel: a 1-D resample along a strided axis, launched once per pass that changes its size -- along W first (samples 3 bytes
// apart) into the caller's workspace, which holds only the rows the second pass reads, then along H (samples one row apart).  Byte
// work bound by what it moves: a lane makes PER_LANE consecutive output bytes of a row and stores them as one word, so that a wave's
// loads of each tap and its stores are contiguous; the taps come from the small table (a few KB, cached).
// Built with -ffp-contract=off: the host doubles of pil_resize.h round step by step.
#include "common.h"
#include "pil_resize.h"

namespace {

constexpr int NT = 256;
constexpr int PER_LANE = 4;

// dst [B][R][n_out][inner] bytes, contiguous.  src: image b at b * src_b, its slice r at r * src_r, and in a slice the axis samples
// `inner` bytes apart, of which src holds n_avail, the first being axis index `shift` (the tables' xmin count from 0).
__global__ __launch_bounds__(NT) void pil_resample_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                          const int32_t *__restrict__ table, int ksize, int n_avail, int shift,
                                                          int n_out, int inner, int R, int64_t src_b, int64_t src_r, int64_t total) {
    const int rowlen = PIL_ROW_HEAD + ksize;
    for (int64_t i0 = ((int64_t)blockIdx.x * NT + threadIdx.x) * PER_LANE; i0 < total; i0 += (int64_t)gridDim.x * NT * PER_LANE) {
        int j = (int)(i0 % inner);
        const int64_t q = i0 / inner;
        int xx = (int)(q % n_out);
        int64_t o = q / n_out;
        const uint8_t *slice = src + (o / R) * src_b + (o % R) * src_r;
        const int cnt = total - i0 < PER_LANE ? (int)(total - i0) : PER_LANE;
        uint32_t word = 0;
        for (int e = 0; e < cnt; ++e) {
            const int32_t *row = table + (int64_t)xx * rowlen;
            // a well-formed table keeps [xmin, xmin + n) inside the samples src holds; the clamps keep a bad one from reading outside
            int xmin = row[0] - shift, n = row[1] < ksize ? row[1] : ksize;
            if (xmin < 0) xmin = 0;
            if (n > n_avail - xmin) n = n_avail - xmin;
            word |= (uint32_t)pil_resample_byte(slice + (int64_t)xmin * inner + j, inner, row + PIL_ROW_HEAD, n) << (8 * e);
            if (++j == inner) {
                j = 0;
                if (++xx == n_out) {
                    xx = 0;
                    ++o;
                    slice = src + (o / R) * src_b + (o % R) * src_r;
                }
            }
        }
        if (cnt == PER_LANE) {
            *reinterpret_cast<uint32_t *>(dst + i0) = word;     // i0 % 4 == 0 and dst is 4-byte aligned (checked by the entry)
        } else {
            for (int e = 0; e < cnt; ++e) dst[i0 + e] = (uint8_t)(word >> (8 * e));
        }
    }
}

int resample(const uint8_t *src, uint8_t *dst, const int32_t *table, int ksize, int n_avail, int shift, int n_out, int inner, int R,
             int64_t src_b, int64_t src_r, int B, hipStream_t st) {
    const int64_t total = (int64_t)B * R * n_out * inner;
    pil_resample_kernel<<<hoig_stream_grid(hoig_cdiv(total, PER_LANE), NT), NT, 0, st>>>(src, dst, table, ksize, n_avail, shift, n_out,
                                                                                        inner, R, src_b, src_r, total);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}

}  // namespace

extern "C" int hoig_resize_pil_bilinear_u8(const uint8_t *src, int B, int H, int W, int C, uint8_t *dst, int Ho, int Wo,
                                           const int32_t *table_w, const int32_t *table_h, void *workspace, hoig_stream_t stream) {
    if (!src || !dst || B < 1 || C != 3 || !pil_side_ok(H) || !pil_side_ok(W) || !pil_side_ok(Ho) || !pil_side_ok(Wo)) return HOIG_EINVAL;
    const bool horiz = W != Wo, vert = H != Ho;
    if ((horiz && !table_w) || (vert && !table_h) || (horiz && vert && !workspace)) return HOIG_EINVAL;
    if (((uintptr_t)dst & 3) || ((uintptr_t)workspace & 3)) return HOIG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int64_t in_row = (int64_t)W * C, in_img = (int64_t)H * in_row;
    const int out_row = Wo * C;
    if (!horiz && !vert) {
        if (hipMemcpyAsync(dst, src, (size_t)B * in_img, hipMemcpyDeviceToDevice, st) != hipSuccess) return HOIG_ELAUNCH;
        return HOIG_OK;
    }
    if (!vert) return resample(src, dst, table_w, pil_ksize(W, Wo), W, 0, Wo, C, H, in_img, in_row, B, st);
    if (!horiz) return resample(src, dst, table_h, pil_ksize(H, Ho), H, 0, Ho, out_row, 1, in_img, 0, B, st);
    int first, rows;
    pil_rows_read(H, Ho, &first, &rows);
    uint8_t *mid = static_cast<uint8_t *>(workspace);   // [B][rows][Wo][C]
    const int rc = resample(src + first * in_row, mid, table_w, pil_ksize(W, Wo), W, 0, Wo, C, rows, in_img, in_row, B, st);
    if (rc != HOIG_OK) return rc;
    return resample(mid, dst, table_h, pil_ksize(H, Ho), rows, first, Ho, out_row, 1, (int64_t)rows * out_row, 0, B, st);
}
