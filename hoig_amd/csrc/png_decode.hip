// PNG files decoded on the device (the format subset, the per-lane code and the phases: png_inflate.h; docs/png_decode.md): the metric
// directory functions take file bytes to pixels without pixel work on the host.  Integer-only; two launches for a batch:
//
//   inflate   a wave per image runs PNGD_RUN_INFLATE: the zlib stream -> the filtered stream in the workspace, status[i].  About
//             39 KiB of LDS (the 32 KiB window, 1 KiB of the stream, the block's tables, a round's tokens): four images share a CU.
//   rows      a 256-lane workgroup per image runs PNGD_RUN_ROWS: the five filters undone as a skewed pipeline over rows, bits unpacked,
//             grey scaled, palette looked up, alpha dropped -> RGB or BGR at the image's out_off.  An image with a status is skipped.
#include "common.h"
#include "png_inflate.h"
#include "tuning.h"

namespace {

// LDS accesses of the workgroup ordered, without waiting for its global stores (vmcnt 63, expcnt 7, lgkmcnt 0 on gfx9); the signal
// fences keep the compiler from moving a memory access across
#define PNGD_LDS_BARRIER()                        \
    do {                                          \
        __atomic_signal_fence(__ATOMIC_SEQ_CST);  \
        __builtin_amdgcn_s_waitcnt(0xc07f);       \
        __builtin_amdgcn_s_barrier();             \
        __atomic_signal_fence(__ATOMIC_SEQ_CST);  \
    } while (0)
#define PNGD_DEVICE_LANES(body)       \
    {                                 \
        const int lane = threadIdx.x; \
        body;                         \
    }

// WS: the "png_window" key's other side -- matches read the workspace, so every barrier also orders the global accesses
template <bool WS>
__global__ __launch_bounds__(PNGD_LANES) void png_inflate_kernel(const uint8_t *__restrict__ bytes, const hoig_png_decode_plan *__restrict__ plans,
                                                                 uint8_t *ws, int32_t *status) {
    __shared__ PngdShared sh;
    const hoig_png_decode_plan p = plans[blockIdx.x];
    PngdCtx c;
    c.sh = &sh;
    c.data = bytes + p.data_off, c.data_len = p.data_len;
    c.out = ws + p.filt_off, c.expect = pngd_expect(&p);
    c.status = status + blockIdx.x;
    c.ws_window = WS;
#define PNGD_WINDOW_BARRIER()             \
    do {                                  \
        if (WS) __syncthreads();          \
        else PNGD_LDS_BARRIER();          \
    } while (0)
    PNGD_RUN_INFLATE(c, PNGD_DEVICE_LANES, __syncthreads(), PNGD_WINDOW_BARRIER());
#undef PNGD_WINDOW_BARRIER
}

__global__ __launch_bounds__(PNGD_ROWS) void png_rows_kernel(const uint8_t *__restrict__ bytes, const hoig_png_decode_plan *__restrict__ plans,
                                                             uint8_t *ws, uint8_t *out, int32_t *status, int bgr) {
    __shared__ PngdRowShared sh;
    const hoig_png_decode_plan p = plans[blockIdx.x];
    PngdRowCtx c;
    c.sh = &sh;
    c.filt = ws + p.filt_off, c.out = out + p.out_off, c.pal = bytes + (p.color_type == 3 ? p.pal_off : 0);
    c.status = status + blockIdx.x;
    c.W = p.width, c.H = p.height, c.ctype = p.color_type, c.depth = p.bit_depth;
    c.bpp = pngd_bpp(p.color_type, p.bit_depth), c.rowbytes = (int32_t)pngd_rowbytes(p.width, p.color_type, p.bit_depth);
    c.units = c.rowbytes / c.bpp, c.pal_entries = p.pal_entries, c.bgr = bgr;
    PngdLane st;
#define PNGD_DEVICE_ST(lane) st
    PNGD_RUN_ROWS(c, PNGD_DEVICE_LANES, __syncthreads(), PNGD_LDS_BARRIER(), PNGD_DEVICE_ST);
#undef PNGD_DEVICE_ST
}

}  // namespace

extern "C" int hoig_png_decode_u8(const uint8_t *bytes, int64_t nbytes, const hoig_png_decode_plan *plans_host,
                                  const hoig_png_decode_plan *plans_dev, int n, uint8_t *out, int64_t out_bytes, int32_t *status,
                                  void *workspace, int64_t workspace_bytes, int bgr, hoig_stream_t stream) {
    if (!bytes || !plans_host || !plans_dev || !out || !status || !workspace || n < 1) return HOIG_EINVAL;
    if ((nbytes & 15) || ((uintptr_t)bytes & 15) || ((uintptr_t)workspace & 15)) return HOIG_EINVAL;
    const int rc = pngd_check_batch(plans_host, n, nbytes, out_bytes, workspace_bytes);
    if (rc != HOIG_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    if (hoig_tuning(HOIG_TUNE_PNG_WINDOW) == 1) png_inflate_kernel<true><<<dim3((unsigned)n), PNGD_LANES, 0, st>>>(bytes, plans_dev, ws, status);
    else png_inflate_kernel<false><<<dim3((unsigned)n), PNGD_LANES, 0, st>>>(bytes, plans_dev, ws, status);
    HOIG_LAUNCH_CHECK();
    png_rows_kernel<<<dim3((unsigned)n), PNGD_ROWS, 0, st>>>(bytes, plans_dev, ws, out, status, bgr ? 1 : 0);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}
