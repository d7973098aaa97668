// Host half of the PNG decoder (png_inflate.h): the plan checks and the workspace layout, and the CPU twins of the two kernels of
// png_decode.hip -- the same per-lane code, a workgroup walked lane by lane and phase by phase.  Plain C++ with no HIP call (it also
// builds on its own under a host sanitizer).
#include <string.h>
#include <vector>

#include "png_inflate.h"

extern "C" int64_t hoig_png_decode_workspace_bytes(hoig_png_decode_plan *plans, int n) {
    if (!plans || n < 1) return HOIG_EINVAL;
    int64_t at = 0;
    for (int i = 0; i < n; ++i) {
        const int rc = pngd_plan_check(&plans[i]);
        if (rc != HOIG_OK) return rc;
        plans[i].filt_off = at;
        at += (pngd_expect(&plans[i]) + 15) / 16 * 16;
    }
    return at;
}

int pngd_check_batch(const hoig_png_decode_plan *plans, int n, int64_t nbytes, int64_t out_bytes, int64_t workspace_bytes) {
    for (int i = 0; i < n; ++i) {
        const hoig_png_decode_plan *p = &plans[i];
        const int rc = pngd_plan_check(p);
        if (rc != HOIG_OK) return rc;
        if (p->data_off + p->data_len > nbytes) return HOIG_EINVAL;
        if (p->color_type == 3 && p->pal_off + 3 * (int64_t)p->pal_entries > nbytes) return HOIG_EINVAL;
        if (p->out_off + (int64_t)p->width * p->height * 3 > out_bytes) return HOIG_EINVAL;
        if (p->filt_off < 0 || (p->filt_off & 15) || p->filt_off + pngd_expect(p) > workspace_bytes) return HOIG_EINVAL;
    }
    return HOIG_OK;
}

namespace {

#define PNGD_HOST_LANES(body) \
    for (int lane = 0; lane < PNGD_LANES; ++lane) { body; }
#define PNGD_HOST_ROW_LANES(body) \
    for (int lane = 0; lane < PNGD_ROWS; ++lane) { body; }

// one inflate workgroup: its LDS is a heap block of exactly the kernel's size
void inflate_image(const uint8_t *data, int64_t data_len, uint8_t *out, int64_t expect, int32_t *status) {
    PngdShared *sh = new PngdShared;
    PngdCtx c;
    c.sh = sh;
    c.data = data, c.data_len = data_len, c.out = out, c.expect = expect, c.status = status, c.ws_window = 0;
    PNGD_RUN_INFLATE(c, PNGD_HOST_LANES, (void)0, (void)0);
    delete sh;
}

void rows_image(const uint8_t *bytes, const hoig_png_decode_plan &p, uint8_t *ws, uint8_t *out, int32_t *status, int bgr) {
    PngdRowShared *sh = new PngdRowShared;
    std::vector<PngdLane> lanes(PNGD_ROWS);
    PngdRowCtx c;
    c.sh = sh;
    c.filt = ws + p.filt_off, c.out = out + p.out_off, c.pal = bytes + (p.color_type == 3 ? p.pal_off : 0);
    c.status = status;
    c.W = p.width, c.H = p.height, c.ctype = p.color_type, c.depth = p.bit_depth;
    c.bpp = pngd_bpp(p.color_type, p.bit_depth), c.rowbytes = (int32_t)pngd_rowbytes(p.width, p.color_type, p.bit_depth);
    c.units = c.rowbytes / c.bpp, c.pal_entries = p.pal_entries, c.bgr = bgr;
#define PNGD_HOST_ST(lane) lanes[lane]
    PNGD_RUN_ROWS(c, PNGD_HOST_ROW_LANES, (void)0, (void)0, PNGD_HOST_ST);
#undef PNGD_HOST_ST
    delete sh;
}

}  // namespace

extern "C" int hoig_png_inflate_host(const uint8_t *data, int64_t data_len, uint8_t *out, int64_t expect, int32_t *status) {
    if (!data || !status || data_len < 0 || expect < 0 || (expect > 0 && !out)) return HOIG_EINVAL;
    if (data_len >= ((int64_t)1 << 31) || expect >= ((int64_t)1 << 31)) return HOIG_EUNSUPPORTED;
    inflate_image(data, data_len, out, expect, status);
    return HOIG_OK;
}

extern "C" int hoig_png_decode_host(const uint8_t *bytes, int64_t nbytes, const hoig_png_decode_plan *plans, int n, uint8_t *out,
                                    int64_t out_bytes, int32_t *status, void *workspace, int64_t workspace_bytes, int bgr) {
    if (!bytes || !plans || !out || !status || !workspace || n < 1) return HOIG_EINVAL;
    const int rc = pngd_check_batch(plans, n, nbytes, out_bytes, workspace_bytes);
    if (rc != HOIG_OK) return rc;
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    for (int i = 0; i < n; ++i) inflate_image(bytes + plans[i].data_off, plans[i].data_len, ws + plans[i].filt_off, pngd_expect(&plans[i]), status + i);
    for (int i = 0; i < n; ++i) rows_image(bytes, plans[i], ws, out, status + i, bgr ? 1 : 0);
    return HOIG_OK;
}
