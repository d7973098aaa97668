// Host half of the device JPEG decoder: the workspace layout and the CPU twin of the entropy kernel.  Plain C++ with no HIP call (it
// also builds on its own, e.g. with -fsanitize=address for the corrupt-stream tests: tests/test_jpeg_cpu.py).
#include <string.h>

#include "jpeg_entropy.h"

static_assert(sizeof(hoig_jpeg_plan) == 1376, "hoig_amd/data/jpeg.py restates this layout as a numpy dtype");

namespace {

struct HostCtx {
    const uint8_t *data;   // the image's scan data
    int16_t blk[64];
    uint8_t byte(int pos) const { return data[pos]; }
    void window(int) {}
    int16_t *stage() {
        memset(blk, 0, sizeof blk);
        return blk;
    }
    bool decoder() const { return true; }
    int share(int v) const { return v; }
    void flush(int16_t *dst) const {
        for (int k = 0; k < 64; ++k) dst[jpeg_natural(k)] = blk[k];
    }
};

}  // namespace

extern "C" int64_t hoig_jpeg_decode_workspace_bytes(hoig_jpeg_plan *plans, int n) {
    if (!plans || n <= 0) return HOIG_EINVAL;
    int64_t at = 0;
    for (int i = 0; i < n; ++i) {
        if (!jpeg_plan_sane(plans[i])) return HOIG_EUNSUPPORTED;
        plans[i].coef_off = at;
        at += jpeg_geometry(plans[i]).blocks * 128;
    }
    for (int i = 0; i < n; ++i) {
        plans[i].plane_off = at;
        at += jpeg_geometry(plans[i]).blocks * 64;
    }
    return at;
}

extern "C" int hoig_jpeg_entropy_host(const uint8_t *bytes, int64_t nbytes, const hoig_jpeg_plan *plans, int n, const int32_t *intervals,
                                      int64_t n_entries, void *coef, int64_t coef_bytes, int32_t *status) {
    if (!bytes || !plans || !intervals || !coef || !status || n <= 0 || nbytes < 0) return HOIG_EINVAL;
    for (int i = 0; i < n; ++i) {
        const hoig_jpeg_plan &P = plans[i];
        if (!jpeg_plan_sane(P)) return HOIG_EUNSUPPORTED;
        if (P.data_off + P.data_len > nbytes || (int64_t)P.interval_first + P.n_intervals + 1 > n_entries) return HOIG_EINVAL;
        if (P.coef_off < 0 || P.coef_off % 16 || P.coef_off + jpeg_geometry(P).blocks * 128 > coef_bytes) return HOIG_EINVAL;
    }
    JpegHuff *tab = new JpegHuff[6];
    for (int i = 0; i < n; ++i) {
        const hoig_jpeg_plan &P = plans[i];
        status[i] = 0;
        bool ok = true;
        for (int c = 0; c < P.ncomp; ++c) {
            ok = jpeg_build_huff(P.dc_counts[c], P.dc_vals[c], 16, tab + c) && ok;
            ok = jpeg_build_huff(P.ac_counts[c], P.ac_vals[c], 256, tab + 3 + c) && ok;
        }
        if (!ok) {
            status[i] = HOIG_JPEG_ECODE;
            continue;
        }
        HostCtx cx;
        cx.data = bytes + P.data_off;
        int16_t *out = reinterpret_cast<int16_t *>(static_cast<char *>(coef) + P.coef_off);
        for (int iv = 0; iv < P.n_intervals; ++iv)
            status[i] |= jpeg_decode_interval(P, tab, tab + 3, intervals + P.interval_first, iv, out, cx);
    }
    delete[] tab;
    return HOIG_OK;
}
