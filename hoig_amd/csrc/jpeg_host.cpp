// Host half of the device JPEG decoder: the workspace layouts and the CPU twins of the two entropy kernels (serial inside a restart
// interval: jpeg_entropy.h; parallel inside it: jpeg_parallel.h).  Plain C++ with no HIP call (it also builds on its own, e.g. with
// -fsanitize=address for the corrupt-stream tests: tests/test_jpeg_cpu.py, tests/test_jpeg_par_cpu.py).
#include <string.h>

#include "jpeg_entropy.h"
#include "jpeg_parallel.h"

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

// the lanes of jpeg_parallel.h's workgroup, one after the other: every loop over "my lanes" covers all of them, a barrier is nothing
struct HostParCtx {
    const uint8_t *data;
    JpegParTab T;
    uint8_t byte(int pos) const { return data[pos]; }
    void stage(int, int) {}
    int first() const { return 0; }
    int step() const { return 1; }
    void barrier() {}
    bool any(bool v) const { return v; }
    JpegParTab *tab() { return &T; }
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

extern "C" int64_t hoig_jpeg_decode_par_workspace_bytes(hoig_jpeg_plan *plans, int n, int subseq_bytes) {
    if (subseq_bytes && !jpeg_par_subseq_ok(subseq_bytes)) return HOIG_EINVAL;
    const int64_t serial = hoig_jpeg_decode_workspace_bytes(plans, n);
    if (serial < 0) return serial;
    int64_t off, entries;
    jpeg_par_tables(plans, n, &off, &entries);
    return off + entries * (int64_t)sizeof(int32_t);
}

extern "C" int hoig_jpeg_entropy_par_host(const uint8_t *bytes, int64_t nbytes, const hoig_jpeg_plan *plans, int n, const int32_t *intervals,
                                          int64_t n_entries, int subseq_bytes, int lanes, void *coef, int64_t coef_bytes, int32_t *status,
                                          int32_t *rounds, int32_t *states, int64_t n_states) {
    if (!bytes || !plans || !intervals || !coef || !status || n <= 0 || nbytes < 0 || lanes < 1 || lanes > 65536) return HOIG_EINVAL;
    const int S = subseq_bytes ? subseq_bytes : HOIG_JPEG_SUBSEQ_BYTES;
    if (!jpeg_par_subseq_ok(S)) return HOIG_EINVAL;
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        const hoig_jpeg_plan &P = plans[i];
        if (!jpeg_plan_sane(P)) return HOIG_EUNSUPPORTED;
        if (P.data_off + P.data_len > nbytes || (int64_t)P.interval_first + P.n_intervals + 1 > n_entries) return HOIG_EINVAL;
        if (P.coef_off < 0 || P.coef_off % 16 || P.coef_off + jpeg_geometry(P).blocks * 128 > coef_bytes) return HOIG_EINVAL;
        for (int iv = 0; iv < P.n_intervals; ++iv) total += jpeg_par_nsub(P, intervals + P.interval_first, iv, S);
    }
    if (states && n_states < total) return HOIG_EINVAL;
    JpegHuff *tab = new JpegHuff[6];
    uint32_t *words = new uint32_t[(size_t)lanes * 7 + 8];
    HostParCtx px;
    px.T.state = words;
    px.T.cand = words + lanes;
    px.T.dirty = reinterpret_cast<int32_t *>(words + 2 * (size_t)lanes);
    px.T.nblk = px.T.dirty + lanes;
    px.T.dc0 = px.T.nblk + lanes;
    px.T.dc1 = px.T.dc0 + lanes;
    px.T.dc2 = px.T.dc1 + lanes;
    px.T.carry = px.T.dc2 + lanes;
    int64_t at = 0;
    for (int i = 0; i < n; ++i) {
        const hoig_jpeg_plan &P = plans[i];
        const int32_t *ivs = intervals + P.interval_first;
        status[i] = 0;
        if (rounds) rounds[i] = 0;
        bool ok = true;
        for (int c = 0; c < P.ncomp; ++c) {
            ok = jpeg_build_huff(P.dc_counts[c], P.dc_vals[c], 16, tab + c) && ok;
            ok = jpeg_build_huff(P.ac_counts[c], P.ac_vals[c], 256, tab + 3 + c) && ok;
        }
        int16_t *out = reinterpret_cast<int16_t *>(static_cast<char *>(coef) + P.coef_off);
        memset(out, 0, (size_t)jpeg_geometry(P).blocks * 128);
        if (!ok) status[i] = HOIG_JPEG_ECODE;
        HostCtx cx;
        cx.data = px.data = bytes + P.data_off;
        for (int iv = 0; iv < P.n_intervals; ++iv) {
            const int nsub = jpeg_par_nsub(P, ivs, iv, S);
            int32_t *st = states ? states + at * 4 : nullptr;
            if (st) memset(st, 0, (size_t)nsub * 4 * sizeof(int32_t));
            at += nsub;
            if (!ok) continue;
            int32_t r = 0;
            if (jpeg_par_interval(P, tab, tab + 3, ivs, iv, out, S, lanes, px, &r, st))
                status[i] |= jpeg_decode_interval(P, tab, tab + 3, ivs, iv, out, cx);
            if (rounds && r > rounds[i]) rounds[i] = r;
        }
    }
    delete[] words;
    delete[] tab;
    return HOIG_OK;
}
