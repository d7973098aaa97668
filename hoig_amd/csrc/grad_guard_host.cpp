// The host half of the gradient guard (grad_guard.h, docs/grad_guard.md): the workspace size, the constants the binding reads, and CPU
// twins that run the shared per-lane code with every workgroup walked thread by thread -- the same order in every sum, so the same
// bits.  No HIP call; host memory only.  Built with -ffp-contract=off.
#include "grad_guard.h"

namespace {

// the butterfly of the device's wave join: afterwards every entry holds what every lane holds there
gg_acc butterfly(gg_acc *v) {
    gg_acc t[GG_WAVE];
    for (int o = 32; o > 0; o >>= 1) {
        for (int l = 0; l < GG_WAVE; ++l) t[l] = gg_join(v[l], v[l ^ o]);
        memcpy(v, t, sizeof(t));
    }
    return v[0];
}

void store3(double *p, const gg_acc &a) { p[0] = a.s, p[1] = a.mx, p[2] = a.nf; }

gg_acc chunk_partial(const float *x, int64_t base, int cnt) {
    gg_acc w[GG_NT / GG_WAVE];
    for (int wave = 0; wave < GG_NT / GG_WAVE; ++wave) {
        gg_acc v[GG_WAVE];
        for (int l = 0; l < GG_WAVE; ++l) v[l] = gg_thread_chunk(x, base, cnt, wave * GG_WAVE + l);
        w[wave] = butterfly(v);
    }
    return gg_join(gg_join(gg_join(w[0], w[1]), w[2]), w[3]);
}

gg_acc piece_partial(const float *x, int64_t b, int64_t e) {
    gg_acc v[GG_WAVE];
    for (int l = 0; l < GG_WAVE; ++l) v[l] = gg_lane_piece(x, b, e, l);
    return butterfly(v);
}

gg_acc join_parts(const double *parts, int64_t first, int64_t last) {
    gg_acc r = gg_zero();
    for (int wave = 0; wave < GG_NT2 / GG_WAVE; ++wave) {
        gg_acc v[GG_WAVE];
        for (int l = 0; l < GG_WAVE; ++l) v[l] = gg_thread_parts(parts, first, last, wave * GG_WAVE + l);
        const gg_acc w = butterfly(v);
        r = wave == 0 ? w : gg_join(r, w);
    }
    return r;
}

}  // namespace

extern "C" int hoig_grad_stats_chunk(void) { return GG_CHUNK; }
extern "C" int hoig_grad_stats_max_grid(void) { return GG_MAX_GRID; }

extern "C" int64_t hoig_grad_stats_workspace_bytes(int64_t n, int nseg) { return gg_workspace_bytes(n, nseg); }

extern "C" int hoig_grad_stats_host(const float *x, int64_t n, const int64_t *segs, int nseg, double *seg_out, double *total,
                                    void *workspace) {
    if (!x || !total || !workspace || !gg_table_ok(n, segs, nseg) || (nseg > 0 && !seg_out)) return HOIG_EINVAL;
    const int64_t nchunk = gg_chunks(n);
    double *chunk_part = static_cast<double *>(workspace), *piece_part = chunk_part + 3 * nchunk;
    for (int64_t c = 0; c < nchunk; ++c) {
        const int64_t base = c * GG_CHUNK;
        const int cnt = (int)(n - base < GG_CHUNK ? n - base : GG_CHUNK);
        const int64_t end = base + cnt;
        const gg_acc tot = chunk_partial(x, base, cnt);
        store3(chunk_part + 3 * c, tot);
        for (int s = gg_first_row(segs, nseg, base); s < nseg; ++s) {
            const int64_t f = segs[2 * s];
            if (f >= end) break;
            const int64_t b = f > base ? f : base, e = f + segs[2 * s + 1] < end ? f + segs[2 * s + 1] : end;
            store3(piece_part + 3 * (c + s), b == base && e == end ? tot : piece_partial(x, b, e));
        }
    }
    store3(total, join_parts(chunk_part, 0, nchunk));
    for (int s = 0; s < nseg; ++s) {
        int64_t first, last;
        gg_row_slots(segs, s, nchunk, &first, &last);
        store3(seg_out + 3 * (int64_t)s, join_parts(piece_part, first, last));
    }
    return HOIG_OK;
}

extern "C" int hoig_guard_decide_host(const double *total, double pre_scale, double max_norm, int flags, float *guard, double *record) {
    if (!total || !guard || !record || (flags & ~HOIG_GUARD_SKIP) || !(pre_scale > 0.0) || !(max_norm >= 0.0)) return HOIG_EINVAL;
    gg_decide(total, pre_scale, max_norm, flags, guard, record);
    return HOIG_OK;
}
