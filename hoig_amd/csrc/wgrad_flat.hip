// Weight gradient of the attention's VALID 5x5 convolutions (models/networks/extract_attn.py:18) on a FLATTENED pixel axis.
//
// dW[co][(r,s)][ci] = sum over output positions of dy[pos][co] * x[pos + (r,s)][ci].  wgrad_halo_bf16_kernel (wgrad_igemm_bf16.hip)
// does this on 2 x 32-pixel tiles, which needs an output width that is a multiple of 32: the source-side convolution's 36-wide
// output fell to the generic kernel (160 TFLOP/s: it re-gathers x for each of the 25 taps), and a 64-pixel tile pays a 6 x 36
// halo for 2 x 32 outputs.  Here the batch is ONE sequence of canvas positions q = (b, y, x) over the INPUT grid (pitch Wc = Wi):
// dy is placed on the canvas (zero where y >= Ho or x >= Wo), tap (r, s) reads x at q + r * Wc + s, a pixel tile is 128
// consecutive positions and its x halo 128 + 4 * (Wc + 1) positions (1.3x instead of 3.4x).  Everything else is the halo kernel's:
// a workgroup owns dW[64 co][25 taps][32 ci], ten waves = (32-channel group of co) x (tap row) with five accumulators each, both
// operands staged as they arrive ([position][channel], split to bf16) and read with ds_read_b64_tr_b16 (x rows 64 B apart: the
// four rows a 32-lane half reads are 256 contiguous bytes at every tap offset), pixel tiles split over blockIdx.y, fp32 atomics.
//
// wgrad_tile5_kernel (below): the same workgroup on 2-D pixel tiles, for the 72- and 136-wide maps whose flattened halo (676 positions
// at Wc = 136) is too large an image.
#include "conv_bf16_common.h"
#include "tuning.h"

namespace hoig_detail {
namespace {

typedef short s4_t __attribute__((ext_vector_type(4)));
constexpr int KS = 5, PTW = 128, BM = 64, BC = 32, NT = 640;
constexpr int PSTR = 192, QSTR = 64;                       // dy / x row strides in LDS (wgrad_halo_bf16_kernel)
constexpr int PSL = (PTW * 16 + NT - 1) / NT;              // dy float4s per thread (16 per position)
constexpr int QSL = 5;                                     // x float4s per thread: halo positions * 8 <= QSL * NT

__device__ __forceinline__ bf16x8 tr_frag(const unsigned char *a, int stride4) {
    const s4_t lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4_t *)a);
    const s4_t hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4_t *)(a + stride4));
    bf16x8 f;
    f[0] = lo4[0]; f[1] = lo4[1]; f[2] = lo4[2]; f[3] = lo4[3];
    f[4] = hi4[0]; f[5] = hi4[1]; f[6] = hi4[2]; f[7] = hi4[3];
    return f;
}

template <int NSX>
__global__ __launch_bounds__(NT) void wgrad_flat_kernel(const WFlatArgs p) {
    constexpr int NS = NSX == 1 ? 1 : 2, NB = NSX == 2 ? 2 : 1;      // operand planes: dy, x
    constexpr int PLANE_P = PTW * PSTR;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int HPOS = p.HPOS;                               // halo positions of a tile: PTW + (KS-1) * (Wc + 1)
    const int PLANE_Q = (HPOS * QSTR + 255) / 256 * 256;
    unsigned char *Ph = smem, *Pl = smem + PLANE_P;
    unsigned char *Qh = smem + NS * PLANE_P, *Ql = Qh + PLANE_Q;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cb = wave & 1, tr = wave >> 1;               // 32-channel group of co, tap row
    const int tile = hoig_xcd_remap(blockIdx.x, p.nblk);
    const int c0 = (tile / p.nblk_ci) * BM, ci0 = (tile % p.nblk_ci) * BC;
    const int mt_begin = blockIdx.y * p.mt_per_split;
    const int mt_end = min(p.n_mtiles, mt_begin + p.mt_per_split);

    float4 rp[PSL], rq[QSL];
    const bool do_bias = p.DB != nullptr && ci0 == 0;
    float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
    auto load_tiles = [&](int mt) {
        const int q0 = mt * PTW;
#pragma unroll
        for (int i = 0; i < PSL; ++i) {
            const int idx = tid + NT * i;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (idx < PTW * 16) {
                const int q = q0 + (idx >> 4), c4 = idx & 15;
                if (q < p.Q) {
                    const int b = q / p.HWc, rem = q - b * p.HWc;
                    const int y = rem / p.Wc, x = rem - y * p.Wc;
                    if (y < p.Ho && x < p.Wo)
                        v = *reinterpret_cast<const float4 *>(p.DY + ((size_t)(b * p.Ho + y) * p.Wo + x) * p.Co + c0 + c4 * 4);
                }
            }
            rp[i] = v;       // (the bias sum takes it in store_tiles: wgrad_igemm_bf16.hip, load_tiles)
        }
#pragma unroll
        for (int i = 0; i < QSL; ++i) {
            const int idx = tid + NT * i;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            const int q = q0 + (idx >> 3);
            if ((idx >> 3) < HPOS && q < p.Q) v = *reinterpret_cast<const float4 *>(p.X + (size_t)q * p.Ci + ci0 + (idx & 7) * 4);
            rq[i] = v;
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int i = 0; i < PSL; ++i) {
            const int idx = tid + NT * i;
            if (do_bias) {                 // this thread always holds the same four channels (NT % 16 == 0); idle slices hold zeros
                bsum.x += rp[i].x; bsum.y += rp[i].y; bsum.z += rp[i].z; bsum.w += rp[i].w;
            }
            if (idx < PTW * 16) {
                uint2 hi, lo;
                split4(rp[i], hi, lo);
                const int off = (idx >> 4) * PSTR + (idx & 15) * 8;
                *reinterpret_cast<uint2 *>(Ph + off) = hi;
                if (NS == 2) *reinterpret_cast<uint2 *>(Pl + off) = lo;
            }
        }
#pragma unroll
        for (int i = 0; i < QSL; ++i) {
            const int idx = tid + NT * i;
            if ((idx >> 3) < HPOS) {
                uint2 hi, lo;
                split4(rq[i], hi, lo);
                *reinterpret_cast<uint2 *>(Qh + idx * 8) = hi;
                if (NB == 2) *reinterpret_cast<uint2 *>(Ql + idx * 8) = lo;
            }
        }
    };

    // transpose-read addressing (wgrad_bf16_kernel): 16-lane group g, lane 4q+c -> row 8*(g>>1)+q, channels 16*(g&1)+4c
    const int grp = lane >> 4, li = lane & 15;
    const int trow = (grp >> 1) * 8 + (li >> 2), tch = ((grp & 1) * 16 + (li & 3) * 4) * 2;
    const int trP = trow * PSTR + tch + cb * 64, trQ = (trow + tr * p.Wc) * QSTR + tch;

    f32x16 acc[KS];
#pragma unroll
    for (int t = 0; t < KS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    if (mt_begin < mt_end) {
        load_tiles(mt_begin);
        store_tiles();
    }
    __syncthreads();
    for (int mt = mt_begin; mt < mt_end; ++mt) {
        const bool nxt = mt + 1 < mt_end;
        if (nxt) load_tiles(mt + 1);
#pragma unroll
        for (int kk = 0; kk < PTW / 16; ++kk) {            // 16 consecutive positions per k-step
            const bf16x8 ah = tr_frag(Ph + trP + kk * 16 * PSTR, 4 * PSTR);
            bf16x8 al;
            if (NS == 2) al = tr_frag(Pl + trP + kk * 16 * PSTR, 4 * PSTR);
            bf16x8 bh[KS], bl[KS];
#pragma unroll
            for (int t = 0; t < KS; ++t) {
                const int qoff = trQ + (kk * 16 + t) * QSTR;
                bh[t] = tr_frag(Qh + qoff, 4 * QSTR);
                if (NB == 2) bl[t] = tr_frag(Ql + qoff, 4 * QSTR);
            }
            // term-major: the KS accumulators take turns, so no MFMA waits on the one issued just before it
            if (NS == 2) {
#pragma unroll
                for (int t = 0; t < KS; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[t], acc[t], 0, 0, 0);
            }
            if (NB == 2) {
#pragma unroll
                for (int t = 0; t < KS; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[t], acc[t], 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < KS; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[t], acc[t], 0, 0, 0);
        }
        __syncthreads();                      // every wave is done reading the stage
        if (nxt) store_tiles();
        __syncthreads();
    }

    if (do_bias) {                         // the threads that hold partial sums of the same four channels combine in LDS
        float *red = reinterpret_cast<float *>(smem);          // (the tiles are dead: the loop ended with a barrier)
        if (tid < BM) red[tid] = 0.f;
        __syncthreads();
        const int ch = (tid & 15) * 4;
        atomicAdd(&red[ch + 0], bsum.x);
        atomicAdd(&red[ch + 1], bsum.y);
        atomicAdd(&red[ch + 2], bsum.z);
        atomicAdd(&red[ch + 3], bsum.w);
        __syncthreads();
        if (tid < BM) atomicAdd(&p.DB[c0 + tid], red[tid]);
    }
    const int l31 = lane & 31, lh = lane >> 5;
    const int K = KS * KS * p.Ci;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = c0 + cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        float *row = p.DW + (size_t)co * K + (tr * KS) * p.Ci + ci0 + l31;
#pragma unroll
        for (int t = 0; t < KS; ++t) atomicAdd(row + t * p.Ci, acc[t][r]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same weight gradient on 2-D pixel tiles (tuning key `halo5`): a tile is 8 rows x 16 columns of ONE image's output grid, its x halo
// 12 x 20 = 240 positions (1.9x the tile; the flattened axis needs 128 + 4 * (Wc + 1) = 676 at Wc = 136 and launch_wgrad_flat5 declines
// above Wc = 66, which left the 72- and 136-wide layers to the generic register kernels at 165 TFLOP/s).  A k-step is one tile row: its 16
// dy positions are 16 consecutive rows of the dy image, and tap (r, s) reads 16 consecutive rows of the halo image at (row + r) * 20 + s.
// Workgroup tile (dW[64 co][25 taps][32 ci]), waves, transpose reads, bias sum, pixel splits and atomics are wgrad_flat_kernel's.
// Both images are DOUBLE-BUFFERED (the halo is small): the next tile is fetched in two halves, each stored into the other buffer half a
// tile later, so that at most 16 staging registers are live beside the 80 accumulators (the flattened kernel holds 36 through a whole
// tile and spills), and a tile costs one barrier.  Thread -> (row, column, channels) is chosen so that a slice is a fixed stride from
// the previous one: dy 512 threads x 4 slices of two tile rows, x 640 threads x 3 slices of four halo rows.
constexpr int TROWS = PTW / 16, THW = 16 + KS - 1, THPOS = (TROWS + KS - 1) * THW;
constexpr int TPLANE_P = PTW * PSTR, TPLANE_Q = THPOS * QSTR;
constexpr int TPSL = 4, TQSL = 3;
static_assert(TPSL * 512 == PTW * 16 && TQSL * NT == THPOS * 8, "slices cover the two images exactly");
constexpr int tile5_lds(int nsx) { return 2 * (ns_a(nsx) * TPLANE_P + ns_b(nsx) * TPLANE_Q); }

template <int NSX>
__global__ __launch_bounds__(NT) void wgrad_tile5_kernel(const WFlatArgs p) {      // p.Wc / p.HWc: tiles per tile row / per image
    constexpr int NS = NSX == 1 ? 1 : 2, NB = NSX == 2 ? 2 : 1;      // operand planes: dy, x
    constexpr int PBUF = NS * TPLANE_P, QBUF = NB * TPLANE_Q;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];      // P[2][PBUF], Q[2][QBUF]
    unsigned char *const Qbase = smem + 2 * PBUF;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cb = wave & 1, tr = wave >> 1;               // 32-channel group of co, tap row
    const int tile = hoig_xcd_remap(blockIdx.x, p.nblk);
    const int c0 = (tile / p.nblk_ci) * BM, ci0 = (tile % p.nblk_ci) * BC;
    const int mt_begin = blockIdx.y * p.mt_per_split;
    const int mt_end = min(p.n_mtiles, mt_begin + p.mt_per_split);
    const int Hi = p.Ho + KS - 1, Wi = p.Wo + KS - 1;

    // dy: tile row (tid >> 8) + 2 i, column (tid >> 4) & 15, channels 4 (tid & 15) ..; x: halo row tid / 160 + 4 i, column, channels
    const bool p_on = tid < 512;
    const int prow = tid >> 8, pcol = (tid >> 4) & 15;
    const int qrow = tid / (THW * 8), qcol = (tid - qrow * (THW * 8)) >> 3;
    const int p_goff = (prow * p.Wo + pcol) * p.Co + c0 + (tid & 15) * 4, p_gstep = 2 * p.Wo * p.Co;
    const int q_goff = (qrow * Wi + qcol) * p.Ci + ci0 + (tid & 7) * 4, q_gstep = 4 * Wi * p.Ci;
    const int p_lds = (prow * 16 + pcol) * PSTR + (tid & 15) * 8, q_lds = tid * 8;

    float4 rp[TPSL], rq[TQSL];
    const bool do_bias = p.DB != nullptr && ci0 == 0;
    float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
    auto load_part = [&](int mt, int half) {               // half 0: rp[0..1], rq[0..1]; half 1: rp[2..3], rq[2]
        const int b = mt / p.HWc, rem = mt - b * p.HWc;
        const int ty = rem / p.Wc, y0 = ty * TROWS, x0 = (rem - ty * p.Wc) * 16;
        const float *dyt = p.DY + ((size_t)(b * p.Ho + y0) * p.Wo + x0) * p.Co;
        const float *xt = p.X + ((size_t)(b * Hi + y0) * Wi + x0) * p.Ci;
        const bool pc_ok = p_on && x0 + pcol < p.Wo, qc_ok = x0 + qcol < Wi;
#pragma unroll
        for (int i = 0; i < TPSL; ++i)
            if ((i >> 1) == half)
                rp[i] = (pc_ok && y0 + prow + 2 * i < p.Ho) ? *reinterpret_cast<const float4 *>(dyt + p_goff + i * p_gstep)
                                                            : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < TQSL; ++i)
            if ((i >> 1) == half)
                rq[i] = (qc_ok && y0 + qrow + 4 * i < Hi) ? *reinterpret_cast<const float4 *>(xt + q_goff + i * q_gstep)
                                                          : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto store_part = [&](int buf, int half) {
        unsigned char *Ph = smem + buf * PBUF, *Pl = Ph + TPLANE_P;
        unsigned char *Qh = Qbase + buf * QBUF, *Ql = Qh + TPLANE_Q;
#pragma unroll
        for (int i = 0; i < TPSL; ++i)
            if ((i >> 1) == half) {
                if (do_bias) {             // this thread always holds the same four channels; idle threads and positions hold zeros
                    bsum.x += rp[i].x; bsum.y += rp[i].y; bsum.z += rp[i].z; bsum.w += rp[i].w;
                }
                if (p_on) {
                    uint2 hi, lo;
                    split4(rp[i], hi, lo);
                    const int off = p_lds + i * (2 * 16 * PSTR);
                    *reinterpret_cast<uint2 *>(Ph + off) = hi;
                    if (NS == 2) *reinterpret_cast<uint2 *>(Pl + off) = lo;
                }
            }
#pragma unroll
        for (int i = 0; i < TQSL; ++i)
            if ((i >> 1) == half) {
                uint2 hi, lo;
                split4(rq[i], hi, lo);
                const int off = q_lds + i * (NT * 8);
                *reinterpret_cast<uint2 *>(Qh + off) = hi;
                if (NB == 2) *reinterpret_cast<uint2 *>(Ql + off) = lo;
            }
    };

    // transpose-read addressing (wgrad_bf16_kernel): 16-lane group g, lane 4q+c -> row 8*(g>>1)+q, channels 16*(g&1)+4c
    const int grp = lane >> 4, li = lane & 15;
    const int trow = (grp >> 1) * 8 + (li >> 2), tch = ((grp & 1) * 16 + (li & 3) * 4) * 2;
    const int trP = trow * PSTR + tch + cb * 64, trQ = (trow + tr * THW) * QSTR + tch;

    f32x16 acc[KS];
#pragma unroll
    for (int t = 0; t < KS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    auto compute = [&](int buf, int kk) {                  // tile row kk: 16 positions per k-step
        const unsigned char *Ph = smem + buf * PBUF, *Pl = Ph + TPLANE_P;
        const unsigned char *Qh = Qbase + buf * QBUF, *Ql = Qh + TPLANE_Q;
        const bf16x8 ah = tr_frag(Ph + trP + kk * 16 * PSTR, 4 * PSTR);
        bf16x8 al;
        if (NS == 2) al = tr_frag(Pl + trP + kk * 16 * PSTR, 4 * PSTR);
        bf16x8 bh[KS];
#pragma unroll
        for (int t = 0; t < KS; ++t) bh[t] = tr_frag(Qh + trQ + (kk * THW + t) * QSTR, 4 * QSTR);
        // term-major: the KS accumulators take turns, so no MFMA waits on the one issued just before it
        if (NB == 2) {                       // (the x lo fragments first and on their own: five fragment registers fewer are live)
#pragma unroll
            for (int t = 0; t < KS; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, tr_frag(Ql + trQ + (kk * THW + t) * QSTR, 4 * QSTR), acc[t], 0, 0, 0);
        }
        if (NS == 2) {
#pragma unroll
            for (int t = 0; t < KS; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[t], acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < KS; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[t], acc[t], 0, 0, 0);
    };

    if (mt_begin < mt_end) {
        load_part(mt_begin, 0);
        load_part(mt_begin, 1);
        store_part(0, 0);
        store_part(0, 1);
    }
    __syncthreads();
    int buf = 0;
#pragma unroll 1
    for (int mt = mt_begin; mt < mt_end; ++mt) {
        const bool nxt = mt + 1 < mt_end;
        if (nxt) load_part(mt + 1, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < TROWS / 2; ++kk) compute(buf, kk);
        __builtin_amdgcn_sched_barrier(0);
        if (nxt) {                            // (the other buffer: nobody reads it before the barrier below)
            store_part(buf ^ 1, 0);
            load_part(mt + 1, 1);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = TROWS / 2; kk < TROWS; ++kk) compute(buf, kk);
        __builtin_amdgcn_sched_barrier(0);
        if (nxt) store_part(buf ^ 1, 1);
        __syncthreads();
        buf ^= 1;
    }

    if (do_bias) {                         // the threads that hold partial sums of the same four channels combine in LDS
        float *red = reinterpret_cast<float *>(smem);          // (the tiles are dead: the loop ended with a barrier)
        if (tid < BM) red[tid] = 0.f;
        __syncthreads();
        const int ch = (tid & 15) * 4;
        atomicAdd(&red[ch + 0], bsum.x);
        atomicAdd(&red[ch + 1], bsum.y);
        atomicAdd(&red[ch + 2], bsum.z);
        atomicAdd(&red[ch + 3], bsum.w);
        __syncthreads();
        if (tid < BM) atomicAdd(&p.DB[c0 + tid], red[tid]);
    }
    const int l31 = lane & 31, lh = lane >> 5;
    const int K = KS * KS * p.Ci;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = c0 + cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        float *row = p.DW + (size_t)co * K + (tr * KS) * p.Ci + ci0 + l31;
#pragma unroll
        for (int t = 0; t < KS; ++t) atomicAdd(row + t * p.Ci, acc[t][r]);
    }
}

// `a`: as launch_wgrad_flat5 filled it in (nblk, nblk_ci, Ho, Wo)
int launch_wgrad_tile5(WFlatArgs a, int Bn, int ns, hipStream_t st) {
    a.Wc = (int)hoig_cdiv(a.Wo, 16);
    a.HWc = a.Wc * (int)hoig_cdiv(a.Ho, TROWS);
    a.n_mtiles = Bn * a.HWc;
    int splits = (int)hoig_cdiv(256, a.nblk);           // every pixel split costs |dW| fp32 atomics: one round of workgroups
    if (splits > a.n_mtiles) splits = a.n_mtiles;
    a.mt_per_split = (int)hoig_cdiv(a.n_mtiles, splits);
    splits = (int)hoig_cdiv(a.n_mtiles, a.mt_per_split);
    static_assert(tile5_lds(2) <= 160 * 1024, "both double-buffered images must fit in LDS");
    dim3 grid(a.nblk, splits);
    HOIG_ROUTE_W(wgrad_tile5);
    HOIG_NS_SWITCH(ns, return hoig_launch<wgrad_tile5_kernel<NSX>, tile5_lds(NSX)>(grid, NT, tile5_lds(NSX), st, a));
    return HOIG_EINVAL;
}

}  // namespace

// dW (and the bias gradient) of a valid 5x5 stride-1 convolution: x [Bn][Hi][Wi][Ci], dy [Bn][Hi-4][Wi-4][Co]
int launch_wgrad_flat5(const float *x, const float *dy, float *dw, float *dbias, int Bn, int Hi, int Wi, int Ci, int Co, int ns,
                       hipStream_t st) {
    if (Co % 64 || Ci % 32 || Hi < 5 || Wi < 5) return HOIG_EUNSUPPORTED;
    WFlatArgs a;
    a.X = x; a.DY = dy; a.DW = dw; a.DB = dbias;
    a.Ci = Ci; a.Co = Co; a.Wc = Wi; a.HWc = Hi * Wi; a.Q = Bn * Hi * Wi; a.Ho = Hi - 4; a.Wo = Wi - 4;
    a.HPOS = PTW + (KS - 1) * (Wi + 1);
    a.nblk_ci = Ci / 32;
    a.nblk = (Co / 64) * a.nblk_ci;
    if (a.HPOS * 8 > QSL * NT)                          // canvas too wide for one halo image (Wi > 66): 2-D tiles (key halo5 = 0: declined)
        return hoig_tuning(HOIG_TUNE_HALO5) != 0 ? launch_wgrad_tile5(a, Bn, ns, st) : HOIG_EUNSUPPORTED;
    a.n_mtiles = (int)hoig_cdiv(a.Q, PTW);
    int splits = (int)hoig_cdiv(256, a.nblk);           // every pixel split costs |dW| fp32 atomics: one round of workgroups
    if (splits > a.n_mtiles) splits = a.n_mtiles;
    if (splits < 1) splits = 1;
    a.mt_per_split = (int)hoig_cdiv(a.n_mtiles, splits);
    splits = (int)hoig_cdiv(a.n_mtiles, a.mt_per_split);
    const int shm = ns_a(ns) * PTW * PSTR + ns_b(ns) * ((a.HPOS * QSTR + 255) / 256 * 256);
    dim3 grid(a.nblk, splits);
    HOIG_ROUTE_W(wgrad_flat5);
    HOIG_NS_SWITCH(ns, return hoig_launch<wgrad_flat_kernel<NSX>, 128 * 1024>(grid, NT, shm, st, a));
    return HOIG_EINVAL;
}

}  // namespace hoig_detail
