// VALID 5x5 stride-1 convolutions over WIDE maps and their data gradients, on v_mfma_f32_16x16x32, with an LDS-resident input halo of
// a 2-D tile: the attention's 136 -> 132 -> 128 and 72 -> 68 -> 64 pixel wide layers (models/networks/extract_attn.py:18), whose halo
// on the flattened pixel axis of conv_flat16.hip (256 + 4 * (Wc + 1) positions: 804 at Wc = 136) does not fit in LDS.
//
// A workgroup owns a 16 x 16 pixel tile of one image x 128 output channels; per 32-channel block it stages the 20 x 20 canvas
// positions its taps touch ONCE (split to 16-bit hi / lo planes, the two-half-image layout of conv_halo16.hip), every tap reads its
// fragments out of that image at the offset (r * 20 + s) * 32 B, and only the weight tiles stream: three or five taps per step
// (taps_per_step), double-buffered, by LDS-DMA.  Step walk, fragment pipeline, swapped operand roles (a lane stores four consecutive channels) and the
// split-K permlane epilogue are those of conv_flat_m16_kernel; the geometry is FlatArgs':
//
//   forward      : canvas = the input grid, source = x, outputs kept for y < Ho, x < Wo (partial tiles on both edges);
//   data gradient: canvas = the input grid, source = dy placed at offset (4, 4) (zero elsewhere), taps flipped: every canvas
//                  position is an output.
// A 16-pixel column granule wastes 8 % of a 132-wide and 15 % of a 68-wide output; 8 x 32 tiles (432 halo pixels) would waste 21 % /
// 41 %, 4 x 64 (544 halo pixels) more.
#include "conv_bf16_common.h"
#include "conv_m16_common.h"
#include "tuning.h"

namespace hoig_detail {
namespace {

typedef unsigned u2_t __attribute__((ext_vector_type(2)));

constexpr int KS = 5, KK = 25, TS = 16, HW = TS + KS - 1, HPIX = HW * HW;      // tile side, halo side, halo pixels
constexpr int BN = 128, NT = 512;                                              // channels per workgroup, threads
constexpr int HSL = (HPIX * 8 + NT - 1) / NT;                                  // halo slices (4 channels of a pixel) per thread
constexpr int PHALF = HPIX * 32, P23 = round128(PHALF) + 64, PLANE_P = round128(P23 + PHALF);
constexpr int W23 = BN * 32 + 64, PLANE_W = round128(W23 + BN * 32);
constexpr int ngrp(int tps) { return (KK + tps - 1) / tps; }                   // steps per channel block at `tps` taps per step
// one weight plane per tap (NSX 1 and 3: the two-term data gradients of the step): a whole TAP ROW per step, five steps per channel
// block and 135 KB of LDS -- 4 % faster on all four data gradients than three taps per step (217 -> 209, 141 -> 135, 216 -> 207,
// 140 -> 135 us); two weight planes (NSX 2: the three-term forward): three taps, nine steps, the last of one tap, 151 KB -- four do not fit
constexpr int taps_per_step(int nsx) { return ns_b(nsx) == 1 ? 5 : 3; }
constexpr size_t lds_bytes(int nsx, int tps) { return (size_t)ns_a(nsx) * PLANE_P + 2 * tps * ns_b(nsx) * PLANE_W; }

template <int NSX, bool F16, bool SPLITK, int TPS>
__global__ __launch_bounds__(NT) void conv_halo5_m16_kernel(const FlatArgs p) {
    constexpr int NS = NSX == 1 ? 1 : 2, NB = NSX == 2 ? 2 : 1;
    constexpr int NGRP = ngrp(TPS);
    constexpr int WN = 2, MT = 4, NTW = 4;                // a wave: 4 tile rows of 16 pixels x 4 channel tiles of 16
    constexpr int BBUF = TPS * NB * PLANE_W;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *Ph = smem, *Pl = smem + PLANE_P;
    unsigned char *Wbase = smem + NS * PLANE_P;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lg = lane >> 4;
    const int wm = wave / WN, wn = wave % WN;
    const int tile = hoig_xcd_remap(blockIdx.x, p.nblk);
    const int n_mt = p.nblk / p.nblk_n;
    int mt_ = tile % n_mt;
    const int n0 = (tile / n_mt) * BN;                    // channel-tile major: an XCD streams few weight tiles
    const int tiles_x = (p.Wd + TS - 1) / TS, tiles_y = (p.Hd + TS - 1) / TS;
    const int tx_ = mt_ % tiles_x;
    mt_ /= tiles_x;
    const int ty_ = mt_ % tiles_y, b = mt_ / tiles_y;
    const int y0 = ty_ * TS, x0 = tx_ * TS;
    // split over K: this workgroup multiplies steps [s_begin, s_end) of the (channel block, tap group) walk
    const int s_begin = blockIdx.y * p.steps_per_split, s_end = min((p.Cg >> 5) * NGRP, s_begin + p.steps_per_split);

    // halo: thread -> (halo pixel h, 4-channel group c4); the source offset of a pixel does not depend on the channel block
    int src_off[HSL];
#pragma unroll
    for (int sl = 0; sl < HSL; ++sl) {
        const int i = tid + NT * sl, h = i >> 3;
        int off = -1;
        if (h < HPIX) {
            const int hy = h / HW, hx = h - hy * HW;
            const int sy = y0 + hy - p.oy, sx = x0 + hx - p.ox;
            if (sy >= 0 && sy < p.Hs && sx >= 0 && sx < p.Ws) off = ((b * p.Hs + sy) * p.Ws + sx) * p.Cg + (i & 7) * 4;
        }
        src_off[sl] = off;
    }
    int wread[NTW], pread[MT];
#pragma unroll
    for (int j = 0; j < NTW; ++j) wread[j] = (lg >> 1) * W23 + (wn * (NTW * 16) + j * 16 + l15) * 32 + (lg & 1) * 16;
#pragma unroll
    for (int m = 0; m < MT; ++m) pread[m] = (lg >> 1) * P23 + ((wm * MT + m) * HW + l15) * 32 + (lg & 1) * 16;

    f32x4 acc[NTW][MT];
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[j][m] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int T = s_end - s_begin;                        // step = (channel block, group of TPS taps)
    // weight tiles by LDS-DMA (dma_piece of conv_halo16.hip): piece q of a step = (tap t of the group, plane, 32-row block, half
    // image); wave w issues pieces w, w + 8, ..
    constexpr int NPIECE_STEP = TPS * NB * (BN / 32) * 2, NPW = (NPIECE_STEP + 7) / 8;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const unsigned lds_w0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)Wbase);
    const int drow = lane >> 1;
    const unsigned dlane0 = drow * 32 + (((0 + (lane & 1)) ^ ((drow >> 2) & 3)) << 3);
    const unsigned dlane1 = drow * 32 + (((2 + (lane & 1)) ^ ((drow >> 2) & 3)) << 3);
    auto dma_piece = [&](int step, int buf, int i) {
        const int q = wave_u + 8 * i;
        if (q >= NPIECE_STEP) return;
        const int h = q & 1, blk = (q >> 1) % (BN / 32), tp = (q >> 1) / (BN / 32);
        const int t = tp / NB, pl = tp - t * NB;
        const int cb = (s_begin + step) / NGRP, g = (s_begin + step) % NGRP;
        const int tap = min(g * TPS + t, KK - 1);
        const int wtap = p.flip ? (KK - 1 - tap) : tap;
        const size_t koff = (size_t)(wtap * p.Cg + cb * 32) * 32;
        const unsigned short *src = (pl ? p.Wl : p.Wh) + ((size_t)((n0 >> 5) + blk) * (p.K >> 5)) * 1024 + koff + (h ? dlane1 : dlane0);
        const unsigned to = __builtin_amdgcn_readfirstlane(lds_w0 + buf * BBUF + tp * PLANE_W + h * W23 + blk * 1024);
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(src), "s"(to) : "memory");
    };
    float4 hreg[HSL];
    auto halo_load = [&](int cb) {
#pragma unroll
        for (int sl = 0; sl < HSL; ++sl)
            hreg[sl] = src_off[sl] >= 0 ? *reinterpret_cast<const float4 *>(p.A + (size_t)src_off[sl] + cb * 32)
                                        : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto halo_store = [&]() {
#pragma unroll
        for (int sl = 0; sl < HSL; ++sl) {
            const int i = tid + NT * sl, h = i >> 3, c4 = i & 7;
            if (h < HPIX) {
                uint2 hi, lo;
                split4t<F16>(hreg[sl], hi, lo);
                const int off = (c4 >> 2) * P23 + h * 32 + (c4 & 3) * 8;
                *reinterpret_cast<uint2 *>(Ph + off) = hi;
                if (NS == 2) *reinterpret_cast<uint2 *>(Pl + off) = lo;
            }
        }
    };
    struct PF {
        bf16x8 h[MT], l[MT];
    };
    struct WF {
        bf16x8 h, l;
    };
    // a group = (tap, channel tile): its weight fragments against the tap's eight pixel fragments (read once per tap); the
    // fragments of the next group, and a quarter of the next tap's pixel fragments, are read before this group's MFMAs issue
    auto compute = [&](int g, int bbuf, int dma_step) {
        const unsigned char *Wst = Wbase + bbuf * BBUF;
        const int ntap = min(TPS, KK - g * TPS);
        int tapoff[TPS];
#pragma unroll
        for (int t = 0; t < TPS; ++t) {
            const int tap = min(g * TPS + t, KK - 1), r = tap / KS, s_ = tap - r * KS;
            tapoff[t] = (r * HW + s_) * 32;
        }
        auto read_p = [&](PF &f, int t, int m) {
            f.h[m] = *reinterpret_cast<const bf16x8 *>(Ph + pread[m] + tapoff[t]);
            if (NS == 2) f.l[m] = *reinterpret_cast<const bf16x8 *>(Pl + pread[m] + tapoff[t]);
        };
        auto read_w = [&](WF &f, int t, int j) {
            const unsigned char *Wh = Wst + t * NB * PLANE_W, *Wl = Wh + PLANE_W;
            f.h = *reinterpret_cast<const bf16x8 *>(Wh + wread[j]);
            if (NB == 2) f.l = *reinterpret_cast<const bf16x8 *>(Wl + wread[j]);
        };
        PF pf[2];
        WF wf[2];
#pragma unroll
        for (int m = 0; m < MT; ++m) read_p(pf[0], 0, m);
        read_w(wf[0], 0, 0);
#pragma unroll
        for (int t = 0; t < TPS; ++t) {
            if (t >= ntap) break;                              // (the last group of a channel block holds KK % TPS taps)
#pragma unroll
            for (int j = 0; j < NTW; ++j) {
                const int gi = t * NTW + j;
                if (gi + 1 < TPS * NTW) read_w(wf[(gi + 1) & 1], (gi + 1) / NTW, (gi + 1) % NTW);
                if (t + 1 < TPS) read_p(pf[(t + 1) & 1], t + 1, j);
                if (dma_step >= 0 && gi < NPW) dma_piece(dma_step, bbuf ^ 1, gi);
                __builtin_amdgcn_sched_barrier(0);
                const PF &pc = pf[t & 1];
                const WF &wc = wf[gi & 1];
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    if (SPLITK) {
                        if (NS == 2) acc[j][m] = mfma_m16<F16>(pc.l[m], wc.h, acc[j][m]);
                        if (NB == 2) acc[j][m] = mfma_m16<F16>(pc.h[m], wc.l, acc[j][m]);
                        acc[j][m] = mfma_m16<F16>(pc.h[m], wc.h, acc[j][m]);
                    } else {
                        if (NS == 2) acc[j][m] = mfma_m16<F16>(wc.h, pc.l[m], acc[j][m]);
                        if (NB == 2) acc[j][m] = mfma_m16<F16>(wc.l, pc.h[m], acc[j][m]);
                        acc[j][m] = mfma_m16<F16>(wc.h, pc.h[m], acc[j][m]);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (dma_step >= 0) {                                   // (a channel block's last group has KK % TPS taps: fewer slots than pieces)
#pragma unroll
            for (int i = 0; i < NPW; ++i)
                if (i >= ntap * NTW) dma_piece(dma_step, bbuf ^ 1, i);
        }
    };

    if (T > 0) {
        halo_load(s_begin / NGRP);
        halo_store();
#pragma unroll
        for (int i = 0; i < NPW; ++i) dma_piece(0, 0, i);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int bbuf = 0;
#pragma unroll 1
    for (int step = 0; step < T; ++step) {
        const int cb = (s_begin + step) / NGRP, g = (s_begin + step) - cb * NGRP;
        const bool more = step + 1 < T;
        const bool boundary = more && g == NGRP - 1;
        if (boundary) halo_load(cb + 1);
        compute(g, bbuf, more ? step + 1 : -1);
        if (boundary) {
            __syncthreads();                          // every wave is done with the halo
            halo_store();
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's pieces of step + 1 have landed
        __syncthreads();
        bbuf ^= 1;
    }

    // destination of tile pixel (row, col): kept if it lies inside the Hd x Wd output grid
    auto dest = [&](int row, int col) -> long {
        const int y = y0 + row, x = x0 + col;
        if (y >= p.Hd || x >= p.Wd) return -1;
        return ((long)(b * p.Hd + y) * p.Wd + x) * p.N;
    };
    if (!SPLITK) {
        // lane -> pixel (lane & 15) of tile row m, channels 4 * (lane >> 4) .. + 3 of channel tile j
        const float nslope = p.act == HOIG_ACT_NONE ? 1.f : (p.act == HOIG_ACT_RELU ? 0.f : p.slope);
        const bool special = p.act == HOIG_ACT_TANH || p.act == HOIG_ACT_SIGMOID;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const long d = dest(wm * MT + m, l15);
            if (d < 0) continue;
#pragma unroll
            for (int j = 0; j < NTW; ++j) {
                const int n = n0 + wn * 64 + j * 16 + lg * 4;
                float4 o = make_float4(acc[j][m][0] * p.oscale, acc[j][m][1] * p.oscale, acc[j][m][2] * p.oscale, acc[j][m][3] * p.oscale);
                if (p.bias) {
                    const float4 bv = *reinterpret_cast<const float4 *>(p.bias + n);
                    o.x += bv.x; o.y += bv.y; o.z += bv.z; o.w += bv.w;
                }
                o.x = fast_act(o.x, nslope, special, p.act, p.slope); o.y = fast_act(o.y, nslope, special, p.act, p.slope);
                o.z = fast_act(o.z, nslope, special, p.act, p.slope); o.w = fast_act(o.w, nslope, special, p.act, p.slope);
                if (p.addend) {
                    const float4 ad = *reinterpret_cast<const float4 *>(p.addend + d + n);
                    o.x += ad.x; o.y += ad.y; o.z += ad.z; o.w += ad.w;
                }
                *reinterpret_cast<float4 *>(p.C + d + n) = o;
            }
        }
    } else {
        // register r of acc[j][m]: pixel 4 * (lane >> 4) + r of tile row m, channel (lane & 15) of tile j; after the swap of the
        // registers of tiles j, j + 1 lanes 0-31 / 32-63 hold channels 0..31 of the pair at pixels r / 8 + r (first) and
        // 4 + r / 12 + r (second)
        const int l31 = lane & 31, lh = lane >> 5;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                long d[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) d[h] = dest(wm * MT + m, r + 8 * lh + 4 * h);
#pragma unroll
                for (int j = 0; j < NTW; j += 2) {
                    const int n = n0 + wn * 64 + j * 16 + l31;
                    const u2_t sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[j][m][r]), __float_as_uint(acc[j + 1][m][r]),
                                                                     false, false);
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        if (d[h] >= 0) {
                            float v = __uint_as_float(sw[h]) * p.oscale;
                            if (blockIdx.y == 0 && p.bias) v += p.bias[n];
                            atomicAdd(p.C + d[h] + n, v);
                        }
                }
            }
    }
}

template <int NSX, bool F16, bool SPLITK>
int launch_one(const FlatArgs &a, dim3 grid, hipStream_t st) {
    constexpr int TPS = taps_per_step(NSX);
    constexpr int shm = (int)lds_bytes(NSX, TPS);
    static_assert(shm <= 160 * 1024, "the halo and the weight buffers must fit in LDS");
    if (SPLITK) HOIG_ROUTE_FD(F16, halo5_m16_ksplit);
    else HOIG_ROUTE_FD(F16, halo5_m16);
    return hoig_launch<conv_halo5_m16_kernel<NSX, F16, SPLITK, TPS>, shm>(grid, NT, shm, st, a);
}

}  // namespace

// `a`: filled in as for launch_flat_m16 (KS = 5); the canvas is tiled over the destination grid (Hd x Wd)
int launch_halo5_m16(FlatArgs a, int ns, hipStream_t st) {
    if (a.KS != 5 || a.N % BN || a.Cg % 32) return HOIG_EUNSUPPORTED;
    if ((long)a.Bn * a.Hs * a.Ws * a.Cg >= (1L << 31)) return HOIG_EUNSUPPORTED;      // (the halo's source offsets are 32-bit)
    const int n_mt = a.Bn * (int)hoig_cdiv(a.Hd, TS) * (int)hoig_cdiv(a.Wd, TS);
    a.nblk_n = a.N / BN;
    a.nblk = n_mt * a.nblk_n;
    const int TPS = taps_per_step(ns);
    const int steps = (a.Cg >> 5) * ngrp(TPS);
    int split = 1;
    // few tiles, long K: split the step walk, add with atomics (key halo5 = 2: never -- tests and A/B of the split)
    if (a.nblk <= 128 && !a.addend && a.act == HOIG_ACT_NONE && hoig_tuning(HOIG_TUNE_HALO5) != 2) {
        // ONE round of workgroups on the 256 CUs (the 68-wide forward of the step: 128 tiles, split in two); up to TWO rounds at a
        // quarter of the chip or less, where one round would leave the chains longer than the generic kernel's (its 1024 / tiles
        // workgroups, four to a CU, reach the k-block minimum below on such launches; 256 / tiles here do not)
        split = (a.nblk <= 64 ? 512 : 256) / a.nblk;
        // at least 8 k-blocks (one tap x 32 channels) per workgroup: the generic kernel's rule (launch_igemm_m16), so that a launch of
        // few tiles adds as many partial sums here as there -- the fp32 rounding of a three-term forward is set by the chain length
        if (split > steps * TPS / 8) split = steps * TPS / 8;
        if (split < 1) split = 1;
    }
    a.steps_per_split = (int)hoig_cdiv(steps, split);
    split = (int)hoig_cdiv(steps, a.steps_per_split);
    dim3 grid(a.nblk, split);
    if (split > 1 && hipMemsetAsync(a.C, 0, (size_t)a.Bn * a.Hd * a.Wd * a.N * sizeof(float), st) != hipSuccess) return HOIG_ELAUNCH;
    if (split > 1) HOIG_NS_SWITCH(ns, HOIG_F16_SWITCH(a.f16, return launch_one<NSX, F16X, true>(a, grid, st)));
    HOIG_NS_SWITCH(ns, HOIG_F16_SWITCH(a.f16, return launch_one<NSX, F16X, false>(a, grid, st)));
    return HOIG_EINVAL;
}

}  // namespace hoig_detail
