// The LDS-halo convolution kernels on v_mfma_f32_32x32x16 (fp32 accumulate) and their launchers: stride-1 1x1 / 5x5, stride-1 3x3
// and stride-2 3x3.  The packed-plane dispatcher (run() of conv_igemm_bf16.hip) fills a HaloArgs and calls launch_halo<KS>,
// launch_halo3 or launch_halo_s2<SCATTER>; the tiles every large launch takes are on v_mfma_f32_16x16x32 (conv_halo16.hip,
// conv_s2_16.hip), which these launchers hand on to.  Operand planes and the split are those of conv_bf16_common.h.
#include "conv_bf16_common.h"
#include "tuning.h"

#ifndef HOIG_HALO_BSTAGES
#define HOIG_HALO_BSTAGES 1
#endif

namespace {
using namespace hoig_detail;

// ---------------------------------------------------------------------------------------------------------------------
// Stride-1 convolutions with an LDS-resident INPUT HALO tile.  The generic kernel above re-gathers the A tile from
// L2 for every tap (9x for a 3x3) and is bound by the per-CU load path (~60-70 GB/s from L2), not by the matrix
// pipe.  Here a workgroup owns 4 rows x 32 columns of output pixels (BM = 128); for each 32-channel block it stages the
// (4+KS-1) x (32+KS-1) input halo ONCE (split to bf16 hi/lo) and all KS*KS taps read their A fragments out of that same
// LDS image at a tap-dependent, lane-uniform row offset -- only the weight tile streams per tap (double-buffered).
// Halo rows are 80 B apart (64 B of data + 16 B pad): any 16 consecutive rows fall on 16 distinct 16-B bank slots, so
// ds_read_b128 stays conflict-free at every tap shift without an address-dependent swizzle.
// Used for conv fwd (stride 1) and for the data gradient of stride-1 convs (taps walked flipped).

// Instance-norm statistics from a convolution's epilogue.  s1 / s2: the lane's sums of v and v*v over the pixels it stored, per
// 32-channel column group j (channel = n0 + wn * TN * 32 + j * 32 + (lane & 31)).  The two 32-lane halves hold different pixels of
// the same channels (one cross-lane add), the WM waves with the same wn different image rows (LDS, which is dead after the main
// loop), and the workgroup then issues ONE atomic per (channel, moment) into the image's accumulators -- as many per address as
// the streaming statistics kernel it replaces issued (norm.hip: one per 16 pixel rows).
template <int TN, int WM, int WN, int NT>
__device__ __forceinline__ void halo_stats_epilogue(float (&s1)[TN], float (&s2)[TN], unsigned char *lds, double *stats, int b, int N,
                                                    int n0, int wm, int wn, int lane) {
    const int l31 = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        s1[j] += __shfl_xor(s1[j], 32);
        s2[j] += __shfl_xor(s2[j], 32);
    }
    __syncthreads();                                   // every wave has left the main loop's LDS tiles
    float *red = reinterpret_cast<float *>(lds);       // [WM][WN][TN][2][32]
    if (lh == 0) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            red[(((wm * WN + wn) * TN + j) * 2 + 0) * 32 + l31] = s1[j];
            red[(((wm * WN + wn) * TN + j) * 2 + 1) * 32 + l31] = s2[j];
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < WN * TN * 64; e += NT) {
        const int l = e & 31, m = (e >> 5) & 1, j = (e >> 6) % TN, w = (e >> 6) / TN;
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < WM; ++k) v += red[(((k * WN + w) * TN + j) * 2 + m) * 32 + l];
        const int n = n0 + w * (TN * 32) + j * 32 + l;
        if (n < N) hoig_stats_add(stats, b, N, m, n, v);
    }
}

template <int KS, int NSX, int WN, int BN, bool F16>
__global__ __launch_bounds__(128 * WN) void conv_halo_bf16_kernel(const HaloArgs p) {
    constexpr int NS = NSX == 1 ? 1 : 2, NB = NSX == 2 ? 2 : 1;      // operand planes: A (activations / dy), B (weights / x)
    constexpr int TH = 4, TW = 32;
    constexpr int NT = 128 * WN;                           // 2 x WN waves: 256 or 512 threads
    constexpr int RB = BN * 4 / NT;                        // 16-B weight chunks per thread per plane
    constexpr int HH = TH + KS - 1, HW = TW + KS - 1, HPIX = HH * HW;
    constexpr int AROW = 80;                               // bytes per halo pixel row (32 bf16 + pad)
    constexpr int PLANE_A = HPIX * AROW, PLANE_B = BN * 64;
    constexpr int TM = 2, TN = BN / (32 * WN);
    static_assert(TN >= 1, "BN = 64 needs the 4-wave variant");
    // LDS: one halo stage + two weight stages = 64 KB at KS=3 -> two workgroups per CU
    constexpr int NBST = HOIG_HALO_BSTAGES;                // weight stages in LDS
    __shared__ __attribute__((aligned(16))) unsigned char smem[NS * PLANE_A + NBST * NB * PLANE_B];
    unsigned char *Ah = smem, *Al = smem + PLANE_A;
    unsigned char *Bst = smem + NS * PLANE_A;              // two stages of (Bh, Bl)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    const int tile = hoig_xcd_remap(blockIdx.x, p.nblk);
    int mt = tile / p.nblk_n;
    const int n0 = (tile % p.nblk_n) * BN;
    const int tx_ = mt % p.tiles_x;
    mt /= p.tiles_x;
    const int ty_ = mt % p.tiles_y, b = mt / p.tiles_y;
    const int y0 = ty_ * TH, x0 = tx_ * TW;                // tile origin (output pixels)

    const int brow = tid >> 2, bchunk = tid & 3;
    const unsigned short *wrow_h[RB], *wrow_l[RB];
    int boff[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int n = n0 + brow + (NT / 4) * i;
        const size_t o = plane_index(n, bchunk * 8, p.K);
        wrow_h[i] = n < p.N ? p.Wh + o : nullptr;
        wrow_l[i] = (NB == 2 && n < p.N) ? p.Wl + o : nullptr;
        const int row = brow + (NT / 4) * i;
        boff[i] = row * 64 + ((bchunk ^ ((row >> 2) & 3)) << 4);
    }
    // fragment read offsets: wave wm owns output rows 2*wm, 2*wm+1 of the tile (32 pixels each = one MFMA row tile)
    int aread[TM], bread[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) aread[i] = ((wm * TM + i) * HW + l31) * AROW + lh * 16;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int row = wn * (TN * 32) + j * 32 + l31;
        bread[j] = row * 64 + ((lh ^ ((row >> 2) & 3)) << 4);
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // Weight tiles are prefetched TWO steps ahead (step = one tap of one 32-channel block) into two register sets: the
    // weights of a 512x512x3x3 layer (9.4 MB of bf16 planes) live in the Infinity Cache, whose latency under load exceeds
    // one step's MFMA phase (768 cycles per wave).
    uint4 rb0h[RB], rb0l[RB], rb1h[RB], rb1l[RB];
    constexpr int KK = KS * KS;
    const int ncb = p.Cg >> 5, T = ncb * KK;
    auto load_b = [&](int step, uint4 (&rh)[RB], uint4 (&rl)[RB]) {
        const int cb = step / KK, tap = step - cb * KK;
        const int wtap = p.flip ? (KK - 1 - tap) : tap;
        const size_t koff = (size_t)(wtap * p.Cg + cb * 32) * 32;      // k-block index * 1024
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            rh[i] = wrow_h[i] ? *reinterpret_cast<const uint4 *>(wrow_h[i] + koff) : make_uint4(0, 0, 0, 0);
            if (NB == 2) rl[i] = wrow_l[i] ? *reinterpret_cast<const uint4 *>(wrow_l[i] + koff) : make_uint4(0, 0, 0, 0);
        }
    };
    auto store_b = [&](int stage, const uint4 (&rh)[RB], const uint4 (&rl)[RB]) {
        unsigned char *Bh = Bst + stage * NB * PLANE_B, *Bl = Bh + PLANE_B;
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            *reinterpret_cast<uint4 *>(Bh + boff[i]) = rh[i];
            if (NB == 2) *reinterpret_cast<uint4 *>(Bl + boff[i]) = rl[i];
        }
    };
    const float *Aimg = p.A + (size_t)b * p.H * p.W * p.Cg;
    constexpr int HSLICES = (HPIX * 8 + NT - 1) / NT;      // halo float4s per thread
    float4 hreg[HSLICES];
    auto halo_load = [&](int cb) {
#pragma unroll
        for (int sl = 0; sl < HSLICES; ++sl) {
            const int i = tid + NT * sl;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < HPIX * 8) {
                const int pix = i >> 3, c4 = i & 7;
                const int hy = pix / HW, hx = pix - hy * HW;
                const int gy = y0 - p.pad + hy, gx = x0 - p.pad + hx;
                if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W)
                    v = *reinterpret_cast<const float4 *>(Aimg + ((size_t)gy * p.W + gx) * p.Cg + cb * 32 + c4 * 4);
            }
            hreg[sl] = v;
        }
    };
    auto halo_store = [&]() {
#pragma unroll
        for (int sl = 0; sl < HSLICES; ++sl) {
            const int i = tid + NT * sl;
            if (i < HPIX * 8) {
                const int pix = i >> 3, c4 = i & 7;
                uint2 hi, lo;
                split4t<F16>(hreg[sl], hi, lo);
                *reinterpret_cast<uint2 *>(Ah + pix * AROW + c4 * 8) = hi;
                if (NS == 2) *reinterpret_cast<uint2 *>(Al + pix * AROW + c4 * 8) = lo;
            }
        }
    };
    auto compute = [&](int stage, int step) {
        const int tap = step % KK;
        const int r = tap / KS, s_ = tap - r * KS;
        const int tapoff = (r * HW + s_) * AROW;
        const unsigned char *Bh = Bst + stage * NB * PLANE_B, *Bl = Bh + PLANE_B;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 ah[TM], al[TM], bhf[TN], blf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int off = aread[i] + tapoff + ks * 32;
                ah[i] = *reinterpret_cast<const bf16x8 *>(Ah + off);
                if (NS == 2) al[i] = *reinterpret_cast<const bf16x8 *>(Al + off);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int off = bread[j] ^ (ks << 5);
                bhf[j] = *reinterpret_cast<const bf16x8 *>(Bh + off);
                if (NB == 2) blf[j] = *reinterpret_cast<const bf16x8 *>(Bl + off);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if (NS == 2)
                        acc[i][j] = mfma16<F16>(al[i], bhf[j], acc[i][j]);
                        if (NB == 2) acc[i][j] = mfma16<F16>(ah[i], blf[j], acc[i][j]);
                    acc[i][j] = mfma16<F16>(ah[i], bhf[j], acc[i][j]);
                }
        }
    };
    // one step: prefetch weights of step+2, multiply `stage`, then publish the weights of step+1 (and, at a channel-block
    // boundary, the next halo, whose loads were issued before the multiply) behind one barrier
    auto do_step = [&](int step, int stage, uint4 (&nh)[RB], uint4 (&nl)[RB], uint4 (&fh)[RB], uint4 (&fl)[RB]) {
        if (step + 2 < T) load_b(step + 2, fh, fl);
        const bool boundary = (step % KK == KK - 1) && (step + 1 < T);
        if (boundary) halo_load(step / KK + 1);
        compute(NBST == 2 ? stage : 0, step);
        if (step + 1 < T) {
            if (boundary || NBST == 1) __syncthreads();   // every wave has finished reading the halo / the single B stage
            if (boundary) halo_store();
            store_b(NBST == 2 ? (stage ^ 1) : 0, nh, nl);
            __syncthreads();
        }
    };

    halo_load(0);
    load_b(0, rb0h, rb0l);
    halo_store();
    store_b(0, rb0h, rb0l);
    if (T > 1) load_b(1, rb0h, rb0l);
    __syncthreads();
#pragma unroll 1
    for (int step = 0; step < T; step += 2) {
        do_step(step, 0, rb0h, rb0l, rb1h, rb1l);
        if (step + 1 < T) do_step(step + 1, 1, rb1h, rb1l, rb0h, rb0l);
    }

    // epilogue: MFMA row (reg) -> pixel inside the wave's 32-pixel image row; col = lane&31 -> channel
    const float nslope = p.act == HOIG_ACT_NONE ? 1.f : (p.act == HOIG_ACT_RELU ? 0.f : p.slope);
    const bool special = p.act == HOIG_ACT_TANH || p.act == HOIG_ACT_SIGMOID;
    float bias_r[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * (TN * 32) + j * 32 + l31;
        bias_r[j] = (p.bias && n < p.N) ? p.bias[n] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int oy = y0 + wm * TM + i;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ox = x0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const size_t pix = ((size_t)b * p.H + oy) * p.W + ox;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wn * (TN * 32) + j * 32 + l31;
                if (n < p.N) {
                    float v = acc[i][j][r] * p.oscale;
                    v += bias_r[j];
                    v = fast_act(v, nslope, special, p.act, p.slope);
                    if (p.addend) v += p.addend[pix * p.N + n];
                    p.C[pix * p.N + n] = v;
                }
            }
        }
    }
}

// 3x3 variant with ONE TAP ROW (three taps) per step: the weight tiles of taps (r,0..2) of a 32-channel block are
// published together, so the two barriers, the weight publication and the fragment-read ramp that bracket every step are
// paid once per 3 x 768 MFMA cycles instead of once per 768.  LDS: halo 32 KB + 3 weight tiles 48 KB = 80 KB (dynamic),
// exactly two workgroups per CU.  Weights are prefetched one step (2304 MFMA cycles per wave) ahead.
// MODE 0: single LDS stage (two barriers per step; two 80-KB workgroups per CU)
// MODE 1: halo and weight tiles double-buffered (one 160-KB workgroup per CU, one barrier per step)
// (MODE 2 -- 8 rows x 32 pixels, weight tiles double-buffered, halo single -- was this kernel's form of the tile every large launch
//  takes; since round 4 those launches run on v_mfma_f32_16x16x32 (conv_halo16.hip: conv_halo3_m16_kernel) and round 6 removed the
//  32x32x16 instantiations together with the tuning key `mfma16` that selected them)
template <int NSX, int WM, int WN, int BN, int MODE, bool F16>
__global__ __launch_bounds__(64 * WM * WN) void conv_halo3_bf16_kernel(const HaloArgs p) {
    constexpr int NS = NSX == 1 ? 1 : 2, NB = NSX == 2 ? 2 : 1;      // operand planes: A (activations / dy), B (weights / x)
    constexpr int KS = 3, TH = 2 * WM, TW = 32;
    constexpr int NT = 64 * WM * WN;
    constexpr bool DB = MODE == 1;
    constexpr int RB = BN * 4 >= NT ? BN * 4 / NT : 1;     // 16-B weight chunks per thread per plane per tap
    constexpr bool B_PART = BN * 4 < NT;                   // more threads than chunks: only the first BN*4 threads load weights
    constexpr int HH = TH + KS - 1, HW = TW + KS - 1, HPIX = HH * HW;
    constexpr int AROW = 80;
    constexpr int PLANE_A = HPIX * AROW, PLANE_B = BN * 64;
    constexpr int TM = 2, TN = BN / (32 * WN);
    static_assert(TN >= 1, "BN = 64 needs the 4-wave variant");
    // DB (the 8-wave variant: ONE workgroup per CU, so LDS is free): halo and weight tiles are double-buffered -- the next
    // step's weights (and, at a channel-block boundary, the next halo) are written into the other buffer BEFORE this
    // step's multiply, one barrier per step, nothing but barrier skew is exposed.  160 KB exactly.
    static_assert(MODE == 0 || MODE == 1, "the 8-row tilings live in conv_halo16.hip");
    constexpr int NBUF_A = MODE == 1 ? 2 : 1, NBUF_B = MODE == 0 ? 1 : 2;
    constexpr int ABUF = NS * PLANE_A, BBUF = KS * NB * PLANE_B;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // NBUF_A * ABUF + NBUF_B * BBUF
    unsigned char *Abase = smem;
    unsigned char *Bbase = smem + NBUF_A * ABUF;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    // XCD-contiguous tile ranges (hoig_xcd_remap) enumerate the PIXEL tiles of one channel tile first: an XCD then streams
    // the weights of one or two channel tiles (2.4 MB each at 512x512x3x3) through its 4-MB L2 instead of all of them
    const int tile = hoig_xcd_remap(blockIdx.x, p.nblk);
    const int n_mt = p.nblk / p.nblk_n;
    int mt = p.nmajor ? tile % n_mt : tile / p.nblk_n;
    const int n0 = (p.nmajor ? tile / n_mt : tile % p.nblk_n) * BN;
    const int tx_ = mt % p.tiles_x;
    mt /= p.tiles_x;
    const int ty_ = mt % p.tiles_y, b = mt / p.tiles_y;
    const int y0 = ty_ * TH, x0 = tx_ * TW;

    const int brow = tid >> 2, bchunk = tid & 3;
    const unsigned short *wrow_h[RB], *wrow_l[RB];
    int boff[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int n = n0 + brow + (NT / 4) * i;
        const size_t o = plane_index(n, bchunk * 8, p.K);
        const bool ok = n < p.N && (!B_PART || brow < BN);
        wrow_h[i] = ok ? p.Wh + o : nullptr;
        wrow_l[i] = (NB == 2 && ok) ? p.Wl + o : nullptr;
        const int row = brow + (NT / 4) * i;
        boff[i] = row * 64 + ((bchunk ^ ((row >> 2) & 3)) << 4);
    }
    int aread[TM], bread[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) aread[i] = ((wm * TM + i) * HW + l31) * AROW + lh * 16;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int row = wn * (TN * 32) + j * 32 + l31;
        bread[j] = row * 64 + ((lh ^ ((row >> 2) & 3)) << 4);
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    uint4 rbh[KS][RB], rbl[KS][RB];
    const int ncb = p.Cg >> 5, T = ncb * KS;               // step = (channel block, tap row)
    auto load_b = [&](int step) {
        const int cb = step / KS, r = step - cb * KS;
#pragma unroll
        for (int t = 0; t < KS; ++t) {
            const int tap = r * KS + t;
            const int wtap = p.flip ? (KS * KS - 1 - tap) : tap;
            const size_t koff = (size_t)(wtap * p.Cg + cb * 32) * 32;
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                rbh[t][i] = wrow_h[i] ? *reinterpret_cast<const uint4 *>(wrow_h[i] + koff) : make_uint4(0, 0, 0, 0);
                if (NB == 2)
                    rbl[t][i] = wrow_l[i] ? *reinterpret_cast<const uint4 *>(wrow_l[i] + koff) : make_uint4(0, 0, 0, 0);
            }
        }
    };
    auto store_b = [&](int buf) {
#pragma unroll
        for (int t = 0; t < KS; ++t) {
            unsigned char *Bh = Bbase + buf * BBUF + t * NB * PLANE_B, *Bl = Bh + PLANE_B;
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                if (B_PART && brow >= BN) continue;
                *reinterpret_cast<uint4 *>(Bh + boff[i]) = rbh[t][i];
                if (NB == 2) *reinterpret_cast<uint4 *>(Bl + boff[i]) = rbl[t][i];
            }
        }
    };
    constexpr int HSLICES = (HPIX * 8 + NT - 1) / NT;
    float4 hreg[HSLICES];
    auto halo_load = [&](int cb) {
        // one or two source tensors along the channel axis (p.A2: see HaloArgs)
        const bool second = p.A2 != nullptr && cb * 32 >= p.cg1;
        const int ld = p.A2 ? (second ? p.Cg - p.cg1 : p.cg1) : p.Cg;
        const float *Aimg = (second ? p.A2 : p.A) + (size_t)b * p.H * p.W * ld + (second ? cb * 32 - p.cg1 : cb * 32);
#pragma unroll
        for (int sl = 0; sl < HSLICES; ++sl) {
            const int i = tid + NT * sl;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < HPIX * 8) {
                const int pix = i >> 3, c4 = i & 7;
                const int hy = pix / HW, hx = pix - hy * HW;
                const int gy = y0 - p.pad + hy, gx = x0 - p.pad + hx;
                if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W)
                    v = *reinterpret_cast<const float4 *>(Aimg + ((size_t)gy * p.W + gx) * ld + c4 * 4);
            }
            hreg[sl] = v;
        }
    };
    auto halo_store = [&](int buf) {
        unsigned char *Ah = Abase + buf * ABUF, *Al = Ah + PLANE_A;
#pragma unroll
        for (int sl = 0; sl < HSLICES; ++sl) {
            const int i = tid + NT * sl;
            if (i < HPIX * 8) {
                const int pix = i >> 3, c4 = i & 7;
                uint2 hi, lo;
                split4t<F16>(hreg[sl], hi, lo);
                *reinterpret_cast<uint2 *>(Ah + pix * AROW + c4 * 8) = hi;
                if (NS == 2) *reinterpret_cast<uint2 *>(Al + pix * AROW + c4 * 8) = lo;
            }
        }
    };
    // fragments of sub-step i+1 (tap t, k-half ks) are read into a second register set before the MFMAs of sub-step i
    // issue: with one or two waves per SIMD the LDS latency of a just-in-time read is otherwise exposed
    struct Frags {
        bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
    };
    auto compute = [&](int r, int abuf, int bbuf) {
        const unsigned char *Ah = Abase + abuf * ABUF, *Al = Ah + PLANE_A;
        auto read = [&](Frags &f, int i) {
            const int t = i >> 1, ks = i & 1;
            const int tapoff = (r * HW + t) * AROW;
            const unsigned char *Bh = Bbase + bbuf * BBUF + t * NB * PLANE_B, *Bl = Bh + PLANE_B;
#pragma unroll
            for (int ii = 0; ii < TM; ++ii) {
                const int off = aread[ii] + tapoff + ks * 32;
                f.ah[ii] = *reinterpret_cast<const bf16x8 *>(Ah + off);
                if (NS == 2) f.al[ii] = *reinterpret_cast<const bf16x8 *>(Al + off);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int off = bread[j] ^ (ks << 5);
                f.bh[j] = *reinterpret_cast<const bf16x8 *>(Bh + off);
                if (NB == 2) f.bl[j] = *reinterpret_cast<const bf16x8 *>(Bl + off);
            }
        };
        auto mma = [&](const Frags &f) {
#pragma unroll
            for (int ii = 0; ii < TM; ++ii)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if (NS == 2)
                        acc[ii][j] = mfma16<F16>(f.al[ii], f.bh[j], acc[ii][j]);
                        if (NB == 2) acc[ii][j] = mfma16<F16>(f.ah[ii], f.bl[j], acc[ii][j]);
                    acc[ii][j] = mfma16<F16>(f.ah[ii], f.bh[j], acc[ii][j]);
                }
        };
        Frags f0, f1;
        read(f0, 0);
#pragma unroll
        for (int i = 0; i < 2 * KS; i += 2) {
            read(f1, i + 1);
            __builtin_amdgcn_sched_barrier(0);      // keep the reads of sub-step i+1 AHEAD of the MFMAs of sub-step i
            mma(f0);
            __builtin_amdgcn_sched_barrier(0);
            if (i + 2 < 2 * KS) read(f0, i + 2);
            __builtin_amdgcn_sched_barrier(0);
            mma(f1);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // (staging the weight tiles by LDS-DMA -- global_load_lds, the pre-swizzled plane blocks are LDS images -- measured
    // ~9 % SLOWER here than the register-staged ds_write_b128 path below)
    halo_load(0);
    halo_store(0);
    load_b(0);
    store_b(0);
    if (DB) {
        if (T > 1) load_b(1);
        __syncthreads();
        int abuf = 0, bbuf = 0;
#pragma unroll 1
        for (int step = 0; step < T; ++step) {
            const int cb = step / KS, r = step - cb * KS;
            const bool more = step + 1 < T;
            const bool boundary = more && r == KS - 1;
            if (more) store_b(bbuf ^ 1);                  // weights of step+1 (registers loaded during the previous step)
            if (boundary) halo_store(abuf ^ 1);           // halo of the next channel block (loaded during the previous step)
            if (step + 2 < T) load_b(step + 2);
            if (r == KS - 2 && cb + 1 < ncb) halo_load(cb + 1);
            compute(r, abuf, bbuf);
            __syncthreads();
            bbuf ^= 1;
            if (boundary) abuf ^= 1;
        }
    } else {
        __syncthreads();
#pragma unroll 1
        for (int step = 0; step < T; ++step) {
            const int cb = step / KS, r = step - cb * KS;
            const bool more = step + 1 < T;
            const bool boundary = more && r == KS - 1;
            if (more) load_b(step + 1);
            if (boundary) halo_load(cb + 1);
            compute(r, 0, 0);
            if (more) {
                __syncthreads();                  // every wave has finished reading the weight tiles (and the halo)
                if (boundary) halo_store(0);
                store_b(0);
                __syncthreads();
            }
        }
    }

    const float nslope = p.act == HOIG_ACT_NONE ? 1.f : (p.act == HOIG_ACT_RELU ? 0.f : p.slope);
    const bool special = p.act == HOIG_ACT_TANH || p.act == HOIG_ACT_SIGMOID;
    float bias_r[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * (TN * 32) + j * 32 + l31;
        bias_r[j] = (p.bias && n < p.N) ? p.bias[n] : 0.f;
    }
    float st1[TN], st2[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) st1[j] = st2[j] = 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int oy = y0 + wm * TM + i;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ox = x0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const size_t pix = ((size_t)b * p.H + oy) * p.W + ox;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wn * (TN * 32) + j * 32 + l31;
                if (n < p.N) {
                    float v = acc[i][j][r] * p.oscale;
                    v += bias_r[j];
                    v = fast_act(v, nslope, special, p.act, p.slope);
                    if (p.addend) v += p.addend[pix * p.N + n];
                    st1[j] += v;
                    st2[j] += v * v;
                    if (!p.C2) p.C[pix * p.N + n] = v;
                    else if (n < p.n1) p.C[pix * p.n1 + n] = v;                  // (a whole 32-column group goes one way)
                    else p.C2[pix * (p.N - p.n1) + (n - p.n1)] = v;
                }
            }
        }
    }
    if (p.stats) halo_stats_epilogue<TN, WM, WN, NT>(st1, st2, smem, p.stats, b, p.N, n0, wm, wn, lane);
}

template <int NS, int WM, int WN, int BN, int MODE>
int launch_halo3_one(const HaloArgs &a, hipStream_t st) {
    constexpr int HPIX = (2 * WM + 2) * 34;
    constexpr int shm = (MODE == 1 ? 2 : 1) * (ns_a(NS) * (HPIX * 80)) + (MODE == 0 ? 1 : 2) * (3 * ns_b(NS) * (BN * 64));
    if (BN == 64) HOIG_ROUTE_FD(a.f16, halo3_64);
    else if (MODE == 1) HOIG_ROUTE_FD(a.f16, halo3_128w);
    else HOIG_ROUTE_FD(a.f16, halo3_128);
    HOIG_F16_SWITCH(a.f16, return hoig_launch<conv_halo3_bf16_kernel<NS, WM, WN, BN, MODE, F16X>, shm>(a.nblk, 64 * WM * WN, shm, st, a));
}

// ---------------------------------------------------------------------------------------------------------------------
// Stride-2 3x3 layers (pad 1; ConvTranspose2d with output_padding 1) on LDS halo tiles.  On the generic kernel these re-gather
// their fp32 input from L2 / HBM for every tap (the 268-MB full-resolution tensors do not stay in L2) and run at 85-150 TF.
// Decomposed by the PARITY of the fine-grid coordinate, every tap becomes a unit-stride read of a small halo image:
//   GATHER mode (Conv2d s2 forward, ConvTranspose2d data gradient): out[o] = sum_{r,s} in[2o - 1 + (r,s)] w[r][s].  The input
//     is read as its four parity phases in[2i+p][2j+q]; tap r uses phase p = (r != 1) at coarse index o + (r == 0 ? -1 : 0).
//     Per 32-channel block: phase (1,1) serves taps (0,0),(0,2),(2,0),(2,2), phase (1,0) taps (0,1),(2,1), phase (0,1) taps
//     (1,0),(1,2), phase (0,0) tap (1,1): five steps of <= 2 taps, four (TH+1) x 33 halo loads (stride-2 source addressing).
//   SCATTER mode (ConvTranspose2d forward, Conv2d s2 data gradient): out[2i - 1 + (r,s)] += in[i] w[r][s].  A workgroup owns ONE
//     output parity phase (P,Q) of a coarse tile: out[2I+P][2J+Q] = sum over the taps with r = 1 (P = 0) or r in {0,2} (P = 1)
//     of in[I + (r == 0)][J + (s == 0)] w[r][s] -- a stride-1 conv with 1, 2 or 4 taps over one halo image; strided stores.
// Tile: 4 x 32 coarse pixels x BN channels, 4 waves, single LDS stage (58 KB: two workgroups per CU).
template <int NSX, int BN, bool SCATTER, bool F16>
__global__ __launch_bounds__(256) void conv_halo_s2_bf16_kernel(const HaloArgs p) {
    constexpr int NS = NSX == 1 ? 1 : 2, NB = NSX == 2 ? 2 : 1;      // operand planes: A (activations / dy), B (weights / x)
    constexpr int TH = 4, TW = 32, NT = 256, WN = 2;
    constexpr int RB = BN * 4 / NT;                        // 16-B weight chunks per thread per plane per tap
    constexpr int HH = TH + 1, HW = TW + 1, HPIX = HH * HW;
    constexpr int AROW = 80;
    constexpr int PLANE_A = HPIX * AROW, PLANE_B = BN * 64;
    constexpr int TM = 2, TN = BN / (32 * WN);
    __shared__ __attribute__((aligned(16))) unsigned char smem[NS * PLANE_A + 2 * NB * PLANE_B];
    unsigned char *Ah = smem, *Al = smem + PLANE_A;
    unsigned char *Bbase = smem + NS * PLANE_A;            // two tap tiles of (Bh, Bl)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    int tile = hoig_xcd_remap(blockIdx.x, p.nblk);
    int P = 0, Q = 0;
    if (SCATTER) {
        P = (tile >> 1) & 1;
        Q = tile & 1;
        tile >>= 2;
    }
    int mt = tile / p.nblk_n;
    const int n0 = (tile % p.nblk_n) * BN;
    const int tx_ = mt % p.tiles_x;
    mt /= p.tiles_x;
    const int ty_ = mt % p.tiles_y, b = mt / p.tiles_y;
    const int y0 = ty_ * TH, x0 = tx_ * TW;                // coarse-grid tile origin

    const int brow = tid >> 2, bchunk = tid & 3;
    const unsigned short *wrow_h[RB], *wrow_l[RB];
    int boff[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int n = n0 + brow + (NT / 4) * i;
        const size_t o = plane_index(n, bchunk * 8, p.K);
        wrow_h[i] = n < p.N ? p.Wh + o : nullptr;
        wrow_l[i] = (NB == 2 && n < p.N) ? p.Wl + o : nullptr;
        const int row = brow + (NT / 4) * i;
        boff[i] = row * 64 + ((bchunk ^ ((row >> 2) & 3)) << 4);
    }
    int aread[TM], bread[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) aread[i] = ((wm * TM + i) * HW + l31) * AROW + lh * 16;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int row = wn * (TN * 32) + j * 32 + l31;
        bread[j] = row * 64 + ((lh ^ ((row >> 2) & 3)) << 4);
    }
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // ---- step table (wave-uniform scalar code) ----
    struct Step {
        int cb, ntap, tap[2], pp, qq;
        bool load;
    };
    const int spc = SCATTER ? ((P ? 2 : 1) * (Q ? 2 : 1) + 1) / 2 : 5;     // steps per 32-channel block
    const int ncb = p.Cg >> 5, T = ncb * spc;
    auto step_info = [&](int step) -> Step {
        Step s_;
        s_.cb = step / spc;
        const int idx = step - s_.cb * spc;
        s_.pp = s_.qq = 0;
        if (!SCATTER) {
            s_.load = idx != 1;
            switch (idx) {
                case 0: s_.pp = 1; s_.qq = 1; s_.ntap = 2; s_.tap[0] = 0; s_.tap[1] = 2; break;
                case 1: s_.pp = 1; s_.qq = 1; s_.ntap = 2; s_.tap[0] = 6; s_.tap[1] = 8; break;
                case 2: s_.pp = 1; s_.qq = 0; s_.ntap = 2; s_.tap[0] = 1; s_.tap[1] = 7; break;
                case 3: s_.pp = 0; s_.qq = 1; s_.ntap = 2; s_.tap[0] = 3; s_.tap[1] = 5; break;
                default: s_.ntap = 1; s_.tap[0] = 4; s_.tap[1] = 4; break;
            }
        } else {
            s_.load = idx == 0;
            // rows of the phase: P = 0 -> r = 1; P = 1 -> r in {0, 2}; same for columns
            const int r0 = P ? 0 : 1, r1 = 2, s0 = Q ? 0 : 1, s1 = 2;
            if (P && Q) {
                s_.ntap = 2;
                s_.tap[0] = (idx ? r1 : r0) * 3 + s0;
                s_.tap[1] = (idx ? r1 : r0) * 3 + s1;
            } else if (P) {
                s_.ntap = 2; s_.tap[0] = r0 * 3 + s0; s_.tap[1] = r1 * 3 + s0;
            } else if (Q) {
                s_.ntap = 2; s_.tap[0] = r0 * 3 + s0; s_.tap[1] = r0 * 3 + s1;
            } else {
                s_.ntap = 1; s_.tap[0] = s_.tap[1] = 4;
            }
        }
        return s_;
    };
    // halo offset (rows, columns in {0,1}) of tap (r,s):  gather: (r != 0, s != 0)   scatter: (r == 0, s == 0)
    auto tap_off = [&](int tap) -> int {
        const int r = tap / 3, s_ = tap - r * 3;
        const int dr = SCATTER ? (r == 0) : (r != 0), dc = SCATTER ? (s_ == 0) : (s_ != 0);
        return (dr * HW + dc) * AROW;
    };

    uint4 rbh[2][RB], rbl[2][RB];
    auto load_b = [&](const Step &s_) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const size_t koff = (size_t)(s_.tap[t] * p.Cg + s_.cb * 32) * 32;
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                rbh[t][i] = wrow_h[i] ? *reinterpret_cast<const uint4 *>(wrow_h[i] + koff) : make_uint4(0, 0, 0, 0);
                if (NB == 2)
                    rbl[t][i] = wrow_l[i] ? *reinterpret_cast<const uint4 *>(wrow_l[i] + koff) : make_uint4(0, 0, 0, 0);
            }
        }
    };
    auto store_b = [&]() {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            unsigned char *Bh = Bbase + t * NB * PLANE_B, *Bl = Bh + PLANE_B;
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                *reinterpret_cast<uint4 *>(Bh + boff[i]) = rbh[t][i];
                if (NB == 2) *reinterpret_cast<uint4 *>(Bl + boff[i]) = rbl[t][i];
            }
        }
    };
    const float *Aimg = p.A + (size_t)b * p.H * p.W * p.Cg;       // p.H x p.W: the gathered tensor (fine grid in gather mode)
    constexpr int HSLICES = (HPIX * 8 + NT - 1) / NT;
    // halo images are fetched TWO steps ahead into alternating register sets: a step is only one or two taps long (768-1536
    // MFMA cycles per wave), less than the HBM latency of the full-resolution tensors
    float4 hregs[2][HSLICES];
    auto halo_load = [&](const Step &s_, float4 (&hreg)[HSLICES]) {
#pragma unroll
        for (int sl = 0; sl < HSLICES; ++sl) {
            const int i = tid + NT * sl;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < HPIX * 8) {
                const int pix = i >> 3, c4 = i & 7;
                const int hy = pix / HW, hx = pix - hy * HW;
                const int gy = SCATTER ? y0 + hy : 2 * (y0 - 1 + hy) + s_.pp;
                const int gx = SCATTER ? x0 + hx : 2 * (x0 - 1 + hx) + s_.qq;
                if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W)
                    v = *reinterpret_cast<const float4 *>(Aimg + ((size_t)gy * p.W + gx) * p.Cg + s_.cb * 32 + c4 * 4);
            }
            hreg[sl] = v;
        }
    };
    auto halo_store = [&](const float4 (&hreg)[HSLICES]) {
#pragma unroll
        for (int sl = 0; sl < HSLICES; ++sl) {
            const int i = tid + NT * sl;
            if (i < HPIX * 8) {
                const int pix = i >> 3, c4 = i & 7;
                uint2 hi, lo;
                split4t<F16>(hreg[sl], hi, lo);
                *reinterpret_cast<uint2 *>(Ah + pix * AROW + c4 * 8) = hi;
                if (NS == 2) *reinterpret_cast<uint2 *>(Al + pix * AROW + c4 * 8) = lo;
            }
        }
    };
    auto compute = [&](const Step &s_) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (t >= s_.ntap) break;
            const int tapoff = tap_off(s_.tap[t]);
            const unsigned char *Bh = Bbase + t * NB * PLANE_B, *Bl = Bh + PLANE_B;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 ah[TM], al[TM], bhf[TN], blf[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int off = aread[i] + tapoff + ks * 32;
                    ah[i] = *reinterpret_cast<const bf16x8 *>(Ah + off);
                    if (NS == 2) al[i] = *reinterpret_cast<const bf16x8 *>(Al + off);
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int off = bread[j] ^ (ks << 5);
                    bhf[j] = *reinterpret_cast<const bf16x8 *>(Bh + off);
                    if (NB == 2) blf[j] = *reinterpret_cast<const bf16x8 *>(Bl + off);
                }
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        if (NS == 2)
                            acc[i][j] = mfma16<F16>(al[i], bhf[j], acc[i][j]);
                            if (NB == 2) acc[i][j] = mfma16<F16>(ah[i], blf[j], acc[i][j]);
                        acc[i][j] = mfma16<F16>(ah[i], bhf[j], acc[i][j]);
                    }
            }
        }
    };

    Step cur = step_info(0);
    halo_load(cur, hregs[0]);
    load_b(cur);
    halo_store(hregs[0]);
    store_b();
    Step nxt = cur;
    if (T > 1) {
        nxt = step_info(1);
        if (nxt.load) halo_load(nxt, hregs[1]);           // (the set that "step -1" would have filled)
    }
    __syncthreads();
    // two-fold unrolled so that the register-set index is static
    auto one_step = [&](int step, float4 (&mine)[HSLICES], float4 (&other)[HSLICES]) {
        const bool more = step + 1 < T;
        if (more) load_b(nxt);
        if (step + 2 < T) {
            const Step n2 = step_info(step + 2);
            if (n2.load) halo_load(n2, mine);             // stored at the end of step+1
        }
        compute(cur);
        if (more) {
            __syncthreads();                  // every wave has finished reading the weight tiles (and the halo)
            if (nxt.load) halo_store(other);  // fetched during step-1
            store_b();
            __syncthreads();
            cur = nxt;
            if (step + 2 < T) nxt = step_info(step + 2);
        }
    };
#pragma unroll 1
    for (int step = 0; step < T; step += 2) {
        one_step(step, hregs[0], hregs[1]);
        if (step + 1 < T) one_step(step + 1, hregs[1], hregs[0]);
    }

    const float nslope = p.act == HOIG_ACT_NONE ? 1.f : (p.act == HOIG_ACT_RELU ? 0.f : p.slope);
    const bool special = p.act == HOIG_ACT_TANH || p.act == HOIG_ACT_SIGMOID;
    float bias_r[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * (TN * 32) + j * 32 + l31;
        bias_r[j] = (p.bias && n < p.N) ? p.bias[n] : 0.f;
    }
    float st1[TN], st2[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) st1[j] = st2[j] = 0.f;
    // output grid: gather mode = the coarse grid (tiles_y*TH x tiles_x*TW); scatter mode = twice the coarse grid, phase (P,Q)
    const int Ho = SCATTER ? 2 * p.H : p.tiles_y * TH, Wo = SCATTER ? 2 * p.W : p.tiles_x * TW;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int cy = y0 + wm * TM + i;
        const int oy = SCATTER ? 2 * cy + P : cy;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int cx = x0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const int ox = SCATTER ? 2 * cx + Q : cx;
            const size_t pix = ((size_t)b * Ho + oy) * Wo + ox;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wn * (TN * 32) + j * 32 + l31;
                if (n < p.N) {
                    float v = acc[i][j][r] * p.oscale;
                    v += bias_r[j];
                    v = fast_act(v, nslope, special, p.act, p.slope);
                    if (p.addend) v += p.addend[pix * p.N + n];
                    st1[j] += v;
                    st2[j] += v * v;
                    p.C[pix * p.N + n] = v;
                }
            }
        }
    }
    if (p.stats) halo_stats_epilogue<TN, 2, WN, NT>(st1, st2, smem, p.stats, b, p.N, n0, wm, wn, lane);
}

}  // namespace

namespace hoig_detail {

int launch_halo3(HaloArgs a, int ns, hipStream_t st) {
    a.tiles_x = a.W / 32;
    a.tiles_y = a.H / 4;
    a.nmajor = 1;
    const bool n64 = (a.N % 128) != 0 || (a.C2 && a.n1 % 128 != 0);      // (a channel tile must not straddle the two outputs)
    a.nblk_n = (int)hoig_cdiv(a.N, n64 ? 64 : 128);
    a.nblk = a.Bn * a.tiles_x * a.tiles_y * a.nblk_n;
    // 8 rows x 32 pixels x bn channels per workgroup on the 16x16 MFMA (conv_halo16.hip); the tests below see the 4-row tile count
    auto rows8 = [&](int bn) {
        a.tiles_y = a.H / 8;
        a.nblk_n = (int)hoig_cdiv(a.N, bn);
        a.nblk = a.Bn * a.tiles_x * a.tiles_y * a.nblk_n;
        return launch_halo3_m16(a, ns, bn, st);
    };
    if (n64) {
        // 64-channel layers (the full-resolution levels): 8 x 32 x 64 where that leaves every CU a workgroup
        if (a.H % 8 == 0 && a.nblk / 2 >= 256) return rows8(64);
        if (a.a_split || a.b_split || a.in_scale) return HOIG_EUNSUPPORTED;  // (pre-split input, grouped launch: conv_halo16.hip only)
        HOIG_NS_SWITCH(ns, return launch_halo3_one<NSX, 2, 2, 64, 0>(a, st));
    }
    // the 8-image launches of src_model / tsf_model (which run side by side on two streams) on 128-channel tiles -- 128
    // workgroups each, half the chip per launch -- instead of 256 workgroups of 64-channel tiles (round 4: step -0.65 ms,
    // profiles/r04_few128_ab.txt)
    if (a.H % 8 == 0 && a.nblk / 2 < 256 && a.nblk >= 192 && a.N % 128 == 0) return rows8(128);
    if (a.H % 8 == 0 && a.nblk / 2 < 256 && a.nblk >= 192) return rows8(64);   // too few 8-row tiles at BN = 128: 64 channels
    // 8 x 32 pixel tiles (8 waves, weight tile shared by 256 pixels) when that still gives every CU a workgroup
    if (a.H % 8 == 0 && a.nblk / 2 >= 256) return rows8(128);
    if (a.a_split || a.b_split || a.in_scale) return HOIG_EUNSUPPORTED;
    const bool wide = a.nblk < 384;
    HOIG_NS_SWITCH(ns, return wide ? launch_halo3_one<NSX, 2, 4, 128, 1>(a, st) : launch_halo3_one<NSX, 2, 2, 128, 0>(a, st));
    return HOIG_EINVAL;
}

// a: H, W = spatial size of the GATHERED tensor (gather mode: the fine grid, output is H/2 x W/2; scatter mode: the coarse
// grid, output is 2H x 2W)
template <bool SCATTER>
int launch_halo_s2(HaloArgs a, int ns, hipStream_t st) {
    const int ch = SCATTER ? a.H : a.H / 2, cw = SCATTER ? a.W : a.W / 2;      // coarse grid
    a.tiles_x = cw / 32;
    a.tiles_y = ch / 4;
    const bool n64 = (a.N % 128) != 0;
    a.nblk_n = a.N / (n64 ? 64 : 128);
    a.nblk = a.Bn * a.tiles_x * a.tiles_y * a.nblk_n * (SCATTER ? 4 : 1);
    a.nmajor = 0;
    // on v_mfma_f32_16x16x32 (conv_halo16.hip): +10..24 % (profiles/r04_s2_16_ab.txt) except the THREE-term scatter launches with
    // 64-channel tiles (ConvTranspose2d 128 -> 64 forward at full resolution: -5 %; the two-term data gradient of the same
    // shape: +24 %), which stay on the 32x32 kernel
    if (hoig_tuning(HOIG_TUNE_S2_16) != 0 && !(SCATTER && n64 && ns == 2)) return launch_halo_s2_m16(a, ns, SCATTER, st);
    if (n64) SCATTER ? HOIG_ROUTE_FD(a.f16, s2s_64) : HOIG_ROUTE_FD(a.f16, s2g_64);
    else SCATTER ? HOIG_ROUTE_FD(a.f16, s2s_128) : HOIG_ROUTE_FD(a.f16, s2g_128);
    if (n64)
        HOIG_NS_SWITCH(ns, HOIG_F16_SWITCH(a.f16, return hoig_launch<conv_halo_s2_bf16_kernel<NSX, 64, SCATTER, F16X>>(a.nblk, 256, 0, st, a)));
    HOIG_NS_SWITCH(ns, HOIG_F16_SWITCH(a.f16,
                                       return hoig_launch<conv_halo_s2_bf16_kernel<NSX, 128, SCATTER, F16X>>(a.nblk, 256, 0, st, a)));
}

template <int KS>
int launch_halo(HaloArgs a, int ns, hipStream_t st) {
    a.tiles_x = a.W / 32;
    a.tiles_y = a.H / 4;
    const bool n64 = (a.N % 128) != 0;        // 64-channel layers (the full-resolution levels, VGG conv1): BN = 64 tiles
    a.nblk_n = (int)hoig_cdiv(a.N, n64 ? 64 : 128);
    a.nblk = a.Bn * a.tiles_x * a.tiles_y * a.nblk_n;
    const bool wide = a.nblk < 384;
    if (KS == 1) n64 ? HOIG_ROUTE_FD(a.f16, halo1_64) : (wide ? HOIG_ROUTE_FD(a.f16, halo1_128w) : HOIG_ROUTE_FD(a.f16, halo1_128));
    else n64 ? HOIG_ROUTE_FD(a.f16, same5_64) : (wide ? HOIG_ROUTE_FD(a.f16, same5_128w) : HOIG_ROUTE_FD(a.f16, same5_128));
    if (n64)
        HOIG_NS_SWITCH(ns, HOIG_F16_SWITCH(a.f16, return hoig_launch<conv_halo_bf16_kernel<KS, NSX, 2, 64, F16X>>(a.nblk, 256, 0, st, a)));
    // fewer than ~1.5 workgroups per CU (wide): 8 waves per workgroup keep two waves on every SIMD
    if (wide)
        HOIG_NS_SWITCH(ns, HOIG_F16_SWITCH(a.f16, return hoig_launch<conv_halo_bf16_kernel<KS, NSX, 4, 128, F16X>>(a.nblk, 512, 0, st, a)));
    HOIG_NS_SWITCH(ns, HOIG_F16_SWITCH(a.f16, return hoig_launch<conv_halo_bf16_kernel<KS, NSX, 2, 128, F16X>>(a.nblk, 256, 0, st, a)));
}

template int launch_halo<1>(HaloArgs, int, hipStream_t);
template int launch_halo<5>(HaloArgs, int, hipStream_t);
template int launch_halo_s2<false>(HaloArgs, int, hipStream_t);
template int launch_halo_s2<true>(HaloArgs, int, hipStream_t);

}  // namespace hoig_detail
