// bf16-operand MFMA variants of the implicit-GEMM convolution (v_mfma_f32_32x32x16_bf16, fp32 accumulate): the generic kernel, the
// packed-plane dispatcher run() and the convolution entry points.  The LDS-halo kernels run() routes to are in conv_halo32.hip and the
// 16x16x32 files (conv_halo16.hip, conv_s2_16.hip, conv_flat16.hip, conv_halo5.hip, conv_igemm16.hip), the packers in weight_planes.hip.
//
//   HOIG_PREC_BF16X3 : every fp32 operand x is split x = hi + lo (both bf16, hi = rne(x), lo = rne(x - hi));
//                      a*b ~= ah*bh + ah*bl + al*bh  -> 3 MFMAs per k-step, ~2^-16 relative product error, i.e. fp32-class
//                      parity (north_star bound 1e-3) at 1/3 of the 2.5 PFLOP/s dense bf16 rate (5.3x the fp32 MFMA rate).
//   HOIG_PREC_BF16   : hi only, 1 MFMA per k-step (for experiments; ~2^-9 relative per operand).
//
// Operands: activations stay fp32 NHWC in HBM and are split while the gathered tile is staged into LDS; weights are
// pre-split ONCE per optimiser step into K-contiguous bf16 planes by hoig_pack_conv_weight_bf16 ([N][K], K=(r,s,c);
// for the data gradient the plane is the transposed pack [Ci][R][S][Co]), so the B tile needs no conversion and both
// MFMA fragments are plain ds_read_b128 of 8 consecutive k.
// LDS image per operand plane: rows of 32 bf16 (64 B = four 16-B chunks), chunk index XOR-ed with (row>>2)&3 so the
// 16-lane groups of ds_read_b128 hit 16 distinct slots of the 256-B bank row.
// Shapes outside the fast path (gathered channels not a multiple of 32) return HOIG_EUNSUPPORTED and the caller uses the
// exact-fp32 kernels of conv_igemm.hip.
#include "conv_bf16_common.h"
#include "tuning.h"
#include <cstdlib>

namespace {
using namespace hoig_detail;

// LDS plane = [rows][BK] bf16; the 16-B chunk index of a row is XOR-ed with a row-dependent value so that the 16-lane
// groups of ds_read_b128 (rows r..r+3, r+12.., r+20..) fall on 16 distinct slots of the 256-B bank row:
//   BK = 32 (64-B rows, 4 chunks): chunk ^ ((row >> 2) & 3)      BK = 64 (128-B rows, 8 chunks): chunk ^ ((row >> 1) & 7)
template <int BK>
__device__ __forceinline__ int lds_swz(int row) {
    return BK == 32 ? ((row >> 2) & 3) : ((row >> 1) & 7);
}
// byte offset of (row, k), k a multiple of 4
template <int BK>
__device__ __forceinline__ int lds_off(int row, int k) {
    return row * (BK * 2) + (((k >> 3) ^ lds_swz<BK>(row)) << 4) + ((k & 4) << 1);
}

template <int BM, int BN, int WM, int WN, int NSX, int BK, bool F16>
__global__ __launch_bounds__(WM * WN * 64) void igemm_bf16_kernel(const Args p) {
    constexpr int NS = NSX == 1 ? 1 : 2, NB = NSX == 2 ? 2 : 1;      // operand planes: A (activations / dy), B (weights / x)
    constexpr int NT = WM * WN * 64;        // 256 or 512 threads
    constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);
    constexpr int TPR_A = BK / 4, TPR_B = BK / 8;      // threads per tile row: float4 gathers / 16-B weight chunks
    constexpr int RA = BM * TPR_A / NT;     // float4 gathers per thread
    constexpr int RB = BN * TPR_B / NT;     // 16-B weight chunks per thread per plane
    constexpr int AROWS = NT / TPR_A, BROWS = NT / TPR_B;
    constexpr int PLANE_A = BM * BK * 2, PLANE_B = BN * BK * 2;
    constexpr int STAGE = NS * PLANE_A + NB * PLANE_B;
    // two LDS stages: k-block t is multiplied out of one while k-block t+1 is converted into the other -> ONE barrier
    // per k-block; 64 KB at 128x128 (2 workgroups per CU)
    // BK = 32: ONE stage (32 KB at 128x128) so that four or five workgroups share a CU and cover each other's waits
    // (same finding as for wgrad); BK = 64 keeps two stages
    constexpr int NSTAGE = BK == 32 ? 1 : 2;
    __shared__ __attribute__((aligned(16))) unsigned char smem[NSTAGE * STAGE];

    const Geom &g = p.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    const int tile = hoig_xcd_remap(blockIdx.x, p.nblk);
    const int m0 = (tile / p.nblk_n) * BM, n0 = (tile % p.nblk_n) * BN;

    const int kc = (tid % TPR_A) * 4, lrow = tid / TPR_A;
    int pb[RA], bh[RA], bw[RA];
#pragma unroll
    for (int i = 0; i < RA; ++i) {
        const int m = m0 + lrow + AROWS * i;
        if (m < p.M) {
            int b, hp, wp;
            decode_m(g, m, b, hp, wp);
            pb[i] = b * g.Hg;
            bh[i] = row_base(g, hp);
            bw[i] = row_base(g, wp);
        } else {
            pb[i] = -1;
            bh[i] = bw[i] = 0;
        }
    }
    int t_hp = 0, t_wp = 0;
    if (g.tile_skip) {
        int b;
        decode_m(g, m0, b, t_hp, t_wp);
    }
    const int brow = tid / TPR_B, bchunk = tid % TPR_B;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float4 ra[RA];
    uint4 rbh[RB], rbl[RB];
    // K is walked tap by tap ((r,s) outer, 32-channel blocks inner).  Everything that depends only on the tap -- the
    // validity and the address of each gathered pixel row -- is computed once per tap, so the per-k-block VALU work is
    // one pointer add per load plus the bf16 split (MFMA and VALU of ONE wave serialise; this keeps the matrix pipe fed).
    const int cpb = g.Cg / BK, RS = g.R * g.S;
    const float *aptr[RA];
    const unsigned short *wrow_h[RB], *wrow_l[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int n = n0 + brow + BROWS * i;
        const size_t o = plane_index(n, bchunk * 8, p.K);
        wrow_h[i] = n < p.N ? p.Wh + o : nullptr;
        wrow_l[i] = (NB == 2 && n < p.N) ? p.Wl + o : nullptr;
    }
    int aoff[RA], boff[RB];
#pragma unroll
    for (int i = 0; i < RA; ++i) aoff[i] = lds_off<BK>(lrow + AROWS * i, kc);
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int row = brow + BROWS * i;
        boff[i] = row * (BK * 2) + ((bchunk ^ lds_swz<BK>(row)) << 4);
    }
    // split-K: this workgroup multiplies k-blocks [begin, begin + steps_per_split) of the (tap, channel-block) walk
    const int begin = p.ksplit > 1 ? (int)blockIdx.y * p.steps_per_split : 0;
    int steps_left = p.ksplit > 1 ? min(p.steps_per_split, RS * cpb - begin) : 0x7fffffff;
    int rs = begin / cpb - 1, cb = cpb - 1, wk = 0;
    int cb_next_tap = begin - (begin / cpb) * cpb;      // channel block to start the first tap at
    auto advance = [&]() -> bool {      // move (rs, cb) to the next live k-block; false when K is exhausted
        if (steps_left-- <= 0) return false;
        if (++cb < cpb) return true;
        cb = cb_next_tap;
        cb_next_tap = 0;
        do {
            ++rs;
        } while (rs < RS && g.tile_skip && !tap_alive(g, t_hp, t_wp, rs));
        if (rs >= RS) return false;
        const int r = rs / g.S, s_ = rs - r * g.S;
        wk = rs * g.Cg;
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            aptr[i] = nullptr;
            if (pb[i] >= 0) {
                const int hg = gcoord(g, bh[i], r, g.Hg), wg = gcoord(g, bw[i], s_, g.Wg);
                if (hg >= 0 && wg >= 0) aptr[i] = p.A + ((size_t)(pb[i] + hg) * g.Wg + wg) * g.Cg + kc;
            }
        }
        return true;
    };
    auto load_tiles = [&]() {
        const int c = cb * BK;
#pragma unroll
        for (int i = 0; i < RA; ++i)
            ra[i] = aptr[i] ? *reinterpret_cast<const float4 *>(aptr[i] + c) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            rbh[i] = wrow_h[i] ? *reinterpret_cast<const uint4 *>(wrow_h[i] + (size_t)(wk + c) * 32) : make_uint4(0, 0, 0, 0);
            if (NB == 2)
                rbl[i] = wrow_l[i] ? *reinterpret_cast<const uint4 *>(wrow_l[i] + (size_t)(wk + c) * 32) : make_uint4(0, 0, 0, 0);
        }
    };
    auto store_tiles = [&](int stage) {
        unsigned char *Ah = smem + stage * STAGE, *Al = Ah + PLANE_A;
        unsigned char *Bh = Ah + NS * PLANE_A, *Bl = Bh + PLANE_B;
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            uint2 hi, lo;
            split4t<F16>(ra[i], hi, lo);
            *reinterpret_cast<uint2 *>(Ah + aoff[i]) = hi;
            if (NS == 2) *reinterpret_cast<uint2 *>(Al + aoff[i]) = lo;
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            *reinterpret_cast<uint4 *>(Bh + boff[i]) = rbh[i];
            if (NB == 2) *reinterpret_cast<uint4 *>(Bl + boff[i]) = rbl[i];
        }
    };
    int aread[TM], bread[TN];       // ds_read_b128 offsets of this lane's fragments for ks = 0 (ks = 1: chunk ^ 2)
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int row = wm * (TM * 32) + i * 32 + l31;
        aread[i] = row * (BK * 2) + ((lh ^ lds_swz<BK>(row)) << 4);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int row = wn * (TN * 32) + j * 32 + l31;
        bread[j] = row * (BK * 2) + ((lh ^ lds_swz<BK>(row)) << 4);
    }

    bool more = advance();
    if (more) {
        load_tiles();
        store_tiles(0);
    }
    __syncthreads();
    int cur = 0;
    while (more) {
        const bool nxt = advance();
        if (nxt) load_tiles();
        const unsigned char *Ah = smem + cur * STAGE, *Al = Ah + PLANE_A;
        const unsigned char *Bh = Ah + NS * PLANE_A, *Bl = Bh + PLANE_B;
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            bf16x8 ah[TM], al[TM], bhf[TN], blf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int off = aread[i] ^ (ks << 5);
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
        if (NSTAGE == 2) {
            if (nxt) store_tiles(cur ^ 1);
            __syncthreads();
            cur ^= 1;
        } else {
            __syncthreads();
            if (nxt) store_tiles(0);
            __syncthreads();
        }
        more = nxt;
    }

    // bias values of this lane's TN output columns, loaded once (a load inside the store loop is re-issued and waited for
    // per element: the stores may alias it)
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
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * (TM * 32) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (m >= p.M) continue;
            size_t pix = m;
            if (g.phase_major) {
                int b, hp, wp;
                decode_m(g, m, b, hp, wp);
                pix = ((size_t)b * g.Hp + hp) * g.Wp + wp;
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wn * (TN * 32) + j * 32 + l31;
                if (n < p.N) {
                    float v = acc[i][j][r] * p.oscale;
                    if (p.ksplit > 1) {
                        if (blockIdx.y == 0) v += bias_r[j];
                        atomicAdd(&p.C[pix * p.N + n], v);
                    } else {
                        v += bias_r[j];
                        p.C[pix * p.N + n] = fast_act(v, nslope, special, p.act, p.slope);
                    }
                }
            }
        }
    }
}

template <int BM, int BN, int WM, int WN, int BK = 32>
int launch(Args a, int ns, hipStream_t st) {
    constexpr int NT = WM * WN * 64;
    const int nbm = (int)hoig_cdiv(a.M, BM), nbn = (int)hoig_cdiv(a.N, BN);
    a.nblk_n = nbn;
    a.nblk = nbm * nbn;
    if (a.g.gatherT && a.g.stride == 2 && (a.g.Hp % 2 == 0) && (a.g.Wp % 2 == 0)) {
        a.g.phase_major = 1;
        const long per_phase = (long)a.g.Bn * (a.g.Hp / 2) * (a.g.Wp / 2);
        a.g.tile_skip = (per_phase % BM == 0) ? 1 : 0;
    }
    // few output tiles but a long K (the attention MLP: 128 outputs, K = 25*C): split K over blockIdx.y
    a.ksplit = 1;
    a.steps_per_split = 0;
    const int steps = (a.K / BK);
    constexpr int sk_target = 1024;      // (sweep 512 / 768 / 1024: 2.07 / 1.90 / 1.91 ms for the attention forward GEMMs)
    constexpr int sk_maxblk = 192;
    if (a.nblk < sk_maxblk && steps >= 32 && a.act == HOIG_ACT_NONE && !a.g.tile_skip) {
        int want = (int)hoig_cdiv(sk_target, a.nblk);
        if (want > steps / 8) want = steps / 8;
        if (want > 1) {
            a.steps_per_split = (int)hoig_cdiv(steps, want);
            a.ksplit = (int)hoig_cdiv(steps, a.steps_per_split);
            if (hipMemsetAsync(a.C, 0, (size_t)a.M * a.N * sizeof(float), st) != hipSuccess) return HOIG_ELAUNCH;
        }
    }
    dim3 grid(a.nblk, a.ksplit);
    if (BM == 128 && BN == 128) WN == 4 ? HOIG_ROUTE_FD(a.f16, igemm_bf16_128x128w) : HOIG_ROUTE_FD(a.f16, igemm_bf16_128x128);
    else if (BN == 128) HOIG_ROUTE_FD(a.f16, igemm_bf16_64x128);
    else if (BM == 128) HOIG_ROUTE_FD(a.f16, igemm_bf16_128x64);
    else HOIG_ROUTE_FD(a.f16, igemm_bf16_64x64);
    HOIG_NS_SWITCH(ns, HOIG_F16_SWITCH(a.f16, return hoig_launch<igemm_bf16_kernel<BM, BN, WM, WN, NSX, BK, F16X>>(grid, NT, 0, st, a)));
}

// the norm a forward launch applies to its gathered tensor (HaloArgs::in_scale ...)
struct InNorm {
    const float *scale, *shift;
    int relu_c0;
};
// the second problem of a grouped launch (hoig_conv2d_*_pair): same descriptor, its own tensors
struct PairSet {
    const float *a;
    const unsigned short *wh, *wl;
    const float *bias, *addend;
    float *c;
};

// One launch of the packed-plane dispatcher; an entry point fills the fields it uses.
// a2 / cg1: the gathered tensor is [a | a2] along channels; c2 / n1: the output is [c | c2] (3x3 stride-1 halo kernel only:
// HOIG_EUNSUPPORTED for every other shape, the caller then concatenates / slices itself)
struct Conv {
    const hoig_conv_desc *d = nullptr;
    const float *a = nullptr;                        // the gathered tensor: x (forward) / dy (data gradient)
    const unsigned short *wh = nullptr, *wl = nullptr;
    const float *bias = nullptr;
    float *c = nullptr;                              // the output: y / dx
    bool dgrad = false;
    hipStream_t st = nullptr;
    const float *a2 = nullptr;                       // second input: the gathered tensor is [a | a2], a holds cg1 channels
    int cg1 = 0;
    float *c2 = nullptr;                             // second output: [c | c2], c holds n1 channels
    int n1 = 0;
    const float *addend = nullptr;                   // added to the output in the epilogue
    double *stats = nullptr;                         // per-image channel sums of the output (hoig_stats_add)
    bool a_split = false;                            // a holds pre-split bf16 hi | lo planes
    const PairSet *g2 = nullptr;
    const InNorm *in = nullptr;
};

// What the halo kernels (HaloArgs) and the flattened-axis kernels (FlatArgs) take over from a launch and its GEMM view `p`: tensors,
// sizes, epilogue.  The grid the taps walk, and whatever only one route has, is set by that route's block of run().
HaloArgs halo_args(const Conv &q, const Args &p) {
    HaloArgs h;
    h.A = q.a; h.Wh = q.wh; h.Wl = q.wl; h.bias = q.bias; h.C = q.c;
    h.Bn = q.d->B; h.Cg = p.g.Cg; h.N = p.N; h.K = p.K;
    h.act = p.act; h.slope = p.slope;
    h.f16 = p.f16; h.oscale = p.oscale;
    h.addend = q.addend;
    h.stats = q.stats;
    return h;
}
FlatArgs flat_args(const Conv &q, const Args &p, int ks) {
    FlatArgs f;
    f.A = q.a; f.Wh = q.wh; f.Wl = q.wl; f.bias = q.bias; f.C = q.c; f.addend = q.addend;
    f.Bn = q.d->B; f.KS = ks; f.act = p.act; f.slope = p.slope;
    f.Cg = p.g.Cg; f.N = p.N; f.K = p.K; f.flip = q.dgrad ? 1 : 0; f.f16 = p.f16; f.oscale = p.oscale;
    return f;
}

int run(const Conv &q) {
    const hoig_conv_desc *d = q.d;
    if (q.in && (q.dgrad || d->R != 3 || d->S != 3 || d->stride != 1 || d->pad != 1 || d->transposed || q.a_split || q.g2))
        return HOIG_EUNSUPPORTED;
    Args p;
    p.A = q.a; p.Wh = q.wh; p.Wl = q.wl; p.bias = q.bias; p.C = q.c;
    p.f16 = q.dgrad ? 0 : 1;                       // forward: fp16-split operands over the 2^8-scaled forward planes
    p.oscale = q.dgrad ? 1.f : 1.f / W_SCALE_F16;
    Geom &g = p.g;
    g.Bn = d->B;
    if (!q.dgrad) {
        g.Hg = d->Hi; g.Wg = d->Wi; g.Cg = d->Ci; g.Hp = d->Ho; g.Wp = d->Wo;
        g.gatherT = d->transposed ? 1 : 0;
        p.M = d->B * d->Ho * d->Wo; p.N = d->Co; p.K = d->R * d->S * d->Ci;
        p.act = d->act; p.slope = d->slope;
    } else {
        g.Hg = d->Ho; g.Wg = d->Wo; g.Cg = d->Co; g.Hp = d->Hi; g.Wp = d->Wi;
        g.gatherT = d->transposed ? 0 : 1;
        p.M = d->B * d->Hi * d->Wi; p.N = d->Ci; p.K = d->R * d->S * d->Co;
        p.act = HOIG_ACT_NONE; p.slope = 0.f;
    }
    g.R = d->R; g.S = d->S; g.stride = d->stride; g.pad = d->pad;
    if (g.Cg % 32 != 0) return HOIG_EUNSUPPORTED;
    if (g.gatherT && g.stride == 2 && ((g.Hp | g.Wp) & 1)) return HOIG_EUNSUPPORTED;
    const int ns = ns_of_precision(d->precision);
    if (ns == 2 && !q.wl) return HOIG_EINVAL;
    const long t128 = hoig_cdiv(p.M, 128);
    if (p.N <= 32 || p.N % 32 != 0) return HOIG_EUNSUPPORTED;
    if (q.dgrad && !d->transposed && d->R == 1 && d->S == 1 && d->stride == 1 && d->pad == 0 && g.Cg == 128 &&
        p.N >= 1024 && p.N % 64 == 0 && p.M % 128 == 0 && !q.a2 && !q.c2 && !q.addend && !q.stats)
        return launch_dgrad_thin(q.a, q.wh, q.wl, q.c, p.M, p.N, ns, q.st);
    // stride-1 "same" convolutions (and their data gradients): LDS-resident input halo, weights streamed per tap
    if (!d->transposed && d->stride == 1 && d->R == d->S && 2 * d->pad == d->R - 1 && (d->R == 1 || d->R == 3 || d->R == 5) &&
        d->Wi % 32 == 0 && d->Hi % 4 == 0 && p.N % 64 == 0 &&
        (long)(q.g2 ? 2 : 1) * d->B * (d->Hi / 4) * (d->Wi / 32) * ((p.N + 127) / 128) >= 160) {   // fewer tiles: the generic kernel splits K
        HaloArgs h = halo_args(q, p);
        h.A2 = q.a2; h.cg1 = q.cg1; h.C2 = q.c2; h.n1 = q.n1;
        h.a_split = q.a_split ? 1 : 0;
        if (q.in) { h.in_scale = q.in->scale; h.in_shift = q.in->shift; h.in_relu_c0 = q.in->relu_c0; }
        if (q.a_split && (d->R != 3 || q.a2 || !q.dgrad)) return HOIG_EUNSUPPORTED;
        if ((q.addend || q.stats) && q.c2) return HOIG_EUNSUPPORTED;
        if (q.stats && d->R != 3) return HOIG_EUNSUPPORTED;          // (only the 3x3 kernel has the statistics epilogue)
        if ((q.a2 || q.c2) && d->R != 3) return HOIG_EUNSUPPORTED;
        if (q.a2 && (q.cg1 % 32 || q.cg1 <= 0 || q.cg1 >= g.Cg)) return HOIG_EINVAL;
        if (q.c2 && (q.n1 % 64 || q.n1 <= 0 || q.n1 >= p.N)) return HOIG_EINVAL;
        h.H = d->Hi; h.W = d->Wi;
        if (q.g2) {                          // grouped launch: both problems' images in one grid (3x3 kernel of conv_halo16.hip only)
            if (d->R != 3 || q.a2 || q.c2 || q.stats) return HOIG_EUNSUPPORTED;
            h.Bn = 2 * d->B; h.b_split = d->B;
            h.A_g2 = q.g2->a; h.Wh_g2 = q.g2->wh; h.Wl_g2 = q.g2->wl; h.bias_g2 = q.g2->bias; h.addend_g2 = q.g2->addend; h.C_g2 = q.g2->c;
        }
        h.pad = d->pad;                      // dgrad: KS-1-pad == pad for "same" convolutions
        h.flip = q.dgrad ? 1 : 0;
        if (d->R == 1) return launch_halo<1>(h, ns, q.st);
        if (d->R == 3) return launch_halo3(h, ns, q.st);
        return launch_halo<5>(h, ns, q.st);
    }
    if (q.a2 || q.c2 || q.a_split || q.g2 || q.in) return HOIG_EUNSUPPORTED;
    // 3x3 "same" layers with too few tiles for the halo kernel above (N = 128 at 32 x 32: the data gradient of SPADE's 128 -> 1024
    // convolutions): a valid convolution over the zero-padded canvas on the flattened-axis kernel, split over the channel blocks
    if (hoig_tuning(HOIG_TUNE_FLAT5) >= 2 && !d->transposed && d->stride == 1 && d->R == 3 && d->S == 3 && d->pad == 1 &&
        p.N % 128 == 0 && !q.stats) {
        FlatArgs f = flat_args(q, p, 3);
        f.Hc = d->Hi + 2; f.Wc = d->Wi + 2;
        f.Hs = d->Hi; f.Ws = d->Wi; f.oy = f.ox = 1; f.Hd = d->Hi; f.Wd = d->Wi;
        const int rc = launch_flat_m16(f, ns, q.st);
        if (rc != HOIG_EUNSUPPORTED) return rc;
    }
    // the attention's VALID 5x5 convolutions over narrow maps (and their data gradients) on the flattened-axis halo kernel
    if (hoig_tuning(HOIG_TUNE_FLAT5) != 0 && !d->transposed && d->stride == 1 && d->R == 5 && d->S == 5 && d->pad == 0 &&
        d->Ho == d->Hi - 4 && d->Wo == d->Wi - 4 && p.N % 128 == 0 && !q.stats) {
        FlatArgs f = flat_args(q, p, 5);
        f.Hc = d->Hi; f.Wc = d->Wi;
        if (!q.dgrad) {
            f.Hs = d->Hi; f.Ws = d->Wi; f.oy = f.ox = 0; f.Hd = d->Ho; f.Wd = d->Wo;
        } else {
            f.Hs = d->Ho; f.Ws = d->Wo; f.oy = f.ox = 4; f.Hd = d->Hi; f.Wd = d->Wi;
        }
        const int rc = launch_flat_m16(f, ns, q.st);
        if (rc != HOIG_EUNSUPPORTED) return rc;
        // the wide maps (72 / 68 / 136 / 132 pixels), whose flattened halo does not fit: 16 x 16 pixel tiles (conv_halo5.hip)
        if (hoig_tuning(HOIG_TUNE_HALO5) != 0) {
            const int rc5 = launch_halo5_m16(f, ns, q.st);
            if (rc5 != HOIG_EUNSUPPORTED) return rc5;
        }
    }
    // stride-2 3x3 pad-1 layers on the parity-phase halo kernel.  gather: Conv2d forward / ConvTranspose2d data gradient;
    // scatter: ConvTranspose2d forward / Conv2d data gradient
    if (d->stride == 2 && d->R == 3 && d->S == 3 && d->pad == 1 && d->Hi % 2 == 0 && d->Wi % 2 == 0 &&
        p.N % 64 == 0) {
        // fine / coarse grids: Conv2d: fine = input (Hi), coarse = output (Ho = Hi/2); ConvTranspose2d: fine = output
        const int fine_h = d->transposed ? d->Ho : d->Hi, fine_w = d->transposed ? d->Wo : d->Wi;
        const int coarse_h = d->transposed ? d->Hi : d->Ho, coarse_w = d->transposed ? d->Wi : d->Wo;
        if (fine_h == 2 * coarse_h && fine_w == 2 * coarse_w && coarse_w % 32 == 0 && coarse_h % 4 == 0) {
            HaloArgs h = halo_args(q, p);
            h.pad = 1;
            const bool gather = !g.gatherT;      // the operand is read at 2*o - 1 + tap (fine grid) -> gather mode
            if (gather) {
                h.H = fine_h; h.W = fine_w;
                return launch_halo_s2<false>(h, ns, q.st);
            }
            h.H = coarse_h; h.W = coarse_w;
            return launch_halo_s2<true>(h, ns, q.st);
        }
    }
    if (q.addend || q.stats) return HOIG_EUNSUPPORTED;
    // on v_mfma_f32_16x16x32 (conv_igemm16.hip): 1 = forward launches (three fp16 terms: +16 % on the attention's 5x5 convolutions),
    // 2 = data gradients too (two bf16 terms per k-block leave less to hide the single LDS stage behind: measured 0-25 % slower)
    const int t16 = hoig_tuning(HOIG_TUNE_IGEMM16);
    const bool m16 = t16 >= 2 || (t16 == 1 && !q.dgrad);
    if (p.N <= 64) {
        if (t128 >= 512) return m16 ? launch_igemm_m16(p, ns, 3, q.st) : launch<128, 64, 2, 2>(p, ns, q.st);
        return m16 ? launch_igemm_m16(p, ns, 4, q.st) : launch<64, 64, 2, 2>(p, ns, q.st);
    }
    const long n128 = hoig_cdiv(p.N, 128);
    // fewer than two 128x128 workgroups per CU: run 8 waves per workgroup so every SIMD still holds two waves and one
    // wave's bf16 split (VALU) overlaps the other's MFMAs.  (A BK = 64, double-buffered variant measured slower.)
    if (t128 * n128 >= 512) return m16 ? launch_igemm_m16(p, ns, 0, q.st) : launch<128, 128, 2, 2>(p, ns, q.st);
    if (t128 * n128 >= 128) return m16 ? launch_igemm_m16(p, ns, 1, q.st) : launch<128, 128, 2, 4>(p, ns, q.st);
    return m16 ? launch_igemm_m16(p, ns, 2, q.st) : launch<64, 128, 2, 2>(p, ns, q.st);
}

// what every entry point asks before it fills a Conv: a descriptor with a 16-bit precision and the tensors it cannot do without
template <class... T>
bool usable(const hoig_conv_desc *d, const T *...needed) {
    return d && (... && needed) && is_16bit_precision(d->precision);
}

}  // namespace

extern "C" int hoig_conv2d_fwd_packed(const hoig_conv_desc *d, const float *x, const uint16_t *w_hi, const uint16_t *w_lo,
                                      const float *bias, float *y, hoig_stream_t stream) {
    if (!usable(d, x, w_hi, y)) return HOIG_EINVAL;
    return run(Conv{.d = d, .a = x, .wh = w_hi, .wl = w_lo, .bias = bias, .c = y, .st = (hipStream_t)stream});
}

extern "C" int hoig_conv2d_bwd_data_packed(const hoig_conv_desc *d, const float *dy, const uint16_t *wt_hi,
                                           const uint16_t *wt_lo, float *dx, hoig_stream_t stream) {
    if (!usable(d, dy, wt_hi, dx)) return HOIG_EINVAL;
    return run(Conv{.d = d, .a = dy, .wh = wt_hi, .wl = wt_lo, .c = dx, .dgrad = true, .st = (hipStream_t)stream});
}

// y = conv(x) and, from the same epilogue, stats[b][0/1][co] += sum / sum of squares of y over image b (HOIG_EUNSUPPORTED where the
// layer's kernel has no such epilogue: 3x3 stride-1 "same" and 3x3 stride-2 layers on the halo kernels have it)
extern "C" int hoig_conv2d_fwd_packed_stats(const hoig_conv_desc *d, const float *x, const uint16_t *w_hi, const uint16_t *w_lo,
                                            const float *bias, float *y, double *stats, hoig_stream_t stream) {
    if (!usable(d, x, w_hi, y, stats)) return HOIG_EINVAL;
    return run(Conv{.d = d, .a = x, .wh = w_hi, .wl = w_lo, .bias = bias, .c = y, .st = (hipStream_t)stream, .stats = stats});
}
extern "C" int hoig_conv2d_cat_fwd_packed_stats(const hoig_conv_desc *d, const float *x1, int C1, const float *x2,
                                                const uint16_t *w_hi, const uint16_t *w_lo, const float *bias, float *y,
                                                double *stats, hoig_stream_t stream) {
    if (!usable(d, x1, x2, w_hi, y, stats)) return HOIG_EINVAL;
    return run(Conv{.d = d, .a = x1, .wh = w_hi, .wl = w_lo, .bias = bias, .c = y, .st = (hipStream_t)stream, .a2 = x2, .cg1 = C1, .stats = stats});
}

// forward of conv -> instance norm (+ affine) -> ReLU -> THIS 3x3 stride-1 convolution in INFERENCE: x (and x2) are RAW, the loader
// applies x * in_scale + in_shift per (image, gathered channel) and ReLU on channels >= in_relu_c0 (include/hoig_kernels.h)
extern "C" int hoig_conv2d_fwd_packed_normin(const hoig_conv_desc *d, const float *x, int C1, const float *x2, const uint16_t *w_hi,
                                             const uint16_t *w_lo, const float *bias, const float *in_scale, const float *in_shift,
                                             int in_relu_c0, float *y, double *stats, hoig_stream_t stream) {
    if (!usable(d, x, w_hi, y, in_scale, in_shift) || in_relu_c0 < 0) return HOIG_EINVAL;
    const InNorm in{in_scale, in_shift, in_relu_c0};
    return run(Conv{.d = d, .a = x, .wh = w_hi, .wl = w_lo, .bias = bias, .c = y, .st = (hipStream_t)stream, .a2 = x2, .cg1 = x2 ? C1 : 0,
                    .stats = stats, .in = &in});
}

// dx = data gradient + addend (HOIG_EUNSUPPORTED where the layer's kernel has no such epilogue: the caller adds separately)
extern "C" int hoig_conv2d_bwd_data_packed_add(const hoig_conv_desc *d, const float *dy, const uint16_t *wt_hi,
                                               const uint16_t *wt_lo, const float *addend, float *dx, hoig_stream_t stream) {
    if (!usable(d, dy, wt_hi, dx, addend)) return HOIG_EINVAL;
    return run(Conv{.d = d, .a = dy, .wh = wt_hi, .wl = wt_lo, .c = dx, .dgrad = true, .st = (hipStream_t)stream, .addend = addend});
}

// data gradient (+ addend, nullable) from PRE-SPLIT dy (include/hoig_kernels.h): the 3x3 stride-1 "same" layers on conv_halo16.hip
extern "C" int hoig_conv2d_bwd_data_packed_split(const hoig_conv_desc *d, const uint16_t *dy_split, const uint16_t *wt_hi,
                                                 const uint16_t *wt_lo, const float *addend, float *dx, hoig_stream_t stream) {
    if (!usable(d, dy_split, wt_hi, dx)) return HOIG_EINVAL;
    if (d->precision == HOIG_PREC_BF16X3 || d->transposed || d->stride != 1 || d->R != 3 || d->S != 3) return HOIG_EUNSUPPORTED;
    return run(Conv{.d = d, .a = reinterpret_cast<const float *>(dy_split), .wh = wt_hi, .wl = wt_lo, .c = dx, .dgrad = true,
                    .st = (hipStream_t)stream, .addend = addend, .a_split = true});
}

// GROUPED launches (include/hoig_kernels.h): two convolutions of ONE descriptor -- different tensors, different weights -- as one grid
extern "C" int hoig_conv2d_fwd_packed_pair(const hoig_conv_desc *d, const float *xa, const float *xb, const uint16_t *wa_hi,
                                           const uint16_t *wa_lo, const uint16_t *wb_hi, const uint16_t *wb_lo, const float *bias_a,
                                           const float *bias_b, float *ya, float *yb, hoig_stream_t stream) {
    if (!usable(d, xa, xb, wa_hi, wb_hi, ya, yb)) return HOIG_EINVAL;
    if (d->transposed || d->stride != 1 || d->R != 3 || d->S != 3) return HOIG_EUNSUPPORTED;
    const PairSet g2{xb, wb_hi, wb_lo, bias_b, nullptr, yb};
    return run(Conv{.d = d, .a = xa, .wh = wa_hi, .wl = wa_lo, .bias = bias_a, .c = ya, .st = (hipStream_t)stream, .g2 = &g2});
}
extern "C" int hoig_conv2d_bwd_data_packed_split_pair(const hoig_conv_desc *d, const uint16_t *dys_a, const uint16_t *dys_b,
                                                      const uint16_t *wta_hi, const uint16_t *wta_lo, const uint16_t *wtb_hi,
                                                      const uint16_t *wtb_lo, const float *addend_a, const float *addend_b, float *dxa,
                                                      float *dxb, hoig_stream_t stream) {
    if (!usable(d, dys_a, dys_b, wta_hi, wtb_hi, dxa, dxb)) return HOIG_EINVAL;
    if (d->precision == HOIG_PREC_BF16X3 || d->transposed || d->stride != 1 || d->R != 3 || d->S != 3) return HOIG_EUNSUPPORTED;
    if ((addend_a == nullptr) != (addend_b == nullptr)) return HOIG_EINVAL;
    const PairSet g2{reinterpret_cast<const float *>(dys_b), wtb_hi, wtb_lo, nullptr, addend_b, dxb};
    return run(Conv{.d = d, .a = reinterpret_cast<const float *>(dys_a), .wh = wta_hi, .wl = wta_lo, .c = dxa, .dgrad = true,
                    .st = (hipStream_t)stream, .addend = addend_a, .a_split = true, .g2 = &g2});
}

// conv(cat[x1, x2]) and its data gradient [dx1 | dx2] without materialising the concatenation (3x3 stride-1 "same" only)
extern "C" int hoig_conv2d_cat_fwd_packed(const hoig_conv_desc *d, const float *x1, int C1, const float *x2,
                                          const uint16_t *w_hi, const uint16_t *w_lo, const float *bias, float *y,
                                          hoig_stream_t stream) {
    if (!usable(d, x1, x2, w_hi, y)) return HOIG_EINVAL;
    return run(Conv{.d = d, .a = x1, .wh = w_hi, .wl = w_lo, .bias = bias, .c = y, .st = (hipStream_t)stream, .a2 = x2, .cg1 = C1});
}
extern "C" int hoig_conv2d_cat_bwd_data_packed(const hoig_conv_desc *d, const float *dy, const uint16_t *wt_hi,
                                               const uint16_t *wt_lo, float *dx1, int C1, float *dx2,
                                               hoig_stream_t stream) {
    if (!usable(d, dy, wt_hi, dx1, dx2)) return HOIG_EINVAL;
    return run(Conv{.d = d, .a = dy, .wh = wt_hi, .wl = wt_lo, .c = dx1, .dgrad = true, .st = (hipStream_t)stream, .c2 = dx2, .n1 = C1});
}
