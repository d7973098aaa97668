// The convolution launcher that ran last on this host thread (hoig_conv_last_route, include/hoig_kernels.h): every convolution
// launcher stores its id immediately before its kernel launch.  One thread-local integer per pass on the host; nothing on the device.
// One id per launcher and per template variant that differs in tiling or in how it accumulates.  Launchers that the forward and the
// data gradient share (the packed-plane dispatcher, the fp32 implicit GEMM) have one id per pass: fwd_<name> and dgrad_<name>.
#pragma once

// W: weight gradient, D: data gradient only, F: forward only, FD: forward and data gradient (two ids)
#define HOIG_CONV_ROUTES(W, D, F, FD)                                                                                              \
    /* conv_thin.hip: thin-input / thin-output layers; _ws: per-workgroup partials + thin_reduce_kernel, _direct: fp32 atomics */      \
    W(wgrad_thin_in_ws) W(wgrad_thin_in_direct) W(wgrad_thin_out_ws) W(wgrad_thin_out_direct)                                      \
    W(wgrad_small)                                                                                                                 \
    /* wgrad_flat.hip: the valid 5x5 layers */                                                                                    \
    W(wgrad_flat5) W(wgrad_tile5)                                                                                                  \
    /* wgrad_igemm_bf16.hip: launch_wgrad_halo by template variant */                                                             \
    W(wgrad_halo_th4) W(wgrad_halo_cm2) W(wgrad_halo_cm1) W(wgrad_halo_s2_cm2) W(wgrad_halo_s2_cm1) W(wgrad_halo_5x5)              \
    W(wgrad_halo_tout) /* (transposed: Ci % 128 == 0 is asked for before this launcher, so always 128-channel workgroups) */       \
    /* wgrad_dma.hip: pre-split dy */                                                                                              \
    W(wgrad_dma) W(wgrad_dma_pair)                                                                                                 \
    W(wgrad_bf16_64) W(wgrad_bf16_128)                                                                                             \
    /* conv_igemm.hip: launch_wgrad<BM, BN> in fp32 */                                                                             \
    W(wgrad_f32_32x64) W(wgrad_f32_32x128) W(wgrad_f32_64x128) W(wgrad_f32_128x64) W(wgrad_f32_128x128)                            \
    /* conv_igemm.hip: launch_igemm<BM, BN> in fp32 */                                                                             \
    FD(igemm_f32_128x32) FD(igemm_f32_128x64) FD(igemm_f32_64x64) FD(igemm_f32_128x128) FD(igemm_f32_64x128)                       \
    /* conv_halo32.hip: launch_halo<1>, launch_halo<5> (64-channel tiles, 128 on 8 waves, 128 on 4 waves) */                       \
    FD(halo1_64) FD(halo1_128w) FD(halo1_128) FD(same5_64) FD(same5_128w) FD(same5_128)                                            \
    /* launch_halo3_one */                                                                                                         \
    FD(halo3_64) FD(halo3_128w) FD(halo3_128)                                                                                      \
    /* conv_halo16.hip: launch_halo3_m16; _split: pre-split dy, _pair: grouped launch, _normin: norm folded into the loader */     \
    FD(halo3_m16_64) FD(halo3_m16_128)                                                                                             \
    D(halo3_m16_64_split) D(halo3_m16_128_split) D(halo3_m16_64_split_pair) D(halo3_m16_128_split_pair)                            \
    F(halo3_m16_64_pair) F(halo3_m16_128_pair) F(halo3_m16_64_normin) F(halo3_m16_128_normin)                                      \
    /* conv_flat16.hip, conv_halo5.hip; _ksplit: split over K, added with atomics */                                               \
    FD(flat_m16_k3) FD(flat_m16_k5) FD(halo5_m16) FD(halo5_m16_ksplit)                                                             \
    /* stride-2 3x3: g gather, s scatter; conv_halo32.hip, conv_halo16.hip (m16), conv_s2_16.hip (m16p4: 4-row, m16p8: 8-row tiles) */ \
    FD(s2g_64) FD(s2g_128) FD(s2s_64) FD(s2s_128)                                                                                  \
    FD(s2g_m16_64) FD(s2g_m16_128) FD(s2s_m16_64) FD(s2s_m16_128)                                                                  \
    FD(s2g_m16p4_64) FD(s2g_m16p4_128) FD(s2s_m16p4_64) FD(s2s_m16p4_128) FD(s2g_m16p8_128) FD(s2s_m16p8_128)                      \
    /* conv_igemm16.hip (launch_igemm_m16 cfg 0..4) and the generic launch<BM, BN, WM, WN> of conv_igemm_bf16.hip */               \
    FD(igemm_m16_128x128) FD(igemm_m16_128x128w) FD(igemm_m16_64x128) FD(igemm_m16_128x64) FD(igemm_m16_64x64)                     \
    FD(igemm_bf16_128x128) FD(igemm_bf16_128x128w) FD(igemm_bf16_64x128) FD(igemm_bf16_128x64) FD(igemm_bf16_64x64)                \
    /* dgrad_k128.hip, conv_thin.hip, conv_small.hip */                                                                            \
    D(k128) D(thin) D(thin_out) D(small)                                                                                           \
    F(head7) F(small) F(small_ci) F(dot) F(thin) F(thin_out)                                                                       \
    /* conv_f6.hip: launch_f6 (64- / 128-channel tiles; _normin: norm folded into the loader) */                                    \
    F(f6_64) F(f6_128) F(f6_64_normin) F(f6_128_normin)

enum HoigConvRoute {
    HOIG_ROUTE_NONE = 0,
#define HOIG_R_W(n) HOIG_ROUTE_##n,
#define HOIG_R_D(n) HOIG_ROUTE_dgrad_##n,
#define HOIG_R_F(n) HOIG_ROUTE_fwd_##n,
#define HOIG_R_FD(n) HOIG_ROUTE_fwd_##n, HOIG_ROUTE_dgrad_##n,
    HOIG_CONV_ROUTES(HOIG_R_W, HOIG_R_D, HOIG_R_F, HOIG_R_FD)
#undef HOIG_R_W
#undef HOIG_R_D
#undef HOIG_R_F
#undef HOIG_R_FD
    HOIG_ROUTE_COUNT
};

enum { HOIG_PASS_FWD = 0, HOIG_PASS_DGRAD = 1, HOIG_PASS_WGRAD = 2 };

extern thread_local int hoig_route_last[3];          // tuning.hip

static inline void hoig_route_set(int which, int id) { hoig_route_last[which] = id; }
#define HOIG_ROUTE_W(name) hoig_route_set(HOIG_PASS_WGRAD, HOIG_ROUTE_##name)
#define HOIG_ROUTE_F(name) hoig_route_set(HOIG_PASS_FWD, HOIG_ROUTE_fwd_##name)
#define HOIG_ROUTE_D(name) hoig_route_set(HOIG_PASS_DGRAD, HOIG_ROUTE_dgrad_##name)
// a launcher both passes share; fwd: is this launch a forward?
#define HOIG_ROUTE_FD(fwd, name) ((fwd) ? HOIG_ROUTE_F(name) : HOIG_ROUTE_D(name))
