/* hoig_kernels.h -- C ABI of libhoig_hip.so: the hand-written gfx950 (CDNA4)
 * kernels behind the HOGAN generator/discriminator hot path.
 *
 * Boundary conventions (they mirror what the reference's own native layer does,
 * thirdparty/block_extractor/block_extractor_cuda.cc:5-33 and
 * thirdparty/local_attn_reshape/local_attn_reshape_cuda.cc:5-29, wrapped by
 * block_extractor.py:5-54 / local_attn_reshape.py:5-46):
 *   - plain device pointers + sizes, no torch types;
 *   - the CALLER owns and allocates every buffer (outputs, workspaces);
 *   - work is enqueued on the given hipStream_t, never synchronises, no
 *     allocation inside (graph-capturable);
 *   - return 0 on success, a negative HOIG_E* code on a rejected argument or a
 *     failed launch (the reference returns `int 1` and never checks).
 * Differences from the reference ops, by design: activations are NHWC fp32
 * ("channels-last"), conv weights are packed [Cout][kh][kw][Cin] for Conv2d AND
 * ConvTranspose2d (the host keeps the reference's logical NCHW shapes as views
 * of that storage, hoig_amd/nn.py), gradients of weights ACCUMULATE into the
 * caller's (zeroed) flat gradient buffer.
 *
 * Reference call sites each family replaces are cited per function
 * (paths relative to /root/reference/HOIG_HOv3).
 */
#ifndef HOIG_KERNELS_H
#define HOIG_KERNELS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *hoig_stream_t; /* hipStream_t */

enum { HOIG_OK = 0, HOIG_EINVAL = -1, HOIG_ELAUNCH = -2, HOIG_EUNSUPPORTED = -3 };

/* epilogue activations */
enum { HOIG_ACT_NONE = 0, HOIG_ACT_RELU = 1, HOIG_ACT_LRELU = 2, HOIG_ACT_TANH = 3, HOIG_ACT_SIGMOID = 4 };

/* arithmetic of the MFMA contraction (accumulation is always fp32):
 *   F32    v_mfma_f32_32x32x2_f32, exact fp32 products (parity mode)
 *   BF16X3 both operands split hi+lo into 16-bit halves, 3 MFMAs per k-step (hi*hi + lo*hi + hi*lo): forward launches split
 *          on fp16 (v_mfma_f32_32x32x16_f16, products to ~2^-21), backward launches on bf16 (~2^-16)
 *   F16X2  the gathered operand (activations / dy) split hi+lo, the other one (weights; x in the weight gradient) rounded
 *          to ONE 16-bit value: 2 MFMAs per k-step (hi*hi + lo*hi), ~2^-12 (fp16 forward) / ~2^-9 (bf16 backward) per product
 *   BF16   one MFMA per k-step, both operands rounded to 16 bits (fp16 forward, bf16 backward)
 *   F16F6  FORWARD only (hoig_conv2d_fwd_f6): hi*hi on fp16, the two cross terms of the split on block-scaled e2m3 (fp6)
 *          v_mfma_scale_f32_32x32x64_f8f6f4 (one E8M0 scale per 32 channels): BF16X3's three terms at 1.6 instead of 3 MFMA
 *          units per product; shapes outside that kernel run as BF16X3 */
enum { HOIG_PREC_F32 = 0, HOIG_PREC_BF16X3 = 1, HOIG_PREC_BF16 = 2, HOIG_PREC_F16X2 = 3, HOIG_PREC_F16F6 = 4 };

/* One convolution problem.  NHWC activations, weights [Co][R][S][Ci].
 * transposed=0: y = conv2d(x, w, stride, pad)            x:[B,Hi,Wi,Ci] y:[B,Ho,Wo,Co]
 * transposed=1: y = conv_transpose2d(x, w, stride, pad)  (output_padding implied by Ho,Wo)
 * Replaces the cuDNN convolutions reached from generator.py:15-235,
 * spade.py:18-22, discriminator.py:29-49, extract_attn.py:18-20, vgg19.py:56. */
typedef struct hoig_conv_desc {
    int32_t B, Hi, Wi, Ci;
    int32_t Ho, Wo, Co;
    int32_t R, S;
    int32_t stride, pad;
    int32_t transposed;
    int32_t act;       /* forward epilogue: HOIG_ACT_* applied after +bias */
    float slope;       /* LeakyReLU slope */
    int32_t precision; /* HOIG_PREC_* */
} hoig_conv_desc;

int hoig_conv2d_fwd(const hoig_conv_desc *d, const float *x, const float *w, const float *bias /*nullable*/,
                    float *y, hoig_stream_t stream);
/* dx = d(loss)/dx given dy (dy already carries the activation derivative) */
int hoig_conv2d_bwd_data(const hoig_conv_desc *d, const float *dy, const float *w, float *dx, hoig_stream_t stream);
/* dw += ..., dbias += ... (atomic accumulation into caller-zeroed buffers; dbias nullable) */
int hoig_conv2d_bwd_weight(const hoig_conv_desc *d, const float *x, const float *dy, float *dw, float *dbias,
                           hoig_stream_t stream);

/* PRE-SPLIT gradients (round 5).  The two-term backward arithmetic (HOIG_PREC_F16X2) multiplies bf16(dy) and bf16(dy - bf16(dy)) with
 * one bf16 plane of the other operand; the kernels above make that split of every dy tile in every workgroup that loads it.  A "split
 * tensor" holds it once: for an fp32 NHWC tensor [.., C] the same 4 bytes per element laid out per pixel as [hi: C x bf16][lo: C x bf16].
 * hoig_split_planes_bf16 converts (C % 4 == 0); producers of gradients (hoig_inorm_tile_bwd_split ...) write it directly.  The
 * consumers below compute exactly what their fp32-dy counterparts compute (same two MFMA terms, same accumulation order).
 * hoig_conv2d_bwd_weight_split: stride-1 "same" 3x3 layers with Wo % 32 == 0, Ho % 4 == 0, Co % 128 == 0, Ci % 32 == 0 in
 * HOIG_PREC_F16X2 / HOIG_PREC_BF16 (the lo plane is not read then), no bias gradient; HOIG_EUNSUPPORTED otherwise. */
int hoig_split_planes_bf16(const float *x, uint16_t *out, int64_t npix, int C, hoig_stream_t stream);
/* split -> fp32 (hi + lo; out may alias nothing): for a consumer that has no pre-split form */
int hoig_unsplit_planes_bf16(const uint16_t *in, float *out, int64_t npix, int C, hoig_stream_t stream);
/* hoig_inorm_bwd_add_ld / hoig_inorm_bwd_fused_add with dx written as a split tensor (same arguments otherwise; addend stays fp32) */
int hoig_inorm_bwd_add_ld_split(const float *x, const float *mean, const float *rstd, int mode, const float *p0, const float *p1,
                                int ld_p, const float *y, const float *dy, int act, float slope, const float *addend /*nullable*/,
                                uint16_t *dx_split, float *dp0, float *dp1, int B, int HW, int C, void *workspace,
                                hoig_stream_t stream);
int hoig_inorm_bwd_fused_add_split(const float *x, const float *mean, const float *rstd, int mode, const float *p0, const float *p1,
                                   int ld_p, const float *y, const float *dy, int act, float slope, const float *addend /*nullable*/,
                                   uint16_t *dx_split, float *dp0, float *dp1, int B, int HW, int C, hoig_stream_t stream);
/* ---- Winograd F(2x2,3x3) forward for stride-1 "same" 3x3 layers (round 6; hoig_amd/csrc/conv_wino.hip): 16
 *      element-wise products per 2 x 2 outputs instead of 36, on three fp16 terms like the direct forward (HOIG_PREC_BF16X3): U = G (2^8 w) G^T
 *      is made once per weight version by hoig_pack_conv_weight_wino -- u_hi / u_lo: hoig_wino_plane_halfs(Co, Ci) = 16 Co Ci fp16 values
 *      each, in MFMA A-fragment order [position][Co / 16][Ci / 32][64 lanes][8] -- V = B^T d B is made in the kernel from the fp32 input
 *      and split after the transform, the accumulators are fp32, Y = A^T M A, then 2^-8, bias (nullable), activation.  Hi % 16 == 0,
 *      Wi % 16 == 0, Ci % 32 == 0, Co % 64 == 0; HOIG_EUNSUPPORTED otherwise (the caller then uses hoig_conv2d_fwd_packed).  Replaces, for
 *      these layers, the same F.conv2d calls as hoig_conv2d_fwd_packed (models/networks/generator.py:9-32,35-71, spade.py:18-22). ---- */
int64_t hoig_wino_plane_halfs(int Co, int Ci);
int hoig_pack_conv_weight_wino(const float *w /*[Co][3][3][Ci]*/, int Co, int Ci, uint16_t *u_hi, uint16_t *u_lo, hoig_stream_t stream);
int hoig_conv2d_fwd_wino(const hoig_conv_desc *d, const float *x, const uint16_t *u_hi, const uint16_t *u_lo, const float *bias /*nullable*/,
                         float *y, hoig_stream_t stream);
/* ---- INFERENCE: the norm between two convolutions applied by the second one's loader (VERDICT r1-r4 "consumer half of the norm
 *      fusion"; the reference chains generator.py:16-22 (ResidualBlock: conv - IN - ReLU - conv) and :298-309 (decoder level: ConvTranspose
 *      - IN - ReLU - cat - conv)).  hoig_inorm_fold turns the statistics of the RAW tensor (hoig_inorm_stats / _stats_from_sums) and the
 *      affine parameters (nullable) into one FMA per element: scale[b][c] = rstd * gamma, shift[b][c] = beta - mean * scale, rows of
 *      ld_out floats.  hoig_conv2d_fwd_packed_normin is hoig_conv2d_fwd_packed / hoig_conv2d_cat_fwd_packed(_stats) (x2 nullable: the
 *      gathered tensor is [x | x2] with C1 channels in x) for stride-1 "same" 3x3 layers on the 8-row tilings of the 16x16x32 kernel:
 *      every in-image element of the gathered tensor becomes x * in_scale[b][c] + in_shift[b][c] (c over all Ci gathered channels), then
 *      max(., 0) for c >= in_relu_c0, before it is split for the MFMAs; the zero padding stays zero.  No backward: forward-only launches
 *      (torch.no_grad()).  HOIG_EUNSUPPORTED where that kernel cannot run the layer (the caller then normalises in a pass of its own). */
int hoig_inorm_fold(const float *mean, const float *rstd, const float *gamma /*nullable*/, const float *beta /*nullable*/, int B, int C,
                    float *scale, float *shift, int ld_out, hoig_stream_t stream);
int hoig_conv2d_fwd_packed_normin(const hoig_conv_desc *d, const float *x, int C1, const float *x2 /*nullable*/, const uint16_t *w_hi,
                                  const uint16_t *w_lo, const float *bias /*nullable*/, const float *in_scale, const float *in_shift,
                                  int in_relu_c0, float *y, double *stats /*nullable*/, hoig_stream_t stream);
int hoig_conv2d_bwd_weight_split(const hoig_conv_desc *d, const float *x, const uint16_t *dy_split, float *dw, hoig_stream_t stream);
/* dx = data gradient (+ addend when non-null: hoig_conv2d_bwd_data_packed_add) of a stride-1 "same" 3x3 Conv2d from pre-split dy, on the
 * 8-row tilings of the v_mfma_f32_16x16x32 kernel (Hi % 8 == 0, Wi % 32 == 0 and enough tiles: HOIG_EUNSUPPORTED otherwise -- the
 * caller then converts nothing and uses the fp32 entry points). */
int hoig_conv2d_bwd_data_packed_split(const hoig_conv_desc *d, const uint16_t *dy_split, const uint16_t *wt_hi, const uint16_t *wt_lo,
                                      const float *addend /*nullable*/, float *dx, hoig_stream_t stream);

/* GROUPED launches (round 5): two convolutions of ONE descriptor d (d->B images each) over different tensors with different weights --
 * src_model's and tsf_model's layer (generator.py:379-464: same architecture, separate parameters) -- as ONE grid: the tiles of the
 * second problem ride behind the first's, so the launch fills the chip where the two half-size launches each covered half of it.
 * Results are those of the two single launches.  Stride-1 "same" 3x3 layers on the 8-row tilings of conv_halo16.hip / on
 * wgrad_dma.hip; HOIG_EUNSUPPORTED otherwise (the caller launches the two problems one after the other).  The backward forms read
 * pre-split dy ('PRE-SPLIT gradients' above); addend_a / addend_b: both or neither. */
int hoig_conv2d_fwd_packed_pair(const hoig_conv_desc *d, const float *xa, const float *xb, const uint16_t *wa_hi, const uint16_t *wa_lo,
                                const uint16_t *wb_hi, const uint16_t *wb_lo, const float *bias_a /*nullable*/,
                                const float *bias_b /*nullable*/, float *ya, float *yb, hoig_stream_t stream);
int hoig_conv2d_bwd_data_packed_split_pair(const hoig_conv_desc *d, const uint16_t *dys_a, const uint16_t *dys_b, const uint16_t *wta_hi,
                                           const uint16_t *wta_lo, const uint16_t *wtb_hi, const uint16_t *wtb_lo,
                                           const float *addend_a /*nullable*/, const float *addend_b /*nullable*/, float *dxa, float *dxb,
                                           hoig_stream_t stream);
int hoig_conv2d_bwd_weight_split_pair(const hoig_conv_desc *d, const float *xa, const float *xb, const uint16_t *dys_a,
                                      const uint16_t *dys_b, float *dwa, float *dwb, hoig_stream_t stream);

/* Forward of a stride-1 'same' convolution with <= 16 output channels over Ci % 64 == 0 inputs and ONE activation PER OUTPUT
 * CHANNEL (acts: the HOIG_ACT_* code of channel f in bits [4f, 4f+4)): the generator's image / mask heads (generator.py:219-235,
 * 311-315: tanh image, sigmoid masks) evaluated as one convolution over the decoder's last feature map.  7x7 with <= 5
 * outputs: exact fp32 (VALU kernel) in every precision mode; 3x3 with <= 16 outputs: 16-bit MFMA arithmetic of d->precision;
 * HOIG_EUNSUPPORTED otherwise. */
int hoig_conv2d_fwd_heads(const hoig_conv_desc *d, const float *x, const float *w, const float *bias /*nullable*/, float *y,
                          uint64_t acts, hoig_stream_t stream);

/* 16-bit-operand fast path (HOIG_PREC_BF16X3 / HOIG_PREC_F16X2 / HOIG_PREC_BF16): weights are pre-split once per optimiser step into
 * 16-bit planes hi and lo of n rows x K reduction indices: the FORWARD planes (for_dgrad=0) hold fp16(256*w) and
 * fp16(256*w - hi) -- forward launches split their operands on fp16 and scale the accumulator by 1/256 -- the
 * DATA-GRADIENT planes (for_dgrad=1) hold bf16(w) and bf16(w - hi).  for_dgrad=0: n = co, k = (r*S+s)*Ci + ci
 * (forward GEMM); for_dgrad=1: n = ci, k = (r*S+s)*Co + co (data-gradient GEMM).  A plane is stored in 32(n) x 32(k)
 * blocks of 2 KB, and inside a block the four 8-element groups of a row are XOR-swizzled by the row: element (n, k) at
 * ((n/32)*(K/32) + k/32)*1024 + (n%32)*32 + ((((k%32)/8) ^ ((n/4)%4))*8) + k%8 (plane_index, hoig_amd/csrc/conv_bf16_common.h: the
 * block is the LDS image the kernels read), so that the weight tile of one k-step is a few fully used contiguous runs.  Co and Ci must be multiples of 32 (else HOIG_EUNSUPPORTED).  The *_packed
 * entry points return HOIG_EUNSUPPORTED for shapes outside the fast path (channels % 32 != 0, <= 32 output channels);
 * use the fp32 entry points then. */
int hoig_pack_conv_weight_bf16(const float *w, int Co, int RS, int Ci, int for_dgrad, uint16_t *hi, uint16_t *lo /*nullable*/,
                               hoig_stream_t stream);
/* The same split for every conv weight of a network's flat parameter buffer in one launch.  segs (device memory) holds
 * nseg rows of 6 int64: {element offset in flat, Co, R*S, Ci, flags (1: forward planes, 2: data-gradient planes), index
 * of the weight's first 32x32 (co, ci) tile}; ntiles = total tile count (the grid).  The planes of a weight are written
 * at the weight's own element offset of hi_f/lo_f (forward) and hi_d/lo_d (dgrad). */
int hoig_pack_conv_weights_bf16_all(const float *flat, const int64_t *segs, int nseg, int64_t ntiles, uint16_t *hi_f,
                                    uint16_t *lo_f, uint16_t *hi_d, uint16_t *lo_d, hoig_stream_t stream);
int hoig_conv2d_fwd_packed(const hoig_conv_desc *d, const float *x, const uint16_t *w_hi, const uint16_t *w_lo,
                           const float *bias /*nullable*/, float *y, hoig_stream_t stream);
int hoig_conv2d_bwd_data_packed(const hoig_conv_desc *d, const float *dy, const uint16_t *wt_hi, const uint16_t *wt_lo,
                                float *dx, hoig_stream_t stream);
/* y = conv(x) AND, from the same epilogue, the statistics of the instance norm that reads y next (generator.py:16-22 conv -> IN ->
 * ReLU): stats[b][0][co] += sum of y over image b, stats[b][1][co] += sum of y*y -- DOUBLES, B * 2 * Co of them, in
 * every entry point that takes `stats` (fp64
 * atomics, one per workgroup and channel, of the workgroup's fp32 partial; stats = the accumulators of an instance-norm workspace,
 * zero on entry: B * 4 * Co <= 2^18 floats of its pool), consumed by hoig_inorm_stats_from_sums instead of
 * a pass over y.  HOIG_EUNSUPPORTED where the layer's kernel has no such epilogue (it exists on the 3x3 stride-1 "same" and the 3x3
 * stride-2 halo kernels, Conv2d and ConvTranspose2d): the caller then runs the plain convolution and hoig_inorm_stats. */
int hoig_conv2d_fwd_packed_stats(const hoig_conv_desc *d, const float *x, const uint16_t *w_hi, const uint16_t *w_lo,
                                 const float *bias /*nullable*/, float *y, double *stats, hoig_stream_t stream);
int hoig_conv2d_cat_fwd_packed_stats(const hoig_conv_desc *d, const float *x1, int C1, const float *x2, const uint16_t *w_hi,
                                     const uint16_t *w_lo, const float *bias /*nullable*/, float *y, double *stats,
                                     hoig_stream_t stream);
/* The same for the layers the packed kernels do not take: hoig_conv2d_fwd (unpacked weights) with the sums, HOIG_EUNSUPPORTED unless
 * the layer is a thin-INPUT convolution on the MFMA path (Ci <= 8 (12 for 3x3), Co % 64 == 0, odd square stride-1 "same" kernel,
 * Hi % 4 == 0, Wi % 32 == 0, a 16-bit precision): the generator's 7x7 stems (generator.py:100,262), whose output is the largest
 * tensor an instance norm's statistics pass would re-read. */
int hoig_conv2d_fwd_stats(const hoig_conv_desc *d, const float *x, const float *w, const float *bias /*nullable*/, float *y, double *stats,
                          hoig_stream_t stream);
/* dx = data gradient + addend (addend: the gradient that reaches the same tensor through its OTHER consumer, e.g. the skip path of
 * a residual block, generator.py:29-32 `x + self.main(x)`; torch's autograd engine sums the two in a separate pass).  Returns
 * HOIG_EUNSUPPORTED for layers whose kernel has no such epilogue (everything but stride-1 "same" 1x1/3x3/5x5 and stride-2 3x3 on the halo kernels): the
 * caller then adds separately. */
int hoig_conv2d_bwd_data_packed_add(const hoig_conv_desc *d, const float *dy, const uint16_t *wt_hi, const uint16_t *wt_lo,
                                    const float *addend, float *dx, hoig_stream_t stream);

/* fp16 + block-scaled fp6 forward of 3x3 stride-1 pad-1 convolutions (hoig_amd/csrc/conv_f6.hip).  q_hi / q_lo: fp6 records of
 * the hi / lo fp16 halves of 256*w, hoig_f6_plane_bytes(Co, 9, Ci) bytes each, made by hoig_pack_conv_weight_f6 once per
 * optimiser step: [(tap * Ci/64 + ci/64)][co] records of 56 B = 2 x 24 B of e2m3 elements (32 channels each, element j in bits
 * [6j, 6j+6)) + the two E8M0 scale bytes.  w_hi: the forward hi plane of hoig_pack_conv_weight_bf16.  HOIG_EUNSUPPORTED unless
 * Ci % 64 == 0, Co % 64 == 0, H % 8 == 0, W % 32 == 0 and the launch has enough 8x32-pixel tiles to fill the chip. */
int64_t hoig_f6_plane_bytes(int Co, int RS, int Ci);
int hoig_pack_conv_weight_f6(const float *w, int Co, int RS, int Ci, uint8_t *q_hi, uint8_t *q_lo, hoig_stream_t stream);
int hoig_conv2d_fwd_f6(const hoig_conv_desc *d, const float *x, const uint16_t *w_hi, const uint8_t *q_hi, const uint8_t *q_lo,
                       const float *bias /*nullable*/, float *y, hoig_stream_t stream);
/* The same kernel with the loader and epilogue options of the three-term path (round 6: eval.py's forward runs on this arithmetic
 * by default, and the inference chain conv - IN - ReLU - conv, generator.py:16-22 / :298-309, keeps its two fusions):
 *   x2 (nullable, C1 % 32 == 0) -- the gathered tensor is [x | x2] along channels, x holding C1 of them, without the concatenated tensor;
 *   in_scale / in_shift (nullable, together; B x Ci floats from hoig_inorm_fold) and in_relu_c0 (% 32 == 0) -- the gathered tensor is
 *     RAW: x * in_scale + in_shift per (image, gathered channel) and ReLU on channels >= in_relu_c0 are applied when the halo is
 *     converted, as hoig_conv2d_fwd_packed_normin does (Ci <= 1024: the image's two rows live in LDS);
 *   stats (nullable) -- the accumulators of an instance-norm workspace, as hoig_conv2d_fwd_packed_stats.
 * Same HOIG_EUNSUPPORTED conditions as hoig_conv2d_fwd_f6. */
int hoig_conv2d_fwd_f6_ex(const hoig_conv_desc *d, const float *x, int C1, const float *x2 /*nullable*/, const uint16_t *w_hi,
                          const uint8_t *q_hi, const uint8_t *q_lo, const float *bias /*nullable*/, const float *in_scale /*nullable*/,
                          const float *in_shift /*nullable*/, int in_relu_c0, float *y, double *stats /*nullable*/, hoig_stream_t stream);
/* all eligible weights of a flat parameter buffer in one launch: rows = int64[nrows][6] = (offset of the weight in `flat`, Co,
 * RS, Ci, byte offset of its records in q_hi / q_lo (a multiple of 4), index of its first task); a task = one (output channel,
 * tap, 32 input channels) half record: Co*RS*Ci/32 per weight */
int hoig_pack_conv_weights_f6_all(const float *flat, const int64_t *rows, int nrows, int64_t ntasks, uint8_t *q_hi, uint8_t *q_lo,
                                  hoig_stream_t stream);
/* launches with fewer workgroups than this run as three fp16 terms (default 192; returns the previous value; n <= 0: query).
 * Parity tests set 1 so that the fp6 kernel is exercised at their small sizes. */
int hoig_set_f6_min_tiles(int n);

/* conv(cat[x1, x2] along channels) without materialising the concatenation (the decoder's skip convolutions,
 * generator.py:305-306): 3x3 stride-1 "same" convolutions on the fast path only -- every other shape returns
 * HOIG_EUNSUPPORTED and the caller concatenates.  d->Ci = C1 + C2; x1 holds the first C1 (multiple of 32) channels.
 * The data gradient writes [dx1 | dx2] (C1 a multiple of 64); the weight gradient accumulates like hoig_conv2d_bwd_weight. */
int hoig_conv2d_cat_fwd_packed(const hoig_conv_desc *d, const float *x1, int C1, const float *x2, const uint16_t *w_hi,
                               const uint16_t *w_lo, const float *bias /*nullable*/, float *y, hoig_stream_t stream);
int hoig_conv2d_cat_bwd_data_packed(const hoig_conv_desc *d, const float *dy, const uint16_t *wt_hi, const uint16_t *wt_lo,
                                    float *dx1, int C1, float *dx2, hoig_stream_t stream);
int hoig_conv2d_cat_bwd_weight(const hoig_conv_desc *d, const float *x1, int C1, const float *x2, const float *dy, float *dw,
                               float *dbias /*nullable*/, hoig_stream_t stream);

/* ---- instance norm (generator.py:16-22,101-120,154-208; spade.py:13; discriminator.py:37,45 via
 *      base_network.py:31): per-(b,c) mean / biased variance over H*W, eps 1e-5, no running stats. ---- */
/* stats: mean[b*C+c], rstd[b*C+c].  workspace: >= hoig_inorm_workspace_bytes(B,HW,C) bytes whose first 2^18 floats (the pool
 * of atomic accumulators, B*2*C of them used) must be ZERO on entry; hoig_inorm_stats / hoig_inorm_bwd* leave them zero again on return, so one
 * zero-initialised workspace per stream serves every call without memset launches. */
int64_t hoig_inorm_workspace_bytes(int B, int HW, int C);
int hoig_inorm_stats(const float *x, int B, int HW, int C, float eps, float *mean, float *rstd, void *workspace,
                     hoig_stream_t stream);
/* y = act( (x-mean)*rstd * scale + shift ) + residual
 *   mode 0: scale=1, shift=0 (param-free)           mode 1: scale=weight[c], shift=bias[c] (affine)
 *   mode 2: scale=1+gamma[b,hw,c], shift=beta[b,hw,c] (SPADE, spade.py:36) */
int hoig_inorm_apply(const float *x, const float *mean, const float *rstd, int mode, const float *p0, const float *p1,
                     int act, float slope, const float *residual /*nullable*/, float *y, int B, int HW, int C,
                     hoig_stream_t stream);
/* same with gamma/beta rows `ld_p` floats apart (mode 2 only): lets gamma and beta live side by side in ONE [.,2C] tensor
 * (the output of the fused gamma|beta convolution), p0 = gb, p1 = gb + C, ld_p = 2C */
/* mean / rstd of y from the sums that the convolution which wrote y left in the workspace's accumulators (hoig_conv2d_fwd_packed_stats
 * and its kin: PLAIN sums in fp64).  var = E[y^2] - E[y]^2, taken in fp64, is kept only for the channels where it is well conditioned
 * (E[y^2] <= 8 var, |mean|/sigma below ~2.6); every other (image, channel) -- a near-constant channel, a stem channel over a flat
 * image -- is recomputed in the same launch from y, centred on the mean the sums gave, so the result holds the bound of the two-pass
 * kernels for any input (tests/test_norm_gpu.py; figures in docs/norm_conditioning.md).  C % 4 == 0 and B * 4 * C <= 2^18,
 * HOIG_EUNSUPPORTED otherwise; leaves the accumulators zero like hoig_inorm_stats, whose shifted sums take their pivot from a median
 * of means of twelve pixels spread over the map. */
int hoig_inorm_stats_from_sums(const float *y, int B, int HW, int C, float eps, float *mean, float *rstd, void *workspace,
                               hoig_stream_t stream);
int hoig_inorm_apply_ld(const float *x, const float *mean, const float *rstd, int mode, const float *p0, const float *p1,
                        int ld_p, int act, float slope, const float *residual /*nullable*/, float *y, int B, int HW, int C,
                        hoig_stream_t stream);
int hoig_inorm_bwd_ld(const float *x, const float *mean, const float *rstd, int mode, const float *p0, const float *p1,
                      int ld_p, const float *y, const float *dy, int act, float slope, float *dx, float *dp0, float *dp1, int B,
                      int HW, int C, void *workspace, hoig_stream_t stream);
/* Single-launch instance norm for maps of at most 1024 pixels with C % 32 == 0 (the 32x32 bottleneck and below): a workgroup
 * keeps a (sample, 32-channel) slab in registers -- statistics (two-pass), normalise / modulate / activate (+ residual) from
 * one read of x; the backward likewise from one read of x and dy.  Same argument meaning as hoig_inorm_stats +
 * hoig_inorm_apply_ld / hoig_inorm_bwd_ld; mode-1 parameter gradients accumulate atomically, no workspace.
 * HOIG_EUNSUPPORTED for other shapes: the caller then uses the streaming kernels above. */
int hoig_inorm_fwd_fused(const float *x, int mode, const float *p0, const float *p1, int ld_p, int act, float slope,
                         const float *residual /*nullable*/, float eps, float *y, float *mean, float *rstd, int B, int HW,
                         int C, hoig_stream_t stream);
int hoig_inorm_bwd_fused(const float *x, const float *mean, const float *rstd, int mode, const float *p0, const float *p1,
                         int ld_p, const float *y /*nullable, see hoig_inorm_bwd_ld*/, const float *dy, int act, float slope,
                         float *dx, float *dp0, float *dp1, int B, int HW, int C, hoig_stream_t stream);
/* ... + addend (nullable; same shape as x): dx = norm backward + addend.  The SPADE residual block reads its input twice -- the
 * first norm and the skip `x + dx` (generator.py:63-71) -- and the skip's gradient is added here instead of by a pass of its own. */
int hoig_inorm_bwd_add_ld(const float *x, const float *mean, const float *rstd, int mode, const float *p0, const float *p1,
                          int ld_p, const float *y, const float *dy, int act, float slope, const float *addend, float *dx,
                          float *dp0, float *dp1, int B, int HW, int C, void *workspace, hoig_stream_t stream);
int hoig_inorm_bwd_fused_add(const float *x, const float *mean, const float *rstd, int mode, const float *p0, const float *p1,
                             int ld_p, const float *y, const float *dy, int act, float slope, const float *addend, float *dx,
                             float *dp0, float *dp1, int B, int HW, int C, hoig_stream_t stream);

/* backward of hoig_inorm_apply(+stats).  dy is d/d(y) ; y is the forward output (for the activation mask; pass
 * the pre-residual activation output, or NULL when act==NONE).  For ReLU / LeakyReLU after a plain (mode 0) or affine
 * (mode 1, p1 = its bias) norm, y may also be NULL: the mask is recomputed from x, one tensor less to read per pass.
 * p1 is only read in that case (nullable otherwise).
 * Outputs: dx; mode 1: dweight[c] += , dbias[c] += ; mode 2: dgamma, dbeta (same shape as x, overwritten).
 * workspace >= hoig_inorm_workspace_bytes. */
int hoig_inorm_bwd(const float *x, const float *mean, const float *rstd, int mode, const float *p0, const float *p1,
                   const float *y, const float *dy, int act, float slope, float *dx, float *dp0, float *dp1, int B, int HW,
                   int C, void *workspace, hoig_stream_t stream);

/* ---- local attention warping: ExtractorAttn (extract_attn.py:23-29) = K1 block extraction of source (with flow)
 *      and target (zero flow) + conv k5/s5 + LeakyReLU(0.01) + conv1x1 + softmax(25) + K3 reshape + weighted 5x5 average.
 *      Composition (host: hoig_amd/ops.py::_LocalAttn), no 25x-sized tensor anywhere: the taps of a pixel share their
 *      bilinear fractions and each corner is border-clamped on its own, so the sampling commutes with the linear map over
 *      the taps -- the target half of the k5/s5 conv is a 5x5 valid convolution Gt of replicate_pad(target, 2), the source
 *      half a BILINEAR READ (at pixel + flow) of the 5x5 valid convolution Gs of replicate_pad(source, 4), both on
 *      hoig_conv2d_*; the weighted average reads the source's 6x6 footprint.  These entry points are the pieces around the
 *      two convolutions.  flow: [B,2,H,W] (ch0 = x, ch1 = y, PIXEL units as K1 reads them,
 *      block_extractor_kernel.cu:62-67); it carries no gradient on the path (it is data: generator.py:481-488). ---- */
/* y[b, py, px] = x[b, clamp(py-pad), clamp(px-pad)]  ([B,H,W,C] -> [B,H+2pad,W+2pad,C]) and its adjoint */
int hoig_replicate_pad_fwd(const float *x, float *y, int B, int H, int W, int C, int pad, hoig_stream_t stream);
int hoig_replicate_pad_bwd(const float *dy, float *dx, int B, int H, int W, int C, int pad, hoig_stream_t stream);
/* ... + addend (nullable, [B,H,W,C]): the gradient that reached x through another consumer (tx = tx + attention(.., target = tx),
 * generator.py:391-392,413-414), added here instead of by a pass of its own */
int hoig_replicate_pad_bwd_add(const float *dy, const float *addend, float *dx, int B, int H, int W, int C, int pad,
                               hoig_stream_t stream);
/* hidden[m] = gt[m] + bilinear(gs; m + flow(m))            gt: [B,H,W,128] (bias included), gs: [B,H+4,W+4,128] = Gs on the
 *                                                          grid [-2,H+1] x [-2,W+1], hidden: [M,128] pre-activation (out)
 * attn[m]   = softmax_25(w2 . leaky_0.01(hidden[m]) + b2)  w2: [25][128]
 * out[m][c] = (1/25) sum_q attn[m][q] * S[m][q][c]         S = K1's border-clamped bilinear samples of `source` [B,H,W,C],
 *                                                          evaluated over the pixel's 6x6 footprint, never stored */
int hoig_attn_pixel_fwd(const float *gt, const float *gs, const float *flow, const float *w2, const float *b2,
                        const float *source, float *hidden, float *attn, float *out, float *kf /*nullable*/, int B, int H,
                        int W, int C, hoig_stream_t stream);
/* kf (training only): [M][36] weights of the pixel's 6x6 source footprint in `out`, k[i][j] = (1/25) sum_ab w_ab attn[i-a][j-b],
 * kept for hoig_attn_src_gather */
/* given dout: dhidden (overwritten; it is also dGt), dw2 / db2 (accumulated); e_ws: M*36 floats of scratch (the dot products
 * of dout[m] with the 36 source cells of pixel m's footprint) */
int hoig_attn_pixel_bwd(const float *hidden, const float *attn, const float *w2, const float *source, const float *flow,
                        const float *dout, float *dhidden, float *dw2, float *db2, float *e_ws, int B, int H, int W, int C,
                        hoig_stream_t stream);
/* The two source-side gradients are transposes of gathers through the pixels' sampling frames P(m) = floor(m + flow(m)).
 * Instead of scattering with atomics (K2, block_extractor_kernel.cu:158-161) the pixels are bucketed by their frame cell
 * (counting sort: `index`, hoig_attn_index_ints(B,H,W) ints of caller memory; depends on the flow only, so one index serves
 * every attention layer of a resolution) and each output cell gathers from the buckets whose footprints reach it. */
int64_t hoig_attn_index_ints(int B, int H, int W);
int hoig_attn_build_index(const float *flow, int32_t *index, int B, int H, int W, hoig_stream_t stream);
/* dsource[cell] = init[cell] + sum_m kf[m][cell's position in m's 6x6 footprint] * dout[m]   (the weighted average's source
 * gradient; every element written; init (nullable = zeros): the gradient the source receives from its other consumers) */
int hoig_attn_src_gather(const int32_t *index, const float *kf, const float *dout, const float *init, float *dsource, int B,
                         int H, int W, int C, hoig_stream_t stream);
/* dgs = bilinear^T(dhidden)  (dgs: [B,H+4,W+4,128], every element written) */
int hoig_attn_gs_gather(const int32_t *index, const float *flow, const float *dhidden, float *dgs, int B, int H, int W,
                        hoig_stream_t stream);

/* Stand-alone drop-ins for the reference's two pybind ops, same argument meaning, contiguous NCHW fp32,
 * caller zero-fills outputs: block_extractor_cuda.forward/backward (block_extractor_cuda.cc:5-33) and
 * local_attn_reshape_cuda.forward/backward (local_attn_reshape_cuda.cc:5-29). */
int hoig_block_extractor_forward(const float *source, const float *flow, float *output, int B, int C, int Hs, int Ws,
                                 int Hf, int Wf, int kernel_size, hoig_stream_t stream);
int hoig_block_extractor_backward(const float *source, const float *flow, const float *grad_output, float *grad_source,
                                  float *grad_flow, int B, int C, int Hs, int Ws, int Hf, int Wf, int kernel_size,
                                  hoig_stream_t stream);
int hoig_local_attn_reshape_forward(const float *inputs, float *output, int B, int Hs, int Ws, int kernel_size,
                                    hoig_stream_t stream);
int hoig_local_attn_reshape_backward(const float *grad_output, float *grad_inputs, int B, int Hs, int Ws,
                                     int kernel_size, hoig_stream_t stream);

/* ---- sampling (generator.py:466-478; spade.py:30) ---- */
/* F.grid_sample(x, grid) bilinear / zeros / align_corners=False. x:[B,H,W,C] NHWC, grid:[B,Ho,Wo,2], y:[B,Ho,Wo,C] */
int hoig_grid_sample_fwd(const float *x, const float *grid, float *y, int B, int H, int W, int C, int Ho, int Wo,
                         hoig_stream_t stream);
/* dx accumulates (caller zero-fills) */
int hoig_grid_sample_bwd(const float *grid, const float *dy, float *dx, int B, int H, int W, int C, int Ho, int Wo,
                         hoig_stream_t stream);
/* F.interpolate(bilinear, align_corners=True) on NHWC [B,Hi,Wi,C] -> [B,Ho,Wo,C] */
int hoig_resize_bilinear_ac(const float *x, float *y, int B, int Hi, int Wi, int C, int Ho, int Wo,
                            hoig_stream_t stream);
/* F.interpolate(nearest) NHWC */
int hoig_resize_nearest(const float *x, float *y, int B, int Hi, int Wi, int C, int Ho, int Wo, hoig_stream_t stream);
/* attention flow of generator.py:484-488: flow[b,ch,y,x] = Tscale[b,y,x,ch] - idt ; idt ch0 = -1+2*y/h (the ROW
 * coordinate, 'ij' meshgrid quirk), ch1 = -1+2*x/h.  tscale:[B,h,h,2] -> flow:[B,2,h,h] */
int hoig_attn_flow(const float *tscale, float *flow, int B, int h, hoig_stream_t stream);

/* ---- pooling for the VGG19 feature path (vgg19.py:56; MaxPool2d(2,2)) NHWC ---- */
int hoig_maxpool2_fwd(const float *x, float *y, int B, int H, int W, int C, hoig_stream_t stream);
int hoig_maxpool2_bwd(const float *x, const float *y, const float *dy, float *dx, int B, int H, int W, int C,
                      hoig_stream_t stream);

/* ---- pointwise / layout ---- */
int hoig_nchw_to_nhwc(const float *x, float *y, int B, int C, int H, int W, hoig_stream_t stream);
int hoig_nhwc_to_nchw(const float *x, float *y, int B, int C, int H, int W, hoig_stream_t stream);
/* y[:, c_off : c_off+Cx] = x  for NHWC tensors with Cy channels (channel concat building block) */
int hoig_copy_channels(const float *x, float *y, int64_t npix, int Cx, int x_off, int Cy, int y_off, int Ccopy,
                       int accumulate, hoig_stream_t stream);
/* torch.cat([x1, x2], channel axis) of two contiguous [npix][C] tensors in one pass over y (coalesced for any C1 + C2) */
int hoig_cat2_channels(const float *x1, int C1, const float *x2, int C2, float *y, int64_t npix, hoig_stream_t stream);
/* y = a + b (n elements) ; y = act_bwd: dx = dy * act'(y) */
int hoig_add(const float *a, const float *b, float *y, int64_t n, hoig_stream_t stream);
/* y = act(a + b): the activation of a convolution that was split over two input tensors (conv(cat[x1, x2]) = conv(x1) + conv(x2)) */
int hoig_add_act(const float *a, const float *b, float *y, int act, float slope, int64_t n, hoig_stream_t stream);
int hoig_act_bwd(const float *y, const float *dy, float *dx, int act, float slope, int64_t n, hoig_stream_t stream);
/* the same, fused with the bias gradient of the convolution that produced y [rows][C]: g = dy * act'(y), dbias[c] += sum_rows g */
int hoig_act_bwd_colsum(const float *y, const float *dy, float *g, float *dbias, int act, float slope, int64_t rows, int C,
                        hoig_stream_t stream);
/* column sums: out[c] += sum_rows x[row][c]  (bias gradients) */
int hoig_colsum_accum(const float *x, float *out, int64_t rows, int C, hoig_stream_t stream);

/* alpha compositing of trainer.py:400-401 : img = mbg*bg + (1-mbg)*(obj*mh + hand*(1-mh)); NHWC, masks 1 channel */
int hoig_compose_fwd(const float *bg, const float *obj, const float *hand, const float *mbg, const float *mh, float *img,
                     int64_t npix, int C, hoig_stream_t stream);
int hoig_compose_bwd(const float *bg, const float *obj, const float *hand, const float *mbg, const float *mh,
                     const float *dimg, float *dbg, float *dobj, float *dhand, float *dmbg, float *dmh, int64_t npix,
                     int C, hoig_stream_t stream);

/* ---- losses (trainer.py:436-481): each writes sum-reductions into out[] (caller-zeroed, fp32 atomics of
 *      per-block partials) and, when dpred != NULL, the gradient of (scale * mean-loss) w.r.t. pred. ---- */
enum { HOIG_LOSS_L1 = 0, HOIG_LOSS_MSE = 1, HOIG_LOSS_BCE = 2 };
/* out[0] += sum loss(pred, target) ; dpred = gscale * dloss/dpred (gscale already includes 1/n and lambda).
 * target_const used when target == NULL (LSGAN targets 0/+1/-1, trainer.py:439,467-468). */
int hoig_loss_fwd_bwd(int kind, const float *pred, const float *target, float target_const, float gscale, float *out,
                      float *dpred, int64_t n, hoig_stream_t stream);
/* TV-L1 smoothness trainer.py:479-481 on [B,H,W] single-channel maps: out[0] += sum|dx|, out[1] += sum|dy| ;
 * dm (overwritten) = gx * d(sum|dx|) + gy * d(sum|dy|) */
int hoig_tv_fwd_bwd(const float *m, float gx, float gy, float *out, float *dm, int B, int H, int W, hoig_stream_t stream);
/* The same two as TERMS OF AN OBJECTIVE (trainer.py:448-457: loss_G = g_adv + g_rec + g_tsf + g_mask + g_mask_smooth): *term +=
 * gscale * sum loss(pred, target)  resp.  gx * sum|dx| + gy * sum|dy|  -- the scaled value goes straight into a caller-owned
 * fp32 slot (several calls may share one: the five VGG levels of g_tsf), so that the host composes the objective without
 * per-term scalar launches. */
int hoig_loss_accumulate(int kind, const float *pred, const float *target, float target_const, float gscale, float *term,
                         float *dpred, int64_t n, hoig_stream_t stream);
int hoig_tv_accumulate(const float *m, float gx, float gy, float *term, float *dm, int B, int H, int W, hoig_stream_t stream);
/* out[0] += sum x */
int hoig_sum(const float *x, float *out, int64_t n, hoig_stream_t stream);
/* out[0] += scale * sum x   (a mean written straight into a report slot: d_real / d_fake, trainer.py:470-471) */
int hoig_sum_scaled(const float *x, float scale, float *out, int64_t n, hoig_stream_t stream);

/* ---- fused Adam over one flat parameter buffer (torch.optim.Adam defaults of trainer.py:275-278:
 *      no weight decay, no amsgrad): step is the 1-based step count after increment ----
 * hoig_adam_step, hoig_adam_step_dev and hoig_adam_step_dev_guarded take a slice that may start at ANY element: when one of the four
 * pointers is not 16-byte aligned the kernel takes its scalar loop for all n (the same arithmetic, element for element; slower), so
 * a slice cut off a multiple of 4 elements is as valid as an aligned one. */
int hoig_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, double lr,
                   double beta1, double beta2, double eps, int step, float grad_scale, hoig_stream_t stream);

/* The same update with the schedule in DEVICE memory (an optimiser step that can be captured in a hipGraph):
 * `state` = {lr, beta1, beta2, eps, step} as doubles (the host only ever rewrites lr: Trainer.update_learning_rate,
 * trainer.py:574-591); hoig_adam_tick advances state[4] by one and writes the six fp32 scalars of this step into `derived`
 * (bias corrections evaluated in double, as hoig_adam_step does on the host); hoig_adam_step_dev applies them to a slice. */
int hoig_adam_tick(double *state, float *derived, hoig_stream_t stream);
int hoig_adam_step_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, const float *derived,
                       float grad_scale, hoig_stream_t stream);
/* hoig_adam_step_dev over a WHOLE flat buffer and hoig_pack_conv_weights_bf16_all of the updated weights in one launch: the
 * weights of the table (`segs`, `nseg`, `ntiles`: as for hoig_pack_conv_weights_bf16_all; every table weight has Co % 32 == Ci % 32
 * == 0 and the rows must not overlap) are updated tile by tile and their planes written from the registers that hold the new values;
 * `plain` (device memory) holds nplain rows of 2 int64 {first element, count <= 1024, both multiples of 4}: the rest of the buffer,
 * updated without planes.  Every element of the buffer must be covered exactly once by the table or by `plain`.  Same arithmetic as
 * hoig_adam_step_dev, element for element. */
int hoig_adam_pack_step(float *flat, const float *grad, float *exp_avg, float *exp_avg_sq, const float *derived, float grad_scale,
                        const int64_t *segs, int nseg, int64_t ntiles, const int64_t *plain, int64_t nplain, uint16_t *hi_f,
                        uint16_t *lo_f, uint16_t *hi_d, uint16_t *lo_d, hoig_stream_t stream);

/* A non-blocking HIP stream owned by the library (the step's side streams: see hoig_amd/ops.py new_stream for why they are not
 * taken from PyTorch's round-robin stream pool). */
int hoig_stream_create(hoig_stream_t *out);
int hoig_stream_destroy(hoig_stream_t stream);   /* also forgets the stream's scratch block */
/* Per-stream scratch, CALLER-owned like every other buffer of this interface (nothing behind it allocates device memory): kernels
 * that reduce per-workgroup partial sums through memory -- the thin-channel weight gradients behind hoig_conv2d_bwd_weight -- use the
 * block registered for the stream they are launched on (launches of one stream are ordered, so they share it).  Register >=
 * hoig_stream_scratch_bytes() bytes per stream that launches weight gradients; ptr = NULL forgets the stream.  Without a block those
 * kernels take a (slower, same-result-up-to-summation-order) atomic path and report it once on stderr.  The block must stay valid
 * until the stream's last launch that may use it has run. */
int64_t hoig_stream_scratch_bytes(void);
/* what hoig_conv2d_bwd_weight would use of it for layer d: hoig_stream_scratch_bytes() for the thin-channel layers, 0 for all others
 * (a caller may register scratch only on the streams that launch such layers) */
int64_t hoig_conv2d_bwd_weight_scratch_bytes(const hoig_conv_desc *d);
int hoig_stream_scratch_set(hoig_stream_t stream, void *ptr, int64_t bytes);

/* eval.py output stage (utils/util.py:249-264): uint8 = (x+1)/2*255 truncated, NHWC fp32 -> CHW uint8 grid tile */
int hoig_tensor2im_u8(const float *x, uint8_t *out, int B, int H, int W, int C, int nrow, int unnormalize,
                      hoig_stream_t stream);
/* the same bytes without the grid: x [n] fp32 -> out [n] uint8 in x's own (NHWC, per-sample) layout, so that eval.py's three images
 * can stay on the device (Trainer.eval_images_u8) */
int hoig_tensor2im_nhwc_u8(const float *x, uint8_t *out, int64_t n, int unnormalize, hoig_stream_t stream);

/* ---- input preparation AFTER the rasteriser (tensor stage): HandRecoveryFlow.forward
 *      (models/trainer.py:46-145) + the MANORenderer helpers it calls (utils/nmr.py:567-595, 874-968, 973-1100) +
 *      util.morph (utils/util.py:142-158).  Planar NCHW fp32 (the reference's layout at this boundary), int32 face index
 *      maps (-1 = no face; ids < 1538 are hand faces), 256 x 256 images and a 256 x 640 texture atlas as in the reference.
 *      Replaces, per sample: get_texture_backward_warp -> hoig_prep_texture; encode_fim / encode_sem /
 *      sample_from_texture_dense + F.grid_sample(align_corners=True) / cal_bc_transform -> hoig_prep_lookup (once per view);
 *      and, per batch, trainer.py:73,79,82,110-141 -> hoig_prep_assemble. ---- */
/* src_img [3,256,256]; src_faces [F,3,3] (x, y, z of the projected face vertices as render_fim_wim returns them: y is
 * negated here, trainer.py:67-68); fim_uv [256,640], wim_uv [256,640,3], obj_tex_img [256,256,3] (HWC): the object's
 * buffers; occ_ws: 256*640 bytes of workspace; tex [3,256,640] out */
int hoig_prep_texture(const float *src_img, const float *src_faces, const int32_t *src_fim, const int32_t *fim_uv,
                      const float *wim_uv, const float *obj_tex_img, unsigned char *occ_ws, float *tex,
                      hoig_stream_t stream);
/* one view of one sample: fim [256,256], wim [256,256,3]; map_fn [(F+1),3], sem_full [F+1], faces_uv_coord [F,3,2] with
 * F = n_faces (row F = background, what index -1 addresses in the reference); tex from hoig_prep_texture.
 * out: cond [3,256,256], seg [256,256] (label), hand_region [256,256] (1 - hand faces, BEFORE the erosion),
 * rend [3,256,256]; T [256,256,2] (nullable; needs src_faces): cal_bc_transform of THIS view's fim / wim */
int hoig_prep_lookup(const int32_t *fim, const float *wim, const float *map_fn, const float *sem_full,
                     const float *faces_uv_coord, int n_faces, const float *tex, const float *src_faces, float *cond,
                     float *seg, float *hand_region, float *rend, float *T, hoig_stream_t stream);
/* The same two stages for a whole BATCH in one call each (round 6: two + one launches instead of B x (two + one); the chain of small
 * launches is what the raw-batch stage costs a loader-fed step).  Tensors are the per-sample ones stacked over B; src_faces is
 * [B][.][3][3] with face_stride floats between samples; the per-sample object buffers -- every sample may hold another object -- are
 * passed as HOST arrays of B device pointers (n_faces: host array of B ints) and travel to the kernels by value, so B <=
 * HOIG_PREP_MAX_BATCH (HOIG_EUNSUPPORTED beyond: the caller then loops over the per-sample entry points).  occ_ws: B * 256 * 640 bytes;
 * tex [B,3,256,640]. */
#define HOIG_PREP_MAX_BATCH 32
int hoig_prep_texture_batched(int B, const float *src_img, const float *src_faces, int64_t face_stride, const int32_t *src_fim,
                              const int32_t *const *fim_uv, const float *const *wim_uv, const float *const *obj_tex_img,
                              unsigned char *occ_ws, float *tex, hoig_stream_t stream);
int hoig_prep_lookup_batched(int B, const int32_t *fim, const float *wim, const float *const *map_fn, const float *const *sem_full,
                             const float *const *faces_uv_coord, const int *n_faces, const float *tex, const float *src_faces,
                             int64_t face_stride, float *cond, float *seg, float *hand_region, float *rend, float *T /*nullable*/,
                             hoig_stream_t stream);
/* batch: images [B,3,256,256]; the hoig_prep_lookup outputs of both views stacked over the batch; T_raw [B,256,256,2].
 * out: src_bg [B,4,..], tsf_bg (nullable: bg_both) [B,4,..], src_obj / tsf_obj [B,15,..], src_hand / ref_hand
 * [B,hand_channels,..] with hand_channels = 6 (HOv3) or 12 (DexYCB: + the six hand-part one-hots, HOIG_DexYCB/models/trainer.py:131,135),
 * T_hand [B,256,256,2], the four crop masks [B,1,..] (bg src, bg ref, hand src, hand ref) */
int hoig_prep_assemble(int B, const float *src_img, const float *ref_img, const float *cond_s, const float *cond_r,
                       const float *seg_s, const float *seg_r, const float *hr_s, const float *hr_r, const float *rend_s,
                       const float *rend_r, const float *T_raw, float *src_bg, float *tsf_bg, float *src_obj,
                       float *tsf_obj, float *src_hand, float *ref_hand, int hand_channels, float *T_hand, float *smb,
                       float *rmb, float *smh, float *rmh, hoig_stream_t stream);

/* ---- rasteriser of MANORenderer.render_fim_wim (utils/nmr.py:496-513): replaces
 *      nr.rasterize_face_index_map_and_weight_map(faces, image_size, anti_aliasing=False), i.e. neural_renderer's
 *      forward_face_index_map kernels 1+2 (thirdparty/neural_renderer/neural_renderer/cuda/rasterize_cuda_kernel.cu:40-186)
 *      with the wrapper's -1 / 0 fill and vertical flip (neural_renderer/rasterize.py:50-52,334-338).
 *      faces [B,F,3,3] (vertices_to_faces output: x, y in [-1,1], y up, z depth); fim [B,S,S] int32 (-1 = no face),
 *      wim [B,S,S,3]; workspace: hoig_rasterize_workspace_bytes(B, F) bytes.  Tile-binned (16x16-pixel tiles). ---- */
size_t hoig_rasterize_workspace_bytes(int B, int F);
/* The vertex stage in front of it for a whole batch in ONE launch: MANORenderer's projection (orthographic_proj_withz_idrot,
 * utils/nmr.py:109-140: cam_dim 15 = 3x3 camera matrix | 2x3 crop transform; HOIG_DexYCB/utils/nmr.py:146-163: cam_dim 10 = fx, fy, cx,
 * cy | crop transform), the y flip (:506), nr.look_at with the renderer's eye (z - eye_z) and nr.vertices_to_faces (:508-511).
 * verts [B][V][3]; face_lists: HOST array of B device pointers to [n_faces[b]][3] int64 vertex indices (a sample's object decides its
 * list; it may be null where n_faces[b] is 0), n_faces: host array; faces_out [B][Fmax][3][3], rows >= n_faces[b] filled with pad_value (a point no pixel can see).
 * B <= HOIG_PREP_MAX_BATCH. */
int hoig_project_faces(const float *cam, int cam_dim, const float *verts, int V, const int64_t *const *face_lists, const int *n_faces,
                       int B, int Fmax, float eye_z, float pad_value, float *faces_out, hoig_stream_t stream);
int hoig_rasterize_fim_wim(const float *faces, int B, int F, int image_size, float near, float far, int32_t *fim,
                           float *wim, void *workspace, hoig_stream_t stream);
/* The CPU twin of the rasteriser's setup stage (hoig_amd/csrc/raster_box.h, raster_host.cpp; docs/raster_parity.md): the packed tile
 * box x0 | x1 << 8 | y0 << 16 | y1 << 24 (16 x 16-pixel tiles) inside which the tile kernel tests each of n_faces faces [n][3][3];
 * 0x00ff00ff: in no tile (a back face, or off screen).  Host memory only. */
int hoig_raster_face_boxes_host(const float *faces, int n_faces, int image_size, uint32_t *boxes_out);

/* ---- data loader, device side: the image work of HOv3Dataset._get_sample (HOIG_HOv3/data/hov3_dataset.py:215-223,
 *      63-91) and of __getitem__'s transform (:208-212,267) for a batch of decoded 8-bit frames.  Both replace calls into
 *      opencv-python 4.5.1.48 (requirements.txt:99) and follow its fixed-point algorithms integer for integer (hoig_amd/csrc/data_prep.hip).
 * hoig_resize_linear_u8: cv2.resize(src, (Wd, Hd)) with the default INTER_LINEAR (:219): uint8 [B][Hs][Ws][C] -> [B][Hd][Wd][C], C <= 4.
 * hoig_warp_affine_u8: cv2.warpAffine(src, M, (Wd, Hd), flags=cv2.INTER_LINEAR) (:78; BORDER_CONSTANT, value 0) with M the FORWARD
 *   2x3 transform of each sample as the reference passes it (float32 values widened to double: M [B][6]); mode 0: dst uint8
 *   [B][Hd][Wd][C]; mode 1 (C == 3): dst float [B][3][Hd][Wd], channel c = ((float(v[2-c]) / 255) - 0.5) / 0.5 -- astype(float32),
 *   / 255.0, [:, :, ::-1], ToTensor, Normalize(0.5, 0.5) (:79,222,209,267); mode 2: dst float [B][1][Hd][Wd] = float(v[C-1]) / 128
 *   (:223). ---- */
int hoig_resize_linear_u8(const uint8_t *src, int B, int Hs, int Ws, int C, uint8_t *dst, int Hd, int Wd, hoig_stream_t stream);
int hoig_warp_affine_u8(const uint8_t *src, int B, int Hs, int Ws, int C, const double *M, int Hd, int Wd, int mode, void *dst,
                        hoig_stream_t stream);

const char *hoig_version(void);

/* Kernel-variant choices that are tuning, not semantics (every value computes the same result up to summation order): one table
 * instead of per-variant environment switches.  key -> value; returns the previous value, or -1 for an unknown key; value < 0 only
 * queries.  Keys and defaults (each adopted on an interleaved A/B committed under profiles/r04_*):
 *   "s2_16"   1  the stride-2 3x3 layers on v_mfma_f32_16x16x32 (conv_halo16.hip; scatter launches with 64-channel tiles stay on 32x32x16)
 *   "igemm16" 1  the generic implicit GEMM on it (conv_igemm16.hip): 1 = forward launches, 2 = data gradients too
 *   "flat5"   2  the flattened-axis halo kernel (conv_flat16.hip): 1 = the attention's valid 5x5 convolutions and their data
 *                gradients, 2 = also the 3x3 "same" layers with too few tiles for the halo kernels
 *   "wflat5"  1  the weight gradient of the attention's valid 5x5 convolutions on the flattened pixel axis (wgrad_flat.hip):
 *                1 = where the output width is not a multiple of 32 (the 2 x 32-pixel halo kernel cannot run), 2 = always
 *   "head16"  1  the forward of the 7x7 image / mask heads (64 -> 3..5 channels) on 16x16x32 with the horizontal taps as MFMA
 *                columns (conv_head16.hip), three-term forward arithmetic only; 0: the exact-fp32 VALU kernel (conv_small.hip)
 *   "d_early" 1  (read by the host side, hoig_amd/models/trainer.py) without a gradient exchange the D step is issued on its stream BEFORE
 *                G's backward instead of after it; 0: after (both orders compute the same step: D's weights change only in D's own
 *                update, which stays last).  With an exchange (world > 1) it always follows G's backward: G's all-reduce hides behind it
 *   "pair"    2  (read by the host side, hoig_amd/models/networks/generator.py) the 3x3 512 -> 512 convolutions of src_model's and
 *                tsf_model's residual blocks as grouped launches (hoig_conv2d_*_pair): 1 = always, 2 = in CAPTURED steps only, 0 = never
 *                (one launch per sub-network, on two streams).  Measured (profiles/r05_pair_ab.txt): the eager step loses 0.6 ms to the
 *                lock-step of the two chains (the norms between the convolutions no longer overlap), the replayed graph gains 0.7 ms
 *   "wdma16"  2  the weight tiles of the 16x16x32 3x3 stride-1 kernel (1) and of the flattened-axis kernel (2) by LDS-DMA (conv_halo16.hip /
 *                conv_flat16.hip WDMA: inline-asm global_load_lds, one step ahead, pieces spread over the MFMA groups): +3..7 % on every
 *                layer of the first, +2..5 % on the attention's 5x5 layers, step 63.85 -> 63.03 -> 62.8 ms (profiles/r05_wdma16_ab.txt);
 *                0: through registers, two steps ahead
 *   "s2_pipe"  1  the stride-2 3x3 kernel on the 16x16 MFMA in its statically walked form (conv_s2_16.hip: loads in flight behind the
 *                MFMAs, weight tiles by LDS-DMA) where it measured faster: 8 x 32 tiles with eight waves wherever that leaves every CU
 *                a workgroup and N % 128 == 0 (12-24 %: 132 -> 100 us on 16 x 64x64 256 -> 512), 4 x 32 tiles for grids of at most one
 *                workgroup per CU (15-30 %); 2 / 3: the 4-row / 8-row form wherever it can run; 0: never.  profiles/r05_s2_dma_ab.txt
 *   "norm_in"  1  (read by the host side, hoig_amd/ops.py conv2d_after_norm) INFERENCE forwards apply the norm + ReLU of a single-reader
 *                conv - IN - ReLU - conv3x3 chain in the second convolution's loader (hoig_conv2d_fwd_packed_normin); 0: every norm is a
 *                pass of its own.  Batch-32 generator forward 2.511 -> 2.494 ms per image (the flagship's SPADE norms modulate per
 *                pixel and stay passes)
 *   "split_grads" 1  (read by the host side, hoig_amd/ops.py) the backward of a norm that follows an eligible 3x3 convolution writes its
 *                dx as bf16 hi | lo planes and that convolution's weight / data gradient read them without splitting ('PRE-SPLIT
 *                gradients' above); 0: fp32 gradients everywhere, split in every consuming workgroup
 *   "wino8"    0  (read by the host side, hoig_amd/ops.py _conv_fwd_raw; round 6) 1: three-term FORWARD launches of 3x3 stride-1 layers that
 *                the direct kernel would run on at most half the chip (<= 128 workgroups) and that ONE round of the Winograd F(2x2,3x3)
 *                kernel covers (<= 256 workgroups: 8 images of 512 -> 512 at 32 x 32) go to hoig_conv2d_fwd_wino.  Alone such a launch
 *                is 37 % faster; in the step they are the src / tsf twins, which already share the chip
 *                (profiles/r06_winograd_ab.txt: the in-step A/B); off
 *   "png_window" 0  the window of the PNG decoder's inflate kernel (hoig_png_decode_u8): 0 a 32 KiB ring in LDS, barriers that order LDS
 *                only; 1 the image's own filtered stream in the workspace with a workgroup-scope fence between a store and a later read
 *                of it.  The same bytes; profiles/png_decode.txt has the A/B
 * Round 6 removed the keys whose losing side had lost two rounds running, and with them that side's code: "wgrad16" (the 3x3 weight
 * gradient on 16x16x32: 5-20 % slower, wgrad_halo16.hip deleted), "mfma16" (the 8-row 3x3 stride-1 tilings on 16x16x32: always; their
 * 32x32x16 instantiations are gone), "wgrad_ko" (knock-out instantiations of the LDS-DMA weight gradient:
 * a diagnostic), "few128" / "wgrad_few" (launch sizing for the 8-image launches: always on), "adam_pack" / "pad_in" (always on),
 * "split_grads" 2 / 3 (a split pass of its own, SPADE's [dgamma | dbeta] as planes: both +0.25 ms per step, profiles/r05_split_*_ab.txt).
 * Process-wide, not synchronised: set before launching. */
int hoig_set_tuning(const char *key, int value);

/* The route record: which convolution launcher ran last on the calling host thread.  Every convolution launcher stores its id (one
 * thread-local integer per pass, hoig_amd/csrc/conv_route.h) immediately before its kernel launch; nothing on the device changes and a
 * stream capture records the same ids.  which: 0 forward, 1 data gradient, 2 weight gradient -> the id (0: none yet; -1: bad `which`).
 * hoig_conv_route_name(id): "wgrad_halo_cm2", "dgrad_halo3_m16_128", ... for 0 <= id < the number of routes, NULL beyond: walk the
 * ids from 0 until NULL for the whole table.  The tests assert with it that a shape ran on the kernel it was chosen for. */
int hoig_conv_last_route(int which);
const char *hoig_conv_route_name(int id);

/* ---- MANO hand layer: pose / shape parameters -> skinned hand vertices, the step in front of the rasteriser.
 *      Replaces, for this path, smplx 0.1.28's MANO layer (HOIG_HOv3/models/networks/hmr.py:55,84-85: `mano_layer_right(global_orient,
 *      hand_pose, betas, transl).vertices`, use_pca=False, flat_hand_mean=True) and manopth's ManoLayer (HOIG_DexYCB/models/networks/
 *      hmr.py:55-60,85-86: 45 PCA coefficients + hand mean, `+ trans`, x 1000 / 1000): linear blend skinning (smplx.lbs.lbs) in ONE
 *      launch, one workgroup per sample.
 * model (device, fp32): v_template [V][3], shapedirs [V][3][10], posedirs [135][V*3] (smplx's buffer layout), lbs_weights [V][16],
 *   parents [16] (int32, parents[0] ignored), j_template [16][3] = J_regressor . v_template and j_shapedirs [16][3][10] =
 *   J_regressor . shapedirs (the joint regression is linear in betas: folded once on the host).
 * pose: root [B][3] axis-angle; hand [B][45] axis-angle (hands_components == NULL) or [B][ncomps] PCA coefficients expanded with
 *   hands_components [ncomps][45]; hands_mean [45] (nullable = flat hand) is added either way.  betas [B][10], transl [B][3] (nullable).
 * out: verts rows 0..V-1 of a [B][ld_v][3] tensor (ld_v >= V: the caller's [hand | object] vertex buffer, hmr.py:89, is written
 *   in place), joints [B][16][3] posed joints + transl (nullable). */
int hoig_mano_lbs(const float *v_template, const float *shapedirs, const float *posedirs, const float *j_template,
                  const float *j_shapedirs, const float *lbs_weights, const int32_t *parents, const float *hands_mean /*nullable*/,
                  const float *hands_components /*nullable*/, int ncomps, int V, const float *root, const float *hand,
                  const float *betas, const float *transl /*nullable*/, float *verts, int ld_v, float *joints /*nullable*/, int B,
                  hoig_stream_t stream);

/* ---- EVALUATION METRICS (forward only; hoig_amd/csrc/metrics.hip, hoig_amd/metrics): FID's InceptionV3 (metrics/pytorch_fid/
 *      inception.py), LPIPS-AlexNet (metrics/lpips.py) and SSIM / MS-SSIM (metrics/ssim.py through pytorch_msssim 0.2.1).  The
 *      networks' convolutions run on hoig_conv2d_fwd (bias + ReLU in its epilogue).  Reductions are deterministic: per-workgroup
 *      partials in the caller's workspace, summed in a fixed order by the last workgroup of an image to arrive (an integer ticket per
 *      image); the workspace must be zero-filled once before its first use and is left zero-filled by every call. ---- */
enum { HOIG_POOL_MAX = 0, HOIG_POOL_AVG = 1 };
/* F.max_pool2d / F.avg_pool2d(k, stride, padding=(pad_h, pad_w), count_include_pad), floor output size, NHWC [B,H,W,C] ->
 * [B,Ho,Wo,C] with Ho = (H + 2 pad_h - k) / stride + 1; pad <= k / 2 */
int hoig_pool2d_fwd(const float *x, float *y, int B, int H, int W, int C, int k, int stride, int pad_h, int pad_w, int mode,
                    int count_include_pad, hoig_stream_t stream);
/* uint8 [B,Hi,Wi,C] (C <= 4) -> fp32 NHWC [B,Ho,Wo,C]: v = u8 / 255 (ToTensor), bilinear resize with align_corners=False when
 * (Ho,Wo) != (Hi,Wi) (F.interpolate), then n_affine (0..2) per-channel steps v = (v - sub[c]) / div[c] in order.  affine: HOST
 * memory, n_affine x [sub[C] | div[C]] (read at the call: a captured launch keeps the values) */
int hoig_stage_images_u8(const uint8_t *src, float *y, int B, int Hi, int Wi, int C, int Ho, int Wo, int n_affine, const float *affine,
                         hoig_stream_t stream);
/* Pillow's 8-bit Image.resize((Wo, Ho), Image.BILINEAR) of every image of a batch, equal in every byte (what get_eval_loader applies
 * twice before LPIPS and SSIM see an image; hoig_amd/csrc/pil_resize.h states the fixed-point algorithm): uint8 [B,H,W,3] ->
 * [B,Ho,Wo,3], along W first, then along H on the rounded bytes; a pass that keeps its size is skipped.  C != 3 or a size outside
 * 1..4096: HOIG_EINVAL.
 * hoig_pil_bilinear_ksize / _table (HOST, no HIP call): the taps of one axis for in -> out samples, `out` rows of 2 + ksize int32:
 *   [xmin, n, k[0..ksize)], n <= ksize = 2 ceil(max(in / out, 1)) + 1 taps of 22 fractional bits on src[xmin .. xmin + n).
 * hoig_resize_pil_bilinear_u8_host (HOST twin, the same tap code, no HIP call): src, dst in host memory.
 * hoig_resize_pil_bilinear_u8: src, dst, table_w (W -> Wo), table_h (H -> Ho), workspace in device memory; a table may be NULL when
 *   its pass is skipped, the workspace (hoig_resize_pil_bilinear_u8_workspace_bytes: the rows of the first pass's result that the
 *   second reads; 0 unless both passes run) when that is 0.  dst and workspace 4-byte aligned.  One launch per pass. */
int hoig_pil_bilinear_ksize(int in, int out);
int hoig_pil_bilinear_table(int in, int out, int32_t *table);
int64_t hoig_resize_pil_bilinear_u8_workspace_bytes(int B, int H, int W, int C, int Ho, int Wo);
int hoig_resize_pil_bilinear_u8_host(const uint8_t *src, int B, int H, int W, int C, uint8_t *dst, int Ho, int Wo);
int hoig_resize_pil_bilinear_u8(const uint8_t *src, int B, int H, int W, int C, uint8_t *dst, int Ho, int Wo, const int32_t *table_w,
                                const int32_t *table_h, void *workspace, hoig_stream_t stream);
/* zero-padded copy [B,H,W,C] -> [B,H+2pad_h,W+2pad_w,C] (the asymmetric paddings of Inception's 1x7 / 7x1 / 1x3 / 3x1 layers, which
 * then run on hoig_conv2d_fwd with pad 0); C % 4 == 0, HOIG_EUNSUPPORTED otherwise */
int hoig_pad2d(const float *x, float *y, int B, int H, int W, int C, int pad_h, int pad_w, hoig_stream_t stream);
/* y[b][c] = mean over the HW pixels of x[b][.][c] (adaptive_avg_pool2d to 1x1) */
int hoig_global_avgpool(const float *x, float *y, int B, int HW, int C, hoig_stream_t stream);
/* One LPIPS layer (lpips.py:8-9,64-74): per pixel x * rsqrt(sum_c x^2 + 1e-10) for fx and fy, squared difference, dot with the
 * head's C weights w; out[b] += the mean of that over the HW pixels of image b.  fx, fy: [B,HW,C], C % 4 == 0 and C <= 512
 * (HOIG_EUNSUPPORTED otherwise).  workspace: hoig_lpips_workspace_bytes(B, HW) bytes */
int64_t hoig_lpips_workspace_bytes(int B, int HW);
int hoig_lpips_layer(const float *fx, const float *fy, const float *w, float *out, int B, int HW, int C, void *workspace,
                     hoig_stream_t stream);
/* One SSIM level of pytorch_msssim 0.2.1 (_ssim): separable Gaussian window (win odd taps, sigma, normalised to sum 1), valid
 * padding, C1 = (K1 data_range)^2, C2 = (K2 data_range)^2; ssim_out[b][c] / cs_out[b][c] = the means of the ssim and cs maps.
 * x, y: [B,H,W,C], win <= 15 (HOIG_EUNSUPPORTED above).  workspace: hoig_ssim_workspace_bytes(B, H, W, C, win) bytes */
int64_t hoig_ssim_workspace_bytes(int B, int H, int W, int C, int win);
int hoig_ssim(const float *x, const float *y, float *ssim_out, float *cs_out, int B, int H, int W, int C, float data_range, float K1,
              float K2, int win, float sigma, void *workspace, hoig_stream_t stream);

/* ---- JPEG FRAMES DECODED ON THE DEVICE (hoig_amd/csrc/jpeg.hip, jpeg_entropy.h, jpeg_host.cpp; hoig_amd/data/jpeg.py parses the
 *      headers on the host).  Baseline and extended-sequential Huffman, 8-bit, one interleaved scan; 4:4:4, 4:2:2 (2x1), 4:2:0 (2x2)
 *      and single-component files.  The result is what Pillow on libjpeg-turbo gives, byte for byte: jidctint's islow IDCT, fancy
 *      upsampling, libjpeg's fixed-point YCbCr -> RGB -- as interleaved BGR uint8 [H][W][3], cv2.imread's layout
 *      and hoig_warp_affine_u8's input.
 *      Three launches per batch: entropy decode (one wave per image and restart interval; serial inside an interval) -> int16
 *      coefficients; dequantise + IDCT -> padded uint8 component planes; upsample + colour conversion -> BGR. ---- */
enum { HOIG_JPEG_ECODE = 1,     /* no Huffman code matches, a run leaves the block, or a table is not a prefix code */
       HOIG_JPEG_EOVERRUN = 2,  /* the interval's blocks need more bits than it holds (a truncated file) */
       HOIG_JPEG_EMARKER = 4,   /* a restart marker is missing, out of order, or an interval's offsets are not inside the data */
       HOIG_JPEG_ETRAILING = 8  /* whole bytes are left in an interval after its last block */ };
/* One image of a batch.  The caller fills everything above `coef_off`; hoig_jpeg_decode_workspace_bytes fills the two offsets. */
typedef struct hoig_jpeg_plan {
    int64_t data_off;          /* first byte of the scan's entropy-coded data in the packed byte buffer */
    int64_t out_off;           /* first byte of this image's [height][width][3] result in the output buffer */
    int64_t coef_off;          /* workspace: int16 coefficients, [component][block row][block column][64] of the padded planes */
    int64_t plane_off;         /* workspace: uint8 planes, [component][8 x block rows][8 x block columns] */
    int32_t data_len;          /* bytes of entropy-coded data (up to the marker that ends the scan) */
    int32_t width, height;
    int32_t ncomp;             /* 1 or 3 (Y, Cb, Cr; the chroma components are sampled 1 x 1) */
    int32_t hs, vs;            /* sampling factors of the first component: 1x1, 2x1 or 2x2 */
    int32_t restart_interval;  /* MCUs per restart interval (DRI); 0: the scan is one interval */
    int32_t n_intervals;       /* ceil(MCUs / restart_interval), 1 without DRI */
    int32_t interval_first;    /* this image's first entry in the `intervals` array (it owns n_intervals + 1 entries) */
    int32_t reserved[3];
    uint16_t quant[3][64];     /* per component, row-major (NOT zigzag) */
    uint8_t dc_counts[3][16], dc_vals[3][16], ac_counts[3][16], ac_vals[3][256]; /* per component, canonical: 16 counts + values */
} hoig_jpeg_plan;
/* HOST, no HIP call: checks the n plans, writes each one's coef_off / plane_off and returns the workspace size in bytes (< 0: a plan
 * is outside the supported set) */
int64_t hoig_jpeg_decode_workspace_bytes(hoig_jpeg_plan *plans, int n);
/* HOST twin of the entropy kernel (the same code, jpeg_entropy.h; no HIP call): bytes / plans / intervals / coef / status are host
 * memory, coef is the workspace laid out by hoig_jpeg_decode_workspace_bytes (only the coefficient part is written: it comes first).
 * intervals: int32 offsets relative to each image's data_off -- per image n_intervals starts, then data_len; n_entries of them in all.
 * status[i] = 0 or HOIG_JPEG_E* bits of image i.  A bad STREAM is a status, not a return code. */
int hoig_jpeg_entropy_host(const uint8_t *bytes, int64_t nbytes, const hoig_jpeg_plan *plans, int n, const int32_t *intervals,
                           int64_t n_entries, void *coef, int64_t coef_bytes, int32_t *status);
/* The batch on the device.  bytes (nbytes % 16 == 0, 16-byte aligned), plans_dev, intervals, out, status, workspace: device memory;
 * plans_host: the same plans in host memory, read at the call (sizes and offsets are checked there; the launch geometry comes from
 * them).  Images may differ in size.  status[i] as above, written by the device; never synchronises, allocates nothing. */
int hoig_jpeg_decode_bgr_u8(const uint8_t *bytes, int64_t nbytes, const hoig_jpeg_plan *plans_host, const hoig_jpeg_plan *plans_dev,
                            int n, const int32_t *intervals, int64_t n_entries, uint8_t *out, int64_t out_bytes, int32_t *status,
                            void *workspace, int64_t workspace_bytes, hoig_stream_t stream);
/* The last two stages alone: the workspace already holds the coefficients (at each plan's coef_off) */
int hoig_jpeg_reconstruct_bgr_u8(const hoig_jpeg_plan *plans_host, const hoig_jpeg_plan *plans_dev, int n, uint8_t *out,
                                 int64_t out_bytes, void *workspace, int64_t workspace_bytes, hoig_stream_t stream);

/* ---- The same decode with the entropy stage PARALLEL INSIDE a restart interval (hoig_amd/csrc/jpeg_parallel.h: self-synchronising
 *      sub-sequences of `subseq_bytes` raw bytes, one lane each), for files without restart markers.  Five launches per batch: the
 *      coefficients are zeroed, a workgroup per image and interval decodes, the serial kernel above decodes again the intervals that
 *      workgroup found irregular (a corrupt stream: so status[i] is what hoig_jpeg_decode_bgr_u8 writes), then the two reconstruction
 *      kernels.  subseq_bytes: 0 (HOIG_JPEG_SUBSEQ_BYTES), 32, 64, 128 or 256; anything else is HOIG_EINVAL. ---- */
#define HOIG_JPEG_SUBSEQ_BYTES 64
/* HOST: hoig_jpeg_decode_workspace_bytes (the same coef_off / plane_off), plus the parallel decoder's table behind the planes */
int64_t hoig_jpeg_decode_par_workspace_bytes(hoig_jpeg_plan *plans, int n, int subseq_bytes);
/* HOST twin of the parallel entropy kernel: the same code, a workgroup of `lanes` lanes walked round by round (no HIP call).  Arguments
 * as hoig_jpeg_entropy_host; the coefficient part of each image is zeroed first.  rounds (optional) [n]: the largest number of decode
 * rounds among image i's intervals.  states (optional) [n_states][4]: per sub-sequence, image after image and interval after interval,
 * the final (bit offset, block in MCU, zigzag position, completed blocks); zeros for an interval that went to the serial code. */
int hoig_jpeg_entropy_par_host(const uint8_t *bytes, int64_t nbytes, const hoig_jpeg_plan *plans, int n, const int32_t *intervals,
                               int64_t n_entries, int subseq_bytes, int lanes, void *coef, int64_t coef_bytes, int32_t *status,
                               int32_t *rounds, int32_t *states, int64_t n_states);
/* hoig_jpeg_decode_bgr_u8 with the parallel entropy stage; workspace: hoig_jpeg_decode_par_workspace_bytes.  Same promises: status[i]
 * as the serial entry writes it, never synchronises, allocates nothing, the plans are checked on the host. */
int hoig_jpeg_decode_bgr_u8_par(const uint8_t *bytes, int64_t nbytes, const hoig_jpeg_plan *plans_host, const hoig_jpeg_plan *plans_dev,
                                int n, const int32_t *intervals, int64_t n_entries, uint8_t *out, int64_t out_bytes, int32_t *status,
                                void *workspace, int64_t workspace_bytes, int subseq_bytes, hoig_stream_t stream);

/* ---- PNG FILES ENCODED ON THE DEVICE (hoig_amd/csrc/png.hip, png_deflate.h, png_host.cpp; docs/png_encode.md): uint8 [B][H][W][C],
 *      C = 3 or 1, to B ordinary PNG files (8 bit, colour type 2 or 0, no interlace, no ancillary chunk) that decode to the input.
 *      Each row takes the filter with the smallest sum of absolute (signed) values; the filtered stream of H (1 + W C) bytes is cut
 *      into segments of `segment_bytes`, each a deflate block of its own (dynamic Huffman, or stored where that is not larger) closed
 *      by an empty stored block and carried by an IDAT chunk of its own; the Adler-32 follows in a 4-byte IDAT.  The bytes are a
 *      function of the input and segment_bytes alone.  segment_bytes: 0 (HOIG_PNG_SEGMENT_BYTES), 4096, 8192, 16384 or 32768;
 *      anything else is HOIG_EINVAL.  C outside {1, 3}, a size < 1 or a filtered stream of 2^31 bytes or more: HOIG_EUNSUPPORTED. ---- */
#define HOIG_PNG_SEGMENT_BYTES 8192
/* HOST, no HIP call: the bytes to reserve per image in `out` (negative: the code above) and the device workspace of a batch */
int64_t hoig_png_encode_bound(int H, int W, int C, int segment_bytes);
int64_t hoig_png_encode_workspace_bytes(int B, int H, int W, int C, int segment_bytes);
/* src, out, sizes [B], workspace (16-byte aligned) in device memory: image i's file is out[i * out_stride .. + sizes[i]), the rest of
 * its slot is left alone.  out_stride >= hoig_png_encode_bound, workspace_bytes >= hoig_png_encode_workspace_bytes (HOIG_EINVAL
 * otherwise, before any launch).  Three launches on `stream`; never synchronises, allocates nothing. */
int hoig_png_encode_u8(const uint8_t *src, int B, int H, int W, int C, uint8_t *out, int64_t out_stride, int32_t *sizes, void *workspace,
                       int64_t workspace_bytes, int segment_bytes, hoig_stream_t stream);
/* HOST twins (the same per-lane code, a workgroup walked lane by lane and phase by phase; no HIP call, host memory).
 * hoig_png_filter_host: one image [H][W][C] -> its filtered stream, H (1 + W C) bytes.
 * hoig_png_deflate_host: any byte stream -> the zlib stream (header, the segments, Adler-32) in out[0 .. *out_size); out_bytes >=
 *   2 + n + 10 * segments + 4.  dist_c / dist_row: the two fixed match distances tried next to 1 and the hash table's (0: none);
 *   dist_c = -1: no match search, every byte a literal (crafted streams reach the Huffman edge cases with it).
 *   seg_sizes (optional) [segments]: the bytes of each segment's blocks.
 * hoig_png_encode_host: what hoig_png_encode_u8 writes, byte for byte. */
int hoig_png_filter_host(const uint8_t *src, int H, int W, int C, uint8_t *filtered);
int hoig_png_deflate_host(const uint8_t *stream, int64_t n, int segment_bytes, int dist_c, int dist_row, uint8_t *out, int64_t out_bytes,
                          int64_t *out_size, int32_t *seg_sizes);
int hoig_png_encode_host(const uint8_t *src, int B, int H, int W, int C, uint8_t *out, int64_t out_stride, int32_t *sizes,
                         int segment_bytes);

/* ---- PNG FILES DECODED ON THE DEVICE (hoig_amd/csrc/png_decode.hip, png_inflate.h, png_decode_host.cpp; hoig_amd/png_decode.py walks
 *      the chunks on the host; docs/png_decode.md).  Non-interlaced files of colour type 0, 2, 3, 4, 6 at 8 bits and of type 0 and 3 at
 *      1, 2 and 4 bits, without tRNS.  The result is np.asarray(Image.open(f).convert('RGB')), byte for byte: uint8 [H][W][3] (grey
 *      scaled to 0..255, palette entries looked up, alpha dropped), or the same in B, G, R order.
 *      Two launches per batch: inflate (one 64-lane workgroup per image: stored, fixed and dynamic blocks, tables and a 32 KiB window
 *      in LDS, the Adler-32 compared at the end) -> the filtered stream in the workspace; unfilter + convert (a workgroup per image,
 *      rows as a skewed pipeline) -> RGB / BGR. ---- */
enum { HOIG_PNG_ECODE = 1,      /* no code matches, a code is over-subscribed or incomplete, or the block header's counts are invalid */
       HOIG_PNG_EBTYPE = 2,     /* block type 3 */
       HOIG_PNG_ESTORED = 4,    /* a stored block's LEN and NLEN disagree */
       HOIG_PNG_EDIST = 8,      /* a match reaches in front of the stream */
       HOIG_PNG_EEARLY = 16,    /* the data ends inside a block, or before the Adler-32 */
       HOIG_PNG_EMORE = 32,     /* more output than height * (1 + row bytes) */
       HOIG_PNG_ELESS = 64,     /* less output than that */
       HOIG_PNG_EFILTER = 128,  /* a row's filter type is above 4 */
       HOIG_PNG_EADLER = 256    /* the Adler-32 of the filtered stream is not the stored one */ };
/* One image of a batch.  The caller fills everything above `filt_off`; hoig_png_decode_workspace_bytes fills that. */
typedef struct hoig_png_decode_plan {
    int64_t data_off;          /* first byte of the zlib stream (the IDAT payloads, concatenated) in the packed buffer; % 16 == 0 */
    int64_t out_off;           /* first byte of this image's [height][width][3] result in the output buffer */
    int64_t pal_off;           /* first byte of the PLTE payload in the packed buffer (colour type 3; otherwise unused) */
    int64_t filt_off;          /* workspace: the filtered stream, height * (1 + row bytes) */
    int32_t data_len;          /* bytes of the zlib stream, header and Adler-32 included */
    int32_t width, height;
    int32_t color_type;        /* 0, 2, 3, 4, 6 */
    int32_t bit_depth;         /* 8; 1, 2, 4 as well for colour types 0 and 3 */
    int32_t pal_entries;       /* PLTE entries (colour type 3: 1 .. 256; an index at or above it is black, as in Pillow) */
    int32_t reserved[2];
} hoig_png_decode_plan;
/* HOST, no HIP call: checks the n plans, writes each one's filt_off and returns the workspace size in bytes (< 0: a plan is outside
 * the supported set, or its filtered stream has 2^31 bytes or more) */
int64_t hoig_png_decode_workspace_bytes(hoig_png_decode_plan *plans, int n);
/* HOST twin of the inflate kernel alone (the same per-lane code, the workgroup walked lane by lane; no HIP call): the zlib stream
 * data[0 .. data_len) -> out[0 .. expect) and *status (0 or HOIG_PNG_E* bits; `expect` is the size the stream must have).  data must
 * be readable up to data_len rounded up to 16.  A bad STREAM is a status, not a return code. */
int hoig_png_inflate_host(const uint8_t *data, int64_t data_len, uint8_t *out, int64_t expect, int32_t *status);
/* HOST twin of the whole call: what hoig_png_decode_u8 writes to out and status, byte for byte; all pointers host memory. */
int hoig_png_decode_host(const uint8_t *bytes, int64_t nbytes, const hoig_png_decode_plan *plans, int n, uint8_t *out,
                         int64_t out_bytes, int32_t *status, void *workspace, int64_t workspace_bytes, int bgr);
/* The batch on the device.  bytes (nbytes % 16 == 0, 16-byte aligned), plans_dev, out, status, workspace (16-byte aligned): device
 * memory; plans_host: the same plans in host memory, read at the call (sizes and offsets are checked there: HOIG_EINVAL before any
 * launch).  Images may differ in size and kind.  status[i] is written by the device; an image with a status leaves its slot of `out`
 * unspecified, and nothing outside the slots and the workspace is written.  Never synchronises, allocates nothing. */
int hoig_png_decode_u8(const uint8_t *bytes, int64_t nbytes, const hoig_png_decode_plan *plans_host,
                       const hoig_png_decode_plan *plans_dev, int n, uint8_t *out, int64_t out_bytes, int32_t *status, void *workspace,
                       int64_t workspace_bytes, int bgr, hoig_stream_t stream);

/* ---- STREAMING FID STATISTICS AND THE FRECHET DISTANCE IN FP64 (hoig_amd/csrc/fid_stats.hip, fid_stats.h, fid_stats_host.cpp;
 *      hoig_amd/metrics/fid_device.py; docs/fid_device.md).  Matrices are row-major with explicit leading dimensions (in elements).
 *      The *_host twins take host memory and make no HIP call; they walk every sum in the device's order. ---- */
enum { HOIG_GEMM_ACCUMULATE = 1,  /* C += A^T B instead of C = A^T B */
       HOIG_GEMM_SYMMETRIC = 2,   /* A == B (same pointer, M == N): only the tiles on and above the diagonal are computed, each element
                                     is stored at its mirror place too (with ACCUMULATE, C is taken to be symmetric) */
       HOIG_GEMM_F32 = 4          /* A and B hold fp32; element [k][c] enters as (double)x - pivot[c] (pivot: max(M, N) doubles, or
                                     NULL for none) */ };
/* C [M][N] (+)= A^T B for A [K][M] and B [K][N] on v_mfma_f64_16x16x4_f64; any M, N >= 1 and K >= 0.  One owner per element of C and
 * a fixed order over K: no atomics, the result does not depend on scheduling.  Non-finite operands propagate by the IEEE rules.
 * HOIG_EINVAL: a NULL pointer (A and B may be NULL when K is 0), a leading dimension below its row length, unknown flags, a pivot without HOIG_GEMM_F32. */
int hoig_gemm_tn_f64(const void *A, int64_t lda, const void *B, int64_t ldb, const double *pivot, double *C, int64_t ldc, int M, int N,
                     int K, int flags, hoig_stream_t stream);
int hoig_gemm_tn_f64_host(const void *A, int64_t lda, const void *B, int64_t ldb, const double *pivot, double *C, int64_t ldc, int M,
                          int N, int K, int flags);
/* Rank-revealing pivoted Cholesky of the symmetric positive semi-definite S [D][D]: S = L L^T with L [D][rank] (row i of L belongs to
 * row i of S: nothing is permuted in memory; piv[j] is the row step j took).  The pivot is the largest remaining diagonal entry, the
 * lowest index on ties; the factorisation ends when that entry is <= D * 2^-52 * d0 or <= 0 (d0: the largest diagonal entry of S;
 * d0 <= 0 gives rank 0).  info[0] = rank, info[1] = status: 0, or HOIG_EINVAL for a non-finite entry of S, in which case L, piv and
 * info[0] are left as they are.  Columns [rank, D) of L and piv[rank ..] are left as they are too.
 * Device: 3 + D launches on `stream` (a step that finds the factorisation finished returns at once); never synchronises, allocates
 * nothing; info, piv, workspace (8-byte aligned, >= hoig_pchol_f64_workspace_bytes) in device memory.  The twin also RETURNS the status. */
int64_t hoig_pchol_f64_workspace_bytes(int D);
int hoig_pchol_f64(const double *S, int64_t lds, int D, double *L, int64_t ldl, int32_t *piv, int32_t *info, void *workspace,
                   int64_t workspace_bytes, hoig_stream_t stream);
int hoig_pchol_f64_host(const double *S, int64_t lds, int D, double *L, int64_t ldl, int32_t *piv, int32_t *info);
/* The eigenvalues of the symmetric A [n][n] (both triangles are read), ascending: unblocked Householder tridiagonalisation (three
 * launches per step) in the workspace, then bisection on Sturm counts with Gershgorin bounds and dstebz's pivmin, one lane per
 * eigenvalue, to a width of 2 * 2^-52 * |lambda|.  info[0] = status: 0, or HOIG_EINVAL for a non-finite entry (lambda is then left as
 * it is).  The workspace holds, after its 32-byte header, the reduced matrix [n][n], then the tridiagonal's d [n] and e [n].
 * hoig_tridiag_eigvals_f64: the bisection alone, on d [n] and e [n - 1]; hoig_sym_tridiag_f64_host: the twin's tridiagonal alone. */
int64_t hoig_sym_eigvals_f64_workspace_bytes(int n);
int hoig_sym_eigvals_f64(const double *A, int64_t lda, int n, double *lambda, int32_t *info, void *workspace, int64_t workspace_bytes,
                         hoig_stream_t stream);
int hoig_sym_eigvals_f64_host(const double *A, int64_t lda, int n, double *lambda, int32_t *info);
int hoig_tridiag_eigvals_f64(const double *d, const double *e, int n, double *lambda, hoig_stream_t stream);
int hoig_tridiag_eigvals_f64_host(const double *d, const double *e, int n, double *lambda);
int hoig_sym_tridiag_f64_host(const double *A, int64_t lda, int n, double *d, double *e);

/* ---- FEATURE-SPACE METRICS IN FP64: KID AND PRECISION / RECALL (hoig_amd/csrc/feature_metrics.hip, feature_metrics.h,
 *      feature_metrics_host.cpp; hoig_amd/metrics/feature_metrics.py; docs/feature_metrics.md).  Feature sets are row-major fp32
 *      [n][D], any D >= 1; every product is a 64 x 64 tile of P Q^T on v_mfma_f64_16x16x4_f64 from rows staged through LDS, and no tile
 *      is stored.  No floating-point atomics, no grid-wide wait: every sum has one owner and a fixed order.  A status word (one int32 in
 *      device memory, written by the call) is 0 or an OR of 1: a non-finite feature was read, 2: an index of a gather table lay
 *      outside its set and was clamped into it.  Every device entry never synchronises and allocates nothing; workspaces are 8-byte
 *      aligned device memory of at least the stated size.  The *_host twins take host memory, make no HIP call and walk the same
 *      tiles, lanes and reductions; their dot products are summed in order of k, so tile values are close to the device's, not
 *      equal, while every reduction of tile values is the device's bit for bit. ---- */
/* S * 3 * ceil(m / 64)^2 doubles: one partial per (subset, term, tile) -- O(tiles), never O(m^2).  HOIG_EINVAL for S < 1, S > 65535
 * or m < 2. */
int64_t hoig_kid_workspace_bytes(int S, int m);
/* The polynomial-kernel sums of KID for S subsets at once.  k(a, b) = (gamma a.b + coef0)^degree, degree in 1 .. 4 by repeated
 * multiplication.  Subset s is the rows ix[s][0 .. m) of X [nx][D] and iy[s][0 .. m) of Y [ny][D] (int32 tables in device memory; an
 * index is clamped into its set before every read, which also sets status bit 2).  out[s] = {sum_{i != j} k(x_i, x_j),
 * sum_{i != j} k(y_i, y_j), sum_{i, j} k(x_i, y_j), mmd^2} with mmd^2 = (Sxx / (m (m - 1)) + Syy / (m (m - 1))) - 2 Sxy / m^2; i and j
 * are positions in the subset, and i == j is left out by position.  Grid (tile, term, subset): xx and yy run the tiles on and above
 * the diagonal only and count the others twice; a workgroup leaves one partial at its own slot and hoig_kid_finish_f64, one wave per
 * subset, adds the slots in slot order.  A non-zero status makes every entry of out NaN.  Two launches.
 * HOIG_EINVAL, and nothing launched: a NULL pointer, a size below 1, m < 2, S > 65535, degree outside 1 .. 4, a small workspace. */
int hoig_kid_poly_f64(const float *X, int nx, const float *Y, int ny, int D, const int32_t *ix, const int32_t *iy, int S, int m,
                      double gamma, double coef0, int degree, double *out, int32_t *status, void *workspace, int64_t workspace_bytes,
                      hoig_stream_t stream);
int hoig_kid_poly_f64_host(const float *X, int nx, const float *Y, int ny, int D, const int32_t *ix, const int32_t *iy, int S, int m,
                           double gamma, double coef0, int degree, double *out, int32_t *status);
/* The finishing stage alone: partials [S][3][nt * nt] (nt = ceil(m / 64), slot ti * nt + tj; of xx and yy only the slots with
 * tj >= ti are read) -> out [S][4].  Lane l of the subset's wave adds slots l, l + 64, .. in order, then the 64 lane sums meet in the
 * butterfly of fid_stats.h: a function of the partials alone.  status may be NULL (taken as 0). */
int hoig_kid_finish_f64(const double *partials, int S, int m, const int32_t *status, double *out, hoig_stream_t stream);
int hoig_kid_finish_f64_host(const double *partials, int S, int m, const int32_t *status, double *out);
/* radius[i] = the k-th smallest of d2(x_i, x_j) over j != i (left out by index, not by value), 1 <= k <= min(8, n - 1), for the rows
 * of X [n][D].  d2 = max(0, (|x|^2 + |y|^2) - 2 x.y) in fp64 on operands (double)x - pivot[c] (pivot: D doubles, or NULL; distances
 * do not depend on it, the cancellation does).  Grid (row tile, column chunk): a chunk leaves its 8 smallest candidates per row in the
 * workspace and a merge kernel takes the k-th of them all; the k smallest of a multiset do not depend on the order.  A non-zero
 * status makes every radius NaN.  Three launches.  HOIG_EINVAL: a NULL pointer, n < 2, D < 1, k out of range, a small workspace. */
int64_t hoig_knn_workspace_bytes(int n);
int hoig_knn_radius_f64(const float *X, int n, int D, const double *pivot, int k, double *radius, int32_t *status, void *workspace,
                        int64_t workspace_bytes, hoig_stream_t stream);
int hoig_knn_radius_f64_host(const float *X, int n, int D, const double *pivot, int k, double *radius, int32_t *status);
/* hits[j] = the number of rows i of X [nx][D] with d2(x_i, y_j) <= radius[i], for the rows of Y [ny][D]; d2 and pivot as above.
 * Grid (probe tile, row chunk): per-chunk int32 counts in the workspace, added by a second kernel; integer sums do not depend on the
 * order.  With a non-zero status the counts are unspecified.  Four launches. */
int64_t hoig_manifold_hits_workspace_bytes(int nx, int ny);
int hoig_manifold_hits_f64(const float *X, int nx, const double *radius, const float *Y, int ny, int D, const double *pivot,
                           int32_t *hits, int32_t *status, void *workspace, int64_t workspace_bytes, hoig_stream_t stream);
int hoig_manifold_hits_f64_host(const float *X, int nx, const double *radius, const float *Y, int ny, int D, const double *pivot,
                                int32_t *hits, int32_t *status);

/* ---- GRADIENT GUARD: STATISTICS, SKIP-STEP AND NORM CLIPPING ON THE DEVICE (hoig_amd/csrc/grad_guard.hip, grad_guard.h,
 *      grad_guard_host.cpp; hoig_amd/guard.py; docs/grad_guard.md).  The *_host twins take host memory, make no HIP call and walk
 *      every sum in the device's order: their results are the device's, bit for bit. ---- */
#define HOIG_GRAD_CHUNK 4096          /* elements of a stage-1 chunk (hoig_grad_stats_chunk() returns it) */
enum { HOIG_GUARD_SKIP = 1 };         /* hoig_guard_decide: a non-finite gradient skips the update (without it, it is only counted) */
int hoig_grad_stats_chunk(void);
int hoig_grad_stats_max_grid(void);   /* the most workgroups stage 1 uses: a longer buffer is walked in several rounds */
/* Statistics of the fp32 buffer x[0 .. n), for the whole of it (total[3]) and for each of the nseg rows {first, count} of a table
 * (seg_out[nseg][3]): {sum x^2 over the finite elements, max |x| over the finite elements, the number of non-finite elements}, doubles,
 * the count exact.  Rows are int64, sorted, disjoint, count >= 1, inside [0, n); gaps are allowed.  Squares and sums are fp64 and the
 * order of the additions is a function of (n, table) alone (grad_guard.h); `total` does not depend on the table at all.
 * The table is given twice, as for the PNG decoder's plans: segs_host is read at the call (HOIG_EINVAL for n <= 0, a bad table, a NULL
 * or misaligned pointer: nothing is launched, the outputs stay as they are), segs_dev is the same rows in device memory, read by the
 * kernels.  Only segs_host is checked: THE CALLER GUARANTEES THAT THE TWO COPIES HOLD THE SAME ROWS.  (The kernels clamp every piece to
 * its chunk and every row's slots to the workspace, so a differing device copy gives wrong statistics, not an access outside x or the
 * workspace; seg_out is indexed by the row number alone.)  x, seg_out, total and workspace (8-byte aligned, >= hoig_grad_stats_workspace_bytes(n, nseg); < 0: invalid) are device
 * memory.  Two launches on `stream`; never synchronises, allocates nothing. */
int64_t hoig_grad_stats_workspace_bytes(int64_t n, int nseg);
int hoig_grad_stats(const float *x, int64_t n, const int64_t *segs_host, const int64_t *segs_dev, int nseg, double *seg_out,
                    double *total, void *workspace, hoig_stream_t stream);
int hoig_grad_stats_host(const float *x, int64_t n, const int64_t *segs, int nseg, double *seg_out, double *total, void *workspace);
/* The decision, one thread: norm = pre_scale * sqrt(total[0]) in double.  guard[1] (skip) = 1.0f when total[2] > 0 and flags has
 * HOIG_GUARD_SKIP, else 0.0f; guard[0] (scale) = 1.0f, or (float)(max_norm / (norm + 1e-6)) -- torch.nn.utils.clip_grad_norm_'s
 * coefficient -- when max_norm > 0, total[2] == 0 and norm > max_norm.  record[7] (doubles, the caller zeroes it once): steps seen,
 * steps skipped, steps clipped, the last norm, the last pre_scale * max |x|, the last non-finite count, the largest finite norm seen.
 * HOIG_EINVAL: a NULL pointer, unknown flags, pre_scale <= 0, max_norm < 0. */
int hoig_guard_decide(const double *total, double pre_scale, double max_norm, int flags, float *guard, double *record,
                      hoig_stream_t stream);
int hoig_guard_decide_host(const double *total, double pre_scale, double max_norm, int flags, float *guard, double *record);
/* The device-schedule Adam entry points under a guard = {scale, skip} (two floats in device memory, written by hoig_guard_decide).
 * skip != 0: the tick leaves state[4] and `derived` as they are (as torch's GradScaler leaves the step count), the step kernels
 * return without touching a parameter, a moment or an operand plane.  Otherwise the gradient is read as g * (grad_scale * guard[0]);
 * with guard = {1.0f, 0.0f} the results are those of the unguarded entry points bit for bit.  The same kernel bodies, instantiated
 * with a template flag.  The host-schedule hoig_adam_step has no guarded form: a guard's decision exists on the device only. */
int hoig_adam_tick_guarded(double *state, float *derived, const float *guard, hoig_stream_t stream);
int hoig_adam_step_dev_guarded(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, const float *derived,
                               float grad_scale, const float *guard, hoig_stream_t stream);
int hoig_adam_pack_step_guarded(float *flat, const float *grad, float *exp_avg, float *exp_avg_sq, const float *derived,
                                float grad_scale, const int64_t *segs, int nseg, int64_t ntiles, const int64_t *plain, int64_t nplain,
                                uint16_t *hi_f, uint16_t *lo_f, uint16_t *hi_d, uint16_t *lo_d, const float *guard,
                                hoig_stream_t stream);

/* ---- EMA OF A NETWORK'S WEIGHTS ON THE DEVICE (hoig_amd/csrc/ema.hip, ema.h, ema_host.cpp; hoig_amd/ema.py; docs/ema.md).  The
 *      *_host twins take host memory, make no HIP call and run the same inline functions: their results are the device's, bit for
 *      bit.  `guard` is NULL or the {scale, skip} pair of hoig_guard_decide; only skip (guard[1]) is read. ---- */
/* The schedule, one thread: state = {decay, warmup (0 or 1), updates} (doubles).  With t = state[2],
 * beta = warmup ? min(decay, (1 + t) / (10 + t)) : decay in double; derived[0] = (float)(1.0 - beta), state[2] = t + 1.  guard[1] != 0:
 * nothing changes, as hoig_adam_tick_guarded leaves its count.  HOIG_EINVAL: state or derived NULL. */
int hoig_ema_tick(double *state, float *derived, const float *guard, hoig_stream_t stream);
int hoig_ema_tick_host(double *state, float *derived, const float *guard);
/* ema[i] = ema[i] + (param[i] - ema[i]) * derived[0] for i in [0, n), fp32, three roundings in that order (no contraction).  `param`
 * is only read.  guard[1] != 0: the kernel returns before the first load.  HOIG_EINVAL, and nothing launched: a NULL ema, param or
 * derived, n <= 0, ema or param not 16-byte aligned, the two ranges sharing an element (ema == param among them). */
int hoig_ema_update(float *ema, const float *param, int64_t n, const float *derived, const float *guard, hoig_stream_t stream);
int hoig_ema_update_host(float *ema, const float *param, int64_t n, const float *derived, const float *guard);
/* Exchanges a[0 .. n) and b[0 .. n) in place.  HOIG_EINVAL, and nothing launched: a NULL pointer, n <= 0, a pointer not 16-byte
 * aligned, overlapping ranges. */
int hoig_swap_f32(float *a, float *b, int64_t n, hoig_stream_t stream);

/* ---- DIFFERENTIABLE AUGMENTATION IN FRONT OF THE DISCRIMINATOR (hoig_amd/csrc/d_augment.hip, d_augment.h, d_augment_host.cpp;
 *      hoig_amd/d_augment.py; docs/d_augment.md).  The *_host twins take host memory, make no HIP call and run the same inline
 *      functions: their results are the device's, bit for bit.  Every entry point returns HOIG_EINVAL, and writes nothing, for a NULL
 *      or misaligned pointer (state: 8 bytes; params: 16; floats: 4), a non-positive size or an unknown site. ---- */
#define HOIG_DAUG_COLOR 1          /* the bits of a record's flags and of the state's policy word */
#define HOIG_DAUG_TRANSLATION 2
#define HOIG_DAUG_CUTOUT 4
#define HOIG_DAUG_SITES 3          /* 0: D(fake) in the G phase, 1: real in the D phase, 2: fake in the D phase */
#define HOIG_DAUG_STATE_WORDS 16   /* 64-bit words of the state (layout: d_augment.h, docs/d_augment.md) */
#define HOIG_DAUG_THREADS 256      /* threads of a reduction workgroup */
#define HOIG_DAUG_MAX_PARTS 16     /* the most partial sums per sample; ws holds B * HOIG_DAUG_MAX_PARTS floats */
/* B * HOIG_DAUG_MAX_PARTS: the floats of the workspace hoig_daug_fwd / hoig_daug_bwd take (HOIG_EINVAL for B <= 0) */
int hoig_daug_ws_floats(int B);
/* One thread: the step index (state word 0) goes up by one.  Once per training step, before its first draw. */
int hoig_daug_tick(uint64_t *state, hoig_stream_t stream);
int hoig_daug_tick_host(uint64_t *state);
/* params[i] = the 8-word record {b, s, k, ty, tx, cut_y0, cut_x0, flags} of sample i in [0, B) for maps of H x W, from
 * Philox4x32-10 with key (seed, rank) and counters (step low, step high, site, 3 i + j), j = 0, 1, 2; a family that the policy lacks
 * or whose gate fails writes its identity (b 0, s 1, k 1, shifts 0, box origin 0) and clears its flag. */
int hoig_daug_draw(const uint64_t *state, int site, int B, int H, int W, uint32_t *params, hoig_stream_t stream);
int hoig_daug_draw_host(const uint64_t *state, int site, int B, int H, int W, uint32_t *params);
/* The adaptive probability: counts d_real[0 .. n) > 0 and < 0 (integers), adds them to the interval's counters, and on every
 * `interval`-th call sets p <- clamp(p + sign((pos - neg) / total - target) * increment, 0, 1) and clears the counters. */
int hoig_daug_adapt(uint64_t *state, const float *d_real, int64_t n, hoig_stream_t stream);
int hoig_daug_adapt_host(uint64_t *state, const float *d_real, int64_t n);
/* out [B][H][W][3 + k] = the augmented concatenation of img [B][H][W][3] and cond [B][H][W][k] under params [B][8] (NHWC fp32; `out`
 * may be one half of a larger tensor).  Two launches: the per-sample image sums into ws (samples without the colour flag are left
 * out), then the output.  With every flag clear `out` is hoig_cat2_channels' bit for bit.  `out` and `ws` may not overlap an input. */
int hoig_daug_fwd(const float *img, const float *cond, const uint32_t *params, float *out, int B, int H, int W, int k, float *ws,
                  hoig_stream_t stream);
int hoig_daug_fwd_host(const float *img, const float *cond, const uint32_t *params, float *out, int B, int H, int W, int k, float *ws);
/* dimg [B][H][W][3] = the gradient of hoig_daug_fwd with respect to img, from g [B][H][W][3 + k], the gradient of its output.  Two
 * launches: the per-sample sums of g over the image channels of the surviving pixels into ws, then dimg. */
int hoig_daug_bwd(const float *g, const uint32_t *params, float *dimg, int B, int H, int W, int k, float *ws, hoig_stream_t stream);
int hoig_daug_bwd_host(const float *g, const uint32_t *params, float *dimg, int B, int H, int W, int k, float *ws);

/* ---- LAPLACIAN-PYRAMID SLICED WASSERSTEIN DISTANCE (hoig_amd/csrc/swd.hip, swd.h, swd_host.cpp; hoig_amd/metrics/swd.py;
 *      docs/swd.md).  A distribution metric between two sets of uint8 images that needs no network.  No floating-point atomics and
 *      no launch that waits for another workgroup: every sum has one owner and an order fixed by the sizes alone.  Device entries
 *      never synchronise and allocate nothing; workspaces are 8-byte aligned device memory of at least the stated size.  The *_host
 *      twins take host memory, make no HIP call and run the same inline functions in the same order: their results are the device's,
 *      bit for bit.  HOIG_EINVAL, and nothing launched, for a NULL or misaligned pointer, a size out of range or a small workspace. ---- */
#define HOIG_SWD_K 147             /* floats of a descriptor: a 7 x 7 patch of 3 channels, flattened as (c, dy, dx) */
#define HOIG_SWD_DEGENERATE 7      /* status bits 1 << c: channel c of hoig_swd_channel_stats_f64 has a zero standard deviation */
#define HOIG_SORT_NAN 8            /* status bit of hoig_sort_segments_f32: a NaN key was read */
#define HOIG_SORT_LDS_MAX 2048     /* the longest segment of the sort's single-workgroup LDS route */
#define HOIG_SORT_TILE 4096        /* keys of a workgroup's tile in the multi-pass route */
/* floor(log2(min(H, W) / 16)) + 1 (0 below 16): the levels of an H x W image */
int hoig_swd_levels(int H, int W);
/* positions [n][L][patches][2] (int32: y0, x0) of the patches of images first_index .. first_index + n - 1 of set `set_id`: the
 * top-left corner at level l is uniform on [0, (H >> l) - 7] x [0, (W >> l) - 7], drawn as (u32 * range) >> 32 from words 0 and 1
 * of Philox4x32-10 with key (seed low, seed high) and counter (set id, level, image index low word, patch index). */
int hoig_swd_positions(uint64_t seed, int set_id, int64_t first_index, int n, int H, int W, int L, int patches, int32_t *positions,
                       hoig_stream_t stream);
int hoig_swd_positions_host(uint64_t seed, int set_id, int64_t first_index, int n, int H, int W, int L, int patches, int32_t *positions);
/* The Gaussian levels 1 .. L - 1 of n images as NHWC fp32 (HOIG_EINVAL for a shape the pyramid does not take: H or W below 16 or
 * not divisible by 2^(L-1), L above hoig_swd_levels). */
int64_t hoig_swd_descriptors_workspace_bytes(int n, int H, int W, int L);
/* out [L][n][patches][147] fp32: the patches of the Laplacian pyramid of u8 [n][H][W][3] at `positions` (clamped into the level).
 * Filter [1, 4, 6, 4, 1] / 16 as two passes with scipy's 'mirror' boundary; lap[l] = g[l] - up(g[l+1]), lap[L-1] = g[L-1].  The
 * Gaussian chain goes to the workspace (L - 1 launches, the horizontal pass staged in LDS); the Laplacian levels are never stored:
 * the gather kernel takes each value from g[l] and at most 3 x 3 values of g[l+1].  L launches. */
int hoig_swd_descriptors_u8(const uint8_t *u8, int n, int H, int W, int L, int patches, const int32_t *positions, float *out,
                            void *workspace, int64_t workspace_bytes, hoig_stream_t stream);
int hoig_swd_descriptors_u8_host(const uint8_t *u8, int n, int H, int W, int L, int patches, const int32_t *positions, float *out);
/* stats [3][2] doubles = {mean, population standard deviation} of channel c over all 49 * rows values of descriptor rows
 * [rows][147]: the sum, then sum (x - mean)^2, both fp64 in chunks (swd.h).  status = OR of 1 << c for a zero deviation.  Three
 * launches. */
int64_t hoig_swd_channel_stats_workspace_bytes(int64_t rows);
int hoig_swd_channel_stats_f64(const float *desc, int64_t rows, double *stats, int32_t *status, void *workspace, int64_t workspace_bytes,
                               hoig_stream_t stream);
int hoig_swd_channel_stats_f64_host(const float *desc, int64_t rows, double *stats, int32_t *status);
/* out [D][rows] (direction-major) = the projections of the normalised descriptors on dirs [147][D]: operand
 * (float)(((double)x - mean_c) / std_c), the sum over k = 0 .. 146 in order by fp32 fused multiply-adds from 0.  64 x 64 tiles, the
 * operands staged through LDS one channel at a time. */
int hoig_swd_project_f32(const float *desc, int64_t rows, const double *stats, const float *dirs, int D, float *out, hoig_stream_t stream);
int hoig_swd_project_f32_host(const float *desc, int64_t rows, const double *stats, const float *dirs, int D, float *out);
/* Sorts each of the S segments of n fp32 keys (keys [S][n], 4-byte aligned) ascending, in place, as unsigned integers under the
 * order-preserving map (-0 before +0; a NaN sorts by its bits and sets HOIG_SORT_NAN in *status, which the call clears first).
 * n <= HOIG_SORT_LDS_MAX: one workgroup per segment, a bitonic network in LDS.  Longer: four passes of an 8-bit LSD radix sort --
 * per-tile digit counts, a scan per segment, a rank-preserving scatter -- between `keys` and the workspace. */
int64_t hoig_sort_segments_workspace_bytes(int64_t S, int64_t n);
int hoig_sort_segments_f32(float *keys, int64_t S, int64_t n, void *workspace, int32_t *status, hoig_stream_t stream);
int hoig_sort_segments_f32_host(float *keys, int64_t S, int64_t n, int32_t *status);
int hoig_sort_segments_lds_max(void);
int hoig_sort_segments_tile(void);
/* out[0] = sum |a[i] - b[i]|, i in [0, N), in fp64: one partial per workgroup, then one finishing wave.  Two launches. */
int64_t hoig_swd_sorted_l1_workspace_bytes(int64_t N);
int hoig_swd_sorted_l1_f64(const float *a, const float *b, int64_t N, double *out, void *workspace, int64_t workspace_bytes,
                           hoig_stream_t stream);
int hoig_swd_sorted_l1_f64_host(const float *a, const float *b, int64_t N, double *out);

/* ---- REGION SCORES: MASKED PSNR / MAE SUMS AND SQUARE CROPS OF LABELLED REGIONS (hoig_amd/csrc/region_metrics.hip,
 *      region_metrics.h, region_metrics_host.cpp; hoig_amd/metrics/regions.py; docs/region_metrics.md).  A label map is uint8
 *      [N][H][W]: 0 background, r in 1 .. R region r.  Every quantity is an integer or a byte, so no result depends on the order
 *      of a sum.  Device entries never synchronise and allocate nothing; the *_host twins take host memory, make no HIP call and
 *      run the same inline functions.  HOIG_EINVAL, and nothing launched, for a NULL or misaligned pointer, H or W outside
 *      1 .. 4096, R outside 1 .. HOIG_REGION_MAX, S outside HOIG_REGION_MIN_SIZE .. HOIG_REGION_MAX_SIZE. ---- */
#define HOIG_REGION_MAX 7          /* the most regions (label values 1 .. 7) */
#define HOIG_REGION_ROW 8          /* int64 of a statistics row */
#define HOIG_REGION_MIN_SIZE 4     /* the range of a crop's output side S */
#define HOIG_REGION_MAX_SIZE 512
#define HOIG_REGION_BAD_LABEL 1    /* status bit 0: a label above R was read; bits 8 .. 15 then hold the largest such label */
/* stats [N][R + 1][8] int64, row = [count, sum |d|, sum d^2, x0, y0, x1, y1, 0] with d = gen - gt per channel, summed over the 3
 * channels of the row's pixels; (x0, y0, x1, y1) their inclusive bounding box, (W, H, -1, -1) for an empty row.  Row 0: every
 * pixel of the image; row r: the pixels labelled r.  A label above R counts in row 0 only and sets *status (above).  One pass over
 * gen, gt [N][H][W][3] and labels: per-lane integer partials, a sum per workgroup, then integer atomics on `stats` (add, min,
 * max), which the entry initialises together with *status in a launch of its own.  8-byte aligned stats, 4-byte aligned status. */
int hoig_region_stats_u8(const uint8_t *gen, const uint8_t *gt, const uint8_t *labels, int N, int H, int W, int R, int64_t *stats,
                         int32_t *status, hoig_stream_t stream);
int hoig_region_stats_u8_host(const uint8_t *gen, const uint8_t *gt, const uint8_t *labels, int N, int H, int W, int R, int64_t *stats,
                              int32_t *status);
/* boxes [N][R][4] int32 = [left, top, side, valid] from the rows 1 .. R of `stats`: side0 = max(x1 - x0 + 1, y1 - y0 + 1),
 * pad = (side0 + 3) / 4, side = min(side0 + 2 pad, H, W), left = clamp(floor((x0 + x1 + 1 - side) / 2), 0, W - side), top likewise
 * with y and H, valid = count >= max(min_pixels, 1); an invalid box is (0, 0, 0, 0).  Square and inside the image. */
int hoig_region_boxes(const int64_t *stats, int N, int H, int W, int R, int min_pixels, int32_t *boxes, hoig_stream_t stream);
int hoig_region_boxes_host(const int64_t *stats, int N, int H, int W, int R, int min_pixels, int32_t *boxes);
/* The taps of Pillow's 8-bit BILINEAR resize (hoig_pil_bilinear_table) of every source side 1 .. max_side to S, in one int32
 * buffer: [max_side, S], then (offset, ksize) of side s at words 2 s and 2 s + 1, then the tables; offsets count int32 from the
 * start.  hoig_region_tables fills host memory of hoig_region_tables_bytes bytes. */
int64_t hoig_region_tables_bytes(int max_side, int S);
int hoig_region_tables(int max_side, int S, int32_t *tables);
/* dst [R][N][S][S][3]: crop (r, n) is the window (left, top, side) of boxes [N][R][4] in image n of src [N][H][W][3], resized to
 * S x S as Image.crop(box).resize((S, S), Image.BILINEAR) does it, equal in every byte (taps never reach outside the window); an
 * invalid box, or one that is not inside the image or the tables, gives zeros.  `tables`: hoig_region_tables(min(H, W), S) in
 * device memory.  Two launches: along x into the workspace (a grid sized for side = min(H, W), each workgroup reads its box and
 * leaves when it has nothing to do), then along y.  4-byte aligned dst and workspace. */
int64_t hoig_region_crop_workspace_bytes(int N, int H, int W, int R, int S);
int hoig_region_crop_resize_u8(const uint8_t *src, int N, int H, int W, const int32_t *boxes, int R, int S, const int32_t *tables,
                               uint8_t *dst, void *workspace, hoig_stream_t stream);
int hoig_region_crop_resize_u8_host(const uint8_t *src, int N, int H, int W, const int32_t *boxes, int R, int S, uint8_t *dst);

/* ---- OPT-IN GAN OBJECTIVES AND THE LECAM REGULARISER (hoig_amd/csrc/gan_loss.hip, gan_loss.h, gan_loss_host.cpp;
 *      hoig_amd/gan_loss.py; docs/gan_objectives.md).  One pass over D's logits gives the objective, its pre-scaled gradients, the
 *      report means and the regulariser; every sum is fp64 in an order fixed by the two sizes (no floating-point atomics, no wait
 *      between workgroups); the LeCam anchors live in a device state that the same call ticks.  The *_host twins take host memory, make
 *      no HIP call and run the same inline functions in the same order: outside HOIG_GAN_LOGISTIC their results are the device's, bit
 *      for bit.  Every entry point returns HOIG_EINVAL, and launches nothing, for an unknown mode or form, a non-positive count, a
 *      negative or non-finite weight, a misaligned pointer (state, workspace: 8 bytes; floats: 4), a missing logit pointer, a short
 *      workspace, or a gradient that overlaps the other side's logits or gradient. ---- */
#define HOIG_GAN_LSGAN 0           /* D: s mean((a - 1)^2) + s mean((b + 1)^2);          G: s mean(b^2) */
#define HOIG_GAN_HINGE 1           /* D: s mean(max(0, 1 - a)) + s mean(max(0, 1 + b));  G: -s mean(b) */
#define HOIG_GAN_LOGISTIC 2        /* D: s mean(softplus(-a)) + s mean(softplus(b));     G: s mean(softplus(-b)) */
#define HOIG_LECAM_PAPER 0         /* R = mean((a - alpha_F)^2) + mean((b - alpha_R)^2) */
#define HOIG_LECAM_RELU 1          /* R = mean(max(0, a - alpha_F)^2) + mean(max(0, alpha_R - b)^2) */
#define HOIG_LECAM_STATE_WORDS 8   /* 64-bit words of the state (layout: gan_loss.h, docs/gan_objectives.md) */
#define HOIG_GAN_THREADS 256       /* threads of a workgroup */
#define HOIG_GAN_CHUNK 512         /* logits of a chunk: a workgroup takes whole chunks */
#define HOIG_GAN_MAX_GRID 64       /* the most workgroups: with more chunks than this a workgroup walks several */
/* The D head.  a[0 .. n_a): D(real), b[0 .. n_b): D(fake), fp32; s: the objective's weight; state: the LeCam state (device memory,
 * HOIG_LECAM_STATE_WORDS words) or NULL for no regulariser.  With w = 1 when the state's tick count, as it stands before the call, has
 * reached its start word, else 0:
 *   da[i] = (float)(s / n_a) f_a'(a[i]) + (float)(w lambda_lc / n_a) r_a'(a[i]),   db likewise   (either may be NULL: not written)
 *   *term   += (float)(s mean f_a(a) + s mean f_b(b) + lambda_lc w R)
 *   *mean_a += (float)mean(a),  *mean_b += (float)mean(b),  *reg += (float)(w R)                 (each may be NULL)
 * and then the state takes its tick: alpha_R <- gamma alpha_R + (1 - gamma) mean(a), alpha_F likewise with mean(b) (the first tick
 * sets them to the means), count + 1 -- or, when a mean is not finite, only the state's refusal counter + 1.  The regulariser reads
 * the anchors as they stood before the call.  Two launches on `stream`; never synchronises, allocates nothing.  workspace: device
 * memory of hoig_gan_d_loss_workspace_bytes(n_a, n_b) bytes (< 0: invalid sizes). */
int64_t hoig_gan_d_loss_workspace_bytes(int64_t n_a, int64_t n_b);
int hoig_gan_d_loss(int mode, const float *a, int64_t n_a, const float *b, int64_t n_b, double s, double lambda_lc, int lecam_form,
                    uint64_t *state, float *da, float *db, float *term, float *mean_a, float *mean_b, float *reg, void *workspace,
                    int64_t workspace_bytes, hoig_stream_t stream);
int hoig_gan_d_loss_host(int mode, const float *a, int64_t n_a, const float *b, int64_t n_b, double s, double lambda_lc, int lecam_form,
                         uint64_t *state, float *da, float *db, float *term, float *mean_a, float *mean_b, float *reg);
/* The G head: db[i] = (float)(s / n_b) g'(b[i]) (or NULL) and *term += (float)(s mean g(b)) for the mode's generator term g.  No
 * state: the generator's objective has no LeCam term. */
int64_t hoig_gan_g_loss_workspace_bytes(int64_t n_b);
int hoig_gan_g_loss(int mode, const float *b, int64_t n_b, double s, float *db, float *term, void *workspace, int64_t workspace_bytes,
                    hoig_stream_t stream);
int hoig_gan_g_loss_host(int mode, const float *b, int64_t n_b, double s, float *db, float *term);

/* ---- OPT-IN REGION RECONSTRUCTION TERM FOR G (hoig_amd/csrc/region_loss.hip, region_loss.h, region_loss_host.cpp;
 *      hoig_amd/region_loss.py; docs/region_loss.md).  An L1 term per labelled region, each normalised by the region's own pixel
 *      count in its image, beside the whole-frame L1; the counts, the validity of every (image, region) row and the gradient scales
 *      are made and consumed on the device in the same call.  pred, target: fp32 [N][H][W][C]; labels: uint8 [N][H][W], 0 .. R.
 *      With n_ir the pixels of image i labelled r, row (i, r) valid when n_ir >= min_pixels, V_r the valid images of region r, d =
 *      pred - target:
 *        L_r   = (1 / V_r) sum_{i valid} (1 / (C n_ir)) sum_{p in r, c} |d|        (0 when V_r = 0)
 *        L_all = (1 / (N H W C)) sum |d|
 *        dpred = sign(d) ((float)(lambda_all / (N H W C)) + (valid_ir ? (float)(lambda_r / (V_r C n_ir)) : 0))   (NULL: not written)
 *        *term      += (float)(sum_r lambda_r L_r)     -- plus lambda_all L_all when term_all is NULL
 *        *term_all  += (float)(lambda_all L_all)       (may be NULL)
 *        terms_r[r] += (float)L_r, r = 0 .. R          (unweighted report slots; may be NULL)
 *        counts_out[i][r] = n_ir                       (int32 [N][R + 1]; may be NULL)
 *        *status = 0, or HOIG_REGION_BAD_LABEL with the largest label above R in bits 8 .. 15 (such a pixel is in L_all only)
 *      sign(0) = 0, and a NaN difference gets the gradient 0 (its sums are NaN).  Every floating-point sum is fp64 in an order fixed
 *      by (N, H, W, C): no floating-point atomics, no wait between workgroups; the counts are integer atomics.  One memset node and
 *      three launches on `stream`; never synchronises, allocates nothing.  The *_host twin takes host memory, makes no HIP call and
 *      gives the device's bits.  HOIG_EINVAL, and nothing launched, for a NULL or misaligned pointer (floats, int32: 4 bytes;
 *      workspace: 16), N outside 1 .. HOIG_RLOSS_MAX_N, H or W outside 1 .. 4096, C outside 1 .. HOIG_RLOSS_MAX_C, R outside
 *      0 .. HOIG_RLOSS_MAX_R, a negative or non-finite weight, min_pixels < 1, a short workspace, or a dpred that overlaps pred,
 *      target or labels. ---- */
#define HOIG_RLOSS_MAX_R 7         /* the most regions (label values 1 .. 7, as HOIG_REGION_MAX) */
#define HOIG_RLOSS_MAX_N 4096      /* the most images of a call */
#define HOIG_RLOSS_MAX_C 64        /* the most channels */
#define HOIG_RLOSS_THREADS 256     /* threads of a workgroup */
#define HOIG_RLOSS_TILE 4096       /* floats of one image that a workgroup of the value-and-gradient launch takes */
#define HOIG_RLOSS_COUNT_TILE 4096 /* labels of one image that a workgroup of the counting launch takes */
int64_t hoig_region_loss_workspace_bytes(int N, int H, int W, int C, int R);
int hoig_region_loss(const float *pred, const float *target, const uint8_t *labels, int N, int H, int W, int C, int R,
                     const double *lambda /*[R + 1], host memory*/, double lambda_all, int min_pixels, float *dpred, float *term,
                     float *terms_r, float *term_all, int32_t *counts_out, int32_t *status, void *workspace, int64_t workspace_bytes,
                     hoig_stream_t stream);
int hoig_region_loss_host(const float *pred, const float *target, const uint8_t *labels, int N, int H, int W, int C, int R,
                          const double *lambda, double lambda_all, int min_pixels, float *dpred, float *term, float *terms_r,
                          float *term_all, int32_t *counts_out, int32_t *status);

/* ---- OPT-IN STYLE (GRAM-MATRIX) TERM FOR G (hoig_amd/csrc/style_loss.hip, style_loss.h, style_loss_host.cpp; hoig_amd/style_loss.py;
 *      docs/style_loss.md).  fx, fy: fp32 [N][P][C], the NHWC features of one VGG level with P = H W.  Per image n:
 *        G(F)[n] = F[n]^T F[n] / (C P)                                  (C x C)
 *        L       = (1 / (N C^2)) sum_{n,i,j} |G(fx) - G(fy)|
 *        S[n]    = sign(G(fx)[n] - G(fy)[n]) (float)(2 scale / (N C^3 P))   (symmetric; sign(0) = 0, and 0 for a NaN difference)
 *        *term   += (float)(scale L),  *report += (float)L                 (either may be NULL)
 *        gram    = G(fx)[0 .. N), G(fy)[0 .. N) in double                  ([2N][C][C]; may be NULL)
 *        dfx[n]  = fx[n] S[n] = d(scale L) / d fx[n]                       (hoig_style_dfeat; fy gets no gradient)
 *      The Gram pass is split over tile pairs tj >= ti of HOIG_STYLE_TILE channels and over chunks of HOIG_STYLE_CHUNK pixels: every entry
 *      of a chunk's partial tile is an fp32 fma chain from +0 over the chunk's pixels in ascending order (v_mfma_f32_32x32x2_f32); the
 *      chunks are added in index order in double, and |d| in double in an order fixed by (N, P, C).  Every element of dfx is an fp32
 *      fma chain from +0 over the channels in ascending order.  No atomics, no wait between workgroups; three launches (gram) and one
 *      (dfeat) on `stream`; never synchronises, allocates nothing.  The *_host twins take host memory, make no HIP call and give the
 *      device's bits.  Nothing is launched and HOIG_EUNSUPPORTED is returned for N above HOIG_STYLE_MAX_N, P above HOIG_STYLE_MAX_P, or a C
 *      that is no multiple of 16 in 16 .. HOIG_STYLE_MAX_C; HOIG_EINVAL for N, P or C below 1, a NULL or misaligned pointer (fx, fy, S,
 *      dfx, gram, workspace: 16 bytes; term, report: 4), a negative or non-finite scale, a short workspace, an S or gram that overlaps
 *      an input or each other, or a dfx that overlaps fx or S. ---- */
#define HOIG_STYLE_TILE 64        /* channels of a Gram tile's edge, and columns of a gradient tile */
#define HOIG_STYLE_CHUNK 1024     /* pixels of one Gram partial: the longest fma chain of the Gram pass */
#define HOIG_STYLE_MAX_N 4096     /* the most images of a call */
#define HOIG_STYLE_MAX_P 4194304  /* the most pixels of an image (2^22) */
#define HOIG_STYLE_MAX_C 512      /* the most channels */
int64_t hoig_style_workspace_bytes(int N, int P, int C);
int hoig_style_gram(const float *fx, const float *fy, int N, int P, int C, double scale, float *S, float *term, float *report,
                    double *gram, void *workspace, int64_t workspace_bytes, hoig_stream_t stream);
int hoig_style_dfeat(const float *fx, const float *S, int N, int P, int C, float *dfx, hoig_stream_t stream);
int hoig_style_gram_host(const float *fx, const float *fy, int N, int P, int C, double scale, float *S, float *term, float *report,
                         double *gram);
int hoig_style_dfeat_host(const float *fx, const float *S, int N, int P, int C, float *dfx);

#ifdef __cplusplus
}
#endif
#endif
