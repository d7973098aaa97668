"""ctypes binding of libhoig_hip.so (the C ABI declared in include/hoig_kernels.h).

There is NO fallback: if the shared library is missing, or a symbol the header
declares is absent, importing this module raises.  Every product op in
``hoig_amd.ops`` goes through here.
"""
import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', '_build', 'libhoig_hip.so')
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'hoig_kernels.h')

OK, EINVAL, ELAUNCH, EUNSUPPORTED = 0, -1, -2, -3
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4
PREC_F32, PREC_BF16X3, PREC_BF16, PREC_F16X2, PREC_F16F6 = 0, 1, 2, 3, 4
LOSS_L1, LOSS_MSE, LOSS_BCE = 0, 1, 2
POOL_MAX, POOL_AVG = 0, 1
JPEG_SUBSEQ_BYTES = 64              # HOIG_JPEG_SUBSEQ_BYTES
PNG_SEGMENT_BYTES = 8192            # HOIG_PNG_SEGMENT_BYTES
GEMM_ACCUMULATE, GEMM_SYMMETRIC, GEMM_F32 = 1, 2, 4      # HOIG_GEMM_*
FM_NONFINITE, FM_CLAMPED = 1, 2     # the bits of a feature-metric status word (feature_metrics.h)
# HOIG_PNG_E*: the bits of a PNG decoder status word
PNG_ECODE, PNG_EBTYPE, PNG_ESTORED, PNG_EDIST, PNG_EEARLY, PNG_EMORE, PNG_ELESS, PNG_EFILTER, PNG_EADLER = 1, 2, 4, 8, 16, 32, 64, 128, 256
_ERR = {EINVAL: 'invalid argument', ELAUNCH: 'kernel launch failed', EUNSUPPORTED: 'unsupported shape'}


class HoigKernelError(RuntimeError):
    pass


class ConvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('B', 'Hi', 'Wi', 'Ci', 'Ho', 'Wo', 'Co', 'R', 'S', 'stride', 'pad',
                                              'transposed', 'act')] + \
               [('slope', ctypes.c_float), ('precision', ctypes.c_int32)]


def build(verbose=False):
    """Compile every HIP source for gfx950 into hoig_amd/csrc/_build/libhoig_hip.so."""
    script = os.path.join(_HERE, 'csrc', 'build.sh')
    out = subprocess.run(['bash', script], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or out.returncode != 0:
        print(out.stdout)
    if out.returncode != 0:
        raise RuntimeError('hipcc build of libhoig_hip.so failed')
    return LIB_PATH


def declared_symbols():
    """Entry points the header declares (used by the CPU test that checks the library exports all of them)."""
    text = open(HEADER_PATH).read()
    return sorted(set(re.findall(r'\b(hoig_[a-z0-9_]+)\s*\(', text)) - {'hoig_stream_t'})


_vp, _i, _i64, _f, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
_SIGS = {
    'hoig_conv2d_fwd': [ctypes.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp],
    'hoig_conv2d_bwd_data': [ctypes.POINTER(ConvDesc), _vp, _vp, _vp, _vp],
    'hoig_conv2d_fwd_heads': [ctypes.POINTER(ConvDesc), _vp, _vp, _vp, _vp, ctypes.c_uint64, _vp],
    'hoig_conv2d_bwd_weight': [ctypes.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp],
    'hoig_pack_conv_weight_bf16': [_vp, _i, _i, _i, _i, _vp, _vp, _vp],
    'hoig_pack_conv_weights_bf16_all': [_vp, _vp, _i, _i64, _vp, _vp, _vp, _vp, _vp],
    'hoig_conv2d_fwd_packed': [ctypes.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp],
    'hoig_conv2d_bwd_data_packed': [ctypes.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp],
    'hoig_conv2d_fwd_packed_stats': [ctypes.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'hoig_conv2d_fwd_stats': [ctypes.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp],
    'hoig_conv2d_cat_fwd_packed_stats': [ctypes.POINTER(ConvDesc), _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'hoig_inorm_stats_from_sums': [_vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp],
    'hoig_conv2d_bwd_data_packed_add': [ctypes.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp],
    'hoig_pack_conv_weight_f6': [_vp, _i, _i, _i, _vp, _vp, _vp],
    'hoig_conv2d_fwd_f6': [ctypes.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'hoig_pack_conv_weights_f6_all': [_vp, _vp, _i, _i64, _vp, _vp, _vp],
    'hoig_conv2d_cat_fwd_f6': [ctypes.POINTER(ConvDesc), _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'hoig_conv2d_fwd_f6_ex': [ctypes.POINTER(ConvDesc), _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp],
    'hoig_conv2d_cat_fwd_packed': [ctypes.POINTER(ConvDesc), _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    'hoig_conv2d_cat_bwd_data_packed': [ctypes.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _i, _vp, _vp],
    'hoig_split_planes_bf16': [_vp, _vp, _i64, _i, _vp],
    'hoig_conv2d_bwd_weight_split': [ctypes.POINTER(ConvDesc), _vp, _vp, _vp, _vp],
    'hoig_conv2d_bwd_data_packed_split': [ctypes.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp],
    'hoig_conv2d_fwd_packed_pair': [ctypes.POINTER(ConvDesc)] + [_vp] * 11,
    'hoig_conv2d_bwd_data_packed_split_pair': [ctypes.POINTER(ConvDesc)] + [_vp] * 11,
    'hoig_conv2d_bwd_weight_split_pair': [ctypes.POINTER(ConvDesc)] + [_vp] * 7,
    'hoig_conv2d_cat_bwd_weight': [ctypes.POINTER(ConvDesc), _vp, _i, _vp, _vp, _vp, _vp, _vp],
    'hoig_inorm_stats': [_vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp],
    'hoig_inorm_apply': [_vp, _vp, _vp, _i, _vp, _vp, _i, _f, _vp, _vp, _i, _i, _i, _vp],
    'hoig_inorm_apply_ld': [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _f, _vp, _vp, _i, _i, _i, _vp],
    'hoig_inorm_bwd_ld': [_vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _f, _vp, _vp, _vp, _i, _i, _i, _vp, _vp],
    'hoig_inorm_fwd_fused': [_vp, _i, _vp, _vp, _i, _i, _f, _vp, _f, _vp, _vp, _vp, _i, _i, _i, _vp],
    'hoig_inorm_bwd_fused': [_vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _f, _vp, _vp, _vp, _i, _i, _i, _vp],
    'hoig_inorm_bwd_add_ld': [_vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp],
    'hoig_inorm_bwd_add_ld_split': [_vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp],
    'hoig_inorm_bwd_fused_add_split': [_vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    'hoig_inorm_fold': [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp],
    'hoig_conv2d_fwd_packed_normin': [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp],
    'hoig_unsplit_planes_bf16': [_vp, _vp, _i64, _i, _vp],
    'hoig_inorm_bwd_fused_add': [_vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    'hoig_inorm_bwd': [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _i, _i, _i, _vp, _vp],
    'hoig_replicate_pad_fwd': [_vp, _vp, _i, _i, _i, _i, _i, _vp],
    'hoig_replicate_pad_bwd': [_vp, _vp, _i, _i, _i, _i, _i, _vp],
    'hoig_replicate_pad_bwd_add': [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    'hoig_attn_pixel_fwd': [_vp] * 10 + [_i, _i, _i, _i, _vp],
    'hoig_attn_pixel_bwd': [_vp] * 10 + [_i, _i, _i, _i, _vp],
    'hoig_attn_build_index': [_vp, _vp, _i, _i, _i, _vp],
    'hoig_attn_src_gather': [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    'hoig_attn_gs_gather': [_vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    'hoig_block_extractor_forward': [_vp, _vp, _vp] + [_i] * 7 + [_vp],
    'hoig_block_extractor_backward': [_vp] * 5 + [_i] * 7 + [_vp],
    'hoig_local_attn_reshape_forward': [_vp, _vp] + [_i] * 4 + [_vp],
    'hoig_local_attn_reshape_backward': [_vp, _vp] + [_i] * 4 + [_vp],
    'hoig_grid_sample_fwd': [_vp, _vp, _vp] + [_i] * 6 + [_vp],
    'hoig_grid_sample_bwd': [_vp, _vp, _vp] + [_i] * 6 + [_vp],
    'hoig_resize_bilinear_ac': [_vp, _vp] + [_i] * 6 + [_vp],
    'hoig_resize_nearest': [_vp, _vp] + [_i] * 6 + [_vp],
    'hoig_attn_flow': [_vp, _vp, _i, _i, _vp],
    'hoig_maxpool2_fwd': [_vp, _vp] + [_i] * 4 + [_vp],
    'hoig_maxpool2_bwd': [_vp, _vp, _vp, _vp] + [_i] * 4 + [_vp],
    'hoig_nchw_to_nhwc': [_vp, _vp] + [_i] * 4 + [_vp],
    'hoig_nhwc_to_nchw': [_vp, _vp] + [_i] * 4 + [_vp],
    'hoig_copy_channels': [_vp, _vp, _i64, _i, _i, _i, _i, _i, _i, _vp],
    'hoig_cat2_channels': [_vp, _i, _vp, _i, _vp, _i64, _vp],
    'hoig_add': [_vp, _vp, _vp, _i64, _vp],
    'hoig_add_act': [_vp, _vp, _vp, _i, _f, _i64, _vp],
    'hoig_act_bwd': [_vp, _vp, _vp, _i, _f, _i64, _vp],
    'hoig_act_bwd_colsum': [_vp, _vp, _vp, _vp, _i, _f, _i64, _i, _vp],
    'hoig_colsum_accum': [_vp, _vp, _i64, _i, _vp],
    'hoig_compose_fwd': [_vp] * 6 + [_i64, _i, _vp],
    'hoig_compose_bwd': [_vp] * 11 + [_i64, _i, _vp],
    'hoig_loss_fwd_bwd': [_i, _vp, _vp, _f, _f, _vp, _vp, _i64, _vp],
    'hoig_tv_fwd_bwd': [_vp, _f, _f, _vp, _vp, _i, _i, _i, _vp],
    'hoig_loss_accumulate': [_i, _vp, _vp, _f, _f, _vp, _vp, _i64, _vp],
    'hoig_tv_accumulate': [_vp, _f, _f, _vp, _vp, _i, _i, _i, _vp],
    'hoig_sum': [_vp, _vp, _i64, _vp],
    'hoig_sum_scaled': [_vp, _f, _vp, _i64, _vp],
    'hoig_adam_step': [_vp, _vp, _vp, _vp, _i64, _d, _d, _d, _d, _i, _f, _vp],
    'hoig_adam_tick': [_vp, _vp, _vp],
    'hoig_adam_step_dev': [_vp, _vp, _vp, _vp, _i64, _vp, _f, _vp],
    'hoig_resize_linear_u8': [_vp, _i, _i, _i, _i, _vp, _i, _i, _vp],
    'hoig_warp_affine_u8': [_vp, _i, _i, _i, _i, _vp, _i, _i, _i, _vp, _vp],
    'hoig_adam_pack_step': [_vp, _vp, _vp, _vp, _vp, _f, _vp, _i, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp],
    'hoig_stream_create': [ctypes.POINTER(ctypes.c_void_p)],
    'hoig_stream_destroy': [_vp],
    'hoig_stream_scratch_set': [_vp, _vp, _i64],
    'hoig_tensor2im_u8': [_vp, _vp] + [_i] * 6 + [_vp],
    'hoig_tensor2im_nhwc_u8': [_vp, _vp, _i64, _i, _vp],
    'hoig_prep_texture': [_vp] * 9,
    'hoig_prep_lookup': [_vp] * 5 + [_i] + [_vp] * 8,
    'hoig_prep_assemble': [_i] + [_vp] * 17 + [_i] + [_vp] * 6,
    'hoig_rasterize_fim_wim': [_vp, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp],
    'hoig_pack_conv_weight_wino': [_vp, _i, _i, _vp, _vp, _vp],
    'hoig_conv2d_fwd_wino': [ctypes.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp],
    'hoig_project_faces': [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _f, _f, _vp, _vp],
    'hoig_prep_texture_batched': [_i, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'hoig_prep_lookup_batched': [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp],
    'hoig_mano_lbs': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp],
    'hoig_pool2d_fwd': [_vp, _vp] + [_i] * 10 + [_vp],
    'hoig_stage_images_u8': [_vp, _vp] + [_i] * 7 + [_vp, _vp],
    'hoig_pad2d': [_vp, _vp] + [_i] * 6 + [_vp],
    'hoig_global_avgpool': [_vp, _vp, _i, _i, _i, _vp],
    'hoig_lpips_layer': [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp],
    'hoig_ssim': [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _f, _i, _f, _vp, _vp],
    'hoig_jpeg_entropy_host': [_vp, _i64, _vp, _i, _vp, _i64, _vp, _i64, _vp],
    'hoig_jpeg_decode_bgr_u8': [_vp, _i64, _vp, _vp, _i, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp],
    'hoig_jpeg_reconstruct_bgr_u8': [_vp, _vp, _i, _vp, _i64, _vp, _i64, _vp],
    'hoig_jpeg_entropy_par_host': [_vp, _i64, _vp, _i, _vp, _i64, _i, _i, _vp, _i64, _vp, _vp, _vp, _i64],
    'hoig_jpeg_decode_bgr_u8_par': [_vp, _i64, _vp, _vp, _i, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i, _vp],
    'hoig_pil_bilinear_ksize': [_i, _i],
    'hoig_pil_bilinear_table': [_i, _i, _vp],
    'hoig_resize_pil_bilinear_u8_host': [_vp, _i, _i, _i, _i, _vp, _i, _i],
    'hoig_resize_pil_bilinear_u8': [_vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp],
    'hoig_png_encode_u8': [_vp, _i, _i, _i, _i, _vp, _i64, _vp, _vp, _i64, _i, _vp],
    'hoig_png_filter_host': [_vp, _i, _i, _i, _vp],
    'hoig_png_deflate_host': [_vp, _i64, _i, _i, _i, _vp, _i64, ctypes.POINTER(ctypes.c_int64), _vp],
    'hoig_png_encode_host': [_vp, _i, _i, _i, _i, _vp, _i64, _vp, _i],
    'hoig_png_inflate_host': [_vp, _i64, _vp, _i64, _vp],
    'hoig_png_decode_host': [_vp, _i64, _vp, _i, _vp, _i64, _vp, _vp, _i64, _i],
    'hoig_png_decode_u8': [_vp, _i64, _vp, _vp, _i, _vp, _i64, _vp, _vp, _i64, _i, _vp],
    'hoig_gemm_tn_f64': [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _i, _i, _i, _i, _vp],
    'hoig_gemm_tn_f64_host': [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _i, _i, _i, _i],
    'hoig_pchol_f64': [_vp, _i64, _i, _vp, _i64, _vp, _vp, _vp, _i64, _vp],
    'hoig_pchol_f64_host': [_vp, _i64, _i, _vp, _i64, _vp, _vp],
    'hoig_sym_eigvals_f64': [_vp, _i64, _i, _vp, _vp, _vp, _i64, _vp],
    'hoig_sym_eigvals_f64_host': [_vp, _i64, _i, _vp, _vp],
    'hoig_tridiag_eigvals_f64': [_vp, _vp, _i, _vp, _vp],
    'hoig_tridiag_eigvals_f64_host': [_vp, _vp, _i, _vp],
    'hoig_sym_tridiag_f64_host': [_vp, _i64, _i, _vp, _vp],
    'hoig_kid_poly_f64': [_vp, _i, _vp, _i, _i, _vp, _vp, _i, _i, _d, _d, _i, _vp, _vp, _vp, _i64, _vp],
    'hoig_kid_poly_f64_host': [_vp, _i, _vp, _i, _i, _vp, _vp, _i, _i, _d, _d, _i, _vp, _vp],
    'hoig_kid_finish_f64': [_vp, _i, _i, _vp, _vp, _vp],
    'hoig_kid_finish_f64_host': [_vp, _i, _i, _vp, _vp],
    'hoig_knn_radius_f64': [_vp, _i, _i, _vp, _i, _vp, _vp, _vp, _i64, _vp],
    'hoig_knn_radius_f64_host': [_vp, _i, _i, _vp, _i, _vp, _vp],
    'hoig_manifold_hits_f64': [_vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i64, _vp],
    'hoig_manifold_hits_f64_host': [_vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp],
    'hoig_grad_stats_chunk': [],
    'hoig_grad_stats_max_grid': [],
    'hoig_grad_stats': [_vp, _i64, _vp, _vp, _i, _vp, _vp, _vp, _vp],
    'hoig_grad_stats_host': [_vp, _i64, _vp, _i, _vp, _vp, _vp],
    'hoig_guard_decide': [_vp, _d, _d, _i, _vp, _vp, _vp],
    'hoig_guard_decide_host': [_vp, _d, _d, _i, _vp, _vp],
    'hoig_adam_tick_guarded': [_vp, _vp, _vp, _vp],
    'hoig_adam_step_dev_guarded': [_vp, _vp, _vp, _vp, _i64, _vp, _f, _vp, _vp],
    'hoig_adam_pack_step_guarded': [_vp, _vp, _vp, _vp, _vp, _f, _vp, _i, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp],
    'hoig_ema_tick': [_vp, _vp, _vp, _vp],
    'hoig_ema_tick_host': [_vp, _vp, _vp],
    'hoig_ema_update': [_vp, _vp, _i64, _vp, _vp, _vp],
    'hoig_ema_update_host': [_vp, _vp, _i64, _vp, _vp],
    'hoig_swap_f32': [_vp, _vp, _i64, _vp],
    'hoig_daug_ws_floats': [_i],
    'hoig_daug_tick': [_vp, _vp],
    'hoig_daug_tick_host': [_vp],
    'hoig_daug_draw': [_vp, _i, _i, _i, _i, _vp, _vp],
    'hoig_daug_draw_host': [_vp, _i, _i, _i, _i, _vp],
    'hoig_daug_adapt': [_vp, _vp, _i64, _vp],
    'hoig_daug_adapt_host': [_vp, _vp, _i64],
    'hoig_daug_fwd': [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp],
    'hoig_daug_fwd_host': [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    'hoig_daug_bwd': [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp],
    'hoig_daug_bwd_host': [_vp, _vp, _vp, _i, _i, _i, _i, _vp],
    'hoig_swd_levels': [_i, _i],
    'hoig_swd_positions': [ctypes.c_uint64, _i, _i64, _i, _i, _i, _i, _i, _vp, _vp],
    'hoig_swd_positions_host': [ctypes.c_uint64, _i, _i64, _i, _i, _i, _i, _i, _vp],
    'hoig_swd_descriptors_u8': [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i64, _vp],
    'hoig_swd_descriptors_u8_host': [_vp, _i, _i, _i, _i, _i, _vp, _vp],
    'hoig_swd_channel_stats_f64': [_vp, _i64, _vp, _vp, _vp, _i64, _vp],
    'hoig_swd_channel_stats_f64_host': [_vp, _i64, _vp, _vp],
    'hoig_swd_project_f32': [_vp, _i64, _vp, _vp, _i, _vp, _vp],
    'hoig_swd_project_f32_host': [_vp, _i64, _vp, _vp, _i, _vp],
    'hoig_sort_segments_f32': [_vp, _i64, _i64, _vp, _vp, _vp],
    'hoig_sort_segments_f32_host': [_vp, _i64, _i64, _vp],
    'hoig_sort_segments_lds_max': [],
    'hoig_sort_segments_tile': [],
    'hoig_swd_sorted_l1_f64': [_vp, _vp, _i64, _vp, _vp, _i64, _vp],
    'hoig_swd_sorted_l1_f64_host': [_vp, _vp, _i64, _vp],
    'hoig_region_stats_u8': [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp],
    'hoig_region_stats_u8_host': [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp],
    'hoig_region_boxes': [_vp, _i, _i, _i, _i, _i, _vp, _vp],
    'hoig_region_boxes_host': [_vp, _i, _i, _i, _i, _i, _vp],
    'hoig_region_tables': [_i, _i, _vp],
    'hoig_region_crop_resize_u8': [_vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp],
    'hoig_region_crop_resize_u8_host': [_vp, _i, _i, _i, _vp, _i, _i, _vp],
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            'hoig_amd: %s not found. The HIP extension is mandatory (no CPU / eager fallback exists); build it with '
            '`python -c "import __graft_entry__ as g; g.build()"` or `bash hoig_amd/csrc/build.sh`.' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, args in _SIGS.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch: fail loudly
        fn.argtypes = args
        fn.restype = ctypes.c_int
    lib.hoig_inorm_workspace_bytes.argtypes = [_i, _i, _i]
    lib.hoig_inorm_workspace_bytes.restype = ctypes.c_int64
    lib.hoig_set_f6_min_tiles.argtypes = [_i]
    lib.hoig_set_f6_min_tiles.restype = ctypes.c_int
    lib.hoig_f6_plane_bytes.argtypes = [_i, _i, _i]
    lib.hoig_f6_plane_bytes.restype = ctypes.c_int64
    lib.hoig_wino_plane_halfs.argtypes = [_i, _i]
    lib.hoig_wino_plane_halfs.restype = ctypes.c_int64
    lib.hoig_attn_index_ints.argtypes = [_i, _i, _i]
    lib.hoig_attn_index_ints.restype = ctypes.c_int64
    lib.hoig_rasterize_workspace_bytes.restype = ctypes.c_size_t
    lib.hoig_rasterize_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.hoig_set_tuning.argtypes = [ctypes.c_char_p, _i]
    lib.hoig_set_tuning.restype = ctypes.c_int
    lib.hoig_stream_scratch_bytes.argtypes = []
    lib.hoig_stream_scratch_bytes.restype = ctypes.c_int64
    lib.hoig_conv2d_bwd_weight_scratch_bytes.argtypes = [ctypes.POINTER(ConvDesc)]
    lib.hoig_conv2d_bwd_weight_scratch_bytes.restype = ctypes.c_int64
    lib.hoig_lpips_workspace_bytes.argtypes = [_i, _i]
    lib.hoig_lpips_workspace_bytes.restype = ctypes.c_int64
    lib.hoig_ssim_workspace_bytes.argtypes = [_i, _i, _i, _i, _i]
    lib.hoig_ssim_workspace_bytes.restype = ctypes.c_int64
    lib.hoig_resize_pil_bilinear_u8_workspace_bytes.argtypes = [_i] * 6
    lib.hoig_resize_pil_bilinear_u8_workspace_bytes.restype = ctypes.c_int64
    lib.hoig_png_encode_bound.argtypes = [_i] * 4
    lib.hoig_png_encode_bound.restype = ctypes.c_int64
    lib.hoig_png_encode_workspace_bytes.argtypes = [_i] * 5
    lib.hoig_png_encode_workspace_bytes.restype = ctypes.c_int64
    lib.hoig_png_decode_workspace_bytes.argtypes = [_vp, _i]
    lib.hoig_png_decode_workspace_bytes.restype = ctypes.c_int64
    lib.hoig_pchol_f64_workspace_bytes.argtypes = [_i]
    lib.hoig_pchol_f64_workspace_bytes.restype = ctypes.c_int64
    lib.hoig_sym_eigvals_f64_workspace_bytes.argtypes = [_i]
    lib.hoig_sym_eigvals_f64_workspace_bytes.restype = ctypes.c_int64
    lib.hoig_kid_workspace_bytes.argtypes = [_i, _i]
    lib.hoig_kid_workspace_bytes.restype = ctypes.c_int64
    lib.hoig_knn_workspace_bytes.argtypes = [_i]
    lib.hoig_knn_workspace_bytes.restype = ctypes.c_int64
    lib.hoig_manifold_hits_workspace_bytes.argtypes = [_i, _i]
    lib.hoig_manifold_hits_workspace_bytes.restype = ctypes.c_int64
    lib.hoig_swd_descriptors_workspace_bytes.argtypes = [_i] * 4
    lib.hoig_swd_descriptors_workspace_bytes.restype = ctypes.c_int64
    lib.hoig_swd_channel_stats_workspace_bytes.argtypes = [_i64]
    lib.hoig_swd_channel_stats_workspace_bytes.restype = ctypes.c_int64
    lib.hoig_sort_segments_workspace_bytes.argtypes = [_i64, _i64]
    lib.hoig_sort_segments_workspace_bytes.restype = ctypes.c_int64
    lib.hoig_swd_sorted_l1_workspace_bytes.argtypes = [_i64]
    lib.hoig_swd_sorted_l1_workspace_bytes.restype = ctypes.c_int64
    lib.hoig_region_tables_bytes.argtypes = [_i, _i]
    lib.hoig_region_tables_bytes.restype = ctypes.c_int64
    lib.hoig_region_crop_workspace_bytes.argtypes = [_i] * 5
    lib.hoig_region_crop_workspace_bytes.restype = ctypes.c_int64
    lib.hoig_grad_stats_workspace_bytes.argtypes = [_i64, _i]
    lib.hoig_grad_stats_workspace_bytes.restype = ctypes.c_int64
    lib.hoig_jpeg_decode_workspace_bytes.argtypes = [_vp, _i]
    lib.hoig_jpeg_decode_workspace_bytes.restype = ctypes.c_int64
    lib.hoig_jpeg_decode_par_workspace_bytes.argtypes = [_vp, _i, _i]
    lib.hoig_jpeg_decode_par_workspace_bytes.restype = ctypes.c_int64
    lib.hoig_conv_last_route.argtypes = [_i]
    lib.hoig_conv_last_route.restype = ctypes.c_int
    lib.hoig_conv_route_name.argtypes = [_i]
    lib.hoig_conv_route_name.restype = ctypes.c_char_p
    lib.hoig_version.argtypes = []
    lib.hoig_version.restype = ctypes.c_char_p
    return lib


lib = _load()

DAUG_COLOR, DAUG_TRANSLATION, DAUG_CUTOUT = 1, 2, 4      # HOIG_DAUG_*: the bits of a record's flags and of the policy word
DAUG_STATE_WORDS, DAUG_MAX_PARTS = 16, 16                # HOIG_DAUG_STATE_WORDS, HOIG_DAUG_MAX_PARTS
SWD_K, SWD_DEGENERATE, SORT_NAN = 147, 7, 8             # HOIG_SWD_K; the status bits HOIG_SWD_DEGENERATE (1 << channel), HOIG_SORT_NAN
SORT_LDS_MAX = lib.hoig_sort_segments_lds_max()          # HOIG_SORT_LDS_MAX: the longest segment of the sort's LDS route
SORT_TILE = lib.hoig_sort_segments_tile()                # HOIG_SORT_TILE: keys of a tile of its multi-pass route
REGION_MAX, REGION_BAD_LABEL = 7, 1                      # HOIG_REGION_MAX; the status bit HOIG_REGION_BAD_LABEL (the label: bits 8 .. 15)
GUARD_SKIP = 1                                   # HOIG_GUARD_SKIP
GRAD_CHUNK = lib.hoig_grad_stats_chunk()         # HOIG_GRAD_CHUNK: elements of a stage-1 chunk of hoig_grad_stats
GRAD_MAX_GRID = lib.hoig_grad_stats_max_grid()   # the most workgroups its stage 1 uses


def set_tuning(key, value):
    """hoig_set_tuning: kernel-variant choice `key` -> `value` (returns the previous value)."""
    prev = lib.hoig_set_tuning(key.encode(), int(value))
    if prev < 0:
        raise KeyError('unknown tuning key %r' % key)
    return prev


# HOIG_TUNING="key=value,key=value": variant choices for A/B runs (bench.py and the tools set them through this one variable)
for _kv in filter(None, os.environ.get('HOIG_TUNING', '').split(',')):
    set_tuning(*_kv.split('='))


ROUTE_FWD, ROUTE_DGRAD, ROUTE_WGRAD = 0, 1, 2


def route_names():
    """The library's table of convolution routes (hoig_amd/csrc/conv_route.h), by id."""
    names, i = [], 0
    while True:
        n = lib.hoig_conv_route_name(i)
        if n is None:
            return names
        names.append(n.decode())
        i += 1


def last_route(which):
    """hoig_conv_last_route: the name of the convolution launcher that ran last on this thread (0 forward, 1 data gradient,
    2 weight gradient; 'none' before the first)."""
    rid = lib.hoig_conv_last_route(int(which))
    if rid < 0:
        raise ValueError('last_route(%r): 0 forward, 1 data gradient, 2 weight gradient' % (which,))
    return lib.hoig_conv_route_name(rid).decode()


def check(rc, what):
    if rc != 0:
        raise HoigKernelError('%s failed: %s (code %d)' % (what, _ERR.get(rc, 'unknown'), rc))


# Every launch of the package goes through one of these two, reached as `L.call` / `L.attempt` (an attribute of this module, read at
# call time): a tool that rebinds the two names sees every launch (tools/op_table.py, tools/conv_table.py).
def call(name, *args):
    check(getattr(lib, name)(*args), name)


def attempt(name, *args):
    """call() for an entry point that may refuse the shape: False on EUNSUPPORTED (nothing ran: the caller takes its next kernel)."""
    rc = getattr(lib, name)(*args)
    if rc == EUNSUPPORTED:
        return False
    check(rc, name)
    return True
