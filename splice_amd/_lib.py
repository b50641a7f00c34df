"""ctypes binding of libsplice_hip.so (the C ABI of include/splice_hip.h).

The product path has NO CPU fallback: if the HIP library is missing or a call fails,
a RuntimeError is raised.  Build it with ``python -c "import __graft_entry__ as g; g.build()"``
or ``make -C splice_amd/csrc``.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsplice_hip.so")

_lib = None


class GemmEpilogue(C.Structure):
    _fields_ = [
        ("bias", C.c_void_p), ("resid", C.c_void_p), ("ldr", C.c_int), ("resid_mod", C.c_int),
        ("out_f32", C.c_void_p), ("ldo", C.c_int),
        ("out_bf", C.c_void_p), ("ldbf", C.c_int),
        ("out_bf_t", C.c_void_p), ("ldt", C.c_int),
        ("out_pre", C.c_void_p), ("ldp", C.c_int), ("pre_row_lo", C.c_int),
        ("aux", C.c_void_p), ("ldaux", C.c_int),
        ("out_f32_cols", C.c_void_p), ("ld_cols", C.c_int), ("col_lo", C.c_int), ("col_hi", C.c_int),
        ("alpha", C.c_float), ("ksplit", C.c_int), ("slab_stride", C.c_longlong),
        ("rd_other", C.c_void_p), ("ld_rd", C.c_int), ("rd_rows", C.c_int), ("rowdot", C.c_void_p),
        ("row_scale", C.c_void_p), ("col_scale", C.c_void_p),
        ("out_f8", C.c_void_p), ("ld8", C.c_int),
        ("out_f8_t", C.c_void_p), ("ldt8", C.c_int),
    ]


class GenArch(C.Structure):
    _fields_ = [("n_scales", C.c_int), ("in_channels", C.c_int), ("out_channels", C.c_int),
                ("down", C.c_int * 6), ("up", C.c_int * 6), ("skip", C.c_int * 6),
                ("filter_down", C.c_int * 6), ("filter_up", C.c_int * 6), ("filter_skip", C.c_int), ("reflect", C.c_int)]


class StepConfig(C.Structure):
    _fields_ = [
        ("crop_h", C.c_int), ("crop_w", C.c_int), ("vit_h", C.c_int), ("vit_w", C.c_int),
        ("ent_h", C.c_int), ("ent_w", C.c_int), ("ent_vit_h", C.c_int), ("ent_vit_w", C.c_int),
        ("lambda_global_cls", C.c_float), ("lambda_global_ssim", C.c_float), ("lambda_global_identity", C.c_float),
        ("lambda_entire_cls", C.c_float), ("lambda_entire_ssim", C.c_float),
        ("entire_every", C.c_int), ("cls_warmup", C.c_int),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("pairs", C.c_int), ("arena_stride", C.c_longlong), ("fp8_selfsim", C.c_int), ("top_cls_only", C.c_int), ("n_crops", C.c_int), ("n_crops_b", C.c_int),
    ]


class StopState(C.Structure):   # splice_stop_state
    _fields_ = [("sum", C.c_float), ("count", C.c_int), ("windows", C.c_int), ("best", C.c_float), ("bad", C.c_int), ("stop_step", C.c_int)]


class ClipState(C.Structure):   # splice_clip_state
    _fields_ = [("sumsq", C.c_float), ("norm", C.c_float), ("coef", C.c_float), ("skip", C.c_int), ("clipped", C.c_int), ("skipped", C.c_int)]


class ClipAutoState(C.Structure):   # splice_clip_auto_state
    _fields_ = [("ref", C.c_float * 2), ("count", C.c_int * 2), ("thr", C.c_float), ("regime", C.c_int)]


class BestState(C.Structure):   # splice_best_state
    _fields_ = [("best_step", C.c_int), ("best_window", C.c_int)]


class LrState(C.Structure):   # splice_lr_state
    _fields_ = [("scale", C.c_float), ("bad", C.c_int), ("cuts", C.c_int), ("last_cut_step", C.c_int)]


class OptimExt(C.Structure):   # splice_optim_ext
    _fields_ = [("weight_decay", C.c_float), ("momentum", C.c_float), ("dampening", C.c_float), ("nesterov", C.c_int), ("decoupled", C.c_int),
                ("amsgrad", C.c_int), ("centered", C.c_int)]


def optim_ext(options):
    """The ``splice_optim_ext`` record of ``options`` (a dict of its field names, ``util.fused_optimizer_ext``; an absent field is neutral)."""
    if isinstance(options, OptimExt):
        return options
    return OptimExt(float(options.get("weight_decay", 0.0)), float(options.get("momentum", 0.0)), float(options.get("dampening", 0.0)),
                    int(bool(options.get("nesterov", False))), int(bool(options.get("decoupled", False))), int(bool(options.get("amsgrad", False))),
                    int(bool(options.get("centered", False))))


class GenConvArgs(C.Structure):   # splice_gen_conv_args (test hooks)
    _fields_ = [("in", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p)] + \
               [(n, C.c_size_t) for n in ("in_nstride", "in_cstride", "out_nstride", "out_cstride", "w_jstride", "w_cstride", "p_nstride")] + \
               [(n, C.c_int) for n in ("N", "Cin", "Hi", "Wi", "Cout", "Ho", "Wo", "ks", "stride", "pad", "reflect", "act", "transposed", "accumulate")] + \
               [("ws", C.c_void_p), ("ws_floats", C.c_size_t), ("p_group", C.c_int), ("defer_reduce", C.c_int)]


class GenWgradArgs(C.Structure):   # splice_gen_wgrad_args (test hooks)
    _fields_ = [("x", C.c_void_p), ("dy", C.c_void_p), ("ws", C.c_void_p), ("ws_floats", C.c_size_t)] + \
               [(n, C.c_size_t) for n in ("x_nstride", "x_cstride", "dy_nstride", "dy_cstride")] + \
               [(n, C.c_int) for n in ("N", "Cin", "Hi", "Wi", "Cout", "Ho", "Wo", "ks", "stride", "pad", "reflect")]


class GenBnArgs(C.Structure):   # splice_gen_bn_args (test hooks)
    _fields_ = [("y", C.c_void_p), ("out", C.c_void_p), ("y_nstride", C.c_size_t), ("out_nstride", C.c_size_t),
                ("N", C.c_int), ("C", C.c_int), ("HW", C.c_int), ("batch", C.c_int),
                ("gamma", C.c_void_p), ("beta", C.c_void_p), ("eps", C.c_float), ("slope", C.c_float), ("p_nstride", C.c_size_t),
                ("part", C.c_void_p), ("part_floats", C.c_size_t), ("mean", C.c_void_p), ("rstd", C.c_void_p),
                ("up_src", C.c_void_p), ("up_d_src", C.c_void_p), ("up_src_ns", C.c_size_t), ("up_d_src_ns", C.c_size_t),
                ("up_c0", C.c_int), ("up_h", C.c_int), ("up_w", C.c_int), ("up_Ho", C.c_int), ("up_Wo", C.c_int),
                ("slabs", C.c_void_p), ("bias", C.c_void_p), ("ksplit", C.c_int),
                ("da", C.c_void_p), ("dy", C.c_void_p), ("da_nstride", C.c_size_t), ("dy_nstride", C.c_size_t),
                ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("accumulate", C.c_int),
                ("da_slabs", C.c_void_p), ("da_ksplit", C.c_int), ("da_accumulate", C.c_int),
                ("pre_y", C.c_void_p), ("pre_y_ns", C.c_size_t), ("pre_slabs", C.c_void_p), ("pre_bias", C.c_void_p),
                ("pre_ksplit", C.c_int), ("pre_C", C.c_int), ("pre_gamma", C.c_void_p), ("pre_beta", C.c_void_p),
                ("pre_mean", C.c_void_p), ("pre_rstd", C.c_void_p), ("pre_slope", C.c_float),
                ("pre_dy", C.c_void_p), ("pre_dgamma", C.c_void_p), ("pre_dbeta", C.c_void_p)]


GEN_CONV_FORM_INTS, GEN_WGRAD_FORM_INTS, GEN_BN_FORM_INTS = 5, 6, 7   # SPLICE_GEN_*_FORM_INTS

STOP_HISTORY = 64   # SPLICE_STOP_HISTORY

EPI_BIAS, EPI_RESID, EPI_OUT_F32, EPI_OUT_BF, EPI_OUT_T = 1, 2, 4, 8, 16
EPI_GELU, EPI_GELU_GRAD, EPI_COLS_F32, EPI_ALPHA, EPI_ROWDOT, EPI_SCALE_RC, EPI_OUT_F8, EPI_OUT_F8T = 32, 64, 128, 256, 512, 1024, 2048, 4096

_vp, _i, _f, _sz, _u = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_uint

_SIGNATURES = {
    "splice_version": ([], C.c_int),
    "splice_dev_switches": ([], C.c_int),
    "splice_last_error": ([], C.c_char_p),
    "splice_gemm_nt_bf16": ([_u, _vp, _i, _vp, _i, _i, _i, _i, C.POINTER(GemmEpilogue), _vp], _i),
    "splice_gemm_nt_fp8": ([_u, _vp, _i, _vp, _i, _i, _i, _i, C.POINTER(GemmEpilogue), _vp], _i),
    "splice_quantize_rows_fp8": ([_vp, _i, _vp, _i, _vp, _i, _i, _vp], _i),
    "splice_gemm_splitk_slabs": ([_i, _i], _i),
    "splice_gemm_force_tile": ([_i], _i),
    "splice_attention_variant": ([_i], _i),
    "splice_attention_qfold": ([_i], _i),
    "splice_attention_bwd_variant": ([_i], _i),
    "splice_layernorm_fwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp], _i),
    "splice_layernorm_bwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp], _i),
    "splice_attention_fwd": ([_vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp], _i),
    "splice_attention_fwd_fp8": ([_vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp], _i),
    "splice_attention_bwd": ([_vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i),
    "splice_attention_probs": ([_vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp], _i),
    "splice_augment_structure": ([_vp, _vp, _vp, _i, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_float), _f, _vp], _i),
    "splice_keys_selfsim_ws_bytes": ([_i, _i], _sz),
    "splice_keys_selfsim_fwd": ([_vp, _i, _i, _i, _f, _vp, _vp, _vp], _i),
    "splice_keys_selfsim_bwd": ([_vp, _vp, _i, _i, _f, _vp, _i, _i, _vp, _vp], _i),
    "splice_mse": ([_vp, _i, _vp, _i, _i, _i, _f, _vp, _vp, _i, _vp], _i),
    # test hooks: the fused step's loss-stage launchers
    "splice_selfsim_loss_pairs_ws_bytes": ([_i, _i, _i], _sz),
    "splice_selfsim_loss_pairs": ([_vp, _vp, _i, _sz, _vp, _i, _sz, _i, _i, _i, _f, _vp, _i, _f, _vp, _sz, _vp, _i, _sz, _vp, _vp], _i),
    "splice_mse_pairs": ([_vp, _i, _sz, _vp, _i, _sz, _i, _i, _f, _f, _vp, _sz, _vp, _i, _sz, _i, _vp, _vp], _i),
    "splice_total_loss_pairs": ([_vp, _sz, _i, _f, _f, _f, _f, _f, _vp, _i, _i, _i, _i, _i, _vp, _i, _i, _vp], _i),
    # test hooks: the [CLS]-tail launchers of the top ViT block
    "splice_attn_cls_fwd": ([_vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp], _i),
    "splice_attn_cls_bwd": ([_vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp, _vp, _i, _sz, _vp, _vp], _i),
    "splice_ln_rows_fwd": ([_vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _i, _i, _f, _vp, _i, _sz, _vp, _vp, _sz, _vp], _i),
    "splice_ln_rows_bwd": ([_vp, _sz, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _i, _i, _i, _sz, _vp], _i),
    "splice_rows_finish": ([_i, _vp, _i, _sz, _i, _i, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _sz, _i, _vp], _i),
    # test hooks: generator launchers on caller-owned buffers
    "splice_gen_conv": ([C.POINTER(GenConvArgs), C.POINTER(_i), _vp], _i),
    "splice_gen_conv_pair": ([C.POINTER(GenConvArgs), C.POINTER(GenConvArgs), C.POINTER(_i), _vp], _i),
    "splice_gen_conv_reflect_dgrad": ([C.POINTER(GenConvArgs), _vp, _sz, _vp], _i),
    "splice_gen_conv_wgrad_ws_floats": ([_i, _i, _i, _i, _i, _i], _sz),
    "splice_gen_conv_wgrad": ([C.POINTER(GenWgradArgs), _vp, _i, _i, _sz, C.POINTER(_i), _vp], _i),
    "splice_gen_wgrad_reduce": ([_vp, _i, _i, _vp, _i, _i, _sz, _vp], _i),
    "splice_gen_bn_small_instance": ([_i], _i),
    "splice_gen_bn_form": ([_i, _i, _sz, _i, C.POINTER(_i)], _i),
    "splice_gen_bn_part_floats": ([_i, _i], _sz),
    "splice_gen_bn_fwd": ([C.POINTER(GenBnArgs), _vp], _i),
    "splice_gen_bn_bwd": ([C.POINTER(GenBnArgs), _vp], _i),
    "splice_gen_upsample2x_fwd": ([_vp, _sz, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp], _i),
    "splice_gen_upsample2x_bwd": ([_vp, _sz, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp], _i),
    "splice_gen_sigmoid_bias_part_floats": ([_i, _i], _sz),
    "splice_gen_sigmoid_bwd_bias": ([_vp, _vp, _vp, _i, _i, _i, _vp, _sz, _sz, _i, C.POINTER(_i), _vp], _i),
    "splice_patchify": ([_vp, _vp, _i, _i, _i, _i, _i, _i, _vp], _i),
    "splice_unpatchify": ([_vp, _vp, _i, _i, _i, _i, _i, _i, _vp], _i),
    "splice_cast_f32_bf16": ([_vp, _vp, _sz, _vp], _i),
    "splice_cast_bf16_f32": ([_vp, _vp, _sz, _vp], _i),
    "splice_transpose_f32_bf16": ([_vp, _vp, _i, _i, _i, _vp], _i),
    "splice_resize_bilinear_fwd": ([_vp, _vp, _i, _i, _i, _i, _i, _vp], _i),
    "splice_resize_bilinear_bwd": ([_vp, _vp, _i, _i, _i, _i, _i, _vp], _i),
    # ViT engine
    "splice_vit_create": ([_i, _i, _i, _i, C.POINTER(_vp)], _i),
    "splice_vit_destroy": ([_vp], None),
    "splice_vit_set_param": ([_vp, C.c_char_p, _vp, C.c_longlong, _vp], _i),
    "splice_vit_params_complete": ([_vp], _i),
    "splice_vit_enable_fp8": ([_vp, _vp], _i),
    "splice_vit_ctx_create": ([_vp, _i, _i, _i, _vp, _i, _vp, C.POINTER(_vp)], _i),
    "splice_vit_ctx_destroy": ([_vp], None),
    "splice_vit_ctx_info": ([_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)], _i),
    "splice_vit_ctx_set_top_cls_only": ([_vp, _i], _i),
    "splice_vit_ctx_set_transposed_layers": ([_vp, _i, _vp], _i),
    "splice_vit_ctx_set_cls_seeds": ([_vp, _vp, _i, _i], _i),
    "splice_vit_ctx_set_key_f32_layers": ([_vp, _i, _vp], _i),
    "splice_vit_ctx_set_fp8": ([_vp, _i], _i),
    "splice_vit_forward": ([_vp, _vp, _i, _vp], _i),
    "splice_vit_forward_ex": ([_vp, _vp, _i, _i, _vp], _i),
    "splice_vit_forward_passes": ([_vp, _vp, _i, _i, _i, _i, _vp], _i),
    "splice_vit_get_tensor": ([_vp, _i, _i, C.POINTER(_vp)], _i),
    "splice_vit_qscale": ([_vp], C.c_float),
    "splice_vit_read_tensor": ([_vp, _i, _i, _vp, _sz, _vp], _i),
    "splice_vit_backward": ([_vp, _i, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _vp, _i, _vp], _i),
    # generator engine
    "splice_gen_create": ([C.POINTER(_vp)], _i),
    "splice_gen_create_arch": ([C.POINTER(GenArch), C.POINTER(_vp)], _i),
    "splice_gen_destroy": ([_vp], None),
    "splice_gen_param_count": ([_vp], C.c_longlong),
    "splice_gen_num_tensors": ([_vp], _i),
    "splice_gen_tensor_info": ([_vp, _i, C.POINTER(C.c_char_p), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)], _i),
    "splice_gen_plan_create": ([_vp, _i, _i, _i, _i, C.POINTER(_vp)], _i),
    "splice_gen_plan_destroy": ([_vp], None),
    "splice_gen_forward": ([_vp, _vp, _vp, _vp, _vp], _i),
    "splice_gen_forward_borrowed": ([_vp, _vp, _vp, _vp, _vp], _i),
    "splice_gen_backward": ([_vp, _vp, _vp, _vp, _i, _vp], _i),
    "splice_adam_step": ([_vp, _vp, _vp, _vp, C.c_longlong, _f, _f, _f, _f, _i, _i, _vp], _i),
    "splice_optim_step": ([_i, _vp, _vp, _vp, _vp, C.c_longlong, _f, _f, _f, _f, _i, _i, _vp], _i),
    "splice_optim_step_ex": ([_i, _vp, _vp, _vp, _vp, _vp, C.c_longlong, _f, _vp, _f, _f, _f, _i, _i, _vp], _i),
    "splice_optim_step_pairs": ([_i, _vp, _vp, _vp, _vp, _vp, _i, C.c_longlong, C.c_longlong, _vp, _f, _f, _f, _i, _i, _vp], _i),
    # weight average
    "splice_optim_step_ema": ([_i, _vp, _vp, _vp, _vp, _vp, _vp, C.c_longlong, _f, _vp, _f, _f, _f, _i, _i, _f, _i, _vp], _i),
    "splice_optim_step_pairs_ema": ([_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.c_longlong, C.c_longlong, _vp, _f, _f, _f, _vp, _vp, _i, _f, _i, _vp], _i),
    "splice_step_set_ema": ([_vp, _vp, _f, _i], _i),
    # gradient clipping by the pair's global norm
    "splice_grad_norm_pairs": ([_vp, _vp, _i, C.c_longlong, C.c_longlong, _f, _vp, _vp, _vp, _vp, _vp], _i),
    "splice_optim_step_pairs_clip": ([_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.c_longlong, C.c_longlong, _vp, _f, _f, _f, _vp, _vp, _i, _f, _i, _vp, _vp], _i),
    "splice_optim_step_clip": ([_i, _vp, _vp, _vp, _vp, _vp, _vp, C.c_longlong, _f, _vp, _f, _f, _f, _i, _i, _f, _i, _vp, _vp], _i),
    "splice_step_set_grad_clip": ([_vp, _f, _vp], _i),
    # ... and against the pair's own running norm
    "splice_grad_norm_pairs_auto": ([_vp, _vp, _i, C.c_longlong, C.c_longlong, _f, _f, _f, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp], _i),
    "splice_step_set_grad_clip_auto": ([_vp, _f, _f, _f, _i, _vp, _vp], _i),
    # keep the best window's weights under the stop rule
    "splice_plateau_update_best": ([_vp, _vp, _vp, _vp, _i, _i, _f, _i, _i, _i, _i, _vp], _i),
    "splice_optim_step_pairs_best": ([_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.c_longlong, C.c_longlong, _vp, _f, _f, _f, _vp, _vp, _i, _f, _i, _vp, _vp, _vp, _vp, _vp], _i),
    "splice_step_set_keep_best": ([_vp, _vp, _vp, _vp, _vp], _i),
    # per-step loss trace
    "splice_step_set_loss_trace": ([_vp, _vp, _i], _i),
    "splice_total_loss_pairs_trace": ([_vp, _sz, _i, _f, _f, _f, _f, _f, _vp, _i, _i, _i, _i, _i, _vp, _i, _i, _vp, _i, _f, _i, _i, _vp, _vp, _i, _vp], _i),
    # plateau lr rule
    "splice_step_set_lr_plateau": ([_vp, _f, _i, _f, _vp, _vp], _i),
    "splice_plateau_update_lr": ([_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _f, _i, _i, _f, _i, _f, _i, _i, _vp], _i),
    # extended optimiser rules (weight decay, momentum, AdamW, amsgrad, centred RMSprop)
    "splice_optim_step_ext": ([_i, _vp, _vp, _vp, _vp, _vp, _vp, C.c_longlong, _f, _vp, _f, _f, _f, _i, _i, C.POINTER(OptimExt), _vp], _i),
    "splice_optim_step_pairs_ext": ([_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.c_longlong, C.c_longlong, _vp, _f, _f, _f, _i, _vp, _vp, _i, _f, _i, _vp, _vp,
                                     _vp, _vp, C.POINTER(OptimExt), _vp], _i),
    "splice_step_set_optimizer_ext": ([_vp, C.POINTER(OptimExt), _vp], _i),
    # image-space loss terms (total variation of x', pixel identity of y')
    "splice_step_set_image_terms": ([_vp, _f, _f], _i),
    "splice_step_set_ssim_layers": ([_vp, _i, _vp, _vp], _i),
    "splice_step_ssim_layer_values": ([_vp, _i, _vp, _vp], _i),
    "splice_selfsim_loss_layers": ([_i, _vp, _vp, _vp, _vp, _i, _sz, _i, _sz, _i, _i, _i, _f, _vp, _f, _vp, _sz, _vp, _i, _sz, _vp, _vp], _i),
    # the [CLS] appearance terms over several ViT blocks
    "splice_step_set_cls_layers": ([_vp, _i, _vp, _vp], _i),
    "splice_step_cls_layer_values": ([_vp, _i, _vp, _i], _i),
    "splice_cls_loss_layers": ([_i, _vp, _vp, _vp, _sz, _sz, _i, _i, _f, _vp, _vp, _sz, _vp, _sz, _vp, _vp], _i),
    # the key-identity term over several ViT blocks
    "splice_step_set_id_layers": ([_vp, _i, _vp, _vp], _i),
    "splice_step_id_layer_values": ([_vp, _vp, _i], _i),
    "splice_id_loss_layers": ([_i, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _i, _i, _i, _f, _vp, _vp, _i, _sz, _vp, _sz, _vp, _vp, _sz, _i, _vp], _i),
    # the key second-moment appearance term
    "splice_step_set_key_gram": ([_vp, _f, _i], _i),
    "splice_step_key_gram_values": ([_vp, _vp], _i),
    "splice_key_gram_pairs": ([_vp, _i, _sz, _vp, _i, _sz, _vp, _i, _sz, _i, _i, _i, _f, _vp, _vp, _sz, _vp, _vp, _i, _sz, _vp], _i),
    # ... over several blocks, and centred
    # the nearest-neighbour key appearance term
    "splice_step_set_key_nn": ([_vp, _f, _i], _i),
    "splice_step_key_nn_values": ([_vp, _vp], _i),
    "splice_step_key_nn_match": ([_vp, _vp, _vp], _i),
    "splice_key_nn_ws_bytes": ([_i, _i, _i], _sz),
    "splice_key_nn_pairs": ([_vp, _vp, _i, _sz, _sz, _i, _i, _i, _f, _f, _vp, _vp, _vp, _sz, _vp, _vp, _i, _sz, _vp, _vp], _i),
    "splice_step_set_key_gram_layers": ([_vp, _f, _i, _vp, _vp, _i], _i),
    "splice_step_key_gram_layer_values": ([_vp, _vp], _i),
    "splice_key_gram_layers_pairs": ([_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _sz, _i, _sz, _i, _sz, _i, _i, _i, _i, _sz, _vp, _vp, _vp, _i, _sz, _vp], _i),
    "splice_image_terms_value": ([_vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _sz, _i, _vp], _i),
    "splice_image_terms_grad_add": ([_vp, _vp, _vp, _i, _i, _i, _f, _vp], _i),
    "splice_total_loss_pairs_img": ([_vp, _sz, _i, _f, _f, _f, _f, _f, _vp, _i, _i, _i, _i, _i, _vp, _i, _i, _f, _f, _vp], _i),
    "splice_prof_begin": ([_i], _i),
    "splice_prof_end": ([C.POINTER(_f), C.POINTER(_i)], _i),
    "splice_prof_end_ex": ([C.POINTER(_f), C.POINTER(_i), C.POINTER(_i)], _i),
    "splice_prof_end_detail": ([C.POINTER(_f), C.POINTER(_i), C.POINTER(_i), C.c_char_p, _i], _i),
    "splice_prof_active": ([], _i),
    "splice_step_use_graph": ([_vp, _i], _i),
    "splice_step_graph_stats": ([_vp, C.POINTER(C.c_longlong)], _i),
    "splice_step_use_overlap": ([_vp, _i], _i),
    "splice_vit_ctx_dims": ([_vp] + [C.POINTER(_i)] * 7, _i),
    "splice_gen_plan_dims": ([_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_longlong)], _i),
    # fused step
    "splice_step_create": ([C.POINTER(StepConfig), _vp, _vp, _vp, _vp, _vp, C.POINTER(_vp)], _i),
    "splice_step_destroy": ([_vp], None),
    "splice_step_run": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp], _i),
    "splice_step_output": ([_vp, _i, C.POINTER(_vp)], _i),
    "splice_step_set_crops": ([_vp, _i, _i, _i, _i], _i),
    "splice_step_set_running_stats": ([_vp, _vp, C.c_longlong], _i),
    "splice_step_set_mode": ([_vp, _i, _i], _i),
    "splice_step_set_optimizer": ([_vp, _i, _f, _f, _f], _i),
    "splice_step_set_lr": ([_vp, _f], _i),
    "splice_step_set_pair_weights": ([_vp, _vp], _i),
    "splice_step_set_pair_lr": ([_vp, _vp], _i),
    "splice_step_set_phases": ([_vp, _i, _vp], _i),
    # plateau stop rule
    "splice_step_set_stop_rule": ([_vp, _i, _f, _i, _i], _i),
    "splice_step_stop_state": ([_vp, _vp, _vp], _i),
    "splice_plateau_update": ([_vp, _vp, _i, _i, _f, _i, _i, _i, _i, _vp], _i),
    # pair snapshots: start a handle at step k, stage the live pairs out of the caller's larger batches
    "splice_step_restore": ([_vp, _i, _vp, _vp], _i),
    "splice_step_set_input_rows": ([_vp, _i, _vp], _i),
    "splice_gen_buffer_count": ([_vp], C.c_longlong),
    "splice_gen_num_buffers": ([_vp], _i),
    "splice_gen_buffer_info": ([_vp, _i, C.POINTER(C.c_char_p), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)], _i),
    "splice_gen_running_stats_update": ([C.POINTER(_vp), _i, _vp, C.c_longlong, _f, _vp], _i),
    "splice_gen_plan_resize": ([_vp, _i, _i], _i),
    "splice_gen_plan_set_arena_stride": ([_vp, C.c_longlong], _i),
    "splice_gen_plan_set_batch_stats": ([_vp, _i], _i),
    "splice_gen_plan_set_groups": ([_vp, _i], _i),
}


def exported_symbols():
    """Names include/splice_hip.h declares (checked against the .so by the CPU tests)."""
    return sorted(_SIGNATURES)


def register(name, argtypes, restype):
    _SIGNATURES[name] = (argtypes, restype)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP extension is not built "
                "(run __graft_entry__.build() or `make -C splice_amd/csrc`). There is no CPU fallback.")
        _lib = C.CDLL(LIB_PATH)
        for name, (argtypes, restype) in _SIGNATURES.items():
            fn = getattr(_lib, name)
            fn.argtypes = argtypes
            fn.restype = restype
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().splice_last_error().decode(errors="replace")
        raise RuntimeError(f"libsplice_hip {what} failed (rc={rc}): {msg}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def current_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
