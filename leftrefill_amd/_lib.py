"""ctypes binding of libleftrefill_hip.so (the C ABI declared in include/leftrefill_hip.h).

The product path has NO fallback: if the shared library is missing or a symbol is absent this module raises, and every
op raises RuntimeError on a non-zero return code.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# LEFTREFILL_LIB_PATH: developer override (same-box A/B of two builds of the library)
LIB_PATH = os.environ.get("LEFTREFILL_LIB_PATH") or os.path.join(HERE, "lib", "libleftrefill_hip.so")
ABI_VERSION = 30

c_void_p, c_int, c_float, c_int64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64


class GemmArgs(ctypes.Structure):
    """struct lr_gemm_args (include/leftrefill_hip.h)."""
    _fields_ = [
        ("p1", c_void_p), ("C1", ctypes.c_int32),
        ("p2", c_void_p), ("C2", ctypes.c_int32),
        ("B", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
        ("Hs", ctypes.c_int32), ("Ws", ctypes.c_int32),
        ("taps", ctypes.c_int32), ("stride", ctypes.c_int32), ("up", ctypes.c_int32),
        ("asym", ctypes.c_int32),
        ("wt", c_void_p), ("N", ctypes.c_int32),
        ("bias", c_void_p),
        ("rowvec", c_void_p), ("ld_rowvec", ctypes.c_int32),
        ("resid", c_void_p), ("ld_resid", ctypes.c_int32),
        ("out", c_void_p), ("ld_out", ctypes.c_int32),
        ("geglu", ctypes.c_int32),
        ("tile_n", ctypes.c_int32),
        ("tile_m", ctypes.c_int32),
        ("splits", ctypes.c_int32),
        ("workspace", c_void_p), ("workspace_bytes", ctypes.c_int64),
        ("ln_stats", c_void_p), ("ln_parts", ctypes.c_int32), ("ln_eps", ctypes.c_float),
        ("ln_colsum", c_void_p),
        ("stats_out", c_void_p),
        ("gn_stats_out", c_void_p),
        ("dtype", ctypes.c_int32),
        ("pipe", ctypes.c_int32),
        ("gn_group_out", c_void_p), ("gn_hw", ctypes.c_int32),
        ("wt_bstride", ctypes.c_int32), ("bias_bstride", ctypes.c_int32),
        ("wt_pm", ctypes.c_int32),
        ("skip1", c_void_p), ("skip2", c_void_p), ("Cs1", ctypes.c_int32), ("Cs2", ctypes.c_int32),
        ("splitk_mode", ctypes.c_int32),
    ]


class AttnBwdArgs(ctypes.Structure):
    """struct lr_attn_bwd_args (include/leftrefill_hip.h)."""
    _fields_ = ([(n, c_void_p) for n in ("q", "k", "v", "o", "dout", "qt", "kt", "dot", "lse", "dsum", "dq", "dk", "dv")] +
                [(n, ctypes.c_int32) for n in ("ldq", "ldk", "ldv", "ldo", "lddo", "ld_qt", "ld_kt", "lddq", "lddk", "lddv",
                                               "B", "heads", "Nq", "Nkv")] + [("scale", ctypes.c_float)])


class XattnArgs(ctypes.Structure):
    """struct lr_xattn_args (include/leftrefill_hip.h)."""
    _fields_ = [("x", c_void_p), ("out", c_void_p), ("wq", c_void_p), ("bq", c_void_p), ("k", c_void_p), ("ldk", ctypes.c_int32),
                ("vt", c_void_p), ("wo", c_void_p), ("bo", c_void_p), ("stats_out", c_void_p),
                ("M", ctypes.c_int32), ("HW", ctypes.c_int32), ("C", ctypes.c_int32), ("heads", ctypes.c_int32),
                ("Lc", ctypes.c_int32), ("ln_eps", ctypes.c_float), ("scale", ctypes.c_float),
                ("pre_a", c_void_p), ("pre_w", c_void_p), ("pre_b", c_void_p)]


class RowCopyJob(ctypes.Structure):
    """struct lr_row_copy_job (include/leftrefill_hip.h)."""
    _fields_ = [("src", c_void_p), ("src_pitch", ctypes.c_int64), ("src_off", ctypes.c_int64),
                ("dst", c_void_p), ("dst_pitch", ctypes.c_int64), ("dst_off", ctypes.c_int64),
                ("row_bytes", ctypes.c_int32), ("n_rows", ctypes.c_int32), ("src_idx", c_void_p), ("dst_idx", c_void_p)]


class StinArgs(ctypes.Structure):
    """struct lr_stin_args (include/leftrefill_hip.h)."""
    _fields_ = [("x", c_void_p), ("wp", c_void_p), ("bp", c_void_p), ("wqkv", c_void_p), ("bqkv", c_void_p), ("x1", c_void_p),
                ("qkv", c_void_p), ("M", ctypes.c_int32), ("C", ctypes.c_int32), ("NQ", ctypes.c_int32), ("ld_qkv", ctypes.c_int32),
                ("ln_eps", ctypes.c_float), ("gn_part", c_void_p), ("gn_gamma", c_void_p), ("gn_beta", c_void_p),
                ("gn_chunks", ctypes.c_int32), ("gn_hw", ctypes.c_int32), ("gn_eps", ctypes.c_float)]


class RowlinArgs(ctypes.Structure):
    """struct lr_rowlin_args (include/leftrefill_hip.h)."""
    _fields_ = [("x", c_void_p), ("w", c_void_p), ("bias", c_void_p), ("out", c_void_p), ("M", ctypes.c_int32), ("C", ctypes.c_int32),
                ("N", ctypes.c_int32), ("ld_out", ctypes.c_int32), ("geglu", ctypes.c_int32), ("ln_eps", ctypes.c_float), ("ln", ctypes.c_int32),
                ("gn_part", c_void_p), ("gn_gamma", c_void_p), ("gn_beta", c_void_p), ("gn_chunks", ctypes.c_int32), ("gn_hw", ctypes.c_int32),
                ("gn_eps", ctypes.c_float)]


class FfnArgs(ctypes.Structure):
    """struct lr_ffn_args (include/leftrefill_hip.h)."""
    _fields_ = [("x", c_void_p), ("out", c_void_p), ("w1", c_void_p), ("b1", c_void_p), ("w2", c_void_p), ("b2", c_void_p),
                ("stats_out", c_void_p), ("M", ctypes.c_int32), ("C", ctypes.c_int32), ("H", ctypes.c_int32), ("ln_eps", ctypes.c_float),
                ("post_w", c_void_p), ("post_b", c_void_p), ("post_resid", c_void_p), ("gn_stats_out", c_void_p),
                ("gn_group_out", c_void_p), ("gn_hw", ctypes.c_int32)]


class LpipsArgs(ctypes.Structure):
    """struct lr_lpips_args (include/leftrefill_hip.h)."""
    _fields_ = [("pred", c_void_p), ("pred_kind", ctypes.c_int32), ("origin", c_void_p), ("mask", c_void_p)] + \
               [(n, ctypes.c_int32) for n in ("N", "H", "W", "x0", "Wc", "r")] + \
               [("wt", c_void_p * 5), ("bias", c_void_p * 5), ("lin", c_void_p * 5),
                ("workspace", c_void_p), ("workspace_bytes", ctypes.c_int64), ("out", c_void_p)]


class PrepJob(ctypes.Structure):
    """struct lr_prep_job (include/leftrefill_hip.h); leftrefill_amd.dataprep.JOB_DTYPE is its numpy image."""
    _fields_ = [("img_off", c_int64), ("mask_off", c_int64 * 2)] + \
               [(n, ctypes.c_int32) for n in ("img_h", "img_w", "rh", "rw", "y0", "x0")] + \
               [("mask_h", ctypes.c_int32 * 2), ("mask_w", ctypes.c_int32 * 2)] + \
               [(n, ctypes.c_int32) for n in ("outpaint_col", "flags", "sample", "tile")]


class NvsJob(ctypes.Structure):
    """struct lr_nvs_job (include/leftrefill_hip.h); leftrefill_amd.nvsprep.JOB_DTYPE is its numpy image."""
    _fields_ = [("cond_off", c_int64), ("target_off", c_int64), ("plane_off", c_int64)] + \
               [(n, ctypes.c_int32) for n in ("cond_h", "cond_w", "target_h", "target_w", "mode", "k", "flags", "sample")] + \
               [("lo", ctypes.c_uint8 * 32), ("hi", ctypes.c_uint8 * 32)]


class PilJob(ctypes.Structure):
    """struct lr_pil_job (include/leftrefill_hip.h); leftrefill_amd.refill.JOB_DTYPE is its numpy image."""
    _fields_ = [(n, c_int64) for n in ("src_off", "tmp_off", "dst_off", "h_off", "v_off")] + \
               [(n, ctypes.c_int32) for n in ("hs", "ws", "hd", "wd", "c", "h_ksize", "v_ksize", "reserved")]


class LoraDrop(ctypes.Structure):
    """struct lr_lora_drop (include/leftrefill_hip.h)."""
    _fields_ = [("seed", ctypes.c_uint64), ("stream", ctypes.c_uint32), ("draw", ctypes.c_uint32), ("threshold", ctypes.c_uint32),
                ("inv_keep", ctypes.c_float), ("colgrp", c_void_p)]


class GridSource(ctypes.Structure):
    """struct lr_grid_source (include/leftrefill_hip.h)."""
    _fields_ = [("ptr", c_void_p)] + [(n, ctypes.c_int32) for n in ("kind", "C", "W", "col")] + \
               [(n, c_int64) for n in ("stride_n", "stride_c", "stride_h", "stride_w")]


class OptimTensor(ctypes.Structure):
    """struct lr_optim_tensor (include/leftrefill_hip.h)."""
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p), ("numel", ctypes.c_int64),
                ("grad_kind", ctypes.c_int32), ("group", ctypes.c_int32)]


class OptimGroup(ctypes.Structure):
    """struct lr_optim_group (include/leftrefill_hip.h)."""
    _fields_ = [("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double), ("weight_decay", ctypes.c_double),
                ("lr_table", c_void_p), ("lr_len", ctypes.c_int32), ("reserved", ctypes.c_int32)]


# struct of include/leftrefill_hip.h -> its mirror above (tests/test_abi_cpu.py holds every field's name, offset and size to the header)
STRUCTS = {"lr_gemm_args": GemmArgs, "lr_attn_bwd_args": AttnBwdArgs, "lr_xattn_args": XattnArgs, "lr_row_copy_job": RowCopyJob,
           "lr_stin_args": StinArgs, "lr_rowlin_args": RowlinArgs, "lr_ffn_args": FfnArgs, "lr_lpips_args": LpipsArgs,
           "lr_prep_job": PrepJob, "lr_nvs_job": NvsJob, "lr_pil_job": PilJob, "lr_lora_drop": LoraDrop, "lr_grid_source": GridSource,
           "lr_optim_tensor": OptimTensor, "lr_optim_group": OptimGroup}

# symbol -> argtypes; every function returns int
SIGNATURES = {
    "lr_abi_version": [],
    "lr_nchw_f32_to_nhwc_f16": [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "lr_nhwc_f16_to_nchw": [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "lr_groupnorm_stats": [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p],
    "lr_groupnorm_apply": [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_float,
                           c_int, c_void_p, c_void_p],
    "lr_layernorm_bwd": [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int, c_int, c_void_p],
    "lr_groupnorm_bwd": [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_float,
                         c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "lr_layernorm_bwd_res": [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int, c_int, c_void_p],
    "lr_groupnorm_bwd_res": [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p,
                             c_void_p, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "lr_mv_gather_bwd": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "lr_mv_scatter_bwd": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "lr_geglu_fwd": [c_void_p, c_void_p, c_int, c_int, c_void_p],
    "lr_geglu_bwd": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "lr_sumpool2x2": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "lr_softmax_rows_f16": [c_void_p, c_void_p, c_int, c_int, c_float, c_void_p],
    "lr_layernorm": [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int, c_int, c_void_p],
    "lr_timestep_embedding": [c_void_p, c_int, c_int, c_void_p, c_void_p],
    "lr_linear_small_m": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                          c_void_p],
    "lr_gemm_workspace_bytes": [ctypes.POINTER(GemmArgs)],
    "lr_gemm_stats_parts": [ctypes.POINTER(GemmArgs)],
    "lr_gemm_gn_rows": [ctypes.POINTER(GemmArgs)],
    "lr_gemm_gn_group_chunks": [ctypes.POINTER(GemmArgs)],
    "lr_gn_conv_out_f16": [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_float, c_void_p, c_int, c_void_p,
                           c_int, c_void_p, c_void_p],
    "lr_groupnorm_finalize": [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    "lr_groupnorm_apply_n": [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_float,
                             c_int, c_void_p, c_void_p],
    "lr_gemm_plan": [ctypes.POINTER(GemmArgs), ctypes.POINTER(ctypes.c_int32)],
    "lr_gemm_conv_f16": [ctypes.POINTER(GemmArgs), c_void_p],
    "lr_attention_f16": [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                         c_int, c_float, c_void_p],
    "lr_attention_vt_f16": [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                         c_int, c_float, c_void_p],
    "lr_attention_causal_f16": [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_float,
                                c_void_p],
    "lr_attention_lse_f16": [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int,
                             c_int, c_float, c_void_p],
    "lr_attention_bwd_f16": [ctypes.POINTER(AttnBwdArgs), c_void_p],
    "lr_attention_causal_lse_f16": [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int,
                                    c_float, c_void_p],
    "lr_attention_causal_bwd_f16": [ctypes.POINTER(AttnBwdArgs), c_void_p],
    "lr_gelu_fwd_f16": [c_void_p, c_void_p, c_int64, c_void_p],
    "lr_gelu_bwd_f16": [c_void_p, c_void_p, c_void_p, c_int64, c_void_p],
    "lr_transpose_v_f16": [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "lr_xattn_block_f16": [ctypes.POINTER(XattnArgs), c_void_p],
    "lr_xattn_pack_vt_f16": [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p],
    "lr_ffn_block_f16": [ctypes.POINTER(FfnArgs), c_void_p],
    "lr_stin_block_f16": [ctypes.POINTER(StinArgs), c_void_p],
    "lr_rowlin_f16": [ctypes.POINTER(RowlinArgs), c_void_p],
    "lr_mv_gather": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "lr_row_copy": [c_void_p, c_int, c_void_p],
    "lr_gemm_splitk_timeouts": [],
    "lr_mv_scatter": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "lr_ddim_cfg_step": [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float,
                         c_float, c_float, c_void_p],
    "lr_timestep_embedding_f32": [c_void_p, c_int, c_int, c_void_p, c_void_p],
    "lr_plms_cfg_step": [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_int64,
                         c_float, c_float, c_float, c_float, c_void_p],
    "lr_dpmpp_cfg_step": [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float,
                          c_float, c_float, c_float, c_void_p],
    "lr_ddim_inv_cfg_step": [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_float, c_float, c_float, c_void_p],
    "lr_ddim_cfg3_step": [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float,
                          c_float, c_float, c_float, c_void_p],
    "lr_ddpm_step": [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p,
                     c_int64, c_float, c_float, c_float, c_float, c_float, c_float, c_float, c_void_p],
    "lr_ddim_q_sample": [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_void_p],
    # added under ABI 30 (one new symbol; a library built before it fails the getattr in load())
    "lr_eval_metrics": [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                        c_void_p],
    # added under ABI 30 as well: the sync-free AMP AdamW tail (csrc/optim.hip)
    "lr_amp_adamw_step": [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_float, c_float, c_int,
                          ctypes.POINTER(c_int), c_void_p],
    # added under ABI 30 as well: LPIPS(alex) on the device (csrc/lpips.hip)
    "lr_lpips_workspace_bytes": [c_int, c_int, c_int, c_int],
    "lr_lpips_alex": [ctypes.POINTER(LpipsArgs), c_void_p],
    # added under ABI 30 as well: batch assembly from raw decoded images (csrc/batch_prep.hip)
    "lr_batch_prep": [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    # added under ABI 30 as well: NVS batch assembly from raw RGBA renders (csrc/nvs_prep.hip)
    "lr_nvs_prep": [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    # added under ABI 30 as well: Pillow's resampler and the one-call inpainting canvas (csrc/pil_resample.hip)
    "lr_pil_resize": [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int,
                      c_void_p],
    "lr_refill_canvas": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    # added under ABI 30 as well: the training logger's image grid and token drift (csrc/image_grid.hip)
    "lr_image_grid": [ctypes.POINTER(GridSource), c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p],
    "lr_token_drift": [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p],
    # added under ABI 30 as well: the attention-map probe behind return_attn (csrc/attention_probe.hip)
    "lr_attention_probe_f16": [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_float,
                               c_float, c_float, c_void_p],
    # added under ABI 30 as well: LoRA factor products, factor gradients and the fp32 merge (csrc/lora.hip)
    "lr_lora_down_f16": [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p],
    "lr_lora_up_f16": [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "lr_lora_wgrad_workspace_bytes": [c_int, c_int, c_int],
    "lr_lora_wgrad_f16": [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_int64, c_void_p],
    "lr_lora_merge_f32": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p],
    # added under ABI 30 as well: the three LoRA products with the dropout mask regenerated in the kernel (csrc/lora.hip)
    "lr_lora_down_drop_f16": [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_float, ctypes.POINTER(LoraDrop),
                              c_void_p],
    "lr_lora_up_drop_f16": [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(LoraDrop),
                            c_void_p],
    "lr_lora_wgrad_drop_f16": [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_int64,
                               ctypes.POINTER(LoraDrop), c_void_p],
    # added under ABI 30 as well: FID features and float64 statistics on the device (csrc/inception.hip); no struct: scalars, pointers
    # and the int32 program in host memory
    "lr_fid_input": [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, ctypes.POINTER(c_int), c_void_p],
    "lr_fid_run": [c_void_p, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, ctypes.POINTER(c_int), c_void_p],
    "lr_fid_head": [c_void_p, c_int, c_int, c_int, c_int, c_void_p, ctypes.POINTER(c_int), c_void_p],
    "lr_fid_accumulate": [c_void_p, c_int, c_int, c_void_p, c_void_p, ctypes.POINTER(c_int), c_void_p],
    # added under ABI 30 as well: seeded sampling noise (csrc/seeded_noise.hip); fp32 only, no bf16 twin.  A library built before it
    # fails the getattr in load() like every other additive entry: rebuild
    "lr_seeded_normal": [c_void_p, c_int, c_int64, ctypes.c_int32, ctypes.c_int32, c_void_p, c_void_p],
}
INT64_RETURNS = ("lr_gemm_workspace_bytes", "lr_lpips_workspace_bytes", "lr_lora_wgrad_workspace_bytes")

# bfloat16 twins (include/leftrefill_hip.h, last section): same argument lists as the fp16 entry points
BF16_TWINS = ["lr_groupnorm_stats", "lr_groupnorm_apply", "lr_groupnorm_apply_n", "lr_layernorm", "lr_layernorm_bwd",
              "lr_groupnorm_bwd", "lr_layernorm_bwd_res", "lr_groupnorm_bwd_res", "lr_nchw_f32_to_nhwc_f16", "lr_nhwc_f16_to_nchw", "lr_timestep_embedding", "lr_linear_small_m",
              "lr_mv_gather", "lr_mv_scatter", "lr_ddim_cfg_step", "lr_timestep_embedding_f32", "lr_plms_cfg_step",
              "lr_dpmpp_cfg_step", "lr_ddim_inv_cfg_step", "lr_ddim_cfg3_step", "lr_ddpm_step", "lr_geglu_fwd", "lr_geglu_bwd", "lr_sumpool2x2",
              "lr_mv_gather_bwd", "lr_mv_scatter_bwd", "lr_attention_f16", "lr_attention_causal_f16", "lr_attention_lse_f16",
              "lr_attention_vt_f16", "lr_transpose_v_f16", "lr_attention_bwd_f16", "lr_xattn_block_f16",
              "lr_xattn_pack_vt_f16", "lr_ffn_block_f16", "lr_stin_block_f16", "lr_rowlin_f16", "lr_gn_conv_out_f16",
              "lr_attention_causal_lse_f16", "lr_attention_causal_bwd_f16", "lr_gelu_fwd_f16", "lr_gelu_bwd_f16",
              "lr_attention_probe_f16", "lr_lora_down_f16", "lr_lora_up_f16", "lr_lora_wgrad_f16",
              "lr_lora_down_drop_f16", "lr_lora_up_drop_f16", "lr_lora_wgrad_drop_f16"]


def twin(name):
    """fp16 entry point -> its bfloat16 twin."""
    return (name[:-4] if name.endswith("_f16") else name) + "_bf16"


for _n in BF16_TWINS:
    SIGNATURES[twin(_n)] = SIGNATURES[_n]

# entry points of developer builds only (-DLR_DEV_VARIANTS, include/leftrefill_hip.h last section): bound when present
_FOLD_SIG = [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]
DEV_SIGNATURES = {"lr_dev_set": [ctypes.c_char_p, c_int], "lr_dev_unset": [ctypes.c_char_p],
                  "lr_gn_fold_weights_f16": _FOLD_SIG, "lr_gn_fold_weights_bf16": _FOLD_SIG}

_lib = None


def fn(lib, name, dtype):
    """The entry point `name` for 16-bit element type `dtype` (torch.float16 | torch.bfloat16)."""
    import torch
    if dtype == torch.bfloat16:
        return getattr(lib, twin(name))
    assert dtype == torch.float16, dtype
    return getattr(lib, name)


def load():
    """Load the shared library once; raises if it is missing (no CPU / eager fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch must be imported first: PyTorch-ROCm ships its own HIP runtime (torch/lib/libamdhip64.so) and owns the
    # streams we launch on; loading our library afterwards binds its libamdhip64 dependency to that same runtime.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -m leftrefill_amd.build` (hipcc --offload-arch=gfx950). "
            "leftrefill_amd has no fallback path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export what the header declares
        fn.argtypes = argtypes
        fn.restype = c_int64 if name in INT64_RETURNS else c_int
    v = lib.lr_abi_version()
    if v != ABI_VERSION:
        raise RuntimeError(f"libleftrefill_hip.so ABI {v} != binding ABI {ABI_VERSION}; rebuild")
    for name, argtypes in DEV_SIGNATURES.items():
        if hasattr(lib, name):
            f_ = getattr(lib, name)
            f_.argtypes, f_.restype = argtypes, c_int
    _lib = lib
    if dev_variants():      # developer library: its knobs come from the LR_* environment variables of the tools/ A/B scripts
        for k, val in os.environ.items():
            if k.startswith("LR_") and val.lstrip("-").isdigit():
                lib.lr_dev_set(k.encode(), int(val))
    return lib


def dev_variants():
    """True when the loaded library is a developer build (tools/build_variant.sh: -DLR_DEV_VARIANTS) -- the only kind that has knobs."""
    return hasattr(load(), "lr_dev_set")


def dev_set(name, value):
    """Set (int) or clear (None) a developer knob of a developer build; the product library has none (RuntimeError)."""
    lib = load()
    if not hasattr(lib, "lr_dev_set"):
        raise RuntimeError(f"{name}: developer knobs exist only in a -DLR_DEV_VARIANTS build (tools/build_variant.sh)")
    if value is None:
        lib.lr_dev_unset(name.encode())
    else:
        lib.lr_dev_set(name.encode(), int(value))


def check(rc, what):
    if rc != 0:
        kind = {-1: "bad argument", -2: "alignment", -3: "unsupported"}.get(rc, f"hipError {rc}")
        raise RuntimeError(f"{what} failed: {kind} (rc={rc})")
