"""ctypes binding of libscail_hip.so (include/scail_hip.h, include/scail_dit.h, include/scail_vae.h).  Fails loudly when the library is
missing -- there is deliberately no fallback path."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SCAIL_ABLATIONS=1 selects the measurement build that also holds the timing-ablation kernels (scail_amd/build.py)
LIB_PATH = os.path.join(_HERE, "libscail_hip_abl.so" if os.environ.get("SCAIL_ABLATIONS", "0") not in ("", "0") else "libscail_hip.so")

_p = C.c_void_p
_i64 = C.c_int64
_i = C.c_int
_f = C.c_float

# name -> argtypes; must list EVERY symbol declared in include/scail_hip.h (tests/test_abi.py
# cross-checks this table against the header).
SIGNATURES = {
    "scail_gemm_bf16": [_p, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, _i, _p, _i64, _p, _i64, _i64, _p],
    "scail_ln_modulate": [_p, _i64, _p, _i64, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _f, _p],
    "scail_layernorm_affine": [_p, _i64, _p, _i64, _p, _p, _i64, _i64, _f, _p],
    "scail_rmsnorm_rope": [_p, _i64, _p, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, _f, _p],
    "scail_rmsnorm_rope_scaled": [_p, _i64, _p, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, _f, _f, _p],
    "scail_rmsnorm_rope_slabs": [_p, _i64, _p, _i64, _i64, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, _f, _f, _p],
    "scail_row_kernel_name_for": [_i, _i64, _i64, _i64, _i64, _p, _i64, _p],
    "scail_slabs_to_rows": [_p, _i64, _i64, _p, _i64, _i64, _i64, _p],
    "scail_transpose_v": [_p, _i64, _i64, _p, _i64, _i64, _i64, _i64, _p],
    "scail_flash_attn_bf16": [_p, _i64, _i64, _p, _i64, _i64, _i64, _p, _i64, _i64, _p, _i64, _i64,
                              _i64, _i64, _i64, _i64, _i64, _f, _i, _p],
    "scail_flash_attn_kernel_for": [_i64, _i64, _i64, _i64, _i64, _i, _i],
    "scail_flash_attn_kernel_name_for": [_i64, _i64, _i64, _i64, _i64, _i64, _i64, _i, _i, _p, _i64, _p],
    "scail_flash_attn_vrows_bf16": [_p, _i64, _i64, _p, _i64, _i64, _p, _i64, _i64, _p, _i64, _i64, _i64, _i64, _i64, _i64, _f, _p],
    "scail_flash_attn_vrows_for": [_i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64],
    "scail_flash_attn_vrows_kernel_name_for": [_i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p, _i64, _p],
    "scail_flash_attn_rows_for": [_i64, _i64, _i64],
    "scail_flash_attn_count_restarts": [_p],
    "scail_comm_standin": [_p, _p, _i64, C.c_int32, _i64, _p],
    "scail_cross_attn2_kernel_for": [_i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64],
    "scail_cross_attn2_kernel_name_for": [_i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p, _i64, _p],
    "scail_gemm_kernel_for": [_i64, _i64, _i64, _i64, _i64, _i64, _i],
    "scail_gemm_kernel_name_for": [_i64, _i64, _i64, _i64, _i64, _i64, _i, _i, _p, _i64],
    "scail_conv3d_kernel_for": [_p, _i64, _i64, _i],
    "scail_conv3d_norm_fused_for": [_p, _i64],
    "scail_conv3d_kernel_name_for": [_p, _i64, _i64, _i, _p, _i64],
    "scail_cross_attn2_bf16": [_p, _i64, _i64, _p, _i64, _i64, _p, _i64, _i64, _p, _i64, _i64, _p, _i64, _i64, _p, _i64, _i64,
                               _i64, _i64, _i64, _f, _p],
    "scail_timestep_embedding": [_p, _p, _i64, _i64, _p],
    "scail_small_linear": [_p, _p, _p, _p, _i64, _i64, _i64, _i, _i, _p],
    "scail_adaln_table": [_p, _p, _p, _i64, _i64, _i64, _p],
    "scail_patchify": [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p],
    "scail_patchify_chars": [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p],
    "scail_unpatchify": [_p, _p, _i64, _i64, _i64, _i64, _p],
    "scail_cfg_euler": [_p, _p, _i64, _f, _f, _p],
    # the guidance plan's fp32 passes: v_c - v_u stored, and the Euler update around a stored delta (NULL: no guidance)
    "scail_cfg_delta_store": [_p, _p, _i64, _p],
    "scail_cfg_euler_delta": [_p, _p, _p, _i64, _f, _f, _p],
    # the solver plan's fp32 pass: CFG + one multistep update (x, v, hist, n, cfg, sigma, a, b, c, use_prev)
    "scail_cfg_multistep": [_p, _p, _p, _i64, _f, _f, _f, _f, _f, _i, _p],
    "scail_tile_gather": [_p, _p, _p, _i64, _i64, _i64, _p],
    "scail_tile_blend_acc": [_p, _p, _p, _p, _i64, _i64, _i64, _f, _p],
    "scail_tile_finish": [_p, _p, _p, _i64, _i64, _f, _p],
    "scail_tile_finish_multistep": [_p, _p, _p, _p, _i64, _i64, _f, _f, _f, _f, _i, _p],
    "scail_conv3d_cl": [_p, _p, _p, _p, _i64, _p, _i64, _p, _p],
    "scail_conv3d_cl_norm": [_p, _p, _p, _p, _i64, _p, _p, _p],
    "scail_conv3d_cl_resid_norm": [_p, _p, _p, _p, _p, _i64, _p, _i64, _p, _p, _p],
    "scail_rms_silu": [_p, _p, _p, _i64, _i64, _i, _p],
    "scail_softmax_rows": [_p, _i64, _i64, _i64, _f, _p],
    "scail_transpose2d": [_p, _i64, _i64, _p, _i64, _i64, _i64, _i64, _i64, _p],
    "scail_to_channels_last": [_p, _p, _p, _p, _i64, _i64, _i64, _p],
    "scail_from_channels_last": [_p, _i64, _p, _p, _p, _i64, _i64, _f, _f, _p],
    "scail_to_channels_last_frames": [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _p],
    "scail_from_channels_last_frames": [_p, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, _f, _f, _p],
    "scail_frames_u8": [_p, _i64, _p, _i64, _i64, _i64, _i64, _i64, _p],
    "scail_attn_small": [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _f, _p, _p, _p, _i64, _p],
    "scail_mul_bf16": [_p, _p, _p, _i64, _p],
    "scail_row_affine": [_p, _p, _p, _p, _i64, _i64, _i64, _p],
    "scail_set_option": [C.c_char_p, _i],
    "scail_release_caches": [],
    "scail_f32_to_bf16": [_p, _p, _i64, _p],
    "scail_bf16_to_f32": [_p, _p, _i64, _p],
    "scail_quant_fp8_rows": [_p, _i64, _p, _i64, _p, _i64, _i64, _p],
    "scail_gemm_fp8": [_p, _i64, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i, _p, _i64, _p, _i64, _i64, _p],
    "scail_rel_err_rows": [_p, _i64, _p, _i64, _p, _i64, _i64, _p],
    # the row kernels of the step cache
    "scail_resid_store": [_p, _i64, _p, _i64, _p, _i64, _i64, _i64, _p],
    "scail_resid_apply": [_p, _i64, _p, _p, _i64, _i64, _i64, _i64, _p],
    "scail_abs_diff_sums": [_p, _p, _i64, _p, _p],
    # MX block scaling: E8M0 bytes [rows, cols / 32] beside the e4m3 codes
    "scail_quant_mxfp8_rows": [_p, _i64, _p, _i64, _p, _i64, _i64, _i64, _p],
    "scail_gemm_mxfp8": [_p, _i64, _p, _i64, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i, _p, _i64, _p, _i64, _i64, _p],
    # MXFP6: packed e2m3 codes [rows, 3 cols / 4 bytes] + E8M0 bytes; leading dimensions of packed matrices in bytes
    "scail_quant_mxfp6_rows": [_p, _i64, _p, _i64, _p, _i64, _i64, _i64, _p],
    "scail_gemm_mxfp6": [_p, _i64, _p, _i64, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i, _p, _i64, _p, _i64, _i64, _p],
    # LoRA adapters: the in-place merge of up @ down, or of a full difference, into a bf16 weight window (scail_amd/lora.py)
    "scail_lora_merge_bf16": [_p, _i64, _i64, _i64, _p, _i64, _p, _i64, _i64, _f, _p],
    "scail_add_scaled_bf16": [_p, _i64, _i64, _i64, _p, _i64, _f, _p],
    "scail_resize_crop_aa": [_p, _i, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p],
    "scail_pose_half": [_p, _p, _i64, _i64, _p, _i64, _i64, _i64, _i64, _p],
    # include/scail_dit.h (structs are passed by pointer; scail_amd/cstep.py builds them)
    "scail_dit_create": [_p, _p, _p],
    "scail_dit_destroy": [_p],
    "scail_dit_workspace_bytes": [_p, _i64, _i64, _i64, _i64],
    "scail_dit_step": [_p, _p, _p, _p, _p, _i64, _p, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, C.c_uint32, _p, _i64, _p],
    # the *_chars forms take n_char (and the pose tensor's frame count) -- include/scail_dit.h "more than one character"
    "scail_dit_chars_workspace_bytes": [_p, _i64, _i64, _i64, _i64, _i64],
    "scail_dit_step_chars": [_p, _p, _p, _p, _p, _i64, _p, _i64, _i64, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, C.c_uint32, _p, _i64, _p],
    "scail_dit_sp_chars_workspace_bytes": [_p, C.c_int32, C.c_int32, _i64, _i64, _i64, _i64, _i64],
    "scail_dit_step_sp_chars": [_p, _p, _p, _p, _p, _i64, _p, _i64, _i64, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, _p, C.c_uint32, _p, _i64, _p],
    "scail_dit_sample_chars_workspace_bytes": [_p, _i64, _i64, _i64, _i64],
    "scail_dit_sample_chars": [_p, _p, _p, _p, _i64, _f, _p, _p, _p, _i64, _i64, _p, _p, _i64, _i64, _i64, _p, _i64, _p],
    "scail_dit_profile": [_p, _i],
    "scail_dit_profile_read": [_p, _i, _p, _p],
    "scail_dit_block_workspace_bytes": [_p, _i64, _i64],
    "scail_dit_block": [_p, _i64, _p, _p, _p, _p, _p, _i64, _i64, _p, _i64, _p],
    "scail_dit_sp_workspace_bytes": [_p, C.c_int32, C.c_int32, _i64, _i64, _i64, _i64],
    "scail_dit_step_sp": [_p, _p, _p, _p, _p, _i64, _p, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, _p, C.c_uint32, _p, _i64, _p],
    "scail_dit_block_sp_workspace_bytes": [_p, C.c_int32, C.c_int32, _i64, _i64],
    "scail_dit_block_sp": [_p, _i64, _p, _p, _p, _p, _p, _i64, _i64, _p, _p, _i64, _p],
    "scail_dit_sample_workspace_bytes": [_p, _i64, _i64, _i64],
    "scail_dit_sample": [_p, _p, _p, _p, _i64, _f, _p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _i64, _p],
    # temporal tiling (RFSamplerLong): host arrays tile_frames / tile_w / inv_wsum after the pose tiles
    "scail_dit_sample_tiled_workspace_bytes": [_p, _i64, _i64, _i64, _i64],
    "scail_dit_sample_tiled": [_p, _p, _p, _p, _i64, _f, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _i64, _i64, _p, _i64, _p],
    "scail_dit_fp8_weight_bytes": [_p, C.c_uint32],
    "scail_dit_enable_fp8": [_p, C.c_uint32, _p, _i64, _p],
    # the same two with the scaling (FP8_SCALINGS) named
    "scail_dit_fp8_weight_bytes_scaled": [_p, C.c_uint32, _i],
    "scail_dit_enable_fp8_scaled": [_p, C.c_uint32, _i, _p, _i64, _p],
    # the 6-bit form (packed e2m3 + E8M0): its own pair of entries, not a third FP8_SCALINGS value
    "scail_dit_fp6_weight_bytes": [_p, C.c_uint32],
    "scail_dit_enable_fp6": [_p, C.c_uint32, _p, _i64, _p],
    # per-layer fp8 selection (host uint32 masks [num_layers]) and the on-device GEMM error probe (device fp64 table [layers][6][4])
    "scail_dit_fp8_select_layers": [_p, _p],
    "scail_dit_fp8_probe_bytes": [_p, _i64, _i64],
    "scail_dit_fp8_probe": [_p, _p, _p, _i64],
    # the step cache: the _chars step / sampler + (mode | host uint8 reuse mask), cache, cache bytes; the time-embedding distances
    "scail_dit_step_cache_bytes": [_p, _i64, _i64, _i64, _i64],
    "scail_dit_step_cached": [_p, _p, _p, _p, _p, _i64, _p, _i64, _i64, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, C.c_uint32, _p, _i64,
                              _i, _p, _i64, _p],
    "scail_dit_sample_cached": [_p, _p, _p, _p, _i64, _f, _p, _p, _p, _i64, _i64, _p, _p, _i64, _i64, _i64, _p, _i64, _p, _p, _i64, _p],
    # the tiled sampler with one residual slab per tile: scail_dit_sample_tiled's arguments up to the workspace + (reuse, cache, cache bytes)
    "scail_dit_sample_tiled_cache_bytes": [_p, _i64, _i64, _i64, _i64],
    "scail_dit_sample_tiled_cached": [_p, _p, _p, _p, _i64, _f, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _i64, _i64, _p, _i64,
                                      _p, _p, _i64, _p],
    # the guidance plan: one branch of the pair (cond, cond_batch, elem; mode, cache, cache bytes) and the sampler loop with a plan
    # (host uint8 guide, delta, delta bytes, host uint8 reuse or NULL, cache, cache bytes)
    "scail_dit_step_branch": [_p, _p, _p, _p, _i64, _i64, _p, _p, _i64, _i64, _p, _p, _p, _i64, _i64, _i64, _p, _i64, _i, _p, _i64, _p],
    "scail_dit_guidance_bytes": [_i64, _i64, _i64],
    "scail_dit_sample_guided": [_p, _p, _p, _p, _i64, _f, _p, _p, _p, _i64, _i64, _p, _p, _i64, _i64, _i64, _p, _i64, _p, _p, _i64,
                                _p, _p, _i64, _p],
    # the solver plan: the sampler loops with a coefficient table (host fp32 sigma, host fp32 coef [n][3], hist, hist bytes)
    "scail_dit_solver_bytes": [_i64, _i64, _i64],
    "scail_dit_sample_solver": [_p, _p, _p, _p, _i64, _f, _p, _p, _p, _i64, _i64, _p, _p, _i64, _i64, _i64, _p, _i64, _p, _p, _p, _i64, _p],
    "scail_dit_sample_tiled_solver": [_p, _p, _p, _p, _i64, _f, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _i64, _i64, _p, _i64,
                                      _p, _p, _p, _i64, _p],
    "scail_dit_time_distances_bytes": [_p, _i],
    "scail_dit_time_distances": [_p, _p, _i64, _i, _p, _p, _i64, _p],
    # include/scail_vae.h (scail_amd/cvae.py builds the structs)
    "scail_vae_create": [_p, _p],
    "scail_vae_destroy": [_p],
    "scail_vae_set_trace": [_p, _p, _p],
    "scail_vae_workspace_bytes": [_p, _i64, _i64, _i64],
    "scail_vae_encode": [_p, _p, _p, _i64, _i64, _i64, _p, _i64, _p],
    "scail_vae_decode": [_p, _p, _p, _i64, _i64, _i64, _p, _i64, _p],
    "scail_vae_decode_stream_workspace_bytes": [_p, _i64, _i64, _i64],
    "scail_vae_decode_stream": [_p, _p, _p, _i64, _i64, _i64, _i64, _p, _i64, _p],
    "scail_vae_decode_u8": [_p, _p, _p, _i64, _i64, _i64, _p, _i64, _p],
    "scail_vae_decode_stream_u8": [_p, _p, _p, _i64, _i64, _i64, _i64, _p, _i64, _p],
}
# return types other than the int status: every *_bytes query answers an int64_t, the destroy functions nothing
RESTYPES = {"scail_dit_destroy": None, "scail_vae_destroy": None, "scail_dit_fp8_weight_bytes_scaled": _i64,
            **{n: _i64 for n in SIGNATURES if n.endswith("_bytes")}}

# include/scail_hip_ablation.h: only libscail_hip_abl.so (SCAIL_ABLATIONS=1) exports these
ABLATION_SIGNATURES = {
    "scail_tune_set": [C.c_char_p, _i],
    "scail_debug_cycles": [C.c_void_p, _i],
}
ABLATIONS = LIB_PATH.endswith("_abl.so")

EPI_BIAS, EPI_GELU_TANH, EPI_GELU_ERF, EPI_RESID = 0, 1, 2, 3
ACT_NONE, ACT_SILU, ACT_GELU_TANH = 0, 1, 2
# include/scail_hip.h SCAIL_ROW_*: the call scail_row_kernel_name_for is asked about
ROW_LN_MODULATE, ROW_LN_AFFINE, ROW_RMSNORM, ROW_RMSNORM_ROPE, ROW_COPY = 0, 1, 2, 3, 4
# include/scail_dit.h SCAIL_DIT_FP8_*: the per-token GEMMs of a block that scail_dit_enable_fp8 switches to fp8
FP8_GEMMS = {"qkv": 1, "o": 2, "cq": 4, "co": 8, "w1": 16, "w2": 32}
FP8_ALL = 63
# include/scail_dit.h SCAIL_DIT_FP8_SCALE_*: one fp32 scale per row, or OCP MX (one E8M0 scale per block of 32 along K)
FP8_SCALINGS = {"row": 0, "mx": 1}
# DiffusionTransformer(gemm_precision=...): what the selected per-token GEMMs run in ("fp6": scail_dit_enable_fp6, OCP MXFP6 e2m3)
GEMM_PRECISIONS = ("fp8", "fp6")
# include/scail_dit.h SCAIL_DIT_CACHE_*: the modes of scail_dit_step_cached; the signals of scail_dit_time_distances
CACHE_MODES = {"fill": 1, "reuse": 2}
CACHE_SIGNALS = {"time": 0, "modulation": 1}
# include/scail_dit.h SCAIL_DIT_GUIDE_*: the entries of a guidance plan (scail_dit_sample_guided)
GUIDE_PAIR, GUIDE_DELTA, GUIDE_COND = 0, 1, 2
# include/scail_hip.h scail_resize_crop_aa: source layouts, and the largest in / out per axis its tap budget covers
SRC_U8_NHWC, SRC_F32_NCHW = 0, 1
RESIZE_MAX_SCALE = 16
ABI_VERSION = 8          # (the streamed VAE decode only adds entry points -- scail_vae_decode_stream, its workspace query, scail_to / from_channels_last_frames --
                         # and no existing call changed: still 8; load() fails on a library that lacks them; likewise the request
                         # preprocessing, scail_resize_crop_aa / scail_pose_half, and the convolution queries scail_conv3d_norm_fused_for /
                         # scail_conv3d_kernel_name_for, the GEMM query scail_gemm_kernel_name_for, the uint8 output route,
                         # scail_frames_u8 / scail_vae_decode_u8 / scail_vae_decode_stream_u8, and the row-kernel query
                         # scail_row_kernel_name_for, the attention queries scail_flash_attn_kernel_name_for /
                         # scail_cross_attn2_kernel_name_for, and the fp8 probe and per-layer selection, scail_rel_err_rows /
                         # scail_dit_fp8_select_layers / scail_dit_fp8_probe / scail_dit_fp8_probe_bytes, and MX block scaling,
                         # scail_quant_mxfp8_rows / scail_gemm_mxfp8 / scail_dit_fp8_weight_bytes_scaled / scail_dit_enable_fp8_scaled,
                         # and the step cache, scail_resid_store / scail_resid_apply / scail_abs_diff_sums / scail_dit_step_cache_bytes /
                         # scail_dit_step_cached / scail_dit_sample_cached / scail_dit_time_distances / scail_dit_time_distances_bytes,
                         # and the 6-bit GEMMs, scail_quant_mxfp6_rows / scail_gemm_mxfp6 / scail_dit_fp6_weight_bytes / scail_dit_enable_fp6,
                         # and the tiled step cache, scail_dit_sample_tiled_cache_bytes / scail_dit_sample_tiled_cached,
                         # and the guidance plan, scail_cfg_delta_store / scail_cfg_euler_delta / scail_dit_step_branch /
                         # scail_dit_guidance_bytes / scail_dit_sample_guided,
                         # and the solver plan, scail_cfg_multistep / scail_tile_finish_multistep / scail_dit_solver_bytes /
                         # scail_dit_sample_solver / scail_dit_sample_tiled_solver,
                         # and the LoRA merge, scail_lora_merge_bf16 / scail_add_scaled_bf16)
                         # 8 = temporal tiling (scail_tile_gather / _blend_acc / _finish, scail_dit_sample_tiled);
                         # 7 = the character count in the network-level calls (scail_patchify_chars, scail_dit_*_chars);
                         # 6 = the fp8 GEMM path (scail_quant_fp8_rows, scail_gemm_fp8, scail_dit_fp8_weight_bytes, scail_dit_enable_fp8);
                         # 5 = scail_rmsnorm_rope_slabs takes a slab row stride; the sequence-parallel exchange is ONE collective per direction
                         # (send / recv layouts of scail_dit.h), exchange-wait / restart categories of scail_dit_profile_read;
                         # 4 = `flags` argument of scail_dit_step / scail_dit_step_sp (SCAIL_DIT_CFG_PAIR), options "attn4_rows" / "attn4_xcd";
                         # include/scail_hip.h scail_abi_version: 2 = negative SCAIL_ATTN_Q_PRESCALED sentinel + the SP executor entry points;
                         # 3 = scail_vae_set_trace, options "row_wave" / "conv_direct", scail_conv3d_kernel_for = 4 for the kt = 1 / narrow / fused-norm shapes

_lib = None


class ScailHipError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load the HIP library (once).  Raises if it has not been built (``python -m scail_amd.build``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ScailHipError(
            f"{LIB_PATH} not found: build it with `python -m scail_amd.build` (hipcc, gfx950). "
            "scail_amd has no CPU/torch fallback.")
    lib = C.CDLL(LIB_PATH)
    lib.scail_last_error.restype = C.c_char_p
    lib.scail_last_error.argtypes = []
    lib.scail_abi_version.restype = C.c_int
    lib.scail_abi_version.argtypes = []
    if lib.scail_abi_version() != ABI_VERSION:
        raise ScailHipError(f"ABI mismatch: library {lib.scail_abi_version()} vs binding {ABI_VERSION}")
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)     # AttributeError if the symbol is missing: loud by design
        fn.argtypes = args
        fn.restype = RESTYPES.get(name, C.c_int)
    if ABLATIONS:
        for name, args in ABLATION_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = C.c_int
        for env, knob in (("SCAIL_ATTN_VARIANT", b"attn_variant"), ("SCAIL_GEMM_TILE", b"gemm_tile")):   # A/B overrides for measurement runs
            if os.environ.get(env):
                lib.scail_tune_set(knob, int(os.environ[env]))
    _lib = lib
    return lib


def call(name: str, *args) -> None:
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise ScailHipError(f"{name} failed ({rc}): {lib.scail_last_error().decode()}")


def set_option(name: str, value: int) -> None:
    """Runtime option of the product library (include/scail_hip.h scail_set_option: "attn4", "attn4_thr")."""
    call("scail_set_option", name.encode(), int(value))


def tune_set(knob: str, value: int) -> None:
    """Schedule A/B knobs and timing ablations: measurement build only (SCAIL_ABLATIONS=1, include/scail_hip_ablation.h)."""
    if not ABLATIONS:
        raise ScailHipError(f"tune_set({knob!r}): kernel variants exist only in the measurement build; run with SCAIL_ABLATIONS=1 "
                            "after `SCAIL_ABLATIONS=1 python -m scail_amd.build`")
    call("scail_tune_set", knob.encode(), int(value))
