/*
 * scail_hip.h -- C ABI of libscail_hip.so, the MI355X (gfx950) implementation of the SCAIL
 * video-DiT sampling hot path.
 *
 * The reference (zai-org/SCAIL) has no C/FFI boundary: its plugin seam is Python (config-named
 * classes + SAT mixin hooks).  This header is the boundary a maintainer
 * binds instead of the torch calls the reference makes at those seams; every entry point cites
 * the reference code it replaces (paths relative to the reference root).  INTEGRATION.md shows
 * the ctypes binding and where each call plugs into the reference's hooks.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless stated otherwise;
 *   - caller owns every buffer; nothing is retained after the call returns (no handles yet);
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); no host sync inside;
 *   - activations / weights are bf16 (uint16 storage), row-major, weights in torch Linear
 *     layout [out, in] (sat/mpu/layers.py:208-210); small per-channel vectors are fp32;
 *   - every function returns 0 on success, non-zero on error; scail_last_error() returns the
 *     message of the calling thread's last error (reference convention: Python exceptions /
 *     asserts, e.g. dit_video_crossattn_sc_xc.py:1456 -- the binding raises RuntimeError).
 */
#ifndef SCAIL_HIP_H
#define SCAIL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint16_t scail_bf16;

const char* scail_last_error(void);
/* ABI version of this header; bumped on any signature OR semantic change of an existing entry point (2: SCAIL_ATTN_Q_PRESCALED became a
 * negative sentinel and `scale` must be positive; the sequence-parallel executor entry points of scail_dit.h.  3: scail_vae_set_trace,
 * options "row_wave" / "conv_direct", scail_conv3d_kernel_for = 4 for the kt = 1 / narrow / fused-norm shapes.  4: `flags` of
 * scail_dit_step / _sp.  5: scail_rmsnorm_rope_slabs takes the slab row stride; scail_dit.h's sequence-parallel send / recv layouts carry
 * q | k | v (k | v) in one message per peer; scail_dit_profile_read categories for the exchange waits and the attention restarts);
 * 6: the fp8 GEMM path (scail_quant_fp8_rows, scail_gemm_fp8, scail_dit_fp8_weight_bytes, scail_dit_enable_fp8).  7: the character count
 * in the network-level calls (scail_patchify_chars, scail_dit_*_chars).  8: temporal tiling (scail_tile_gather / _blend_acc / _finish,
 * scail_dit_sample_tiled).  (The streamed VAE decode -- scail_vae_decode_stream, its workspace query, scail_to / from_channels_last_frames --
 * only ADDS entry points: still 8; a binding that meets a library without them fails on the missing symbol.  The same holds for the
 * request preprocessing, scail_resize_crop_aa and scail_pose_half, for the convolution queries scail_conv3d_norm_fused_for and
 * scail_conv3d_kernel_name_for, for the GEMM query scail_gemm_kernel_name_for, for the uint8 output route, scail_frames_u8 and
 * scail_vae_decode_u8 / scail_vae_decode_stream_u8, for the row-kernel query scail_row_kernel_name_for, for the attention queries
 * scail_flash_attn_kernel_name_for / scail_cross_attn2_kernel_name_for, and for the fp8 probe, scail_rel_err_rows and scail_dit.h's scail_dit_fp8_select_layers /
 * scail_dit_fp8_probe / scail_dit_fp8_probe_bytes, and for MX block scaling of the fp8 GEMMs, scail_quant_mxfp8_rows / scail_gemm_mxfp8 and
 * scail_dit.h's scail_dit_fp8_weight_bytes_scaled / scail_dit_enable_fp8_scaled, and for the step cache, scail_resid_store /
 * scail_resid_apply / scail_abs_diff_sums and scail_dit.h's scail_dit_step_cache_bytes / scail_dit_step_cached / scail_dit_sample_cached /
 * scail_dit_time_distances / scail_dit_time_distances_bytes, and for the 6-bit GEMMs, scail_quant_mxfp6_rows / scail_gemm_mxfp6 and
 * scail_dit.h's scail_dit_fp6_weight_bytes / scail_dit_enable_fp6, and for the guidance plan, scail_cfg_delta_store / scail_cfg_euler_delta
 * and scail_dit.h's scail_dit_step_branch / scail_dit_guidance_bytes / scail_dit_sample_guided, and for the solver plan,
 * scail_cfg_multistep / scail_tile_finish_multistep and scail_dit.h's scail_dit_solver_bytes / scail_dit_sample_solver /
 * scail_dit_sample_tiled_solver, and for the LoRA merge, scail_lora_merge_bf16 / scail_add_scaled_bf16.) */
int scail_abi_version(void);

/* ---- epilogues of scail_gemm_bf16 ---------------------------------------------------------- */
enum {
    SCAIL_EPI_BIAS = 0,       /* y = x W^T + b                                                  */
    SCAIL_EPI_GELU_TANH = 1,  /* y = gelu_tanh(x W^T + b)   (MLP up-proj, text_embedding)         */
    SCAIL_EPI_GELU_ERF = 2,   /* y = gelu(x W^T + b)        (MLPProj, dit...:31-45)               */
    SCAIL_EPI_RESID = 3       /* y = resid + gate[b,:] * (x W^T + b); gate==NULL -> ungated        */
};

/*
 * y[M,N] = epilogue( x[M,K] . W[N,K]^T + bias[N] ),  bf16 in, fp32 accumulate on MFMA, bf16 out.
 * Replaces every F.linear on the per-token path: QKV / dense (sat/model/transformer.py:66-118,
 * dit...:1065-1101), cross query/dense (dit...:1116,1200), MLP (sat/transformer_defaults.py:163-176),
 * patch embedding as a per-patch linear (dit...:99-130), final linear (dit...:826).
 *   lda/ldr/ldc: row strides in elements.  K % 64 == 0, N % 8 == 0.  bias may be NULL.
 *   SCAIL_EPI_RESID: gate is fp32 [n_batch, gate_stride] indexed gate[(m / rows_per_batch) * gate_stride + n]
 *   (the AdaLN gate of dit...:1036,1050); resid may alias y.
 */
int scail_gemm_bf16(const scail_bf16* x, int64_t lda, const scail_bf16* w, const float* bias,
                    scail_bf16* y, int64_t ldc, int64_t M, int64_t N, int64_t K, int epilogue,
                    const scail_bf16* resid, int64_t ldr, const float* gate, int64_t gate_stride,
                    int64_t rows_per_batch, void* stream);

/*
 * Which kernel scail_gemm_bf16 runs for a shape: 4 = the hand-scheduled 4-wave kernels generated by scail_amd/asmgen/gemm4.py
 * (csrc/gemm4.s: 256 x 256 x 64 tile, one wave per SIMD, accumulators in the AGPR file, LDS-DMA staging two tiles deep; need
 * M >= 2048 (or M >= 512 with at least 128 tiles of 256 x 256) with M % 256 == 0 or >= 8, N % 256 == 0, K % 64 == 0, K >= 128, a bias / GELU-tanh / residual epilogue and 32-bit
 * byte offsets), 0 = the kernels of csrc/gemm.hip (ragged N, small M, GELU-erf; in the measurement build also whenever a tile is forced).  Host-only
 * query, a projection of the choice scail_gemm_bf16 follows (csrc/gemm.hip gemm_choose).  The first gemm4 launch for
 * a tile grid allocates its tile-order table: make it outside hipStreamBeginCapture.
 */
int scail_gemm_kernel_for(int64_t lda, int64_t ldc, int64_t ldr, int64_t M, int64_t N, int64_t K, int epilogue);
/* The kernel scail_gemm_bf16 would launch under the options in force, in words, into buf[len] (`gated`: the residual epilogue has a gate).  A
 * generated kernel's symbol ("scail_gemm4_e0", "_e1", "_e3" gated residual, "_e4" ungated), or a hipcc kernel's template name with its arguments
 * as csrc/gemm.hip instantiates it, the epilogue code among them: "gemm_bf16_kernel<128, 128, 2, 2, 0, false>" (the 128 tile: M < 2048 or
 * N < 1024), "gemm_bf16_q8_kernel<2>" (the quadrant-phase kernel: the big shapes the generated kernels refuse -- N % 256 != 0, an M tail of 1 to 7
 * rows, GELU-erf, option "gemm4" off) and "gemm_bf16_kernel<256, 256, 2, 4, 0, true>" (256 tile + LDS-DMA: big shapes whose row strides exceed
 * q8's 2 GB buffer descriptor).  In the measurement build a tile forced by the gemm_tile knob is named "gemm_tile <code>: <kernel>".
 * scail_gemm_kernel_for is the same answer reduced to generated (4) or not (0).  Tile counts and grids are not part of the name.  Host-only.
 * 0, or 1 + scail_last_error. */
int scail_gemm_kernel_name_for(int64_t lda, int64_t ldc, int64_t ldr, int64_t M, int64_t N, int64_t K, int epilogue, int gated,
                               char* buf, int64_t len);

/*
 * LayerNorm (no affine, eps) + AdaLN modulate:  y = LN(x) * (1 + scale[b]) + shift[b]
 * (sat/ops/layernorm.py:16-24 + modulate dit...:760-761, used at :1031-1032, :1045-1046, :825).
 * Output row r in [0, n_batch*rows_out) reads source row
 *   (r / rows_out) * src_rows_per_batch + src_row_offset + (r % rows_out)
 * so the final layer can normalise only the noise-token slice (dit...:771).
 * shift/scale: fp32, indexed [b * mod_stride + col].
 */
int scail_ln_modulate(const scail_bf16* x, int64_t ldx, scail_bf16* y, int64_t ldy,
                      const float* shift, const float* scale, int64_t mod_stride,
                      int64_t n_batch, int64_t rows_out, int64_t src_rows_per_batch,
                      int64_t src_row_offset, int64_t D, float eps, void* stream);

/* LayerNorm with affine weight/bias (post_cross_attention_layernorm, sat/model/transformer.py:409;
 * nn.LayerNorm in MLPProj dit...:36,40).  w, b fp32 [D]. */
int scail_layernorm_affine(const scail_bf16* x, int64_t ldx, scail_bf16* y, int64_t ldy,
                           const float* w, const float* b, int64_t rows, int64_t D, float eps,
                           void* stream);

/*
 * RMSNorm over the FULL hidden dim D (RMSNorm dit...:48-68 with hidden_size_head == D, yaml :72)
 * followed (optionally) by the interleaved-pair 3D RoPE of Rotary3DPositionEmbeddingMixin
 * (dit...:336-340, 556-557) with per-token cos/sin tables [L, head_dim/2] (fp32) built by the
 * host from the three segment rules (ref / noise / pose, dit...:525-645).
 *   x, y: [rows, D] with strides ldx / ldy (y may alias x); w fp32 [D];
 *   cos/sin == NULL -> no rotation (cross-attention q/k, dit...:1131-1142).
 *   token index for the tables = row % rows_per_batch.
 */
int scail_rmsnorm_rope(const scail_bf16* x, int64_t ldx, scail_bf16* y, int64_t ldy, const float* w,
                       const float* cos_tab, const float* sin_tab, int64_t rows,
                       int64_t rows_per_batch, int64_t D, int64_t head_dim, float eps, void* stream);

/*
 * scail_rmsnorm_rope with the result multiplied by out_scale before the one rounding to bf16.  The DiT executor uses it to hand
 * the self-attention its queries in log2 units (out_scale = log2(e) / sqrt(head_dim)), see scail_flash_attn_bf16 SCAIL_ATTN_Q_PRESCALED.
 */
int scail_rmsnorm_rope_scaled(const scail_bf16* x, int64_t ldx, scail_bf16* y, int64_t ldy,
                              const float* w, const float* cos_tab, const float* sin_tab,
                              int64_t rows, int64_t rows_per_batch, int64_t D, int64_t head_dim,
                              float eps, float out_scale, void* stream);

/*
 * The same row operation writing COLUMN SLABS instead of rows: the D columns are cut into D / slab_w slabs and slab g is a
 * [rows, slab_w] matrix with row stride slab_ld (>= slab_w; == slab_w: dense) at y + g * slab_stride (elements).  This is the send layout of
 * the Ulysses head <-> sequence all-to-all of the sequence-parallel self-attention (sat/mpu/ulysses_attn_layer.py:41-110: the reference's
 * `.permute(...).contiguous()` before its all_to_all_single; one slab per destination rank = that rank's heads of this rank's tokens),
 * produced by the q / k norm + RoPE itself rather than by a separate pack pass.  slab_ld = 3 * slab_w with y offset by 0 / slab_w /
 * 2 * slab_w lays q | k | v side by side in ONE [rows, 3 * slab_w] message per destination rank (one all-to-all instead of three;
 * scail_dit.h).  w == NULL: no normalisation, RoPE or scale -- a plain copy into the slab layout (the V third).
 */
int scail_rmsnorm_rope_slabs(const scail_bf16* x, int64_t ldx, scail_bf16* y, int64_t slab_w, int64_t slab_ld, int64_t slab_stride,
                             const float* w, const float* cos_tab, const float* sin_tab,
                             int64_t rows, int64_t rows_per_batch, int64_t D, int64_t head_dim,
                             float eps, float out_scale, void* stream);

/*
 * Which kernel the LayerNorm and RMSNorm (+ RoPE) entry points above run, in words, into buf[len], and -- `workgroups` != NULL -- the number of
 * workgroups of the launch.  `form` says which call is meant; its rows are n_batch * rows_out (scail_ln_modulate's arguments; every other
 * form: n_batch = 1, rows_out = rows), head_dim is read by the RMSNorm forms only.  The name is the kernel's template with the arguments of the
 * instantiation as csrc/rowops.hip launches it: "ln_kernel<0>" (modulate) / "ln_kernel<1>" (affine) and "rmsnorm_rope_kernel", one workgroup
 * per row; or, for D = 1536 / 2048 / 4096 / 5120 / 6144 under option "row_wave", one wave per row: "ln_wave_kernel<MODE, CPL>" and -- with
 * RoPE tables only -- "rmsnorm_rope_wave_kernel<CPL, HD128>", CPL = D / 512, HD128 = (head_dim == 128).  The name depends on the shape and
 * the option only and needs no device; the workgroup count of a wave form is sized by the device's compute units (about three persistent
 * workgroups per unit) and needs one.  A projection of the one choice function the launches follow (csrc/rowops.hip row_choose).
 * 0, 1 + scail_last_error (bad argument), or 2 (workgroups asked for and no device).
 */
enum {
    SCAIL_ROW_LN_MODULATE = 0,   /* scail_ln_modulate                                                   */
    SCAIL_ROW_LN_AFFINE = 1,     /* scail_layernorm_affine                                              */
    SCAIL_ROW_RMSNORM = 2,       /* scail_rmsnorm_rope / _scaled / _slabs with cos_tab == NULL          */
    SCAIL_ROW_RMSNORM_ROPE = 3,  /* ... with RoPE tables                                                */
    SCAIL_ROW_COPY = 4           /* scail_rmsnorm_rope_slabs with w == NULL                             */
};
int scail_row_kernel_name_for(int form, int64_t n_batch, int64_t rows_out, int64_t D, int64_t head_dim, char* buf, int64_t len,
                              int64_t* workgroups);

/*
 * The inverse layout pass: column slabs -> rows.  Slab g is a dense [rows, slab_w] matrix at x + g * slab_stride (elements); row r of
 * y [rows, D] (row stride ldy) receives slab g's row r at columns [g * slab_w, (g + 1) * slab_w).  The way back of the Ulysses exchange:
 * what a rank receives from the attention all-to-all is (source rank = head group, token, head-group columns); the out-projection wants
 * (token, all columns) (sat/mpu/ulysses_attn_layer.py:100-107, the reference's permute + reshape after its second all_to_all_single).
 */
int scail_slabs_to_rows(const scail_bf16* x, int64_t slab_w, int64_t slab_stride, scail_bf16* y, int64_t ldy,
                        int64_t rows, int64_t D, void* stream);

/*
 * V -> V^T staging for scail_flash_attn_bf16: v [n_batch, Lk, heads*head_dim] (row stride ldv,
 * batch stride v_batch_stride, elements) -> vt [n_batch, heads, head_dim, Lkp], Lkp = ceil64(Lk),
 * zero padded; inside every 16-key group key bits 2 and 3 are swapped so that one 16-byte LDS
 * read yields the 8 keys an MFMA 32x32x16 k-slot group consumes (see DESIGN.md "P.V operand").
 */
int scail_transpose_v(const scail_bf16* v, int64_t ldv, int64_t v_batch_stride, scail_bf16* vt,
                      int64_t n_batch, int64_t heads, int64_t head_dim, int64_t Lk, void* stream);

/*
 * Un-masked softmax attention, head_dim 128, replaces F.scaled_dot_product_attention at
 * sat/transformer_defaults.py:67-72 and the layout churn around it (dit...:1078-1100).
 *   q  [n_batch, Lq, heads, 128]   element strides (q_bs, q_rs); head h at column h*128
 *   k  [n_seg][n_batch, Lk, heads, 128]  strides (k_ss, k_bs, k_rs)
 *   vt [n_seg][n_batch, heads, 128, Lkp] from scail_transpose_v; strides (vt_ss, vt_bs); Lkp=ceil64(Lk)
 *   o  [n_batch, Lq, heads, 128]   strides (o_bs, o_rs); accumulate != 0 -> o += result
 *      (text + CLIP cross-attention sum, dit...:1197)
 * n_seg > 1: the key axis is the concatenation of n_seg equally sized segments (sequence-parallel
 * K/V all-gather); a batch stride of 0 broadcasts K/V over the batch.
 * softmax scale = `scale` (1/sqrt(128) in the reference; must be positive).  scale == SCAIL_ATTN_Q_PRESCALED (a negative sentinel)
 * means: q already carries the factor scale * log2(e) (scail_rmsnorm_rope_scaled) and the kernels compute exp2(q k^T - M) directly.
 * The 4-wave kernel (scail_attn4_m16f) works in log2 units either way: a raw scale is multiplied into its Q fragments once per
 * workgroup (one extra rounding of q to bf16), so both kinds of caller run the same loop; the 8-wave kernel applies the scale per
 * score.
 */
#define SCAIL_ATTN_Q_PRESCALED (-1.0f)
int scail_flash_attn_bf16(const scail_bf16* q, int64_t q_bs, int64_t q_rs,
                          const scail_bf16* k, int64_t k_ss, int64_t k_bs, int64_t k_rs,
                          const scail_bf16* vt, int64_t vt_ss, int64_t vt_bs,
                          scail_bf16* o, int64_t o_bs, int64_t o_rs,
                          int64_t n_batch, int64_t heads, int64_t Lq, int64_t Lk, int64_t n_seg,
                          float scale, int accumulate, void* stream);

/*
 * Which kernel scail_flash_attn_bf16 runs for a shape: 4 = the hand-scheduled 4-wave kernel scail_attn4_m16f (csrc/attn4.s, generated
 * by scail_amd/asmgen/attn4.py: one wave per SIMD, 64 query rows per wave; any key count >= 512, any scale, no accumulate, 32-bit byte
 * offsets inside one (batch, head) slice), 8 = the 8-wave kernel of csrc/attn.hip (everything else: short key sets, accumulate).  The
 * query answers for ONE (batch, head) pair: grids too large for the 4-wave kernel's workgroup-id decode -- 32 768 or more heads or batch
 * elements, (Lq / 192)^2 * heads * batch or heads^2 * batch >= 2^31 -- run the 8-wave kernel too, and scail_flash_attn_kernel_name_for,
 * which takes the pair counts, says so.  `prescaled` is kept for ABI stability and no longer changes the answer.  Host-only query; lets
 * a caller (and the tests) see the path taken.
 */
int scail_flash_attn_kernel_for(int64_t q_rs, int64_t k_rs, int64_t o_rs, int64_t Lq, int64_t Lk, int accumulate, int prescaled);

/*
 * The kernels a scail_flash_attn_bf16 call with these arguments runs, by name, under the options in force -- a projection of the one choice
 * function the launch follows (csrc/attn.hip attn_choose), as scail_flash_attn_kernel_for is.  The NUL-terminated name goes to buf[0, len).
 *   plan == NULL: the kernel alone, which needs no device: "scail_attn4_m16f" (the generated kernel's base symbol) or
 *       "flash_attn_swp_kernel<4, 4, 0, 1>" (the hipcc kernel's template with the arguments of the instantiation).
 *   plan != NULL (int64_t[9]): also the launches, {n_launch, rows, item0, n_items, xcd_mode of launch 0, the same of launch 1}, unused
 *       entries 0.  rows: query rows per workgroup; a launch covers items [item0, item0 + n_items) of the pair-major list of (pair, query
 *       block of `rows` rows) items; xcd_mode: the workgroup-id decode, 0 plain, 1 pairs dealt round-robin to the 8 XCDs, 2 the item list cut
 *       into 8 equal runs (grid padded to 8 * ceil(n_items / 8)).  The name then lists one symbol per launch joined by " + ":
 *       "scail_attn4_m16f + scail_attn4_m16f_q3" is scail_flash_attn_rows_for's 448.  The plan of the generated kernel needs the current
 *       device's compute-unit count unless option "attn4_rows" forces a height; a hipcc kernel is one launch of 256-row blocks, mode 0.
 * In the measurement build a schedule forced with "attn_variant" carries the prefix "attn_variant <code>: ".
 * 0, 1 + scail_last_error (bad argument; nothing is written), or 2 (a plan asked for and no device).
 */
int scail_flash_attn_kernel_name_for(int64_t q_rs, int64_t k_rs, int64_t o_rs, int64_t n_batch, int64_t heads, int64_t Lq, int64_t Lk,
                                     int accumulate, int prescaled, char* buf, int64_t len, int64_t* plan);

/*
 * Self-attention that reads V as the QKV projection wrote it -- no scail_transpose_v pass, no V^T image:
 *   v  [n_batch, Lk, heads, 128]  element strides (v_bs, v_rs), like k; q, k, o, scale as scail_flash_attn_bf16; ONE key segment, no accumulate.
 * It runs the V-rows forms of the 4-wave kernels, scail_attn4_m16f_vr / scail_attn4_m16f_q3_vr (generated by asmgen/attn4.py at build time: the V tile arrives row-major by
 * LDS-DMA and the P.V operand comes out of it through the transposed LDS read ds_read_b64_tr_b16), with scail_flash_attn_bf16's launch plan,
 * workgroup-id decodes and restart counter.  The same keys sit in the same MFMA k-slots in the same order: the result is bit for bit that of
 * scail_transpose_v + scail_flash_attn_bf16.  The kernel never reads a row of v past Lk - 1.
 * There is no other kernel behind this entry: what the 4-wave kernel cannot take -- Lk < 512, v_rs < heads * 128 or no multiple of 8,
 * Lk * v_rs (or Lk * k_rs, Lq * q_rs, Lq * o_rs) of 2^30 elements or more (32-bit byte offsets), a grid beyond the workgroup-id decode, options
 * "attn_vrows" or "attn4" at 0 -- is refused (1 + scail_last_error naming the value).  scail_flash_attn_vrows_for answers 1 exactly for the
 * calls that run (host-only, no device needed); a caller asks it and keeps scail_transpose_v + scail_flash_attn_bf16 for the rest.
 * scail_flash_attn_vrows_kernel_name_for: the kernels and the plan as scail_flash_attn_kernel_name_for gives them ("none", no launches, for a
 * call that would be refused).
 */
int scail_flash_attn_vrows_bf16(const scail_bf16* q, int64_t q_bs, int64_t q_rs,
                                const scail_bf16* k, int64_t k_bs, int64_t k_rs,
                                const scail_bf16* v, int64_t v_bs, int64_t v_rs,
                                scail_bf16* o, int64_t o_bs, int64_t o_rs,
                                int64_t n_batch, int64_t heads, int64_t Lq, int64_t Lk, float scale, void* stream);
int scail_flash_attn_vrows_for(int64_t q_rs, int64_t k_rs, int64_t v_rs, int64_t o_rs, int64_t n_batch, int64_t heads, int64_t Lq, int64_t Lk);
int scail_flash_attn_vrows_kernel_name_for(int64_t q_rs, int64_t k_rs, int64_t v_rs, int64_t o_rs, int64_t n_batch, int64_t heads, int64_t Lq,
                                           int64_t Lk, char* buf, int64_t len, int64_t* plan);

/*
 * Launch shape the 4-wave kernel would use for an attention of n_batch x heads (batch, head) pairs x Lq queries on the current device:
 *   256  one launch of scail_attn4_m16f (256 query rows per workgroup),
 *   192  one launch of scail_attn4_m16f_q3 (192 rows: 3 of the 4 query blocks per wave; 0.79 of the tile cost),
 *   448  both: whole rounds of 256-row workgroups, then the remaining rows (from a 768-row boundary on) as 192-row workgroups.
 * One workgroup fills a CU, so W workgroups take ceil(W / CUs) rounds of one tile; the plan minimises rounds x tile cost -- it matters for
 * the rank-sized launches of sequence-parallel execution (5 heads x 48 832 queries: 3.73 -> 4 rounds of 256 rows, against 3 + 0.79).
 * Results do not depend on the shape, except in workgroups that restart after an exp2 overflow of the optimistic pass (a score more than
 * 167 log2 units above its row's first-tile maximum): their rows go through the lazy-maximum loop, whose last-bit rounding differs, and
 * which rows share a workgroup depends on the tile height.  Option "attn4_rows" forces one height.  Host-only query.
 */
int scail_flash_attn_rows_for(int64_t n_batch, int64_t heads, int64_t Lq);

/*
 * Restart counter of the 4-wave self-attention kernel.  scail_attn4_m16f runs an OPTIMISTIC pass over the keys (scores relative to the
 * first key tile's row maximum, no maximum tracking in the hot loop) and verifies it on the row sums; a workgroup in which a score
 * exceeded that maximum by more than ~167 log2 units runs again with the lazy-maximum loop (correct either way, about twice the time for
 * that workgroup).  With a non-NULL `device_counter` (4-byte aligned device memory, caller-owned, caller-zeroed) every following
 * scail_flash_attn_bf16 launch of the CALLING THREAD adds 1 per restarting workgroup (one atomic in the restart path; nothing in the hot
 * loop); NULL switches it off.  Random data never restarts; trained q / k norm weights may (the rate a deployment should look at:
 * scail_dit_profile_read category SCAIL_DIT_PROF_ATTN_RESTARTS, bench.py `roofline.attn_restarts_per_launch`).
 */
int scail_flash_attn_count_restarts(uint32_t* device_counter);

/*
 * Cross attention over TWO key sets in one launch:
 *     o = bf16( bf16(softmax(scale q k1^T) v1) + softmax(scale q k2^T) v2 )
 * Replaces the text + CLIP-image cross attention of CrossAttentionLayer (dit_video_crossattn_sc_xc.py:1107-1203: two
 * attention_fn calls over the same queries, outputs added in bf16) -- independent softmax states per set, Q read once, O written
 * once (no read-modify-write).  Layouts as scail_flash_attn_bf16 with n_seg = 1: q / o row-strided token-major views with
 * heads * 128 columns, k1 / k2 (batch stride 0 = shared by the batch) with Lk1 / Lk2 >= 1 valid keys each, vt1 / vt2 =
 * scail_transpose_v images (heads, 128, ceil64(Lk)) per batch element (batch stride 0 = shared).  Meant for short key sets
 * (hundreds of keys).  scale: a positive number, or SCAIL_ATTN_Q_PRESCALED (q already carries scale * log2(e), scail_rmsnorm_rope_scaled).
 * Two kernels (scail_cross_attn2_kernel_for; option "cross4"): 4 = scail_attn4_x2 (csrc/attn4.s, generated: the 4-wave pipeline of the self-attention
 * kernel with PERSISTENT workgroups -- one per CU walks over the (batch, head, 256-row query block) items, loads an item's Q fragments
 * once and runs the key pipeline once per key set; needs k1_rs == k2_rs, >= 64 keys per set, 32-bit byte offsets per slice); 2 =
 * cross_attn2_kernel of csrc/attn.hip (128-row query blocks, two workgroups per CU): short key sets (fewer than 21 tiles together -- the
 * shipped text + CLIP shape) and everything the generated kernel is not eligible for.
 * scail_cross_attn2_kernel_name_for answers the same by name, "scail_attn4_x2" or "cross_attn2_kernel", into buf[0, len), and with
 * workgroups != NULL the launch's workgroup count: one persistent workgroup per compute unit of the current device (at most one per item)
 * for the generated kernel, which needs the device; one per (128-row query block, head, batch element) for the hipcc kernel.  Both queries
 * are projections of the one choice function the launch follows (csrc/attn.hip cross_choose).  0, 1 + scail_last_error (bad argument;
 * nothing is written), or 2 (workgroups asked for and no device).
 */
int scail_cross_attn2_kernel_for(int64_t q_rs, int64_t k1_rs, int64_t k2_rs, int64_t o_rs, int64_t Lq, int64_t Lk1, int64_t Lk2,
                                 int64_t n_batch, int64_t heads);
int scail_cross_attn2_kernel_name_for(int64_t q_rs, int64_t k1_rs, int64_t k2_rs, int64_t o_rs, int64_t Lq, int64_t Lk1, int64_t Lk2,
                                      int64_t n_batch, int64_t heads, char* buf, int64_t len, int64_t* workgroups);
int scail_cross_attn2_bf16(const scail_bf16* q, int64_t q_bs, int64_t q_rs,
                           const scail_bf16* k1, int64_t k1_bs, int64_t k1_rs, const scail_bf16* vt1, int64_t vt1_bs, int64_t Lk1,
                           const scail_bf16* k2, int64_t k2_bs, int64_t k2_rs, const scail_bf16* vt2, int64_t vt2_bs, int64_t Lk2,
                           scail_bf16* o, int64_t o_bs, int64_t o_rs,
                           int64_t n_batch, int64_t heads, int64_t Lq, float scale, void* stream);

/* Sinusoidal timestep embedding in fp64 like sgm/modules/diffusionmodules/util.py:207-231:
 * out[b, :dim/2] = cos(t*f), out[b, dim/2:] = sin(t*f), f_j = exp(-ln(1e4) j/(dim/2)). fp32 out; an odd dim gets a trailing zero column.
 * Errors (host side, before any launch): dim < 1, n outside [0, 2^31), a null pointer with n > 0. */
int scail_timestep_embedding(const float* t, float* out, int64_t n, int64_t dim, void* stream);

/* y[M,N] = act_out( act_in(x[M,K]) . W[N,K]^T + b ), M <= 8, x/y fp32, W bf16, b fp32.
 * act codes: 0 none, 1 SiLU, 2 GELU-tanh.  time_embed / adaln_projection (dit...:1327-1335,1524,1555). */
int scail_small_linear(const float* x, const scail_bf16* w, const float* b, float* y, int64_t M,
                       int64_t N, int64_t K, int act_in, int act_out, void* stream);

/* out[layer, b, j] = emb[b, j] + table[layer, j]   (AdaLN tables, dit...:1025-1028 and :823). fp32: one addition, the bits of torch's.
 * Errors: a size outside [0, 2^20), a null pointer with a non-empty table. */
int scail_adaln_table(const float* emb, const float* table, float* out, int64_t n_layers,
                      int64_t n_batch, int64_t width, void* stream);

/*
 * Token assembly for the patch embedding (DiffusionTransformer.forward dit...:1457-1503 +
 * ImagePatchEmbeddingMixin dit...:99-130): writes the per-patch im2col matrix
 *   tok [n_batch, L, kpad] bf16,  L = (1+T)*(H/2)*(W/2) + T*(H/4)*(W/4), kpad >= 80 (zero padded),
 * column (c*4 + p*2 + q), c<16 latent channel, c in 16..19 mask channel (0 noise, 1 ref/pose),
 * token order [ref | noise | pose], each (t h w) row-major.
 *   x fp32 [n_batch,T,16,H,W] (rounded to bf16 as dit...:1454-1455); ref bf16 [n_ref,1,16,H,W];
 *   pose bf16 [n_pose,T,16,H/2,W/2]; n_ref/n_pose in {1, n_batch} (CFG repeat :1479-1495).
 * Errors (host side, before any launch): a size outside [0, 2^15), H or W no multiple of 4, kpad < 80 or no multiple of 8, and for a
 * non-empty token matrix a null pointer, a misaligned one (x 4 bytes, ref / pose 2, tok 16: 16-byte stores) or 2^31 workgroups or more.
 */
int scail_patchify(const float* x, const scail_bf16* ref, const scail_bf16* pose, scail_bf16* tok,
                   int64_t n_batch, int64_t n_ref, int64_t n_pose, int64_t T, int64_t H, int64_t W,
                   int64_t kpad, void* stream);

/*
 * Multi-character token assembly (an EXTENSION: the reference has one reference frame and one pose stream, dit...:1559): the same
 * im2col matrix for n_char >= 1 characters in ONE launch,
 *   tok [n_batch, L, kpad],  L = (n_char + T)*(H/2)*(W/2) + n_char*T*(H/4)*(W/4),
 * token order [ref_0..ref_{C-1} | noise | pose_0..pose_{C-1}], columns and mask channels as above;
 *   ref bf16 [n_ref, n_char, 16, H, W];  pose bf16 [n_pose, n_char*T, 16, H/2, W/2] (character k = frames k*T .. (k+1)*T - 1).
 * n_char == 1 writes byte for byte what scail_patchify writes.  n_char outside 1..64 and pointers that are not aligned for the
 * kernel's paired reads (x 8 bytes, ref / pose 4, tok 16) are errors.
 */
int scail_patchify_chars(const float* x, const scail_bf16* ref, const scail_bf16* pose, scail_bf16* tok,
                         int64_t n_batch, int64_t n_ref, int64_t n_pose, int64_t n_char, int64_t T, int64_t H, int64_t W,
                         int64_t kpad, void* stream);

/* unpatchify dit...:764-784: tok [n_batch, T*(H/2)*(W/2), 64] bf16 ((o p q c) columns)
 * -> out fp32 [n_batch, T, 16, H, W]: out[b, t, c, 2h+p, 2w+q] = tok[b, (t h w), 32p + 16q + c].
 * Errors: a size outside [0, 2^15), H or W odd (the kernel would read a neighbouring token's row, and on the last token past the end),
 * and for a non-empty latent a null pointer or 2^31 workgroups or more. */
int scail_unpatchify(const scail_bf16* tok, float* out, int64_t n_batch, int64_t T, int64_t H,
                     int64_t W, void* stream);

/* x += dsigma * (v_u + cfg * (v_c - v_u)),  v = [v_u; v_c] fp32 [2, n]
 * (guiders.py:41-45 + sampling_utils.py:7-10 + Euler update sampling.py:960-963), all fp32.  Its two multiply-adds may contract: an element is
 * one of the four results with each of them fused or rounded separately.  Errors: n < 0 or 2^31 workgroups or more, a null pointer with n > 0. */
int scail_cfg_euler(float* x, const float* v, int64_t n, float cfg_scale, float dsigma, void* stream);

/*
 * The two fp32 passes of the guidance plan (scail_dit.h "guidance plan"): classifier-free guidance around a STORED v_c - v_u.
 *   scail_cfg_delta_store:  delta[i] = v_c[i] - v_u[i]                                 v = [v_u; v_c] fp32 [2, n], only read
 *   scail_cfg_euler_delta:  x[i] = x[i] + dsigma * (v_c[i] + g * delta[i])             g = cfg_scale - 1, formed once on the host in fp32
 *                           x[i] = x[i] + dsigma * v_c[i]                              with delta == NULL: no guidance
 * v_c + (s - 1) (v_c - v_u) is v_u + s (v_c - v_u) rewritten around the difference.  EVERY operation is rounded on its own (no fused
 * multiply-add), so each call gives the bits of the torch fp32 expression, one tensor operation per arithmetic operation -- unlike
 * scail_cfg_euler, whose multiply-adds contract.  v_c and delta are only read.
 * Errors (host side, naming the value): n < 0 or 2^31 workgroups or more; a null v / delta (store) or x / v_c (euler).  n == 0 launches
 * nothing.
 */
int scail_cfg_delta_store(const float* v, float* delta, int64_t n, void* stream);
int scail_cfg_euler_delta(float* x, const float* v_c, const float* delta, int64_t n, float cfg_scale, float dsigma, void* stream);

/*
 * The fp32 pass of the solver plan (scail_dit.h "solver plan"): classifier-free guidance and ONE step of a linear multistep solver in the
 * data prediction, x <- a x + b D + c D_prev.  v = [v_u; v_c] fp32 [2, n], only read; x and hist fp32 [n], updated in place.  Per
 * element, in this order:
 *   d = v_u + cfg_scale * (v_c - v_u)
 *   D = x - sigma * d                      the data prediction of rectified flow at the step's STARTING sigma
 *   y = a * x + b * D
 *   y = y + c * hist                       only with use_prev != 0
 *   x = y;  hist = D
 * EVERY operation is rounded on its own (no fused multiply-add), as in scail_cfg_euler_delta: the call gives the bits of the torch fp32
 * expression, one tensor operation per arithmetic operation.  With use_prev == 0 hist is never READ -- it may hold anything, NaN
 * included -- and is written all the same.  Elementwise: one thread reads, then writes, its own elements; 16-byte accesses where x, v
 * and hist are 16-byte aligned, with a scalar tail.  a, b, c are the caller's (scail_amd/sampler.py plan_solver).
 * Errors (host side, naming the value): n < 0 or 2^31 workgroups or more; with n > 0 a null x, v or hist.  n == 0 launches nothing.
 */
int scail_cfg_multistep(float* x, const float* v, float* hist, int64_t n, float cfg_scale, float sigma, float a, float b, float c,
                        int use_prev, void* stream);

/*
 * LoRA adapters (scail_amd/lora.py): merge a low-rank weight update, or a full difference, into a bf16 weight, in place and once.
 * w is an N x K window of a bf16 matrix with row stride ldw (elements); a row slice of a fused matrix is w + n0 * ldw.  up is fp32
 * [N, r] (row stride ld_up), down fp32 [r, K] (ld_down), d fp32 [N, K] (ldd).  The factors are fp32 because adapter files come in fp16,
 * bf16 or fp32 and all three widen exactly.  Per element (n, k), in this order:
 *   acc = 0.0f
 *   for j = 0 .. r-1 (ascending):   acc = acc + up[n, j] * down[j, k]
 *   w[n, k] = bf16_rne( float(w[n, k]) + scale * acc )          scail_lora_merge_bf16
 *   w[n, k] = bf16_rne( float(w[n, k]) + scale * d[n, k] )      scail_add_scaled_bf16
 * EVERY operation is rounded on its own (no fused multiply-add), as in scail_cfg_euler_delta: the call gives the bits of the torch fp32
 * expression, one tensor operation per arithmetic operation, and one rounding to bf16 (to nearest, ties to even).  The product runs on
 * the VALU: an fp32 MFMA is an fmaf chain, which is not this arithmetic.
 * In place and elementwise in (n, k): one thread reads, then writes, its own elements; nothing outside the N x K window is touched.
 * 16-byte accesses to w where w is 16-byte aligned and ldw a multiple of 8, a scalar path for row tails and everything else.  There is
 * no limit on r below 2^15: the r loop is chunked through LDS.  N == 0, K == 0 or (merge) r == 0 launches nothing and w keeps its bits,
 * a -0 included.
 * Errors (host side, before any launch, naming the value): negative N, K or r; r >= 2^15; ldw < K, ld_up < r, ld_down < K, ldd < K; a
 * scale that is not finite; 2^31 workgroups or more; with a non-empty problem a null w, up, down or d.
 */
int scail_lora_merge_bf16(scail_bf16* w, int64_t ldw, int64_t N, int64_t K, const float* up, int64_t ld_up, const float* down,
                          int64_t ld_down, int64_t r, float scale, void* stream);
int scail_add_scaled_bf16(scail_bf16* w, int64_t ldw, int64_t N, int64_t K, const float* d, int64_t ldd, float scale, void* stream);

/*
 * Temporal tiling of RFSamplerLong (sampling.py:986-1085): the three elementwise fp32 passes of one sampler step around the network
 * evaluations of its tiles.  A latent frame is F = 16*H*W floats, x / den are [T, F], a tile has Tt <= min(T, 64) frames f_0 .. f_{Tt-1}
 * of [0, T) in any order.  `frames`, `wk` and `inv_wsum` are HOST arrays read during the call: their values travel in the kernel
 * arguments, so there is no host-to-device copy and no synchronisation, and the launches can be stream-captured.
 *   scail_tile_gather     xin[j, :] = xin[Tt + j, :] = x[f_j, :] for j < Tt     (xin fp32 [2, Tt, F]: the CFG batch torch.cat([x[:, idx]] * 2))
 *   scail_tile_blend_acc  d = v_u + cfg * (v_c - v_u);  den[f_j, e] = den[f_j, e] + wk[j] * d      (v = [v_u; v_c] fp32 [2, Tt, F];
 *                         wk[j] = float(m_k) * tile_weight[j], m_k = 1 for the first and last tile and 2 otherwise)
 *   scail_tile_finish     x[f, e] = x[f, e] + dsigma * (den[f, e] * inv_wsum[f]) for every f < T, then den[f, e] = 0
 * EVERY operation is rounded on its own (no fused multiply-add), so each call gives the bits of the torch expression it replaces in
 * scail_amd/sampler.py RFSamplerLong.sample_hip -- unlike scail_cfg_euler, whose multiply-adds contract.
 * Errors (host side, naming the value): Tt outside 1..min(T, 64), a frame index outside [0, T), and for scail_tile_blend_acc an index
 * repeated inside the tile (two tile frames would accumulate into one latent frame concurrently).
 */
int scail_tile_gather(const float* x, float* xin, const int32_t* frames, int64_t Tt, int64_t T, int64_t F, void* stream);
int scail_tile_blend_acc(float* den, const float* v, const int32_t* frames, const float* wk, int64_t Tt, int64_t T, int64_t F,
                         float cfg_scale, void* stream);
int scail_tile_finish(float* x, float* den, const float* inv_wsum, int64_t T, int64_t F, float dsigma, void* stream);
/*
 * scail_tile_finish under a solver plan (scail_dit.h "solver plan"): scail_cfg_multistep's sequence from "D = x - sigma * d" on, with
 * d = den[f, e] * inv_wsum[f], the product scail_tile_finish forms; then den[f, e] = 0.  x, den, hist fp32 [T, F]; inv_wsum a HOST array
 * that travels in the kernel arguments; the same limits on T and F, the same errors, and a null hist.  Every operation is rounded on
 * its own; with use_prev == 0 hist is never read.  16-byte accesses where F % 4 == 0 and x, den and hist are 16-byte aligned.
 */
int scail_tile_finish_multistep(float* x, float* den, const float* inv_wsum, float* hist, int64_t T, int64_t F, float sigma, float a, float b,
                                float c, int use_prev, void* stream);


/* ---- Wan2.1 causal 3D VAE (sgm/models/wan_vae.py), channels-last (T,H,W,C) bf16 activations ------------- */

/*
 * Implicit-GEMM convolution, whole sequence in one pass:
 *   y[voxel(to,ho,wo), n] = bias[n] + sum_{dt,dh,dw,c} x[ti, hi, wi, c] * w[n, ((dt*kh+dh)*kw+dw)*Cin + c] (+ resid)
 *   ti = to*st + dt - pt,  hi = ho*sh + dh - ph,  wi = wo*sw + dw - pw   (out-of-range -> 0);
 *   ups != 0: the input is virtually nearest-exact upsampled 2x in H and W first (hi, wi index the
 *   upsampled grid, source pixel = index >> 1)                                  (Upsample + Conv2d, :76-85)
 * Covers CausalConv3d (:17-36: pt = 2*p front padding only), the stride-2 downsampling convs with
 * ZeroPad2d((0,1,0,1)) (:87-96: ph = pw = 0) and the temporal convs of Resample (:84-96).
 *   x (Ti,Hi,Wi,Cin) with Cin % 8 == 0;  w (>= N rows, Kpad) bf16, K zero-padded to a multiple of 64;
 *   output voxel index = ((to*ot_mul + ot_off)*Ho + ho)*Wo + wo, row stride ldc (resid likewise, ldr);
 *   geom = {Ti,Hi,Wi,Cin, To,Ho,Wo, kt,kh,kw, st,sh,sw, pt,ph,pw, ups, ot_mul,ot_off, N,Kpad} (21 int32, host).
 */
int scail_conv3d_cl(const scail_bf16* x, const scail_bf16* w, const float* bias, scail_bf16* y, int64_t ldc,
                    const scail_bf16* resid, int64_t ldr, const int32_t* geom, void* stream);

/*
 * Host-only queries of the ONE rule by which csrc/conv.hip picks a convolution's kernel (conv_choose: the launches follow the same function,
 * so the shapes are stated there and nowhere else).  None of them sees the pointers: they answer for 16-byte aligned ones (a call with a
 * misaligned output, residual or gamma runs the hipcc kernels).  ldr = 0: no residual.
 * scail_conv3d_kernel_for: what runs scail_conv3d_cl (fused_norm = 0) / scail_conv3d_cl_norm (1) / scail_conv3d_cl_resid_norm (2).
 *   4 = a hand-scheduled kernel generated by scail_amd/asmgen/conv4.py (csrc/conv4.s, conv4u.s: persistent workgroups of 4 waves, 2 frames x
 *       16 x 16 voxels x 96 channels per tile): the 3x3x3 stride-1 'same' convolutions with Cin % 32 == 0, N % 96 == 0 -- or N = 8 / 16, the RGB
 *       head --, To >= 2, ldc % 8 == 0; Resample's 1x3x3 convolution, also behind the 2x upsample; with fused_norm = 1 those with N = 96; with
 *       fused_norm = 2 the whole call in ONE launch (N = ldc = 96, ot_mul = 1, ot_off = 0; options "conv4", "conv4_cont", "conv4_resnorm" on);
 *   2 = (fused_norm = 2 only) one launch as well, of the hipcc direct-gather kernel's dual-output form (the encoder's stem; option "conv_direct");
 *   0 = the hipcc kernels of csrc/conv.hip; for fused_norm = 2 as the two separate calls.
 */
int scail_conv3d_kernel_for(const int32_t* geom, int64_t ldc, int64_t ldr, int fused_norm);
/* Whether a ResidualBlock's residual.2 -> RMS_norm -> SiLU should be ONE scail_conv3d_cl_norm call (1) or scail_conv3d_cl + scail_rms_silu (0:
 * scail_conv3d_cl_norm rejects the geometry, or the plain generated kernel + the pass is the faster pair).  csrc/vae_exec.hip and wan_vae.py ask this. */
int scail_conv3d_norm_fused_for(const int32_t* geom, int64_t ldc);
/* The kernel of a call, in words, into buf[len]: `form` 0 scail_conv3d_cl, 1 scail_conv3d_cl_norm ("rejected" where it refuses), 2 / 3
 * scail_conv3d_cl_resid_norm with / without the raw output.  A generated kernel's symbol ("scail_conv4c_e3"), or a hipcc kernel's template name
 * with its arguments as the source instantiates it ("conv_halo_kernel<0, 32, 1, false, 96, 2>"; " x 2": two launches); a next-norm call that
 * runs as two calls names the convolution's kernel " + scail_rms_silu".  Tile counts and grids are not part of the name.  0, or 1 + scail_last_error. */
int scail_conv3d_kernel_name_for(const int32_t* geom, int64_t ldc, int64_t ldr, int form, char* buf, int64_t len);

/*
 * The same convolution with RMS_norm + SiLU fused into the epilogue (ResidualBlock: residual.2 conv -> residual.3 RMS_norm ->
 * residual.4 SiLU, wan_vae.py:190-196): y = SiLU(RMS_norm(conv(x) + bias) * gamma), RMS_norm as in scail_rms_silu, applied
 * to the bf16-rounded convolution output.  Only the raw convolution output's round trip through HBM disappears; the
 * arithmetic is that of the two separate calls (up to the order of the norm's sum and, on the generated kernel, a reciprocal
 * instead of the division).  3x3x3, stride 1, 'same' spatial extent, Cin % 32 == 0, N <= 96 (one
 * output tile holds every channel of a voxel); anything else is rejected.  gamma fp32 [N], 16-byte aligned.
 */
int scail_conv3d_cl_norm(const scail_bf16* x, const scail_bf16* w, const float* bias, scail_bf16* y, int64_t ldc,
                         const float* gamma, const int32_t* geom, void* stream);

/*
 * The LAST convolution of a ResidualBlock together with the RMS_norm + SiLU of whatever reads the block's output next (wan_vae.py:180-218 x =
 * residual(x) + shortcut(x), then the next block's residual.0 / residual.1 or the decoder head's norm :417):
 *     y      = bf16(resid + conv(x) + bias)                      (skipped when y == NULL: nobody reads the raw sum)
 *     y_norm = SiLU(RMS_norm(y) * gamma)                         RMS_norm as in scail_rms_silu, applied to the bf16-rounded sum
 * = scail_conv3d_cl(.., resid ..) followed by scail_rms_silu(y, y_norm, gamma, .., 1), which is what this entry point runs wherever
 * scail_conv3d_kernel_for(geom, ldc, ldr, 2) == 0 or a pointer is not 16-byte aligned.  Where it is 4 or 2 ONE launch covers the call: the raw
 * sum is bit-identical to scail_conv3d_cl's and the normalised tensor agrees with the separate pass up to the order of the norm's sum (one read
 * of the 14 GB block input of the full-resolution stages disappears).  Dense outputs only: ldc == N, ot_mul = 1, ot_off = 0; y != y_norm; gamma
 * fp32 [N].  The two-call form needs what scail_rms_silu needs, N <= 512: every argument is checked before anything is launched.
 * resid == NULL (ldr ignored): the same for a producer that is not a ResidualBlock -- y = conv + bias is then required -- e.g. Resample's 1x3x3
 * convolution behind the 2x upsample (wan_vae.py:76-85) in front of the decoder's full-resolution blocks.
 */
int scail_conv3d_cl_resid_norm(const scail_bf16* x, const scail_bf16* w, const float* bias, scail_bf16* y, scail_bf16* y_norm, int64_t ldc,
                               const scail_bf16* resid, int64_t ldr, const float* gamma, const int32_t* geom, void* stream);

/* RMS_norm over channels (F.normalize * sqrt(C) * gamma, :39-54) + optional SiLU; x,y (nvox, C), gamma fp32. */
int scail_rms_silu(const scail_bf16* x, scail_bf16* y, const float* gamma, int64_t nvox, int64_t C, int silu,
                   void* stream);

/* In-place row softmax of scale * s over the first n columns of each row (AttentionBlock, :252); 1 <= n <= 32768; rows are
 * padded to a multiple of 8 columns in memory (ld % 8 == 0, ld >= ceil8(n)) and columns n .. ceil8(n) are written as zeros. */
int scail_softmax_rows(scail_bf16* s, int64_t ld, int64_t rows, int64_t n, float scale, void* stream);

/* Batched 2-D transpose (R x C, row stride ldi) -> (C x R, row stride ldo); columns from R on of the output are not written.
 * Errors: a negative size, ceil(R / 64) or batch above 65535 (grid y and z), and for a non-empty call a null pointer, ldi < C or ldo < R. */
int scail_transpose2d(const scail_bf16* in, int64_t ldi, int64_t in_bs, scail_bf16* out, int64_t ldo,
                      int64_t out_bs, int64_t R, int64_t C, int64_t batch, void* stream);

/* planar fp32 (C, N) -> channels-last bf16 (N, Cpad): y = x*a[c] + b[c] (a, b may be NULL), pad channels +0.  The multiply-add may contract:
 * an element is bf16 of the fused or of the separately rounded fp32 result.  Errors: not 0 < C <= Cpad < 2^20, N outside [0, 2^40), and
 * for N > 0 a null x or y or 2^31 workgroups or more. */
int scail_to_channels_last(const float* x, scail_bf16* y, const float* a, const float* b, int64_t C,
                           int64_t Cpad, int64_t N, void* stream);

/* channels-last bf16 (N, ldx) -> planar fp32 (C, N): y = clamp((x + b[c]) * a[c], lo, hi) = fminf(fmaxf(., lo), hi), each operation rounded on
 * its own (nothing to contract).  fmaxf returns its other argument for a NaN: a NaN input comes out as lo.  Errors: not 0 < C <= ldx,
 * C >= 2^20, N outside [0, 2^40), and for N > 0 a null x or y or 2^31 workgroups or more. */
int scail_from_channels_last(const scail_bf16* x, int64_t ldx, float* y, const float* a, const float* b,
                             int64_t C, int64_t N, float lo, float hi, void* stream);

/* The same two passes over a window of frames of a LONGER planar tensor (scail_vae_decode_stream, one chunk of a clip at a time): the planar
 * side has its channel planes `plane` elements apart (Tl*hl*wl of the latent, T*H*W of the video) and the window is the N voxels that start
 * `off` elements into every plane (first frame * frame size); the channels-last side is the dense (N, Cpad) / (N, ldx) tensor of the window.
 * Same arithmetic, scale, shift and clamp as above.  Cpad / ldx multiples of 8 (16-byte rows, 16-byte aligned); the planar side is moved as
 * float4 when plane, off and N are multiples of 4 and its base is 16-byte aligned, else as dwords.  off + N <= plane. */
int scail_to_channels_last_frames(const float* x, scail_bf16* y, const float* a, const float* b, int64_t C, int64_t Cpad,
                                  int64_t plane, int64_t off, int64_t N, void* stream);
int scail_from_channels_last_frames(const scail_bf16* x, int64_t ldx, float* y, const float* a, const float* b, int64_t C,
                                    int64_t plane, int64_t off, int64_t N, float lo, float hi, void* stream);

/* The output end of a request in one pass (the opt-in route of scail_vae_decode_u8; replaces torch.clamp((x + 1) / 2, 0, 1) of
 * sample_video.py:494 and the writers' (255 * x).astype(uint8), :188 / :212): the dense channels-last bf16 tensor x (n_frames * H * W, ldx),
 * whose channels 0, 1, 2 are R, G, B, becomes the uint8 pixels a file writer takes.  Channel c of pixel (t, y, x) is written to
 *   out + t * frame_bytes + y * row_bytes + 3 * x + c.
 * row_bytes = 3 W and frame_bytes = 3 W H is a dense (n_frames, H, W, 3) clip; a larger row_bytes writes one panel of a wider picture (the
 * layout "h (n w) c" of several clips side by side); `out` advanced by whole frames writes a window of a longer clip.  Bytes outside the
 * window's pixels are not touched, and channels >= 3 of a row are never interpreted (they may hold anything, NaN included).
 * Arithmetic, fp32, every operation rounded on its own:  v = float(x);  y = min(max((v + 1) / 2, 0), 1);  u = (uint8) trunc(255 * y)  -- bit
 * for bit what the two reference expressions give for every finite v and for +-inf (255 and 0).  NaN is written as 0: the reference route
 * hands a NaN to numpy's float -> uint8 cast, whose result for it is unspecified.
 * ldx: a multiple of 8, >= 8, x 16-byte aligned; `out` needs no alignment (16-byte stores wherever the addresses allow, bytes at ragged
 * ends).  Refused before anything is enqueued, naming the value: a null pointer, such an ldx or x, row_bytes < 3 W,
 * frame_bytes < H * row_bytes, negative sizes (each size below 2^20).  n_frames * H * W == 0 is accepted and launches nothing. */
int scail_frames_u8(const scail_bf16* x, int64_t ldx, uint8_t* out, int64_t row_bytes, int64_t frame_bytes,
                    int64_t n_frames, int64_t H, int64_t W, void* stream);


/* ---- conditioning encoders (UMT5-XXL text encoder, CLIP ViT-H/14 visual) ---------------- */

/*
 * Small-sequence softmax attention, head_dim <= 128, K and V of one (batch, head) resident in LDS.
 *   o = softmax(scale * q k^T + bias_tab[bucket[i, j], h] + mask) v
 * strides = {q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs} (elements, host array); head h at column h*head_dim.
 * bucket int32 [Lq, Lk] + bias_tab fp32 [n_buckets, heads]: T5 relative-position bias (umt5.py:224-268, 101-113);
 * key_mask int32 [n_batch, key_mask_bs]: 0 -> key excluded (umt5.py:106-110).  CLIP: no bias/mask, scale
 * 1/sqrt(head_dim) (clip.py:96-103).
 * Precondition: every batch element of key_mask has at least one non-zero entry among its Lk keys.  A fully masked row has
 * max = -inf, -inf - -inf in every exponent, and comes back as NaN; the entry point does not look at the mask's contents.  The
 * callers keep it: the only masks are the tokenizer's attention masks, and `</s>` is always there, the empty prompt included
 * (tests/test_conditioner_mask_cpu.py).  K and V of one head must fit in LDS: Lk * (4 * head_dim + 32) + 16 * head_dim <= 163 840
 * bytes (512 keys at head_dim 64, 297 at 128), else the call is refused before any launch.
 */
int scail_attn_small(const scail_bf16* q, const scail_bf16* k, const scail_bf16* v, scail_bf16* o,
                     const int64_t* strides, int64_t n_batch, int64_t heads, int64_t Lq, int64_t Lk, int64_t head_dim,
                     float scale, const int32_t* bucket, const float* bias_tab, const int32_t* key_mask,
                     int64_t key_mask_bs, void* stream);

/* y = a * b elementwise (gated-GELU FFN of T5, umt5.py:141). */
int scail_mul_bf16(const scail_bf16* a, const scail_bf16* b, scail_bf16* y, int64_t n, void* stream);

/* y[r,:] = x[r,:] * rowscale[r] + addrow[r % add_rows,:]  (zeroing padded text rows umt5.py:522; adding the
 * ViT position embedding clip.py:317-318).  rowscale fp32 / addrow bf16 may be NULL. */
int scail_row_affine(const scail_bf16* x, scail_bf16* y, const float* rowscale, const scail_bf16* addrow, int64_t add_rows,
                     int64_t rows, int64_t D, void* stream);

/*
 * Runtime options of the library (process-wide).  Returns 0, or 1 for an unknown option / out-of-range value (scail_last_error names
 * it).  The state is std::atomic: setting an option while other threads launch is defined -- a launch reads each option once and sees the
 * old or the new value; an explicit "attn4_rows" wins over the executor's internal per-thread hint.
 *   "attn4"      1 (default): scail_flash_attn_bf16 uses the 4-wave kernel wherever scail_flash_attn_kernel_for says 4;
 *                0: the 8-wave kernel for every shape.
 *   "attn_vrows" 1 (default): scail_flash_attn_vrows_for says yes wherever the V-rows kernels can run, and the DiT executor then skips
 *                scail_transpose_v (0.39 ms and 2 GB of HBM traffic per layer at 48 832 tokens); 0: it says no, and every caller stages V^T
 *                as before (bit-identical results either way).
 *   "gemm4"     1 (default): scail_gemm_bf16 uses the generated 4-wave kernels wherever scail_gemm_kernel_for says 4;
 *                0: the kernels of csrc/gemm.hip for every shape.
 *   "conv4"      1 (default): scail_conv3d_cl uses the generated kernels wherever scail_conv3d_kernel_for says 4;
 *                0: the kernels of csrc/conv.hip for every convolution.
 *   "conv4_cont" 1 (default): 3x3x3 convolutions with ONE n tile (96 output channels) run the tile-continuation variants of the generated kernels
 *                (scail_conv4c_e0 / e3 / e4: a workgroup's run of frame pairs keeps the patch and W rings going across tiles; bit-identical
 *                results); 0: scail_conv4_e0 / e3 / scail_conv4f_e4 for them too.
 *   "conv4_resnorm" 1 (default): scail_conv3d_cl_resid_norm runs the generated kernels with the consumer's norm in the residual epilogue
 *                (scail_conv4c_e5 / e6) where scail_conv3d_kernel_for(.., 2) says 4; 0: the two separate calls for every shape (the same-process
 *                A/B of round 6).  Needs "conv4" and "conv4_cont" on.
 *   "conv_direct" 1 (default): scail_conv3d_cl runs the direct-gather kernel on the HBM-bound shapes (Cin % 8 == 0, no residual, no upsample,
 *                >= 4096 output voxels; K <= 96 with 32 / 64 / 96 / 128 / 192 / 384 output channels: the VAE's 1x1x1 shortcut 96 -> 192; K <= 224
 *                with 96 output channels: the stem 3 -> 96); 0: the gather kernel for them too.
 *   "conv_s2"    1 (default): scail_conv3d_cl runs conv_s2_kernel on Resample's spatial downsampling -- 1 x 3 x 3, stride (1, 2, 2), no leading padding (the
 *                reference's ZeroPad2d((0, 1, 0, 1)) is the zero row / column behind the input), Cin % 32 == 0, N % 96 == 0, no residual: an 8 x 16 output tile
 *                per workgroup with its 17 x 33 input patch in LDS (columns split by parity).  2: two output frames per workgroup (measured slower: one
 *                workgroup per CU); 0: the gather kernel (4.04 / 3.40 / 1.28 ms against 2.95 / 2.35 / 1.10 ms on the three encoder shapes of config 4).
 *   "row_wave"   1 (default): scail_ln_modulate / scail_layernorm_affine / scail_rmsnorm_rope* run the one-wave-per-row kernels where D is
 *                1536, 2048, 4096, 5120 or 6144; 0: the block-per-row kernels for every D (results agree up to the order of the fp32 sums).
 *   "cross4"     2 (default): scail_cross_attn2_bf16 runs the generated persistent kernel scail_attn4_x2 when the two key sets hold 21 or more
 *                64-key tiles together (measured crossover: 22.6 us + 1.5 us per tile against 8.5 us + 2.17 us per tile of cross_attn2_kernel per
 *                256-row item; 1024 + 64 keys: 2.67 vs 2.74 ms, 4096 + 64: 6.39 vs 9.04 ms) and cross_attn2_kernel below -- the shipped 512 + 257
 *                keys (13 tiles: 2.55 vs 2.19 ms) stay on the hipcc kernel; 1: the generated kernel wherever eligible; 0: never.
 *   "attn4_rows" 0 (default): the 4-wave kernel's launch shape is planned per attention (scail_flash_attn_rows_for: 256-row workgroups,
 *                192-row workgroups, or whole rounds of the former + the latter for the rest); 192 / 256: one launch of that height.
 *   "attn4_cus"  0 (default): the launch plan counts on every CU of the device; n > 0: on n CUs -- for a process whose collectives run
 *                beside the attention (RCCL holds one CU per channel while a collective is in flight: a sequence-parallel rank sets
 *                CUs - channels; scail_amd/parallel.py).
 *   "attn4_xcd"  1 (default): with 8 or more (batch, head) pairs, workgroup ids are decoded so that the CUs of one XCD work on the same pair
 *                and share its K / V^T in that XCD's L2 (whole launches of 8 k pairs: pairs dealt round-robin to the XCDs; otherwise 8 equal
 *                runs of the pair-major tile list); 0: plain decode for every launch.
 *   "attn4_thr"  lazy-rescale threshold of the 4-wave kernel in log2 units (default 8: the running row maximum is only raised,
 *                and O / l rescaled, when a score exceeds it by more than 2^8; exact either way, 0 = rescale on every new
 *                maximum like the 8-wave kernel).  Range [0, 64].
 * Schedule A/B knobs, timing ablations and cycle probes are NOT part of this library: they live in the measurement build
 * (include/scail_hip_ablation.h, SCAIL_ABLATIONS=1 python -m scail_amd.build -> scail_amd/libscail_hip_abl.so).
 */
int scail_set_option(const char* name, int value);

/*
 * MEASUREMENT helper (nothing in the product path calls it): a stand-in for a collective in flight on ONE GPU.  `workgroups` workgroups
 * of 256 threads copy `bytes` (multiple of 16, both pointers 16-byte aligned) from src to dst and then stay resident until `min_ns`
 * nanoseconds have passed since the kernel started -- the way RCCL's channel kernels hold one CU each for the duration of a transfer
 * that the xGMI links, not the CUs, bound.  Launched on `stream` (a side stream, like RCCL's).  scail_amd.parallel.ConcurrentCopyBackend
 * serves a sequence-parallel rank's exchanges with it: the compute side of an N-rank step WITH the CU occupancy of its collectives
 * (tools/sp_rank_compute.py --comm-wgs K; bench.py config.sp_compute_side).
 */
int scail_comm_standin(const void* src, void* dst, int64_t bytes, int32_t workgroups, int64_t min_ns, void* stream);

/*
 * Frees the device memory the library keeps between calls: the tile-order tables of the generated GEMM kernels (a few KB per tile grid,
 * allocated by the first launch of a grid on a device, cached per HIP device id like the embedded code objects).  Call at teardown with
 * no launch in flight; later launches re-create what they need.  A table's device pointer is a kernel argument of the launches that use it,
 * so any hipGraph captured from library calls BEFORE this call holds freed pointers: destroy or re-capture such graphs, never replay them.
 */
int scail_release_caches(void);

/* fp32 -> bf16 (round to nearest even; denormals in and out are kept, not flushed; a NaN stays a NaN) and back (the pattern << 16);
 * plumbing for boundary tensors.  Errors: n < 0 or 2^31 workgroups or more, a null pointer with n > 0. */
int scail_f32_to_bf16(const float* x, scail_bf16* y, int64_t n, void* stream);
int scail_bf16_to_f32(const scail_bf16* x, float* y, int64_t n, void* stream);

/*
 * The row kernels of the step cache (scail_dit.h SCAIL_DIT_CACHE_FILL / _REUSE): the change a run of blocks made to a window of hidden-state
 * rows, kept and added back.  All operands are bf16 with row stride D; element b of an operand starts b * (its batch stride, in elements)
 * after the base; r is dense [n_batch, rows, D].
 *   scail_resid_store:  r[b,i,j] = bf16(float(h_out[b,i,j]) - float(h_in[b,i,j]))
 *   scail_resid_apply:  h[b,i,j] = bf16(float(h_in[b,i,j]) + float(r[b,i,j]))
 * ONE fp32 operation and ONE rounding to nearest even per element, like scail_f32_to_bf16 and with its conventions: denormals are kept,
 * not flushed; a NaN stays a NaN (inf - inf and inf + -inf give one); an fp32 result beyond the largest bf16 rounds to inf.  in_bs may be 0:
 * ONE h_in for every b (the embedded tokens of a classifier-free-guidance pair exist once).  A row window of a larger matrix is passed
 * as the pointer to its first row.
 * In place: scail_resid_apply accepts h == h_in with in_bs == h_bs, and h == h_in with in_bs == 0 (element 0 is both the input of every
 * element and an output).  One thread owns an 8-column chunk of EVERY element: it reads h_in's chunk before it writes h's (in_bs == 0:
 * once, before its first write), and no other thread touches that chunk of any element.  Any other overlap of h and h_in is refused.
 * Both are bandwidth-bound streaming passes: 16-byte loads and stores, at most 2048 workgroups with a grid-stride loop.
 * Checked on the host before any launch, with an error that names the value: n_batch outside 0..64, rows outside 0 .. 2^31 - 1,
 * D % 8 != 0 or D outside 8 .. 2^20 - 8, a batch stride that is negative or no multiple of 8, h_bs below rows * D with n_batch > 1 (the output elements would
 * overlap), a null or not 16-byte aligned base pointer, an overlap of h and h_in other than the two above.  scail_resid_store's r must not
 * overlap its inputs (not checked).  n_batch == 0 or rows == 0 is accepted and launches nothing.
 */
int scail_resid_store(const scail_bf16* h_out, int64_t out_bs, const scail_bf16* h_in, int64_t in_bs, scail_bf16* r,
                      int64_t n_batch, int64_t rows, int64_t D, void* stream);
int scail_resid_apply(const scail_bf16* h_in, int64_t in_bs, const scail_bf16* r, scail_bf16* h, int64_t h_bs,
                      int64_t n_batch, int64_t rows, int64_t D, void* stream);

/*
 * scail_abs_diff_sums: out[0] = sum_j |a_j - b_j|, out[1] = sum_j |b_j| for fp32 a, b [n]; out = device fp64 [2], overwritten.  Every a_j
 * and b_j is widened to fp64 before the subtraction, so a term carries no fp32 rounding.  ONE launch of ONE workgroup (n is a few 10^4
 * at most where the library uses it: the 6 D modulation values of two timesteps, scail_dit.h scail_dit_time_distances): thread t of 256
 * adds its terms j = t, t + 256, .. in ascending order, then a binary tree joins the 256 partial sums.  The order is fixed by n alone
 * and there are no floating-point atomics: the same inputs give the same bits, as scail_rel_err_rows promises.  n == 0 writes {0, 0}.
 * Errors before the launch: n outside 0 .. 2^31 - 1 (named), out null or not 8-byte aligned, a or b null with n > 0 or not 4-byte aligned.
 */
int scail_abs_diff_sums(const float* a, const float* b, int64_t n, double* out, void* stream);

/* ---- fp8 per-token GEMMs (OCP e4m3fn, one fp32 scale per row of each operand) -------------------------------------------
 * scail_quant_fp8_rows: q[r, c] (uint8 e4m3 codes, row stride ldq) and s[r] from bf16 x[r, c] (row stride ldx), per row:
 *   amax = max |x|;  amax == 0: s = 1, q = 0;  else s = amax / 448, q = e4m3_rne(clamp(x * (448 / amax), -448, 448)) (fp32 math).
 *   cols % 8 == 0; x 16-byte, q 8-byte aligned.  Serves activations (per token) and weights (per output channel, [N, K] rows).
 * scail_gemm_fp8: y[M,N] = epilogue(acc[m,n] * sx[m] * sw[n] + bias[n]), acc = x[M,K] . W[N,K]^T of the e4m3 codes in fp32 on the
 *   block-scaled MFMA (unit block scales), bf16 out; epilogue SCAIL_EPI_BIAS / _GELU_TANH / _RESID as for scail_gemm_bf16 (resid may
 *   alias y; gate[(m / rows_per_batch) * gate_stride + n] or NULL).  Any M >= 1, N % 128 == 0, K % 128 == 0, lda % 16 == 0; W rows
 *   are K apart.  Other shapes are refused before any launch.
 */
int scail_quant_fp8_rows(const scail_bf16* x, int64_t ldx, uint8_t* q, int64_t ldq, float* s, int64_t rows, int64_t cols, void* stream);
int scail_gemm_fp8(const uint8_t* x, int64_t lda, const float* sx, const uint8_t* w, const float* sw, const float* bias,
                   scail_bf16* y, int64_t ldc, int64_t M, int64_t N, int64_t K, int epilogue,
                   const scail_bf16* resid, int64_t ldr, const float* gate, int64_t gate_stride,
                   int64_t rows_per_batch, void* stream);

/* ---- the same GEMMs with MX block scales (OCP MX: e4m3 codes + one E8M0 byte per aligned block of 32 along K) ------------------
 * scail_quant_mxfp8_rows: q[r, c] (uint8 e4m3 codes, row stride ldq) and e[r, c / 32] (uint8 E8M0, plain row-major, row stride lde) from
 *   bf16 x[r, c] (row stride ldx).  Per aligned block of 32 columns, bit-exact for finite input:
 *     amax = max |x|;
 *     amax == 0 (-0 included): byte 127 and 32 codes 0x00;
 *     else s = the smallest integer with amax * 2^-s <= 448, clamped to [-127, 127]: with amax = m * 2^E, 1 <= m < 2, s = E - 8 if
 *       m <= 1.75, else E - 7 (the exponent that never clips; floor(log2 amax) - 8 would saturate maxima in (448, 512) * 2^s);
 *     byte = s + 127 (never 255);  q = e4m3fn_rne(clamp(x * 2^-s, -448, 448)).
 *   The multiplication by a power of two is exact in fp32; the clamp never binds for finite bf16 input and stays as the guard against
 *   the NaN code.  A -0 element of a non-zero block keeps its sign bit, as in scail_quant_fp8_rows.  Non-finite input: unspecified.
 *   The row is read once.  cols % 32 == 0, ldx % 8 == 0, ldq % 8 == 0, lde >= cols / 32; x 16-byte, q 8-byte aligned.
 * scail_gemm_mxfp8: y[M,N] = epilogue(sum_b 2^(ex[m,b] + ew[n,b] - 254) * sum_{k in b} xq[m,k] wq[n,k] + bias[n]), b = the blocks of
 *   32 along K; the scales are the MFMA's scale operands, the epilogue applies none.  ex is [M, K / 32] with row stride ldex (a multiple
 *   of 4), ew is [N, K / 32] with row stride K / 32; both 4-byte aligned.  Everything else (shapes, epilogues, tile mapping, the
 *   alignment of x, w, bias, y, resid, gate) as scail_gemm_fp8; a block lies inside a row, so an output row depends on its own input
 *   row alone here too.  Other shapes are refused before any launch.
 */
int scail_quant_mxfp8_rows(const scail_bf16* x, int64_t ldx, uint8_t* q, int64_t ldq, uint8_t* e, int64_t lde, int64_t rows, int64_t cols,
                           void* stream);
int scail_gemm_mxfp8(const uint8_t* x, int64_t lda, const uint8_t* ex, int64_t ldex, const uint8_t* w, const uint8_t* ew, const float* bias,
                     scail_bf16* y, int64_t ldc, int64_t M, int64_t N, int64_t K, int epilogue,
                     const scail_bf16* resid, int64_t ldr, const float* gate, int64_t gate_stride,
                     int64_t rows_per_batch, void* stream);

/* ---- the same GEMMs on 6-bit operands (OCP MXFP6 e2m3: packed 6-bit codes + one E8M0 byte per aligned block of 32 along K) -----
 * Format: 1 sign, 2 exponent (bias 1), 3 mantissa bits, code = sign << 5 | exp << 3 | man; no infinity, no NaN.  Magnitudes: 0,
 *   0.125 .. 0.875 (exp 0, subnormal, man / 8), 1 .. 1.875 by 0.125, 2 .. 3.75 by 0.25, 4 .. 7.5 by 0.5.
 * Packing: a block of 32 codes is 24 bytes; code j of the block occupies bits [6 j, 6 j + 6) of the block's little-endian 192-bit
 *   string (bit i of the string = bit i % 8 of byte i / 8).  A row of K elements is 3 K / 4 bytes, block b at byte 24 b; leading
 *   dimensions of packed matrices are in BYTES.  This is also the order in which the MFMA reads a lane's 6 operand registers.
 * scail_quant_mxfp6_rows: q (packed codes, row stride ldq bytes) and e[r, c / 32] (uint8 E8M0, row stride lde) from bf16 x[r, c] (row
 *   stride ldx).  Per aligned block of 32 columns, bit-exact:
 *     amax = max |x| over the block's non-NaN elements;
 *     amax == 0 (-0 included, or every element NaN): byte 127 and 32 codes 0x00;
 *     else s = the smallest integer with amax * 2^-s <= 7.5, clamped to >= -127: with amax = m * 2^E, 1 <= m < 2, s = E - 2 if
 *       m <= 1.875, else E - 1;  byte = s + 127 (at most 253);  q = e2m3_rne(clamp(x * 2^-s, -7.5, 7.5)), ties to even.
 *   The multiplication by a power of two is exact in fp32 and the clamp never binds for finite input.  A -0 element, or one that
 *   rounds to zero, keeps its sign bit (code 0x20) in a non-zero block.  Non-finite input: an infinity counts as 2^128 in the amax
 *   (byte 253: the block's finite elements keep their exact scaled values, nearly all rounding to zero) and becomes +-7.5 (0x1f / 0x3f);
 *   a NaN is left out of the amax and becomes code 0x00 -- the format has no code for it, and a zero adds nothing to a product.
 *   The row is read once.  cols % 32 == 0, ldx % 8 == 0, ldq >= 3 cols / 4 and ldq % 4 == 0, lde >= cols / 32; x 16-byte, q 4-byte aligned.
 * scail_gemm_mxfp6: y[M,N] = epilogue(sum_b 2^(ex[m,b] + ew[n,b] - 254) * sum_{k in b} xq[m,k] wq[n,k] + bias[n]) on the packed codes,
 *   v_mfma_scale_f32_32x32x64_f8f6f4 with 6-bit operands.  x rows are lda BYTES apart (lda >= 3 K / 4, lda % 16 == 0), W rows 3 K / 4
 *   bytes; ex, ew, epilogues, tile mapping, alignment and shape limits (M >= 1, N % 128 == 0, K % 128 == 0) as scail_gemm_mxfp8.  An
 *   output row depends on its own input row alone.  Other shapes are refused before any launch.
 */
int scail_quant_mxfp6_rows(const scail_bf16* x, int64_t ldx, uint8_t* q, int64_t ldq, uint8_t* e, int64_t lde, int64_t rows, int64_t cols,
                           void* stream);
int scail_gemm_mxfp6(const uint8_t* x, int64_t lda, const uint8_t* ex, int64_t ldex, const uint8_t* w, const uint8_t* ew, const float* bias,
                     scail_bf16* y, int64_t ldc, int64_t M, int64_t N, int64_t K, int epilogue,
                     const scail_bf16* resid, int64_t ldr, const float* gate, int64_t gate_stride,
                     int64_t rows_per_batch, void* stream);

/*
 * scail_rel_err_rows: how far the bf16 matrix b [rows, cols] (row stride ldb) is from a (row stride lda), added to the device
 * accumulator acc (fp64 [4], owned and zeroed by the caller).  Per row r, in fp32 with every operation rounded on its own:
 *   err_r = sum_c (b[r, c] - a[r, c])^2,  pow_r = sum_c a[r, c]^2,  ratio_r = err_r / pow_r (an fp32 division; pow_r == 0: 0 if
 *   err_r == 0, else +inf)
 * and then, in fp64:  acc[0] += sum_r err_r;  acc[1] += sum_r pow_r;  acc[2] = max(acc[2], max_r ratio_r);  acc[3] += rows.
 * sqrt(acc[0] / acc[1]) is the relative Frobenius error of b against a over every call so far, sqrt(acc[2]) the worst row's.
 * The order of every sum is fixed by (rows, cols) alone (lanes and 2048-column chunks of a row; rows in ascending order inside one of at
 * most 1024 workgroup ranges, the ranges in ascending order) and there are no floating-point atomics: the same inputs give the same bits.
 * A NaN ratio (a non-finite element) is kept by the maximum.  16-byte loads: cols % 8 == 0, lda % 8 == 0, ldb % 8 == 0, a and b 16-byte
 * aligned; checked on the host before any launch.  rows == 0 is accepted and launches nothing.  The per-workgroup partial sums are kept
 * in device memory of the library: calls on one device must be ordered among themselves (one stream, or events).
 */
int scail_rel_err_rows(const scail_bf16* a, int64_t lda, const scail_bf16* b, int64_t ldb, double* acc, int64_t rows, int64_t cols,
                       void* stream);

/* ---- request preprocessing (data_video.py:141-170 resize_for_rectangle_crop, sample_video.py:340-351) -----------------------
 * scail_resize_crop_aa: separable ANTIALIASED bicubic resize of n images to the virtual size Hr x Wr, of which only the window
 *   [top, top + Hout) x [left, left + Wout) is computed (the centre crop, fused).  Cubic a = -0.5, align_corners = False -- the weights
 *   of ATen's _upsample_bicubic2d_aa and of Pillow.  Per axis, with s = in / out, sup = 2 * max(s, 1), c = s * (i + 0.5) for output index
 *   i of the RESIZED image: taps j in [max(0, floor(c - sup + 0.5)), min(in, floor(c + sup + 0.5))), weights
 *   k((j - c + 0.5) / max(s, 1)) normalised by their sum; evaluated in the kernel in fp64 and rounded to fp32 once (no device tables, no
 *   copy, no synchronisation).  Horizontal pass first, fp32 intermediate, each pass a left-to-right fused-multiply-add chain over its taps.
 *     src_kind SCAIL_SRC_U8_NHWC  uint8 channels-last (n, Hin, Win, C) (what the video loader returns); the result is rounded
 *                                 half-to-even and clamped to [0, 255]: the uint8 round trip of the reference's torchvision resize,
 *                                 held in fp32;
 *              SCAIL_SRC_F32_NCHW fp32 planar (n, C, Hin, Win) (the reference image in [-1, 1]); not rounded.
 *     dst      fp32 planar (n, C, Hout, Wout), dense.
 *   Scale cap: in / out <= SCAIL_RESIZE_MAX_SCALE on each axis (at most 4 * 16 + 1 = 65 taps per axis in the kernel's weight tables;
 *   2160 -> 256 is 8.44).  Errors, found on the host before any launch and naming the value: null pointers, an unknown src_kind, C outside
 *   1..4, a window outside Hr x Wr, a scale above the cap, a frame of 2^31 or more samples.  n == 0 is accepted and launches nothing.
 * scail_pose_half: one pass over the rounded pixels x fp32 (n, C, H, W), H and W even:
 *     p    = (x - 127.5) / 127.5                                                  (every operation rounded on its own: torch's bits)
 *     half[f * half_frame_stride + c * half_chan_stride + y * (W / 2) + x] = ((a + b) + (c + d)) * 0.25
 *            a, b = p[2y, 2x], p[2y, 2x + 1];  c, d = p[2y + 1, 2x], p[2y + 1, 2x + 1], in fp32 in exactly this order
 *            (the 0.5x bilinear with align_corners = False: the mean of each 2 x 2 block)
 *     full (n, C, H, W) dense = p when full != NULL.
 *   The strides (elements, each at least (H / 2) * (W / 2)) let a chunk of frames land in its slot of a (C, T, H / 2, W / 2) tensor:
 *   frame stride (H / 2) * (W / 2), channel stride T * (H / 2) * (W / 2), half pointing at frame t0 of channel 0.  x and full 8-byte aligned.
 */
#define SCAIL_SRC_U8_NHWC 0
#define SCAIL_SRC_F32_NCHW 1
#define SCAIL_RESIZE_MAX_SCALE 16
int scail_resize_crop_aa(const void* src, int src_kind, float* dst, int64_t n, int64_t C, int64_t Hin, int64_t Win,
                         int64_t Hr, int64_t Wr, int64_t top, int64_t left, int64_t Hout, int64_t Wout, void* stream);
int scail_pose_half(const float* x, float* half, int64_t half_frame_stride, int64_t half_chan_stride, float* full, int64_t n,
                    int64_t C, int64_t H, int64_t W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCAIL_HIP_H */
