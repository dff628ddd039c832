/*
 * scail_dit.h -- network-level entry points of libscail_hip.so (seam B1: what
 * `OpenAIWrapper.forward -> DiffusionTransformer.forward` (wrappers.py:40-45, dit_video_crossattn_sc_xc.py:1452-1587)
 * amounts to for one sampler step), composed in C++ from the operator entry points of scail_hip.h.  No torch, no
 * Python: a C program holding device pointers can run the denoising loop with this header alone.
 *
 * Ownership: the caller owns every buffer (weights, inputs, outputs, workspace, conditioning cache); the handle
 * only keeps the configuration and COPIES OF THE POINTER TABLES (not of the weights).  All work is enqueued on the
 * hipStream_t passed last; there is no host synchronisation, so a step can be stream-captured into a hipGraph after
 * one warm-up call.  Return 0 / non-zero + scail_last_error().  Sequence-parallel ranks run the SAME executor through
 * scail_dit_step_sp / scail_dit_block_sp below: the kernels of a block are enqueued here and only the collectives of the per-layer
 * exchange are handed to the host through a callback (RCCL through torch.distributed in scail_amd/parallel.py; a C host calls
 * ncclAllToAll / ncclAllGather there).
 */
#ifndef SCAIL_DIT_H
#define SCAIL_DIT_H

#include "scail_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct scail_dit_config {
    int32_t hidden_size;       /* D, multiple of 128 */
    int32_t num_heads;         /* D / 128 */
    int32_t inner_hidden_size; /* FF */
    int32_t num_layers;
    int32_t text_dim;          /* 4096 for UMT5-XXL */
    int32_t clip_dim;          /* 1280 */
    int32_t time_freq_dim;     /* 256 */
    int32_t time_embed_dim;
    float layernorm_epsilon;   /* 1e-6 */
} scail_dit_config;

/* One transformer layer (reference state_dict keys in comments; W = bf16 [out,in], b / norm weights = fp32). */
typedef struct scail_dit_layer {
    const scail_bf16* qkv_w; const float* qkv_b;     /* transformer.layers.i.attention.query_key_value */
    const scail_bf16* o_w; const float* o_b;         /* ...attention.dense */
    const float* qn; const float* kn;                /* mixins.adaln_layer.query/key_layernorm_list.i.weight */
    const scail_bf16* cq_w; const float* cq_b;       /* ...cross_attention.query */
    const scail_bf16* co_w; const float* co_b;       /* ...cross_attention.dense */
    const float* cqn;                                /* mixins.adaln_layer.cross_query_layernorm_list.i.weight */
    const float* ln_w; const float* ln_b;            /* ...post_cross_attention_layernorm */
    const scail_bf16* w1; const float* b1;           /* ...mlp.dense_h_to_4h */
    const scail_bf16* w2; const float* b2;           /* ...mlp.dense_4h_to_h */
} scail_dit_layer;

typedef struct scail_dit_weights {
    const scail_bf16* patch_w; const float* patch_b; /* mixins.patch_embed.proj, [D,128] (80 real columns, zero padded) */
    const scail_bf16* pose_w; const float* pose_b;   /* mixins.patch_embed.proj_pose, same layout */
    const scail_bf16* time0_w; const float* time0_b; /* time_embed.0 [Dt, freq] */
    const scail_bf16* time2_w; const float* time2_b; /* time_embed.2 [Dt, Dt] */
    const scail_bf16* adaln_w; const float* adaln_b; /* adaln_projection.1 [6D, Dt] */
    const float* adaln_tables;                       /* mixins.adaln_layer.adaLN_modulations, [layers, 6D] */
    const float* final_table;                        /* mixins.final_layer.adaLN_modulation, [2D] */
    const scail_bf16* final_w; const float* final_b; /* mixins.final_layer.linear [64, D] */
    const scail_dit_layer* layers;                   /* [num_layers] */
} scail_dit_weights;

/* Step-invariant conditioning (text / CLIP keys and transposed values of every layer), produced by the host once per
 * request (scail_amd.dit.DiffusionTransformer._conditioning; dit...:1505-1515, 1116-1142). */
typedef struct scail_dit_cond {
    const scail_bf16* k_text;   /* [layers, B, Lt, D] */
    const scail_bf16* vt_text;  /* [layers, B, heads, 128, ceil64(Lt)] */
    const scail_bf16* k_clip;   /* [layers, Bc, Lc, D], Bc in {1, B} */
    const scail_bf16* vt_clip;  /* [layers, Bc, heads, 128, ceil64(Lc)] */
    int64_t Lt, Lc, Bc;
} scail_dit_cond;

typedef struct scail_dit scail_dit;

int scail_dit_create(const scail_dit_config* cfg, const scail_dit_weights* w, scail_dit** out);
void scail_dit_destroy(scail_dit* h);

/* Bytes of caller-provided device workspace one step needs for a (B, T, H, W) latent batch (-1: bad handle / shape). */
int64_t scail_dit_workspace_bytes(const scail_dit* h, int64_t B, int64_t T, int64_t H, int64_t W);

/*
 * One network evaluation: out[B,T,16,H,W] fp32 = DiT(x[B,T,16,H,W] fp32, timesteps[B] fp32 (= 1000 sigma), cond, ref, pose).
 *   ref bf16 [n_ref,1,16,H,W], pose bf16 [n_pose,T,16,H/2,W/2] (n_* in {1, B}: CFG repeat, dit...:1479-1495);
 *   rope_cos / rope_sin fp32 [L, 64] per-token pair tables for L = (1+T)(H/2)(W/2) + T(H/4)(W/4) tokens
 *   (scail_amd/rope.py; Rotary3DPositionEmbeddingMixin dit...:382-757);  workspace: scail_dit_workspace_bytes().
 *   flags: 0, or SCAIL_DIT_CFG_PAIR -- the caller states that this is the classifier-free-guidance pair of a sampler step
 *   (VanillaCFG.prepare_inputs, guiders.py:41-57: x = cat([x] * 2), s = cat([s] * 2)): B == 2, n_ref == n_pose == 1, and x[1] == x[0],
 *   timesteps[1] == timesteps[0]; only the conditioning differs.  The two elements' hidden states are then equal until the first cross
 *   attention of layer 0 (dit...:1009-1042), so the patch embedding and layer 0's LayerNorm -> QKV -> norm / RoPE -> self-attention ->
 *   out-projection run ONCE and are copied to element 1 (0.94 % of the 14B step).  Results are bit-identical to flags = 0 on such
 *   inputs (every kernel computes a row from that row alone); x[1] is not read.  The flag is a statement about the inputs, not
 *   checked on the device.  The last layer likewise evaluates only the rows the final layer reads (the noise tokens) past its K / V.
 */
#define SCAIL_DIT_CFG_PAIR 1u
int scail_dit_step(scail_dit* h, const float* x, const float* timesteps, const scail_dit_cond* cond,
                   const scail_bf16* ref, int64_t n_ref, const scail_bf16* pose, int64_t n_pose,
                   const float* rope_cos, const float* rope_sin, float* out,
                   int64_t B, int64_t T, int64_t H, int64_t W, uint32_t flags, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * ---- more than one character (an EXTENSION, BASELINE config 5: the reference has one reference frame and one pose stream, dit...:1559) ----
 * Naming scheme: every network-level entry point NAME has a form NAME_chars (scail_dit_X_workspace_bytes -> scail_dit_X_chars_workspace_bytes)
 * that takes the character count n_char = C in 1..64 -- and, where a pose tensor is passed, its frame count pose_frames -- right after the
 * pose arguments (the workspace queries: last).  The entry points without the suffix ARE the n_char == 1 forms: they forward with
 * n_char = 1, pose_frames = T and keep their single-character kernel (scail_patchify), results and signatures.
 *   ref  bf16 [n_ref, C, 16, H, W];  pose bf16 [n_pose, pose_frames = C*T, 16, H/2, W/2] (character k = frames kT .. (k+1)T - 1)
 *   tokens  [ref_0 .. ref_{C-1} | noise | pose_0 .. pose_{C-1}]:  Lref = C (H/2)(W/2), Lnoise = T (H/2)(W/2), Lpose = C T (H/4)(W/4),
 *           Ltok = Lref + Lnoise + Lpose; the noise rows are [Lref, Lref + Lnoise).  Assembled by ONE scail_patchify_chars launch.
 *   rope_cos / rope_sin fp32 [Ltok, 64] from the host in that token order (scail_amd/rope.py build_tables(n_char = C): character k takes RoPE
 *           windows the reference leaves unused).
 * Everything that is a row window follows these lengths: patch_w embeds the ref + noise rows and pose_w the pose rows, the last layer runs
 * past its K / V on the noise rows only, the final layer reads the noise rows.  SCAIL_DIT_CFG_PAIR has the same precondition as for C == 1
 * (B == 2, n_ref == n_pose == 1, equal latents and timesteps).  The fp8 GEMMs work on the single-rank calls; the sequence-parallel calls
 * refuse them as before.  A sequence-parallel rank's slab holds its H- or W-window of EVERY character's reference frame and pose stream (ref
 * and pose sliced like the latent), so its token rows are the layout above for the slab: the exchange layouts do not change.
 * Checked before anything is enqueued, with an error that names the value: n_char outside 1..64, pose_frames != n_char * T, and
 * ranks * Ltok >= 2^31 - 64 (the attention launch takes ceil64(keys) < 2^31).
 * Kernel choice of the self-attention at large Ltok: the 4-wave kernel scail_attn4_m16f addresses each operand with 32-bit byte offsets,
 * rows * row stride < 2^30 elements; beyond that the launch runs the about 2x slower 8-wave kernel, with the same result.  With D = 5120:
 *   one rank   (q, k rows of the fused [Ltok, 3D] projection)  Ltok < 69 906: config 5 (C = 2, L = 60 032) fits; C = 3 at the same latent
 *              (L = 71 232) runs the 8-wave kernel
 *   all-gather (keys: the gathered [ranks * Ltok, 2D] rows)    ranks * Ltok = full L < 104 858, and Ltok < 69 906 per rank
 *   ulysses    (q, k rows of [ranks * Ltok, 3D / ranks])       Ltok < 69 906 per rank, i.e. full L < ranks * 69 906
 * (scail_flash_attn_kernel_name_for answers for a given launch, by kernel name; scail_flash_attn_kernel_for for one (batch, head) pair of it.)
 */
int64_t scail_dit_chars_workspace_bytes(const scail_dit* h, int64_t B, int64_t T, int64_t H, int64_t W, int64_t n_char);
int scail_dit_step_chars(scail_dit* h, const float* x, const float* timesteps, const scail_dit_cond* cond,
                         const scail_bf16* ref, int64_t n_ref, const scail_bf16* pose, int64_t n_pose, int64_t n_char, int64_t pose_frames,
                         const float* rope_cos, const float* rope_sin, float* out,
                         int64_t B, int64_t T, int64_t H, int64_t W, uint32_t flags, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * Seam B2 (the SAT hook `layer_forward`, dit...:1009-1051): ONE transformer block, in place on caller-owned hidden states
 * hidden bf16 [B, Ltok, D].  mod fp32 [B, 6D] = adaLN embedding + this layer's table (shift_a|scale_a|gate_a|shift_m|scale_m|gate_m);
 * cond / rope tables as for scail_dit_step (cond is indexed by `layer`).
 */
int64_t scail_dit_block_workspace_bytes(const scail_dit* h, int64_t B, int64_t Ltok);
int scail_dit_block(scail_dit* h, int64_t layer, scail_bf16* hidden, const float* mod, const scail_dit_cond* cond,
                    const float* rope_cos, const float* rope_sin, int64_t B, int64_t Ltok,
                    void* workspace, int64_t workspace_bytes, void* stream);

/*
 * ---- sequence-parallel execution (reference: DeepSpeed-Ulysses, sat/mpu/ulysses_attn_layer.py:41-110, all_to_all.py:15-108,
 * with the latent split and rank-shifted RoPE of diffusion_video.py:495-585 and dit...:1578-1585) ----------------------------------------
 * Each rank holds an aligned token slab (B, Ltok, D) of [ref | noise | pose] tokens.  A block is per-token except for the self-attention,
 * whose exchange comes in two modes:
 *   SCAIL_SP_ULYSSES    q, k, v head <-> sequence all-to-all after norm + RoPE -- ONE collective for the three (the reference: three,
 *                       ulysses_attn_layer.py:65-80) --, attention over the FULL sequence for heads / ranks heads, one all-to-all back
 *                       (heads % ranks == 0).  Buffers (bf16, caller-owned, contiguous):
 *                         send, recv  [B][ranks][Ltok][3 * D / ranks] (send: one message per destination rank, q | k | v of that rank's heads side
 *                                                                       by side in a row; recv: per source rank, i.e. one (ranks * Ltok, 3 D / ranks)
 *                                                                       matrix in rank-major token order whose column thirds are q, k, v)
 *                         ofull, back [B][ranks][Ltok][D / ranks]      (attention output of all tokens for my heads; my tokens for all head groups)
 *   SCAIL_SP_ALLGATHER  ONE exchange: all-gather of the post-RoPE K rows and of the V rows as ONE collective.  Buffers:
 *                         send [B][Ltok][2 D] (k | v side by side),  recv [B][ranks][Ltok][2 D];  ofull / back unused (NULL).
 * The executor enqueues every kernel and calls `exchange` where a collective has to be started or awaited:
 *   SCAIL_SP_FWD_START   element b's send buffers are complete on `stream` (stream order): start its forward collectives
 *                        (ulysses: all-to-all send[b] -> recv[b] with equal splits; allgather: all-gather send[b] -> recv[b]): 2 collectives per
 *                        element and layer in ulysses mode (this one + the way back), 1 in all-gather mode
 *   SCAIL_SP_FWD_WAIT    make `stream` wait for them (the kernels enqueued next read recv[b])
 *   SCAIL_SP_BACK_START  ulysses: ofull[b] is complete on `stream`: start the all-to-all ofull[b] -> back[b]
 *   SCAIL_SP_BACK_WAIT   make `stream` wait for it
 * Per layer the order of the calls is START(0), START(1), .., WAIT(0), [BACK_START(0)], WAIT(1), [BACK_START(1)], .., [BACK_WAIT(0), ..] on every
 * rank, so collectives are enqueued in the same order everywhere (with SCAIL_DIT_CFG_PAIR layer 0 exchanges element 0 only).  A non-zero
 * return aborts the step (status 3): the side streams are still joined back into `stream`, so work already enqueued stays ordered before
 * whatever the caller enqueues next, but collectives the peers started are left unmatched -- after a status 3 the caller must tear down
 * (abort) the communicator.  The callback runs on the calling thread, between launches; it must not synchronise the device if the step is
 * to stay asynchronous.
 * side_stream: both NULL = everything on `stream`.  Two streams: the two CFG elements' launches of the ulysses exchange section go to
 * side_stream[b & 1] (forked from / joined to `stream` with events inside the call): an element's rank-sized launches leave a partial last
 * round of the chip that the other element's kernels fill (pays up to 4 ranks).
 */
#define SCAIL_SP_ALLGATHER 0
#define SCAIL_SP_ULYSSES 1
#define SCAIL_SP_FWD_START 0
#define SCAIL_SP_FWD_WAIT 1
#define SCAIL_SP_BACK_START 2
#define SCAIL_SP_BACK_WAIT 3
typedef int (*scail_sp_exchange_fn)(void* user, int32_t op, int32_t layer, int32_t element, void* stream);
typedef struct scail_dit_sp {
    int32_t ranks;              /* group size, >= 2 */
    int32_t mode;               /* SCAIL_SP_ALLGATHER | SCAIL_SP_ULYSSES */
    scail_bf16* send;
    scail_bf16* recv;
    scail_bf16* ofull;
    scail_bf16* back;
    scail_sp_exchange_fn exchange;
    void* user;
    void* side_stream[2];
} scail_dit_sp;

/* One network evaluation on this rank's latent slab x [B,T,16,H,W] (H or W = the full extent / ranks; ref / pose sliced alike; rope tables
 * of the slab's tokens with the rank's window shift, scail_amd/rope.py): scail_dit_step with the self-attention exchanged as above.
 * out = this rank's slab of the result.  workspace >= scail_dit_sp_workspace_bytes (the V^T staging buffer holds ALL ranks' keys).
 * flags as for scail_dit_step.  The last layer evaluates the rank's noise rows only past its K / V exchange (all-gather: their queries too;
 * ulysses: the full-sequence attention keeps every query, its rows are rank-major). */
int64_t scail_dit_sp_workspace_bytes(const scail_dit* h, int32_t mode, int32_t ranks, int64_t B, int64_t T, int64_t H, int64_t W);
int scail_dit_step_sp(scail_dit* h, const float* x, const float* timesteps, const scail_dit_cond* cond,
                      const scail_bf16* ref, int64_t n_ref, const scail_bf16* pose, int64_t n_pose,
                      const float* rope_cos, const float* rope_sin, float* out,
                      int64_t B, int64_t T, int64_t H, int64_t W, const scail_dit_sp* sp, uint32_t flags, void* workspace, int64_t workspace_bytes,
                      void* stream);

/* scail_dit_step_sp for n_char characters ("more than one character" above). */
int64_t scail_dit_sp_chars_workspace_bytes(const scail_dit* h, int32_t mode, int32_t ranks, int64_t B, int64_t T, int64_t H, int64_t W,
                                           int64_t n_char);
int scail_dit_step_sp_chars(scail_dit* h, const float* x, const float* timesteps, const scail_dit_cond* cond,
                            const scail_bf16* ref, int64_t n_ref, const scail_bf16* pose, int64_t n_pose, int64_t n_char, int64_t pose_frames,
                            const float* rope_cos, const float* rope_sin, float* out,
                            int64_t B, int64_t T, int64_t H, int64_t W, const scail_dit_sp* sp, uint32_t flags, void* workspace,
                            int64_t workspace_bytes, void* stream);

/* Seam B2 for a sequence-parallel rank: ONE transformer block in place on this rank's hidden [B, Ltok, D] (scail_dit_block + the exchange). */
int64_t scail_dit_block_sp_workspace_bytes(const scail_dit* h, int32_t mode, int32_t ranks, int64_t B, int64_t Ltok);
int scail_dit_block_sp(scail_dit* h, int64_t layer, scail_bf16* hidden, const float* mod, const scail_dit_cond* cond,
                       const float* rope_cos, const float* rope_sin, int64_t B, int64_t Ltok, const scail_dit_sp* sp,
                       void* workspace, int64_t workspace_bytes, void* stream);

/*
 * Timing of the executor's own launches with HIP events recorded on the launch stream (what bench.py's `roofline` objects are computed
 * from: the timed thing is the product path itself, not an instrumented copy).  scail_dit_profile(h, 1): every following scail_dit_step
 * / scail_dit_block / scail_dit_sample brackets each launch of the categories below with an event pair (events are pooled in the
 * handle; counters restart); scail_dit_profile(h, 0) stops.  scail_dit_profile_read waits for the recorded events and returns the summed
 * kernel time in ms and the number of launches of one category since the last enable.  With side streams (scail_dit_sp.side_stream) the
 * two elements' launches overlap, so the sum of a category is NOT wall-exclusive there.  Off by default; do not enable inside a stream
 * capture (event records are not capturable into a replayable graph with readable timings).
 */
#define SCAIL_DIT_PROF_SELF_ATTN 0   /* scail_flash_attn_bf16 of the self-attention (dit...:1058-1105) */
#define SCAIL_DIT_PROF_GEMM 1        /* the six per-token GEMMs of a block: qkv, attention out, cross q, cross out, MLP up, MLP down */
#define SCAIL_DIT_PROF_CROSS_ATTN 2  /* scail_cross_attn2_bf16 (dit...:1107-1203) */
/* sequence-parallel steps: the EXPOSED part of the layer exchange -- the event pair brackets nothing but the launch stream's wait for
 * the collective (SCAIL_SP_FWD_WAIT / SCAIL_SP_BACK_WAIT), so its time is what the exchange adds to the step (0 when the collective
 * finished under the other CFG element's kernels); launches = waits.  An N-rank bench line carries both (bench.py `exchange_exposed`). */
#define SCAIL_DIT_PROF_XCH_FWD_WAIT 3
#define SCAIL_DIT_PROF_XCH_BACK_WAIT 4
/* not a time: `launches` = workgroups of the profiled self-attention launches that RESTARTED (the optimistic pass of scail_attn4_m16f
 * overflowed, scail_hip.h scail_flash_attn_count_restarts; a restarted workgroup costs about twice), ms_total = 0.  0 on random data;
 * on real weights it says whether the kernel's measured rate holds (bench.py `roofline.attn_restarts_per_launch`). */
#define SCAIL_DIT_PROF_ATTN_RESTARTS 5
int scail_dit_profile(scail_dit* h, int enable);
int scail_dit_profile_read(scail_dit* h, int category, double* ms_total, int64_t* launches);

/*
 * fp8 per-token GEMMs (opt-in; the default is bf16).  The selected GEMMs of every block run as scail_quant_fp8_rows on their input rows +
 * scail_gemm_fp8 (include/scail_hip.h: OCP e4m3, one fp32 scale per token and per output channel, so every output row still depends on its
 * own input row alone and SCAIL_DIT_CFG_PAIR / the last-layer row pruning stay exact) under scail_dit_step, scail_dit_block and
 * scail_dit_sample.  The patch embedding, the final layer, the time / AdaLN / conditioning projections and both attentions stay bf16.
 * scail_dit_enable_fp8 quantizes the selected per-layer matrices from the handle's bf16 weights into the caller's device buffer
 * buf (>= scail_dit_fp8_weight_bytes(h, which) bytes, 256-byte aligned; it must outlive the fp8 use), enqueued on `stream`; call it
 * outside stream capture.  A selected shape outside scail_gemm_fp8's limits (N, K multiples of 128) fails it up front, naming the shape.
 * which == 0 or buf == NULL: back to bf16.  Which of the quantised matrices run in fp8 can be narrowed per layer
 * (scail_dit_fp8_select_layers below).  While fp8 is enabled the workspace queries (scail_dit_workspace_bytes, _block_, _sample_)
 * include the e4m3 copy of a GEMM input, and scail_dit_step_sp / scail_dit_block_sp return an error (sequence-parallel ranks: bf16 only).
 * scail_dit_fp8_weight_bytes: -1 for a null handle or an unknown bit.
 */
#define SCAIL_DIT_FP8_QKV 1u    /* self-attention q | k | v projection */
#define SCAIL_DIT_FP8_O 2u      /* self-attention out-projection (gated residual) */
#define SCAIL_DIT_FP8_CQ 4u     /* cross-attention query projection */
#define SCAIL_DIT_FP8_CO 8u     /* cross-attention out-projection (residual) */
#define SCAIL_DIT_FP8_W1 16u    /* MLP up (GELU-tanh) */
#define SCAIL_DIT_FP8_W2 32u    /* MLP down (gated residual) */
#define SCAIL_DIT_FP8_ALL 63u
int64_t scail_dit_fp8_weight_bytes(const scail_dit* h, uint32_t which);
int scail_dit_enable_fp8(scail_dit* h, uint32_t which, void* buf, int64_t bytes, void* stream);
/*
 * Scaling of the fp8 GEMMs: one per handle, chosen at enable time.  SCAIL_DIT_FP8_SCALE_ROW is the scheme above; the two functions above
 * are the ROW forms of the two below.  SCAIL_DIT_FP8_SCALE_MX runs scail_quant_mxfp8_rows + scail_gemm_mxfp8 instead (include/scail_hip.h:
 * e4m3 codes with one E8M0 scale per aligned block of 32 along K, for activations and weights): an outlier then costs the 31 neighbours of
 * its block, not the rest of its row.  A block lies inside a row, so the row independence, SCAIL_DIT_CFG_PAIR and the last-layer pruning
 * hold as under ROW.  Under MX the caller's buffer holds [N, K / 32] scale bytes per matrix where ROW holds N floats
 * (scail_dit_fp8_weight_bytes_scaled), the block scratch holds rows x (widest fp8 K) / 32 scale bytes where ROW holds rows x 4, and every
 * workspace query answers for the scaling in force.  scail_dit_fp8_select_layers works unchanged and scail_dit_fp8_probe measures whichever
 * scaling is enabled, in the same table.  An unknown `scaling` is refused with a message that names it (weight_bytes_scaled: -1).
 * Switching back to bf16 (which == 0 or buf == NULL) also returns the handle to ROW.
 */
#define SCAIL_DIT_FP8_SCALE_ROW 0
#define SCAIL_DIT_FP8_SCALE_MX 1
int64_t scail_dit_fp8_weight_bytes_scaled(const scail_dit* h, uint32_t which, int scaling);
int scail_dit_enable_fp8_scaled(scail_dit* h, uint32_t which, int scaling, void* buf, int64_t bytes, void* stream);
/*
 * 6-bit per-token GEMMs (opt-in): the selected GEMMs run as scail_quant_mxfp6_rows + scail_gemm_mxfp6 (include/scail_hip.h: packed OCP
 * e2m3 codes with one E8M0 scale per aligned block of 32 along K, for activations and weights).  `which` takes the SCAIL_DIT_FP8_* bits.
 * A handle holds ONE quantised form: scail_dit_enable_fp6 replaces an fp8 form and scail_dit_enable_fp8[_scaled] replaces fp6; which == 0
 * or buf == NULL in any of them returns the handle to bf16.  The caller's buffer holds, per layer and selected GEMM in bit order, the
 * packed codes [N, 3 K / 4 bytes] then the scale bytes [N, K / 32], each 256-byte aligned (scail_dit_fp6_weight_bytes; -1 for a null
 * handle or an unknown bit); the block scratch holds rows x 3/4 (widest quantised K) code bytes and rows x (that K) / 32 scale bytes,
 * and every workspace query answers for the form in force.  Blocks lie inside a row: the row independence, SCAIL_DIT_CFG_PAIR and the
 * last-layer pruning hold.  scail_dit_fp8_select_layers and scail_dit_fp8_probe act on whichever quantised form is enabled; the
 * sequence-parallel calls refuse an fp6 handle as they refuse fp8.  This is not a third `scaling` of scail_dit_enable_fp8_scaled.
 */
int64_t scail_dit_fp6_weight_bytes(const scail_dit* h, uint32_t which);
int scail_dit_enable_fp6(scail_dit* h, uint32_t which, void* buf, int64_t bytes, void* stream);

/*
 * Per-layer fp8 selection and the on-device GEMM error probe (both opt-in, both on top of scail_dit_enable_fp8).
 * With per-token and per-channel scales one outlier channel of a GEMM input flushes the rest of that row to zero; the damage is local
 * to a few (layer, GEMM) pairs.  The probe finds them on the request's own activations, the selection keeps only them in bf16.
 *
 * scail_dit_fp8_select_layers: masks[num_layers] (host array, copied), masks[i] = the SCAIL_DIT_FP8_* bits in force in layer i.  Every
 *   masks[i] must be a subset of the mask given to scail_dit_enable_fp8 (only a quantised matrix can be selected): a bit outside it is an
 *   error that names the layer and the bit.  Nothing is re-quantised and the weight buffer is not touched; the executor decides per
 *   (layer, GEMM) which of the two kernels runs.  masks == NULL: uniform again (the enabled mask in every layer).  scail_dit_enable_fp8
 *   resets the selection (and turns the probe off).  The workspace queries keep using the enabled (union) mask.  SCAIL_DIT_CFG_PAIR and the
 *   last-layer row pruning stay exact under any selection: they only need every GEMM to compute a row from that row alone.
 *
 * scail_dit_fp8_probe: table = device fp64 [num_layers][6][4], zeroed by the caller; scratch = scail_dit_fp8_probe_bytes(h, B, Ltok)
 *   bytes of device memory, 256-byte aligned (two bf16 buffers of B * Ltok rows x the widest quantised N); both must outlive the probe.
 *   table == NULL turns the probe off.  While it is on, every single-rank call (scail_dit_step, _chars, scail_dit_block, scail_dit_sample*)
 *   does, for each GEMM whose weight is quantised -- in force or not --, on exactly the rows the real GEMM runs on:
 *     1. Y16 = bf16(x W^T + b) with scail_gemm_bf16, plain bias epilogue, into scratch;
 *     2. Y8 = the same with scail_quant_fp8_rows + scail_gemm_fp8, plain bias epilogue, into scratch;
 *     3. scail_rel_err_rows(Y16, Y8) into table[layer][g] (g = the bit index of SCAIL_DIT_FP8_*):
 *        [0] += sum |Y8 - Y16|^2, [1] += sum |Y16|^2, [2] = max over rows of the row's ratio, [3] += rows;
 *     4. the layer's real GEMM in bf16.
 *   So the network's result is the bf16 network's bit for bit and every probed activation is clean (no fp8 error upstream of it).
 *   sqrt([0] / [1]) is the relative error of that fp8 GEMM, sqrt([2]) its worst token's.  What is measured is the output of the
 *   bias-only GEMM: not what GELU makes of it, not the hidden state after the gated residual.  Cost: two extra GEMMs, one quantisation and
 *   one pass over both results per probed GEMM -- meant for ONE evaluation per request, after which the caller reads the table, selects
 *   layers and turns the probe off.  Nothing synchronises; the caller reads the table after the stream has finished.  A call with more
 *   rows (B * Ltok) than the scratch covers is refused before anything is enqueued.  Needs fp8 enabled; the sequence-parallel calls
 *   refuse such a handle as before.  Not meant for stream capture (scail_rel_err_rows keeps its partial sums in library memory).
 * scail_dit_fp8_probe_bytes: -1 for a null handle or a bad shape; 0 while no GEMM is quantised.
 */
int scail_dit_fp8_select_layers(scail_dit* h, const uint32_t* masks);
int64_t scail_dit_fp8_probe_bytes(const scail_dit* h, int64_t B, int64_t Ltok);
int scail_dit_fp8_probe(scail_dit* h, double* table, void* scratch, int64_t scratch_bytes);

/*
 * The whole Euler sampling loop of RFSampler (sampling.py:920-982) with VanillaCFG (guiders.py:41-57) for one request:
 *   for i < n_steps:  v = DiT([x; x], timesteps[i], cond [uncond | cond], ref, pose);  x += dsigma[i] (v_u + cfg (v_c - v_u))
 * x fp32 [1,T,16,H,W] in / out (device); timesteps DEVICE fp32 [n_steps][2] (= 1000 sigma_i, twice); dsigma HOST fp32
 * [n_steps] (= sigma_{i+1} - sigma_i); cond holds the batch-2 conditioning (index 0 = uncond, 1 = cond).
 * workspace >= scail_dit_sample_workspace_bytes(h, T, H, W), 256-byte aligned like the step's (a workspace that is too small or
 * misaligned is refused before anything is enqueued).  Nothing synchronises; the call returns once all steps are enqueued.
 */
int64_t scail_dit_sample_workspace_bytes(const scail_dit* h, int64_t T, int64_t H, int64_t W);
int scail_dit_sample(scail_dit* h, float* x, const float* timesteps, const float* dsigma, int64_t n_steps, float cfg_scale,
                     const scail_dit_cond* cond, const scail_bf16* ref, const scail_bf16* pose,
                     const float* rope_cos, const float* rope_sin, int64_t T, int64_t H, int64_t W,
                     void* workspace, int64_t workspace_bytes, void* stream);
/* The same loop for n_char characters: ref [1, n_char, 16, H, W], pose [1, pose_frames = n_char * T, 16, H/2, W/2]. */
int64_t scail_dit_sample_chars_workspace_bytes(const scail_dit* h, int64_t T, int64_t H, int64_t W, int64_t n_char);
int scail_dit_sample_chars(scail_dit* h, float* x, const float* timesteps, const float* dsigma, int64_t n_steps, float cfg_scale,
                           const scail_dit_cond* cond, const scail_bf16* ref, const scail_bf16* pose, int64_t n_char, int64_t pose_frames,
                           const float* rope_cos, const float* rope_sin, int64_t T, int64_t H, int64_t W,
                           void* workspace, int64_t workspace_bytes, void* stream);

/*
 * The sampling loop of RFSamplerLong (temporal tiling, sampling.py:986-1085) with VanillaCFG for one request: how this model family
 * samples a clip longer than the trained window.  The latent x fp32 [1,T,16,H,W] (device, in / out) is denoised in n_tiles >= 2 tiles of
 * Tt <= min(T, 64) frames each; tile k is the frames tile_frames[k][0 .. Tt-1] (any order, distinct inside a tile; every frame of [0, T)
 * in at least one tile) and has its own pose latent pose_tiles[k] (bf16 [Tt,16,H/2,W/2]: the VAE encoding of that window on its own).
 * With F = 16*H*W, per step i (scail_hip.h scail_tile_*):
 *   den = 0
 *   for k = 0 .. n_tiles-1, ascending:  xin = [x[f_k]; x[f_k]]                                                   scail_tile_gather
 *                                       v = scail_dit_step_chars(xin, timesteps[i], cond, ref, pose_tiles[k], B = 2, T = Tt, SCAIL_DIT_CFG_PAIR)
 *                                       d = v_u + cfg (v_c - v_u);  den[f_kj, e] = den[f_kj, e] + tile_w[k][j] * d   scail_tile_blend_acc
 *   x[f, e] = x[f, e] + dsigma[i] * (den[f, e] * inv_wsum[f])                                                    scail_tile_finish
 * every operation rounded on its own (no fused multiply-add), accumulation in ascending tile order: the bits of the host loop
 * (scail_amd/sampler.py RFSamplerLong.sample_hip).  The caller computes, in fp32, tile_w[k][j] = float(m_k) * w_j with the triangular
 * w_j = min(u, 2 - u), u = (j + 0.5) * 2 / Tt, and m_k = 1 for the first and last tile and 2 otherwise (the reference evaluates interior
 * tiles twice with equal inputs; here once, with that multiplicity), and inv_wsum[f] = 1 / sum of the tile_w that land on frame f.
 * timesteps DEVICE fp32 [n_steps][2], dsigma / tile_frames / tile_w / inv_wsum HOST arrays read during the call (their values travel in
 * kernel arguments: no host-to-device copy), rope_cos / rope_sin the tables of a Tt-frame clip, shared by every tile.
 * workspace >= scail_dit_sample_tiled_workspace_bytes(h, T, Tt, H, W) (-1: bad handle / shape, T >= 32768 or Tt outside 1..min(T, 64)) = the step workspace of (2, Tt, H, W) + the
 * xin / v pair + den.  Nothing synchronises; the call is capturable after one warm-up call.  fp8 GEMMs work as under scail_dit_step.
 * One character per request: tiles and the _chars forms are not combined.  Sequence-parallel ranks keep the host loop.
 * Refused before anything is enqueued, with an error that names the value: n_tiles < 2, T >= 32768, Tt outside 1..min(T, 64), a frame index outside
 * [0, T), an index repeated inside one tile, a frame covered by no tile, a non-finite or non-positive inv_wsum, a null pointer, a
 * workspace that is too small.
 */
int64_t scail_dit_sample_tiled_workspace_bytes(const scail_dit* h, int64_t T, int64_t Tt, int64_t H, int64_t W);
int scail_dit_sample_tiled(scail_dit* h, float* x, const float* timesteps, const float* dsigma, int64_t n_steps, float cfg_scale,
                           const scail_dit_cond* cond, const scail_bf16* ref, const scail_bf16* pose_tiles,
                           const int32_t* tile_frames, const float* tile_w, const float* inv_wsum, int64_t n_tiles, int64_t T, int64_t Tt,
                           const float* rope_cos, const float* rope_sin, int64_t H, int64_t W, void* workspace, int64_t workspace_bytes,
                           void* stream);

/*
 * ---- step cache (an EXTENSION, opt-in; the scheme the community calls TeaCache: reuse the block residual on skipped steps) ---------------
 * Over a run of adjacent sampler steps the 40 blocks change the hidden states by nearly the same amount.  A FILL evaluation is a full
 * evaluation that also keeps r = (hidden states after the last block) - (patch embedding), on the noise rows -- the only rows the final
 * layer reads, so r is [B, Lnoise, D], not [B, Ltok, D].  A REUSE evaluation adds that r to THIS step's freshly embedded noise rows and
 * runs the final layer: no block, no pose embedding.  Which steps reuse is the caller's plan; scail_dit_time_distances below gives the
 * signal the usual plan is made from (it depends on the sigma schedule alone, so the plan is known before the loop starts and the
 * sampler stays ONE call with no host synchronisation).  Nothing here changes an existing entry point, its launches, its workspace
 * query or its result.
 *
 * scail_dit_step_cache_bytes: bytes of the caller-owned, 256-byte aligned cache of a (B, T, H, W) evaluation (-1: null handle / bad
 *   shape, like the workspace queries).  Layout: r bf16 [B][Lnoise][D] at offset 0, Lnoise = T (H/2) (W/2) -- callers may read it --, then,
 *   from the next multiple of 256, FILL's copy of the embedded noise rows, bf16 [B][Lnoise][D] (the blocks work in place, so the
 *   embedding has to be kept aside until the residual is formed; under SCAIL_DIT_CFG_PAIR its first element serves both), rounded to
 *   256.  It does not depend on n_char, and the step / sample workspace queries do not change.
 *
 * scail_dit_step_cached: scail_dit_step_chars + (mode, cache, cache_bytes).
 *   SCAIL_DIT_CACHE_FILL   the evaluation of scail_dit_step_chars -- fp8 GEMMs, the probe and SCAIL_DIT_CFG_PAIR included; `out` is
 *                          bit-identical to it --, which additionally copies the noise rows [Lref, Lref + Lnoise) of the patch embedding into
 *                          the cache and, after the last block, stores r with scail_resid_store (scail_hip.h).  Under SCAIL_DIT_CFG_PAIR
 *                          the embedding exists once and serves both elements (batch stride 0).
 *   SCAIL_DIT_CACHE_REUSE  time and final-layer tables as usual; patchify; the patch GEMM on the noise rows only (once under
 *                          SCAIL_DIT_CFG_PAIR) -- every kernel computes a row from that row alone, so these are the bits of the full
 *                          embedding --; scail_resid_apply of r into every element's noise rows, in place; then the existing final layer:
 *                          scail_ln_modulate, the 64-column GEMM, scail_unpatchify.  No block runs, the pose GEMM does not run, `cond`
 *                          is not read (it may be NULL) and the cache is only read.
 *   That the cache was filled by a FILL of this handle with the same (B, T, H, W) is the caller's statement, like SCAIL_DIT_CFG_PAIR: it
 *   is not checked on the device.  A REUSE on a cache that was never filled adds whatever the buffer holds.
 *
 * scail_dit_sample_cached: scail_dit_sample_chars + (reuse, cache, cache_bytes).  reuse = HOST uint8 [n_steps], read during the call:
 *   step i runs in REUSE mode where reuse[i] == 1, else in FILL mode; the cache is that of (2, T, H, W).  The same loop otherwise: it only
 *   enqueues, nothing synchronises, and it is capturable on the same terms as scail_dit_sample.  An all-zero mask gives the bits of
 *   scail_dit_sample_chars.
 *
 * scail_dit_sample_tiled_cached: scail_dit_sample_tiled + (reuse, cache, cache_bytes): the step cache for clips longer than one window.
 *   The loop is scail_dit_sample_tiled's, exactly as stated there (gather, evaluation with SCAIL_DIT_CFG_PAIR, blend-accumulate in
 *   ascending tile order, one scail_tile_finish per step), except that the evaluation of tile k at step i is scail_dit_step_cached on
 *   tile k's OWN residual: in REUSE mode where reuse[i] == 1, else in FILL mode.  reuse = HOST uint8 [n_steps], read during the call, one
 *   plan for every tile (it depends on the sigma schedule and the weights alone).  An all-zero mask gives the bits of
 *   scail_dit_sample_tiled.  The workspace is that of scail_dit_sample_tiled (scail_dit_sample_tiled_workspace_bytes); nothing
 *   synchronises, the call is capturable on the same terms, and quantised GEMMs work as under scail_dit_step_cached.
 * scail_dit_sample_tiled_cache_bytes: bytes of its caller-owned, 256-byte aligned cache (-1: null handle, n_tiles outside 2..32767, Tt
 *   outside 1..64, bad H / W).  With R and E the two regions of the step cache of a (2, Tt, H, W) evaluation above -- R = E =
 *   2 * Lnoise * D * 2 bytes rounded up to 256, Lnoise = Tt (H/2) (W/2) -- it is NOT n_tiles step caches: FILL's copy of the embedded
 *   noise rows is dead once scail_resid_store has run, so all tiles share one.  Layout: slabs of r [n_tiles][R] from offset 0 -- slab k
 *   holds tile k's r bf16 [2][Lnoise][D] as its last FILL left it; callers may read it --, then one embedding region E:
 *       scail_dit_sample_tiled_cache_bytes = n_tiles * R + E        (against n_tiles * (R + E) for stacked step caches)
 *
 * Refused before anything is enqueued, with an error that names the value: a mode other than the two; a null cache, one smaller than
 * scail_dit_step_cache_bytes (tiled: scail_dit_sample_tiled_cache_bytes), one that is not 256-byte aligned; reuse == NULL with
 * n_steps > 0; reuse[0] != 0 (the first step has nothing to reuse); an entry other than 0 or 1.  The checks that need no handle come
 * first.  scail_dit_sample_tiled_cached also refuses everything scail_dit_sample_tiled refuses, in its wording, and n_tiles >= 32768.
 *
 * scail_dit_time_distances: for the DEVICE fp32 timesteps [n_steps] (= 1000 sigma_i) the handle's own time embedding of every step, by
 *   the very calls of a step (scail_timestep_embedding, scail_small_linear; scail_small_linear takes at most 8 rows, so in chunks of 8
 *   steps), and between consecutive steps out[i] = scail_abs_diff_sums(v_i, v_{i-1}) for i >= 1, out[0] = {0, 0}; out = DEVICE fp64
 *   [n_steps][2], so out[i][0] / out[i][1] is the relative L1 change of the signal from step i - 1 to step i.  signal 0: v = emb, the
 *   output of time_embed.2, [time_embed_dim]; signal 1: v = its AdaLN projection, [6 D] (what every block's modulation is made of).
 *   scratch >= scail_dit_time_distances_bytes(h, signal) bytes (-1: null handle / unknown signal), 256-byte aligned.  Nothing
 *   synchronises: the host reads the table after the stream has finished.  Refused before anything is enqueued: an unknown signal, n_steps
 *   outside 0 .. 2^20 - 1 (both named), a null handle / pointer, a scratch that is too small or misaligned.
 *
 * Out of scope, each because no *_cached entry point exists for it: the sequence-parallel calls (scail_dit_step_sp*), the per-block
 * seam (scail_dit_block*), and tiles with several characters (scail_dit_sample_tiled takes one character per request).
 */
#define SCAIL_DIT_CACHE_FILL 1
#define SCAIL_DIT_CACHE_REUSE 2
int64_t scail_dit_step_cache_bytes(const scail_dit* h, int64_t B, int64_t T, int64_t H, int64_t W);
int scail_dit_step_cached(scail_dit* h, const float* x, const float* timesteps, const scail_dit_cond* cond,
                          const scail_bf16* ref, int64_t n_ref, const scail_bf16* pose, int64_t n_pose, int64_t n_char, int64_t pose_frames,
                          const float* rope_cos, const float* rope_sin, float* out,
                          int64_t B, int64_t T, int64_t H, int64_t W, uint32_t flags, void* workspace, int64_t workspace_bytes,
                          int mode, void* cache, int64_t cache_bytes, void* stream);
int scail_dit_sample_cached(scail_dit* h, float* x, const float* timesteps, const float* dsigma, int64_t n_steps, float cfg_scale,
                            const scail_dit_cond* cond, const scail_bf16* ref, const scail_bf16* pose, int64_t n_char, int64_t pose_frames,
                            const float* rope_cos, const float* rope_sin, int64_t T, int64_t H, int64_t W,
                            void* workspace, int64_t workspace_bytes, const uint8_t* reuse, void* cache, int64_t cache_bytes, void* stream);
int64_t scail_dit_sample_tiled_cache_bytes(const scail_dit* h, int64_t n_tiles, int64_t Tt, int64_t H, int64_t W);
int scail_dit_sample_tiled_cached(scail_dit* h, float* x, const float* timesteps, const float* dsigma, int64_t n_steps, float cfg_scale,
                                  const scail_dit_cond* cond, const scail_bf16* ref, const scail_bf16* pose_tiles,
                                  const int32_t* tile_frames, const float* tile_w, const float* inv_wsum, int64_t n_tiles, int64_t T, int64_t Tt,
                                  const float* rope_cos, const float* rope_sin, int64_t H, int64_t W, void* workspace, int64_t workspace_bytes,
                                  const uint8_t* reuse, void* cache, int64_t cache_bytes, void* stream);
int64_t scail_dit_time_distances_bytes(const scail_dit* h, int signal);
int scail_dit_time_distances(scail_dit* h, const float* timesteps, int64_t n_steps, int signal, double* out, void* scratch,
                             int64_t scratch_bytes, void* stream);

/*
 * ---- guidance plan (an EXTENSION, opt-in: cond-only steps and a cached CFG delta) --------------------------------------------------------
 * A sampler step is one batch-2 evaluation, [x; x] under the uncond and the cond conditioning.  Two training-free schemes skip the uncond
 * half of a step: a guidance INTERVAL (guide only inside a sigma interval, run the cond branch alone outside it) and a cached CFG DELTA
 * (reuse v_c - v_u of the last guided step).  Which step does what is the caller's plan, known before the loop starts -- it depends on
 * the sigma schedule alone --, so the sampler stays ONE call with no host synchronisation.  Nothing here changes an existing entry point,
 * its launches, its workspace query or its result.  No plan is recommended: nothing has been measured on real weights.
 *
 * scail_dit_step_branch: ONE branch of the pair as an evaluation: scail_dit_step_chars with B = 1 and n_ref = n_pose = 1, whose
 *   conditioning is element `elem` of a `cond` that holds cond_batch elements (k_text [layers][cond_batch][Lt][D] and so on; a CLIP
 *   conditioning with Bc == 1 is shared as ever).  timesteps = ONE device float.  `out` has the bits of scail_dit_step_chars with B = 1 on a
 *   scail_dit_cond that holds that element's slices alone: quantised GEMMs and the last-layer row pruning included (every kernel computes
 *   a row from that row alone, and the conditioning is only addressed differently).  workspace >= scail_dit_chars_workspace_bytes(h, 1, T,
 *   H, W, n_char).  mode: 0 (no cache; cache may be NULL), SCAIL_DIT_CACHE_FILL or SCAIL_DIT_CACHE_REUSE on the step cache of the PAIR,
 *   scail_dit_step_cache_bytes(h, 2, T, H, W): the branch reads and writes slot `elem` of r ([2][Lnoise][D] at offset 0) and nothing of the
 *   other slot; FILL parks its copy of the embedded noise rows in slot `elem` of the embedding region, which is dead after the store.
 *   Refused before anything is enqueued, naming the value: cond_batch outside 1..8, elem outside [0, cond_batch), a mode other than the
 *   three, with a cache mode an elem above 1 and everything scail_dit_step_cached refuses about the cache.
 *
 * scail_dit_guidance_bytes: bytes of the caller-owned, 256-byte aligned delta buffer: fp32 [T * 16 * H * W], rounded up to 256 (-1: a bad
 *   shape, as the workspace queries answer).
 *
 * scail_dit_sample_guided: scail_dit_sample_chars + (guide, delta, delta_bytes) + optionally the step cache's (reuse, cache, cache_bytes);
 *   reuse == NULL: no step cache (cache is not read).  guide = HOST uint8 [n_steps], read during the call; step i does
 *     SCAIL_DIT_GUIDE_PAIR   today's step -- the batch-2 evaluation with SCAIL_DIT_CFG_PAIR and scail_cfg_euler (scail_hip.h) --, and
 *                            additionally scail_cfg_delta_store of its [v_u; v_c] into delta;
 *     SCAIL_DIT_GUIDE_DELTA  the cond branch alone, scail_dit_step_branch(elem 1 of 2) on x itself, then scail_cfg_euler_delta with the
 *                            stored delta: x += dsigma (v_c + (cfg - 1) delta);
 *     SCAIL_DIT_GUIDE_COND   the cond branch alone, then scail_cfg_euler_delta with delta == NULL: x += dsigma v_c, no guidance.
 *   The workspace is scail_dit_sample_chars_workspace_bytes' (the B = 1 layout lies inside the B = 2 one).  With a mask, a PAIR step is
 *   scail_dit_step_cached as in scail_dit_sample_cached, a DELTA or COND step scail_dit_step_branch(elem 1) in FILL mode (reuse[i] == 0)
 *   or REUSE mode.  The call only enqueues, nothing synchronises, and it is capturable on the same terms as scail_dit_sample.
 *   Bit for bit: an all-PAIR plan gives scail_dit_sample_chars' x (with a mask: scail_dit_sample_cached's); after a PAIR step delta holds
 *   v_c - v_u of that step; a plan of COND entries alone neither reads nor writes delta (it may be NULL).
 *   Refused before anything is enqueued, x and both buffers untouched, naming the value: an entry above 2 (index and value); a DELTA entry
 *   with no PAIR entry before it (index); while the plan holds a PAIR or DELTA entry, a delta buffer that is null, not 256-byte aligned
 *   or smaller than scail_dit_guidance_bytes; with a mask, everything scail_dit_sample_cached refuses, in its wording, and a step with
 *   reuse[i] == 1 whose entry does not evaluate the same elements as the last computing step j (PAIR goes with PAIR, DELTA or COND with
 *   DELTA or COND; both indices are named): a reusing step must find the residual slots its last FILL wrote.
 *
 * Cost: by executed FLOPs a branch evaluation is about half a pair evaluation; it does not share layer 0 with a twin as
 * SCAIL_DIT_CFG_PAIR does.  That is an expectation from the FLOP count, NOT a measurement (README "guidance plan" has what was measured).
 *
 * Out of scope, each refused by name in the Python layers: temporal tiles (scail_dit_sample_tiled*: a delta per tile is the natural
 * follow-up), the sequence-parallel calls, the per-block seam, dynamic thresholding and other guiders.
 */
#define SCAIL_DIT_GUIDE_PAIR 0
#define SCAIL_DIT_GUIDE_DELTA 1
#define SCAIL_DIT_GUIDE_COND 2
int scail_dit_step_branch(scail_dit* h, const float* x, const float* timesteps, const scail_dit_cond* cond, int64_t cond_batch, int64_t elem,
                          const scail_bf16* ref, const scail_bf16* pose, int64_t n_char, int64_t pose_frames,
                          const float* rope_cos, const float* rope_sin, float* out, int64_t T, int64_t H, int64_t W,
                          void* workspace, int64_t workspace_bytes, int mode, void* cache, int64_t cache_bytes, void* stream);
int64_t scail_dit_guidance_bytes(int64_t T, int64_t H, int64_t W);
int scail_dit_sample_guided(scail_dit* h, float* x, const float* timesteps, const float* dsigma, int64_t n_steps, float cfg_scale,
                            const scail_dit_cond* cond, const scail_bf16* ref, const scail_bf16* pose, int64_t n_char, int64_t pose_frames,
                            const float* rope_cos, const float* rope_sin, int64_t T, int64_t H, int64_t W,
                            void* workspace, int64_t workspace_bytes, const uint8_t* guide, void* delta, int64_t delta_bytes,
                            const uint8_t* reuse, void* cache, int64_t cache_bytes, void* stream);

/*
 * ---- solver plan (an EXTENSION, opt-in: a linear multistep solver in place of the Euler update) -------------------------------------------
 * Every other extension shortens a step; this one is about the NUMBER of steps.  Rectified flow: x_sigma = (1 - sigma) x0 + sigma eps,
 * the network gives v = eps - x0, the guided velocity is d = v_u + s (v_c - v_u) and Euler is x <- x + (sigma' - sigma) d.  The data
 * prediction at step i is D_i = x_i - sigma_i d_i.  With alpha = 1 - sigma, lambda = log(alpha / sigma), h_i = lambda_{i+1} - lambda_i and
 * r_i = h_{i-1} / h_i, DPM-Solver++(2M) for the step sigma_i -> sigma_{i+1} is
 *     x_{i+1} = (sigma_{i+1} / sigma_i) x_i - alpha_{i+1} expm1(-h_i) [D_i + (1 / (2 r_i)) (D_i - D_{i-1})],
 * and for this parametrisation -alpha_{i+1} expm1(-h_i) = 1 - sigma_{i+1} / sigma_i exactly.  So with rho = sigma_{i+1} / sigma_i every
 * step is x_{i+1} = a x_i + b D_i + c D_{i-1}: first order (a, b, c) = (rho, 1 - rho, 0), second order
 * (rho, (1 - rho)(1 + 1 / (2 r_i)), -(1 - rho) / (2 r_i)); a + b + c = 1.  First order is Euler mathematically, not in bits.  A step is
 * second order only where i >= 1 and lambda_{i-1}, lambda_i, lambda_{i+1} are finite: a schedule from sigma = 1 to sigma = 0 has steps
 * 0, 1 and the last one first order, and its last step is x = 0 x + 1 D.  A second-order step needs no further network evaluation: one
 * fp32 pass over the latent (scail_cfg_multistep, scail_hip.h) and one fp32 latent of history.  The coefficients depend on the sigma
 * schedule alone, so the plan exists before the loop and the sampler stays ONE call with no host synchronisation.  These entry points
 * take a coefficient TABLE, not a solver's name: scail_amd/sampler.py plan_solver makes the table ("dpmpp2m", and "dpm1" = first-order
 * rows everywhere); another solver of the form a x + b D_i + c D_{i-1} is host-only work.  Nothing here changes an existing entry point,
 * its launches, its workspace query or its result.  No step count is recommended: nothing has been measured on real weights.
 *
 * scail_dit_solver_bytes: bytes of the caller-owned, 256-byte aligned history buffer: fp32 [T * 16 * H * W], rounded up to 256 (-1: a bad
 *   shape: T, H or W outside 1..32767, H or W no multiple of 4).  For the tiled call T is the FULL latent's frame count.
 *
 * scail_dit_sample_solver: scail_dit_sample_chars + (sigma, coef, hist, hist_bytes).  sigma = HOST fp32 [n_steps], the steps' STARTING
 *   sigmas; coef = HOST fp32 [n_steps][3] = (a, b, c) per step; both are read during the call.  Step i is scail_dit_sample_chars' [x; x]
 *   copy and evaluation with SCAIL_DIT_CFG_PAIR, then scail_cfg_multistep(x, v, hist, n, cfg_scale, sigma[i], coef[i][0], coef[i][1],
 *   coef[i][2], use_prev = coef[i][2] != 0) in place of scail_cfg_euler; dsigma is checked as there and not used.  The workspace is
 *   scail_dit_sample_chars_workspace_bytes'.  hist need not be initialised: step 0 writes it before any step reads it; after the call it
 *   holds the last step's D.  The call only enqueues, nothing synchronises, and it is capturable on the same terms as scail_dit_sample.
 *
 * scail_dit_sample_tiled_solver: scail_dit_sample_tiled + the same four, hist being that of the FULL latent [T * 16 * H * W].  The loop is
 *   scail_dit_sample_tiled's, except that scail_tile_finish_multistep (scail_hip.h) finishes the step in place of scail_tile_finish: the
 *   update happens once per step, after the blend, so one history serves every tile.
 *
 * Both refuse before anything is enqueued, x and hist untouched, naming the index and the value: a sigma or a coefficient that is not
 * finite; coef[0][2] != 0 (step 0 has no history); a null sigma or coef with n_steps > 0; a hist that is null, not 256-byte aligned or
 * smaller than scail_dit_solver_bytes; and everything their Euler twins refuse, in the twins' wording.
 *
 * Cost: the pass moves 5 to 6 floats per latent element next to a network evaluation of seconds; it does not matter to the time of a
 * step.  What the feature is for is the step count (README "solver plan" has what was measured).
 *
 * Out of scope, each refused by name in the Python layers: a solver plan together with the step cache or the guidance plan (the natural
 * follow-up; it needs the pass to take v_c + g delta in place of [v_u; v_c]), the sequence-parallel calls, UniPC and other correctors.
 */
int64_t scail_dit_solver_bytes(int64_t T, int64_t H, int64_t W);
int scail_dit_sample_solver(scail_dit* h, float* x, const float* timesteps, const float* dsigma, int64_t n_steps, float cfg_scale,
                            const scail_dit_cond* cond, const scail_bf16* ref, const scail_bf16* pose, int64_t n_char, int64_t pose_frames,
                            const float* rope_cos, const float* rope_sin, int64_t T, int64_t H, int64_t W,
                            void* workspace, int64_t workspace_bytes, const float* sigma, const float* coef, void* hist, int64_t hist_bytes,
                            void* stream);
int scail_dit_sample_tiled_solver(scail_dit* h, float* x, const float* timesteps, const float* dsigma, int64_t n_steps, float cfg_scale,
                                  const scail_dit_cond* cond, const scail_bf16* ref, const scail_bf16* pose_tiles,
                                  const int32_t* tile_frames, const float* tile_w, const float* inv_wsum, int64_t n_tiles, int64_t T, int64_t Tt,
                                  const float* rope_cos, const float* rope_sin, int64_t H, int64_t W, void* workspace, int64_t workspace_bytes,
                                  const float* sigma, const float* coef, void* hist, int64_t hist_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCAIL_DIT_H */
