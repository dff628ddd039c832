// Network-level entry points (include/scail_dit.h): one DiT evaluation of the sampler step composed from the
// operator entry points of this library -- the C++ statement of DiffusionTransformer.forward ->
// BaseTransformer.forward -> AdaLNMixin.layer_forward (dit_video_crossattn_sc_xc.py:1452-1587, :1009-1051;
// sat/model/transformer.py:572-746), for one rank or for a sequence-parallel rank (the collectives of the per-layer exchange go to
// the host through a callback).  Host code only: every line below enqueues kernels on the caller's stream; nothing synchronises, so
// a single-rank step is hipGraph-capturable.
#include <algorithm>
#include <array>
#include <cmath>
#include <vector>

#include "common.h"
int scail_attn4_preload();   // attn.hip
void scail_attn4_rows_hint(int rows);   // attn.hip: pins the query-tile height of this thread's attention launches (0 = planned per launch)
int scail_gemm4_preload();   // gemm.hip
#include "../../include/scail_dit.h"

// Optional HIP-event timing of the executor's own launches (scail_dit_profile, include/scail_dit.h): event pairs recorded on the
// launch stream around every launch of a category; the events are pooled in the handle and reused by the next enable.
constexpr int PROF_CATS = 5;     // SCAIL_DIT_PROF_SELF_ATTN / _GEMM / _CROSS_ATTN / _XCH_FWD_WAIT / _XCH_BACK_WAIT
struct ProfPool {
    std::vector<hipEvent_t> ev;  // start / stop alternating
    size_t used = 0;
};

// the third quantised form of a handle beside SCAIL_DIT_FP8_SCALE_ROW / _MX: packed e2m3 codes + E8M0 block scales (scail_dit_enable_fp6).
// Internal: scail_dit_enable_fp8_scaled does not accept it.
enum { QFORM_FP6 = 2 };
struct scail_dit {
    scail_dit_config cfg;
    scail_dit_weights w;
    std::vector<scail_dit_layer> layers;
    bool prof = false;
    ProfPool pool[PROF_CATS];
    hipEvent_t sp_ev[3] = {nullptr, nullptr, nullptr};   // fork / join events of the sequence-parallel block's side streams (created on first use)
    uint32_t* restart_ctr = nullptr;                     // device counter of restarted self-attention workgroups (allocated by the first scail_dit_profile(h, 1))
    // fp8 GEMMs (scail_dit_enable_fp8): the SCAIL_DIT_FP8_* mask in force and, per layer and GEMM (bit index), the e4m3 weight codes and
    // per-channel scales in the caller's buffer
    uint32_t fp8 = 0;
    int fp8_scaling = SCAIL_DIT_FP8_SCALE_ROW;     // one quantised form per handle, chosen at enable time: a SCAIL_DIT_FP8_SCALE_* or QFORM_FP6
    struct Fp8W { const uint8_t* q; const float* s; const uint8_t* e; };   // s: fp32 row scales (ROW); e: E8M0 block scales [N, K / 32] (MX)
    std::vector<std::array<Fp8W, 6>> fp8w;
    // scail_dit_fp8_select_layers: per layer, the subset of `fp8` in force (empty: `fp8` in every layer)
    std::vector<uint32_t> fp8_sel;
    // scail_dit_fp8_probe: the caller's fp64 table [layers][6][4] (null: off) and the two bf16 result buffers of probe_rows x fp8_n() each
    double* probe_table = nullptr;
    scail_bf16 *probe_y16 = nullptr, *probe_y8 = nullptr;
    int64_t probe_rows = 0;
};

namespace {

constexpr int64_t KPAD = 128;   // patch-embedding im2col width (80 real columns, zero padded to the GEMM k-tile)

inline int64_t align256(int64_t n) { return (n + 255) / 256 * 256; }

// hands out the consecutive 256-byte aligned blocks of a workspace (so a total does not depend on the order of its blocks)
struct Carve {
    int64_t off = 0;
    int64_t take(int64_t bytes) { const int64_t o = off; off += align256(bytes); return o; }
};

// elements of the V^T staging buffer of a (B, Ltok) block: one rank (sp_mode < 0): all heads x the local keys; ulysses: heads / ranks
// heads x ALL ranks' keys; all-gather: all heads x all ranks' keys
int64_t vt_elems(const scail_dit_config& c, int64_t B, int64_t Ltok, int sp_mode, int64_t ranks) {
    const int64_t nh = c.num_heads;
    if (sp_mode < 0) return B * nh * 128 * ((Ltok + 63) / 64 * 64);
    const int64_t Lfp = (ranks * Ltok + 63) / 64 * 64;
    return B * (sp_mode == SCAIL_SP_ULYSSES ? nh / ranks : nh) * 128 * Lfp;
}

// Token counts of a (T, H, W) latent (or latent slab) with C characters: [ref_0..ref_{C-1} | noise | pose_0..pose_{C-1}]
struct TokLens {
    int64_t Lref, Lnoise, Lpose, Ltok;
};
TokLens tok_lens(int64_t C, int64_t T, int64_t H, int64_t W) {
    const int64_t hp = H / 2, wp = W / 2;
    TokLens l;
    l.Lref = C * hp * wp;
    l.Lnoise = T * hp * wp;
    l.Lpose = C * T * (H / 4) * (W / 4);
    l.Ltok = l.Lref + l.Lnoise + l.Lpose;
    return l;
}
// the self-attention launch takes ceil64(keys) < 2^31 (scail_flash_attn_bf16); a sequence-parallel rank attends to all ranks' keys
constexpr int64_t MAX_KEYS = (1ll << 31) - 64;
// what keeps a latent (or latent slab) of C characters on `ranks` ranks from the executor: 0 nothing, 1 its sizes (or C / ranks) as
// such, 2 the key count.  The queries answer -1 for either; dit_step_impl names which
int shape_fault(int64_t B, int64_t T, int64_t H, int64_t W, int64_t C, int64_t ranks) {
    if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || H % 4 != 0 || W % 4 != 0 || C < 1 || C > 64 || ranks < 1) return 1;
    if (T >= (1 << 15) || H >= (1 << 15) || W >= (1 << 15)) return 2;      // (keeps the products below in 64 bits)
    return ranks * tok_lens(C, T, H, W).Ltok < MAX_KEYS ? 0 : 2;
}
// a sequence-parallel group the executor has a workspace for (sp_check refuses the rest of a bad descriptor, each part by name)
bool sp_group_ok(const scail_dit_config& c, int32_t mode, int64_t ranks) {
    if (ranks < 2 || (mode != SCAIL_SP_ALLGATHER && mode != SCAIL_SP_ULYSSES)) return false;
    return mode != SCAIL_SP_ULYSSES || c.num_heads % ranks == 0;
}

// the character arguments of the *_chars entry points, checked first (host only; the message names the value)
int chars_check(const char* who, int64_t n_char, int64_t pose_frames, int64_t T) {
    if (n_char < 1 || n_char > 64) {
        scail_set_error(std::string(who) + ": n_char must be 1..64, got " + std::to_string(n_char));
        return 1;
    }
    if (pose_frames != n_char * T) {
        scail_set_error(std::string(who) + ": pose must hold n_char * T = " + std::to_string(n_char) + " * " + std::to_string(T) + " frames, got " +
                        std::to_string(pose_frames));
        return 1;
    }
    return 0;
}

__global__ void dup_rows_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t rows, int64_t w) {
    // out[b, 0:w] = out[b, w:2w] = in[b, :]   (emb.repeat(1, 2) of the final-layer table add, dit...:823)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * w) return;
    const int64_t b = i / w, j = i - b * w;
    const float v = in[i];
    out[b * 2 * w + j] = v;
    out[b * 2 * w + w + j] = v;
}

}  // namespace

#define DIT_TRY(call_)                  \
    {                                   \
        const int rc_ = (call_);        \
        if (rc_ != 0) return rc_;       \
    }

static int prof_mark(scail_dit* h, int cat, void* stream) {
    ProfPool& p = h->pool[cat];
    if (p.used == p.ev.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) {
            scail_set_error("scail_dit_profile: hipEventCreate failed");
            return 2;
        }
        p.ev.push_back(e);
    }
    if (hipEventRecord(p.ev[p.used++], (hipStream_t)stream) != hipSuccess) {
        scail_set_error("scail_dit_profile: hipEventRecord failed (profiling cannot run inside a stream capture)");
        return 2;
    }
    return 0;
}
// while profiling, the self-attention launches of this thread count their restarted workgroups into the handle's device counter
struct RestartCount {
    bool on;
    explicit RestartCount(scail_dit* h, int cat) : on(h->prof && cat == SCAIL_DIT_PROF_SELF_ATTN && h->restart_ctr != nullptr) {
        if (on) (void)scail_flash_attn_count_restarts(h->restart_ctr);
    }
    ~RestartCount() { if (on) (void)scail_flash_attn_count_restarts(nullptr); }
};
// one launch of category cat_ on stream st_, bracketed by an event pair when profiling is on
#define DIT_PROF_S(cat_, st_, call_)                            \
    {                                                           \
        if (h->prof) DIT_TRY(prof_mark(h, cat_, st_));          \
        RestartCount rc_guard_(h, cat_);                        \
        DIT_TRY(call_);                                         \
        if (h->prof) DIT_TRY(prof_mark(h, cat_, st_));          \
    }
#define DIT_PROF(cat_, call_) DIT_PROF_S(cat_, stream, call_)

// The per-token GEMMs of a block, by SCAIL_DIT_FP8_* bit index: (N, K) and the bf16 weight
enum { G_QKV = 0, G_O, G_CQ, G_CO, G_W1, G_W2, G_COUNT };
static const char* const k_gemm_names[G_COUNT] = {"qkv", "o", "cq", "co", "w1", "w2"};
static void gemm_shape(const scail_dit_config& c, int g, int64_t* N, int64_t* K) {
    const int64_t D = c.hidden_size, FF = c.inner_hidden_size;
    *N = g == G_QKV ? 3 * D : g == G_W1 ? FF : D;
    *K = g == G_W2 ? FF : D;
}
static const scail_bf16* gemm_weight(const scail_dit_layer& lw, int g) {
    const scail_bf16* const w[G_COUNT] = {lw.qkv_w, lw.o_w, lw.cq_w, lw.co_w, lw.w1, lw.w2};
    return w[g];
}
static int64_t fp8_k(const scail_dit* h) {
    int64_t kmax = 0;
    for (int g = 0; g < G_COUNT; ++g)
        if (h->fp8 & (1u << g)) {
            int64_t N, K;
            gemm_shape(h->cfg, g, &N, &K);
            kmax = std::max(kmax, K);
        }
    return kmax;
}
// the widest output of a quantised GEMM (the probe's result buffers)
static int64_t fp8_n(const scail_dit* h) {
    int64_t nmax = 0;
    for (int g = 0; g < G_COUNT; ++g)
        if (h->fp8 & (1u << g)) {
            int64_t N, K;
            gemm_shape(h->cfg, g, &N, &K);
            nmax = std::max(nmax, N);
        }
    return nmax;
}
// whether GEMM g of layer i runs in fp8: quantised by scail_dit_enable_fp8 and not deselected by scail_dit_fp8_select_layers
static bool fp8_in_force(const scail_dit* h, int64_t i, int g) {
    return ((h->fp8_sel.empty() ? h->fp8 : h->fp8_sel[i]) & (1u << g)) != 0;
}
static void probe_off(scail_dit* h) {
    h->probe_table = nullptr;
    h->probe_y16 = h->probe_y8 = nullptr;
    h->probe_rows = 0;
}
// a call that runs GEMMs on `rows` rows while the probe is on: refused, before anything is enqueued, when the probe's buffers are smaller
static int probe_check(const scail_dit* h, int64_t rows) {
    if (h->probe_table != nullptr && rows > h->probe_rows) {
        scail_set_error("scail_dit_fp8_probe: this call runs GEMMs on " + std::to_string(rows) + " rows, the probe's scratch covers " +
                        std::to_string(h->probe_rows) + " (scail_dit_fp8_probe_bytes)");
        return 1;
    }
    return 0;
}

// ---- workspaces: every layout is stated once; the *_workspace_bytes query and the call that checks it read the same struct ----
struct BlockBufs {
    scail_bf16 *xn, *qkv, *att, *ff, *vt;
    uint8_t* xq;   // fp8 GEMMs only (else null): e4m3 rows of the GEMM input (rows x the widest fp8 K; fp6: rows x 3/4 of it, packed) and their scales:
    float* sx;     // rows fp32 (per-row scaling) or, through ex(), rows x (the widest fp8 K) / 32 E8M0 bytes (MX and fp6)
    uint8_t* ex() const { return reinterpret_cast<uint8_t*>(sx); }
};
// The scratch of a (B, Ltok) block, xn | qkv | att | ff | vt | xq | sx, as byte offsets into a workspace from `at` on; end: the first
// byte after it.  One rank (sp_mode < 0) or a sequence-parallel rank (bf16 only: xq / sx are empty there and without fp8 GEMMs)
struct BlockWs {
    int64_t xn, qkv, att, ff, vt, xq, sx, end;
    BlockBufs bufs(void* workspace) const {
        char* base = static_cast<char*>(workspace);
        auto P = [&](int64_t o) { return reinterpret_cast<scail_bf16*>(base + o); };
        const bool f8 = sx > xq;
        return {P(xn), P(qkv), P(att), P(ff), P(vt), f8 ? reinterpret_cast<uint8_t*>(base + xq) : nullptr, f8 ? reinterpret_cast<float*>(base + sx) : nullptr};
    }
};
static BlockWs block_ws(const scail_dit* h, int64_t B, int64_t Ltok, int sp_mode = -1, int64_t ranks = 1, int64_t at = 0) {
    const int64_t D = h->cfg.hidden_size, FF = h->cfg.inner_hidden_size, rows = B * Ltok;
    const int64_t f8_k = sp_mode < 0 ? fp8_k(h) : 0;
    Carve c{at};
    BlockWs s;
    s.xn = c.take(rows * D * 2);
    s.qkv = c.take(rows * 3 * D * 2);
    s.att = c.take(rows * D * 2);
    s.ff = c.take(rows * FF * 2);
    s.vt = c.take(vt_elems(h->cfg, B, Ltok, sp_mode, ranks) * 2);
    s.xq = c.take(h->fp8_scaling == QFORM_FP6 ? rows * (f8_k / 4 * 3) : rows * f8_k);
    s.sx = c.take(h->fp8_scaling != SCAIL_DIT_FP8_SCALE_ROW ? rows * (f8_k / 32) : f8_k ? rows * 4 : 0);
    s.end = c.off;
    return s;
}
// the step workspace: token assembly and hidden states, the block scratch, the final layer's rows, the time / AdaLN tables
struct Ws {
    int64_t tok, h, xf, tokout, temb, e1, emb, adaln, mod, emb2, fin, total;
    BlockWs blk;
};
static Ws layout(const scail_dit* h, int64_t B, int64_t T, int64_t H, int64_t W, int64_t C, int sp_mode = -1, int64_t ranks = 1) {
    const scail_dit_config& c = h->cfg;
    const int64_t D = c.hidden_size;
    const TokLens tl = tok_lens(C, T, H, W);
    Ws s;
    Carve cv;
    s.tok = cv.take(B * tl.Ltok * KPAD * 2);
    s.h = cv.take(B * tl.Ltok * D * 2);
    s.blk = block_ws(h, B, tl.Ltok, sp_mode, ranks, cv.off);
    cv.off = s.blk.end;
    s.xf = cv.take(B * tl.Lnoise * D * 2);
    s.tokout = cv.take(B * tl.Lnoise * 64 * 2);
    s.temb = cv.take(B * c.time_freq_dim * 4);
    s.e1 = cv.take(B * c.time_embed_dim * 4);
    s.emb = cv.take(B * c.time_embed_dim * 4);
    s.adaln = cv.take(B * 6 * D * 4);
    s.mod = cv.take((int64_t)c.num_layers * B * 6 * D * 4);
    s.emb2 = cv.take(B * 2 * D * 4);
    s.fin = cv.take(B * 2 * D * 4);
    s.total = cv.off;
    return s;
}
// the sampler loops' workspace: the step workspace of the batch-2 evaluation (`step` bytes), then [x; x] and [v_u; v_c] of Tv frames and
// (tiled) den of Tden frames, fp32.  step = 0: the part that needs no handle
struct SampleWs {
    int64_t xin, v, den, total;
};
static SampleWs sample_ws(int64_t step, int64_t Tv, int64_t H, int64_t W, int64_t Tden = 0) {
    const int64_t F = 16 * H * W, pair = align256(2 * Tv * F * 4);
    return {step, step + pair, step + 2 * pair, step + 2 * pair + align256(Tden * F * 4)};
}

// the step cache of a (B, T, H, W) evaluation: r bf16 [B][Lnoise][D] at offset 0 (documented: callers read it), then FILL's copy of the
// embedded noise rows, [B][Lnoise][D] too (one element of it is used under SCAIL_DIT_CFG_PAIR)
enum { CACHE_NONE = 0 };
struct CacheWs {
    int64_t r, emb, total;
};
static CacheWs cache_ws(const scail_dit_config& c, int64_t B, int64_t Lnoise) {
    Carve cv;
    CacheWs s;
    s.r = cv.take(B * Lnoise * c.hidden_size * 2);
    s.emb = cv.take(B * Lnoise * c.hidden_size * 2);
    s.total = cv.off;
    return s;
}
// the two regions of one step cache, as dit_step_impl takes them
struct CachePtrs {
    scail_bf16 *r, *emb;
};
static CachePtrs cache_ptrs(const scail_dit_config& c, int64_t B, int64_t Lnoise, void* cache) {
    const CacheWs cw = cache_ws(c, B, Lnoise);
    return {reinterpret_cast<scail_bf16*>(static_cast<char*>(cache) + cw.r), reinterpret_cast<scail_bf16*>(static_cast<char*>(cache) + cw.emb)};
}

// x quantised into the block's scratch and multiplied with the quantised weight f, under the handle's scaling
static int fp8_quant_gemm(const scail_dit* h, const scail_dit::Fp8W& f, const BlockBufs& bf, const scail_bf16* x, int64_t lda, const float* bias,
                          scail_bf16* y, int64_t ldc, int64_t M, int64_t N, int64_t K, int epi, const scail_bf16* resid, int64_t ldr,
                          const float* gate, int64_t gs, int64_t rpb, void* stream) {
    if (h->fp8_scaling == QFORM_FP6) {
        DIT_TRY(scail_quant_mxfp6_rows(x, lda, bf.xq, K / 4 * 3, bf.ex(), K / 32, M, K, stream));
        return scail_gemm_mxfp6(bf.xq, K / 4 * 3, bf.ex(), K / 32, f.q, f.e, bias, y, ldc, M, N, K, epi, resid, ldr, gate, gs, rpb, stream);
    }
    if (h->fp8_scaling == SCAIL_DIT_FP8_SCALE_MX) {
        DIT_TRY(scail_quant_mxfp8_rows(x, lda, bf.xq, K, bf.ex(), K / 32, M, K, stream));
        return scail_gemm_mxfp8(bf.xq, K, bf.ex(), K / 32, f.q, f.e, bias, y, ldc, M, N, K, epi, resid, ldr, gate, gs, rpb, stream);
    }
    DIT_TRY(scail_quant_fp8_rows(x, lda, bf.xq, K, bf.sx, M, K, stream));
    return scail_gemm_fp8(bf.xq, K, bf.sx, f.q, f.s, bias, y, ldc, M, N, K, epi, resid, ldr, gate, gs, rpb, stream);
}

// GEMM g of layer i: scail_gemm_bf16, or (SCAIL_DIT_FP8_* bit g in force in layer i) the rows of x quantized to e4m3 into the block's
// scratch and scail_gemm_fp8 on the layer's e4m3 weight (scail_quant_mxfp8_rows + scail_gemm_mxfp8 under MX scaling, scail_quant_mxfp6_rows
// + scail_gemm_mxfp6 under fp6: fp8_quant_gemm above); the same epilogue either way.  While the probe is on, a GEMM whose weight is
// quantised (in force or not) first runs twice on these very rows with the plain bias epilogue -- bf16 and fp8, into the probe's two
// buffers --, their distance goes to table[i][g], and the real GEMM then runs in bf16.
static int dit_gemm(scail_dit* h, int64_t i, int g, const BlockBufs& bf, const scail_bf16* x, int64_t lda, const float* bias, scail_bf16* y,
                    int64_t ldc, int64_t M, int64_t N, int64_t K, int epi, const scail_bf16* resid, int64_t ldr, const float* gate, int64_t gs,
                    int64_t rpb, void* stream) {
    const bool quantised = (h->fp8 & (1u << g)) != 0;
    if (quantised && h->probe_table != nullptr) {
        const scail_dit::Fp8W& f = h->fp8w[i][g];
        DIT_TRY(scail_gemm_bf16(x, lda, gemm_weight(h->layers[i], g), bias, h->probe_y16, N, M, N, K, SCAIL_EPI_BIAS, nullptr, 0, nullptr, 0, 0, stream));
        DIT_TRY(fp8_quant_gemm(h, f, bf, x, lda, bias, h->probe_y8, N, M, N, K, SCAIL_EPI_BIAS, nullptr, 0, nullptr, 0, 0, stream));
        DIT_TRY(scail_rel_err_rows(h->probe_y16, N, h->probe_y8, N, h->probe_table + (i * G_COUNT + g) * 4, M, N, stream));
    } else if (quantised && fp8_in_force(h, i, g)) {
        return fp8_quant_gemm(h, h->fp8w[i][g], bf, x, lda, bias, y, ldc, M, N, K, epi, resid, ldr, gate, gs, rpb, stream);
    }
    return scail_gemm_bf16(x, lda, gemm_weight(h->layers[i], g), bias, y, ldc, M, N, K, epi, resid, ldr, gate, gs, rpb, stream);
}

constexpr float ATTN_SCALE = 0.08838834764831845f;              // 1 / sqrt(128)
constexpr float ATTN_LOG2_SCALE = ATTN_SCALE * 1.4426950408889634f;   // queries in log2 units (scail_flash_attn_bf16 SCAIL_ATTN_Q_PRESCALED)

// Everything of a block AFTER its self-attention, for `nb` batch elements starting at element b0 whose rows lie `rpb` apart in every
// buffer (hid / att: row stride D; q3: the first column third of a row-stride-3D buffer; xn / ff: scratch of nb * rpb rows):
// out-projection + gated residual, cross attention (text + CLIP, ungated residual), MLP (dit...:1036-1050, :1107-1203;
// sat/transformer_defaults.py:163-176).  m = the (6D) modulation row of element b0 (rows of later elements 6D apart).
// block_attn_out: the out-projection + gated residual alone; block_cross_mlp: the rest (the first point of a block at which the two CFG
// elements of a step differ: scail_dit_step's SCAIL_DIT_CFG_PAIR).
static int block_attn_out(scail_dit* h, int64_t i, scail_bf16* hid, scail_bf16* att, const float* m, int64_t nb, int64_t rpb, const BlockBufs& bf,
                          void* stream) {
    const int64_t D = h->cfg.hidden_size;
    const scail_dit_layer& lw = h->layers[i];
    DIT_PROF(SCAIL_DIT_PROF_GEMM, dit_gemm(h, i, G_O, bf, att, D, lw.o_b, hid, D, nb * rpb, D, D, SCAIL_EPI_RESID, hid, D, m + 2 * D, 6 * D, rpb, stream));
    return 0;
}
static int block_cross_mlp(scail_dit* h, int64_t i, scail_bf16* hid, scail_bf16* att, scail_bf16* q3, scail_bf16* xn, scail_bf16* ff,
                           const float* m, const scail_dit_cond* cond, int64_t Btot, int64_t b0, int64_t nb, int64_t rpb, const BlockBufs& bf,
                           void* stream) {
    const scail_dit_config& c = h->cfg;
    const int64_t D = c.hidden_size, FF = c.inner_hidden_size, nh = c.num_heads;
    const float eps = c.layernorm_epsilon;
    const int64_t Ltp = (cond->Lt + 63) / 64 * 64, Lcp = (cond->Lc + 63) / 64 * 64;
    const int64_t M = nb * rpb;
    const scail_dit_layer& lw = h->layers[i];
    // -- cross attention: text + CLIP, ungated residual (dit...:1039-1042, :1107-1203) --
    DIT_TRY(scail_layernorm_affine(hid, D, xn, D, lw.ln_w, lw.ln_b, M, D, eps, stream));
    DIT_PROF(SCAIL_DIT_PROF_GEMM, dit_gemm(h, i, G_CQ, bf, xn, D, lw.cq_b, q3, 3 * D, M, D, D, SCAIL_EPI_BIAS, nullptr, 0, nullptr, 0, 0, stream));
    // (the queries go to the attention in log2 units, like the self-attention's: no scale / shift per score in the kernel)
    DIT_TRY(scail_rmsnorm_rope_scaled(q3, 3 * D, q3, 3 * D, lw.cqn, nullptr, nullptr, M, M, D, 128, eps, ATTN_LOG2_SCALE, stream));
    const bool shared_clip = cond->Bc == 1;
    const scail_bf16* kt = cond->k_text + (i * Btot + b0) * cond->Lt * D;
    const scail_bf16* vtt = cond->vt_text + (i * Btot + b0) * nh * 128 * Ltp;
    const scail_bf16* kc = cond->k_clip + (i * cond->Bc + (shared_clip ? 0 : b0)) * cond->Lc * D;
    const scail_bf16* vtc = cond->vt_clip + (i * cond->Bc + (shared_clip ? 0 : b0)) * nh * 128 * Lcp;
    DIT_PROF(SCAIL_DIT_PROF_CROSS_ATTN, scail_cross_attn2_bf16(q3, rpb * 3 * D, 3 * D, kt, cond->Lt * D, D, vtt, nh * 128 * Ltp, cond->Lt,
                                                               kc, shared_clip ? 0 : cond->Lc * D, D, vtc, shared_clip ? 0 : nh * 128 * Lcp, cond->Lc,
                                                               att, rpb * D, D, nb, nh, rpb, SCAIL_ATTN_Q_PRESCALED, stream));
    DIT_PROF(SCAIL_DIT_PROF_GEMM, dit_gemm(h, i, G_CO, bf, att, D, lw.co_b, hid, D, M, D, D, SCAIL_EPI_RESID, hid, D, nullptr, 0, 0, stream));
    // -- MLP (dit...:1045-1050; sat/transformer_defaults.py:163-176) --
    DIT_TRY(scail_ln_modulate(hid, D, xn, D, m + 3 * D, m + 4 * D, 6 * D, nb, rpb, rpb, 0, D, eps, stream));
    DIT_PROF(SCAIL_DIT_PROF_GEMM, dit_gemm(h, i, G_W1, bf, xn, D, lw.b1, ff, FF, M, FF, D, SCAIL_EPI_GELU_TANH, nullptr, 0, nullptr, 0, 0, stream));
    DIT_PROF(SCAIL_DIT_PROF_GEMM, dit_gemm(h, i, G_W2, bf, ff, FF, lw.b2, hid, D, M, D, FF, SCAIL_EPI_RESID, hid, D, m + 5 * D, 6 * D, rpb, stream));
    return 0;
}
// Where the conditioning of a call's elements lies in `cond`: cond holds Btot elements and element b of the call reads element b0 + b.
// Every call but scail_dit_step_branch reads its own batch from element 0 on: {B, 0}.
struct CondAt {
    int64_t Btot, b0;
};
// Everything after the self-attention of the rows [row0, row0 + rows) of every element (rows == Ltok: the whole block in one set of
// launches; fewer: per element, the wanted rows only).  pair: hid / att / m of element 1 do not exist yet -- the out-projection runs
// for element 0 and its result (the hidden states after the self-attention residual) is copied to element 1 before the elements part.
static int block_tail(scail_dit* h, int64_t i, scail_bf16* hid, const float* m, const scail_dit_cond* cond, int64_t B, int64_t Ltok,
                      const BlockBufs& bf, int64_t row0, int64_t rows, bool pair, void* stream, CondAt ca) {
    const int64_t D = h->cfg.hidden_size;
    scail_bf16 *att = bf.att, *q = bf.qkv, *xn = bf.xn, *ff = bf.ff;
    if (pair) {
        DIT_TRY(block_attn_out(h, i, hid + row0 * D, att + row0 * D, m, 1, rows, bf, stream));
        if (hipMemcpyAsync(hid + Ltok * D, hid, (size_t)Ltok * D * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) {
            scail_set_error("scail_dit (cfg pair): hipMemcpyAsync failed");
            return 2;
        }
    }
    if (rows == Ltok) {
        if (!pair) DIT_TRY(block_attn_out(h, i, hid, att, m, B, Ltok, bf, stream));
        return block_cross_mlp(h, i, hid, att, q, xn, ff, m, cond, ca.Btot, ca.b0, B, Ltok, bf, stream);
    }
    for (int64_t b = 0; b < B; ++b) {
        const int64_t r = b * Ltok + row0;
        if (!pair) DIT_TRY(block_attn_out(h, i, hid + r * D, att + r * D, m + b * 6 * D, 1, rows, bf, stream));
        DIT_TRY(block_cross_mlp(h, i, hid + r * D, att + r * D, q + r * 3 * D, xn, ff, m + b * 6 * D, cond, ca.Btot, ca.b0 + b, 1, rows, bf, stream));
    }
    return 0;
}

// One transformer block in place on hid (B, Ltok, D): AdaLNMixin.layer_forward, dit...:1009-1051.
//   m (B, 6D) fp32 = shift_a | scale_a | gate_a | shift_m | scale_m | gate_m of THIS layer (adaLN emb + table)
//   [row0, row0 + rows): the token rows of every batch element whose OUTPUT is wanted.  rows == Ltok: the whole block.  rows < Ltok
//   (the LAST layer of a step: only the noise tokens reach the final layer, dit...:771, :825-826): every token still contributes its
//   key and value, but the queries, the out-projection, the cross attention and the MLP run on the wanted rows only -- the other
//   rows of hid are left as they were.  Result-preserving: every kernel computes a row of its output from that row alone.
//   pair (B == 2): element 1 of hid is not filled in yet and equals element 0 up to this block's first cross attention (the CFG pair
//   of a sampler step): the self-attention part runs for element 0 only.
static int dit_block(scail_dit* h, int64_t i, scail_bf16* hid, const float* m, const scail_dit_cond* cond,
                     const float* rope_cos, const float* rope_sin, int64_t B, int64_t Ltok, const BlockBufs& bf,
                     int64_t row0, int64_t rows, bool pair, void* stream, CondAt ca) {
    const scail_dit_config& c = h->cfg;
    const int64_t D = c.hidden_size, nh = c.num_heads;
    const float eps = c.layernorm_epsilon;
    const int64_t Lp = (Ltok + 63) / 64 * 64;
    const int64_t Bs = pair ? 1 : B;          // elements of the self-attention part
    const int64_t M = Bs * Ltok;
    scail_bf16 *qkv = bf.qkv, *q = qkv, *k = qkv + D, *v = qkv + 2 * D;   // column thirds of the fused projection, row stride 3D
    const scail_dit_layer& lw = h->layers[i];
    // -- self attention (dit...:1031-1036, :1058-1105) --
    DIT_TRY(scail_ln_modulate(hid, D, bf.xn, D, m, m + D, 6 * D, Bs, Ltok, Ltok, 0, D, eps, stream));
    DIT_PROF(SCAIL_DIT_PROF_GEMM, dit_gemm(h, i, G_QKV, bf, bf.xn, D, lw.qkv_b, qkv, 3 * D, M, 3 * D, D, SCAIL_EPI_BIAS, nullptr, 0, nullptr, 0, 0, stream));
    DIT_TRY(scail_rmsnorm_rope(k, 3 * D, k, 3 * D, lw.kn, rope_cos, rope_sin, M, Ltok, D, 128, eps, stream));
    // V as projected where the V-rows kernels take the call (include/scail_hip.h scail_flash_attn_vrows_bf16: bit-identical, no V^T pass);
    // the V^T image of the workspace serves every other call
    const bool vrows = scail_flash_attn_vrows_for(3 * D, 3 * D, 3 * D, D, Bs, nh, rows, Ltok) != 0;
    if (!vrows) DIT_TRY(scail_transpose_v(v, 3 * D, Ltok * 3 * D, bf.vt, Bs, nh, 128, Ltok, stream));
    // the queries go to the attention in log2 units (q * scale * log2 e, one rounding): its exp2 then needs no scale / shift per score
    DIT_TRY(scail_rmsnorm_rope_scaled(q, 3 * D, q, 3 * D, lw.qn, rope_cos, rope_sin, M, Ltok, D, 128, eps, ATTN_LOG2_SCALE, stream));
    if (vrows) {
        DIT_PROF(SCAIL_DIT_PROF_SELF_ATTN, scail_flash_attn_vrows_bf16(q + row0 * 3 * D, Ltok * 3 * D, 3 * D, k, Ltok * 3 * D, 3 * D, v, Ltok * 3 * D, 3 * D,
                                                                       bf.att + row0 * D, Ltok * D, D, Bs, nh, rows, Ltok, SCAIL_ATTN_Q_PRESCALED, stream));
        return block_tail(h, i, hid, m, cond, B, Ltok, bf, row0, rows, pair, stream, ca);
    }
    DIT_PROF(SCAIL_DIT_PROF_SELF_ATTN, scail_flash_attn_bf16(q + row0 * 3 * D, Ltok * 3 * D, 3 * D, k, 0, Ltok * 3 * D, 3 * D, bf.vt, 0, nh * 128 * Lp,
                                                             bf.att + row0 * D, Ltok * D, D, Bs, nh, rows, Ltok, 1, SCAIL_ATTN_Q_PRESCALED, 0, stream));
    return block_tail(h, i, hid, m, cond, B, Ltok, bf, row0, rows, pair, stream, ca);
}

// ---- the sequence-parallel block (include/scail_dit.h "sequence-parallel execution") ----
static int sp_exchange(const scail_dit_sp* sp, int op, int64_t layer, int64_t b, void* stream) {
    const int rc = sp->exchange(sp->user, (int32_t)op, (int32_t)layer, (int32_t)b, stream);
    if (rc != 0) {
        scail_set_error("scail_dit (sequence parallel): the host's exchange callback failed (op " + std::to_string(op) + ", layer " +
                        std::to_string(layer) + ", element " + std::to_string(b) + ", status " + std::to_string(rc) + ")");
        return 3;
    }
    return 0;
}

static int sp_check(const scail_dit* h, const scail_dit_sp* sp) {
    SCAIL_REQUIRE(h->fp8 == 0, "fp8 GEMMs are enabled on this handle; sequence-parallel ranks run bf16 only (scail_dit_enable_fp8(h, 0, ...) first)");
    SCAIL_REQUIRE(sp != nullptr && sp->exchange != nullptr, "null sequence-parallel descriptor / exchange callback");
    SCAIL_REQUIRE(sp->ranks >= 2 && sp->ranks <= 64, "ranks must be 2..64");
    SCAIL_REQUIRE(sp->mode == SCAIL_SP_ALLGATHER || sp->mode == SCAIL_SP_ULYSSES, "unknown exchange mode");
    SCAIL_REQUIRE(sp->send != nullptr && sp->recv != nullptr, "null send / recv buffer");
    if (sp->mode == SCAIL_SP_ULYSSES) {
        SCAIL_REQUIRE(h->cfg.num_heads % sp->ranks == 0, "ulysses needs heads divisible by the group size");
        SCAIL_REQUIRE(sp->ofull != nullptr && sp->back != nullptr, "ulysses needs the ofull / back buffers");
    }
    SCAIL_REQUIRE((sp->side_stream[0] == nullptr) == (sp->side_stream[1] == nullptr), "give both side streams or none");
    return 0;
}

// hid (B, Ltok, D) = this rank's token slab.  Kernel sequence and results are those of scail_amd.parallel's per-op path (kept as the
// cross-check: tests/test_dit_gpu.py); only the host side differs: one call per layer instead of ~30 launches through the binding.
//   [row0, row0 + rows), pair: as for dit_block.  Every token's key and value is exchanged whatever the wanted rows; with fewer rows the
//   out-projection / cross attention / MLP run on them only, and so do the queries of the all-gather mode (the ulysses attention
//   keeps all queries: its sequence is rank-major, the wanted rows would be `ranks` separate ranges).
namespace {
// Joins the side streams of the ulysses section back into `stream` -- also when the section is left early on an error: kernels and
// collectives already enqueued on the side streams stay ordered before whatever the caller enqueues on `stream` next (freeing or reusing
// the workspace and the exchange buffers included).  A status-3 abort (the host's exchange callback failed) leaves collectives unmatched
// on the peers: the caller must tear down the communicator (include/scail_dit.h).
struct SideJoin {
    scail_dit* h;
    const scail_dit_sp* sp;
    void* stream;
    int n = 0;           // side streams forked
    int join() {
        int rc = 0;
        for (int j = 0; j < n; ++j)
            if (hipEventRecord(h->sp_ev[1 + j], (hipStream_t)sp->side_stream[j]) != hipSuccess ||
                hipStreamWaitEvent((hipStream_t)stream, h->sp_ev[1 + j], 0) != hipSuccess)
                rc = 2;
        n = 0;
        return rc;
    }
    ~SideJoin() { (void)join(); }
};
}  // namespace
static int dit_block_sp(scail_dit* h, int64_t i, scail_bf16* hid, const float* m, const scail_dit_cond* cond,
                        const float* rope_cos, const float* rope_sin, int64_t Btot, int64_t Ltok, const BlockBufs& bf,
                        const scail_dit_sp* sp, int64_t row0, int64_t rows, bool pair, void* stream) {
    const scail_dit_config& c = h->cfg;
    const int64_t D = c.hidden_size, nh = c.num_heads, N = sp->ranks;
    const float eps = c.layernorm_epsilon;
    const int64_t Lf = N * Ltok, Lfp = (Lf + 63) / 64 * 64;
    const int64_t B = pair ? 1 : Btot;        // elements of the self-attention part
    scail_bf16 *qkv = bf.qkv, *q = qkv;
    const scail_dit_layer& lw = h->layers[i];
    DIT_TRY(scail_ln_modulate(hid, D, bf.xn, D, m, m + D, 6 * D, B, Ltok, Ltok, 0, D, eps, stream));
    if (sp->mode == SCAIL_SP_ULYSSES) {
        // head <-> sequence all-to-all of q, k, v after norm + RoPE (sat/mpu/ulysses_attn_layer.py:65-107), full-length attention on
        // heads / N heads, all-to-all back.  The CFG elements are independent sequences: element b + 1's projection runs under
        // element b's exchange, element b's attention under element b + 1's exchange, the ways back under the other's attention.
        const int64_t Hn = nh / N, Dn = Hn * 128, slab = Ltok * Dn;
        const bool side = sp->side_stream[0] != nullptr;
        auto st = [&](int64_t b) { return side ? sp->side_stream[b & 1] : stream; };
        SideJoin sj{h, sp, stream};
        if (side) {
            // one side stream per element (up to 4 ranks: an element's launches leave a partial last round of the chip which the other
            // element's kernels fill).  The collectives are still enqueued in the order fwd(0), fwd(1), back(0), back(1).
            for (hipEvent_t& e : h->sp_ev)
                if (e == nullptr && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
                    scail_set_error("scail_dit (sequence parallel): hipEventCreate failed");
                    return 2;
                }
            if (hipEventRecord(h->sp_ev[0], (hipStream_t)stream) != hipSuccess) { scail_set_error("hipEventRecord failed"); return 2; }
            for (int j = 0; j < (B < 2 ? (int)B : 2); ++j) {
                if (hipStreamWaitEvent((hipStream_t)sp->side_stream[j], h->sp_ev[0], 0) != hipSuccess) { scail_set_error("hipStreamWaitEvent failed"); return 2; }
                sj.n = j + 1;
            }
        }
        for (int64_t b = 0; b < B; ++b) {
            void* s = st(b);
            scail_bf16* qb = qkv + b * Ltok * 3 * D;
            scail_bf16* send = sp->send + b * 3 * N * slab;             // [N][Ltok][3 Dn]: ONE message per destination rank, q | k | v side by side
            DIT_PROF_S(SCAIL_DIT_PROF_GEMM, s, scail_gemm_bf16(bf.xn + b * Ltok * D, D, lw.qkv_w, lw.qkv_b, qb, 3 * D, Ltok, 3 * D, D, SCAIL_EPI_BIAS, nullptr, 0, nullptr, 0, 0, s));
            // the norm + RoPE kernels write the send layout themselves; v is a plain copy into it
            DIT_TRY(scail_rmsnorm_rope_slabs(qb + D, 3 * D, send + Dn, Dn, 3 * Dn, 3 * slab, lw.kn, rope_cos, rope_sin, Ltok, Ltok, D, 128, eps, 1.0f, s));
            DIT_TRY(scail_rmsnorm_rope_slabs(qb, 3 * D, send, Dn, 3 * Dn, 3 * slab, lw.qn, rope_cos, rope_sin, Ltok, Ltok, D, 128, eps, ATTN_LOG2_SCALE, s));
            DIT_TRY(scail_rmsnorm_rope_slabs(qb + 2 * D, 3 * D, send + 2 * Dn, Dn, 3 * Dn, 3 * slab, nullptr, nullptr, nullptr, Ltok, Ltok, D, 128, eps, 1.0f, s));
            DIT_TRY(sp_exchange(sp, SCAIL_SP_FWD_START, i, b, s));
        }
        for (int64_t b = 0; b < B; ++b) {
            void* s = st(b);
            // exposed wait: the event pair brackets nothing but the stream's wait for the collective (0 when it finished under other work)
            DIT_PROF_S(SCAIL_DIT_PROF_XCH_FWD_WAIT, s, sp_exchange(sp, SCAIL_SP_FWD_WAIT, i, b, s));
            const scail_bf16* recv = sp->recv + b * 3 * N * slab;       // [N * Ltok][3 Dn]: all ranks' tokens (rank-major), q | k | v of my heads
            scail_bf16* vt = bf.vt + b * Hn * 128 * Lfp;
            scail_bf16* of = sp->ofull + b * N * slab;
            const bool vrows = scail_flash_attn_vrows_for(3 * Dn, 3 * Dn, 3 * Dn, Dn, 1, Hn, Lf, Lf) != 0;      // (dit_block)
            if (!vrows) DIT_TRY(scail_transpose_v(recv + 2 * Dn, 3 * Dn, 0, vt, 1, Hn, 128, Lf, s));
            // two elements' launches run side by side on the two streams and fill each other's partial rounds: one 256-row launch each
            // (a lone launch gets the planned shape: whole 256-row rounds + 192-row tiles for the rest, csrc/attn.hip attn4_plan)
            struct Hint { Hint(int r) { scail_attn4_rows_hint(r); } ~Hint() { scail_attn4_rows_hint(0); } } hint(side && B > 1 ? 256 : 0);
            if (vrows) {
                DIT_PROF_S(SCAIL_DIT_PROF_SELF_ATTN, s, scail_flash_attn_vrows_bf16(recv, 0, 3 * Dn, recv + Dn, 0, 3 * Dn, recv + 2 * Dn, 0, 3 * Dn, of, 0, Dn, 1, Hn,
                                                                                    Lf, Lf, SCAIL_ATTN_Q_PRESCALED, s));
            } else {
                DIT_PROF_S(SCAIL_DIT_PROF_SELF_ATTN, s, scail_flash_attn_bf16(recv, 0, 3 * Dn, recv + Dn, 0, 0, 3 * Dn, vt, 0, 0, of, 0, Dn, 1, Hn, Lf, Lf, 1,
                                                                              SCAIL_ATTN_Q_PRESCALED, 0, s));
            }
            DIT_TRY(sp_exchange(sp, SCAIL_SP_BACK_START, i, b, s));
        }
        for (int64_t b = 0; b < B; ++b) {
            void* s = st(b);
            DIT_PROF_S(SCAIL_DIT_PROF_XCH_BACK_WAIT, s, sp_exchange(sp, SCAIL_SP_BACK_WAIT, i, b, s));
            // back[b][g] = my tokens, head group g  ->  att rows (token, all columns)
            DIT_TRY(scail_slabs_to_rows(sp->back + b * N * slab, Dn, slab, bf.att + b * Ltok * D, D, Ltok, D, s));
        }
        if (sj.join() != 0) {
            scail_set_error("scail_dit (sequence parallel): joining the side streams failed");
            return 2;
        }
    } else {
        // ONE exchange per layer: all-gather of the post-norm, post-RoPE K rows and of the V rows; K / V projection per element first
        // so that element b's gather runs under element b + 1's projection and the Q projection of all elements.
        const int64_t rowsD = Ltok * D;
        for (int64_t b = 0; b < B; ++b) {
            scail_bf16* qb = qkv + b * Ltok * 3 * D;
            scail_bf16* send = sp->send + b * 2 * rowsD;                // [Ltok][2 D]: ONE message, k | v side by side
            const scail_bf16* xb = bf.xn + b * rowsD;
            DIT_PROF(SCAIL_DIT_PROF_GEMM, scail_gemm_bf16(xb, D, lw.qkv_w + D * D, lw.qkv_b + D, qb + D, 3 * D, Ltok, D, D, SCAIL_EPI_BIAS, nullptr, 0, nullptr, 0, 0, stream));
            DIT_PROF(SCAIL_DIT_PROF_GEMM, scail_gemm_bf16(xb, D, lw.qkv_w + 2 * D * D, lw.qkv_b + 2 * D, send + D, 2 * D, Ltok, D, D, SCAIL_EPI_BIAS, nullptr, 0, nullptr, 0, 0, stream));
            DIT_TRY(scail_rmsnorm_rope(qb + D, 3 * D, send, 2 * D, lw.kn, rope_cos, rope_sin, Ltok, Ltok, D, 128, eps, stream));
            DIT_TRY(sp_exchange(sp, SCAIL_SP_FWD_START, i, b, stream));
        }
        if (rows == Ltok) {
            DIT_PROF(SCAIL_DIT_PROF_GEMM, scail_gemm_bf16(bf.xn, D, lw.qkv_w, lw.qkv_b, q, 3 * D, B * Ltok, D, D, SCAIL_EPI_BIAS, nullptr, 0, nullptr, 0, 0, stream));
            DIT_TRY(scail_rmsnorm_rope_scaled(q, 3 * D, q, 3 * D, lw.qn, rope_cos, rope_sin, B * Ltok, Ltok, D, 128, eps, ATTN_LOG2_SCALE, stream));
        } else {
            for (int64_t b = 0; b < B; ++b) {       // the wanted rows' queries only (their RoPE rows start at row0)
                scail_bf16* qr = q + (b * Ltok + row0) * 3 * D;
                DIT_PROF(SCAIL_DIT_PROF_GEMM, scail_gemm_bf16(bf.xn + (b * Ltok + row0) * D, D, lw.qkv_w, lw.qkv_b, qr, 3 * D, rows, D, D, SCAIL_EPI_BIAS, nullptr, 0, nullptr, 0, 0, stream));
                DIT_TRY(scail_rmsnorm_rope_scaled(qr, 3 * D, qr, 3 * D, lw.qn, rope_cos + row0 * 64, rope_sin + row0 * 64, rows, rows, D, 128, eps, ATTN_LOG2_SCALE, stream));
            }
        }
        for (int64_t b = 0; b < B; ++b) {
            DIT_PROF(SCAIL_DIT_PROF_XCH_FWD_WAIT, sp_exchange(sp, SCAIL_SP_FWD_WAIT, i, b, stream));
            const scail_bf16* recv = sp->recv + b * 2 * N * rowsD;      // [N * Ltok][2 D]: gathered rows (rank-major), k | v
            scail_bf16* vt = bf.vt + b * nh * 128 * Lfp;
            if (scail_flash_attn_vrows_for(3 * D, 2 * D, 2 * D, D, 1, nh, rows, Lf) != 0) {                       // (dit_block)
                DIT_PROF(SCAIL_DIT_PROF_SELF_ATTN, scail_flash_attn_vrows_bf16(q + (b * Ltok + row0) * 3 * D, 0, 3 * D, recv, 0, 2 * D, recv + D, 0, 2 * D,
                                                                               bf.att + b * rowsD + row0 * D, 0, D, 1, nh, rows, Lf, SCAIL_ATTN_Q_PRESCALED, stream));
                continue;
            }
            DIT_TRY(scail_transpose_v(recv + D, 2 * D, 0, vt, 1, nh, 128, Lf, stream));
            DIT_PROF(SCAIL_DIT_PROF_SELF_ATTN, scail_flash_attn_bf16(q + (b * Ltok + row0) * 3 * D, 0, 3 * D, recv, 0, 0, 2 * D, vt, 0, 0, bf.att + b * rowsD + row0 * D, 0, D,
                                                                     1, nh, rows, Lf, 1, SCAIL_ATTN_Q_PRESCALED, 0, stream));
        }
    }
    return block_tail(h, i, hid, m, cond, Btot, Ltok, bf, row0, rows, pair, stream, CondAt{Btot, 0});
}

// Seam B2 (SAT hook layer_forward): one block on caller-owned hidden states.  Workspace: scail_dit_block_workspace_bytes.
extern "C" int64_t scail_dit_block_workspace_bytes(const scail_dit* h, int64_t B, int64_t Ltok) {
    if (h == nullptr || B <= 0 || Ltok <= 0) return -1;
    return block_ws(h, B, Ltok).end;
}
extern "C" int64_t scail_dit_block_sp_workspace_bytes(const scail_dit* h, int32_t mode, int32_t ranks, int64_t B, int64_t Ltok) {
    if (h == nullptr || B <= 0 || Ltok <= 0 || !sp_group_ok(h->cfg, mode, ranks)) return -1;
    return block_ws(h, B, Ltok, mode, ranks).end;
}
extern "C" int scail_dit_block_sp(scail_dit* h, int64_t layer, scail_bf16* hidden, const float* mod, const scail_dit_cond* cond,
                                  const float* rope_cos, const float* rope_sin, int64_t B, int64_t Ltok, const scail_dit_sp* sp,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    SCAIL_REQUIRE(h != nullptr && hidden != nullptr && mod != nullptr && cond != nullptr, "null argument");
    SCAIL_REQUIRE(layer >= 0 && layer < h->cfg.num_layers && B > 0 && Ltok > 0, "bad layer / shape");
    DIT_TRY(sp_check(h, sp));
    const BlockWs s = block_ws(h, B, Ltok, sp->mode, sp->ranks);
    SCAIL_REQUIRE(workspace != nullptr && workspace_bytes >= s.end && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
                  "workspace too small or not 256-byte aligned (scail_dit_block_sp_workspace_bytes)");
    return dit_block_sp(h, layer, hidden, mod, cond, rope_cos, rope_sin, B, Ltok, s.bufs(workspace), sp, 0, Ltok, false, stream);
}
extern "C" int scail_dit_block(scail_dit* h, int64_t layer, scail_bf16* hidden, const float* mod, const scail_dit_cond* cond,
                               const float* rope_cos, const float* rope_sin, int64_t B, int64_t Ltok,
                               void* workspace, int64_t workspace_bytes, void* stream) {
    SCAIL_REQUIRE(h != nullptr && hidden != nullptr && mod != nullptr && cond != nullptr, "null argument");
    SCAIL_REQUIRE(layer >= 0 && layer < h->cfg.num_layers && B > 0 && Ltok > 0, "bad layer / shape");
    const BlockWs s = block_ws(h, B, Ltok);
    SCAIL_REQUIRE(workspace != nullptr && workspace_bytes >= s.end && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
                  "workspace too small or not 256-byte aligned (scail_dit_block_workspace_bytes)");
    DIT_TRY(probe_check(h, B * Ltok));
    return dit_block(h, layer, hidden, mod, cond, rope_cos, rope_sin, B, Ltok, s.bufs(workspace), 0, Ltok, false, stream, CondAt{B, 0});
}

extern "C" int scail_dit_create(const scail_dit_config* cfg, const scail_dit_weights* w, scail_dit** out) {
    SCAIL_REQUIRE(cfg != nullptr && w != nullptr && out != nullptr, "null argument");
    SCAIL_REQUIRE(cfg->hidden_size > 0 && cfg->hidden_size % 128 == 0 && cfg->num_heads * 128 == cfg->hidden_size,
                  "hidden_size must be heads * 128");
    SCAIL_REQUIRE(cfg->num_layers > 0 && cfg->inner_hidden_size % 64 == 0 && cfg->time_embed_dim > 0 && cfg->time_freq_dim > 0,
                  "bad layer count / widths");
    SCAIL_REQUIRE(w->layers != nullptr, "weights.layers is null");
    scail_dit* h = new scail_dit;
    h->cfg = *cfg;
    h->w = *w;
    // the generated kernels live in embedded code objects loaded on first use: do it here, not inside a stream capture of the first
    // step (the per-shape tile-order table of the GEMM is still allocated by the first launch of a shape: warm up once before capturing)
    if (int rc = scail_attn4_preload()) { delete h; return rc; }
    if (int rc = scail_gemm4_preload()) { delete h; return rc; }
    h->layers.assign(w->layers, w->layers + cfg->num_layers);
    h->w.layers = h->layers.data();
    *out = h;
    return 0;
}

extern "C" void scail_dit_destroy(scail_dit* h) {
    if (h != nullptr) {
        for (ProfPool& p : h->pool)
            for (hipEvent_t e : p.ev) (void)hipEventDestroy(e);
        for (hipEvent_t e : h->sp_ev)
            if (e != nullptr) (void)hipEventDestroy(e);
        if (h->restart_ctr != nullptr) (void)hipFree(h->restart_ctr);
    }
    delete h;
}

// ---- fp8 per-token GEMMs (include/scail_dit.h scail_dit_enable_fp8) ----
// caller buffer layout: for every layer, for every selected GEMM in bit order, the e4m3 codes [N, K] then the fp32 scales [N] (per-row
// scaling) or the E8M0 block scales [N, K / 32] (MX), each block 256-byte aligned
// (fp6: the packed e2m3 codes [N, 3 K / 4 bytes] then the E8M0 block scales)
static int64_t fp8_scale_bytes(int scaling, int64_t N, int64_t K) { return scaling != SCAIL_DIT_FP8_SCALE_ROW ? N * (K / 32) : N * 4; }
static int64_t fp8_code_bytes(int scaling, int64_t N, int64_t K) { return scaling == QFORM_FP6 ? N * (K / 4 * 3) : N * K; }
static int fp8_scaling_check(const char* fn, int scaling) {
    if (scaling == SCAIL_DIT_FP8_SCALE_ROW || scaling == SCAIL_DIT_FP8_SCALE_MX) return 0;
    scail_set_error(std::string(fn) + ": unknown scaling " + std::to_string(scaling) + " (SCAIL_DIT_FP8_SCALE_ROW = 0 or SCAIL_DIT_FP8_SCALE_MX = 1)");
    return 1;
}
static int64_t fp8_weight_bytes(const scail_dit_config& c, uint32_t which, int scaling) {
    int64_t per_layer = 0;
    for (int g = 0; g < G_COUNT; ++g)
        if (which & (1u << g)) {
            int64_t N, K;
            gemm_shape(c, g, &N, &K);
            per_layer += align256(fp8_code_bytes(scaling, N, K)) + align256(fp8_scale_bytes(scaling, N, K));
        }
    return per_layer * c.num_layers;
}
extern "C" int64_t scail_dit_fp8_weight_bytes_scaled(const scail_dit* h, uint32_t which, int scaling) {
    if (h == nullptr || (which & ~(uint32_t)SCAIL_DIT_FP8_ALL) != 0 || fp8_scaling_check("scail_dit_fp8_weight_bytes_scaled", scaling)) return -1;
    return fp8_weight_bytes(h->cfg, which, scaling);
}
extern "C" int64_t scail_dit_fp8_weight_bytes(const scail_dit* h, uint32_t which) {
    return scail_dit_fp8_weight_bytes_scaled(h, which, SCAIL_DIT_FP8_SCALE_ROW);
}
// scail_dit_enable_fp8_scaled and scail_dit_enable_fp6: `scaling` is a SCAIL_DIT_FP8_SCALE_* or QFORM_FP6
// (errors carry the public entry's name, as SCAIL_REQUIRE would give them there)
static int enable_quantised(scail_dit* h, uint32_t which, int scaling, void* buf, int64_t bytes, void* stream) {
    const char* const fn = scaling == QFORM_FP6 ? "scail_dit_enable_fp6" : "scail_dit_enable_fp8_scaled";
#define QREQ(cond, msg)                                                                  \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            scail_set_error(std::string(fn) + ": " + (msg) + " [" #cond "]");            \
            return 1;                                                                    \
        }                                                                                \
    } while (0)
    QREQ(h != nullptr, "null handle");
    QREQ((which & ~(uint32_t)SCAIL_DIT_FP8_ALL) == 0, "unknown SCAIL_DIT_FP8_* bit");
    // a new set of quantised matrices: the per-layer selection and the probe (whose buffers were sized for the old set) start over
    h->fp8_sel.clear();
    probe_off(h);
    if (which == 0 || buf == nullptr) {     // back to bf16
        h->fp8 = 0;
        h->fp8_scaling = SCAIL_DIT_FP8_SCALE_ROW;
        h->fp8w.clear();
        return 0;
    }
    for (int g = 0; g < G_COUNT; ++g)
        if (which & (1u << g)) {
            int64_t N, K;
            gemm_shape(h->cfg, g, &N, &K);
            if (N % 128 != 0 || K % 128 != 0) {
                scail_set_error("scail_dit_enable_fp8: the " + std::string(k_gemm_names[g]) + " GEMM (N x K = " + std::to_string(N) + " x " +
                                std::to_string(K) + ") is outside scail_gemm_fp8's limits (N % 128 == 0, K % 128 == 0)");
                return 1;
            }
        }
    QREQ(bytes >= fp8_weight_bytes(h->cfg, which, scaling),
         scaling == QFORM_FP6 ? "buffer too small (scail_dit_fp6_weight_bytes)" : "buffer too small (scail_dit_fp8_weight_bytes_scaled)");
    QREQ((reinterpret_cast<uintptr_t>(buf) & 255) == 0, "buffer must be 256-byte aligned");
#undef QREQ
    h->fp8 = 0;                             // bf16 until every selected matrix is quantized
    h->fp8_scaling = SCAIL_DIT_FP8_SCALE_ROW;
    const bool mx = scaling != SCAIL_DIT_FP8_SCALE_ROW;      // block scales (MX and fp6) or fp32 row scales
    h->fp8w.assign(h->cfg.num_layers, {});
    char* p = static_cast<char*>(buf);
    for (int64_t i = 0; i < h->cfg.num_layers; ++i)
        for (int g = 0; g < G_COUNT; ++g) {
            if (!(which & (1u << g))) continue;
            int64_t N, K;
            gemm_shape(h->cfg, g, &N, &K);
            uint8_t* q = reinterpret_cast<uint8_t*>(p);
            float* sc = reinterpret_cast<float*>(p + align256(fp8_code_bytes(scaling, N, K)));
            uint8_t* ec = reinterpret_cast<uint8_t*>(sc);
            p += align256(fp8_code_bytes(scaling, N, K)) + align256(fp8_scale_bytes(scaling, N, K));
            if (int rc = scaling == QFORM_FP6 ? scail_quant_mxfp6_rows(gemm_weight(h->layers[i], g), K, q, K / 4 * 3, ec, K / 32, N, K, stream)
                         : mx ? scail_quant_mxfp8_rows(gemm_weight(h->layers[i], g), K, q, K, ec, K / 32, N, K, stream)
                            : scail_quant_fp8_rows(gemm_weight(h->layers[i], g), K, q, K, sc, N, K, stream)) {
                h->fp8w.clear();
                return rc;
            }
            h->fp8w[i][g] = {q, mx ? nullptr : sc, mx ? ec : nullptr};
        }
    h->fp8 = which;
    h->fp8_scaling = scaling;
    return 0;
}
extern "C" int scail_dit_enable_fp8_scaled(scail_dit* h, uint32_t which, int scaling, void* buf, int64_t bytes, void* stream) {
    if (fp8_scaling_check("scail_dit_enable_fp8_scaled", scaling)) return 1;
    return enable_quantised(h, which, scaling, buf, bytes, stream);
}
extern "C" int64_t scail_dit_fp6_weight_bytes(const scail_dit* h, uint32_t which) {
    if (h == nullptr || (which & ~(uint32_t)SCAIL_DIT_FP8_ALL) != 0) return -1;
    return fp8_weight_bytes(h->cfg, which, QFORM_FP6);
}
extern "C" int scail_dit_enable_fp6(scail_dit* h, uint32_t which, void* buf, int64_t bytes, void* stream) {
    return enable_quantised(h, which, QFORM_FP6, buf, bytes, stream);
}
extern "C" int scail_dit_enable_fp8(scail_dit* h, uint32_t which, void* buf, int64_t bytes, void* stream) {
    return scail_dit_enable_fp8_scaled(h, which, SCAIL_DIT_FP8_SCALE_ROW, buf, bytes, stream);
}

extern "C" int scail_dit_fp8_select_layers(scail_dit* h, const uint32_t* masks) {
    SCAIL_REQUIRE(h != nullptr, "null handle");
    if (masks == nullptr) {                 // uniform again: the enabled mask in every layer
        h->fp8_sel.clear();
        return 0;
    }
    for (int64_t i = 0; i < h->cfg.num_layers; ++i) {
        const uint32_t extra = masks[i] & ~h->fp8;
        if (extra == 0) continue;
        const uint32_t bit = extra & (~extra + 1u);      // the lowest offending bit
        int g = 0;
        while (g < G_COUNT && (1u << g) != bit) ++g;
        scail_set_error("scail_dit_fp8_select_layers: layer " + std::to_string(i) + " selects bit " + std::to_string(bit) +
                        (g < G_COUNT ? " (" + std::string(k_gemm_names[g]) + ")" : std::string(" (no SCAIL_DIT_FP8_* bit)")) +
                        ", which is outside the mask " + std::to_string(h->fp8) + " given to scail_dit_enable_fp8: only a quantised matrix can be selected");
        return 1;
    }
    h->fp8_sel.assign(masks, masks + h->cfg.num_layers);
    return 0;
}

// the probe's scratch: two bf16 result buffers of rows x fp8_n(), each 256-byte aligned
extern "C" int64_t scail_dit_fp8_probe_bytes(const scail_dit* h, int64_t B, int64_t Ltok) {
    if (h == nullptr || B <= 0 || Ltok <= 0 || B * Ltok >= (1ll << 31)) return -1;
    return 2 * align256(B * Ltok * fp8_n(h) * 2);
}
extern "C" int scail_dit_fp8_probe(scail_dit* h, double* table, void* scratch, int64_t scratch_bytes) {
    SCAIL_REQUIRE(h != nullptr, "null handle");
    probe_off(h);
    if (table == nullptr) return 0;
    SCAIL_REQUIRE(h->fp8 != 0, "no GEMM is quantised: call scail_dit_enable_fp8 first (the probe compares the quantised matrices with their bf16 twins)");
    SCAIL_REQUIRE((reinterpret_cast<uintptr_t>(table) & 7) == 0, "table must be 8-byte aligned");
    SCAIL_REQUIRE(scratch != nullptr && (reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "scratch must be a 256-byte aligned device buffer");
    const int64_t half = scratch_bytes / 2 / 256 * 256, rows = half / (fp8_n(h) * 2);
    SCAIL_REQUIRE(rows >= 1, "scratch too small for a single row (scail_dit_fp8_probe_bytes)");
    h->probe_table = table;
    h->probe_y16 = static_cast<scail_bf16*>(scratch);
    h->probe_y8 = reinterpret_cast<scail_bf16*>(static_cast<char*>(scratch) + half);
    h->probe_rows = rows;
    return 0;
}

extern "C" int scail_dit_profile(scail_dit* h, int enable) {
    SCAIL_REQUIRE(h != nullptr, "null handle");
    h->prof = enable != 0;
    if (h->prof) {
        for (ProfPool& p : h->pool) p.used = 0;       // a new measurement: reuse the pooled events
        // restart counter of the self-attention (SCAIL_DIT_PROF_ATTN_RESTARTS): allocated once, zeroed per measurement (blocking calls:
        // profiling is enabled outside of stream captures)
        if (h->restart_ctr == nullptr && hipMalloc(reinterpret_cast<void**>(&h->restart_ctr), sizeof(uint32_t)) != hipSuccess) {
            h->restart_ctr = nullptr;
            scail_set_error("scail_dit_profile: hipMalloc of the restart counter failed");
            return 2;
        }
        if (hipMemset(h->restart_ctr, 0, sizeof(uint32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
            scail_set_error("scail_dit_profile: clearing the restart counter failed");
            return 2;
        }
    }
    return 0;
}

extern "C" int scail_dit_profile_read(scail_dit* h, int category, double* ms_total, int64_t* launches) {
    SCAIL_REQUIRE(h != nullptr && ms_total != nullptr && launches != nullptr, "null argument");
    if (category == SCAIL_DIT_PROF_ATTN_RESTARTS) {
        // workgroups of the timed self-attention launches that left the optimistic pass and ran again (scail_hip.h
        // scail_flash_attn_count_restarts); read after the launches have finished
        ProfPool& pa = h->pool[SCAIL_DIT_PROF_SELF_ATTN];
        uint32_t n = 0;
        if ((pa.used >= 2 && hipEventSynchronize(pa.ev[pa.used - 1]) != hipSuccess) || h->restart_ctr == nullptr ||
            hipDeviceSynchronize() != hipSuccess || hipMemcpy(&n, h->restart_ctr, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess) {
            scail_set_error("scail_dit_profile_read: reading the restart counter failed (was profiling enabled?)");
            return 2;
        }
        *ms_total = 0.0;
        *launches = (int64_t)n;
        return 0;
    }
    SCAIL_REQUIRE(category >= 0 && category < PROF_CATS, "unknown category");
    ProfPool& p = h->pool[category];
    SCAIL_REQUIRE(p.used % 2 == 0, "unbalanced event pairs (a step failed between the marks)");
    double sum = 0.0;
    for (size_t i = 0; i + 1 < p.used; i += 2) {
        if (hipEventSynchronize(p.ev[i + 1]) != hipSuccess) {
            scail_set_error("scail_dit_profile_read: hipEventSynchronize failed");
            return 2;
        }
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, p.ev[i], p.ev[i + 1]) != hipSuccess) {
            scail_set_error("scail_dit_profile_read: hipEventElapsedTime failed");
            return 2;
        }
        sum += ms;
    }
    *ms_total = sum;
    *launches = (int64_t)(p.used / 2);
    return 0;
}

// The *_chars entry points take the character count; the entry points without it are their n_char == 1 form.
extern "C" int64_t scail_dit_chars_workspace_bytes(const scail_dit* h, int64_t B, int64_t T, int64_t H, int64_t W, int64_t n_char) {
    if (h == nullptr || shape_fault(B, T, H, W, n_char, 1) != 0) return -1;
    return layout(h, B, T, H, W, n_char).total;
}
extern "C" int64_t scail_dit_workspace_bytes(const scail_dit* h, int64_t B, int64_t T, int64_t H, int64_t W) {
    return scail_dit_chars_workspace_bytes(h, B, T, H, W, 1);
}
extern "C" int64_t scail_dit_sp_chars_workspace_bytes(const scail_dit* h, int32_t mode, int32_t ranks, int64_t B, int64_t T, int64_t H, int64_t W,
                                                      int64_t n_char) {
    if (h == nullptr || !sp_group_ok(h->cfg, mode, ranks) || shape_fault(B, T, H, W, n_char, ranks) != 0) return -1;
    return layout(h, B, T, H, W, n_char, mode, ranks).total;
}
extern "C" int64_t scail_dit_sp_workspace_bytes(const scail_dit* h, int32_t mode, int32_t ranks, int64_t B, int64_t T, int64_t H, int64_t W) {
    return scail_dit_sp_chars_workspace_bytes(h, mode, ranks, B, T, H, W, 1);
}

// x (B, T, 16, H, W): the whole latent (sp == nullptr) or this rank's H- or W-slab of it (rope tables rank-shifted by the host).
// n_char characters: ref (n_ref, n_char, 16, H, W), pose (n_pose, pose_frames = n_char * T, 16, H/2, W/2); a rank's slab holds its H- or
// W-window of EVERY character's reference frame and pose stream, so its token rows are [ref_0..ref_{C-1} | noise | pose_0..pose_{C-1}] of
// the slab, as on one rank (scail_amd/parallel.py chunks ref and pose like the latent).
static int dit_step_impl(scail_dit* h, const float* x, const float* timesteps, const scail_dit_cond* cond,
                         const scail_bf16* ref, int64_t n_ref, const scail_bf16* pose, int64_t n_pose, int64_t n_char, int64_t pose_frames,
                         const float* rope_cos, const float* rope_sin, float* out,
                         int64_t B, int64_t T, int64_t H, int64_t W, const scail_dit_sp* sp, uint32_t flags, void* workspace, int64_t workspace_bytes,
                         void* stream, int mode = CACHE_NONE, scail_bf16* cache_r = nullptr, scail_bf16* cache_emb = nullptr,
                         int64_t cond_batch = 0, int64_t cond_elem = 0) {
    // cond_batch > 0 (scail_dit_step_branch): the call's elements read elements cond_elem .. of a conditioning that holds cond_batch
    const CondAt ca = cond_batch > 0 ? CondAt{cond_batch, cond_elem} : CondAt{B, 0};
    DIT_TRY(chars_check("scail_dit_step", n_char, pose_frames, T));
    const bool reuse = mode == SCAIL_DIT_CACHE_REUSE;      // no block runs: the conditioning is not read
    SCAIL_REQUIRE(h != nullptr && (cond != nullptr || reuse), "null handle / conditioning");
    SCAIL_REQUIRE((flags & ~(uint32_t)SCAIL_DIT_CFG_PAIR) == 0, "unknown step flag");
    SCAIL_REQUIRE(!(flags & SCAIL_DIT_CFG_PAIR) || (B == 2 && n_ref == 1 && n_pose == 1),
                  "SCAIL_DIT_CFG_PAIR needs B == 2 with one shared ref / pose (element 1 = element 0 except for the conditioning)");
    const int64_t ranks = sp ? sp->ranks : 1;
    const int bad_shape = shape_fault(B, T, H, W, n_char, ranks);
    SCAIL_REQUIRE(B <= 8 && bad_shape != 1, "latent batch must be 1..8, H and W multiples of 4");
    if (bad_shape != 0) {
        scail_set_error("scail_dit_step: the self-attention takes fewer than 2^31 - 64 keys, got Ltok = " + std::to_string(tok_lens(n_char, T, H, W).Ltok) +
                        " tokens x " + std::to_string(ranks) + " rank(s) (T, H, W must be below 32768)");
        return 1;
    }
    SCAIL_REQUIRE((n_ref == 1 || n_ref == B) && (n_pose == 1 || n_pose == B), "ref / pose batch must be 1 or B");
    SCAIL_REQUIRE(reuse || cond->Bc == 1 || cond->Bc == ca.Btot, "clip batch must be 1 or B");
    const scail_dit_config& c = h->cfg;
    const Ws s = sp ? layout(h, B, T, H, W, n_char, sp->mode, sp->ranks) : layout(h, B, T, H, W, n_char);
    SCAIL_REQUIRE(c.time_embed_dim == c.hidden_size, "final-layer table add needs time_embed_dim == hidden_size");
    SCAIL_REQUIRE(workspace != nullptr && workspace_bytes >= s.total, "workspace too small (scail_dit_workspace_bytes)");
    SCAIL_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "workspace must be 256-byte aligned");
    if (sp == nullptr && !reuse) DIT_TRY(probe_check(h, B * tok_lens(n_char, T, H, W).Ltok));

    const int64_t D = c.hidden_size, nl = c.num_layers;
    const float eps = c.layernorm_epsilon;
    const TokLens tl = tok_lens(n_char, T, H, W);
    const int64_t Lref = tl.Lref, Lnoise = tl.Lnoise, Lpose = tl.Lpose, Ltok = tl.Ltok, Lrn = Lref + Lnoise;   // noise rows: [Lref, Lrn)
    char* base = static_cast<char*>(workspace);
    auto B16 = [&](int64_t off) { return reinterpret_cast<scail_bf16*>(base + off); };
    auto F32 = [&](int64_t off) { return reinterpret_cast<float*>(base + off); };
    scail_bf16 *tok = B16(s.tok), *hid = B16(s.h), *xf = B16(s.xf), *tokout = B16(s.tokout);
    float *temb = F32(s.temb), *e1 = F32(s.e1), *emb = F32(s.emb), *adaln = F32(s.adaln), *mod = F32(s.mod);
    float *emb2 = F32(s.emb2), *fin = F32(s.fin);
    const scail_dit_weights& w = h->w;

    // ---- time / AdaLN tables (dit...:1521-1555, :1025-1028, :823) ----
    DIT_TRY(scail_timestep_embedding(timesteps, temb, B, c.time_freq_dim, stream));
    DIT_TRY(scail_small_linear(temb, w.time0_w, w.time0_b, e1, B, c.time_embed_dim, c.time_freq_dim, 0, 1, stream));
    DIT_TRY(scail_small_linear(e1, w.time2_w, w.time2_b, emb, B, c.time_embed_dim, c.time_embed_dim, 0, 0, stream));
    DIT_TRY(scail_small_linear(emb, w.adaln_w, w.adaln_b, adaln, B, 6 * D, c.time_embed_dim, 1, 0, stream));
    DIT_TRY(scail_adaln_table(adaln, w.adaln_tables, mod, nl, B, 6 * D, stream));
    {
        const int64_t n = B * D;
        hipLaunchKernelGGL(dup_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, emb, emb2, B, D);
        DIT_TRY(scail_check_launch("dit_step.dup_rows"));
    }
    DIT_TRY(scail_adaln_table(emb2, w.final_table, fin, 1, B, 2 * D, stream));

    // ---- patch embedding straight into the token layout [ref_0.. | noise | pose_0..] (dit...:99-130) ----
    // SCAIL_DIT_CFG_PAIR: the two elements are one latent under two conditionings (VanillaCFG, guiders.py:41-57) and stay equal until the
    // first cross attention of layer 0 (dit...:1009-1042): patch embedding and layer 0 up to the self-attention residual run once
    const bool pair = (flags & SCAIL_DIT_CFG_PAIR) != 0 && nl > 1;
    const int64_t Be = pair ? 1 : B;
    if (n_char == 1) {
        DIT_TRY(scail_patchify(x, ref, pose, tok, Be, n_ref, n_pose, T, H, W, KPAD, stream));
    } else {
        DIT_TRY(scail_patchify_chars(x, ref, pose, tok, Be, n_ref, n_pose, n_char, T, H, W, KPAD, stream));
    }
    // the step cache (include/scail_dit.h "step cache"): cache_r = what the blocks added to the noise rows at the last FILL, cache_emb =
    // FILL's copy of the embedded noise rows (the blocks work in place on hid), dead once scail_resid_store has run; the caller places
    // the two (cache_ptrs: one cache; scail_dit_sample_tiled_cached: a slab of r per tile and one shared embedding region)
    scail_bf16* hid_noise = hid + Lref * D;
    if (reuse) {
        // the noise rows of the patch embedding only (every GEMM row comes from its own input row: the bits of the full embedding), plus
        // the cached residual, into every element's noise rows; then straight to the final layer.  The cache is only read.
        for (int64_t b = 0; b < Be; ++b)
            DIT_TRY(scail_gemm_bf16(tok + (b * Ltok + Lref) * KPAD, KPAD, w.patch_w, w.patch_b, hid_noise + b * Ltok * D, D, Lnoise, D, KPAD,
                                    SCAIL_EPI_BIAS, nullptr, 0, nullptr, 0, 0, stream));
        DIT_TRY(scail_resid_apply(hid_noise, pair ? 0 : Ltok * D, cache_r, hid_noise, Ltok * D, B, Lnoise, D, stream));
    }
    for (int64_t b = 0; b < (reuse ? 0 : Be); ++b) {
        DIT_TRY(scail_gemm_bf16(tok + b * Ltok * KPAD, KPAD, w.patch_w, w.patch_b, hid + b * Ltok * D, D, Lrn, D, KPAD,
                                SCAIL_EPI_BIAS, nullptr, 0, nullptr, 0, 0, stream));
        DIT_TRY(scail_gemm_bf16(tok + (b * Ltok + Lrn) * KPAD, KPAD, w.pose_w, w.pose_b, hid + (b * Ltok + Lrn) * D, D, Lpose, D,
                                KPAD, SCAIL_EPI_BIAS, nullptr, 0, nullptr, 0, 0, stream));
    }

    if (mode == SCAIL_DIT_CACHE_FILL)
        for (int64_t b = 0; b < Be; ++b)
            if (hipMemcpyAsync(cache_emb + b * Lnoise * D, hid_noise + b * Ltok * D, (size_t)Lnoise * D * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream) !=
                hipSuccess) {
                scail_set_error("scail_dit_step_cached: hipMemcpyAsync failed");
                return 2;
            }

    const BlockBufs bf = s.blk.bufs(workspace);
    for (int64_t i = 0; i < (reuse ? 0 : nl); ++i) {
        // the last layer's output is only read at the noise tokens (final layer below): queries / out-projection / cross attention /
        // MLP of its ref and pose rows are skipped (23 % of that layer's post-K/V work; same result)
        const bool last = i == nl - 1;
        const int64_t row0 = last ? Lref : 0, rows = last ? Lnoise : Ltok;
        if (sp != nullptr) {
            DIT_TRY(dit_block_sp(h, i, hid, mod + i * B * 6 * D, cond, rope_cos, rope_sin, B, Ltok, bf, sp, row0, rows, pair && i == 0, stream));
        } else {
            DIT_TRY(dit_block(h, i, hid, mod + i * B * 6 * D, cond, rope_cos, rope_sin, B, Ltok, bf, row0, rows, pair && i == 0, stream, ca));
        }
    }

    // (under the pair flag the embedding exists once and serves both elements: batch stride 0)
    if (mode == SCAIL_DIT_CACHE_FILL) DIT_TRY(scail_resid_store(hid_noise, Ltok * D, cache_emb, pair ? 0 : Lnoise * D, cache_r, B, Lnoise, D, stream));

    // ---- final layer on the noise tokens only + unpatchify (dit...:818-835, :764-784) ----
    DIT_TRY(scail_ln_modulate(hid, D, xf, D, fin, fin + D, 2 * D, B, Lnoise, Ltok, Lref, D, eps, stream));
    DIT_TRY(scail_gemm_bf16(xf, D, w.final_w, w.final_b, tokout, 64, B * Lnoise, 64, D, SCAIL_EPI_BIAS, nullptr, 0, nullptr, 0, 0, stream));
    DIT_TRY(scail_unpatchify(tokout, out, B, T, H, W, stream));
    return 0;
}

extern "C" int scail_dit_step_chars(scail_dit* h, const float* x, const float* timesteps, const scail_dit_cond* cond,
                                    const scail_bf16* ref, int64_t n_ref, const scail_bf16* pose, int64_t n_pose, int64_t n_char, int64_t pose_frames,
                                    const float* rope_cos, const float* rope_sin, float* out,
                                    int64_t B, int64_t T, int64_t H, int64_t W, uint32_t flags, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
    return dit_step_impl(h, x, timesteps, cond, ref, n_ref, pose, n_pose, n_char, pose_frames, rope_cos, rope_sin, out, B, T, H, W, nullptr, flags,
                         workspace, workspace_bytes, stream);
}
extern "C" int scail_dit_step(scail_dit* h, const float* x, const float* timesteps, const scail_dit_cond* cond,
                              const scail_bf16* ref, int64_t n_ref, const scail_bf16* pose, int64_t n_pose,
                              const float* rope_cos, const float* rope_sin, float* out,
                              int64_t B, int64_t T, int64_t H, int64_t W, uint32_t flags, void* workspace, int64_t workspace_bytes,
                              void* stream) {
    return scail_dit_step_chars(h, x, timesteps, cond, ref, n_ref, pose, n_pose, 1, T, rope_cos, rope_sin, out, B, T, H, W, flags, workspace,
                                workspace_bytes, stream);
}

extern "C" int scail_dit_step_sp_chars(scail_dit* h, const float* x, const float* timesteps, const scail_dit_cond* cond,
                                       const scail_bf16* ref, int64_t n_ref, const scail_bf16* pose, int64_t n_pose, int64_t n_char,
                                       int64_t pose_frames, const float* rope_cos, const float* rope_sin, float* out,
                                       int64_t B, int64_t T, int64_t H, int64_t W, const scail_dit_sp* sp, uint32_t flags, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
    SCAIL_REQUIRE(h != nullptr, "null handle");
    DIT_TRY(sp_check(h, sp));
    return dit_step_impl(h, x, timesteps, cond, ref, n_ref, pose, n_pose, n_char, pose_frames, rope_cos, rope_sin, out, B, T, H, W, sp, flags,
                         workspace, workspace_bytes, stream);
}
extern "C" int scail_dit_step_sp(scail_dit* h, const float* x, const float* timesteps, const scail_dit_cond* cond,
                                 const scail_bf16* ref, int64_t n_ref, const scail_bf16* pose, int64_t n_pose,
                                 const float* rope_cos, const float* rope_sin, float* out,
                                 int64_t B, int64_t T, int64_t H, int64_t W, const scail_dit_sp* sp, uint32_t flags, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
    return scail_dit_step_sp_chars(h, x, timesteps, cond, ref, n_ref, pose, n_pose, 1, T, rope_cos, rope_sin, out, B, T, H, W, sp, flags, workspace,
                                   workspace_bytes, stream);
}

// ---- the sampler loop (RFSampler.__call__ + VanillaCFG, sampling.py:920-982, guiders.py:41-57) ----
extern "C" int64_t scail_dit_sample_chars_workspace_bytes(const scail_dit* h, int64_t T, int64_t H, int64_t W, int64_t n_char) {
    const int64_t step = scail_dit_chars_workspace_bytes(h, 2, T, H, W, n_char);
    return step < 0 ? -1 : sample_ws(step, T, H, W).total;
}
extern "C" int64_t scail_dit_sample_workspace_bytes(const scail_dit* h, int64_t T, int64_t H, int64_t W) {
    return scail_dit_sample_chars_workspace_bytes(h, T, H, W, 1);
}

extern "C" int scail_dit_sample(scail_dit* h, float* x, const float* timesteps, const float* dsigma, int64_t n_steps,
                                float cfg_scale, const scail_dit_cond* cond, const scail_bf16* ref, const scail_bf16* pose,
                                const float* rope_cos, const float* rope_sin, int64_t T, int64_t H, int64_t W,
                                void* workspace, int64_t workspace_bytes, void* stream) {
    return scail_dit_sample_chars(h, x, timesteps, dsigma, n_steps, cfg_scale, cond, ref, pose, 1, T, rope_cos, rope_sin, T, H, W, workspace,
                                  workspace_bytes, stream);
}

// the Euler loop; reuse == nullptr: every step a plain evaluation (scail_dit_sample_chars), else step i in SCAIL_DIT_CACHE_REUSE mode
// where reuse[i] != 0 and in SCAIL_DIT_CACHE_FILL mode otherwise (scail_dit_sample_cached, which has checked reuse and the cache).
// guide == nullptr: every step the batch-2 pair, else step i as its SCAIL_DIT_GUIDE_* entry says (scail_dit_sample_guided, which has
// checked the plan and the delta buffer).
// solver == nullptr: scail_cfg_euler updates x, else scail_cfg_multistep under row i of the plan, with `hist` (scail_dit_sample_solver,
// which has checked the plan and the history buffer); a solver plan goes with neither reuse nor guide
struct SolverPlan {
    const float *sigma, *coef;      // HOST fp32 [n_steps] and [n_steps][3]
};
static int sample_impl(scail_dit* h, float* x, const float* timesteps, const float* dsigma, int64_t n_steps,
                       float cfg_scale, const scail_dit_cond* cond, const scail_bf16* ref, const scail_bf16* pose,
                       int64_t n_char, int64_t pose_frames, const float* rope_cos, const float* rope_sin,
                       int64_t T, int64_t H, int64_t W, void* workspace, int64_t workspace_bytes, void* stream, const uint8_t* reuse, void* cache,
                       const uint8_t* guide = nullptr, float* delta = nullptr, const SolverPlan* solver = nullptr, float* hist = nullptr) {
    DIT_TRY(chars_check("scail_dit_sample", n_char, pose_frames, T));
    SCAIL_REQUIRE(h != nullptr && x != nullptr && timesteps != nullptr && dsigma != nullptr && n_steps >= 0, "null argument");
    const int64_t step_bytes = scail_dit_chars_workspace_bytes(h, 2, T, H, W, n_char);
    SCAIL_REQUIRE(step_bytes >= 0, "bad latent shape");
    const SampleWs ws = sample_ws(step_bytes, T, H, W);
    SCAIL_REQUIRE(workspace != nullptr && workspace_bytes >= ws.total, "workspace too small (scail_dit_sample_workspace_bytes)");
    // (the step refuses it too, but only after this loop has copied x into the workspace: a refused workspace is left untouched)
    SCAIL_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "workspace must be 256-byte aligned");
    DIT_TRY(probe_check(h, 2 * tok_lens(n_char, T, H, W).Ltok));
    char* base = static_cast<char*>(workspace);
    float *xin = reinterpret_cast<float*>(base + ws.xin), *v = reinterpret_cast<float*>(base + ws.v);
    const int64_t n = T * 16 * H * W;
    hipStream_t s = (hipStream_t)stream;
    const CachePtrs cp = reuse == nullptr ? CachePtrs{nullptr, nullptr} : cache_ptrs(h->cfg, 2, tok_lens(1, T, H, W).Lnoise, cache);
    const int64_t slot1 = tok_lens(1, T, H, W).Lnoise * h->cfg.hidden_size;      // element 1's slot of either cache region, in elements
    for (int64_t i = 0; i < n_steps; ++i) {
        const int mode = reuse == nullptr ? CACHE_NONE : reuse[i] ? SCAIL_DIT_CACHE_REUSE : SCAIL_DIT_CACHE_FILL;
        if (guide != nullptr && guide[i] != SCAIL_DIT_GUIDE_PAIR) {
            // the cond branch alone (scail_dit_step_branch, elem 1 of 2): B = 1 on x itself, which the evaluation only reads, in the
            // B = 1 layout of the same workspace; v_c lands where the pair's v_u does
            DIT_TRY(dit_step_impl(h, x, timesteps + 2 * i, cond, ref, 1, pose, 1, n_char, pose_frames, rope_cos, rope_sin, v, 1, T, H, W, nullptr, 0,
                                  workspace, step_bytes, stream, mode, mode ? cp.r + slot1 : nullptr, mode ? cp.emb + slot1 : nullptr, 2, 1));
            DIT_TRY(scail_cfg_euler_delta(x, v, guide[i] == SCAIL_DIT_GUIDE_DELTA ? delta : nullptr, n, cfg_scale, dsigma[i], stream));
            continue;
        }
        // torch.cat([x] * 2) of VanillaCFG.prepare_inputs (guiders.py:56)
        if (hipMemcpyAsync(xin, x, n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess ||
            hipMemcpyAsync(xin + n, x, n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) {
            scail_set_error("scail_dit_sample: hipMemcpyAsync failed");
            return 2;
        }
        DIT_TRY(dit_step_impl(h, xin, timesteps + 2 * i, cond, ref, 1, pose, 1, n_char, pose_frames, rope_cos, rope_sin, v, 2, T, H, W, nullptr,
                              SCAIL_DIT_CFG_PAIR, workspace, step_bytes, stream, mode, cp.r, cp.emb));
        if (guide != nullptr) DIT_TRY(scail_cfg_delta_store(v, delta, n, stream));
        if (solver != nullptr) {
            const float* co = solver->coef + 3 * i;
            DIT_TRY(scail_cfg_multistep(x, v, hist, n, cfg_scale, solver->sigma[i], co[0], co[1], co[2], co[2] != 0.0f, stream));
            continue;
        }
        DIT_TRY(scail_cfg_euler(x, v, n, cfg_scale, dsigma[i], stream));
    }
    return 0;
}
extern "C" int scail_dit_sample_chars(scail_dit* h, float* x, const float* timesteps, const float* dsigma, int64_t n_steps,
                                      float cfg_scale, const scail_dit_cond* cond, const scail_bf16* ref, const scail_bf16* pose,
                                      int64_t n_char, int64_t pose_frames, const float* rope_cos, const float* rope_sin,
                                      int64_t T, int64_t H, int64_t W, void* workspace, int64_t workspace_bytes, void* stream) {
    return sample_impl(h, x, timesteps, dsigma, n_steps, cfg_scale, cond, ref, pose, n_char, pose_frames, rope_cos, rope_sin, T, H, W, workspace,
                       workspace_bytes, stream, nullptr, nullptr);
}

// ---- the step cache (include/scail_dit.h "step cache") ----
extern "C" int64_t scail_dit_step_cache_bytes(const scail_dit* h, int64_t B, int64_t T, int64_t H, int64_t W) {
    if (h == nullptr || shape_fault(B, T, H, W, 1, 1) != 0) return -1;
    return cache_ws(h->cfg, B, tok_lens(1, T, H, W).Lnoise).total;
}
extern "C" int64_t scail_dit_sample_tiled_cache_bytes(const scail_dit* h, int64_t n_tiles, int64_t Tt, int64_t H, int64_t W) {
    if (h == nullptr || n_tiles < 2 || n_tiles >= (1 << 15) || Tt > 64 || shape_fault(2, Tt, H, W, 1, 1) != 0) return -1;
    const CacheWs cw = cache_ws(h->cfg, 2, tok_lens(1, Tt, H, W).Lnoise);
    return n_tiles * cw.emb + (cw.total - cw.emb);      // [n_tiles][R] slabs of r, then one embedding region E
}
// mode and cache of a *_cached call, before anything is enqueued: what needs no handle first (the message names the value).
// n_tiles = 0: the cache of one (B, T, H, W) evaluation, else the tiled sampler's (n_tiles slabs of r + one embedding region, B = 2)
static int cache_check(const char* who, const scail_dit* h, int mode, bool need_mode, const void* cache, int64_t cache_bytes, int64_t B, int64_t T,
                       int64_t H, int64_t W, int64_t n_tiles = 0) {
    const char* query = n_tiles ? "scail_dit_sample_tiled_cache_bytes" : "scail_dit_step_cache_bytes";
    auto fail = [&](const std::string& msg) {
        scail_set_error(std::string(who) + ": " + msg);
        return 1;
    };
    if (need_mode && mode != SCAIL_DIT_CACHE_FILL && mode != SCAIL_DIT_CACHE_REUSE)
        return fail("unknown cache mode " + std::to_string(mode) + " (SCAIL_DIT_CACHE_FILL = 1 or SCAIL_DIT_CACHE_REUSE = 2)");
    if (cache == nullptr) return fail("null cache (cache_bytes " + std::to_string(cache_bytes) + "; " + query + ")");
    if ((reinterpret_cast<uintptr_t>(cache) & 255) != 0)
        return fail("the cache must be 256-byte aligned, got an address that is " + std::to_string(reinterpret_cast<uintptr_t>(cache) & 255) + " past a multiple of 256");
    if (h == nullptr) return fail("null handle");
    const int64_t need = n_tiles ? scail_dit_sample_tiled_cache_bytes(h, n_tiles, T, H, W) : scail_dit_step_cache_bytes(h, B, T, H, W);
    if (need < 0) return fail("bad latent shape (B " + std::to_string(B) + ", T " + std::to_string(T) + ", H " + std::to_string(H) + ", W " + std::to_string(W) + ")");
    if (cache_bytes < need)
        return fail("cache too small: " + std::to_string(cache_bytes) + " bytes, needs " + std::to_string(need) + " (" + query + ")");
    return 0;
}
// the plan of a sampler loop with a step cache: host uint8 [n_steps], 0 = compute (FILL) or 1 = REUSE, the first step computes
static int reuse_check(const char* who, const uint8_t* reuse, int64_t n_steps) {
    if (n_steps <= 0) return 0;
    if (reuse == nullptr) {
        scail_set_error(std::string(who) + ": null reuse mask with n_steps = " + std::to_string(n_steps));
        return 1;
    }
    for (int64_t i = 0; i < n_steps; ++i)
        if (reuse[i] > 1) {
            scail_set_error(std::string(who) + ": reuse[" + std::to_string(i) + "] = " + std::to_string((int)reuse[i]) + " (an entry is 0 = compute or 1 = reuse)");
            return 1;
        }
    if (reuse[0] != 0) {
        scail_set_error(std::string(who) + ": reuse[0] = " + std::to_string((int)reuse[0]) + ": the first step has nothing to reuse, it must compute");
        return 1;
    }
    return 0;
}
extern "C" int scail_dit_step_cached(scail_dit* h, const float* x, const float* timesteps, const scail_dit_cond* cond,
                                     const scail_bf16* ref, int64_t n_ref, const scail_bf16* pose, int64_t n_pose, int64_t n_char, int64_t pose_frames,
                                     const float* rope_cos, const float* rope_sin, float* out,
                                     int64_t B, int64_t T, int64_t H, int64_t W, uint32_t flags, void* workspace, int64_t workspace_bytes,
                                     int mode, void* cache, int64_t cache_bytes, void* stream) {
    DIT_TRY(cache_check("scail_dit_step_cached", h, mode, true, cache, cache_bytes, B, T, H, W));
    const CachePtrs cp = cache_ptrs(h->cfg, B, tok_lens(1, T, H, W).Lnoise, cache);
    return dit_step_impl(h, x, timesteps, cond, ref, n_ref, pose, n_pose, n_char, pose_frames, rope_cos, rope_sin, out, B, T, H, W, nullptr, flags,
                         workspace, workspace_bytes, stream, mode, cp.r, cp.emb);
}
extern "C" int scail_dit_sample_cached(scail_dit* h, float* x, const float* timesteps, const float* dsigma, int64_t n_steps,
                                       float cfg_scale, const scail_dit_cond* cond, const scail_bf16* ref, const scail_bf16* pose,
                                       int64_t n_char, int64_t pose_frames, const float* rope_cos, const float* rope_sin,
                                       int64_t T, int64_t H, int64_t W, void* workspace, int64_t workspace_bytes,
                                       const uint8_t* reuse, void* cache, int64_t cache_bytes, void* stream) {
    const char* who = "scail_dit_sample_cached";
    DIT_TRY(reuse_check(who, reuse, n_steps));
    DIT_TRY(cache_check(who, h, 0, false, cache, cache_bytes, 2, T, H, W));
    return sample_impl(h, x, timesteps, dsigma, n_steps, cfg_scale, cond, ref, pose, n_char, pose_frames, rope_cos, rope_sin, T, H, W, workspace,
                       workspace_bytes, stream, reuse, cache);
}

// ---- the guidance plan (include/scail_dit.h "guidance plan") ----
extern "C" int scail_dit_step_branch(scail_dit* h, const float* x, const float* timesteps, const scail_dit_cond* cond, int64_t cond_batch, int64_t elem,
                                     const scail_bf16* ref, const scail_bf16* pose, int64_t n_char, int64_t pose_frames,
                                     const float* rope_cos, const float* rope_sin, float* out, int64_t T, int64_t H, int64_t W,
                                     void* workspace, int64_t workspace_bytes, int mode, void* cache, int64_t cache_bytes, void* stream) {
    const char* who = "scail_dit_step_branch";
    auto fail = [&](const std::string& msg) {
        scail_set_error(std::string(who) + ": " + msg);
        return 1;
    };
    if (cond_batch < 1 || cond_batch > 8) return fail("cond_batch must be 1..8, got " + std::to_string(cond_batch));
    if (elem < 0 || elem >= cond_batch)
        return fail("elem must lie in [0, cond_batch = " + std::to_string(cond_batch) + "), got " + std::to_string(elem));
    if (mode != CACHE_NONE && mode != SCAIL_DIT_CACHE_FILL && mode != SCAIL_DIT_CACHE_REUSE)
        return fail("unknown mode " + std::to_string(mode) + " (0 = no cache, SCAIL_DIT_CACHE_FILL = 1 or SCAIL_DIT_CACHE_REUSE = 2)");
    CachePtrs cp{nullptr, nullptr};
    if (mode != CACHE_NONE) {
        // the cache is the (2, T, H, W) step cache of the pair: element `elem`'s slot of r, and of the embedding region for FILL's copy
        if (elem > 1) return fail("a cache mode takes elem 0 or 1 (the step cache of the pair has two slots), got " + std::to_string(elem));
        DIT_TRY(cache_check(who, h, mode, true, cache, cache_bytes, 2, T, H, W));
        const int64_t slot = elem * tok_lens(1, T, H, W).Lnoise * h->cfg.hidden_size;
        cp = cache_ptrs(h->cfg, 2, tok_lens(1, T, H, W).Lnoise, cache);
        cp.r += slot;
        cp.emb += slot;
    }
    return dit_step_impl(h, x, timesteps, cond, ref, 1, pose, 1, n_char, pose_frames, rope_cos, rope_sin, out, 1, T, H, W, nullptr, 0, workspace,
                         workspace_bytes, stream, mode, cp.r, cp.emb, cond_batch, elem);
}

extern "C" int64_t scail_dit_guidance_bytes(int64_t T, int64_t H, int64_t W) {
    if (shape_fault(1, T, H, W, 1, 1) != 0) return -1;
    return align256(T * 16 * H * W * 4);
}
// whether an entry evaluates both elements (the pair) or element 1 alone
static bool guide_is_pair(uint8_t g) { return g == SCAIL_DIT_GUIDE_PAIR; }
extern "C" int scail_dit_sample_guided(scail_dit* h, float* x, const float* timesteps, const float* dsigma, int64_t n_steps, float cfg_scale,
                                       const scail_dit_cond* cond, const scail_bf16* ref, const scail_bf16* pose, int64_t n_char, int64_t pose_frames,
                                       const float* rope_cos, const float* rope_sin, int64_t T, int64_t H, int64_t W,
                                       void* workspace, int64_t workspace_bytes, const uint8_t* guide, void* delta, int64_t delta_bytes,
                                       const uint8_t* reuse, void* cache, int64_t cache_bytes, void* stream) {
    const char* who = "scail_dit_sample_guided";
    auto fail = [&](const std::string& msg) {
        scail_set_error(std::string(who) + ": " + msg);
        return 1;
    };
    if (n_steps < 0) return fail("n_steps must be >= 0, got " + std::to_string(n_steps));
    if (n_steps > 0 && guide == nullptr) return fail("null guide plan with n_steps = " + std::to_string(n_steps));
    bool seen_pair = false, needs_delta = false;
    for (int64_t i = 0; i < n_steps; ++i) {
        if (guide[i] > SCAIL_DIT_GUIDE_COND)
            return fail("guide[" + std::to_string(i) + "] = " + std::to_string((int)guide[i]) + " (an entry is 0 = pair, 1 = delta or 2 = cond)");
        if (guide[i] == SCAIL_DIT_GUIDE_DELTA && !seen_pair)
            return fail("guide[" + std::to_string(i) + "] = 1 (delta) has no pair step before it: there is no stored delta to use");
        seen_pair = seen_pair || guide_is_pair(guide[i]);
        needs_delta = needs_delta || guide[i] != SCAIL_DIT_GUIDE_COND;
    }
    if (needs_delta) {
        if (delta == nullptr) return fail("null delta buffer (delta_bytes " + std::to_string(delta_bytes) + "; scail_dit_guidance_bytes)");
        if ((reinterpret_cast<uintptr_t>(delta) & 255) != 0)
            return fail("the delta buffer must be 256-byte aligned, got an address that is " + std::to_string(reinterpret_cast<uintptr_t>(delta) & 255) +
                        " past a multiple of 256");
        const int64_t need = scail_dit_guidance_bytes(T, H, W);
        if (need < 0) return fail("bad latent shape (T " + std::to_string(T) + ", H " + std::to_string(H) + ", W " + std::to_string(W) + ")");
        if (delta_bytes < need)
            return fail("delta buffer too small: " + std::to_string(delta_bytes) + " bytes, needs " + std::to_string(need) + " (scail_dit_guidance_bytes)");
    }
    if (reuse != nullptr) {
        DIT_TRY(reuse_check(who, reuse, n_steps));
        // a reusing step finds the residual slots its last FILL wrote: the pair fills both, a branch step element 1's alone
        for (int64_t i = 0, j = 0; i < n_steps; ++i) {
            if (reuse[i] == 0) {
                j = i;
            } else if (guide_is_pair(guide[i]) != guide_is_pair(guide[j])) {
                return fail("step " + std::to_string(i) + " reuses (guide " + std::to_string((int)guide[i]) + ") what step " + std::to_string(j) +
                            ", the last computing step, left (guide " + std::to_string((int)guide[j]) +
                            "): they do not evaluate the same elements (0 goes with 0; 1 or 2 with 1 or 2)");
            }
        }
        DIT_TRY(cache_check(who, h, 0, false, cache, cache_bytes, 2, T, H, W));
    }
    // (n_steps == 0: guide may be null; the loop below does not run)
    static const uint8_t none = 0;
    return sample_impl(h, x, timesteps, dsigma, n_steps, cfg_scale, cond, ref, pose, n_char, pose_frames, rope_cos, rope_sin, T, H, W, workspace,
                       workspace_bytes, stream, reuse, cache, guide != nullptr ? guide : &none, static_cast<float*>(delta));
}

// ---- the solver plan (include/scail_dit.h "solver plan") ----
extern "C" int64_t scail_dit_solver_bytes(int64_t T, int64_t H, int64_t W) {
    // (not shape_fault: the history is the FULL latent of a tiled clip, whose token count no single evaluation has to hold)
    if (T <= 0 || H <= 0 || W <= 0 || H % 4 != 0 || W % 4 != 0 || T >= (1 << 15) || H >= (1 << 15) || W >= (1 << 15)) return -1;
    return align256(T * 16 * H * W * 4);
}
// the plan and the history buffer of a *_solver call, before anything is enqueued (host only; the message names index and value)
static int solver_check(const char* who, int64_t n_steps, const float* sigma, const float* coef, const void* hist, int64_t hist_bytes,
                        int64_t T, int64_t H, int64_t W) {
    auto fail = [&](const std::string& msg) {
        scail_set_error(std::string(who) + ": " + msg);
        return 1;
    };
    if (n_steps < 0) return fail("n_steps must be >= 0, got " + std::to_string(n_steps));
    if (n_steps > 0 && sigma == nullptr) return fail("null solver sigma with n_steps = " + std::to_string(n_steps));
    if (n_steps > 0 && coef == nullptr) return fail("null solver coefficients with n_steps = " + std::to_string(n_steps));
    for (int64_t i = 0; i < n_steps; ++i) {
        if (!std::isfinite(sigma[i])) return fail("sigma[" + std::to_string(i) + "] = " + std::to_string(sigma[i]) + " is not finite");
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(coef[3 * i + k]))
                return fail("coef[" + std::to_string(i) + "][" + std::to_string(k) + "] = " + std::to_string(coef[3 * i + k]) + " is not finite");
    }
    if (n_steps > 0 && coef[2] != 0.0f)
        return fail("coef[0][2] = " + std::to_string(coef[2]) + " must be 0: step 0 has no history to use");
    if (hist == nullptr) return fail("null history buffer (hist_bytes " + std::to_string(hist_bytes) + "; scail_dit_solver_bytes)");
    if ((reinterpret_cast<uintptr_t>(hist) & 255) != 0)
        return fail("the history buffer must be 256-byte aligned, got an address that is " + std::to_string(reinterpret_cast<uintptr_t>(hist) & 255) +
                    " past a multiple of 256");
    const int64_t need = scail_dit_solver_bytes(T, H, W);
    if (need < 0) return fail("bad latent shape (T " + std::to_string(T) + ", H " + std::to_string(H) + ", W " + std::to_string(W) + ")");
    if (hist_bytes < need)
        return fail("history buffer too small: " + std::to_string(hist_bytes) + " bytes, needs " + std::to_string(need) + " (scail_dit_solver_bytes)");
    return 0;
}
extern "C" int scail_dit_sample_solver(scail_dit* h, float* x, const float* timesteps, const float* dsigma, int64_t n_steps, float cfg_scale,
                                       const scail_dit_cond* cond, const scail_bf16* ref, const scail_bf16* pose, int64_t n_char, int64_t pose_frames,
                                       const float* rope_cos, const float* rope_sin, int64_t T, int64_t H, int64_t W,
                                       void* workspace, int64_t workspace_bytes, const float* sigma, const float* coef, void* hist,
                                       int64_t hist_bytes, void* stream) {
    DIT_TRY(solver_check("scail_dit_sample_solver", n_steps, sigma, coef, hist, hist_bytes, T, H, W));
    const SolverPlan plan{sigma, coef};
    return sample_impl(h, x, timesteps, dsigma, n_steps, cfg_scale, cond, ref, pose, n_char, pose_frames, rope_cos, rope_sin, T, H, W, workspace,
                       workspace_bytes, stream, nullptr, nullptr, nullptr, nullptr, &plan, static_cast<float*>(hist));
}

// ---- the decision signal of the step cache: distances of consecutive steps' time embeddings (include/scail_dit.h) ----
constexpr int64_t TD_CHUNK = 8;     // scail_small_linear takes M <= 8
// temb | e1 | emb | adaln: the signal's buffer holds TD_CHUNK + 1 rows -- row 0 is the last step of the chunk before
struct TimeDistWs {
    int64_t temb, e1, emb, adaln, total;
};
static TimeDistWs time_dist_ws(const scail_dit_config& c, int signal) {
    Carve cv;
    TimeDistWs s;
    s.temb = cv.take(TD_CHUNK * c.time_freq_dim * 4);
    s.e1 = cv.take(TD_CHUNK * c.time_embed_dim * 4);
    s.emb = cv.take((TD_CHUNK + 1) * c.time_embed_dim * 4);
    s.adaln = cv.take(signal == 1 ? (TD_CHUNK + 1) * 6 * (int64_t)c.hidden_size * 4 : 0);
    s.total = cv.off;
    return s;
}
extern "C" int64_t scail_dit_time_distances_bytes(const scail_dit* h, int signal) {
    if (h == nullptr || (signal != 0 && signal != 1)) return -1;
    return time_dist_ws(h->cfg, signal).total;
}
extern "C" int scail_dit_time_distances(scail_dit* h, const float* timesteps, int64_t n_steps, int signal, double* out, void* scratch,
                                        int64_t scratch_bytes, void* stream) {
    const char* who = "scail_dit_time_distances";
    auto fail = [&](const std::string& msg) {
        scail_set_error(std::string(who) + ": " + msg);
        return 1;
    };
    if (signal != 0 && signal != 1) return fail("unknown signal " + std::to_string(signal) + " (0 = the time embedding, 1 = its AdaLN projection)");
    if (n_steps < 0 || n_steps >= (1 << 20)) return fail("n_steps must be 0 .. 2^20 - 1, got " + std::to_string(n_steps));
    if (h == nullptr) return fail("null handle");
    if (n_steps == 0) return 0;
    if (timesteps == nullptr || out == nullptr) return fail("null pointer: timesteps / out");
    if ((reinterpret_cast<uintptr_t>(out) & 7) != 0) return fail("out must be 8-byte aligned");
    const scail_dit_config& c = h->cfg;
    const TimeDistWs s = time_dist_ws(c, signal);
    if (scratch == nullptr || scratch_bytes < s.total)
        return fail("scratch too small: " + std::to_string(scratch_bytes) + " bytes, needs " + std::to_string(s.total) + " (scail_dit_time_distances_bytes)");
    if ((reinterpret_cast<uintptr_t>(scratch) & 255) != 0) return fail("scratch must be 256-byte aligned");
    char* base = static_cast<char*>(scratch);
    float *temb = reinterpret_cast<float*>(base + s.temb), *e1 = reinterpret_cast<float*>(base + s.e1), *emb = reinterpret_cast<float*>(base + s.emb),
          *adaln = reinterpret_cast<float*>(base + s.adaln);
    const scail_dit_weights& w = h->w;
    const int64_t Dt = c.time_embed_dim, width = signal == 1 ? 6 * (int64_t)c.hidden_size : Dt;
    float* v = signal == 1 ? adaln : emb;            // rows 1 .. m: this chunk's steps; row 0: the step before the chunk
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, 2 * sizeof(double), st) != hipSuccess) {      // out[0] = {0, 0}: the first step has no predecessor
        scail_set_error(std::string(who) + ": hipMemsetAsync failed");
        return 2;
    }
    for (int64_t s0 = 0; s0 < n_steps; s0 += TD_CHUNK) {
        const int64_t m = std::min(TD_CHUNK, n_steps - s0);
        // the step's own composition (dit_step_impl): sinusoid -> time_embed.0 + SiLU -> time_embed.2 [-> SiLU + adaln_projection.1]
        DIT_TRY(scail_timestep_embedding(timesteps + s0, temb, m, c.time_freq_dim, stream));
        DIT_TRY(scail_small_linear(temb, w.time0_w, w.time0_b, e1, m, Dt, c.time_freq_dim, 0, 1, stream));
        DIT_TRY(scail_small_linear(e1, w.time2_w, w.time2_b, emb + Dt, m, Dt, Dt, 0, 0, stream));
        if (signal == 1) DIT_TRY(scail_small_linear(emb + Dt, w.adaln_w, w.adaln_b, adaln + width, m, width, Dt, 1, 0, stream));
        for (int64_t j = s0 == 0 ? 1 : 0; j < m; ++j)
            DIT_TRY(scail_abs_diff_sums(v + (j + 1) * width, v + j * width, width, out + 2 * (s0 + j), stream));
        if (s0 + m < n_steps && hipMemcpyAsync(v, v + m * width, (size_t)width * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            scail_set_error(std::string(who) + ": hipMemcpyAsync failed");
            return 2;
        }
    }
    return 0;
}

// ---- the tiled sampler loop (RFSamplerLong, sampling.py:986-1085; scail_amd/sampler.py RFSamplerLong.sample_hip is the host form) ----
extern "C" int64_t scail_dit_sample_tiled_workspace_bytes(const scail_dit* h, int64_t T, int64_t Tt, int64_t H, int64_t W) {
    if (T >= (1 << 15) || scail_tile_len_check(nullptr, Tt, T) != 0) return -1;
    const int64_t step = scail_dit_chars_workspace_bytes(h, 2, Tt, H, W, 1);
    return step < 0 ? -1 : sample_ws(step, Tt, H, W, T).total;
}

// the tiled loop; cached = false: every evaluation a plain one (scail_dit_sample_tiled), else tile k's evaluation of step i in
// SCAIL_DIT_CACHE_REUSE mode where reuse[i] != 0 and in SCAIL_DIT_CACHE_FILL mode otherwise, on slab k of the cache
// (scail_dit_sample_tiled_cached).  solver != nullptr: scail_tile_finish_multistep under row i of the plan finishes the step instead of
// scail_tile_finish (scail_dit_sample_tiled_solver)
static int sample_tiled_impl(const char* who, scail_dit* h, float* x, const float* timesteps, const float* dsigma, int64_t n_steps, float cfg_scale,
                             const scail_dit_cond* cond, const scail_bf16* ref, const scail_bf16* pose_tiles,
                             const int32_t* tile_frames, const float* tile_w, const float* inv_wsum, int64_t n_tiles, int64_t T, int64_t Tt,
                             const float* rope_cos, const float* rope_sin, int64_t H, int64_t W, void* workspace, int64_t workspace_bytes,
                             void* stream, bool cached, const uint8_t* reuse, void* cache, int64_t cache_bytes,
                             const SolverPlan* solver = nullptr, void* hist = nullptr, int64_t hist_bytes = 0) {
    auto fail = [&](const std::string& msg) {
        scail_set_error(std::string(who) + ": " + msg);
        return 1;
    };
    // every refusal comes before the first enqueue, names the value, and the ones about the tiling need neither a handle nor a device
    if (n_tiles < 2)
        return fail("needs at least 2 tiles (a single tile leaves the weight sums of the reference at zero), got n_tiles = " + std::to_string(n_tiles));
    if (T >= (1 << 15)) return fail("the latent must have fewer than 32768 frames, got T = " + std::to_string(T));
    DIT_TRY(scail_tile_len_check(who, Tt, T));
    if (n_steps < 0) return fail("n_steps must be >= 0, got " + std::to_string(n_steps));
    if (tile_frames == nullptr) return fail("null pointer: tile_frames");
    if (tile_w == nullptr) return fail("null pointer: tile_w");
    if (inv_wsum == nullptr) return fail("null pointer: inv_wsum");
    std::vector<char> covered((size_t)T, 0);
    for (int64_t k = 0; k < n_tiles; ++k) {
        DIT_TRY(scail_tile_check((std::string(who) + ": tile " + std::to_string(k)).c_str(), tile_frames + k * Tt, Tt, T, true));
        for (int64_t j = 0; j < Tt; ++j) covered[(size_t)tile_frames[k * Tt + j]] = 1;
    }
    for (int64_t f = 0; f < T; ++f) {
        if (!covered[(size_t)f]) return fail("frame " + std::to_string(f) + " of [0, T = " + std::to_string(T) + ") is covered by no tile");
        if (!(inv_wsum[f] > 0.0f) || !std::isfinite(inv_wsum[f]))
            return fail("inv_wsum[" + std::to_string(f) + "] = " + std::to_string(inv_wsum[f]) + " must be finite and positive");
    }
    if (H <= 0 || W <= 0 || H % 4 != 0 || W % 4 != 0 || H >= (1 << 15) || W >= (1 << 15))
        return fail("latent H and W must be positive multiples of 4 below 32768, got H = " + std::to_string(H) + ", W = " + std::to_string(W));
    const int64_t own = sample_ws(0, Tt, H, W, T).total;      // the handle-independent part, so this answers without a handle too
    if (workspace_bytes < own)
        return fail("workspace too small: " + std::to_string(workspace_bytes) + " bytes cannot hold the tile pair buffers and den (" +
                    std::to_string(own) + " bytes) next to the step workspace (scail_dit_sample_tiled_workspace_bytes)");
    if (cached) {
        if (n_tiles >= (1 << 15)) return fail("a cached tiled loop takes fewer than 32768 tiles, got n_tiles = " + std::to_string(n_tiles));
        DIT_TRY(reuse_check(who, reuse, n_steps));
        DIT_TRY(cache_check(who, h, 0, false, cache, cache_bytes, 2, Tt, H, W, n_tiles));
    }
    if (solver != nullptr) DIT_TRY(solver_check(who, n_steps, solver->sigma, solver->coef, hist, hist_bytes, T, H, W));
    const void* ptrs[] = {h, x, timesteps, dsigma, cond, ref, pose_tiles, rope_cos, rope_sin, workspace};
    const char* names[] = {"handle", "x", "timesteps", "dsigma", "cond", "ref", "pose_tiles", "rope_cos", "rope_sin", "workspace"};
    for (int i = 0; i < 10; ++i)
        if (ptrs[i] == nullptr && !(i == 3 && n_steps == 0)) return fail(std::string("null pointer: ") + names[i]);
    const int64_t step_bytes = scail_dit_chars_workspace_bytes(h, 2, Tt, H, W, 1);
    if (step_bytes < 0) return fail("bad latent shape (Tt " + std::to_string(Tt) + ", H " + std::to_string(H) + ", W " + std::to_string(W) + ")");
    const SampleWs ws = sample_ws(step_bytes, Tt, H, W, T);
    if (workspace_bytes < ws.total)
        return fail("workspace too small: " + std::to_string(workspace_bytes) + " bytes, needs " + std::to_string(ws.total) +
                    " (scail_dit_sample_tiled_workspace_bytes)");
    SCAIL_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "workspace must be 256-byte aligned");
    DIT_TRY(probe_check(h, 2 * tok_lens(1, Tt, H, W).Ltok));

    char* base = static_cast<char*>(workspace);
    float *xin = reinterpret_cast<float*>(base + ws.xin), *v = reinterpret_cast<float*>(base + ws.v), *den = reinterpret_cast<float*>(base + ws.den);
    const int64_t F = 16 * H * W, pose_tile = Tt * 16 * (H / 2) * (W / 2);
    // the cache (include/scail_dit.h): tile k's residual in slab k of R bytes, then the one embedding region every FILL uses in turn
    const int64_t R = cache_ws(h->cfg, 2, tok_lens(1, Tt, H, W).Lnoise).emb;
    char* slabs = static_cast<char*>(cache);
    scail_bf16* cache_emb = cached ? reinterpret_cast<scail_bf16*>(slabs + n_tiles * R) : nullptr;
    // den starts at zero; scail_tile_finish leaves it zeroed for the next step
    if (n_steps > 0) DIT_TRY(scail_zero_f32(den, T * F, stream));
    for (int64_t i = 0; i < n_steps; ++i) {
        const int mode = !cached ? CACHE_NONE : reuse[i] ? SCAIL_DIT_CACHE_REUSE : SCAIL_DIT_CACHE_FILL;
        for (int64_t k = 0; k < n_tiles; ++k) {      // ascending, the order of the host loop: the accumulation order is part of the result
            const int32_t* fr = tile_frames + k * Tt;
            DIT_TRY(scail_tile_gather(x, xin, fr, Tt, T, F, stream));
            DIT_TRY(dit_step_impl(h, xin, timesteps + 2 * i, cond, ref, 1, pose_tiles + k * pose_tile, 1, 1, Tt, rope_cos, rope_sin, v, 2, Tt, H, W,
                                  nullptr, SCAIL_DIT_CFG_PAIR, workspace, step_bytes, stream, mode,
                                  cached ? reinterpret_cast<scail_bf16*>(slabs + k * R) : nullptr, cache_emb));
            DIT_TRY(scail_tile_blend_acc(den, v, fr, tile_w + k * Tt, Tt, T, F, cfg_scale, stream));
        }
        if (solver != nullptr) {
            // one update of the whole latent after the blend: one history serves every tile
            const float* co = solver->coef + 3 * i;
            DIT_TRY(scail_tile_finish_multistep(x, den, inv_wsum, static_cast<float*>(hist), T, F, solver->sigma[i], co[0], co[1], co[2],
                                                co[2] != 0.0f, stream));
            continue;
        }
        DIT_TRY(scail_tile_finish(x, den, inv_wsum, T, F, dsigma[i], stream));
    }
    return 0;
}
extern "C" int scail_dit_sample_tiled(scail_dit* h, float* x, const float* timesteps, const float* dsigma, int64_t n_steps, float cfg_scale,
                                      const scail_dit_cond* cond, const scail_bf16* ref, const scail_bf16* pose_tiles,
                                      const int32_t* tile_frames, const float* tile_w, const float* inv_wsum, int64_t n_tiles, int64_t T, int64_t Tt,
                                      const float* rope_cos, const float* rope_sin, int64_t H, int64_t W, void* workspace, int64_t workspace_bytes,
                                      void* stream) {
    return sample_tiled_impl("scail_dit_sample_tiled", h, x, timesteps, dsigma, n_steps, cfg_scale, cond, ref, pose_tiles, tile_frames, tile_w, inv_wsum,
                             n_tiles, T, Tt, rope_cos, rope_sin, H, W, workspace, workspace_bytes, stream, false, nullptr, nullptr, 0);
}
extern "C" int scail_dit_sample_tiled_cached(scail_dit* h, float* x, const float* timesteps, const float* dsigma, int64_t n_steps, float cfg_scale,
                                             const scail_dit_cond* cond, const scail_bf16* ref, const scail_bf16* pose_tiles,
                                             const int32_t* tile_frames, const float* tile_w, const float* inv_wsum, int64_t n_tiles, int64_t T,
                                             int64_t Tt, const float* rope_cos, const float* rope_sin, int64_t H, int64_t W, void* workspace,
                                             int64_t workspace_bytes, const uint8_t* reuse, void* cache, int64_t cache_bytes, void* stream) {
    return sample_tiled_impl("scail_dit_sample_tiled_cached", h, x, timesteps, dsigma, n_steps, cfg_scale, cond, ref, pose_tiles, tile_frames, tile_w,
                             inv_wsum, n_tiles, T, Tt, rope_cos, rope_sin, H, W, workspace, workspace_bytes, stream, true, reuse, cache, cache_bytes);
}
extern "C" int scail_dit_sample_tiled_solver(scail_dit* h, float* x, const float* timesteps, const float* dsigma, int64_t n_steps, float cfg_scale,
                                             const scail_dit_cond* cond, const scail_bf16* ref, const scail_bf16* pose_tiles,
                                             const int32_t* tile_frames, const float* tile_w, const float* inv_wsum, int64_t n_tiles, int64_t T,
                                             int64_t Tt, const float* rope_cos, const float* rope_sin, int64_t H, int64_t W, void* workspace,
                                             int64_t workspace_bytes, const float* sigma, const float* coef, void* hist, int64_t hist_bytes,
                                             void* stream) {
    const SolverPlan plan{sigma, coef};
    return sample_tiled_impl("scail_dit_sample_tiled_solver", h, x, timesteps, dsigma, n_steps, cfg_scale, cond, ref, pose_tiles, tile_frames, tile_w,
                             inv_wsum, n_tiles, T, Tt, rope_cos, rope_sin, H, W, workspace, workspace_bytes, stream, false, nullptr, nullptr, 0, &plan,
                             hist, hist_bytes);
}
