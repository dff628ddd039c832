"""Wiring tests of the DiT step: the shared helper (no GPU code; tests/test_dit_wiring_cpu.py, tests/test_dit_wiring_gpu.py).

The kernel-level exact tests decide whether a kernel computes its operation.  What they cannot see is the COMPOSITION: which slice,
table, bias, gamma or offset reaches which kernel in scail_amd/dit.py and csrc/dit_step.hip.  Under oracle.make_state_dict (biases
N(0, 0.02), gammas 1 +- 0.1) and the 96-token dit_tiny inputs every such term is small against the activations, so a dropped wire
passes rtol = atol = 2e-2 and cosine >= 0.999.  This module holds

  * a PLANTED network and inputs (planted_config / planted_state_dict / planted_inputs): TINY's width (D 256, 2 heads of 128, FF 512,
    2 layers) on a T 3, 16 x 24 latent = 8 x 12 patches (H != W), 96 + 288 + 72 = 456 tokens (seven 64-key tiles + 8 keys, across the
    256-row query tile), 20 distinct non-zero text tokens, 9 CLIP tokens, batch 2 = ONE latent and sigma twice (so the CFG-pair form of
    the executor applies) under two different prompts.  Every bias, gamma and table is of the order of the activations it meets; the
    patch embedding is small (rms 0.3) so that every branch of a block is a good part of the hidden state; q and k are mostly their
    biases, so a self-attention score is mostly a function of the two positions through RoPE; the q and k gammas differ 2-3 x inside
    every RoPE pair, opposite ways in q and k (without that, swapping them would only commute); all values bf16-exact.  Seeded; nothing
    comes from a reference tree.

  * a MUTATION CATALOGUE (CATALOGUE): named functions that edit the state dict / config or monkeypatch ONE function of
    oracle.scail_oracle for the duration of a call (``applied``), each one realistic wiring mistake.

  * a BF16-STORAGE MODEL of the oracle (storage_points / storage_sample): the same forward pass in fp32 with one round-to-nearest-even
    to bf16 at exactly the points where the executor stores bf16 (below).  Its distance from the fp32 oracle is the noise N_p a correct
    GPU path is expected to have at observation point p; the GPU tests hold the real path to T_p = 2 N_p (``bounds``), and the CPU
    tests prove that every catalogue entry moves some observation point by >= 4 T_p.

  * the METRIC e(a, b) = ||a - b||_2 / ||b||_2 and the OBSERVATION POINTS: "emb" (patch-embedding output), "h1" .. "hN" (hidden state
    after each block), "out" (the velocity), and the block-local "blk0" .. "blkN-1": the oracle's bf16-rounded input of block i pushed
    through block i alone, compared with the oracle's block output on that same input -- the error does not accumulate and a layer-1
    wire is seen at layer 1.

Store points of the model (csrc/dit_step.hip enqueues the kernels of DiffusionTransformer._run in the same order; every
GEMM / attention accumulates in fp32, per-channel vectors, the time path and the modulation rows are fp32 throughout):
   conditioning (once per prompt): text_embedding.0 + GELU; text_embedding.2; clip LayerNorm; clip_proj.1 + GELU; clip_proj.3; clip
     LayerNorm; per layer the text / CLIP key_value GEMM outputs (V is used as stored), and the RMS-normed keys
   tokens: the patchify image of x (fp32 in the sampler), ref, pose; the patch-embedding GEMM output (bias in the epilogue)
   block:  ln_modulate output; QKV GEMM output; k after RMSNorm + RoPE; q after RMSNorm + RoPE x (log2 e / sqrt 128) (queries travel
           in log2 units, ops.ATTN_LOG2_SCALE); the probabilities exp2(s - max) as the P.V operand (the row sum is fp32); the attention
           output; hidden after dense + bias, gate, residual; layernorm_affine output; cross-query GEMM output; cross query after
           RMSNorm x scale; the text attention output (held as bf16 while the CLIP keys are attended); the sum of the
           two; hidden after dense + residual; ln_modulate output; dense_h_to_4h + GELU output; hidden after dense_4h_to_h, gate, residual
   final:  ln_modulate of the noise rows; the 64-column GEMM output (unpatchify widens it to fp32 unchanged)
   sampler: nothing more -- the latent and the CFG / Euler update are fp32.
"""
from __future__ import annotations

import contextlib
import dataclasses
import math
from typing import Callable, Dict, List, Optional

import torch
import torch.nn.functional as F

from oracle import scail_oracle as O

T, H, W = 3, 16, 24                       # latent frames, height, width: 8 x 12 patches
LT, LC = 20, 9                            # text / CLIP tokens
TIMESTEP = 731.0
CFGD = dict(O.TINY, latent_width=64)      # rope table extent wide enough for a second character's pose window (120 + 2 x 12 <= 32 + 120)
LOG2_SCALE = 1.4426950408889634 / math.sqrt(128.0)
GOLDEN_TOKEN_STRIDE = 3                   # tests/golden/dit_planted.npz holds the hidden states of every third token
SEED, SEED2 = 2024, 4051                  # the planted draw, and the second draw of the inputs for check (a)


def bf16r(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(torch.float32)


def e(a: torch.Tensor, b: torch.Tensor) -> float:
    """the metric: ||a - b||_2 / ||b||_2 in fp64"""
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def planted_config() -> O.DiTConfig:
    return O.DiTConfig(**CFGD)


def _lay(i):
    return f"transformer.layers.{i}."


_M = "mixins.adaln_layer."
GAMMAS = ("query", "key", "cross_query", "cross_key", "clip_feature_key")


# Scales of the planted weights: name suffix -> gain of a matrix (std = gain / sqrt(fan_in)) or std of a vector.  First match wins.
MATRIX_GAIN = (
    ("patch_embed.proj.weight", 0.3), ("patch_embed.proj_pose.weight", 0.3),        # a small trunk: every branch is a good part of h
    ("attention.dense.weight", 1.0), ("mlp.dense_h_to_4h.weight", 1.0), ("mlp.dense_4h_to_h.weight", 0.5), ("cross_attention.dense.weight", 0.5),
    ("cross_attention.key_value.weight", 1.0), ("clip_feature_key_value_list.0.weight", 1.0), ("clip_feature_key_value_list.1.weight", 1.0),
    ("text_embedding.0.weight", 1.0), ("text_embedding.2.weight", 1.0), ("clip_proj.proj.1.weight", 1.0), ("clip_proj.proj.3.weight", 1.0),
    ("final_layer.linear.weight", 1.0), ("", 0.5))
BIAS_STD = (
    ("patch_embed.proj.bias", 0.075), ("patch_embed.proj_pose.bias", 0.075),
    ("post_cross_attention_layernorm.bias", 0.5), ("mlp.dense_h_to_4h.bias", 0.5),
    ("attention.dense.bias", 0.2), ("mlp.dense_4h_to_h.bias", 0.2), ("", 0.25))
QK_BIAS = 1.0             # std of the q and k thirds of the QKV bias (the v third: BIAS_STD)
CROSS_K_BIAS = 1.0        # std of the k halves of the text / CLIP key_value biases (the v halves: BIAS_STD)
V_GAIN = 2.0              # gain of the v third of the QKV weight (the q and k thirds: 0.5)
CROSS_V_GAIN = 0.5        # factor on the v halves of the text / CLIP key_value weights; the CLIP k half is halved too (CLIP_K_GAIN)
CLIP_K_GAIN = 0.5


def _scale(table, name):
    return next(v for k, v in table if name.endswith(k))


def planted_state_dict(cfg: O.DiTConfig, seed: int = SEED) -> Dict[str, torch.Tensor]:
    """Weights on O.state_dict_spec(cfg), bf16-exact, every vector at the scale of what it meets (the tables and constants above): the
    three cross-attention gammas uniform in [1, 3], the query / key gammas in [1, 1.5] and [2, 3] alternating inside every RoPE pair, the
    LayerNorm weights uniform in [0.5, 2], adaLN tables N(0, 0.5), q and k biases N(0, 1) against a projection of std 0.5 (q . k is then
    mostly a function of the two positions, through RoPE), key biases of the cross attention N(0, 1) (an RMS-normed key only shows its
    bias when the bias is a good part of it).  The scales were chosen on the CPU so that condition (b) of tests/test_dit_wiring_cpu.py
    holds; they are data of the tests and are FROZEN: the bounds of the GPU tests follow from them."""
    g = torch.Generator().manual_seed(seed)
    D = cfg.hidden_size
    sd = {}
    for name, shape in O.state_dict_spec(cfg).items():
        if "adaLN_modulation" in name:
            w = 0.5 * torch.randn(shape, generator=g)
        elif ".query_layernorm_list." in name or ".key_layernorm_list." in name:
            # within a RoPE pair (2j, 2j + 1) the two gammas differ by 2 .. 3 x, the other way round in q and in k: without RoPE between
            # them gamma_q and gamma_k only meet as a product, and swapping them would be invisible
            w = 1.0 + 0.5 * torch.rand(shape, generator=g)
            big = 2.0 + torch.rand(D // 2, generator=g)
            w[(0 if ".query_" in name else 1)::2] = big
        elif any(f".{nm}_layernorm_list." in name for nm in GAMMAS):
            w = 1.0 + 2.0 * torch.rand(shape, generator=g)
        elif name.endswith("layernorm.weight") or name in ("clip_proj.proj.0.weight", "clip_proj.proj.4.weight"):
            w = 0.5 + 1.5 * torch.rand(shape, generator=g)
        elif name.endswith("bias"):
            w = _scale(BIAS_STD, name) * torch.randn(shape, generator=g)
            if name.endswith("attention.query_key_value.bias"):
                w[:2 * D] *= QK_BIAS / 0.25
            elif "key_value" in name:
                w[:D] *= CROSS_K_BIAS / 0.25
        else:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            w = torch.randn(shape, generator=g) * (_scale(MATRIX_GAIN, name) / math.sqrt(fan_in))
            if name.endswith("attention.query_key_value.weight"):
                w[2 * D:] *= V_GAIN / 0.5
            elif "key_value" in name:
                w[D:] *= CROSS_V_GAIN
                if "clip" in name:
                    w[:D] *= CLIP_K_GAIN
        sd[name] = bf16r(w)
    return sd


def planted_inputs(seed: int = SEED, n_char: int = 1) -> Dict[str, torch.Tensor]:
    """x (2, T, 16, H, W): one latent twice; ctx (2, LT, text_dim): two prompts, every row distinct, none zero, row norms spread over
    0.5 .. 2 (an RMS-normed key then differs from its neighbour in more than direction); ref (1, n_char, ..), pose (1, n_char * T, ..),
    clip (1, LC, 1280); t: one sigma twice.  bf16-exact."""
    g = torch.Generator().manual_seed(seed)
    x = bf16r(torch.randn(1, T, 16, H, W, generator=g)).repeat(2, 1, 1, 1, 1)
    ctx = torch.randn(2, LT, CFGD["text_dim"], generator=g) * (0.5 + 1.5 * torch.rand(2, LT, 1, generator=g))
    ref = torch.randn(1, 1, 16, H, W, generator=g)
    pose = torch.randn(1, T, 16, H // 2, W // 2, generator=g)
    clip = torch.randn(1, LC, 1280, generator=g) * (0.5 + 1.5 * torch.rand(1, LC, 1, generator=g))
    if n_char > 1:                        # further characters are drawn after everything else: character 0 is the one-character draw
        ref = torch.cat([ref] + [torch.randn(1, 1, 16, H, W, generator=g) for _ in range(n_char - 1)], 1)
        pose = torch.cat([pose] + [torch.randn(1, T, 16, H // 2, W // 2, generator=g) for _ in range(n_char - 1)], 1)
    return dict(x=x, ctx=bf16r(ctx), ref=bf16r(ref), pose=bf16r(pose), clip=bf16r(clip), t=torch.tensor([TIMESTEP, TIMESTEP]))


def _prep(cfg, inp):
    x = inp["x"].float()
    B, T_, _, H_, W_ = x.shape

    def rep(z):
        return z.float().repeat(B // z.shape[0], *([1] * (z.dim() - 1))) if z.shape[0] != B else z.float()

    ref, pose = rep(inp["ref"]), rep(inp["pose"])
    n_char = ref.shape[1]
    assert pose.shape[1] == n_char * T_
    x20 = torch.cat([x, torch.zeros(B, T_, 4, H_, W_)], dim=2)
    ref20 = torch.cat([ref, torch.ones(B, n_char, 4, H_, W_)], dim=2)
    pose20 = torch.cat([pose, torch.ones(B, n_char * T_, 4, H_ // 2, W_ // 2)], dim=2)
    rT, rH, rW = T_, H_ // 2, W_ // 2
    return x20, ref20, pose20, rep, n_char, (rT, rH, rW), n_char * rH * rW, rT * rH * rW


def oracle_points(cfg, sd, inp, block_inputs: Optional[List[torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """O.dit_forward restated through the attributes of the oracle module (so that a monkeypatched function takes effect) with every
    observation point returned; ``block_inputs[i]``: the input of the block-local point of layer i.  Unmutated, "h*" and "out" equal
    O.dit_forward(return_hidden=True) bit for bit (asserted in tests/test_dit_wiring_cpu.py)."""
    x20, ref20, pose20, rep, n_char, (rT, rH, rW), ref_len, seq_len = _prep(cfg, inp)
    text = O.text_embedding(cfg, sd, inp["ctx"].float())
    clip = rep(O.clip_proj(cfg, sd, inp["clip"].float()))
    emb, adaln = O.time_embeddings(cfg, sd, inp["t"])
    cos, sin = (O.rope_tables(cfg, rT, rH, rW) if n_char == 1 else O.rope_tables_multi(cfg, rT, rH, rW, n_char))
    h = O.patch_embed(cfg, sd, x20, ref20, pose20)
    pts = {"emb": h}
    for i in range(cfg.num_layers):
        h = O.block(cfg, sd, i, h, adaln, text, clip, cos, sin)
        pts[f"h{i + 1}"] = h
    pts["out"] = O.final_layer(cfg, sd, h, emb, ref_len, seq_len, rT, rH, rW)
    if block_inputs is not None:
        for i in range(cfg.num_layers):
            pts[f"blk{i}"] = O.block(cfg, sd, i, block_inputs[i], adaln, text, clip, cos, sin)
    return pts


def block_inputs_of(cfg, pts) -> List[torch.Tensor]:
    """the oracle's bf16-rounded block inputs: what the block-local points are fed"""
    return [bf16r(pts["emb"])] + [bf16r(pts[f"h{i}"]) for i in range(1, cfg.num_layers)]


def points_of(cfg) -> List[str]:
    n = cfg.num_layers
    return ["emb"] + [f"h{i + 1}" for i in range(n)] + ["out"] + [f"blk{i}" for i in range(n)]


# ------------------------------------------------------------------------------------------------------------------------------------
# the bf16-storage model
# ------------------------------------------------------------------------------------------------------------------------------------
def _attend(q, k, v, r):
    """q in log2 units (B, n, Lq, hd); unnormalised probabilities rounded as the P.V operand, fp32 row sum, one division"""
    s = torch.matmul(q, k.transpose(-1, -2))
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    return torch.matmul(r(p), v) / p.sum(-1, keepdim=True)


def _model_cond(cfg, sd, inp, rep, r):
    eps, D, n = cfg.layernorm_epsilon, cfg.hidden_size, cfg.num_attention_heads
    lin = lambda x, k: F.linear(x, sd[k + ".weight"], sd[k + ".bias"])
    text = r(O.gelu_tanh(lin(inp["ctx"].float(), "text_embedding.0")))
    text = r(lin(text, "text_embedding.2"))
    c = inp["clip"].float()
    c = r(F.layer_norm(c, (c.shape[-1],), sd["clip_proj.proj.0.weight"], sd["clip_proj.proj.0.bias"], 1e-5))
    c = r(F.gelu(lin(c, "clip_proj.proj.1")))
    c = r(lin(c, "clip_proj.proj.3"))
    c = rep(r(F.layer_norm(c, (c.shape[-1],), sd["clip_proj.proj.4.weight"], sd["clip_proj.proj.4.bias"], 1e-5)))
    layers = []
    for i in range(cfg.num_layers):
        kv = r(lin(text, _lay(i) + "cross_attention.key_value"))
        kvc = r(lin(c, _M + f"clip_feature_key_value_list.{i}"))
        k = r(O.rms_norm(kv[..., :D], sd[_M + f"cross_key_layernorm_list.{i}.weight"], eps))
        kc = r(O.rms_norm(kvc[..., :D], sd[_M + f"clip_feature_key_layernorm_list.{i}.weight"], eps))
        layers.append(tuple(O._heads(z, n) for z in (k, kv[..., D:], kc, kvc[..., D:])))
    return layers


def _model_block(cfg, sd, i, h, adaln, cond, cos, sin, r):
    eps, D, n = cfg.layernorm_epsilon, cfg.hidden_size, cfg.num_attention_heads
    B = h.shape[0]
    lin = lambda x, k: F.linear(x, sd[k + ".weight"], sd[k + ".bias"])
    mod = adaln.view(B, 6, D) + sd[_M + f"adaLN_modulations.{i}"]
    sh_a, sc_a, g_a, sh_m, sc_m, g_m = mod.chunk(6, dim=1)
    # self attention
    xn = r(O.modulate(O.layer_norm(h, eps), sh_a, sc_a))
    q, k, v = r(lin(xn, _lay(i) + "attention.query_key_value")).chunk(3, dim=-1)
    q = O.rms_norm(q, sd[_M + f"query_layernorm_list.{i}.weight"], eps)
    k = O.rms_norm(k, sd[_M + f"key_layernorm_list.{i}.weight"], eps)
    q, k, v = O._heads(q, n), O._heads(k, n), O._heads(v, n)
    q, k = r(O.apply_rope(q, cos, sin) * LOG2_SCALE), r(O.apply_rope(k, cos, sin))
    att = r(O._merge(_attend(q, k, v, r)))
    h = r(h + g_a * lin(att, _lay(i) + "attention.dense"))
    # cross attention
    Lp = _lay(i) + "post_cross_attention_layernorm."
    xn = r(O.layer_norm(h, eps, sd[Lp + "weight"], sd[Lp + "bias"]))
    cq = r(lin(xn, _lay(i) + "cross_attention.query"))
    cq = O._heads(r(O.rms_norm(cq, sd[_M + f"cross_query_layernorm_list.{i}.weight"], eps) * LOG2_SCALE), n)
    kt, vt, kc, vc = cond[i]
    att = r(O._merge(r(_attend(cq, kt, vt, r)) + _attend(cq, kc, vc, r)))
    h = r(h + lin(att, _lay(i) + "cross_attention.dense"))
    # MLP
    xn = r(O.modulate(O.layer_norm(h, eps), sh_m, sc_m))
    ff = r(O.gelu_tanh(lin(xn, _lay(i) + "mlp.dense_h_to_4h")))
    return r(h + g_m * lin(ff, _lay(i) + "mlp.dense_4h_to_h"))


def storage_points(cfg, sd, inp, block_inputs: Optional[List[torch.Tensor]] = None, r: Callable = bf16r) -> Dict[str, torch.Tensor]:
    """The bf16-storage model (module docstring): the observation points of ``oracle_points`` with ``r`` applied at every store point.
    With r = identity it is the oracle up to fp32 re-association (asserted in the CPU tests)."""
    x20, ref20, pose20, rep, n_char, (rT, rH, rW), ref_len, seq_len = _prep(cfg, inp)
    cond = _model_cond(cfg, sd, inp, rep, r)
    emb, adaln = O.time_embeddings(cfg, sd, inp["t"])
    cos, sin = (O.rope_tables(cfg, rT, rH, rW) if n_char == 1 else O.rope_tables_multi(cfg, rT, rH, rW, n_char))
    h = r(O.patch_embed(cfg, sd, r(x20), r(ref20), r(pose20)))
    pts = {"emb": h}
    for i in range(cfg.num_layers):
        h = _model_block(cfg, sd, i, h, adaln, cond, cos, sin, r)
        pts[f"h{i + 1}"] = h
    shift, scale = (emb.unsqueeze(1) + sd["mixins.final_layer.adaLN_modulation"]).chunk(2, dim=1)
    xf = r(O.modulate(O.layer_norm(h[:, ref_len:ref_len + seq_len], cfg.layernorm_epsilon), shift, scale))
    tok = r(F.linear(xf, sd["mixins.final_layer.linear.weight"], sd["mixins.final_layer.linear.bias"]))
    B = tok.shape[0]
    o, p, q = cfg.patch_size
    c = cfg.out_channels
    pts["out"] = tok.reshape(B, rT, rH, rW, o, p, q, c).permute(0, 1, 4, 7, 2, 5, 3, 6).reshape(B, rT * o, c, rH * p, rW * q)
    if block_inputs is not None:
        for i in range(cfg.num_layers):
            pts[f"blk{i}"] = _model_block(cfg, sd, i, block_inputs[i], adaln, cond, cos, sin, r)
    return pts


SAMPLE_STEPS, CFG_SCALE, SHIFT_SCALE = 2, 4.0, 5.0


def sample_args(inp):
    """(x0, cond ctx, uncond ctx) of the two-step sampler run on the planted inputs: batch row 0 is the unconditional prompt"""
    return inp["x"][:1], inp["ctx"][1:2], inp["ctx"][0:1]


def storage_sample(cfg, sd, inp, r: Callable = bf16r) -> torch.Tensor:
    """O.sample (SAMPLE_STEPS Euler steps, CFG) with the storage model as the network; the latent and its update stay fp32"""
    x0, c_ctx, uc_ctx = sample_args(inp)

    def network(xin, t, ctx):
        return storage_points(cfg, sd, dict(inp, x=xin, t=t, ctx=ctx), r=r)["out"]

    return O.sample(cfg, sd, x0, c_ctx, uc_ctx, inp["ref"], inp["pose"], inp["clip"], num_steps=SAMPLE_STEPS, cfg_scale=CFG_SCALE,
                    shift_scale=SHIFT_SCALE, network=network)[0]


def oracle_sample(cfg, sd, inp) -> torch.Tensor:
    x0, c_ctx, uc_ctx = sample_args(inp)
    return O.sample(cfg, sd, x0, c_ctx, uc_ctx, inp["ref"], inp["pose"], inp["clip"], num_steps=SAMPLE_STEPS, cfg_scale=CFG_SCALE,
                    shift_scale=SHIFT_SCALE)[0]


def noise(cfg, sd, inp, sampler: bool = False) -> Dict[str, float]:
    """N_p of one draw of the inputs: the storage model against the oracle at every observation point (+ "sample": the final latent of
    the two-step sampler)"""
    ref = oracle_points(cfg, sd, inp)
    bi = block_inputs_of(cfg, ref)
    ref = oracle_points(cfg, sd, inp, bi)
    got = storage_points(cfg, sd, inp, bi)
    n = {p: e(got[p], ref[p]) for p in points_of(cfg)}
    if sampler:
        n["sample"] = e(storage_sample(cfg, sd, inp), oracle_sample(cfg, sd, inp))
    return n


_BOUNDS: Dict = {}


def bounds(n_char: int = 1, sampler: bool = False) -> Dict[str, Dict[str, float]]:
    """{"N": N_p, "T": T_p = 2 N_p} on the planted network.  N_p is the larger of the storage model's distance on the planted inputs and on
    a second draw of the inputs (SEED2), so T_p does not rest on one draw.  CPU only; the GPU tests take their bounds from here."""
    key = (n_char, sampler)
    if key not in _BOUNDS:
        cfg = planted_config()
        sd = planted_state_dict(cfg)
        a = noise(cfg, sd, planted_inputs(SEED, n_char), sampler)
        b = noise(cfg, sd, planted_inputs(SEED2, n_char), sampler)
        N = {p: max(a[p], b[p]) for p in a}
        _BOUNDS[key] = dict(N=N, T={p: 2.0 * v for p, v in N.items()}, draws=(a, b))
    return _BOUNDS[key]


# ------------------------------------------------------------------------------------------------------------------------------------
# the mutation catalogue
# ------------------------------------------------------------------------------------------------------------------------------------
class Mut:
    """What a catalogue entry may change: ``sd`` (a private copy), ``cfg`` (replace it), ``patch(name, fn)`` of oracle.scail_oracle"""

    def __init__(self, cfg, sd):
        self.cfg, self.sd, self.patches = cfg, dict(sd), {}

    def patch(self, name, fn):
        assert hasattr(O, name) and name not in self.patches
        self.patches[name] = fn

    def zero(self, key, sl=slice(None)):
        w = self.sd[key].clone()
        w[sl] = 0
        self.sd[key] = w


@contextlib.contextmanager
def applied(entry, cfg, sd):
    """``with applied(entry, cfg, sd) as (cfg_m, sd_m):`` -- the mutated config / weights, oracle.scail_oracle patched inside the block"""
    m = Mut(cfg, sd)
    entry.fn(m)
    saved = {k: getattr(O, k) for k in m.patches}
    try:
        for k, f in m.patches.items():
            setattr(O, k, f)
        yield m.cfg, m.sd
    finally:
        for k, f in saved.items():
            setattr(O, k, f)


@dataclasses.dataclass
class Entry:
    name: str
    fn: Callable


CATALOGUE: List[Entry] = []
NLAYERS = CFGD["num_layers"]


def _add(name, fn):
    assert all(c.name != name for c in CATALOGUE), name
    CATALOGUE.append(Entry(name, fn))


def by_name(name: str) -> Entry:
    return next(c for c in CATALOGUE if c.name == name)


# ---- adaLN: rows of the 6 x D modulation.  mod = Linear(SiLU(emb)).view(6, D) + table: permuting the rows of the projection AND of every
# layer's table is exactly a block that reads the rows in another order
def _perm_rows(m, perm):
    D = m.cfg.hidden_size
    w, b = m.sd["adaln_projection.1.weight"], m.sd["adaln_projection.1.bias"]
    m.sd["adaln_projection.1.weight"] = w.view(6, D, -1)[perm].reshape(w.shape).contiguous()
    m.sd["adaln_projection.1.bias"] = b.view(6, D)[perm].reshape(b.shape).contiguous()
    for i in range(m.cfg.num_layers):
        k = _M + f"adaLN_modulations.{i}"
        m.sd[k] = m.sd[k][:, perm].contiguous()


_add("adaln: attention shift <-> scale", lambda m: _perm_rows(m, [1, 0, 2, 3, 4, 5]))
_add("adaln: attention gate <-> MLP gate", lambda m: _perm_rows(m, [0, 1, 5, 3, 4, 2]))
_add("adaln: attention (shift, scale) <-> MLP (shift, scale)", lambda m: _perm_rows(m, [3, 4, 2, 0, 1, 5]))


def _table_from_other(m):
    m.sd[_M + "adaLN_modulations.1"] = m.sd[_M + "adaLN_modulations.0"]


_add("adaln: layer 1 reads layer 0's table", _table_from_other)
for _i in range(NLAYERS):
    _add(f"adaln: layer {_i} table dropped", lambda m, i=_i: m.zero(_M + f"adaLN_modulations.{i}"))
_add("adaln: x * (1 + scale) + shift written as x * scale + shift", lambda m: m.patch("modulate", lambda x, shift, scale: x * scale + shift))


def _gate_one(m):
    def block(cfg, sd, i, h, adaln_emb, text, clip, cos, sin, kv_gather=None):
        eps = cfg.layernorm_epsilon
        B, D = h.shape[0], cfg.hidden_size
        mod = adaln_emb.view(B, 6, D) + sd[f"mixins.adaln_layer.adaLN_modulations.{i}"]
        sh_a, sc_a, g_a, sh_m, sc_m, g_m = mod.chunk(6, dim=1)
        h = h + O.self_attention(cfg, sd, i, O.modulate(O.layer_norm(h, eps), sh_a, sc_a), cos, sin, kv_gather)      # gate taken as 1
        Lp = f"transformer.layers.{i}.post_cross_attention_layernorm."
        h = h + O.cross_attention(cfg, sd, i, O.layer_norm(h, eps, sd[Lp + "weight"], sd[Lp + "bias"]), text, clip)
        return h + g_m * O.mlp(cfg, sd, i, O.modulate(O.layer_norm(h, eps), sh_m, sc_m))
    m.patch("block", block)


_add("adaln: attention gate taken as 1", _gate_one)


def _final_swap(m):
    k = "mixins.final_layer.adaLN_modulation"
    m.sd[k] = m.sd[k][:, [1, 0]].contiguous()


_add("adaln: final-layer shift <-> scale", _final_swap)
_add("adaln: final table dropped", lambda m: m.zero("mixins.final_layer.adaLN_modulation"))

# ---- biases, each dropped on its own (per layer where there is one per layer)
_D = CFGD["hidden_size"]
for _i in range(NLAYERS):
    for _nm, _key, _sl in (
            ("query_key_value (q third)", _lay(_i) + "attention.query_key_value.bias", slice(0, _D)),
            ("query_key_value (k third)", _lay(_i) + "attention.query_key_value.bias", slice(_D, 2 * _D)),
            ("query_key_value (v third)", _lay(_i) + "attention.query_key_value.bias", slice(2 * _D, 3 * _D)),
            ("attention dense", _lay(_i) + "attention.dense.bias", slice(None)),
            ("cross query", _lay(_i) + "cross_attention.query.bias", slice(None)),
            ("text key_value (k half)", _lay(_i) + "cross_attention.key_value.bias", slice(0, _D)),
            ("text key_value (v half)", _lay(_i) + "cross_attention.key_value.bias", slice(_D, 2 * _D)),
            ("clip_feature_key_value (k half)", _M + f"clip_feature_key_value_list.{_i}.bias", slice(0, _D)),
            ("clip_feature_key_value (v half)", _M + f"clip_feature_key_value_list.{_i}.bias", slice(_D, 2 * _D)),
            ("cross dense", _lay(_i) + "cross_attention.dense.bias", slice(None)),
            ("mlp dense_h_to_4h", _lay(_i) + "mlp.dense_h_to_4h.bias", slice(None)),
            ("mlp dense_4h_to_h", _lay(_i) + "mlp.dense_4h_to_h.bias", slice(None)),
            ("post_cross_attention_layernorm", _lay(_i) + "post_cross_attention_layernorm.bias", slice(None))):
        _add(f"bias dropped: {_nm}, layer {_i}", lambda m, k=_key, s=_sl: m.zero(k, s))
    _add(f"post_cross_attention_layernorm weight replaced by 1, layer {_i}",
         lambda m, i=_i: m.sd.__setitem__(_lay(i) + "post_cross_attention_layernorm.weight",
                                          torch.ones_like(m.sd[_lay(i) + "post_cross_attention_layernorm.weight"])))
for _key in ("mixins.patch_embed.proj", "mixins.patch_embed.proj_pose", "text_embedding.0", "text_embedding.2", "clip_proj.proj.1",
             "clip_proj.proj.3", "clip_proj.proj.4", "time_embed.0", "time_embed.2", "adaln_projection.1", "mixins.final_layer.linear"):
    _add(f"bias dropped: {_key}", lambda m, k=_key: m.zero(k + ".bias"))


# ---- RMSNorm gammas
def _gamma(nm, i):
    return _M + f"{nm}_layernorm_list.{i}.weight"


def _swap(m, a, b):
    m.sd[a], m.sd[b] = m.sd[b], m.sd[a]


def _ones(m, k):
    m.sd[k] = torch.ones_like(m.sd[k])


for _i in range(NLAYERS):
    _add(f"gamma: query <-> key, layer {_i}", lambda m, i=_i: _swap(m, _gamma("query", i), _gamma("key", i)))
    _add(f"gamma: cross_key <-> clip_feature_key, layer {_i}", lambda m, i=_i: _swap(m, _gamma("cross_key", i), _gamma("clip_feature_key", i)))
    _add(f"gamma: cross_query taken from the other layer, layer {_i}",
         lambda m, i=_i: m.sd.__setitem__(_gamma("cross_query", i), m.sd[_gamma("cross_query", (i + 1) % NLAYERS)]))
    for _nm in GAMMAS:
        _add(f"gamma: {_nm} replaced by 1, layer {_i}", lambda m, nm=_nm, i=_i: _ones(m, _gamma(nm, i)))


# ---- RoPE
def _cfg(m, **kw):
    m.cfg = dataclasses.replace(m.cfg, **kw)


_add("rope: global_rope_W -> 0", lambda m: _cfg(m, global_rope_W=0))
_add("rope: global_rope_H -> 8", lambda m: _cfg(m, global_rope_H=8))
_add("rope: theta -> 9000", lambda m: _cfg(m, theta=9000.0))


def _hw_swapped(m):
    def rope_angles(cfg, t_pos, h_pos, w_pos):
        dt, dh, dw = O.rope_dims(cfg.head_dim)
        ft = torch.einsum("p,f->pf", t_pos.float(), O._axis_freqs(dt, cfg.theta)).repeat_interleave(2, dim=-1)
        fh = torch.einsum("p,f->pf", h_pos.float(), O._axis_freqs(dw, cfg.theta)).repeat_interleave(2, dim=-1)
        fw = torch.einsum("p,f->pf", w_pos.float(), O._axis_freqs(dh, cfg.theta)).repeat_interleave(2, dim=-1)
        T_, H_, W_ = ft.shape[0], fh.shape[0], fw.shape[0]
        return torch.cat([ft[:, None, None, :].expand(T_, H_, W_, -1), fw[None, None, :, :].expand(T_, H_, W_, -1),     # the w angles in
                          fh[None, :, None, :].expand(T_, H_, W_, -1)], dim=-1)                                         # the h columns
    m.patch("rope_angles", rope_angles)


_add("rope: H and W position axes swapped", _hw_swapped)


def _dims_rotated(m):
    orig = O.rope_dims
    m.patch("rope_dims", lambda head_dim: (lambda t, h, w: (h, w, t))(*orig(head_dim)))


_add("rope: (t, h, w) split of rope_dims rotated", _dims_rotated)


def _ref_at_t1(m):
    orig = O.rope_tables

    def rope_tables(cfg, rope_T, rope_H, rope_W, H_shift=0, W_shift=0):
        cos, sin = orig(cfg, rope_T, rope_H, rope_W, H_shift, W_shift)
        n = rope_H * rope_W
        cos, sin = cos.clone(), sin.clone()
        cos[:n], sin[:n] = cos[n:2 * n], sin[n:2 * n]          # the first noise frame's rows: t = 1, same h / w window
        return cos, sin
    m.patch("rope_tables", rope_tables)


_add("rope: reference frame at the first noise frame's T position", _ref_at_t1)


def _rope_q_only(m):
    orig, calls = O.apply_rope, [0]

    def apply_rope(t, cos, sin):                              # O.self_attention rotates q, then k
        calls[0] += 1
        return orig(t, cos, sin) if calls[0] % 2 == 1 else t
    m.patch("apply_rope", apply_rope)


_add("rope: applied to q only", _rope_q_only)


# ---- tokens and channels
def _pose_first(m):
    orig = O.patch_embed

    def patch_embed(cfg, sd, x20, ref20, pose20):
        h = orig(cfg, sd, x20, ref20, pose20)
        p, q = cfg.patch_size[1], cfg.patch_size[2]
        per = (ref20.shape[3] // p) * (ref20.shape[4] // q)
        lr, ln = ref20.shape[1] * per, x20.shape[1] * per
        return torch.cat([h[:, :lr], h[:, lr + ln:], h[:, lr:lr + ln]], dim=1)
    m.patch("patch_embed", patch_embed)


_add("tokens: pose tokens placed before the noise tokens", _pose_first)


def _const_channels(m, which, value):
    orig = O.patch_embed

    def patch_embed(cfg, sd, x20, ref20, pose20):
        z = [x20.clone(), ref20.clone(), pose20.clone()]
        z[which][:, :, 16:] = value
        return orig(cfg, sd, *z)
    m.patch("patch_embed", patch_embed)


_add("channels: the four constant channels of ref20 as zeros", lambda m: _const_channels(m, 1, 0.0))
_add("channels: the four constant channels of pose20 as zeros", lambda m: _const_channels(m, 2, 0.0))
_add("channels: the four constant channels of x20 as ones", lambda m: _const_channels(m, 0, 1.0))


def _text_kv_swapped(m):
    D = m.cfg.hidden_size
    for i in range(m.cfg.num_layers):
        for suf in ("weight", "bias"):
            k = _lay(i) + "cross_attention.key_value." + suf
            m.sd[k] = torch.cat([m.sd[k][D:], m.sd[k][:D]], dim=0)


_add("channels: k and v halves of the text key_value output swapped", _text_kv_swapped)


# ---- attention and time
def _cross_variant(m, one_softmax=False, no_clip=False):
    def cross_attention(cfg, sd, i, x, text, clip):
        L = f"transformer.layers.{i}.cross_attention."
        eps, n = cfg.layernorm_epsilon, cfg.num_attention_heads
        q = F.linear(x, sd[L + "query.weight"], sd[L + "query.bias"])
        k, v = F.linear(text, sd[L + "key_value.weight"], sd[L + "key_value.bias"]).chunk(2, dim=-1)
        kc, vc = F.linear(clip, sd[f"mixins.adaln_layer.clip_feature_key_value_list.{i}.weight"],
                          sd[f"mixins.adaln_layer.clip_feature_key_value_list.{i}.bias"]).chunk(2, dim=-1)
        q = O._heads(O.rms_norm(q, sd[f"mixins.adaln_layer.cross_query_layernorm_list.{i}.weight"], eps), n)
        k = O.rms_norm(k, sd[f"mixins.adaln_layer.cross_key_layernorm_list.{i}.weight"], eps)
        kc = O.rms_norm(kc, sd[f"mixins.adaln_layer.clip_feature_key_layernorm_list.{i}.weight"], eps)
        if one_softmax:
            ctx = O._merge(O.sdpa(q, O._heads(torch.cat([k, kc], 1), n), O._heads(torch.cat([v, vc], 1), n)))
        else:
            assert no_clip
            ctx = O._merge(O.sdpa(q, O._heads(k, n), O._heads(v, n)))
        return F.linear(ctx, sd[L + "dense.weight"], sd[L + "dense.bias"])
    m.patch("cross_attention", cross_attention)


_add("attention: text and CLIP keys in ONE softmax instead of two summed", lambda m: _cross_variant(m, one_softmax=True))
_add("attention: CLIP attention dropped", lambda m: _cross_variant(m, no_clip=True))


def _sin_cos(m):
    orig = O.timestep_embedding

    def timestep_embedding(timesteps, dim, max_period=10000.0):
        emb = orig(timesteps, dim, max_period)
        half = dim // 2
        return torch.cat([emb[:, half:2 * half], emb[:, :half], emb[:, 2 * half:]], dim=-1)
    m.patch("timestep_embedding", timestep_embedding)


_add("time: [cos | sin] -> [sin | cos]", _sin_cos)


def _cond_prompt_twice(m):
    orig = O.text_embedding

    def text_embedding(cfg, sd, ctx):
        t = orig(cfg, sd, ctx)
        return t[-1:].expand_as(t).contiguous()
    m.patch("text_embedding", text_embedding)


_add("batch: the conditional prompt's context used for both batch rows", _cond_prompt_twice)

# Entries that are provably invariant at every network-level point: name -> (reason, the kernel-level exact test that covers the wire).
# At most 4; none of the mutants of the issue's first table.
NOT_VISIBLE: Dict[str, tuple] = {}


def visibility(cfg, sd, inp, entries=None):
    """[(entry name, best point, e at it / T_p at it, {point: e})] of every catalogue entry: the MUTATED fp32 oracle against the
    unmutated fp32 oracle at every observation point, in units of the GPU tests' bound"""
    Tp = bounds()["T"]
    ref = oracle_points(cfg, sd, inp)
    bi = block_inputs_of(cfg, ref)
    ref = oracle_points(cfg, sd, inp, bi)
    rows = []
    for c in (CATALOGUE if entries is None else entries):
        with applied(c, cfg, sd) as (cfg_m, sd_m):
            got = oracle_points(cfg_m, sd_m, inp, bi)
        es = {p: e(got[p], ref[p]) for p in points_of(cfg)}
        best = max(es, key=lambda p: es[p] / Tp[p])
        rows.append((c.name, best, es[best] / Tp[best], es))
    return rows
