"""Wiring tests of the two conditioning encoders: the shared helper (no GPU code; tests/test_enc_wiring_cpu.py, tests/test_enc_wiring_gpu.py).

The scheme is that of tests/dit_wiring.py -- the same metric e(a, b) = ||a - b||_2 / ||b||_2, the same N_p (distance of a bf16-storage
model from the fp32 oracle at observation point p, the larger of two draws of the inputs), the same T_p = 2 N_p held by the GPU tests,
the same catalogue of single-wire mutants each of which must move some point by >= 4 T_p, the same ``applied``.  What differs is the
object: the COMPOSITION in scail_amd/umt5.py and scail_amd/clip.py (which gamma, bias, table, slice and mask reaches which kernel),
which tests/golden/encoders_tiny.npz cannot see: it was written from the reference classes' default initialisation, where every norm
weight is 1 and every LayerNorm bias 0.  This module holds

  * PLANTED towers and inputs, seeded, bf16-exact, nothing taken from a reference tree:
      UMT5  vocab 64, dim 128, dim_attn 192 = 3 heads x 64 (dim_attn != dim: a q / k / v slice cut at dim lands in the wrong place),
            dim_ffn 320, 2 layers, 32 buckets; ids (3, 136) with valid lengths 136, 51 and 1 (the empty prompt's shape), id 0 as padding.
            136 keys reach all 31 reachable buckets and the clamp min(large, nb - 1) (relative distance >= 128); 136 is no multiple of
            64.  Gammas uniform in [0.5, 2], drawn per norm; position tables N(0, 2) against q . k of std about 1.3 (scores are mostly a
            function of relative position, and the softmax does not saturate); the buckets of the clamp (15, 31) sit at +4 and the
            one bucket the map never reaches (16) at -4; vocabulary row TINY_ID has rms 1e-3 and stands at ten valid positions, where
            eps 1e-6 shows in layer 0's norm1.
      CLIP  image 70, patch 14 -> 5 x 5 + 1 = 26 tokens, dim 320 = 4 heads x 80, mlp_ratio 4, num_layers 3 (two evaluated under
            use_31_block), 3 images.  LayerNorm weights uniform in [0.5, 2], LayerNorm biases N(0, 0.5), Linear biases, cls_embedding and
            pos_embedding at the scale of the activations they meet (TABLES below), the third block's weights 8 x larger (a path that
            evaluates it cannot pass).  mlp.0 has gain 0.5 and a bias of N(-2, 0.5), mlp.2 gain 12: the pre-activations sit around -2,
            where quick-GELU and GELU differ by 10 to 20 % of the value and not by 1 % as around 0, and the MLP branch is still about
            half of the stream.  One planted token makes norm_eps visible: patch (2, 2) of image 1 is black and row TINY_TOKEN
            of pos_embedding has rms 1e-3, so that token meets pre_norm with a variance of about 1e-6.
    Every kernel took these dims as they are; nothing had to be moved to a nearest accepted one.

  * OBSERVATION POINTS: "x0" (T5: the embedding; CLIP: the pre_norm output), "h1" .. "hN" (the stream after each evaluated block), "out"
    (T5: after the final norm; CLIP: the stream after the last evaluated block), for T5 also "model" (T5EncoderModel.forward: padded
    rows zeroed), and "pre" (the preprocessing of CLIPModel.visual alone).  t5_points / clip_points restate
    oracle.encoders_oracle.t5_encoder / clip_visual_31 in pieces (bit for bit, asserted on the CPU), so that a piece can be replaced.
    No entry needed block-local points: every layer-1 wire reaches 4 T_p at "h2" or "out".

  * a MUTATION CATALOGUE (CATALOGUE; Entry.tower is "t5", "clip" or "pre"): each entry edits the state dict / config or monkeypatches ONE
    function of oracle.encoders_oracle or of its restatement here for the duration of a call (``applied``).  EXEMPT names the entries
    that need not reach 4 T_p, each with the assertion that tests/test_enc_wiring_cpu.py makes about it.

  * a BF16-STORAGE MODEL (t5_storage / clip_storage): the oracle in fp32 with one round-to-nearest-even to bf16 at exactly the points
    where the library stores bf16.  Every GEMM, the convolution and attn_small accumulate in fp32; norm weights, biases and the T5
    position tables are fp32.
      umt5.py  the gathered embedding rows (a bf16 table: exact); per layer the norm1 output; the fused q | k | v GEMM output; the
               attn_small output (inside it the scores, exp(s - max) and the row sum stay fp32 in LDS and registers: NOTHING is
               stored between Q.K and P.V); x after the o GEMM + residual; the norm2 output; the gate GEMM output after tanh-GELU; the
               fc1 GEMM output; their product (the in-place mul_ of h by gate); x after the fc2 GEMM + residual; after the layers the
               final norm's output; in T5EncoderModel the row_affine output (x 0 or x 1: exact).
      clip.py  the channels-last image; the patch convolution's output; cls_embedding and pos_embedding as bf16 (W["cls"], W["pos"]);
               tokens + pos (row_affine); the pre_norm output; per block the norm1 output; the qkv GEMM output (bias in the epilogue);
               the attn_small output (q x scale is fp32); x after proj + bias + residual; the norm2 output; the mlp.0 GEMM output after
               erf-GELU; x after mlp.2 + bias + residual.  CLIPModel.visual preprocesses in fp32 torch ops ahead of all that.
"""
from __future__ import annotations

import contextlib
import dataclasses
import math
import sys
from typing import Callable, Dict, List

import torch
import torch.nn.functional as F

from oracle import encoders_oracle as E

T5CFG = dict(vocab=64, dim=128, dim_attn=192, dim_ffn=320, num_heads=3, num_layers=2, num_buckets=32)
VITCFG = dict(image_size=70, patch_size=14, dim=320, mlp_ratio=4, out_dim=64, num_heads=4, num_layers=3, norm_eps=1e-5)
B, LEN, VALID = 3, 136, (136, 51, 1)
TINY_ID, TINY_AT = 9, ((0, 3, 17, 40, 64, 77, 101, 130), (1, 5, 33, 50))      # the rms 1e-3 vocabulary row and where it stands (row, positions)
TINY_TOKEN, TINY_IMAGE = 13, 1                                               # token 13 = patch (2, 2)
CLIP_SHAPE = (3, 1, 96, 160)                                                 # the clip CLIPModel.visual preprocesses
SEED, SEED2 = 2025, 5171                                                     # the planted draw, and the second draw of the inputs
_SELF = sys.modules[__name__]


def bf16r(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(torch.float32)


def e(a: torch.Tensor, b: torch.Tensor) -> float:
    """the metric: ||a - b||_2 / ||b||_2 in fp64 (0 / 0 = 0)"""
    a, b = a.double(), b.double()
    d = float((a - b).norm())
    return d / float(b.norm()) if d else 0.0


# ------------------------------------------------------------------------------------------------------------------------------------
# the planted towers.  TABLES: name suffix -> gain of a matrix (std = gain / sqrt(fan_in)) or std of a vector; first match wins.  The
# scales were chosen on the CPU so that condition (b) of tests/test_enc_wiring_cpu.py holds; they are data of the tests and FROZEN: the
# bounds of the GPU tests follow from them.
# ------------------------------------------------------------------------------------------------------------------------------------
T5_GAIN = (("attn.q.weight", 0.3), ("attn.k.weight", 0.3), ("pos_embedding.embedding.weight", 2.0), ("", 1.0))
VIT_GAIN = (("attn.to_qkv.weight", 0.85), ("mlp.0.weight", 0.5), ("mlp.2.weight", 12.0), ("", 1.0))
MLP0_BIAS_MEAN = -2.0          # module docstring: where quick-GELU shows
VIT_STD = (("attn.to_qkv.bias", 1.0), ("cls_embedding", 1.0), ("pos_embedding", 1.0), ("norm1.bias", 0.5), ("norm2.bias", 0.5),
           ("pre_norm.bias", 0.5), ("post_norm.bias", 0.5), ("", 0.5))
CLAMP_BUCKETS, UNREACHED_BUCKET = (15, 31), 16
THIRD_BLOCK = 8.0


def _scale(table, name):
    return next(v for k, v in table if name.endswith(k))


def t5_spec(cfg=T5CFG):
    D, A, Fd = cfg["dim"], cfg["dim_attn"], cfg["dim_ffn"]
    spec = {"token_embedding.weight": (cfg["vocab"], D)}
    for i in range(cfg["num_layers"]):
        p = f"blocks.{i}."
        spec.update({p + "norm1.weight": (D,), p + "attn.q.weight": (A, D), p + "attn.k.weight": (A, D), p + "attn.v.weight": (A, D),
                     p + "attn.o.weight": (D, A), p + "norm2.weight": (D,), p + "ffn.gate.0.weight": (Fd, D), p + "ffn.fc1.weight": (Fd, D),
                     p + "ffn.fc2.weight": (D, Fd), p + "pos_embedding.embedding.weight": (cfg["num_buckets"], cfg["num_heads"])})
    spec["norm.weight"] = (D,)
    return spec


def planted_t5(cfg=T5CFG, seed: int = SEED) -> Dict[str, torch.Tensor]:
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in t5_spec(cfg).items():
        if name.endswith("norm1.weight") or name.endswith("norm2.weight") or name == "norm.weight":
            w = 0.5 + 1.5 * torch.rand(shape, generator=g)
        elif name == "token_embedding.weight":
            w = torch.randn(shape, generator=g) * (0.5 + torch.rand(shape[0], 1, generator=g))
            w[TINY_ID] *= 1e-3 / float(w[TINY_ID].pow(2).mean().sqrt())
        elif name.endswith("pos_embedding.embedding.weight"):
            w = _scale(T5_GAIN, name) * torch.randn(shape, generator=g)
            w[list(CLAMP_BUCKETS)] = 4.0 + 0.25 * torch.randn(2, shape[1], generator=g)
            w[UNREACHED_BUCKET] = -4.0
        else:
            w = torch.randn(shape, generator=g) * (_scale(T5_GAIN, name) / math.sqrt(shape[1]))
        sd[name] = bf16r(w)
    return sd


def planted_t5_inputs(seed: int = SEED, full_mask: bool = False) -> Dict[str, torch.Tensor]:
    """ids (3, 136) int64: no TINY_ID and no padding id among the draws, TINY_ID at TINY_AT, id 0 where the mask is 0; mask (3, 136)"""
    g = torch.Generator().manual_seed(seed + 1)
    ids = torch.randint(1, T5CFG["vocab"] - 1, (B, LEN), generator=g)
    ids[ids >= TINY_ID] += 1
    for row, *at in TINY_AT:
        ids[row, list(at)] = TINY_ID
    mask = torch.ones(B, LEN, dtype=torch.long)
    if not full_mask:
        for b, n in enumerate(VALID):
            mask[b, n:] = 0
        ids = ids * mask
    return dict(ids=ids, mask=mask)


def vit_spec(cfg=VITCFG):
    D, P, mid = cfg["dim"], cfg["patch_size"], int(cfg["dim"] * cfg["mlp_ratio"])
    n = (cfg["image_size"] // P) ** 2 + 1
    spec = {"patch_embedding.weight": (D, 3, P, P), "cls_embedding": (1, 1, D), "pos_embedding": (1, n, D),
            "pre_norm.weight": (D,), "pre_norm.bias": (D,)}
    for i in range(cfg["num_layers"]):
        p = f"transformer.{i}."
        spec.update({p + "norm1.weight": (D,), p + "norm1.bias": (D,), p + "attn.to_qkv.weight": (3 * D, D), p + "attn.to_qkv.bias": (3 * D,),
                     p + "attn.proj.weight": (D, D), p + "attn.proj.bias": (D,), p + "norm2.weight": (D,), p + "norm2.bias": (D,),
                     p + "mlp.0.weight": (mid, D), p + "mlp.0.bias": (mid,), p + "mlp.2.weight": (D, mid), p + "mlp.2.bias": (D,)})
    spec.update({"post_norm.weight": (D,), "post_norm.bias": (D,), "head": (D, cfg["out_dim"])})
    return spec


def planted_vit(cfg=VITCFG, seed: int = SEED) -> Dict[str, torch.Tensor]:
    g = torch.Generator().manual_seed(seed + 2)
    D = cfg["dim"]
    sd = {}
    for name, shape in vit_spec(cfg).items():
        if name.endswith("norm.weight") or name.endswith("norm1.weight") or name.endswith("norm2.weight"):
            w = 0.5 + 1.5 * torch.rand(shape, generator=g)
        elif len(shape) == 1 or name in ("cls_embedding", "pos_embedding"):
            w = _scale(VIT_STD, name) * torch.randn(shape, generator=g)
            if name == "pos_embedding":
                w[0, TINY_TOKEN] *= 1e-3 / float(w[0, TINY_TOKEN].pow(2).mean().sqrt())
            elif name.endswith("mlp.0.bias"):
                w = w + MLP0_BIAS_MEAN
        else:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            if name == "head":
                fan_in = shape[0]
            w = torch.randn(shape, generator=g) * (_scale(VIT_GAIN, name) / math.sqrt(fan_in))
            if name.endswith("attn.to_qkv.weight"):
                w[2 * D:] *= 1.0 / 0.85                                       # the v third at gain 1
        if name.startswith(f"transformer.{cfg['num_layers'] - 1}.") and not name.endswith("norm1.weight") and not name.endswith("norm2.weight"):
            w = w * THIRD_BLOCK
        sd[name] = bf16r(w)
    return sd


def planted_images(seed: int = SEED) -> torch.Tensor:
    """(3, 3, 70, 70) resized + normalised images, N(0, 1), bf16-exact; patch (2, 2) of image TINY_IMAGE is black"""
    g = torch.Generator().manual_seed(seed + 3)
    S, P = VITCFG["image_size"], VITCFG["patch_size"]
    x = bf16r(torch.randn(B, 3, S, S, generator=g))
    gy, gx = divmod(TINY_TOKEN - 1, S // P)
    x[TINY_IMAGE, :, gy * P:(gy + 1) * P, gx * P:(gx + 1) * P] = 0
    return x


def planted_clip(seed: int = SEED) -> torch.Tensor:
    """one (3, 1, 96, 160) clip in [-1, 1], uniform, bf16-exact: what CLIPModel.visual is given"""
    g = torch.Generator().manual_seed(seed + 4)
    return bf16r(torch.rand(CLIP_SHAPE, generator=g) * 2 - 1).clamp_(-1, 1)


# ------------------------------------------------------------------------------------------------------------------------------------
# the oracle restated in pieces.  Functions of oracle.encoders_oracle are reached through the module (E.t5_norm ...) and the pieces
# below through this module's globals, so that a monkeypatched function takes effect.
# ------------------------------------------------------------------------------------------------------------------------------------
def t5_embed(sd, ids):
    return sd["token_embedding.weight"][ids]


def t5_mask_bias(bias, mask):
    return bias.masked_fill_(mask.view(mask.shape[0], 1, 1, -1) == 0, torch.finfo(bias.dtype).min)


def t5_attention(cfg, sd, i, h, bucket, mask):
    p = f"blocks.{i}."
    Bn, Ln, _ = h.shape
    q, k, v = (F.linear(h, sd[p + f"attn.{c}.weight"]).view(Bn, Ln, cfg["num_heads"], -1) for c in "qkv")
    bias = sd[p + "pos_embedding.embedding.weight"][bucket].permute(2, 0, 1).unsqueeze(0).expand(Bn, -1, -1, -1).clone()
    bias = t5_mask_bias(bias, mask)
    att = torch.softmax(torch.einsum("binc,bjnc->bnij", q, k) + bias, dim=-1)
    a = torch.einsum("bnij,bjnc->binc", att, v).reshape(Bn, Ln, -1)
    return F.linear(a, sd[p + "attn.o.weight"])


def t5_ffn(sd, i, h):
    p = f"blocks.{i}."
    f = F.linear(h, sd[p + "ffn.fc1.weight"]) * E.t5_gelu(F.linear(h, sd[p + "ffn.gate.0.weight"]))
    return F.linear(f, sd[p + "ffn.fc2.weight"])


def t5_residual(i, which, x, y):
    """which: "o" or "fc2" """
    return x + y


def t5_block(cfg, sd, i, x, bucket, mask):
    p = f"blocks.{i}."
    x = t5_residual(i, "o", x, t5_attention(cfg, sd, i, E.t5_norm(x, sd[p + "norm1.weight"]), bucket, mask))
    return t5_residual(i, "fc2", x, t5_ffn(sd, i, E.t5_norm(x, sd[p + "norm2.weight"])))


def t5_final(sd, x):
    return E.t5_norm(x, sd["norm.weight"])


def t5_wrapper(out, mask):
    """T5EncoderModel: context * mask[:, :, None] (umt5.py:522)"""
    return out * mask[:, :, None].to(out.dtype)


def t5_points(cfg, sd, inp) -> Dict[str, torch.Tensor]:
    ids, mask = inp["ids"], inp["mask"]
    x = t5_embed(sd, ids)
    pts = {"x0": x}
    bucket = E.t5_bucket(ids.shape[1], ids.shape[1], cfg["num_buckets"])
    for i in range(cfg["num_layers"]):
        x = t5_block(cfg, sd, i, x, bucket, mask)
        pts[f"h{i + 1}"] = x
    pts["out"] = t5_final(sd, x)
    pts["model"] = t5_wrapper(pts["out"], mask)
    return pts


def clip_stem(cfg, sd, imgs, pre_norm=True, pos_after=False, cls_last=False, column_major=False):
    """patch convolution, cls token, position embedding, pre_norm (the keywords: variants for the catalogue)"""
    x = F.conv2d(imgs, sd["patch_embedding.weight"], None, stride=cfg["patch_size"])
    if column_major:
        x = x.transpose(2, 3)
    x = x.flatten(2).permute(0, 2, 1)
    Bn, _, D = x.shape
    cls = sd["cls_embedding"].expand(Bn, -1, -1)
    x = torch.cat([x, cls] if cls_last else [cls, x], dim=1)
    if not pos_after:
        x = x + sd["pos_embedding"]
    if pre_norm:
        x = F.layer_norm(x, (D,), sd["pre_norm.weight"], sd["pre_norm.bias"], cfg["norm_eps"])
    return x + sd["pos_embedding"] if pos_after else x


def clip_gelu(x):
    return F.gelu(x)


def clip_block(cfg, sd, i, x):
    p = f"transformer.{i}."
    Bn, _, D = x.shape
    H, eps = cfg["num_heads"], cfg["norm_eps"]
    hd = D // H
    h = F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
    qkv = F.linear(h, sd[p + "attn.to_qkv.weight"], sd[p + "attn.to_qkv.bias"]).view(Bn, -1, 3, H, hd).permute(2, 0, 3, 1, 4)
    a = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) / math.sqrt(hd), dim=-1) @ qkv[2]
    x = x + F.linear(a.permute(0, 2, 1, 3).reshape(Bn, -1, D), sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    h = F.layer_norm(x, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
    h = clip_gelu(F.linear(h, sd[p + "mlp.0.weight"], sd[p + "mlp.0.bias"]))
    return x + F.linear(h, sd[p + "mlp.2.weight"], sd[p + "mlp.2.bias"])


def evaluated(cfg) -> int:
    """use_31_block: all blocks but the last"""
    return cfg.get("evaluated", cfg["num_layers"] - 1)


def clip_points(cfg, sd, imgs) -> Dict[str, torch.Tensor]:
    x = clip_stem(cfg, sd, imgs)
    pts = {"x0": x}
    for i in range(evaluated(cfg)):
        x = clip_block(cfg, sd, i, x)
        if i < cfg["num_layers"] - 1:
            pts[f"h{i + 1}"] = x
    pts["out"] = x
    return pts


def pre_points(clip) -> Dict[str, torch.Tensor]:
    return {"pre": E.clip_preprocess(clip.transpose(0, 1), size=VITCFG["image_size"])}


T5_POINTS = ["x0", "h1", "h2", "out", "model"]
CLIP_POINTS = ["x0", "h1", "h2", "out"]


# ------------------------------------------------------------------------------------------------------------------------------------
# the bf16-storage model (store points: module docstring)
# ------------------------------------------------------------------------------------------------------------------------------------
def t5_storage(cfg, sd, inp, r: Callable = bf16r) -> Dict[str, torch.Tensor]:
    ids, mask = inp["ids"], inp["mask"]
    Bn, Ln = ids.shape
    H, A = cfg["num_heads"], cfg["dim_attn"]
    x = r(sd["token_embedding.weight"][ids])
    pts = {"x0": x}
    bucket = E.t5_bucket(Ln, Ln, cfg["num_buckets"])
    for i in range(cfg["num_layers"]):
        p = f"blocks.{i}."
        xn = r(E.t5_norm(x, sd[p + "norm1.weight"]))
        qkv = r(F.linear(xn, torch.cat([sd[p + f"attn.{c}.weight"] for c in "qkv"], 0)))
        q, k, v = (qkv[..., j * A:(j + 1) * A].reshape(Bn, Ln, H, -1) for j in range(3))
        bias = sd[p + "pos_embedding.embedding.weight"][bucket].permute(2, 0, 1).unsqueeze(0).expand(Bn, -1, -1, -1).clone()
        bias.masked_fill_(mask.view(Bn, 1, 1, -1) == 0, float("-inf"))
        att = torch.softmax(torch.einsum("binc,bjnc->bnij", q, k) + bias, dim=-1)
        a = r(torch.einsum("bnij,bjnc->binc", att, v).reshape(Bn, Ln, -1))
        x = r(x + F.linear(a, sd[p + "attn.o.weight"]))
        xn = r(E.t5_norm(x, sd[p + "norm2.weight"]))
        gate = r(E.t5_gelu(F.linear(xn, sd[p + "ffn.gate.0.weight"])))
        h = r(F.linear(xn, sd[p + "ffn.fc1.weight"]))
        h = r(h * gate)
        x = r(x + F.linear(h, sd[p + "ffn.fc2.weight"]))
        pts[f"h{i + 1}"] = x
    pts["out"] = r(E.t5_norm(x, sd["norm.weight"]))
    pts["model"] = r(pts["out"] * mask[:, :, None].float())
    return pts


def clip_storage(cfg, sd, imgs, r: Callable = bf16r) -> Dict[str, torch.Tensor]:
    H, eps, P = cfg["num_heads"], cfg["norm_eps"], cfg["patch_size"]
    pe = r(F.conv2d(r(imgs), sd["patch_embedding.weight"], None, stride=P)).flatten(2).permute(0, 2, 1)
    Bn, _, D = pe.shape
    hd = D // H
    x = r(torch.cat([r(sd["cls_embedding"]).expand(Bn, -1, -1), pe], dim=1) + r(sd["pos_embedding"]))
    x = r(F.layer_norm(x, (D,), sd["pre_norm.weight"], sd["pre_norm.bias"], eps))
    pts = {"x0": x}
    for i in range(evaluated(cfg)):
        p = f"transformer.{i}."
        h = r(F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps))
        qkv = r(F.linear(h, sd[p + "attn.to_qkv.weight"], sd[p + "attn.to_qkv.bias"])).view(Bn, -1, 3, H, hd).permute(2, 0, 3, 1, 4)
        a = torch.softmax((qkv[0] / math.sqrt(hd)) @ qkv[1].transpose(-1, -2), dim=-1) @ qkv[2]
        a = r(a.permute(0, 2, 1, 3).reshape(Bn, -1, D))
        x = r(x + F.linear(a, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"]))
        h = r(F.layer_norm(x, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps))
        h = r(F.gelu(F.linear(h, sd[p + "mlp.0.weight"], sd[p + "mlp.0.bias"])))
        x = r(x + F.linear(h, sd[p + "mlp.2.weight"], sd[p + "mlp.2.bias"]))
        pts[f"h{i + 1}"] = x
    pts["out"] = x
    return pts


_BOUNDS: Dict = {}


def _two_draws(points, storage, draws):
    ab = []
    for inp in draws:
        ref, got = points(inp), storage(inp)
        ab.append({p: e(got[p], ref[p]) for p in ref})
    N = {p: max(ab[0][p], ab[1][p]) for p in ab[0]}
    return dict(N=N, T={p: 2.0 * v for p, v in N.items()}, draws=tuple(ab))


def t5_bounds(full_mask: bool = False) -> Dict[str, Dict[str, float]]:
    """{"N": N_p, "T": T_p = 2 N_p, "draws"} of the planted UMT5 on the planted batch (``full_mask``: the same ids, no padding).  N_p is
    the larger of the storage model's distance on two draws of the ids.  CPU only; the GPU tests take their bounds from here."""
    key = ("t5", full_mask)
    if key not in _BOUNDS:
        sd = planted_t5()
        _BOUNDS[key] = _two_draws(lambda inp: t5_points(T5CFG, sd, inp), lambda inp: t5_storage(T5CFG, sd, inp),
                                  [planted_t5_inputs(s, full_mask) for s in (SEED, SEED2)])
    return _BOUNDS[key]


def clip_bounds() -> Dict[str, Dict[str, float]]:
    """the same for the planted CLIP tower on two draws of the three images"""
    if "clip" not in _BOUNDS:
        sd = planted_vit()
        _BOUNDS["clip"] = _two_draws(lambda x: clip_points(VITCFG, sd, x), lambda x: clip_storage(VITCFG, sd, x),
                                     [planted_images(s) for s in (SEED, SEED2)])
    return _BOUNDS["clip"]


# ------------------------------------------------------------------------------------------------------------------------------------
# the mutation catalogue
# ------------------------------------------------------------------------------------------------------------------------------------
class Mut:
    """What a catalogue entry may change: ``sd`` (a private copy), ``cfg`` (a private copy), ``patch(name, fn)`` of a function of
    oracle.encoders_oracle or, where the oracle has no such piece, of its restatement in this module"""

    def __init__(self, cfg, sd):
        self.cfg, self.sd, self.patches = dict(cfg), dict(sd), {}

    def patch(self, name, fn):
        assert (hasattr(E, name) or hasattr(_SELF, name)) and name not in self.patches
        self.patches[name] = fn

    def zero(self, key, sl=slice(None)):
        w = self.sd[key].clone()
        w[sl] = 0
        self.sd[key] = w

    def ones(self, key):
        self.sd[key] = torch.ones_like(self.sd[key])

    def swap(self, a, b):
        self.sd[a], self.sd[b] = self.sd[b], self.sd[a]


def _home(name):
    return E if hasattr(E, name) else _SELF


@contextlib.contextmanager
def applied(entry, cfg, sd):
    """``with applied(entry, cfg, sd) as (cfg_m, sd_m):`` -- the mutated config / weights, the oracle patched inside the block"""
    m = Mut(cfg, sd)
    entry.fn(m)
    saved = {k: getattr(_home(k), k) for k in m.patches}
    try:
        for k, f in m.patches.items():
            setattr(_home(k), k, f)
        yield m.cfg, m.sd
    finally:
        for k, f in saved.items():
            setattr(_home(k), k, f)


@dataclasses.dataclass
class Entry:
    tower: str
    name: str
    fn: Callable


CATALOGUE: List[Entry] = []


def _add(tower, name, fn):
    name = f"{tower}: {name}"
    assert all(c.name != name for c in CATALOGUE), name
    CATALOGUE.append(Entry(tower, name, fn))


def by_name(name: str) -> Entry:
    return next(c for c in CATALOGUE if c.name == name)


# ---- UMT5
_NL, _A, _D, _H = T5CFG["num_layers"], T5CFG["dim_attn"], T5CFG["dim"], T5CFG["num_heads"]
T5_GAMMAS = [f"blocks.{i}.{n}.weight" for i in range(_NL) for n in ("norm1", "norm2")] + ["norm.weight"]
for _k in T5_GAMMAS:
    _add("t5", f"gamma {_k} replaced by 1", lambda m, k=_k: m.ones(k))
for _i in range(_NL):
    _add("t5", f"norm1 <-> norm2 gammas, layer {_i}", lambda m, i=_i: m.swap(f"blocks.{i}.norm1.weight", f"blocks.{i}.norm2.weight"))
_add("t5", "final norm skipped", lambda m: m.patch("t5_final", lambda sd, x: x))
_POS = "blocks.{}.pos_embedding.embedding.weight"
for _i in range(_NL):
    _add("t5", f"position table zeroed, layer {_i}", lambda m, i=_i: m.zero(_POS.format(i)))
_add("t5", "layer 0's position table used in every layer", lambda m: m.sd.__setitem__(_POS.format(1), m.sd[_POS.format(0)]))


def _bucket_variant(m, transposed=False, max_dist=128, clamp=True):
    orig = E.t5_bucket

    def t5_bucket(lq, lk, num_buckets=32, md=128):
        if clamp:
            b = orig(lq, lk, num_buckets, max_dist)
            return b.t().contiguous() if transposed else b
        rel = torch.arange(lk).unsqueeze(0) - torch.arange(lq).unsqueeze(1)
        nb = num_buckets // 2
        out = (rel > 0).long() * nb
        rel = rel.abs()
        me = nb // 2
        large = me + (torch.log(rel.float() / me) / math.log(max_dist / me) * (nb - me)).long()
        return (out + torch.where(rel < me, rel, large)) % num_buckets           # no min(large, nb - 1); the index wraps inside the table
    m.patch("t5_bucket", t5_bucket)


_add("t5", "bucket map transposed (key - query taken as query - key)", lambda m: _bucket_variant(m, transposed=True))
_add("t5", "bucket map: max_dist 64 for 128", lambda m: _bucket_variant(m, max_dist=64))
_add("t5", "bucket map: the clamp min(large, nb - 1) dropped", lambda m: _bucket_variant(m, clamp=False))
_add("t5", "key mask ignored", lambda m: m.patch("t5_mask_bias", lambda bias, mask: bias))
_add("t5", "mask applied to the queries", lambda m: m.patch(
    "t5_mask_bias", lambda bias, mask: bias.masked_fill_(mask.view(mask.shape[0], 1, -1, 1) == 0, torch.finfo(bias.dtype).min)))


def _all_layers(m, fn):
    for i in range(_NL):
        fn(m, f"blocks.{i}.")


_add("t5", "scores scaled by 1 / sqrt(64)", lambda m: _all_layers(m, lambda m, p: m.sd.__setitem__(p + "attn.q.weight", m.sd[p + "attn.q.weight"] / 8)))
_add("t5", "k and v slices swapped", lambda m: _all_layers(m, lambda m, p: m.swap(p + "attn.k.weight", p + "attn.v.weight")))


def _cut_at_dim(m, p):
    """the fused q | k | v output cut at multiples of dim (128) instead of dim_attn (192), each slice dim_attn wide"""
    fused = torch.cat([m.sd[p + f"attn.{c}.weight"] for c in "qkv"], 0)
    for j, c in enumerate("qkv"):
        m.sd[p + f"attn.{c}.weight"] = fused[j * _D:j * _D + _A].contiguous()


_add("t5", "q / k / v cut at dim instead of dim_attn", lambda m: _all_layers(m, _cut_at_dim))


def _interleaved(m, p):
    """head n takes channels n, n + H, n + 2 H ... of q, k and v, and writes its output there"""
    hd = _A // _H
    perm = torch.arange(_A).view(hd, _H).t().reshape(-1)                        # new channel n * hd + d <- old channel d * H + n
    for c in "qkv":
        m.sd[p + f"attn.{c}.weight"] = m.sd[p + f"attn.{c}.weight"][perm].contiguous()
    m.sd[p + "attn.o.weight"] = m.sd[p + "attn.o.weight"][:, perm].contiguous()


_add("t5", "heads interleaved instead of contiguous", lambda m: _all_layers(m, _interleaved))
_add("t5", "gate and fc1 swapped", lambda m: _all_layers(m, lambda m, p: m.swap(p + "ffn.gate.0.weight", p + "ffn.fc1.weight")))
for _i in range(_NL):
    for _w, _nm in (("o", "o-projection"), ("fc2", "fc2")):
        _add("t5", f"{_nm} residual dropped, layer {_i}",
             lambda m, i=_i, w=_w: m.patch("t5_residual", lambda j, which, x, y: y if (j, which) == (i, w) else x + y))
_add("t5", "ids off by one", lambda m: m.sd.__setitem__("token_embedding.weight", torch.roll(m.sd["token_embedding.weight"], -1, 0)))
_add("t5", "norm eps 1e-5 for 1e-6", lambda m: m.patch("t5_norm", (lambda orig: lambda x, w, eps=1e-6: orig(x, w, 1e-5))(E.t5_norm)))
_add("t5", "the wrapper's zeroing of padded rows dropped", lambda m: m.patch("t5_wrapper", lambda out, mask: out))
_add("t5", "erf-GELU for tanh-GELU", lambda m: m.patch("t5_gelu", lambda x: F.gelu(x)))

# ---- CLIP
_EV = VITCFG["num_layers"] - 1
_VD = VITCFG["dim"]
CLIP_NORMS = ["pre_norm"] + [f"transformer.{i}.{n}" for i in range(_EV) for n in ("norm1", "norm2")]
for _k in CLIP_NORMS:
    _add("clip", f"LayerNorm weight {_k} replaced by 1", lambda m, k=_k: m.ones(k + ".weight"))
    _add("clip", f"LayerNorm bias {_k} zeroed", lambda m, k=_k: m.zero(k + ".bias"))


def _swap_norms(m, i):
    for s in ("weight", "bias"):
        m.swap(f"transformer.{i}.norm1.{s}", f"transformer.{i}.norm2.{s}")


for _i in range(_EV):
    _add("clip", f"norm1 <-> norm2, block {_i}", lambda m, i=_i: _swap_norms(m, i))


def _stem(m, **kw):
    orig = clip_stem
    m.patch("clip_stem", lambda cfg, sd, imgs: orig(cfg, sd, imgs, **kw))


_add("clip", "pre_norm skipped", lambda m: _stem(m, pre_norm=False))
_add("clip", "position embedding added after pre_norm", lambda m: _stem(m, pos_after=True))
for _i in range(_EV):
    _p = f"transformer.{_i}."
    for _nm, _key, _sl in (("to_qkv (q third)", _p + "attn.to_qkv.bias", slice(0, _VD)), ("to_qkv (k third)", _p + "attn.to_qkv.bias", slice(_VD, 2 * _VD)),
                           ("to_qkv (v third)", _p + "attn.to_qkv.bias", slice(2 * _VD, 3 * _VD)), ("proj", _p + "attn.proj.bias", slice(None)),
                           ("mlp.0", _p + "mlp.0.bias", slice(None)), ("mlp.2", _p + "mlp.2.bias", slice(None))):
        _add("clip", f"bias zeroed: {_nm}, block {_i}", lambda m, k=_key, s=_sl: m.zero(k, s))
_add("clip", "cls_embedding zeroed", lambda m: m.zero("cls_embedding"))
_add("clip", "cls_embedding placed last", lambda m: _stem(m, cls_last=True))
_add("clip", "pos_embedding shifted by one token", lambda m: m.sd.__setitem__("pos_embedding", torch.roll(m.sd["pos_embedding"], 1, 1)))


def _scale_by_dim(m):
    f = math.sqrt((_VD // VITCFG["num_heads"]) / _VD)                          # 1 / sqrt(dim) = f / sqrt(head_dim); f = 0.5 is exact
    for i in range(_EV):
        for s in ("weight", "bias"):
            k = f"transformer.{i}.attn.to_qkv.{s}"
            w = m.sd[k].clone()
            w[:_VD] *= f
            m.sd[k] = w


_add("clip", "attention scale 1 / sqrt(dim)", _scale_by_dim)
_add("clip", "quick-GELU for GELU", lambda m: m.patch("clip_gelu", lambda x: x * torch.sigmoid(1.702 * x)))
_add("clip", "tanh-GELU for erf-GELU", lambda m: m.patch("clip_gelu", lambda x: F.gelu(x, approximate="tanh")))
_add("clip", "all 3 blocks evaluated", lambda m: m.cfg.__setitem__("evaluated", VITCFG["num_layers"]))
_add("clip", "patch kernel rows and columns swapped", lambda m: m.sd.__setitem__("patch_embedding.weight", m.sd["patch_embedding.weight"].transpose(2, 3).contiguous()))
_add("clip", "patches in column-major order", lambda m: _stem(m, column_major=True))
_add("clip", "channel order reversed", lambda m: m.sd.__setitem__("patch_embedding.weight", m.sd["patch_embedding.weight"].flip(1).contiguous()))
_add("clip", "norm_eps 1e-6 for 1e-5", lambda m: m.cfg.__setitem__("norm_eps", 1e-6))


# ---- the preprocessing of CLIPModel.visual
def _preprocess_variant(m, affine=True, exchanged=False, reversed_=False, mode="bicubic"):
    def clip_preprocess(frames, size=224):
        x = F.interpolate(frames.float(), size=(size, size), mode=mode, align_corners=False)
        if affine:
            x = x * 0.5 + 0.5
        mean = torch.tensor([0.48145466, 0.4578275, 0.40821073]).view(1, 3, 1, 1)
        std = torch.tensor([0.26862954, 0.26130258, 0.27577711]).view(1, 3, 1, 1)
        if exchanged:
            mean, std = std, mean
        if reversed_:
            mean, std = mean.flip(1), std.flip(1)
        return (x - mean) / std
    m.patch("clip_preprocess", clip_preprocess)


_add("pre", "* 0.5 + 0.5 missing", lambda m: _preprocess_variant(m, affine=False))
_add("pre", "mean and std exchanged", lambda m: _preprocess_variant(m, exchanged=True))
_add("pre", "channel order of mean / std reversed", lambda m: _preprocess_variant(m, reversed_=True))
_add("pre", "bilinear for bicubic", lambda m: _preprocess_variant(m, mode="bilinear"))

# Entries that need not reach 4 T_p: name -> what tests/test_enc_wiring_cpu.py asserts instead ("cancels": e(mutant, oracle) <= 1e-5 at
# every point; "below T_p": the mutant's distance is below T_p at every point -- tests/gemm_exact.py owns which GELU an epilogue computes)
EXEMPT: Dict[str, str] = {
    "clip: bias zeroed: to_qkv (k third), block 0": "cancels",          # a per-query constant on the scores: softmax removes it
    "clip: bias zeroed: to_qkv (k third), block 1": "cancels",
    "t5: erf-GELU for tanh-GELU": "below T_p",
    "clip: tanh-GELU for erf-GELU": "below T_p",
}


def tower(name):
    """(config, planted weights, planted inputs, points function, bounds) of "t5" / "clip" """
    if name == "t5":
        return T5CFG, planted_t5(), planted_t5_inputs(), t5_points, t5_bounds()
    return VITCFG, planted_vit(), planted_images(), clip_points, clip_bounds()


def pre_floor() -> float:
    """What fp32 allows the preprocessing: 16 taps of |weight| <= 1.3 on |x| <= 1 accumulated in fp32, then a division by std ~ 0.27,
    against outputs of rms about 1.3: a few units of 2^-24 per element; 2^-21 stands for it."""
    return 2.0 ** -21


def visibility(name):
    """[(entry name, best point, e at it / T_p at it, {point: e})] of every catalogue entry of one tower ("t5", "clip", "pre"): the MUTATED
    fp32 oracle against the unmutated one, in units of the GPU tests' bound.  "pre" is measured against pre_floor()."""
    rows = []
    if name == "pre":
        clip = planted_clip()
        ref = pre_points(clip)
        for c in (c for c in CATALOGUE if c.tower == "pre"):
            with applied(c, {}, {}):
                es = {"pre": e(pre_points(clip)["pre"], ref["pre"])}
            rows.append((c.name, "pre", es["pre"] / pre_floor(), es))
        return rows
    cfg, sd, inp, points, b = tower(name)
    ref = points(cfg, sd, inp)
    for c in (c for c in CATALOGUE if c.tower == name):
        with applied(c, cfg, sd) as (cfg_m, sd_m):
            got = points(cfg_m, sd_m, inp)
        es = {p: e(got[p], ref[p]) for p in ref}
        ratio = {p: (es[p] / b["T"][p] if b["T"][p] else (float("inf") if es[p] else 0.0)) for p in ref}
        best = max(ratio, key=ratio.get)
        rows.append((c.name, best, ratio[best], es))
    return rows
