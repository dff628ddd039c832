"""MI355X-native SCAIL DiT behind the reference's network interface (drop-in seam B1).

``DiffusionTransformer`` has the constructor signature, ``forward`` signature and state_dict
keys of the reference class (dit_video_crossattn_sc_xc.py:1209-1321, :1452-1587; key layout
SURVEY.md Appendix B) so ``network_config.target: scail_amd.dit.DiffusionTransformer`` works with
the reference's yaml and ``load_checkpoint`` unchanged.  The implementation is NOT a SAT
mixin stack: one forward is a fixed sequence of hand-written HIP kernels from libscail_hip.so
(scail_amd.ops); PyTorch only owns the buffers.

What is restructured relative to the reference (results unchanged, SURVEY 8a "observed
inefficiencies"):
  * text_embedding / clip_proj and all 40x text/CLIP K,V projections + their RMSNorms depend only
    on the prompt/image -> computed once per conditioning and cached (reference: every step);
  * RoPE tables are built once per latent shape as (L, 64) pair tables; RMSNorm + RoPE is one
    pass over q and one over k, in place inside the QKV buffer; no head transposes anywhere --
    attention reads (B, L, H, 128) views and writes the (B, L, D) layout the out-proj consumes;
  * LN+modulate, bias+GELU, bias+gate+residual are fused into the producing kernels;
  * the final Linear runs on the noise tokens only (reference: all L, then slices).
"""
from __future__ import annotations

import os

import math
from functools import reduce
from operator import mul
from typing import Dict, Optional

import torch
from torch import nn

from . import lib as L
from . import ops, rope

_STR2DTYPE = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def _get(args, name, default=None):
    if args is None:
        return default
    if isinstance(args, dict):
        return args.get(name, default)
    return getattr(args, name, default)


class _Node(nn.Module):
    """Anonymous container used to reproduce the reference's parameter paths."""


def _register(root: nn.Module, path: str, p: nn.Parameter):
    parts = path.split(".")
    mod = root
    for name in parts[:-1]:
        if name not in mod._modules:
            mod.add_module(name, _Node())
        mod = mod._modules[name]
    mod.register_parameter(parts[-1], p)


def _as_bf16(t: torch.Tensor, dev) -> torch.Tensor:
    """t on ``dev`` as contiguous bf16 (fp32 through the library's own rounding kernel)"""
    t = t.to(dev)
    return ops.to_bf16(t.contiguous()) if t.dtype == torch.float32 else t.to(torch.bfloat16).contiguous()


def _fp8_options(gemm_precision, fp8_gemms):
    """("bf16" | "fp8" | "fp6", SCAIL_DIT_FP8_* mask) from the constructor options: fp8_gemms = None (all six per-token GEMMs), an iterable
    of names from lib.FP8_GEMMS, or the mask itself.  fp8_gemms keeps its name under "fp6": it selects the quantised GEMMs."""
    if gemm_precision != "bf16" and gemm_precision not in L.GEMM_PRECISIONS:
        raise ValueError(f"gemm_precision must be 'bf16', 'fp8' or 'fp6', got {gemm_precision!r}")
    if gemm_precision == "bf16":
        if fp8_gemms is not None:
            raise ValueError("fp8_gemms needs gemm_precision='fp8'")
        return "bf16", 0
    if fp8_gemms is None:
        return gemm_precision, L.FP8_ALL
    if isinstance(fp8_gemms, int) and not isinstance(fp8_gemms, bool):
        mask = fp8_gemms
    else:
        if isinstance(fp8_gemms, str):
            fp8_gemms = [g for g in fp8_gemms.replace(",", " ").split() if g]
        unknown = [g for g in fp8_gemms if g not in L.FP8_GEMMS]
        if unknown:
            raise ValueError(f"fp8_gemms: unknown GEMM(s) {unknown}; choose from {sorted(L.FP8_GEMMS)}")
        mask = sum(L.FP8_GEMMS[g] for g in set(fp8_gemms))
    if not 0 < mask <= L.FP8_ALL:
        raise ValueError(f"fp8_gemms must select at least one of {sorted(L.FP8_GEMMS)} (mask 1..{L.FP8_ALL}), got {fp8_gemms!r}")
    return gemm_precision, mask


def _fp8_scaling_option(fp8_scaling, gemm_precision):
    """The constructor option ``fp8_scaling``: "row" (one fp32 scale per row, the default) or "mx" (OCP MX: one E8M0 scale per block of
    32 along K; include/scail_dit.h SCAIL_DIT_FP8_SCALE_*).  "mx" needs gemm_precision='fp8': the option scales the fp8 GEMMs only (fp6 is
    block-scaled by its format)."""
    if fp8_scaling not in L.FP8_SCALINGS:
        raise ValueError(f"fp8_scaling must be one of {sorted(L.FP8_SCALINGS)}, got {fp8_scaling!r}")
    if fp8_scaling != "row" and gemm_precision != "fp8":
        raise ValueError(f"fp8_scaling={fp8_scaling!r} needs gemm_precision='fp8'")
    return fp8_scaling


def _fp8_layer_options(fp8_layers, num_layers, mask):
    """Per-layer SCAIL_DIT_FP8_* masks from the constructor option ``fp8_layers`` (None: no per-layer selection): one entry per layer,
    each the mask itself (0 = that layer stays bf16) or an iterable / string of names from lib.FP8_GEMMS, and a subset of ``mask``
    (only a GEMM that fp8_gemms quantises can be selected)."""
    if fp8_layers is None:
        return None
    if not mask:
        raise ValueError("fp8_layers needs gemm_precision='fp8'")
    if isinstance(fp8_layers, (str, bytes)) or not hasattr(fp8_layers, "__len__"):
        raise ValueError(f"fp8_layers must be a sequence with one entry per layer, got {fp8_layers!r}")
    if len(fp8_layers) != num_layers:
        raise ValueError(f"fp8_layers needs one entry per layer ({num_layers}), got {len(fp8_layers)}")
    out = []
    for i, e in enumerate(fp8_layers):
        if isinstance(e, int) and not isinstance(e, bool):
            m = e
        else:
            if isinstance(e, (bool, float)) or e is None:
                raise ValueError(f"fp8_layers[{i}]: expected a mask or GEMM names, got {e!r}")
            if isinstance(e, str):
                e = [g for g in e.replace(",", " ").split() if g]
            unknown = [g for g in e if g not in L.FP8_GEMMS]
            if unknown:
                raise ValueError(f"fp8_layers[{i}]: unknown GEMM(s) {unknown}; choose from {sorted(L.FP8_GEMMS)}")
            m = sum(L.FP8_GEMMS[g] for g in set(e))
        if not 0 <= m <= L.FP8_ALL:
            raise ValueError(f"fp8_layers[{i}]: mask must be 0..{L.FP8_ALL}, got {m}")
        if m & ~mask:
            names = [n for n, b in L.FP8_GEMMS.items() if m & ~mask & b]
            raise ValueError(f"fp8_layers[{i}] selects {names}, which fp8_gemms (mask {mask}) does not quantise")
        out.append(m)
    return out


def fp8_rel_err(table):
    """(layers, 6, 4) probe table (include/scail_dit.h scail_dit_fp8_probe) -> ((layers, 6) sqrt(num / den), (layers, 6) sqrt(worst row
    ratio)) as fp64 CPU tensors.  den == 0: 0 when num == 0 too (nothing there, nothing lost), +inf otherwise."""
    t = torch.as_tensor(table, dtype=torch.float64).cpu()
    if t.dim() != 3 or t.shape[1:] != (6, 4):
        raise ValueError(f"probe table must be (layers, 6, 4), got {tuple(t.shape)}")
    num, den = t[..., 0], t[..., 1]
    q = torch.where(den == 0, torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, float("inf"))), num / den)
    return torch.sqrt(q), torch.sqrt(t[..., 2])


def choose_fp8_layers(rel_err, max_rel_err, enabled_mask):
    """Per-layer fp8 masks from a probe result: GEMM g of layer i stays fp8 iff bit g of ``enabled_mask`` is set and its relative error
    is finite and <= ``max_rel_err``.  ``rel_err``: (layers, 6) values sqrt(num / den) -- or the raw (layers, 6, 4) table, read with
    fp8_rel_err (num == den == 0 counts as 0).  NaN and inf never pass.  Pure: no device, no network."""
    r = torch.as_tensor(rel_err, dtype=torch.float64).cpu()
    if r.dim() == 3:
        r = fp8_rel_err(r)[0]
    if r.dim() != 2 or r.shape[1] != 6:
        raise ValueError(f"rel_err must be (layers, 6) or (layers, 6, 4), got {tuple(r.shape)}")
    max_rel_err = float(max_rel_err)
    if not max_rel_err >= 0.0:
        raise ValueError(f"max_rel_err must be a number >= 0, got {max_rel_err}")
    if isinstance(enabled_mask, bool) or not isinstance(enabled_mask, int) or not 0 <= enabled_mask <= L.FP8_ALL:
        raise ValueError(f"enabled_mask must be 0..{L.FP8_ALL}, got {enabled_mask!r}")
    keep = torch.isfinite(r) & (r <= max_rel_err)
    return [sum(1 << g for g in range(6) if (enabled_mask >> g) & 1 and bool(keep[i, g])) for i in range(r.shape[0])]


class DiffusionTransformer(nn.Module):
    """Reference-compatible network object; see module docstring."""

    def __init__(self, transformer_args=None, num_frames=81, time_compressed_rate=4, latent_width=300,
                 latent_height=300, patch_size=(1, 2, 2), in_channels=20, out_channels=16, hidden_size=5120,
                 text_dim=4096, num_layers=40, num_attention_heads=40, elementwise_affine=False,
                 num_multi_query_heads=0, cross_num_multi_query_heads=0, time_freq_dim=None, time_embed_dim=None,
                 num_classes=None, modules=None, input_time="adaln", share_adaln=False, adm_in_channels=None,
                 parallel_output=True, height_interpolation=1.0, width_interpolation=1.0, time_interpolation=1.0,
                 use_SwiGLU=False, use_RMSNorm=False, cfg_embed_dim=None, ofs_embed_dim=None,
                 layernorm_epsilon=1e-6, inner_hidden_size=None, use_i2v_clip=False, dtype="bf16",
                 device=None, init_seed=1234, gemm_precision="bf16", fp8_gemms=None, fp8_layers=None, fp8_scaling="row", **kwargs):
        super().__init__()
        # ---- options of the reference class this engine does not implement: fail loudly ----
        unsupported = []
        if use_SwiGLU: unsupported.append("use_SwiGLU (shipped configs use the non-gated GELU-tanh MLP)")
        if use_RMSNorm: unsupported.append("use_RMSNorm")
        if not share_adaln: unsupported.append("share_adaln=False")
        if elementwise_affine: unsupported.append("elementwise_affine=True")
        if num_classes is not None: unsupported.append("num_classes")
        if cfg_embed_dim is not None or ofs_embed_dim is not None: unsupported.append("cfg/ofs embeddings")
        if num_multi_query_heads or cross_num_multi_query_heads: unsupported.append("multi-query heads")
        if input_time != "adaln": unsupported.append(f"input_time={input_time}")
        if not use_i2v_clip: unsupported.append("use_i2v_clip=False")
        if _get(transformer_args, "model_parallel_size", 1) != 1: unsupported.append("model_parallel_size>1")
        if unsupported:
            raise NotImplementedError("scail_amd.DiffusionTransformer: unsupported options: " + "; ".join(unsupported))
        modules = modules or {}
        pe = (modules.get("pos_embed_config") or {}).get("params", {})
        al = (modules.get("adaln_layer_config") or {}).get("params", {})
        if pe and not pe.get("interleaved_rope", False):
            raise NotImplementedError("only interleaved_rope=True is implemented (shipped configs)")
        self.hidden_size = hidden_size
        self.num_layers = num_layers
        self.num_attention_heads = num_attention_heads
        self.head_dim = hidden_size // num_attention_heads
        if self.head_dim != 128 or pe.get("hidden_size_head", 128) != 128:
            raise NotImplementedError("the HIP attention kernel is specialised for head_dim 128 (both shipped configs)")
        if al.get("hidden_size_head", hidden_size) != hidden_size or not al.get("qk_ln", True):
            raise NotImplementedError("q/k RMSNorm must span the full hidden size (hidden_size_head == hidden_size)")
        self.patch_size = tuple(patch_size)
        if self.patch_size != (1, 2, 2) or in_channels != 20 or out_channels != 16:
            raise NotImplementedError("patch (1,2,2), 20 input / 16 output channels only")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.text_dim = text_dim
        self.inner_hidden_size = inner_hidden_size if inner_hidden_size is not None else 4 * hidden_size
        self.time_embed_dim = time_embed_dim if time_embed_dim is not None else hidden_size
        self.time_freq_dim = time_freq_dim if time_freq_dim is not None else self.time_embed_dim
        if self.time_embed_dim != hidden_size:
            raise NotImplementedError("final layer adds emb to a (1,2,D) table: time_embed_dim must equal hidden_size")
        self.layernorm_epsilon = layernorm_epsilon
        self.latent_width, self.latent_height = latent_width, latent_height
        self.num_frames, self.time_compressed_rate = num_frames, time_compressed_rate
        self.use_i2v_clip = use_i2v_clip
        self.clip_dim = 1280
        self.global_rope_H, self.global_rope_W = 0, 120          # reference :1570-1571
        self.dtype = _STR2DTYPE.get(dtype, dtype) if isinstance(dtype, str) else dtype
        if self.dtype != torch.bfloat16:
            raise NotImplementedError("the MI355X engine computes in bf16 (reference yaml: bf16: True)")
        for nm, mult in (("hidden_size", 64), ("inner_hidden_size", 64), ("text_dim", 64)):
            if getattr(self, nm) % mult:
                raise NotImplementedError(f"{nm} must be a multiple of {mult}")
        # opt-in fp8 (e4m3) or fp6 (MXFP6 e2m3) per-token GEMMs (include/scail_dit.h scail_dit_enable_fp8 / _fp6); a yaml sets them through
        # network_config.params
        self.gemm_precision, self.fp8_mask = _fp8_options(gemm_precision, fp8_gemms)
        self.fp8_scaling = _fp8_scaling_option(fp8_scaling, self.gemm_precision)
        # fp8_layers: which of those GEMMs stay fp8 in each layer (scail_dit_fp8_select_layers); None = all of them in every layer
        self.fp8_layer_masks = _fp8_layer_options(fp8_layers, num_layers, self.fp8_mask)
        self.fp8_probe_table = None        # the raw (layers, 6, 4) table of the last fp8_probe()
        if self.fp8_mask:
            D, FF = self.hidden_size, self.inner_hidden_size
            for name, (n, k) in (("qkv", (3 * D, D)), ("o", (D, D)), ("cq", (D, D)), ("co", (D, D)), ("w1", (FF, D)), ("w2", (D, FF))):
                if self.fp8_mask & L.FP8_GEMMS[name] and (n % 128 or k % 128):
                    raise NotImplementedError(f"{self.gemm_precision} GEMM {name} ({n} x {k}): the {self.gemm_precision} kernel needs N and K multiples of 128")
        self._build_params(device, init_seed)
        self._prepared: Optional[Dict] = None
        self._cond_cache = None
        self._rope_cache: Dict = {}
        self._ws: Dict = {}
        self.cache_conditioning = True
        self.sp = None                     # scail_amd.parallel.SequenceParallel or None
        self._tap = None                   # debug/test hook: called as _tap(layer_index, hidden_states)
        self.kernel_timer = None           # bench hook: object with .run(tag, fn, *a, **k) bracketing fn with HIP events
        # one C call per network evaluation (include/scail_dit.h) instead of ~25 ctypes calls per layer; env override
        self.use_c_step = os.environ.get("SCAIL_C_STEP", "1") != "0"
        self._cstep = None
        self.loras = []                    # (adapter name or "<dict>", strength, entries) of every merge_lora, in order
        self._c_blocks = False             # test hook: drive the executor block by block (scail_dit_block per layer, the rest from the host): cross-check of the one-call step

    # ------------------------------------------------------------------------------------------
    # parameters (reference names / shapes)
    # ------------------------------------------------------------------------------------------
    def param_spec(self) -> Dict[str, tuple]:
        D, FF, Dt = self.hidden_size, self.inner_hidden_size, self.time_embed_dim
        s: Dict[str, tuple] = {}
        s["mixins.patch_embed.proj.weight"] = (D, 20, 1, 2, 2)
        s["mixins.patch_embed.proj.bias"] = (D,)
        s["mixins.patch_embed.proj_pose.weight"] = (D, 20, 1, 2, 2)
        s["mixins.patch_embed.proj_pose.bias"] = (D,)
        for i in range(self.num_layers):
            s[f"mixins.adaln_layer.adaLN_modulations.{i}"] = (1, 6, D)
        for nm in ("query", "key", "cross_query", "cross_key", "clip_feature_key"):
            for i in range(self.num_layers):
                s[f"mixins.adaln_layer.{nm}_layernorm_list.{i}.weight"] = (D,)
        for i in range(self.num_layers):
            s[f"mixins.adaln_layer.clip_feature_key_value_list.{i}.weight"] = (2 * D, D)
            s[f"mixins.adaln_layer.clip_feature_key_value_list.{i}.bias"] = (2 * D,)
        s["mixins.final_layer.adaLN_modulation"] = (1, 2, D)
        s["mixins.final_layer.linear.weight"] = (64, D)
        s["mixins.final_layer.linear.bias"] = (64,)
        for i in range(self.num_layers):
            p = f"transformer.layers.{i}."
            s[p + "attention.query_key_value.weight"] = (3 * D, D)
            s[p + "attention.query_key_value.bias"] = (3 * D,)
            s[p + "attention.dense.weight"] = (D, D)
            s[p + "attention.dense.bias"] = (D,)
            s[p + "cross_attention.query.weight"] = (D, D)
            s[p + "cross_attention.query.bias"] = (D,)
            s[p + "cross_attention.key_value.weight"] = (2 * D, D)
            s[p + "cross_attention.key_value.bias"] = (2 * D,)
            s[p + "cross_attention.dense.weight"] = (D, D)
            s[p + "cross_attention.dense.bias"] = (D,)
            s[p + "post_cross_attention_layernorm.weight"] = (D,)
            s[p + "post_cross_attention_layernorm.bias"] = (D,)
            s[p + "mlp.dense_h_to_4h.weight"] = (FF, D)
            s[p + "mlp.dense_h_to_4h.bias"] = (FF,)
            s[p + "mlp.dense_4h_to_h.weight"] = (D, FF)
            s[p + "mlp.dense_4h_to_h.bias"] = (D,)
        s["time_embed.0.weight"] = (Dt, self.time_freq_dim)
        s["time_embed.0.bias"] = (Dt,)
        s["time_embed.2.weight"] = (Dt, Dt)
        s["time_embed.2.bias"] = (Dt,)
        s["adaln_projection.1.weight"] = (6 * D, Dt)
        s["adaln_projection.1.bias"] = (6 * D,)
        s["text_embedding.0.weight"] = (D, self.text_dim)
        s["text_embedding.0.bias"] = (D,)
        s["text_embedding.2.weight"] = (D, D)
        s["text_embedding.2.bias"] = (D,)
        C = self.clip_dim
        s["clip_proj.proj.0.weight"] = (C,)
        s["clip_proj.proj.0.bias"] = (C,)
        s["clip_proj.proj.1.weight"] = (C, C)
        s["clip_proj.proj.1.bias"] = (C,)
        s["clip_proj.proj.3.weight"] = (D, C)
        s["clip_proj.proj.3.bias"] = (D,)
        s["clip_proj.proj.4.weight"] = (D,)
        s["clip_proj.proj.4.bias"] = (D,)
        return s

    def _build_params(self, device, seed):
        """Random init in the spirit of the reference (N(0,0.02) linears sat/mpu/utils.py:89-94, zero
        biases, unit norm weights, randn/sqrt(D) AdaLN tables dit...:888-893,814-816), generated
        directly in bf16 on ``device`` so a 14B model never exists in fp32 on the host."""
        if seed is None:
            # init_seed=None: shapes only (meta tensors); the caller attaches real storage with
            # load_state_dict(sd, assign=True) -- e.g. the parameters of a live reference network (scail_amd/sat_mixins.py)
            for name, shape in self.param_spec().items():
                _register(self, name, nn.Parameter(torch.empty(shape, device="meta", dtype=self.dtype), requires_grad=False))
            return
        dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        g = torch.Generator(device=dev).manual_seed(seed)
        D = self.hidden_size
        for name, shape in self.param_spec().items():
            if "adaLN_modulation" in name:
                w = torch.randn(shape, generator=g, device=dev, dtype=torch.float32) / math.sqrt(D)
            elif ("layernorm" in name and name.endswith("weight")) or name in ("clip_proj.proj.0.weight", "clip_proj.proj.4.weight"):
                w = torch.ones(shape, device=dev, dtype=torch.float32)
            elif name.endswith("bias"):
                w = torch.zeros(shape, device=dev, dtype=torch.float32)
            elif "patch_embed" in name or "final_layer.linear" in name:
                fan_in = reduce(mul, shape[1:])
                w = torch.randn(shape, generator=g, device=dev, dtype=torch.float32) / math.sqrt(fan_in)
            else:
                w = torch.randn(shape, generator=g, device=dev, dtype=torch.bfloat16) * 0.02
            _register(self, name, nn.Parameter(w.to(self.dtype), requires_grad=False))

    def _load_from_state_dict(self, *a, **k):
        self._prepared = None
        self._cond_cache = None
        return super()._load_from_state_dict(*a, **k)

    def load_state_dict(self, *a, **k):
        self._prepared = None
        self._cond_cache = None
        return super().load_state_dict(*a, **k)

    def weights_changed(self):
        """Drop everything derived from the parameters' VALUES, after they were changed in place (merge_lora): the prepared arena (fp32
        copies of the vectors and tables, the padded patch matrices), the conditioning cache (K / V projected through the old weights)
        and the executor, and with it the fp8 / MX / fp6 weight buffers, the probe state and every cache the binding owns.  The next
        call rebuilds them.  The per-layer fp8 selection (fp8_layer_masks) is the caller's choice and stays; the probe table it may
        have come from measured the old weights and goes.  (scail_amd/sat_mixins.py HipBackend compares its executor's arena with
        prepare() and follows.)"""
        self._prepared = None
        self._cond_cache = None
        self._cstep = None
        self.fp8_probe_table = None

    @torch.no_grad()
    def merge_lora(self, adapter, strength=1.0):
        """Merge a LoRA adapter into the weights, on the GPU and in place (an extension, opt-in; scail_amd/lora.py has the arithmetic, the
        key conventions and what is not known about them).  ``adapter``: a path (.safetensors or torch.load-able) or a dict of tensors.
        The adapter is validated whole before any weight is touched (ValueError naming the key); parameters without storage (init_seed=None
        before load_state_dict(assign=True)) or off the GPU are refused by name.  Returns the plan's summary rows (lora.summary) and
        appends (name or "<dict>", strength, entries) to ``self.loras``.  Adapters stack; the result depends on their order in the last
        bf16 bit.  There is no un-merge -- merge_lora(adapter, -strength) is not the inverse in bits (two bf16 roundings): load the
        checkpoint again.  Sequence-parallel ranks hold replicated weights: every rank merges the same file."""
        from . import lora
        tensors = adapter if isinstance(adapter, dict) else lora.read_adapter(adapter)
        plan = lora.plan_adapter(self, tensors, strength)
        lora.apply_plan(self, plan)
        self.loras.append(("<dict>" if isinstance(adapter, dict) else str(adapter), float(strength), len(plan)))
        return lora.summary(plan)

    # ------------------------------------------------------------------------------------------
    # weight arena for the kernels
    # ------------------------------------------------------------------------------------------
    def prepare(self):
        """Device-side views/copies the kernels consume: big matrices are the bf16 parameters
        themselves (no copy); per-channel vectors are upcast once to fp32 (exact)."""
        if self._prepared is not None:
            return self._prepared
        sd = dict(self.named_parameters())
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise L.ScailHipError("scail_amd.DiffusionTransformer must live on the GPU (no CPU path); call .cuda()")
        L.load()

        def mat(n):
            return sd[n].detach().to(torch.bfloat16).contiguous()

        def vec(n):
            return sd[n].detach().float().contiguous()

        D = self.hidden_size
        W = {}
        for nm, key in (("patch", "proj"), ("pose", "proj_pose")):
            w = sd[f"mixins.patch_embed.{key}.weight"].detach().to(torch.bfloat16).reshape(D, 80)
            wp = torch.zeros(D, 128, device=dev, dtype=torch.bfloat16)
            wp[:, :80] = w
            W[nm + "_w"] = wp
            W[nm + "_b"] = vec(f"mixins.patch_embed.{key}.bias")
        W["adaln_tables"] = torch.stack([vec(f"mixins.adaln_layer.adaLN_modulations.{i}").reshape(6 * D)
                                         for i in range(self.num_layers)]).contiguous()
        W["final_table"] = vec("mixins.final_layer.adaLN_modulation").reshape(1, 2 * D).contiguous()
        W["final_w"], W["final_b"] = mat("mixins.final_layer.linear.weight"), vec("mixins.final_layer.linear.bias")
        for k in ("time_embed.0", "time_embed.2", "adaln_projection.1", "text_embedding.0", "text_embedding.2",
                  "clip_proj.proj.1", "clip_proj.proj.3"):
            W[k + ".w"], W[k + ".b"] = mat(k + ".weight"), vec(k + ".bias")
        for k in ("clip_proj.proj.0", "clip_proj.proj.4"):
            W[k + ".w"], W[k + ".b"] = vec(k + ".weight"), vec(k + ".bias")
        layers = []
        for i in range(self.num_layers):
            p = f"transformer.layers.{i}."
            m = "mixins.adaln_layer."
            lw = dict(
                qkv_w=mat(p + "attention.query_key_value.weight"), qkv_b=vec(p + "attention.query_key_value.bias"),
                o_w=mat(p + "attention.dense.weight"), o_b=vec(p + "attention.dense.bias"),
                qn=vec(m + f"query_layernorm_list.{i}.weight"), kn=vec(m + f"key_layernorm_list.{i}.weight"),
                cq_w=mat(p + "cross_attention.query.weight"), cq_b=vec(p + "cross_attention.query.bias"),
                ckv_w=mat(p + "cross_attention.key_value.weight"), ckv_b=vec(p + "cross_attention.key_value.bias"),
                co_w=mat(p + "cross_attention.dense.weight"), co_b=vec(p + "cross_attention.dense.bias"),
                cqn=vec(m + f"cross_query_layernorm_list.{i}.weight"), ckn=vec(m + f"cross_key_layernorm_list.{i}.weight"),
                clipkn=vec(m + f"clip_feature_key_layernorm_list.{i}.weight"),
                clipkv_w=mat(m + f"clip_feature_key_value_list.{i}.weight"), clipkv_b=vec(m + f"clip_feature_key_value_list.{i}.bias"),
                ln_w=vec(p + "post_cross_attention_layernorm.weight"), ln_b=vec(p + "post_cross_attention_layernorm.bias"),
                w1=mat(p + "mlp.dense_h_to_4h.weight"), b1=vec(p + "mlp.dense_h_to_4h.bias"),
                w2=mat(p + "mlp.dense_4h_to_h.weight"), b2=vec(p + "mlp.dense_4h_to_h.bias"),
            )
            layers.append(lw)
        W["layers"] = layers
        self._prepared = W
        self._cstep = None                 # pointer tables of a previous prepare() are stale
        return W

    # ------------------------------------------------------------------------------------------
    # step-invariant conditioning (text / CLIP keys and values for all layers)
    # ------------------------------------------------------------------------------------------
    def _conditioning(self, ctx: torch.Tensor, clip: torch.Tensor, cond_key=None):
        """ctx (B, Lt, text_dim) bf16, clip (Bc, Lc, 1280) bf16.  Reference: dit...:1505-1515
        (text_embedding, clip_proj) and :1116-1142 (per-layer K,V projections + RMSNorm)."""
        c = self._cond_cache
        if self.cache_conditioning and c is not None:
            if cond_key is not None and c.get("key") == cond_key:
                return c
            if cond_key is None and "ctx" in c and c["ctx"].shape == ctx.shape and c["clip"].shape == clip.shape \
                    and torch.equal(c["ctx"], ctx) and torch.equal(c["clip"], clip):
                return c
        W = self.prepare()
        text = ops.gemm(ctx, W["text_embedding.0.w"], W["text_embedding.0.b"], epilogue=L.EPI_GELU_TANH)
        text = ops.gemm(text, W["text_embedding.2.w"], W["text_embedding.2.b"])
        cl = ops.layernorm_affine(clip, W["clip_proj.proj.0.w"], W["clip_proj.proj.0.b"], eps=1e-5)
        cl = ops.gemm(cl, W["clip_proj.proj.1.w"], W["clip_proj.proj.1.b"], epilogue=L.EPI_GELU_ERF)
        cl = ops.gemm(cl, W["clip_proj.proj.3.w"], W["clip_proj.proj.3.b"])
        cl = ops.layernorm_affine(cl, W["clip_proj.proj.4.w"], W["clip_proj.proj.4.b"], eps=1e-5)
        c = self.kv_conditioning(text, cl)
        c["key"] = cond_key
        if self.cache_conditioning:
            if cond_key is None:
                c["ctx"], c["clip"] = ctx.clone(), clip.clone()
            self._cond_cache = c
        return c

    def kv_conditioning(self, text: torch.Tensor, cl: torch.Tensor) -> Dict:
        """Per-layer cross-attention keys (post-RMSNorm) and transposed values from the EMBEDDED conditioning: text
        (B, Lt, D) = text_embedding(context), cl (Bc, Lc, D) = clip_proj(image_clip_features), both bf16 -- what the
        reference hands every layer as ``encoder_outputs`` / ``image_clip_features`` (dit...:1505-1515, 1116-1142).
        Also the entry the SAT block seam uses (scail_amd/sat_mixins.py), where the reference's own modules embed."""
        W = self.prepare()
        D, H = self.hidden_size, self.num_attention_heads
        B, Lt, _ = text.shape
        Bc, Lc, _ = cl.shape
        dev = text.device
        Ltp, Lcp = (Lt + 63) // 64 * 64, (Lc + 63) // 64 * 64
        nl = self.num_layers
        k_text = torch.empty(nl, B, Lt, D, device=dev, dtype=torch.bfloat16)
        vt_text = torch.empty(nl, B, H, 128, Ltp, device=dev, dtype=torch.bfloat16)
        k_clip = torch.empty(nl, Bc, Lc, D, device=dev, dtype=torch.bfloat16)
        vt_clip = torch.empty(nl, Bc, H, 128, Lcp, device=dev, dtype=torch.bfloat16)
        kv = torch.empty(B, Lt, 2 * D, device=dev, dtype=torch.bfloat16)
        kvc = torch.empty(Bc, Lc, 2 * D, device=dev, dtype=torch.bfloat16)
        for i, lw in enumerate(W["layers"]):
            ops.gemm(text, lw["ckv_w"], lw["ckv_b"], out=kv)
            ops.rmsnorm_rope(kv[..., :D], lw["ckn"], out=k_text[i], eps=self.layernorm_epsilon)
            ops.transpose_v(kv[..., D:], H, out=vt_text[i])
            ops.gemm(cl, lw["clipkv_w"], lw["clipkv_b"], out=kvc)
            ops.rmsnorm_rope(kvc[..., :D], lw["clipkn"], out=k_clip[i], eps=self.layernorm_epsilon)
            ops.transpose_v(kvc[..., D:], H, out=vt_clip[i])
        return dict(k_text=k_text, vt_text=vt_text, k_clip=k_clip, vt_clip=vt_clip)

    def _timed(self, tag, fn, *a, **k):
        if self.kernel_timer is None:
            return fn(*a, **k)
        return self.kernel_timer.run(tag, fn, *a, **k)

    def _rope(self, T, Hp, Wp, H_shift, W_shift, device, n_char=1):
        key = (T, Hp, Wp, H_shift, W_shift, n_char)
        if key not in self._rope_cache:
            mt = (self.num_frames - 1) // self.time_compressed_rate + 1
            cos, sin = rope.build_tables(self.head_dim, T, Hp, Wp, H_shift, W_shift, self.global_rope_H,
                                         self.global_rope_W, max_T=mt, max_H=self.latent_height // 2,
                                         max_W=self.latent_width // 2 + 120, n_char=n_char)
            self._rope_cache[key] = (cos.to(device), sin.to(device))
        return self._rope_cache[key]

    def _workspace(self, B, Ltok, Lnoise, device, blocks_in_c=False):
        """Activation scratch of the per-op path.  blocks_in_c (the _c_blocks cross-check: every block is one executor call with the
        executor's own block workspace): only the buffers the host-side assembly and the final layer touch."""
        key = (B, Ltok, Lnoise, blocks_in_c)
        ws = self._ws.get(key)
        if ws is None:
            D, FF, H = self.hidden_size, self.inner_hidden_size, self.num_attention_heads
            e = lambda *s: torch.empty(*s, device=device, dtype=torch.bfloat16)
            Lp = (Ltok + 63) // 64 * 64
            ws = dict(tok=e(B, Ltok, 128), h=e(B, Ltok, D), xf=e(B, Lnoise, D), tokout=e(B, Lnoise, 64))
            if blocks_in_c:
                ws.update(xn=None, qkv=None, att=None, ff=None, vt=None)
            else:
                ws.update(xn=e(B, Ltok, D), qkv=e(B, Ltok, 3 * D), att=e(B, Ltok, D), ff=e(B, Ltok, FF), vt=e(B, H, 128, Lp))
            self._ws = {key: ws}          # keep one shape resident
        return ws

    # ------------------------------------------------------------------------------------------
    # forward
    # ------------------------------------------------------------------------------------------
    def forward(self, x, timesteps=None, context=None, y=None, **kwargs):
        """Reference signature (dit...:1452).  x (B,T,16,H,W); timesteps (B,); context (B,Lt,text_dim);
        kwargs: concat_images (only gates the branch, :1457), ref_concat, concat_smpl_render,
        image_clip_features, chunk_dim (sequence parallel), cfg_scale (ignored like the reference).
        Returns (B,T,16,H,W) in the model dtype (bf16)."""
        v = self.forward_f32(x, timesteps, context, y, **kwargs)
        return ops.to_bf16(v)

    def forward_f32(self, x, timesteps=None, context=None, y=None, cond_key=None, **kwargs):
        if kwargs.get("ref_concat", None) is None:
            raise AssertionError("must specify ref_concat")                       # reference :1456
        if kwargs.get("concat_images", None) is None:
            raise NotImplementedError("the reference only builds the 20-channel input when concat_images is given (:1457)")
        if y is not None:
            raise AssertionError("must specify y if and only if the model is class-conditional")  # :1517
        if kwargs.get("concat_smpl_render", None) is None or kwargs.get("image_clip_features", None) is None:
            raise AssertionError("concat_smpl_render and image_clip_features are required (use_pose / use_i2v_clip)")
        dev = x.device
        if dev.type != "cuda":
            raise L.ScailHipError("scail_amd.DiffusionTransformer.forward needs GPU tensors (no CPU path)")
        x32 = x.float().contiguous() if x.dtype != torch.float32 else x.contiguous()
        t32 = timesteps.to(dev).float().contiguous()
        ctx, ref, pose, clip = (_as_bf16(t, dev) for t in (context, kwargs["ref_concat"], kwargs["concat_smpl_render"],
                                                           kwargs["image_clip_features"]))
        B, T, C, H, Wd = x32.shape
        H_shift = W_shift = 0
        chunk_dim = kwargs.get("chunk_dim", None)
        if chunk_dim is not None and self.sp is not None and self.sp.size > 1:   # reference :1578-1585
            if chunk_dim == 3:
                H_shift = self.sp.rank * (H // 2)
            elif chunk_dim == 4:
                W_shift = self.sp.rank * (Wd // 2)
            else:
                raise NotImplementedError
        # cfg_pair (set by scail_amd.sampler.VanillaCFG.prepare_inputs): x / timesteps are one latent twice, only the conditioning differs
        cfg_pair = bool(kwargs.get("cfg_pair", False)) and B == 2 and ref.shape[0] == 1 and pose.shape[0] == 1
        if cfg_pair and (not getattr(self, "_cfg_pair_checked", False) or os.environ.get("SCAIL_CHECK_CFG_PAIR") == "1"):
            # the flag is a statement about the inputs (include/scail_dit.h): element 1 receives element 0's layer-0 self-attention.  It is
            # verified the FIRST time a network object sees it (a guider / denoiser that sets the key without duplicating x and sigma does so
            # on every call) and on every call under SCAIL_CHECK_CFG_PAIR=1 -- one host synchronisation each.
            if not (torch.equal(x32[0], x32[1]) and bool(t32[0] == t32[1])):
                raise ValueError("cfg_pair was passed, but x[0] != x[1] or timesteps[0] != timesteps[1]: the flag states that the batch is ONE latent and "
                                 "ONE sigma twice (scail_amd.sampler.VanillaCFG.prepare_inputs); drop the key for any other batch")
            self._cfg_pair_checked = True
        return self._run(x32, t32, ctx, ref, pose, clip, H_shift, W_shift, cond_key, cfg_pair=cfg_pair, step_cache=kwargs.get("step_cache", None))

    def _step_cache_ok(self, what="step_cache"):
        """The step cache lives in the one-call C executor on one rank (include/scail_dit.h "step cache": no *_cached form of the
        sequence-parallel calls or of the per-block seam; the tiled loop has one, sample_tiled_c): everything else is refused by name"""
        if not self.executor_ok(whole_loop=True) or self._c_blocks:
            raise NotImplementedError(f"{what} runs in the C executor's one-call step on a single rank only: not on sequence-parallel ranks, not "
                                      "with SCAIL_C_STEP=0, _tap, kernel_timer or the per-block seam")

    def time_distances(self, timesteps, signal="time"):
        """The decision signal of the step cache (CStep.time_distances): (n, 2) fp64 CPU table for the host schedule ``timesteps`` (n,)
        fp32 (= 1000 sigma_i); feed it to sampler.plan_step_cache."""
        self._step_cache_ok("step_cache (time_distances)")
        dev = self.prepare()["patch_w"].device
        return self._executor().time_distances(timesteps.float().to(dev).contiguous(), signal)

    def executor_ok(self, whole_loop: bool = False) -> bool:
        """Whether the C executor (include/scail_dit.h) may run a request: C step on, no tap, no kernel timer (both instrument the per-op
        path) and, for the calls that hold a whole sampler loop (``whole_loop``: sample_c / sample_tiled_c), one rank."""
        return bool(self.use_c_step and self._tap is None and self.kernel_timer is None
                    and not (whole_loop and self.sp is not None and self.sp.size > 1))

    def _executor(self):
        if self._cstep is None:
            from .cstep import CStep
            self._cstep = CStep(self, self.prepare())
        return self._cstep

    def select_fp8_layers(self, masks):
        """Set (or, with None, drop) the per-layer fp8 selection: ``masks`` as the constructor option ``fp8_layers``."""
        self.fp8_layer_masks = _fp8_layer_options(masks, self.num_layers, self.fp8_mask)
        if self._cstep is not None:
            self._cstep.select_fp8_layers(self.fp8_layer_masks)

    @torch.no_grad()
    def fp8_probe(self, x, timesteps=None, context=None, y=None, **kwargs):
        """One forward (arguments of ``forward_f32``) with the executor's fp8 probe on: every GEMM that fp8_gemms quantises is evaluated in
        bf16 and in fp8 on the same, clean, bf16 activations and the difference of the two bias-only results is summed on the device
        (include/scail_dit.h scail_dit_fp8_probe).  Returns (rel_err, worst): (layers, 6) fp64 CPU tensors, columns in lib.FP8_GEMMS order,
        rel_err = sqrt(sum |y8 - y16|^2 / sum |y16|^2) and worst = the same for the worst token row; GEMMs that are not quantised read 0.
        The raw table stays in ``fp8_probe_table``.  The forward itself runs in bf16 and its result is dropped; one host synchronisation."""
        if not self.fp8_mask:
            raise ValueError("fp8_probe needs gemm_precision='fp8' (it compares the quantised GEMMs with their bf16 twins)")
        if not self.executor_ok() or (self.sp is not None and self.sp.size > 1):
            raise NotImplementedError("fp8_probe runs in the C executor on a single rank only (not with SCAIL_C_STEP=0, _tap, kernel_timer, "
                                      "sequence-parallel ranks)")
        ref = kwargs.get("ref_concat", None)
        if ref is None:
            raise AssertionError("must specify ref_concat")
        B, T, _, H, Wd = x.shape
        n_char = ref.shape[1]
        Ltok = (n_char + T) * (H // 2) * (Wd // 2) + n_char * T * (H // 4) * (Wd // 4)
        ex = self._executor()
        table = ex.fp8_probe_on(B, Ltok, x.device)
        try:
            self.forward_f32(x, timesteps, context, y, **kwargs)
        finally:
            ex.fp8_probe_off()
        self.fp8_probe_table = table.cpu()
        return fp8_rel_err(self.fp8_probe_table)

    def _check_chars(self, n_char, T, pose_frames):
        if pose_frames != n_char * T:
            raise L.ScailHipError(f"concat_smpl_render needs {n_char} x {T} frames for {n_char} reference frame(s), got {pose_frames}")

    def _sample_prelude(self, x32, ctx, clip, cond_key, T_rope, n_char):
        """What the one-call samplers share: (executor, conditioning, RoPE tables of a T_rope-frame clip, the fp32 latent the call updates)"""
        dev = x32.device
        cond = self._conditioning(_as_bf16(ctx, dev), _as_bf16(clip, dev), cond_key)
        cos, sin = self._rope(T_rope, x32.shape[3] // 2, x32.shape[4] // 2, 0, 0, dev, n_char)
        return self._executor(), cond, cos, sin, x32.float().contiguous().clone()

    def sample_c(self, x32, sigmas, cfg_scale, ctx, ref, pose, clip, cond_key=None, reuse=None, guide=None, solver=None):
        """The whole RFSampler Euler loop as ONE C call (scail_dit_sample_chars, include/scail_dit.h): x32 (1,T,16,H,W) fp32,
        ctx (2, Lt, text_dim) = [uncond; cond], ref (1,C,16,H,W), pose (1,C*T,16,H/2,W/2) for C >= 1 characters (C = ref.shape[1]),
        clip (1,Lc,1280).  Single rank.  ``reuse``: None, or the step cache's plan -- one 0 / 1 per step, 1 = reuse the block residual
        of the last computed step (scail_dit_sample_cached).  ``guide``: None, or the guidance plan -- one lib.GUIDE_* entry per step
        (sampler.plan_guidance; scail_dit_sample_guided), alone or together with ``reuse``.  ``solver``: None, or the solver plan
        (sigma, coef) -- the steps' starting sigmas and one (a, b, c) per step (sampler.plan_solver; scail_dit_sample_solver) --, which
        goes with neither ``reuse`` nor ``guide``."""
        T, n_char, dev = x32.shape[1], ref.shape[1], x32.device
        self._check_chars(n_char, T, pose.shape[1])
        if solver is not None and (reuse is not None or guide is not None):
            raise NotImplementedError("a solver plan together with the step cache or the guidance plan is out of scope (include/scail_dit.h "
                                      "\"solver plan\")")
        if reuse is not None:
            self._step_cache_ok()
        if guide is not None:
            self._step_cache_ok("guidance")
        ex, cond, cos, sin, x = self._sample_prelude(x32, ctx, clip, cond_key, T, n_char)
        if solver is not None:
            return ex.sample(x, sigmas, cfg_scale, cond, _as_bf16(ref, dev), _as_bf16(pose, dev), cos, sin, n_char=n_char, solver=solver)
        if guide is not None:
            return ex.sample_guided(x, sigmas, cfg_scale, cond, _as_bf16(ref, dev), _as_bf16(pose, dev), cos, sin, guide, reuse=reuse, n_char=n_char)
        if reuse is not None:
            return ex.sample_cached(x, sigmas, cfg_scale, cond, _as_bf16(ref, dev), _as_bf16(pose, dev), cos, sin, reuse, n_char=n_char)
        return ex.sample(x, sigmas, cfg_scale, cond, _as_bf16(ref, dev), _as_bf16(pose, dev), cos, sin, n_char=n_char)

    def sample_tiled_c(self, x32, sigmas, cfg_scale, ctx, ref, pose_tiles, clip, tile_indices, tile_w, inv_wsum, cond_key=None, reuse=None,
                       solver=None):
        """The whole RFSamplerLong loop (temporal tiling) as ONE C call (scail_dit_sample_tiled, include/scail_dit.h): x32 (1,T,16,H,W) fp32,
        ctx (2, Lt, text_dim) = [uncond; cond], ref (1,1,16,H,W), pose_tiles (1, n_tiles, Tt, 16, H/2, W/2), clip (1,Lc,1280);
        tile_w (n_tiles, Tt) = m_k * tile_weight and inv_wsum (T) as RFSamplerLong.sample_hip forms them.  Single rank, one character.
        ``reuse``: None, or the step cache's plan -- one 0 / 1 per step, shared by every tile; 1 = every tile reuses its own block
        residual of the last computed step (scail_dit_sample_tiled_cached).  ``solver``: None, or ``sample_c``'s solver plan
        (scail_dit_sample_tiled_solver); not together with ``reuse``."""
        dev, Tt = x32.device, len(tile_indices[0])
        if solver is not None and reuse is not None:
            raise NotImplementedError("a solver plan together with the step cache is out of scope (include/scail_dit.h \"solver plan\")")
        if reuse is not None:
            self._step_cache_ok()
        if ref.shape[1] != 1:
            raise L.ScailHipError(f"temporal tiles take one reference frame (tiles and several characters are not combined), got {ref.shape[1]}")
        if pose_tiles.dim() != 6 or pose_tiles.shape[1] != len(tile_indices) or pose_tiles.shape[2] != Tt:
            raise L.ScailHipError(f"smpl_tiled must be (1, n_tiles = {len(tile_indices)}, Tt = {Tt}, 16, H/2, W/2), got "
                                  f"{tuple(pose_tiles.shape)}")
        ex, cond, cos, sin, x = self._sample_prelude(x32, ctx, clip, cond_key, Tt, 1)
        if solver is not None:
            return ex.sample_tiled(x, sigmas, cfg_scale, cond, _as_bf16(ref, dev), _as_bf16(pose_tiles, dev), tile_indices, tile_w, inv_wsum,
                                   cos, sin, solver=solver)
        if reuse is not None:
            return ex.sample_tiled_cached(x, sigmas, cfg_scale, cond, _as_bf16(ref, dev), _as_bf16(pose_tiles, dev), tile_indices, tile_w, inv_wsum,
                                          cos, sin, reuse)
        return ex.sample_tiled(x, sigmas, cfg_scale, cond, _as_bf16(ref, dev), _as_bf16(pose_tiles, dev), tile_indices, tile_w, inv_wsum, cos, sin)

    def _run(self, x32, t32, ctx, ref, pose, clip, H_shift=0, W_shift=0, cond_key=None, cfg_pair=False, step_cache=None):
        if step_cache is not None:
            self._step_cache_ok()
        W = self.prepare()
        dev = x32.device
        B, T, _, H, Wd = x32.shape
        D, nh, eps = self.hidden_size, self.num_attention_heads, self.layernorm_epsilon
        hp, wp = H // 2, Wd // 2
        # n_char > 1: multi-character in-context concat, an EXTENSION (BASELINE config 5; the reference has one reference
        # frame and one pose stream): ref (n, C, 16, H, W), pose (n, C*T, 16, H/2, W/2), tokens
        # [ref_0..ref_{C-1} | noise | pose_0..pose_{C-1}], RoPE windows of rope.build_tables(n_char=C)
        n_char = ref.shape[1]
        self._check_chars(n_char, T, pose.shape[1])
        Lref1, Lnoise, Lpose1 = hp * wp, T * hp * wp, T * (H // 4) * (Wd // 4)
        Lref, Lpose = n_char * Lref1, n_char * Lpose1
        Ltok = Lref + Lnoise + Lpose
        if ctx.shape[0] != B:
            raise L.ScailHipError("context batch must equal the (CFG-doubled) input batch")
        cond = self._conditioning(ctx, clip, cond_key)
        cos, sin = self._rope(T, hp, wp, H_shift, W_shift, dev, n_char)
        sp = self.sp if (self.sp is not None and self.sp.size > 1) else None
        use_c = self.executor_ok()
        if self.fp8_mask and (sp is not None or not use_c):
            raise NotImplementedError(f"gemm_precision='{self.gemm_precision}' runs in the C executor on a single rank only: not on sequence-parallel ranks, "
                                      "not on the per-op path (SCAIL_C_STEP=0, _tap, kernel_timer)")
        ex = self._executor() if use_c else None
        xch = sp.c_exchange(nh, D, B, Ltok, dev) if (use_c and sp is not None) else None
        if use_c and not self._c_blocks:
            # the whole evaluation as ONE call into the library (include/scail_dit.h), for any number of characters; same kernels, same
            # order.  A sequence-parallel rank runs the same executor: only the collectives of the per-layer exchange come back to the
            # host (xch)
            if step_cache is not None:
                # "fill" | "reuse" (include/scail_dit.h "step cache"; _step_cache_ok above has refused every other route)
                return ex.step_cached(x32, t32, cond, ref.contiguous(), pose.contiguous(), cos, sin, step_cache, cfg_pair=cfg_pair, n_char=n_char)
            if sp is None:
                return ex.step(x32, t32, cond, ref.contiguous(), pose.contiguous(), cos, sin, cfg_pair=cfg_pair, n_char=n_char)
            return ex.step_sp(x32, t32, cond, ref.contiguous(), pose.contiguous(), cos, sin, xch, cfg_pair=cfg_pair, n_char=n_char)
        ws = self._workspace(B, Ltok, Lnoise, dev, blocks_in_c=use_c)

        # ---- time / AdaLN tables (reference :1521-1555, :1025-1028, :823) ----
        temb = ops.timestep_embedding(t32, self.time_freq_dim)
        e1 = ops.small_linear(temb, W["time_embed.0.w"], W["time_embed.0.b"], act_out=L.ACT_SILU)
        emb = ops.small_linear(e1, W["time_embed.2.w"], W["time_embed.2.b"])
        adaln = ops.small_linear(emb, W["adaln_projection.1.w"], W["adaln_projection.1.b"], act_in=L.ACT_SILU)
        mod = ops.adaln_table(adaln, W["adaln_tables"])                       # (layers, B, 6D) fp32
        fin = ops.adaln_table(emb.repeat(1, 2).contiguous(), W["final_table"])[0]   # (B, 2D) fp32

        # ---- patch embedding straight into the token layout [ref_0.. | noise | pose_0..] (:99-130), one launch for any n_char ----
        tok = ops.patchify(x32, ref.contiguous(), pose.contiguous(), kpad=128, out=ws["tok"], n_char=n_char)
        h = ws["h"]
        Lrn = Lref + Lnoise
        for b in range(B):
            ops.gemm(tok[b, :Lrn], W["patch_w"], W["patch_b"], out=h[b, :Lrn])
            ops.gemm(tok[b, Lrn:], W["pose_w"], W["pose_b"], out=h[b, Lrn:])
        if self._tap is not None:
            self._tap(-1, h)

        xn, qkv, att, ff, vt = ws["xn"], ws["qkv"], ws["att"], ws["ff"], ws["vt"]
        q, k, v = (None, None, None) if use_c else (qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:])
        for i, lw in enumerate(W["layers"]):
            m = mod[i]                                                        # (B, 6D)
            if use_c:
                # (_c_blocks: token assembly above in the host, every block as one executor call)
                if sp is None:
                    ex.block(i, h, m, cond, cos, sin)
                else:
                    ex.block_sp(i, h, m, cond, cos, sin, xch)
                continue
            sh_a, sc_a, g_a = m[:, 0:D], m[:, D:2 * D], m[:, 2 * D:3 * D]
            sh_m, sc_m, g_m = m[:, 3 * D:4 * D], m[:, 4 * D:5 * D], m[:, 5 * D:6 * D]
            # -- self attention (:1031-1036, :1058-1105) --
            ops.ln_modulate(h, sh_a, sc_a, out=xn, eps=eps)
            if sp is None:
                ops.gemm(xn, lw["qkv_w"], lw["qkv_b"], out=qkv)
                ops.rmsnorm_rope(k, lw["kn"], cos, sin, rows_per_batch=Ltok, eps=eps)
                ops.transpose_v(v, nh, out=vt)
                ops.rmsnorm_rope(q, lw["qn"], cos, sin, rows_per_batch=Ltok, eps=eps, out_scale=ops.ATTN_LOG2_SCALE)   # q in log2 units
                self._timed("self_attn", ops.flash_attn, q, k, vt, out=att, q_prescaled=True)
            else:
                sp.self_attention(self, lw, xn, qkv, vt, cos, sin, att, Ltok, eps)
            ops.gemm(att, lw["o_w"], lw["o_b"], out=h, epilogue=L.EPI_RESID, resid=h, gate=g_a, rows_per_batch=Ltok)
            # -- cross attention: text + CLIP, ungated residual (:1039-1042, :1107-1203) --
            ops.layernorm_affine(h, lw["ln_w"], lw["ln_b"], out=xn, eps=eps)
            cq = qkv[..., :D]
            ops.gemm(xn, lw["cq_w"], lw["cq_b"], out=cq)
            ops.rmsnorm_rope(cq, lw["cqn"], eps=eps, out_scale=ops.ATTN_LOG2_SCALE)                # q in log2 units (as the executor does)
            ops.cross_attn2(cq, cond["k_text"][i], cond["vt_text"][i], cond["k_clip"][i], cond["vt_clip"][i], out=att, q_prescaled=True)
            ops.gemm(att, lw["co_w"], lw["co_b"], out=h, epilogue=L.EPI_RESID, resid=h)
            # -- MLP (:1045-1050; sat/transformer_defaults.py:163-176) --
            ops.ln_modulate(h, sh_m, sc_m, out=xn, eps=eps)
            ops.gemm(xn, lw["w1"], lw["b1"], out=ff, epilogue=L.EPI_GELU_TANH)
            ops.gemm(ff, lw["w2"], lw["b2"], out=h, epilogue=L.EPI_RESID, resid=h, gate=g_m, rows_per_batch=Ltok)
            if self._tap is not None:
                self._tap(i, h)

        # ---- final layer on the noise tokens only + unpatchify (:818-835, :764-784) ----
        ops.ln_modulate(h, fin[:, :D], fin[:, D:], out=ws["xf"], eps=eps, rows_out=Lnoise, src_row_offset=Lref)
        ops.gemm(ws["xf"], W["final_w"], W["final_b"], out=ws["tokout"])
        return ops.unpatchify(ws["tokout"], T, H, Wd)
