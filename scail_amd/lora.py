"""LoRA adapters for the DiT (an extension, opt-in: the reference ships sgm/modules/diffusionmodules/lora.py, whose ``_fuse_lora`` computes
W + lora_scale * (alpha / rank) * up @ down, but its inference path never calls it).

An adapter is MERGED into the bf16 weights once, on the GPU, by two HIP kernels (include/scail_hip.h scail_lora_merge_bf16 /
scail_add_scaled_bf16; ops.lora_merge_ / ops.add_scaled_); everything downstream -- the schedule, the guidance plan, the quantised GEMMs --
then runs on the merged network as on any other.  Per weight element, every operation rounded on its own in fp32 and ONE rounding to bf16:

    acc = 0;  for j ascending: acc = acc + up[n, j] * down[j, k];   w[n, k] = bf16(float(w[n, k]) + scale * acc)
    w[n, k] = bf16(float(w[n, k]) + scale * diff[n, k])                                        (``.diff`` / ``.diff_b`` keys)

with scale = float32(strength * alpha / rank) (a missing alpha means alpha = rank) and scale = float32(strength) for differences.

    read_adapter(path)                      -> {key: host tensor}         .safetensors or a torch.load-able file
    plan_adapter(network, tensors, strength) -> [Entry]                   the whole validation; needs no device
    apply_plan(network, plan)                                             the kernels + dropping the network's derived state

Keys: ``X.lora_A.weight`` / ``X.lora_B.weight`` (down / up) or ``X.lora_down.weight`` / ``X.lora_up.weight``, optional ``X.alpha``,
``X.diff`` (difference of ``X.weight`` or of a bare parameter such as a modulation table), ``X.diff_b`` (difference of ``X.bias``); an
optional leading ``diffusion_model.`` is dropped.  X is a NATIVE module name (the SAT names of ``DiffusionTransformer.param_spec()``
without ``.weight``: ``transformer.layers.3.attention.query_key_value`` is the whole fused matrix, ``mixins.patch_embed.proj`` is taken
as (D, 80)) or one of Wan2.1's own module names (``wan_aliases``: ``blocks.3.self_attn.q`` is rows [0, D) of that fused matrix).

WHAT IS NOT KNOWN: the Wan names are that project's public module tree as the authors of this file know it.  No real adapter file and
no real weights have been available to check them against; the table is tested for internal consistency only (every alias resolves
to a parameter, the aliases of a block cover each of its matrices exactly once).  The row order [q; k; v] of the fused matrices is the
one the executor reads ("LoRA adapters").

An adapter applies whole or not at all: every refusal (ValueError naming the key) comes from ``plan_adapter``, before any weight is
touched.  Several adapters stack; the result depends on their order in the last bf16 bit.  There is no un-merge: merging with
``-strength`` is not the inverse in bits (two bf16 roundings) -- to drop an adapter, load the checkpoint again."""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Dict, List, Optional

import torch

# param: the parameter's name in param_spec(); row_offset / rows: the window along its first axis (a 1-D parameter: its elements);
# kind: "lora" (up (rows, rank), down (rank, K)) or "diff" (up None, down = the difference, rank 0, alpha None); key: the file's key
Entry = namedtuple("Entry", "param row_offset rows kind up down scale rank alpha key")
# what a module name stands for: the parameter that takes pairs and ``.diff``, the one that takes ``.diff_b``, and the row window
Target = namedtuple("Target", "weight bias row_offset rows")

PREFIX = "diffusion_model."
DOWN_SUFFIXES = (".lora_A.weight", ".lora_down.weight")
UP_SUFFIXES = (".lora_B.weight", ".lora_up.weight")
SUFFIXES = DOWN_SUFFIXES + UP_SUFFIXES + (".alpha", ".diff_b", ".diff")


def wan_aliases(network) -> Dict[str, Target]:
    """Wan2.1 module name -> Target, for every layer of ``network`` (anything with hidden_size, num_layers and param_spec()).  THE table:
    nothing else in the package knows a Wan name."""
    D = network.hidden_size
    a: Dict[str, Target] = {}

    def lin(wan, native, row_offset=0, rows=None):
        a[wan] = Target(native + ".weight", native + ".bias", row_offset, rows)

    for i in range(network.num_layers):
        b, t, m = f"blocks.{i}.", f"transformer.layers.{i}.", "mixins.adaln_layer."
        for j, n in enumerate("qkv"):
            lin(b + "self_attn." + n, t + "attention.query_key_value", j * D, D)
        lin(b + "self_attn.o", t + "attention.dense")
        lin(b + "cross_attn.q", t + "cross_attention.query")
        lin(b + "cross_attn.o", t + "cross_attention.dense")
        for j, n in enumerate("kv"):
            lin(b + "cross_attn." + n, t + "cross_attention.key_value", j * D, D)
            lin(b + f"cross_attn.{n}_img", m + f"clip_feature_key_value_list.{i}", j * D, D)
        lin(b + "ffn.0", t + "mlp.dense_h_to_4h")
        lin(b + "ffn.2", t + "mlp.dense_4h_to_h")
        lin(b + "norm3", t + "post_cross_attention_layernorm")
        for wan, native in (("self_attn.norm_q", "query"), ("self_attn.norm_k", "key"), ("cross_attn.norm_q", "cross_query"),
                            ("cross_attn.norm_k", "cross_key"), ("cross_attn.norm_k_img", "clip_feature_key")):
            a[b + wan] = Target(m + f"{native}_layernorm_list.{i}.weight", None, 0, None)
        a[b + "modulation"] = Target(m + f"adaLN_modulations.{i}", None, 0, None)
    for n in (0, 2):
        lin(f"text_embedding.{n}", f"text_embedding.{n}")
        lin(f"time_embedding.{n}", f"time_embed.{n}")
    lin("time_projection.1", "adaln_projection.1")
    for n in (0, 1, 3, 4):
        lin(f"img_emb.proj.{n}", f"clip_proj.proj.{n}")
    lin("head.head", "mixins.final_layer.linear")
    a["head.modulation"] = Target("mixins.final_layer.adaLN_modulation", None, 0, None)
    return a


def resolve(module: str, spec: Dict[str, tuple], aliases: Dict[str, Target]) -> Optional[Target]:
    """Target of a module name under either convention, or None"""
    if module in aliases:
        t = aliases[module]
        return t if t.weight in spec else None
    if module + ".weight" in spec:
        return Target(module + ".weight", module + ".bias" if module + ".bias" in spec else None, 0, None)
    if module in spec:                                    # a bare parameter: a modulation table
        return Target(module, None, 0, None)
    return None


def window_shape(shape: tuple, rows: Optional[int]):
    """(rows, K) of the window the kernels see: a 1-D parameter and a (1, n, D) table are one row; anything else is (shape[0], the rest)"""
    if len(shape) == 1:
        return 1, (shape[0] if rows is None else rows)
    if len(shape) == 3 and shape[0] == 1:
        return 1, shape[1] * shape[2]
    return (shape[0] if rows is None else rows), math.prod(shape[1:])


def read_adapter(path: str) -> Dict[str, torch.Tensor]:
    """{key: tensor} of a ``.safetensors`` file or of a torch.load-able one (a dict of tensors, possibly under "state_dict"); the tensors
    stay on the host."""
    path = str(path)
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file            # lazily: only adapter files in this format need the package
        return dict(load_file(path, device="cpu"))
    sd = torch.load(path, map_location="cpu")
    if isinstance(sd, dict) and isinstance(sd.get("state_dict"), dict):
        sd = sd["state_dict"]
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: expected a dict of tensors, got {type(sd).__name__}")
    return dict(sd)


def _f32(x: float) -> float:
    return torch.tensor(x, dtype=torch.float64).to(torch.float32).item()


def plan_adapter(network, tensors: Dict[str, torch.Tensor], strength: float = 1.0) -> List[Entry]:
    """Every key of ``tensors`` resolved against ``network.param_spec()`` and validated; entries in param_spec() order.  Raises ValueError
    naming the key for: a key that resolves to no parameter, a pair with one half, ranks that differ, outer shapes that do not match the
    slice, a difference of the wrong shape, an alpha that is not a finite scalar, a non-floating tensor, a strength that is not finite,
    and a file that yields no entry.  Touches nothing: ``network`` only answers param_spec(), hidden_size and num_layers."""
    try:
        strength = float(strength)
    except (TypeError, ValueError):
        raise ValueError(f"strength must be a finite number, got {strength!r}")
    if not math.isfinite(strength):
        raise ValueError(f"strength must be finite, got {strength}")
    spec = network.param_spec()
    order = {n: i for i, n in enumerate(spec)}
    aliases = wan_aliases(network)
    modules: Dict[str, Dict[str, tuple]] = {}              # module -> {"down" | "up" | "alpha" | "diff" | "diff_b": (key, tensor)}
    for key, t in tensors.items():
        name = key[len(PREFIX):] if key.startswith(PREFIX) else key
        suffix = next((s for s in SUFFIXES if name.endswith(s)), None)
        if suffix is None:
            raise ValueError(f"{key}: not an adapter key (expected a name ending in one of {', '.join(SUFFIXES)})")
        module = name[:-len(suffix)]
        if resolve(module, spec, aliases) is None:
            raise ValueError(f"{key}: module {module!r} resolves to no parameter of the network (native SAT names and Wan2.1 module names are known)")
        if not torch.is_tensor(t) or not t.is_floating_point():
            raise ValueError(f"{key}: expected a floating-point tensor, got {getattr(t, 'dtype', type(t).__name__)}")
        role = "down" if suffix in DOWN_SUFFIXES else "up" if suffix in UP_SUFFIXES else suffix[1:]
        slot = modules.setdefault(module, {})
        if role in slot:
            raise ValueError(f"{key}: the same tensor as {slot[role][0]} (both spellings of one half in one file)")
        slot[role] = (key, t)
    plan: List[Entry] = []
    taken: Dict[tuple, list] = {}                          # (param, kind) -> [(first row, end row, key)]

    def add(e: Entry):
        for lo, hi, other in taken.setdefault((e.param, e.kind), []):
            if e.row_offset < hi and lo < e.row_offset + e.rows:
                raise ValueError(f"{e.key}: targets the same rows of {e.param} as {other} (one module under two names)")
        taken[(e.param, e.kind)].append((e.row_offset, e.row_offset + e.rows, e.key))
        plan.append(e)

    for module, slot in modules.items():
        tgt = resolve(module, spec, aliases)
        if ("down" in slot) != ("up" in slot):
            key = slot["down" if "down" in slot else "up"][0]
            raise ValueError(f"{key}: a pair with only one half (module {module!r} has no {'up' if 'down' in slot else 'down'} matrix)")
        if "alpha" in slot and "down" not in slot:
            raise ValueError(f"{slot['alpha'][0]}: an alpha without a pair (module {module!r})")
        if "down" in slot:
            (kd, down), (ku, up) = slot["down"], slot["up"]
            shape = spec[tgt.weight]
            if len(shape) < 2 or (len(shape) == 3 and shape[0] == 1):
                raise ValueError(f"{kd}: module {module!r} resolves to no parameter that takes a low-rank pair ({tgt.weight} {shape} takes .diff only)")
            n, k = window_shape(shape, tgt.rows)
            if down.dim() != 2 or up.dim() != 2:
                raise ValueError(f"{kd if down.dim() != 2 else ku}: expected a 2-D matrix, got shape {tuple((down if down.dim() != 2 else up).shape)}")
            r = down.shape[0]
            if up.shape[1] != r:
                raise ValueError(f"{ku}: ranks differ: up {tuple(up.shape)} against down {tuple(down.shape)} ({kd})")
            if r == 0 or r >= 1 << 15:
                raise ValueError(f"{kd}: rank must be 1 .. 32767, got {r}")
            if up.shape[0] != n:
                raise ValueError(f"{ku}: up {tuple(up.shape)} does not match the slice: {n} rows of {tgt.weight} {shape}")
            if down.shape[1] != k:
                raise ValueError(f"{kd}: down {tuple(down.shape)} does not match the slice: {k} columns of {tgt.weight} {shape}")
            alpha = float(r)
            if "alpha" in slot:
                ka, ta = slot["alpha"]
                if ta.numel() != 1 or not math.isfinite(float(ta)):
                    raise ValueError(f"{ka}: alpha must be a finite scalar, got {tuple(ta.shape) if ta.numel() != 1 else float(ta)}")
                alpha = float(ta)
            scale = _f32(strength * alpha / r)
            if not math.isfinite(scale):
                raise ValueError(f"{kd}: scale = strength * alpha / rank = {strength} * {alpha} / {r} is not finite in fp32")
            add(Entry(tgt.weight, tgt.row_offset, n, "lora", up, down, scale, r, alpha, kd))
        for role, pname in (("diff", tgt.weight), ("diff_b", tgt.bias)):
            if role not in slot:
                continue
            key, d = slot[role]
            if pname is None:
                raise ValueError(f"{key}: module {module!r} resolves to no parameter with a bias")
            shape = spec[pname]
            n, k = window_shape(shape, tgt.rows)
            full = ((shape[0] if tgt.rows is None else tgt.rows),) + tuple(shape[1:])
            if tuple(d.shape) not in (full, (n, k)):
                raise ValueError(f"{key}: a difference of shape {tuple(d.shape)} for {full} ({'rows of ' if tgt.rows is not None else ''}{pname})")
            add(Entry(pname, tgt.row_offset, full[0], "diff", None, d, _f32(strength), 0, None, key))
    if not plan:
        raise ValueError("the adapter yields no entry (no tensors)")
    kinds = {"lora": 0, "diff": 1}
    plan.sort(key=lambda e: (order[e.param], e.row_offset, kinds[e.kind]))
    return plan


def summary(plan: List[Entry]) -> List[tuple]:
    """One row per entry, without the tensors: (param, row_offset, rows, kind, rank, alpha, scale)"""
    return [(e.param, e.row_offset, e.rows, e.kind, e.rank, e.alpha, e.scale) for e in plan]


def _window(p: torch.Tensor, e: Entry) -> torch.Tensor:
    """The 2-D window of parameter ``p`` that entry ``e`` updates: a view of the parameter's storage"""
    if p.dim() == 1:
        return p[e.row_offset:e.row_offset + e.rows].view(1, -1)
    if p.dim() == 3 and p.shape[0] == 1:
        return p.view(1, -1)
    return p.view(p.shape[0], -1)[e.row_offset:e.row_offset + e.rows]


def check_parameters(network, plan: List[Entry]) -> Dict[str, torch.Tensor]:
    """The parameters a plan touches, refused by name when one has no storage yet (meta) or does not live on the GPU"""
    from . import lib as L
    params = dict(network.named_parameters())
    for e in plan:
        p = params.get(e.param)
        if p is None:
            raise ValueError(f"{e.key}: the network has no parameter {e.param}")
        if p.is_meta:
            raise ValueError(f"{e.param} is a meta parameter: attach storage (load_state_dict(..., assign=True)) before merging an adapter")
        if not p.is_cuda:
            raise L.ScailHipError(f"{e.param} is on {p.device}: an adapter is merged on the GPU by the library's kernels (no CPU path); call .cuda()")
        if p.dtype != torch.bfloat16 or not p.is_contiguous():
            raise L.ScailHipError(f"{e.param}: expected a contiguous bf16 parameter, got {p.dtype} with strides {p.stride()}")
    return params


@torch.no_grad()
def apply_plan(network, plan: List[Entry]) -> None:
    """Run a validated plan: per entry the factors (or the difference) go to the device as fp32 (an exact widening of fp16 / bf16) and
    ONE kernel updates the parameter's storage in place.  Afterwards the network's derived state is dropped
    (DiffusionTransformer.weights_changed): the prepared fp32 vectors and padded matrices, the conditioning cache and the executor with
    its fp8 / MX / fp6 weight buffers, probe state and caches; the next call rebuilds them from the merged weights."""
    from . import ops
    params = check_parameters(network, plan)
    try:
        for e in plan:
            p = params[e.param].data
            w = _window(p, e)
            dev = p.device
            if e.kind == "lora":
                ops.lora_merge_(w, e.up.detach().float().contiguous().to(dev), e.down.detach().float().contiguous().to(dev), e.scale)
            else:
                ops.add_scaled_(w, e.down.detach().float().reshape(w.shape).contiguous().to(dev), e.scale)
    finally:
        network.weights_changed()


def format_table(name: str, strength: float, rows: List[tuple]) -> str:
    """The CLI's table for one adapter from its summary rows: entries, matrices touched, rank range, alpha, strength"""
    lo = [r for r in rows if r[3] == "lora"]
    ranks = sorted({r[4] for r in lo})
    alphas = sorted({r[5] for r in lo})
    rng = "-" if not ranks else str(ranks[0]) if len(ranks) == 1 else f"{ranks[0]}..{ranks[-1]}"
    al = "-" if not alphas else f"{alphas[0]:g}" if len(alphas) == 1 else f"{alphas[0]:g}..{alphas[-1]:g}"
    return (f"lora {name}: {len(rows)} entries ({len(lo)} low-rank, {len(rows) - len(lo)} differences) on {len({r[0] for r in rows})} "
            f"parameters ({len({r[0] for r in lo})} matrices), rank {rng}, alpha {al}, strength {strength:g}")
