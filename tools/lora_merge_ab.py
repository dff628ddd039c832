"""A/B of the LoRA merge kernel (include/scail_hip.h scail_lora_merge_bf16; scail_amd/lora.py) against a torch arm on the same device.
  * cells: the four 14B GEMM shapes (15360 x 5120, 5120 x 5120, 13824 x 5120, 5120 x 13824) at r = 16, 64, 128.  The arms alternate in
    one process, --reps repetitions after a warm-up, each call between two device events; median and [min, max].
      arm 1  ops.lora_merge_ (the HIP kernel: every operation rounded on its own, in place)
      arm 2  w.float().addmm_(up, down, alpha=s).bfloat16() -- tools may use it, the product may not; it differs in bits (a GEMM's
             accumulation order and fused multiply-adds) and serves as a TIME only
    Per cell: ms, 4 N K bytes / time (w read and written once) as a fraction of the 8 TB/s HBM peak, and 2 N K r lane-operations / time
    (one multiply and one add per j, not fused).
  * network: merge_lora of a rank-64 adapter over every block matrix (Wan names: 12 modules per layer) of the random-init 14B network
    with --layers layers: wall time of the whole call (host to device copies of the factors included) and the kernels' share.
Nothing here is a criterion.  Usage: python tools/lora_merge_ab.py [--reps 3] [--layers 40] [--log profiles/lora_merge_ab.log]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scail_amd import lib as L, lora, ops  # noqa: E402

P14B = dict(hidden_size=5120, num_attention_heads=40, inner_hidden_size=13824, text_dim=4096, time_freq_dim=256, time_embed_dim=5120)
SHAPES = [(15360, 5120), (5120, 5120), (13824, 5120), (5120, 13824)]
RANKS = [16, 64, 128]
HBM_PEAK = 8.0e12
SCALE = 0.125


def _summ(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": len(ts)}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def cells(reps, say):
    out = {}
    for N, K in SHAPES:
        for r in RANKS:
            g = torch.Generator(device="cuda").manual_seed(N + K + r)
            w = (torch.randn(N, K, generator=g, device="cuda") * 0.02).to(torch.bfloat16)
            up = torch.randn(N, r, generator=g, device="cuda") * 0.05
            down = torch.randn(r, K, generator=g, device="cuda") * 0.05
            arms = {"hip": lambda: ops.lora_merge_(w, up, down, SCALE),
                    "torch": lambda: w.copy_(w.float().addmm_(up, down, alpha=SCALE).bfloat16())}
            for fn in arms.values():                      # warm-up: code objects, allocator
                fn()
            ts = {k: [] for k in arms}
            for _ in range(reps):
                for k, fn in arms.items():
                    ts[k].append(_timed(fn))
            s = {k: _summ(v) for k, v in ts.items()}
            ms = s["hip"]["median_ms"]
            s["hbm_fraction"] = 4.0 * N * K / (ms * 1e-3) / HBM_PEAK
            s["lane_tops"] = 2.0 * N * K * r / (ms * 1e-3) / 1e12
            out[f"{N}x{K} r{r}"] = s
            say(f"{N:>6} x {K:<6} r {r:<4} hip {ms:8.3f} ms [{s['hip']['min_ms']:.3f}, {s['hip']['max_ms']:.3f}]  "
                f"{s['hbm_fraction']:.3f} of HBM peak  {s['lane_tops']:6.2f} T lane-ops/s   torch {s['torch']['median_ms']:8.3f} ms "
                f"[{s['torch']['min_ms']:.3f}, {s['torch']['max_ms']:.3f}]")
            del w, up, down
    return out


def network(layers, say):
    from scail_amd.dit import DiffusionTransformer
    net = DiffusionTransformer(transformer_args=dict(model_parallel_size=1), num_frames=81, latent_width=300, latent_height=300,
                               share_adaln=True, use_i2v_clip=True, device="cuda", init_seed=1234, num_layers=layers, **P14B)
    spec = net.param_spec()
    g = torch.Generator().manual_seed(1)
    t = {}
    for name, tgt in lora.wan_aliases(net).items():
        shape = spec[tgt.weight]
        if name.startswith("blocks.") and len(shape) == 2:
            rows = shape[0] if tgt.rows is None else tgt.rows
            t[name + ".lora_A.weight"] = (torch.randn(64, shape[1], generator=g) * 0.05).to(torch.bfloat16)
            t[name + ".lora_B.weight"] = (torch.randn(rows, 64, generator=g) * 0.05).to(torch.bfloat16)
    plan = lora.plan_adapter(net, t, 1.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lora.apply_plan(net, plan)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    dev = [(lora._window(dict(net.named_parameters())[e.param].data, e), e.up.float().cuda(), e.down.float().cuda(), e.scale) for e in plan[:12]]
    kern = sum(_timed(lambda a=a: ops.lora_merge_(*a)) for a in dev) * len(plan) / len(dev)
    say(f"network: {layers} layers, {len(plan)} rank-64 pairs: merge_lora's apply_plan {wall:.2f} s wall (factors cross from the host), "
        f"of which the kernels about {kern / 1e3:.3f} s (the first layer's twelve, timed again, scaled)")
    return {"layers": layers, "pairs": len(plan), "wall_s": wall, "kernels_s": kern / 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "lora_merge_ab.log"))
    a = ap.parse_args()
    L.load()
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "w") as f:
        def say(s):
            print(s, flush=True)
            f.write(s + "\n")
            f.flush()
        say(f"lora_merge_ab: {torch.cuda.get_device_name(0)}, reps {a.reps}; HBM peak taken as {HBM_PEAK / 1e12:.0f} TB/s")
        res = {"cells": cells(a.reps, say)}
        if a.layers > 0:
            res["network"] = network(a.layers, say)
        say(json.dumps(res))


if __name__ == "__main__":
    main()
