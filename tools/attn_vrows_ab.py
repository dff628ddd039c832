#!/usr/bin/env python
"""Same-process A/B of the two self-attention routes on the config-2 launch (B = 2, 40 heads, L = 48 832, q | k | v the column thirds of one
QKV buffer as the executor holds them): route 0 = scail_transpose_v + scail_flash_attn_bf16 (scail_attn4_m16f on the V^T image), route 1 =
scail_flash_attn_vrows_bf16 (scail_attn4_m16f_vr on v as projected).  The routes alternate, `reps` timed repetitions each after `warm` untimed
ones; per route the minimum, median and maximum of the per-layer time (route 0: transpose + attention) in ms, and the outputs compared bit
for bit.  Usage: attn_vrows_ab.py [reps=10] [warm=2] [L=48832] [heads=40] [batch=2]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scail_amd import lib, ops  # noqa: E402

reps, warm, L, H, B = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 10), (2, 2), (3, 48832), (4, 40), (5, 2)))
D = H * 128
g = torch.Generator(device="cuda").manual_seed(0)
qkv = torch.randn(B, L, 3 * D, device="cuda", generator=g).to(torch.bfloat16)
q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
q.copy_((q.float() * ops.ATTN_LOG2_SCALE).to(torch.bfloat16))
assert lib.load().scail_flash_attn_vrows_for(3 * D, 3 * D, 3 * D, D, B, H, L, L) == 1, "the V-rows route does not take this launch"
vt = torch.empty(B, H, 128, (L + 63) // 64 * 64, device="cuda", dtype=torch.bfloat16)
out = [torch.empty(B, L, D, device="cuda", dtype=torch.bfloat16) for _ in range(2)]


def route(r):
    if r == 0:
        ops.transpose_v(v, H, out=vt)
        ops.flash_attn(q, k, vt, out=out[0], q_prescaled=True)
    else:
        ops.flash_attn_vrows(q, k, v, out=out[1], q_prescaled=True)


times = {0: [], 1: []}
for i in range(warm + reps):
    for r in (0, 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        route(r)
        e1.record()
        e1.synchronize()
        if i >= warm:
            times[r].append(e0.elapsed_time(e1))
res = {f"route{r}_ms": dict(min=round(min(t), 4), median=round(statistics.median(t), 4), max=round(max(t), 4)) for r, t in times.items()}
res.update(shape=dict(batch=B, heads=H, L=L), reps=reps, equal=bool(torch.equal(out[0], out[1])),
           saved_ms_median=round(statistics.median(times[0]) - statistics.median(times[1]), 4))
print(json.dumps(res))
