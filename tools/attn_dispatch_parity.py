"""Kernel-by-kernel parity of the attention dispatch between two checkouts (one GPU): SHA-256 of the output of one small ops.flash_attn call per
route of scail_flash_attn_bf16 -- the 8-wave kernel (plain, raw scale, accumulate, segments, option attn4 = 0), scail_attn4_m16f at 256 and 192 rows,
as planned, in each workgroup-id decode (4, 8 and 9 pairs, attn4_xcd = 0) and in its planned two-launch form (option attn4_cus, the shape searched
with scail_flash_attn_rows_for) -- and of one ops.cross_attn2 call per route of scail_cross_attn2_bf16 (cross_attn2_kernel; scail_attn4_x2 by option
and by key count), on seeded inputs made on the device (a host-to-device copy is a kernel or a DMA as the runtime sees fit: it would make the
kernel tables of two runs differ).  Uses only functions both checkouts have; run it in each, under
`rocprofv3 --kernel-trace --stats -- python tools/attn_dispatch_parity.py`, and compare the lines and the kernel-name -> call-count tables
(profiles/attn_dispatch_parity.log)."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda"
OPTION_DEFAULTS = {"attn4": 1, "attn4_rows": 0, "attn4_xcd": 1, "attn4_cus": 0, "cross4": 2}

# (label, B, H, Lq, Lk, n_seg, raw scale, accumulate, options)
SELF = [("8-wave 2x2 300x257", 2, 2, 300, 257, 1, False, False, {}), ("8-wave raw 2x2 130x64", 2, 2, 130, 64, 1, True, False, {}),
        ("8-wave accumulate 1x2 300x65", 1, 2, 300, 65, 1, False, True, {}), ("8-wave segments 1x2 130x3x100", 1, 2, 130, 100, 3, False, False, {}),
        ("8-wave attn4=0 1x1 256x512", 1, 1, 256, 512, 1, False, False, {"attn4": 0}),
        ("m16f planned 2x2 300x576", 2, 2, 300, 576, 1, False, False, {}), ("m16f 256 rows 2x2 300x576", 2, 2, 300, 576, 1, False, False, {"attn4_rows": 256}),
        ("m16f 192 rows 2x2 300x576", 2, 2, 300, 576, 1, False, False, {"attn4_rows": 192}), ("m16f raw 192 rows 1x3 300x513", 1, 3, 300, 513, 1, True, False, {"attn4_rows": 192}),
        ("m16f 8 pairs 2x4 520x1088", 2, 4, 520, 1088, 1, False, False, {"attn4_rows": 256}), ("m16f 8 pairs xcd off 2x4 300x576", 2, 4, 300, 576, 1, False, False, {"attn4_rows": 256, "attn4_xcd": 0}),
        ("m16f 9 pairs 3x3 300x512", 3, 3, 300, 512, 1, False, False, {"attn4_rows": 256}), ("m16f 12 pairs 192 rows 2x6 130x513", 2, 6, 130, 513, 1, True, False, {"attn4_rows": 192}),
        ("m16f segments 1x2 200x3x512", 1, 2, 200, 512, 3, False, False, {"attn4_rows": 256})]
# (label, B, H, Lq, Lk1, Lk2, raw scale, options)
CROSS = [("cross hipcc 2x2 300x512+257", 2, 2, 300, 512, 257, False, {}), ("cross hipcc raw 1x3 128x77+1", 1, 3, 128, 77, 1, True, {}),
         ("cross x2 by option 2x2 300x512+257", 2, 2, 300, 512, 257, False, {"cross4": 1}), ("cross x2 by key count 2x1 515x1024+320", 2, 1, 515, 1024, 320, True, {})]


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def with_options(L, opts, fn):
    try:
        for k, v in opts.items():
            L.set_option(k, v)
        return fn()
    finally:
        for k in opts:
            L.set_option(k, OPTION_DEFAULTS[k])


def rand(g, *shape):
    return (torch.randn(*shape, generator=g, device=DEV) * 0.5).to(torch.bfloat16)


def self_attention(L, ops, label, B, H, Lq, Lk, S, raw, acc, opts):
    g = torch.Generator(device=DEV).manual_seed(11)
    D = H * 128
    q, k, v = rand(g, B, Lq, D), rand(g, S, B, Lk, D), rand(g, S, B, Lk, D)
    vt = torch.stack([ops.transpose_v(v[s], H) for s in range(S)])
    out = rand(g, B, Lq, D) if acc else torch.zeros(B, Lq, D, dtype=torch.bfloat16, device=DEV)
    kw = dict(scale=0.09) if raw else dict(q_prescaled=True)

    def call():
        ops.flash_attn(q, k[0], vt[0], out=out, accumulate=acc, n_seg=S, k_seg_stride=k.stride(0) if S > 1 else 0, vt_seg_stride=vt.stride(0) if S > 1 else 0, **kw)
        torch.cuda.synchronize()

    with_options(L, opts, call)
    print(f"{label} {sha(out)}", flush=True)


def two_launch(L, ops, B, H, Lq0):
    """the planned two-launch form: the first (attn4_cus, Lq) for which scail_flash_attn_rows_for answers 448"""
    lib = L.load()
    try:
        found = next(((cus, Lq) for Lq in range(Lq0, 4097, 64) for cus in range(1, 17) if L.set_option("attn4_cus", cus) or lib.scail_flash_attn_rows_for(B, H, Lq) == 448), None)
    finally:
        L.set_option("attn4_cus", 0)
    assert found is not None
    cus, Lq = found
    self_attention(L, ops, f"m16f two launches attn4_cus {cus} {B}x{H} {Lq}x512", B, H, Lq, 512, 1, False, False, {"attn4_cus": cus})


def cross_attention(L, ops, label, B, H, Lq, Lk1, Lk2, raw, opts):
    g = torch.Generator(device=DEV).manual_seed(13)
    D = H * 128
    q, k1, v1, k2, v2 = rand(g, B, Lq, D), rand(g, B, Lk1, D), rand(g, B, Lk1, D), rand(g, 1, Lk2, D), rand(g, 1, Lk2, D)
    out = torch.zeros(B, Lq, D, dtype=torch.bfloat16, device=DEV)
    kw = dict(scale=0.09) if raw else dict(q_prescaled=True)

    def call():
        ops.cross_attn2(q, k1, ops.transpose_v(v1, H), k2, ops.transpose_v(v2, H), out=out, **kw)
        torch.cuda.synchronize()

    with_options(L, opts, call)
    print(f"{label} {sha(out)}", flush=True)


if __name__ == "__main__":
    from scail_amd import lib, ops
    lib.load()
    for case in SELF:
        self_attention(lib, ops, *case)
    two_launch(lib, ops, 1, 1, 64)
    two_launch(lib, ops, 3, 3, 256)
    for case in CROSS:
        cross_attention(lib, ops, *case)
