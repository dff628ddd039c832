"""Kernel-by-kernel parity of the convolution dispatch between two checkouts (one GPU): SHA-256 of every output tensor of ops.conv3d_cl,
ops.conv3d_cl_norm and ops.conv3d_cl_resid_norm on seeded inputs for one small geometry per kernel family, then of one WanVAE_ encode, decode
and streamed decode of the vae_dim96 fixture's input.  Uses only functions both checkouts have; run it in each, under
`rocprofv3 --kernel-trace --stats -- python tools/conv_dispatch_parity.py`, and compare the lines and the kernel-name -> call-count tables
(profiles/conv_dispatch_parity.log)."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda"

# (label, Cin, N, kernel, T, H, W of the input, ups, stride 2, ot_mul, forms): forms p plain, r plain + residual, n conv + norm,
# d next-norm with a residual, both outputs, o the same without the raw sum, u next-norm without a residual
CASES = [("96->96 3x3x3 T5 16x16", 96, 96, (3, 3, 3), 5, 16, 16, 0, 0, 1, "prndo"),
         ("96->96 3x3x3 T1 16x16", 96, 96, (3, 3, 3), 1, 16, 16, 0, 0, 1, "prnd"),
         ("32->64 3x3x3 T5 16x16", 32, 64, (3, 3, 3), 5, 16, 16, 0, 0, 1, "prn"),
         ("192->192 3x3x3 T5 16x16", 192, 192, (3, 3, 3), 5, 16, 16, 0, 0, 1, "prd"),
         ("192->96 1x3x3 ups T5 16x16", 192, 96, (1, 3, 3), 5, 16, 16, 1, 0, 1, "pu"),
         ("64->32 1x3x3 ups T1 16x16", 64, 32, (1, 3, 3), 1, 16, 16, 1, 0, 1, "p"),
         ("64->128 1x1x1 T81 12x16", 64, 128, (1, 1, 1), 81, 12, 16, 0, 0, 1, "pr"),
         ("64->128 1x1x1 T8 12x16", 64, 128, (1, 1, 1), 8, 12, 16, 0, 0, 1, "pr"),
         ("96->8 3x3x3 T5 16x16", 96, 8, (3, 3, 3), 5, 16, 16, 0, 0, 1, "p"),
         ("8->96 3x3x3 T17 16x16", 8, 96, (3, 3, 3), 17, 16, 16, 0, 0, 1, "pu"),
         ("96->96 3x1x1 ot_mul 2 T5 16x16", 96, 96, (3, 1, 1), 5, 16, 16, 0, 0, 2, "p"),
         ("96->96 1x3x3 stride 2 T4 40x56", 96, 96, (1, 3, 3), 4, 40, 56, 0, 1, 1, "p"),
         ("64->384 1x1x1 T81 12x16", 64, 384, (1, 1, 1), 81, 12, 16, 0, 0, 1, "p")]


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def convolutions():
    from scail_amd import ops
    for label, cin, n, k, T, H, W, ups, s2, ot_mul, forms in CASES:
        g = torch.Generator().manual_seed(7)
        x = torch.randn(T, H, W, cin, generator=g).to(torch.bfloat16).to(DEV)
        wp = ops.prep_conv_weight((torch.randn(n, cin, *k, generator=g) / (cin * k[0] * k[1] * k[2]) ** 0.5).to(DEV), torch.randn(n, generator=g).to(DEV))
        gam = (1 + 0.1 * torch.randn(wp["N"], generator=g)).to(DEV)
        out = (T, 2 * H, 2 * W) if ups else (T, H // 2, W // 2) if s2 else (T, H, W)
        r = torch.randn(*out, wp["N"], generator=g).to(torch.bfloat16).to(DEV)
        kw = dict(stride=(1, 2, 2), pad=(0, 0, 0)) if s2 else dict(pad=(0, 1, 1), ups=True) if ups else {}
        for f in forms:
            if f in "pr" and ot_mul == 2:
                y = torch.zeros(2 * T, H, W, wp["N"], dtype=torch.bfloat16, device=DEV)
                res = [ops.conv3d_cl(x, wp, out, out=y, ot_mul=2, ot_off=1)]
            elif f in "pr":
                res = [ops.conv3d_cl(x, wp, out, resid=r if f == "r" else None, **kw)]
            elif f == "n":
                res = [ops.conv3d_cl_norm(x, wp, gam)]
            else:
                res = ops.conv3d_cl_resid_norm(x, wp, None if f == "u" else r, gam, want_raw=f != "o", out_shape=out, **({} if not ups else dict(pad=(0, 1, 1), ups=True)))
            torch.cuda.synchronize()
            print(f"{label} [{f}] " + " ".join(sha(t) for t in res if t is not None), flush=True)


def vae():
    from oracle import wan_vae_oracle as V
    from scail_amd.wan_vae import WanVAE_
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(ROOT, "tests", "golden", "vae_dim96.npz")).items()}
    cfg = V.VAEConfig(dim=int(g["dim"]), z_dim=16)
    m = WanVAE_(dim=cfg.dim, z_dim=16, device=DEV)
    m.load_state_dict(V.make_state_dict(cfg, seed=int(g["seed"])), strict=True)
    print("vae_dim96 encode " + sha(m.encode(g["video"].to(DEV))), flush=True)
    print("vae_dim96 decode " + sha(m.decode(g["z_in"].to(DEV))), flush=True)
    print("vae_dim96 decode chunk_frames=2 " + sha(m.decode(g["z_in"].to(DEV), chunk_frames=2)), flush=True)


if __name__ == "__main__":
    from scail_amd import lib
    lib.load()
    convolutions()
    vae()
