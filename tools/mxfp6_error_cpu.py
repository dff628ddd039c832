"""CPU experiment behind DESIGN.md section 4.1 "what 6 bits cost": relative fp64 GEMM error of MXFP6 e2m3 (E8M0 per 32 along K,
include/scail_hip.h scail_quant_mxfp6_rows) next to MX e4m3 (scail_quant_mxfp8_rows) and per-row e4m3 (scail_quant_fp8_rows), each against
the product of the bf16 operands, everything after quantization in fp64.  Activations 256 x 1024, weights 512 x 1024 (0.02 randn), three
kinds of activation data: Gaussian, uniform in [-1, 1), Gaussian with one channel times 100.  The quantizers are written out here on
their own (value table + nearest, ties to even): the tool does not import the tests.  No GPU.
The line "gaussian squared-error ratio" is the figure r that tests/test_mxfp6_gpu.py holds the network-level accuracy to.
Usage: python tools/mxfp6_error_cpu.py [--seeds 10]"""
from __future__ import annotations

import argparse

import torch

E2M3 = torch.tensor([m / 8.0 for m in range(8)] + [(1.0 + m / 8.0) * 2.0 ** (e - 1) for e in (1, 2, 3) for m in range(8)], dtype=torch.float64)


def e2m3_round(v):
    """fp64 values in [-7.5, 7.5] -> the nearest e2m3 value, ties to the even code"""
    a = v.abs()
    lo = (torch.searchsorted(E2M3, a.contiguous(), right=True) - 1).clamp(0, 31)
    hi = (lo + 1).clamp(max=31)
    dl, dh = a - E2M3[lo], E2M3[hi] - a
    up = (dh < dl) | ((dh == dl) & (hi % 2 == 0))
    return torch.where(up, E2M3[hi], E2M3[lo]) * torch.sign(v)


def quant_row(x):
    """per-row e4m3: s = amax / 448; returns the dequantized fp64 matrix"""
    xf = x.float()
    amax = xf.abs().amax(1, keepdim=True)
    q = (xf * (448.0 / amax)).clamp(-448, 448).to(torch.float8_e4m3fn).double()
    return q * (amax / 448.0).double()


def _blocks(x, top_exp, m_thr):
    R, C = x.shape
    b = x.double().reshape(R, C // 32, 32)
    m, e = torch.frexp(b.abs().amax(2).float())
    s = (e - 1 - top_exp + (m > m_thr).int()).double()[:, :, None]
    return b, s, (R, C)


def quant_mx8(x):
    """MX e4m3: s = the smallest integer with amax 2^-s <= 448"""
    b, s, shape = _blocks(x, 8, 0.875)
    q = (b * torch.pow(2.0, -s)).float().clamp(-448, 448).to(torch.float8_e4m3fn).double()
    return (q * torch.pow(2.0, s)).reshape(shape)


def quant_mx6(x):
    """MX e2m3: s = the smallest integer with amax 2^-s <= 7.5"""
    b, s, shape = _blocks(x, 2, 0.9375)
    q = e2m3_round((b * torch.pow(2.0, -s)).clamp(-7.5, 7.5))
    return (q * torch.pow(2.0, s)).reshape(shape)


QUANT = (("row-e4m3", quant_row), ("mx-e4m3", quant_mx8), ("mx-e2m3", quant_mx6))


def activations(kind, g, M=256, K=1024):
    if kind == "uniform":
        return torch.rand(M, K, generator=g) * 2.0 - 1.0
    x = torch.randn(M, K, generator=g)
    if kind == "outlier-channel":
        x[:, 137] *= 100.0
    return x


def errors(kind, seed):
    """{quantizer: squared GEMM error / squared norm of the bf16 product} for one seed"""
    g = torch.Generator().manual_seed(seed)
    x = activations(kind, g).to(torch.bfloat16)
    w = (torch.randn(512, 1024, generator=g) * 0.02).to(torch.bfloat16)
    ref = x.double() @ w.double().T
    den = float((ref ** 2).sum())
    return {n: float(((q(x) @ q(w).T - ref) ** 2).sum()) / den for n, q in QUANT}


def gaussian_squared_ratio(seeds=10):
    """mean over the seeds of (MX-e2m3 squared error) / (MX-e4m3 squared error) on Gaussian data: the figure r"""
    e = [errors("gaussian", s) for s in range(seeds)]
    return sum(v["mx-e2m3"] / v["mx-e4m3"] for v in e) / len(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=10)
    a = ap.parse_args()
    print(f"relative fp64 GEMM error (256 x 1024 by 512 x 1024), mean over {a.seeds} seeds; squared ratio = mx-e2m3 / mx-e4m3")
    for kind in ("gaussian", "uniform", "outlier-channel"):
        e = [errors(kind, s) for s in range(a.seeds)]
        mean = {n: (sum(v[n] for v in e) / len(e)) ** 0.5 for n, _ in QUANT}
        ratios = [v["mx-e2m3"] / v["mx-e4m3"] for v in e]
        print(f"{kind:16s} row-e4m3 {mean['row-e4m3']:.4f}  mx-e4m3 {mean['mx-e4m3']:.4f}  mx-e2m3 {mean['mx-e2m3']:.4f}  "
              f"squared ratio {sum(ratios) / len(ratios):.3f} ({min(ratios):.3f} .. {max(ratios):.3f})")
    print(f"gaussian squared-error ratio r = {gaussian_squared_ratio(a.seeds):.3f}")


if __name__ == "__main__":
    main()
