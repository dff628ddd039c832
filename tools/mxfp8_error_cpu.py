"""CPU experiment behind DESIGN.md section 4.1 "what block scaling does and does not fix": squared error of the fp8 GEMM under MX block
scales (E8M0 per 32 along K, include/scail_hip.h scail_quant_mxfp8_rows) relative to per-row fp32 scales (scail_quant_fp8_rows), both
against the product of the bf16 operands, everything after quantization in fp64.  Gaussian data without outliers: randn activations
(448 x K), 0.02 randn weights (256 x K), 10 seeds, K = 256, 512, 5120.  No GPU.
Usage: python tools/mxfp8_error_cpu.py [--seeds 10]"""
from __future__ import annotations

import argparse

import torch


def quant_row(x):
    """per-row: s = amax / 448, q = e4m3(x * 448 / amax); returns the dequantized fp64 matrix"""
    xf = x.float()
    amax = xf.abs().amax(1, keepdim=True)
    q = (xf * (448.0 / amax)).clamp(-448, 448).to(torch.float8_e4m3fn).double()
    return q * (amax / 448.0).double()


def quant_mx(x):
    """per block of 32: s = the smallest integer with amax 2^-s <= 448, q = e4m3(x 2^-s); returns the dequantized fp64 matrix"""
    R, C = x.shape
    b = x.float().reshape(R, C // 32, 32)
    m, e = torch.frexp(b.abs().amax(2))
    s = (e - 1 - 8 + (m > 0.875).int()).double()[:, :, None]
    q = (b.double() * torch.pow(2.0, -s)).float().clamp(-448, 448).to(torch.float8_e4m3fn).double()
    return (q * torch.pow(2.0, s)).reshape(R, C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=10)
    a = ap.parse_args()
    for K in (256, 512, 5120):
        ratios = []
        for seed in range(a.seeds):
            g = torch.Generator().manual_seed(seed)
            x = torch.randn(448, K, generator=g).to(torch.bfloat16)
            w = (torch.randn(256, K, generator=g) * 0.02).to(torch.bfloat16)
            ref = x.double() @ w.double().T
            err = {n: float(((q(x) @ q(w).T - ref) ** 2).sum()) for n, q in (("row", quant_row), ("mx", quant_mx))}
            ratios.append(err["mx"] / err["row"])
        print(f"K = {K:5d}: squared GEMM error, mx / row over {a.seeds} seeds: {min(ratios):.3f} .. {max(ratios):.3f} "
              f"(relative error row {(err['row'] / float((ref ** 2).sum())) ** 0.5:.4f})")


if __name__ == "__main__":
    main()
