"""The CPU restatement of the LoRA merge (include/scail_hip.h scail_lora_merge_bf16 / scail_add_scaled_bf16; scail_amd/lora.py): the loop
over j with ONE torch fp32 operation per arithmetic operation, and the merge of a whole state dict built on it.  Shared by
test_lora_cpu.py and test_lora_gpu.py; the tests compare on bits."""
import math

import torch

f32 = torch.float32
bf16 = torch.bfloat16


def _s(v):
    """a 0-dim fp32 tensor, so that every operation below is one fp32 operation on fp32 operands"""
    return torch.tensor(float(v), dtype=torch.float64).to(f32)


def cpu_acc(up, down, order=None):
    """acc = 0; for j ascending (or in ``order``): acc = acc + up[:, j] * down[j, :].  up (N, r), down (r, K), fp32 on the CPU"""
    assert up.dtype == down.dtype == f32 and up.shape[1] == down.shape[0]
    acc = torch.zeros(up.shape[0], down.shape[1], dtype=f32)
    for j in (range(up.shape[1]) if order is None else order):
        p = up[:, j:j + 1] * down[j:j + 1, :]
        acc = acc + p
    return acc


def cpu_add_scaled(w, d, scale):
    """bf16_rne(float(w) + scale * d): two fp32 operations and one rounding"""
    assert w.dtype == bf16 and d.dtype == f32
    sd = _s(scale) * d
    return (w.float() + sd).to(bf16)


def cpu_merge(w, up, down, scale):
    return cpu_add_scaled(w, cpu_acc(up, down), scale)


def scale_of(strength, alpha, rank):
    """float32(strength * alpha / rank), formed in Python floats and rounded once"""
    return float(_s(strength * alpha / rank))


def window(p, row_offset, rows):
    """the (rows, K) window of a parameter as scail_amd/lora.py sees it: a 1-D parameter and a (1, n, D) table are one row"""
    if p.dim() == 1:
        return p[row_offset:row_offset + rows].view(1, -1)
    if p.dim() == 3 and p.shape[0] == 1:
        return p.view(1, -1)
    return p.view(p.shape[0], -1)[row_offset:row_offset + rows]


def cpu_apply(sd, steps):
    """A copy of the CPU bf16 state dict ``sd`` with ``steps`` applied in order.  A step is
    (param, row_offset, rows, "lora", up, down, scale) or (param, row_offset, rows, "diff", None, diff, scale), tensors of any float
    dtype (widened exactly)."""
    out = {k: v.detach().cpu().clone() for k, v in sd.items()}
    for param, row_offset, rows, kind, up, down, scale in steps:
        w = window(out[param], row_offset, rows)
        if kind == "lora":
            w.copy_(cpu_merge(w.contiguous(), up.float(), down.float(), scale))
        else:
            w.copy_(cpu_add_scaled(w.contiguous(), down.float().reshape(w.shape), scale))
    return out


def bits16(t):
    return t.detach().contiguous().view(torch.int16).cpu()


def same_bf16(got, want, what):
    """bit equality of two bf16 tensors, a NaN compared as NaN-ness"""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype == bf16, what
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f"{what}: NaN in {int((gn != wn).sum())} different places"
    bad = (bits16(got) != bits16(want)) & ~wn
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} values differ, first at flat index {int(bad.flatten().nonzero()[0])}"


def bf16_ulp(x):
    """the spacing of bf16 at |x| (fp64 tensor of normal values): 2^(floor(log2 |x|) - 7)"""
    return torch.exp2(torch.floor(torch.log2(x.abs())) - 7.0)


def gamma(n):
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


assert math.isclose(gamma(1), 2.0 ** -24, rel_tol=1e-6)
