"""The timing ablations of the generated kernels (scail_amd/asmgen/gemm4.py, attn4.py variant_cfgs(): the shipped schedule with an instruction
class of its inner loop removed) exist in the measurement build only and compute wrong results on purpose, so no result is compared.  What a
tool that times them relies on is checked: the knob selects the kernel (the name queries report its symbol), the launch succeeds at the smallest
shape the dispatch gives to a generated kernel, the stream synchronises, and the kernel writes nowhere but into its M x N / Lq x 128 output --
the guard rows behind the output keep their sentinel."""
import pytest
import torch

import attn_exact as AX
import gemm_exact as G
from scail_amd.asmgen import attn4, gemm4

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x5A5A          # bf16 bits of the output buffer before the launch
GUARD_ROWS = 64


@pytest.fixture(autouse=True)
def measurement_build():
    from scail_amd import lib as L
    if not L.ABLATIONS:
        pytest.skip("kernels of the measurement build (run with SCAIL_ABLATIONS=1)")


def _guarded(rows, cols):
    """(rows + GUARD_ROWS, cols) of sentinel bits; returns the whole buffer (int16) and the bf16 view of its first `rows` rows"""
    buf = torch.full((rows + GUARD_ROWS, cols), SENTINEL, device=DEV, dtype=torch.int16)
    return buf, buf.view(torch.bfloat16)[:rows]


def _guard_intact(buf, rows):
    return bool((buf[rows:] == SENTINEL).all())


@pytest.mark.parametrize("name", [c.name for c in gemm4.variant_cfgs()])
def test_gemm4_timing_ablation_launches_and_stays_inside_its_output(name):
    from scail_amd import lib as L, ops
    M, N, K = 2048, 256, 128
    assert name.startswith("scail_gemm4_e0_")
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, device=DEV, generator=g)
    buf, y = _guarded(M, N)
    L.tune_set("gemm4_kernel:" + name[len("scail_gemm4_e0_"):], 0)
    try:
        assert G.kernel_name(K, N, 0, M, N, K, L.EPI_BIAS, False) == name
        ops.gemm(x, w, bias, out=y)                 # raises unless scail_gemm_bf16 returns 0
        torch.cuda.synchronize()
        assert _guard_intact(buf, M)
    finally:
        L.tune_set("gemm4_kernel", 0)
    assert G.kernel_name(K, N, 0, M, N, K, L.EPI_BIAS, False) == "scail_gemm4_e0"


@pytest.mark.parametrize("name", [c.name for c in attn4.variant_cfgs()])
def test_attn4_timing_ablation_launches_and_stays_inside_its_output(name):
    from scail_amd import lib as L, ops
    Lq, Lk, D = 256, 512, 128                       # one (batch, head) pair, one 256-row workgroup, 8 key tiles
    assert name.startswith("scail_attn4_")
    g = torch.Generator(device=DEV).manual_seed(2)
    q = (torch.randn(1, Lq, D, device=DEV, generator=g) * ops.ATTN_LOG2_SCALE).to(torch.bfloat16)
    k = torch.randn(1, Lk, D, device=DEV, generator=g).to(torch.bfloat16)
    v = torch.randn(1, Lk, D, device=DEV, generator=g).to(torch.bfloat16)
    vt = ops.transpose_v(v, 1)
    buf, o = _guarded(Lq, D)
    L.tune_set("attn4_kernel:" + name[len("scail_attn4_"):], 0)
    try:
        assert AX.kernel_name(D, D, D, 1, 1, Lq, Lk, False, True) == name
        ops.flash_attn(q, k, vt, out=o.view(1, Lq, D), q_prescaled=True)      # raises unless scail_flash_attn_bf16 returns 0
        torch.cuda.synchronize()
        assert _guard_intact(buf, Lq)
    finally:
        L.tune_set("attn4_kernel", 0)
    assert AX.kernel_name(D, D, D, 1, 1, Lq, Lk, False, True) == AX.GEN
