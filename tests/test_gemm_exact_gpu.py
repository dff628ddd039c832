"""Every bf16 GEMM kernel scail_gemm_bf16 can pick in a product build -- the 128 tile and the quadrant kernel q8 of csrc/gemm.hip, the generated
scail_gemm4_e0 / _e1 / _e3 / _e4 -- on operands for which fp32 accumulation and the bias / residual / gate epilogues are exact in any order
(tests/gemm_exact.py): bias, NULL bias, ungated residual (aliasing y, and in a separate tensor with ldr != ldc) and gated residual (the gate a column
slice of a (B, 6 N) table, B >= 3, rows per batch no multiple of any tile) bit for bit against the fp64 value rounded once to bf16; GELU-tanh and
GELU-erf correctly rounded wherever fp32 arithmetic can decide it (check_budget_bf16 with the derived budget B(v)).  Every case first asserts what
scail_gemm_kernel_name_for says the call runs -- the query and the launch share gemm_choose, so this pins the ROUTE; that launch_gemm maps the choice to
the instantiation of that name is not visible by name, and bit-equal results cannot show it either --, reads x as a column slice of a wider NaN-filled tensor (lda > K), writes into a NaN-filled tensor with
ldc > N and a guard row, and asserts that nothing outside M x N changed and nothing inside stayed NaN.  Where a second route accepts the case (option
"gemm4" = 0) it runs too, and for the exact epilogues the two give equal bits.  With SCAIL_ABLATIONS=1 the same cases run on the forced tiles 256, 257,
260, 261 and 262 of the measurement build.  tests/test_gemm_exact_cpu.py proves that these checks reject truncation, ties away from zero, a dropped
k-element, a k-tile added twice, a bias added after the rounding, a neighbouring batch's gate row, a transposed result and a GELU constant off by 2^-16.

Out of scope: the plain 256 tile with LDS-DMA as a PRODUCT route -- scail_gemm_bf16 picks it only for a big shape whose lda exceeds about 4 M elements
(q8's 2 GB buffer descriptor), which no small test can allocate; the forced tile 257 runs the same instantiation in the measurement build."""
import functools

import pytest
import torch

import gemm_exact as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(params=[0, 256, 257, 260, 261, 262])
def gemm_tile(request):
    """0 = the product dispatch (by shape).  The forced tile instantiations exist only in the measurement build (SCAIL_ABLATIONS=1,
    include/scail_hip_ablation.h) and are skipped without it."""
    from scail_amd import lib as L
    if request.param == 0:
        yield 0
        return
    if not L.ABLATIONS:
        pytest.skip("kernel variant of the measurement build (run with SCAIL_ABLATIONS=1)")
    L.tune_set("gemm_tile", request.param)
    yield request.param
    L.tune_set("gemm_tile", 0)


@functools.lru_cache(maxsize=2)
def _device_operands(id, gelu):
    """x as columns [64, 64 + K) of a NaN-filled (M, K + 64) tensor, w, bias, the residual and the gate table on the device: uploaded once per case"""
    case = G.case_of(id)
    o = G._operands(id, gelu)
    xbig = torch.full((case["M"], case["K"] + 64), NAN, dtype=torch.bfloat16)
    xbig[:, 64:] = o["x"].to(torch.bfloat16)
    return dict(x=xbig.to(DEV)[:, 64:], w=o["w"].to(torch.bfloat16).to(DEV), bias=o["bias"].to(DEV), resid=o["resid"].to(torch.bfloat16).to(DEV),
                table=o["table"].to(DEV))


def _run(case, form, name):
    """one launch under the options in force, after asserting that it is kernel ``name``; returns the whole (M + 1, N + 8) output tensor on the CPU"""
    from scail_amd import ops
    M, N, K = case["M"], case["N"], case["K"]
    d = _device_operands(case["id"], form in G.GELU_FORMS)
    o = G.operands(case, form)
    ldc = N + 8
    ybig = torch.full((M + 1, ldc), NAN, dtype=torch.bfloat16, device=DEV)      # one guard row, 8 guard columns
    y = ybig[:M, :N]
    kw, ldr = {}, 0
    if form in ("resid_alias", "gated"):
        y.copy_(d["resid"])
        kw, ldr = dict(resid=y), ldc
    if form == "resid_sep":
        rbig = torch.full((M, N + 16), NAN, dtype=torch.bfloat16, device=DEV)
        rbig[:, :N] = d["resid"]
        kw, ldr = dict(resid=rbig[:, :N]), N + 16
    if form == "gated":
        kw.update(gate=d["table"][:, 2 * N:3 * N], rows_per_batch=o["rpb"])
    assert d["x"].stride(0) == K + 64 and y.stride(0) == ldc
    got = G.kernel_name(K + 64, ldc, ldr, M, N, K, G.EPI_OF[form], form == "gated")
    assert got == name, (case["id"], form, got)
    ops.gemm(d["x"], d["w"], None if form == "nobias" else d["bias"], out=y, epilogue=G.EPI_OF[form], **kw)
    return ybig.cpu()


def _check(case, form, ybig, what):
    """the exact forms bit for bit, the GELUs by budget; nothing outside M x N written, nothing inside left NaN.  Returns the undecided share (GELU)"""
    M, N = case["M"], case["N"]
    ref, budget = G.reference(case, form)
    if budget is None:
        want = torch.full(tuple(ybig.shape), NAN, dtype=torch.bfloat16)
        want[:M, :N] = G.round_bf16(ref)
        G.assert_bits(ybig, want, what)
        print(f"{what}: bit-exact, {M * N} elements")
        return None
    assert bool(torch.isnan(ybig[M].float()).all()) and bool(torch.isnan(ybig[:, N:].float()).all()), f"{what}: written outside the M x N result"
    share = G.check_budget_bf16(ybig[:M, :N].contiguous(), ref, budget, what)
    assert share <= G.UNDECIDED_CAP, share
    return share


@pytest.mark.parametrize("id,form", G.CASE_FORMS, ids=[f"{i}-{f}" for i, f in G.CASE_FORMS])
def test_gemm_exact(gemm_tile, id, form):
    from scail_amd import lib as L
    L.load()
    case = G.case_of(id)
    name = G.expected_name(case, form, gemm_tile)
    ybig = G.with_options(case["opts"], lambda: _run(case, form, name))
    _check(case, form, ybig, f"{id} {form}: {name}")
    other = G.other_route(case, form)
    if other is None or gemm_tile:
        return
    ybig2 = G.with_options(other[0], lambda: _run(case, form, other[1]))
    assert other[1] != name
    _check(case, form, ybig2, f"{id} {form}: {other[1]} (the other route)")
    if form in G.EXACT_FORMS:                      # (the two GELU-tanh chains differ by design: each is held to the budget)
        assert torch.equal(ybig.view(torch.int16)[:case["M"], :case["N"]], ybig2.view(torch.int16)[:case["M"], :case["N"]]), "the two routes give equal bits"
