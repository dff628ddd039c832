"""The operands, references and checkers of tests/gemm_exact.py, proven on the CPU before a GPU sees them: fp32 accumulation of the operands is exact
in any order, and so is the gated residual epilogue as mul + add; every case of tests/test_gemm_exact_gpu.py really exercises the rounding (truncation
and round-to-nearest-even differ on >= 10 % of its outputs, an exact tie whose even and away roundings differ is present) or, for the GELUs, keeps the
undecided share under its cap with enough negative pre-activations, and an IEEE fp32 restatement of each kernel chain passes; the checks reject
truncation, ties away from zero, one dropped k-element, one k-tile added twice, a bias added after the rounding, the gate row of the neighbouring batch
at a batch boundary, a transposed result and a GELU whose input constant (sqrt(2 / pi), 1 / sqrt 2) is off by 2^-16 = 256 u; the generated kernels scail_gemm4_e0 / _e3 / _e4 are bit-identical to
the reference in the CPU emulator and _e1 is inside the budget; and scail_gemm_kernel_name_for answers as expected on both sides of every boundary of
the route (a host-only query).  Needs no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_exact as G

CASE_IDS = [c["id"] for c in G.CASES]


def _bits_stats(ref64):
    """(share of elements where truncation and RNE differ, number of exact ties whose even and away roundings differ) of EXACT fp32 values, from
    the fp32 bit pattern: the 16 bits bf16 drops, and the last bit it keeps"""
    f = ref64.float()
    assert torch.equal(f.double(), ref64)
    b = f.contiguous().view(torch.int32)
    low, odd = b & 0xFFFF, ((b >> 16) & 1) == 1
    up = (low > 0x8000) | ((low == 0x8000) & odd)
    return float(up.double().mean()), int(((low == 0x8000) & ~odd).sum())


# ---- the helpers -------------------------------------------------------------------------------------------------------------------------
def test_one_step_rounding_helpers():
    g = torch.Generator().manual_seed(0)
    v = torch.randn(100000, generator=g, dtype=torch.float64) * torch.exp(torch.randn(100000, generator=g, dtype=torch.float64) * 8)
    v[:5] = torch.tensor([0.0, 1.00390625, -1.01171875, 3.0, -0.0], dtype=torch.float64)
    lo, hi, _ = G.bf16_neighbours(v)
    a = v.abs()
    assert torch.equal(G.rne_bf16(v), G.rne_bf16_slow(v)) and torch.equal(G.truncate_bf16(v), lo)
    assert torch.equal(G.away_bf16(v), torch.where(a - lo.abs() < hi.abs() - a, lo, hi))
    x = torch.randint(-2 ** 20, 2 ** 20, (100000,), generator=g).double() / 64            # exact in fp32: the two-step rounding is right
    assert torch.equal(G.rne_bf16(x), G.round_bf16(x).double())
    st = _bits_stats(x)
    assert st[0] == float((G.truncate_bf16(x) != G.rne_bf16(x)).double().mean()) and st[1] == G.even_away_ties(x) > 0
    t = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30], dtype=torch.float64)                  # through fp32 this becomes a tie and goes to even: 1.0
    assert float(G.rne_bf16(t)) == 1.0078125 and float(G.round_bf16(t)) == 1.0


def test_budget_is_derived_not_measured():
    assert G.SLACK == 2.0 and G.UNDECIDED_CAP == 0.05 and G.V_ABS_MAX == 8.0 and G.U == 2.0 ** -24
    v = torch.linspace(-8, 8, 1601, dtype=torch.float64)
    Uv = G.K0 * (v + G.K1 * v ** 3)
    s = torch.sigmoid(2 * Uv)
    ref = G.gelu_tanh64(v)
    assert torch.allclose(ref, 0.5 * v * (1 + torch.tanh(Uv)), rtol=0, atol=1e-14) and torch.allclose(G.gelu_erf64(v), 0.5 * v * (1 + torch.erf(v / 2 ** 0.5)), rtol=0, atol=1e-14)
    hip = v.abs() * (1 - s) * (2 + s * (2 + 18 * Uv.abs())) + 0.5 * v.abs() * (2 * s + (2 * s - 1).abs()) + ref.abs()      # the two chains of the docstring
    e1 = v.abs() * (1 - s) * (3 + s * (2 + 8 * Uv.abs())) + ref.abs()
    assert bool((G.budget_tanh(v) >= G.SLACK * G.U * torch.maximum(hip, e1) * (1 - 1e-12)).all())
    z = v / 2 ** 0.5
    erf = 0.5 * v.abs() * (torch.special.erfc(-z) + 32 * torch.erf(z).abs() + 4 / np.pi ** 0.5 * z.abs() * torch.exp(-z * z)) + G.gelu_erf64(v).abs()
    assert torch.allclose(G.budget_erf(v), G.SLACK * G.U * erf, rtol=1e-12, atol=0)
    # the cancellation: at v = -4 the budget is absolute -- thousands of u relative to the reference
    assert float(G.budget_erf(v[400:401]) / G.gelu_erf64(v[400:401]).abs()) > 1e4 * G.U and float(v[400]) == -4.0


@pytest.mark.parametrize("id", ["t128-77x72x13824", "t128-300x136x128"])
def test_fp32_accumulation_is_exact_in_any_order(id):
    case = G.case_of(id)
    o = G.operands(case, "bias")
    M, K = case["M"], case["K"]
    want = G.dot64(o["x"], o["w"])
    for width in (16, 32, 64):
        for reverse in (False, True):
            acc = torch.zeros(M, case["N"], dtype=torch.float32)
            for k0 in list(range(0, K, width))[::-1 if reverse else 1]:
                acc = acc + o["x"][:, k0:k0 + width] @ o["w"][:, k0:k0 + width].t()
            assert torch.equal(acc.double(), want), (width, reverse)
    v = acc + o["bias"]
    gate = G.gate_rows(o, M).float()
    assert torch.equal(v.double(), G.value64(want, o, "bias"))
    assert torch.equal((o["resid"] + v).double(), G.value64(want, o, "resid_sep"))
    prod = gate * v                                                           # mul + add in fp32; the fma has the same, exact, value
    assert torch.equal(prod.double(), gate.double() * v.double()) and torch.equal((o["resid"] + prod).double(), G.value64(want, o, "gated"))
    half_units = G.value64(want, o, "gated").abs().max() * 2.0 ** (6 + o["s"])
    assert float(half_units) < 2 ** 24 and float(half_units) == int(half_units)


# ---- the conditions on every case's inputs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", CASE_IDS)
def test_every_case_exercises_rounding(id):
    case = G.case_of(id)
    for form in case["forms"]:
        ref, budget = G.reference(case, form)
        if budget is None:
            differ, ties = _bits_stats(ref)
            print(f"{id} {form}: truncation != RNE on {differ:.1%}, {ties} even / away ties")
            assert differ >= 0.10 and ties >= 1, (form, differ, ties)
            continue
        v = G.pre_activation(case, form)
        assert float(v.abs().max()) <= G.V_ABS_MAX and float((v < -1).double().mean()) >= 0.10, "v of O(1), with negative values for the cancellation"
        chains = [G.gelu_tanh_hip_fp32, G.gelu_tanh_e1_fp32] if form == "gelu_tanh" else [G.gelu_erf_fp32]
        for chain in chains:
            share = G.check_budget_bf16(chain(v).to(G.BF16), ref, budget, f"{id} {form} ({chain.__name__}, IEEE fp32)")
            assert share <= G.UNDECIDED_CAP, share


# ---- the checks reject wrong results -----------------------------------------------------------------------------------------------------
def _fails(bad64, ref64, what, pattern="differ"):
    with pytest.raises(AssertionError, match=pattern):
        G.assert_bits(bad64.float().to(G.BF16), G.round_bf16(ref64), what)


@pytest.mark.parametrize("id", CASE_IDS)
def test_checkers_reject_the_faults(id):
    case = G.case_of(id)
    M, N, K = case["M"], case["N"], case["K"]
    for form in case["forms"]:
        o = G.operands(case, form)
        ref, budget = G.reference(case, form)
        if budget is not None:
            v = G.pre_activation(case, form)
            off = 1 - 2.0 ** -16                                                  # the chain's input constant off by 256 u: a few times the budget
            cut = G.gelu_tanh_hip_fp32(v, k0=0.7978845608028654 * off) if form == "gelu_tanh" else G.gelu_erf_fp32(v, c=0.7071067811865476 * off)
            with pytest.raises(AssertionError, match="not the correctly rounded"):
                G.check_budget_bf16(cut.to(G.BF16), ref, budget, f"{id} {form}: input constant off by 2^-16")
            with pytest.raises(AssertionError, match="not the correctly rounded"):
                G.check_budget_bf16(G.truncate_bf16(ref).float().to(G.BF16), ref, budget, f"{id} {form}: truncated")
            continue
        G.assert_bits(G.rne_bf16(ref).float().to(G.BF16), G.round_bf16(ref), "the reference itself")
        _fails(G.truncate_bf16(ref), ref, f"{id} {form}: truncation")
        _fails(G.away_bf16(ref), ref, f"{id} {form}: ties away from zero")
        sq = min(M, N)
        t = ref.clone()
        t[:sq, :sq] = ref[:sq, :sq].t()
        _fails(t, ref, f"{id} {form}: transposed")
        if form == "bias":
            acc = ref - o["bias"].double()
            m = M - 1                                                             # the last row of the ragged last tile; the column where one product weighs most
            big = (o["x"][m].double() * o["w"].double()).abs().max(dim=1).values / G.bf16_neighbours(ref[m])[2]
            n = int(big.argmax())
            terms = o["x"][m].double() * o["w"][n].double()
            k = int(terms.abs().argmax())
            assert float(big[n]) >= 1, "one product survives the rounding only where it is at least one bf16 step"
            bad = ref.clone()
            bad[m, n] -= terms[k]
            _fails(bad, ref, f"{id}: one dropped k-element", "1 of .* elements differ")
            kt = (K // 64 - 1) * 64                                               # the last k-tile once more, on the odd rows of every 32
            twice = o["x"][:, kt:kt + 64].double() @ o["w"][:, kt:kt + 64].double().t()
            twice[(torch.arange(M) // 16) % 2 == 0] = 0
            _fails(ref + twice, ref, f"{id}: one k-tile added twice")
            if case["kind"] == "random":                                          # (the identity-like products are bf16 values: nothing is rounded before the bias)
                _fails(G.rne_bf16(acc) + o["bias"].double(), ref, f"{id}: bias added after the rounding")
        if form == "gated":
            m = o["rpb"]                                                          # the first row of batch 1 takes batch 0's gate
            assert not torch.equal(o["gate"][0], o["gate"][1])
            bad = ref.clone()
            bad[m] = o["resid"][m].double() + o["gate"][0].double() * (o["x"][m].double() @ o["w"].double().t() + o["bias"].double())
            _fails(bad, ref, f"{id}: the neighbouring batch's gate row at a batch boundary")


def test_an_identity_like_x_shows_the_transposed_weight():
    case = G.case_of("t128-identity")
    o = G.operands(case, "bias")
    ref, _ = G.reference(case, "bias")
    K = case["K"]
    assert torch.equal(ref, 1.75 * o["w"].double().t()[torch.arange(case["M"]) % K] + o["bias"].double())
    assert not torch.equal(o["w"][:K, :K], o["w"][:K, :K].t())


# ---- the generated kernels in the CPU emulator -------------------------------------------------------------------------------------------
# ragged m-tile with the smallest legal tail (264 = 256 + 8 rows, or the 8 rows alone), 2 / 3 / 5 k-tiles, two n-tiles, lda > K, NULL bias, 3 gate
# batches of 88 rows (no multiple of 32)
EMU_CASES = [("scail_gemm4_e0", (264, 256, 128), dict(bias=False, lda=128 + 64)),
             ("scail_gemm4_e0", (8, 512, 320), dict(bias=True, lda=None)),
             ("scail_gemm4_e1", (264, 256, 192), dict(bias=True, lda=192 + 64)),
             ("scail_gemm4_e3", (264, 256, 192), dict(bias=True, lda=192 + 64)),
             ("scail_gemm4_e3", (8, 512, 128), dict(bias=False, lda=None)),
             ("scail_gemm4_e4", (8, 512, 320), dict(bias=True, lda=320 + 64)),
             ("scail_gemm4_e4", (264, 256, 128), dict(bias=False, lda=None))]


@pytest.mark.parametrize("name,shape,kw", EMU_CASES, ids=[f"{n[-2:]}-{'x'.join(map(str, s))}" for n, s, _ in EMU_CASES])
def test_generated_kernels_exact_in_the_emulator(name, shape, kw):
    from scail_amd.asmgen import gemm4
    from tools import gemm4_emu_run as R
    cfg = next(c for c in gemm4.DEFAULTS if c.name == name)
    M, N, K = shape
    gelu = cfg.epi == 1
    o = G.exact_operands(M, N, K, seed=1000 * cfg.epi + K + M, gelu=gelu)
    if M >= 96:
        assert (M + o["rpb"] - 1) // o["rpb"] >= 3 and o["rpb"] % 32 != 0
    run_kw = dict(bias=o["bias"].numpy() if kw["bias"] else None, lda=kw["lda"])
    if cfg.epi in (3, 4):
        run_kw["resid"] = o["resid"].numpy()
    if cfg.epi == 3:
        run_kw.update(gate=o["gate"].contiguous().numpy(), rows_per_batch=o["rpb"])
    y, _ = R.run(cfg, o["x"].numpy(), o["w"].numpy(), lazy=True, **run_kw)
    got = torch.from_numpy(np.ascontiguousarray(y)).to(G.BF16)
    assert torch.equal(got.float(), torch.from_numpy(np.ascontiguousarray(y))), "the emulator hands back bf16 values"
    form = {0: "bias" if kw["bias"] else "nobias", 1: "gelu_tanh", 3: "gated", 4: "resid_sep"}[cfg.epi]
    acc = G.dot64(o["x"], o["w"])
    if not kw["bias"]:
        o = dict(o, bias=torch.zeros(N))
    v = G.value64(acc, o, form)
    if gelu:
        share = G.check_budget_bf16(got, G.gelu_tanh64(v), G.budget_tanh(v), f"{name} {shape} in the emulator")
        assert share <= G.UNDECIDED_CAP
    else:
        differ, ties = _bits_stats(v)
        assert differ >= 0.10 and ties >= 1
        G.assert_bits(got, G.round_bf16(v), f"{name} {shape} in the emulator")


# ---- the route: scail_gemm_kernel_name_for on both sides of every boundary (host-only queries of the built library) ------------------------
def _library():
    from scail_amd import build
    build.build(verbose=False)
    from scail_amd import lib as L
    return L.load()


B, T, E, R_ = G.EPI_BIAS, G.EPI_GELU_TANH, G.EPI_GELU_ERF, G.EPI_RESID
# (M, N, K, epilogue, gated, kernel, other arguments: lda / ldc / ldr in place of K / N / N-or-0, option gemm4)
ROUTES = [
    (2047, 1024, 128, B, 0, G.T128, {}), (2048, 1024, 128, B, 0, G.GEN, {}),                      # M 2047 / 2048 (8 x 4 = 32 tiles < 128: no small-M branch)
    (2055, 1024, 128, B, 0, G.Q8, {}), (2056, 1024, 128, B, 0, G.GEN, {}),                        # an M tail of 7 / 8 rows
    (2049, 1024, 128, T, 0, G.Q8, {}), (2304, 1024, 128, T, 0, G.GEN, {}),                        # ... of 1 / none
    (2051, 1016, 128, B, 0, G.T128, {}), (2051, 1024, 128, B, 0, G.Q8, {}),                       # N 1016 / 1024 where the generated kernel is out (tail 3)
    (2048, 1032, 128, B, 0, G.Q8, {}), (2048, 1280, 128, B, 0, G.GEN, {}),                        # N % 256
    (2048, 768, 128, B, 0, G.GEN, {}), (2048, 776, 128, B, 0, G.T128, {}), (2048, 264, 128, R_, 1, G.T128, {}),
    (2048, 1024, 64, B, 0, G.Q8, {}), (2048, 1024, 128, R_, 0, G.GEN, {}), (2048, 1024, 128, R_, 1, G.GEN, {}),      # K 64 / 128; ungated e4 / gated e3
    (2048, 256, 64, T, 0, G.T128, {}), (2048, 256, 128, T, 0, G.GEN, {}),
    (2048, 1024, 128, E, 0, G.Q8, {}), (2048, 512, 128, E, 0, G.T128, {}), (4096, 5120, 5120, E, 0, G.Q8, {}),       # GELU-erf: never generated
    # 512 <= M < 2048: generated from 128 tiles of 256 x 256 on.  127 = 127 x 1 is no tile count of fewer than 8 m-tiles: 126 (2 x 63, 7 x 18) and 124 (4 x 31) are the nearest
    (512, 16384, 128, B, 0, G.GEN, {}), (512, 16128, 128, B, 0, G.T128, {}), (1024, 8192, 128, T, 0, G.GEN, {}), (1024, 7936, 128, T, 0, G.T128, {}),
    (1800, 4096, 128, R_, 1, G.GEN, {}), (1792, 4608, 128, R_, 1, G.T128, {}), (511, 32768, 128, B, 0, G.T128, {}), (519, 16384, 128, B, 0, G.T128, {}),
    (520, 16384, 128, B, 0, G.GEN, {}),
    (2048, 1024, 128, B, 0, G.Q8, {"gemm4": 0}), (2048, 512, 128, T, 0, G.T128, {"gemm4": 0}), (512, 16384, 128, B, 0, G.T128, {"gemm4": 0}),      # option "gemm4" off
    (97664, 5120, 5120, R_, 1, G.Q8, {"gemm4": 0}),
    # byte offsets: M ldc / M ldr / 256 lda below 2^31 for the generated kernels; 512 lda + 2 K and 514 K below 2^31 for q8, else the plain 256 tile with LDS-DMA
    (2048, 1024, 128, B, 0, G.GEN, {"ldc": 2 ** 20 - 8}), (2048, 1024, 128, B, 0, G.Q8, {"ldc": 2 ** 20}),
    (2048, 1024, 128, R_, 0, G.GEN, {"ldr": 2 ** 20 - 8}), (2048, 1024, 128, R_, 0, G.Q8, {"ldr": 2 ** 20}),
    (2048, 1024, 128, B, 0, G.GEN, {"lda": 2 ** 22}), (2048, 1024, 128, B, 0, G.T256_DMA, {"lda": 2 ** 23}), (2048, 1024, 128, E, 0, G.Q8, {"lda": 2 ** 22 - 8}),
    (2048, 1024, 128, E, 0, G.T256_DMA, {"lda": 2 ** 22}), (2048, 1032, 128, B, 0, G.T256_DMA, {"lda": 2 ** 22}), (2047, 1024, 128, E, 0, G.T128, {"lda": 2 ** 23}),
]


def test_the_route_table():
    _library()
    from scail_amd import lib as L
    if L.ABLATIONS:
        L.tune_set("gemm_tile", 0)
    for M, N, K, epi, gated, kernel, other in ROUTES:
        opts = {k: v for k, v in other.items() if k in G.OPTION_DEFAULTS}
        lda, ldc, ldr = other.get("lda", K), other.get("ldc", N), other.get("ldr", N if epi == R_ else 0)
        want = kernel.format(e=epi, g=(3 if gated else 4) if epi == R_ else epi)
        got = G.with_options(opts, lambda: G.kernel_name(lda, ldc, ldr, M, N, K, epi, gated))       # (asserts that scail_gemm_kernel_for agrees)
        assert got == want, (M, N, K, epi, gated, other, got)
    buf = C.create_string_buffer(8)
    for args, needle in [((128, 256, 0, 64, 256, 128, 0, 0, buf, 8), "buffer too small"), ((128, 256, 0, 64, 256, 128, 4, 0, buf, 8), "unknown epilogue"),
                         ((128, 256, 0, 64, 256, 96, 0, 0, buf, 8), "multiple of 64"), ((128, 256, 0, 64, 256, 128, 0, 0, None, 8), "null argument")]:
        with pytest.raises(L.ScailHipError, match=needle):
            L.call("scail_gemm_kernel_name_for", *args)


def test_case_table_names_every_product_kernel():
    """what tests/test_gemm_exact_gpu.py asserts before each launch, for the strides it uses, without a GPU"""
    _library()
    from scail_amd import lib as L
    if L.ABLATIONS:
        L.tune_set("gemm_tile", 0)
    named = []
    for case in G.CASES:
        M, N, K = case["M"], case["N"], case["K"]
        for form in case["forms"]:
            ldc = N + 8
            ldr = {"resid_alias": ldc, "gated": ldc, "resid_sep": N + 16}.get(form, 0)
            got = G.with_options(case["opts"], lambda: G.kernel_name(K + 64, ldc, ldr, M, N, K, G.EPI_OF[form], form == "gated"))
            assert got == G.expected_name(case, form), (case["id"], form, got)
            named.append(got)
    if L.ABLATIONS:                                  # the measurement build: every case under every forced tile of the GPU file
        try:
            for tile in G.FORCED:
                L.tune_set("gemm_tile", tile)
                for case in G.CASES:
                    M, N, K = case["M"], case["N"], case["K"]
                    for form in case["forms"]:
                        ldr = {"resid_alias": N + 8, "gated": N + 8, "resid_sep": N + 16}.get(form, 0)
                        got = G.with_options(case["opts"], lambda: G.kernel_name(K + 64, N + 8, ldr, M, N, K, G.EPI_OF[form], form == "gated"))
                        assert got == G.expected_name(case, form, tile), (tile, case["id"], form, got)
        finally:
            L.tune_set("gemm_tile", 0)
    for k in G.KERNELS:
        assert any(n.startswith(k) for n in named), f"no case runs {k}"
    for e in range(4):
        assert G.T128.format(e=e) in named and G.Q8.format(e=e) in named
