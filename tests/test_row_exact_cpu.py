"""The conditions tests/test_row_exact_gpu.py rests on, checked without a GPU (tests/row_exact.py): for every GPU case the undecided share of its fp64
reference stays under the cap and its rows stay inside the value ranges the margin's derivation assumes; the kernels' chains restated in IEEE fp32
(torch on the CPU), in block order and in wave order, pass the checker; every seeded fault of the restatement is rejected, on the case named next to it;
and scail_row_kernel_name_for, which needs no device for the name, sends every case to the kernel it is meant to run."""
import pytest
import torch

import row_exact as E

LN_IDS = [c["id"] for c in E.LN_CASES]
RMS_IDS = [c["id"] for c in E.RMS_CASES]


def _margin_for(c, inp, kind):
    """reference and margin for the summation order ``kind`` (the shared ones are for the case's own kernel)"""
    own = "block" if c["kind"].startswith("block") else "wave"
    if kind == own:
        return inp["ref"], inp["margin"]
    A = E.depth(kind, c["D"])
    if "form" in c:
        ref, m = E.ln_reference(inp["X"], _mult(c, inp), inp["add"], c["eps"], A)
    elif c["rope"]:
        ref, m = E.rms_reference(inp["x"], inp["w"], E.f32(E.EPS), A, inp["cos"], inp["sin"], torch.arange(inp["rows"]) % inp["rpb"], c["hd"], c["out_scale"])
    else:
        ref, m = E.rms_reference(inp["x"], inp["w"], E.f32(E.EPS), A, out_scale=c["out_scale"])
    assert torch.equal(ref, inp["ref"])
    return ref, m


def _mult(c, inp):
    rows = inp["X"].shape[0]
    if c["form"] == "mod":
        return (1.0 + inp["scale"].double())[torch.arange(rows) // inp["rows_out"]]
    return inp["w"].double()[None].expand(rows, c["D"])


def _conditions(X, what):
    """what the derivation assumes of a row: finite bf16 values, squares and sums far from fp32's overflow and flush-to-zero ranges"""
    a = X.double().abs()
    assert bool(torch.isfinite(a).all())
    assert float(a.max()) <= 2.0 ** 14, what                      # sum of 6144 squares below 2^41
    nz = a[a > 0]
    assert float(nz.min()) >= 2.0 ** -40, what                    # squares above 2^-80: no denormal anywhere on the chain


@pytest.mark.parametrize("id", LN_IDS)
def test_layernorm_case_conditions_and_fp32_restatement(id):
    c = E.case_of(id)
    inp = E.ln_inputs(c)
    _conditions(inp["X"], id)
    if c["loops"]:
        assert inp["rows_out"] > 4 * max(1, min((inp["rows_out"] + 3) // 4, (3 * E.NOMINAL_CUS + inp["n_batch"] - 1) // inp["n_batch"]))
    for kind in ("block", "wave"):
        ref, m = _margin_for(c, inp, kind)
        fig = E.check_case(E.ln_fp32(c, inp, kind), ref, m, inp["n_special"], f"{id} [fp32 restatement, {kind} order]")
        assert fig["share"] <= E.UNDECIDED_CAP
    k = inp["X"].shape[0] - E.N_SPECIAL                            # the all-zero row: the addend, bit for bit, whatever the margin says
    want = E.rne_bf16(inp["add"][k]).float().to(E.BF16)
    E.assert_bits(E.ln_fp32(c, inp, "block")[k], want, id + " zero row")


@pytest.mark.parametrize("id", RMS_IDS)
def test_rmsnorm_case_conditions_and_fp32_restatement(id):
    c = E.case_of(id)
    inp = E.rms_inputs(c)
    _conditions(inp["x"], id)
    if c["rope"]:
        cf, sf = inp["cos_full"].double(), inp["sin_full"].double()
        assert torch.stack((cf.flatten(), sf.flatten()), 1).unique(dim=0).shape[0] == cf.numel(), "every (token, pair) has its own angle, as fp32 (cos, sin)"
        assert float((sf.abs() < 0.05).double().mean()) < 0.05 and float((cf.abs() < 0.05).double().mean()) < 0.05      # the full circle, not a cluster at the identity
        assert float((cf * cf + sf * sf - 1).abs().max()) < 1e-6
    for kind in ("block", "wave"):
        ref, m = _margin_for(c, inp, kind)
        E.check_case(E.rms_fp32(c, inp, kind), ref, m, inp["n_special"], f"{id} [fp32 restatement, {kind} order]")
    k = inp["rows"] - E.N_SPECIAL
    assert float(E.rms_fp32(c, inp, "wave")[k].float().abs().max()) == 0.0, "zero row"


# every seeded fault, and the case on which the checker must reject it
LN_FAULT_CASES = [
    ("variance over D - 1", "ln-mod-block-264"), ("variance over D - 1", "ln-aff-wave-6144"),          # 1 / (2 D): 1.9e-3 and, the smallest, 8.1e-5
    ("eps 1e-5", "ln-mod-wave-1536"), ("eps dropped", "ln-mod-wave-1536"),                               # (seen on the 2^-10 rows)
    ("eps 1e-5", "ln-aff-block-8"), ("eps dropped", "ln-aff-block-4104"),
    ("chunk left out of the mean", "ln-mod-wave-1536"), ("chunk left out of the mean", "ln-aff-block-6144"),
    ("chunk left out of the sum of squares", "ln-mod-wave-6144"), ("chunk left out of the sum of squares", "ln-aff-block-4104"),
    ("scale instead of 1 + scale", "ln-mod-block-264"), ("scale instead of 1 + scale", "ln-mod-wave-5120"),
    ("batch 0's modulation", "ln-mod-block-table2-slice-ldx"), ("batch 0's modulation", "ln-mod-wave-table6-slice-ldx"),
    ("src_row_offset ignored", "ln-mod-wave-table6-slice-ldx"), ("src_row_offset ignored", "ln-mod-block-table2-slice-ldx"),
    ("truncate", "ln-mod-wave-2048"), ("truncate", "ln-aff-block-1280"),
    ("output row unwritten", "ln-mod-wave-4096"), ("output row unwritten", "ln-aff-block-2056"),
]
RMS_FAULT_CASES = [
    ("sine sign flipped", "rms-wave-1536-hd128"), ("sine sign flipped", "rms-block-1280-hd80"),
    ("pair index shifted by one chunk", "rms-block-256-hd64"), ("pair index shifted by one chunk", "rms-wave-2048-hd256"),
    ("table row r", "rms-wave-batch3"), ("table row r", "rms-block-batch3"),
    ("table row r + 1", "rms-wave-1536-hd128"), ("table row r + 1", "rms-block-128-hd128"),
    ("HD128 shortcut at another head_dim", "rms-wave-1536-hd64"), ("HD128 shortcut at another head_dim", "rms-wave-1536-hd96"),
    ("out_scale after a bf16 rounding", "rms-wave-row0"), ("out_scale after a bf16 rounding", "rms-block-5120-norope-scaled"),
    ("truncate", "rms-wave-4096-hd128"), ("truncate", "rms-block-4096-norope"),
    ("eps dropped", "rms-wave-6144-hd128"), ("chunk left out of the sum of squares", "rms-wave-6144-hd128"),
    ("chunk left out of the sum of squares", "rms-block-4104-hd216"),
]


def test_every_fault_of_the_issue_is_seeded():
    assert {f for f, _ in LN_FAULT_CASES} == set(E.LN_FAULTS) and {f for f, _ in RMS_FAULT_CASES} == set(E.RMS_FAULTS)


@pytest.mark.parametrize("fault,id", LN_FAULT_CASES)
def test_layernorm_fault_is_rejected(fault, id):
    c = E.case_of(id)
    inp = E.ln_inputs(c)
    got = E.ln_fp32(c, inp, c["kind"], fault)
    with pytest.raises(AssertionError):
        E.check_case(got, inp["ref"], inp["margin"], inp["n_special"], f"{id} [{fault}]")


@pytest.mark.parametrize("fault,id", RMS_FAULT_CASES)
def test_rmsnorm_rope_fault_is_rejected(fault, id):
    c = E.case_of(id)
    inp = E.rms_inputs(c)
    got = E.rms_fp32(c, inp, "block" if c["kind"].startswith("block") else "wave", fault)
    with pytest.raises(AssertionError):
        E.check_case(got, inp["ref"], inp["margin"], inp["n_special"], f"{id} [{fault}]")


def test_regular_rows_alone_reject_the_arithmetic_faults():
    """without the special rows: variance over D - 1 fails on the regular rows of the largest D by thousands of elements"""
    c = E.case_of("ln-aff-wave-6144")
    inp = E.ln_inputs(c)
    k = inp["X"].shape[0] - E.N_SPECIAL
    got = E.ln_fp32(c, inp, "wave", "variance over D - 1")
    lo, hi = E.rne_bf16(inp["ref"] - inp["margin"])[:k], E.rne_bf16(inp["ref"] + inp["margin"])[:k]
    g = got[:k].double()
    assert int(((g < lo) | (g > hi)).sum()) > 1000


def test_checker_interval_rule():
    """the rule itself: the RNE value passes with margin 0, its neighbour only when the margin reaches the rounding boundary, a second neighbour never"""
    ref = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -20, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0], dtype=torch.float64)      # just below / above a boundary; exact
    rne = torch.tensor([1.0, 1.0 + 2.0 ** -7, -3.0]).to(E.BF16)
    other = torch.tensor([1.0 + 2.0 ** -7, 1.0, -3.0]).to(E.BF16)
    zero = torch.zeros(3, dtype=torch.float64)
    assert E.check_margin_bf16(rne, ref, zero) == (0.0, 0)
    with pytest.raises(AssertionError):
        E.check_margin_bf16(other, ref, zero)
    with pytest.raises(AssertionError):
        E.check_margin_bf16(other, ref, zero + 2.0 ** -21)
    share, allowed = E.check_margin_bf16(other, ref, zero + 2.0 ** -19)
    assert abs(share - 2 / 3) < 1e-12 and allowed == 2
    with pytest.raises(AssertionError):
        E.check_margin_bf16(torch.tensor([1.0 + 2.0 ** -6, 1.0, -3.0]).to(E.BF16), ref, zero + 2.0 ** -19)
    with pytest.raises(AssertionError):
        E.check_margin_bf16(torch.tensor([float("nan"), 1.0, -3.0]).to(E.BF16), ref, zero + 1.0)


def test_reference_on_the_models_tables_is_the_oracles_rope():
    """the one case on the oracle's rope_tables, cos[:, 0::2] as the executor passes them: row_exact's reference is the oracle's RMSNorm + apply_rope"""
    from oracle import scail_oracle as O
    cos, sin = O.rope_tables(O.DiTConfig(hidden_size=1536, num_attention_heads=12, latent_height=32, latent_width=32, num_frames=13), 3, 6, 4)
    assert torch.equal(cos[:, 0::2], cos[:, 1::2]) and torch.equal(sin[:, 0::2], sin[:, 1::2])
    ref, margin, x, w = E.table_case(cos[:, 0::2].contiguous(), sin[:, 0::2].contiguous(), 1536)
    want = O._merge(O.apply_rope(O._heads(O.rms_norm(x.float()[None], w, 1e-6), 12), cos, sin))[0]
    assert float((ref - want.double()).abs().max()) < 1e-4
    share, _ = E.check_margin_bf16(E.rne_bf16(ref).float().to(E.BF16), ref, margin, "rms-wave-oracle-tables [reference]")
    assert share <= E.UNDECIDED_CAP


@pytest.mark.parametrize("act_in,act_out", [(1, 0), (2, 0), (0, 1), (0, 2), (1, 1)])
@pytest.mark.parametrize("K", [8, 520])
def test_small_linear_margin_holds_for_an_fp32_restatement(K, act_in, act_out):
    import gemm_exact
    x, w, b, ref, margin = E.small_linear_act_case(8, 5, K, act_in, act_out)
    act = {0: lambda v: v, 1: lambda v: v / (1.0 + torch.exp2(v * torch.tensor(-1.4426950408889634))), 2: gemm_exact.gelu_tanh_hip_fp32}
    y = act[act_out](act[act_in](x) @ w.float().t() + b[None])
    assert bool(((y.double() - ref).abs() <= margin).all())
    assert not bool(((act[act_out]((act[act_in](x) * (1 + 2e-5)) @ w.float().t() + b[None]).double() - ref).abs() <= margin).all()), "a 2e-5 error is seen"


def test_small_linear_integer_operands_are_exact():
    for M, N, K in ((1, 5, 8), (8, 64, 1032)):
        x, w, b, y64 = E.small_linear_operands(M, N, K)
        assert float((x.double().abs() @ w.double().abs().t()).max()) + 8 < 2 ** 24
        assert torch.equal((x @ w.float().t() + b[None]).double(), y64)


# ---- the route: the name needs no device ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from scail_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


@pytest.mark.parametrize("id", LN_IDS + RMS_IDS)
def test_case_runs_the_kernel_it_is_meant_to(lib, id):
    c = E.case_of(id)
    if "form" in c:
        inp = E.ln_inputs(c)
        args = (c["form"], inp["n_batch"], inp["rows_out"], c["D"])
    else:
        inp = E.rms_inputs(c)
        args = ("rope" if c["rope"] else "rms", 1, inp["rows"], c["D"], c["hd"])
    assert E.with_options(E.options_of(c), lambda: E.kernel_name(*args)[0]) == E.expected_name(c)


def test_route_boundaries(lib):
    name = lambda *a: E.kernel_name(*a)[0]
    for D in (512, 1024, 2560, 3072, 3584, 5632, 1528, 1544):        # multiples of 512 without an instantiation, and the neighbours of one
        assert name("mod", 2, 9, D) == "ln_kernel<0>" and name("aff", 1, 9, D) == "ln_kernel<1>" and name("rope", 1, 9, D, 8) == "rmsnorm_rope_kernel"
    for D in (1536, 2048, 4096, 5120, 6144):
        assert name("mod", 2, 9, D) == f"ln_wave_kernel<0, {D // 512}>" and name("aff", 1, 9, D) == f"ln_wave_kernel<1, {D // 512}>"
        assert name("rope", 1, 9, D, 128) == f"rmsnorm_rope_wave_kernel<{D // 512}, true>"
        assert name("rope", 1, 9, D, 64) == f"rmsnorm_rope_wave_kernel<{D // 512}, false>"
        assert name("rms", 1, 9, D, 128) == "rmsnorm_rope_kernel" and name("copy", 1, 9, D, 128) == "rmsnorm_rope_kernel"
        assert E.with_options({"row_wave": 0}, lambda: (name("mod", 2, 9, D), name("rope", 1, 9, D, 128))) == ("ln_kernel<0>", "rmsnorm_rope_kernel")
    from scail_amd import lib as L
    with pytest.raises(L.ScailHipError, match="multiple of 8 and <= 6144"):
        E.kernel_name("mod", 1, 1, 6152)
    with pytest.raises(L.ScailHipError, match="unknown form"):
        L.call("scail_row_kernel_name_for", 5, 1, 1, 128, 128, 0x1000, 8, None)
    with pytest.raises(L.ScailHipError, match="head_dim"):
        E.kernel_name("rope", 1, 1, 128, 48)
