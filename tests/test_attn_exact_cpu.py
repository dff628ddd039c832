"""The operands, references, budget and checkers of tests/attn_exact.py, proven on the CPU before a GPU sees them: every case of
tests/test_attn_exact_gpu.py has integer scores, keeps the exactness bound (asserted inside attn_exact.reference), is exact in bf16, stays under the
undecided cap and runs the kernel the table names (host-only route queries); the raw scale is found by search; an IEEE fp32 restatement of each kernel
family's chain passes the checker with nothing decided wrong; the checker rejects a dropped key tile, padded keys counted with score 0, a row sum off
by 2^-8 and by 5 %, one doubled weight, V keys in the order scail_transpose_v did not write, a skipped segment, a lost O rescale, truncation, the
cross attention without its bf16 intermediate, accumulate without / with a late old value, and a raw scale applied twice / not at all; and the
generated kernels scail_attn4_m16f (256 and 192 rows) and scail_attn4_x2 are inside the budget with every decided element equal, in the CPU
emulator -- where a +12 spike provably changes nothing in their first pass (reference point = first tile's maximum + 40) and the rescale subroutine
provably executes, on rows held exactly, in the lazy-maximum loop after a restart (instruction counts with and without the lazy rows' +12 key, at
attn4_thr 8, 2 and 0).  Needs no GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import attn_exact as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SELF_CASES = X.W8_CASES + X.G4_CASES


# ---- the inputs of every GPU case -------------------------------------------------------------------------------------------------------
def test_raw_scale_is_found_by_search():
    s = np.float32(X.raw_scale())
    assert np.float32(s * np.float32(1.4426950408889634)) == np.float32(0.125)
    assert abs(float(s) - 0.125 / 1.4426950408889634) < 1e-8
    assert float(np.float32(1.0 / np.sqrt(128.0)) * np.float32(1.4426950408889634)) != 0.125      # (the default scale is no such number)


def test_case_table_covers_what_it_must():
    ids = [c["id"] for c in SELF_CASES] + [c["id"] for c in X.X_CASES]
    assert len(set(ids)) == len(ids)
    g4 = [c for c in X.G4_CASES if c["form"] == "plain" and not c["opts"] and c["n_seg"] == 1]
    assert {c["Lk"] for c in g4} == {512, 576, 832, 1088, 513, 849} and {c["Lq"] for c in g4} == {256, 130, 300, 520}
    assert {(c["B"], c["H"]) for c in g4} == {(1, 1), (2, 2), (1, 3), (2, 4), (3, 3), (2, 6)}
    assert {c["kind"] for c in g4} == {"sparse_q", "sparse_k"} and {c["raw"] for c in g4} == {True, False}
    assert {(c["B"], c["H"], c["Lq"], c["Lk"]) for c in X.W8_CASES} >= {(1, 1, 40, 1), (2, 2, 130, 64), (1, 2, 300, 65), (2, 2, 300, 257), (1, 1, 256, 512)}
    assert {c["form"] for c in X.W8_CASES} == {"plain", "accumulate", "bcast", "strided", "spike"} and any(c["n_seg"] == 3 and c["Lk"] == 100 for c in X.W8_CASES)
    assert {c["opts"].get("attn4_thr", 8) for c in X.G4_CASES if c["form"] == "spike"} == {8, 0, 2}
    assert X.TARGETS[0] < 48 <= X.TARGETS[1] < 96 <= X.TARGETS[2] < 144 <= X.TARGETS[3] < 192 <= X.TARGETS[4] < 256          # the four waves of a 192-row workgroup
    assert {r // 64 for r in X.TARGETS} == {0, 1, 2, 3}                                                                    # ... and of a 256-row one
    assert [r // 64 for r in X.LAZY_ROWS] == [r // 64 for r in X.TARGETS] and [r // 48 for r in X.LAZY_ROWS] == [r // 48 for r in X.TARGETS]
    assert {c["opts"].get("attn4_thr", 8) for c in X.G4_CASES if c["form"] == "restart"} == {8, 0, 2} and all(c["lazy_key"] for c in X.G4_CASES if c["form"] == "restart")
    assert {c["B"] * c["H"] for c in X.G4_CASES} >= {1, 3, 4, 8, 9, 12}                                                    # XCD decode modes 0 (< 8 pairs), 1 (8), 2 (9, 12)


@pytest.mark.parametrize("case", SELF_CASES, ids=lambda c: c["id"])
def test_self_attention_case_inputs(case):
    """integer scores and the exactness bound (asserted by reference()), bf16 operands (asserted by exact_qkv()), the reserved dimensions, the
    undecided cap; the spike is where the docstring says it is"""
    d = X.self_case(case)
    q, k, v, r = d["q"], d["k"], d["v"], d["r"]
    assert float(v.abs().max()) <= 7 and torch.equal(v, v.round())
    qm = 8.0 if case["raw"] else 1.0
    assert set(q.unique().tolist()) <= {-qm, 0.0, qm} and (k.abs().max() <= 1 or case["form"] in ("spike", "restart"))
    s = X._heads(q.double(), case["H"]) @ X._heads(k.double(), case["H"]).transpose(-1, -2) * X.sl2_of(case)
    ordinary = torch.ones(case["Lq"], dtype=torch.bool)
    if case["spike_key"] is not None:
        rows = [t for t in X.TARGETS if t < case["Lq"]]
        ordinary[rows] = False
        lift = 4 * (X.RESTART_C if case["form"] == "restart" else X.SPIKE_C)
        key = case["spike_key"]
        assert key >= 64 and bool((s[:, :, rows, key] == lift).all()) and bool((s[:, :, ordinary, key] == 0).all())
        others = torch.ones(k.shape[1], dtype=torch.bool)
        others[key] = False
        if case["lazy_key"] is not None:
            others[case["lazy_key"]] = False
        assert bool((s[:, :, :, others].abs() <= 4).all()) and bool((s[:, :, rows][..., others].abs() <= 2).all())       # the spike: >= 10 (254) above a target row's maximum
        if case["lazy_key"] is not None:                                                     # the lazy rows: +12 on their key, blind to the restart key and vice versa
            lz, lk = [t for t in X.LAZY_ROWS if t < case["Lq"]], case["lazy_key"]
            rest = torch.ones(case["Lq"], dtype=torch.bool)
            rest[lz] = False
            assert lk > key and lk >= 64 and bool((s[:, :, lz, lk] == 12).all()) and bool((s[:, :, rest, lk] == 0).all()) and bool((s[:, :, lz, key] == 0).all())
            others[lk] = False
            assert bool((s[:, :, lz][..., others].abs() <= 2).all())
            rz, rk = [t for t in X.RISER_ROWS if t < case["Lq"]], lk - X.RISER_BACK             # the riser rows: 0 everywhere, + 4 on their key alone
            assert rk // 64 not in (0, key // 64, lk // 64) and bool((s[:, :, rz, rk] == 4).all())
            others[rk] = False
            rest[rz] = False
            assert bool((s[:, :, rz][..., others] == 0).all()) and bool((s[:, :, rz, lk] == 0).all()) and bool((s[:, :, rz, key] == 0).all())
            ordinary[rz] = ordinary[lz] = False
            assert bool((s[:, :, ordinary, rk] == 0).all()) and bool((s[:, :, lz, rk] == 0).all()) and bool((s[:, :, rows, rk] == 0).all())
            assert {t // 256 for t in lz} <= {t // 256 for t in rows} and {t // 192 for t in lz} <= {t // 192 for t in rows}       # in workgroups that restart
    else:
        assert float(s.abs().max()) <= 4 and (float(s.max() - s.min()) == 8 or case["Lk"] == 1)
    share = X.undecided_share(r["lo"], r["hi"])
    print(f"{case['id']}: undecided share {share:.4%}, widest row span {r['span_max']:.0f} log2 units")
    assert share <= X.UNDECIDED_CAP
    assert bool((r["budget"] >= 0).all()) and bool((r["budget"] <= 64 * X.U * (r["A"] + r["ref"].abs())).all())


@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("case", X.X_CASES, ids=lambda c: c["id"])
def test_cross_attention_case_inputs(case, raw):
    d = X.cross_case(case, raw)
    share = X.undecided_share(d["lo"], d["hi"])
    print(f"{case['id']} raw={raw}: undecided share {share:.4%}")
    assert share <= X.UNDECIDED_CAP
    assert d["k2"].shape[0] == (1 if case["shared2"] else case["B"])


def test_budget_is_derived_not_measured():
    """one key tile, nothing moves: B = SLACK u (2 A + 5 |ref|); a maximum that rises in the last of three tiles adds one v_exp result (2 u) to every
    weight of the first two"""
    assert X.SLACK == 2.0 and X.UNDECIDED_CAP == 0.05 and X.U == 2.0 ** -24
    q, k, v = X.exact_qkv("sparse_q", 1, 1, 40, 64, 5)
    r = X.reference(q, k, v, 1)
    assert torch.allclose(r["budget"], X.SLACK * X.U * (2 * r["A"] + 5 * r["ref"].abs()), rtol=1e-12, atol=0)
    q, k, v = X.exact_qkv("sparse_q", 1, 1, 256, 192, 6, spike=(150, X.SPIKE_C))
    r = X.reference(q, k, v, 1)
    s = q[0].double() @ k[0].double().t()
    rows = [t for t in X.TARGETS if float(s[t, :64].max()) == float(s[t, :128].max())]          # target rows whose maximum rises in the spike's tile alone
    assert len(rows) >= 2
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    w = p / p.sum(-1, keepdim=True)
    c = torch.where(torch.arange(192) < 128, 2.0, 1.0).double()
    want = X.SLACK * X.U * (2 * (w * c) @ v[0].double().abs() + (2 * (w * c).sum(-1, keepdim=True) + 3) * r["ref"][0].abs())
    assert torch.allclose(r["budget"][0, rows], want[rows], rtol=1e-12, atol=0)


# ---- routes (host-only queries) --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SELF_CASES, ids=lambda c: c["id"])
def test_self_attention_routes(case):
    q_rs, k_rs, o_rs = X.strides_of(case)
    acc = case["form"] == "accumulate"
    got = X.with_options({k: v for k, v in case["opts"].items() if k == "attn4"}, lambda: X.flash_route(q_rs, k_rs, o_rs, case["Lq"], case["Lk"], acc, not case["raw"]))
    assert got == case["route"], case["id"]
    if case["route"] == 4:                                                                   # the same inputs on the 8-wave kernel (equal-bits assertion)
        assert X.with_options({"attn4": 0}, lambda: X.flash_route(q_rs, k_rs, o_rs, case["Lq"], case["Lk"], acc, not case["raw"])) == 8


@pytest.mark.parametrize("case", X.X_CASES, ids=lambda c: c["id"])
def test_cross_attention_routes(case):
    D = case["H"] * X.HD
    args = (D, D, D, D, case["Lq"], case["Lk1"], case["Lk2"], case["B"], case["H"])
    assert X.with_options({"cross4": 1}, lambda: X.cross_route(*args)) == case["route"]
    assert X.with_options({"cross4": 0}, lambda: X.cross_route(*args)) == 2


@pytest.mark.parametrize("case", SELF_CASES, ids=lambda c: c["id"])
def test_self_attention_expected_names(case):
    """the name query without a plan (no device), under the case's options; kernel_name asserts that the number query agrees"""
    q_rs, k_rs, o_rs = X.strides_of(case)
    args = (q_rs, k_rs, o_rs, case["B"], case["H"], case["Lq"], case["Lk"], case["form"] == "accumulate", not case["raw"])
    assert X.with_options(case["opts"], lambda: X.kernel_name(*args)) == X.expected_name(case)
    assert X.expected_name(case) == (X.GEN if case["route"] == 4 else X.W8)
    if case["route"] == 4:
        assert X.with_options(dict(case["opts"], attn4=0), lambda: X.kernel_name(*args)) == X.W8


@pytest.mark.parametrize("case", X.X_CASES, ids=lambda c: c["id"])
def test_cross_attention_expected_names(case):
    D = case["H"] * X.HD
    args = (D, D, D, D, case["Lq"], case["Lk1"], case["Lk2"], case["B"], case["H"])
    assert X.with_options({"cross4": 1}, lambda: X.cross_kernel_name(*args)) == X.expected_name(case) == (X.X_GEN if case["route"] == 4 else X.X_HIP)
    assert X.with_options({"cross4": 0}, lambda: X.cross_kernel_name(*args)) == X.X_HIP


def test_expected_decode_modes_of_the_named_cases():
    """what tests/test_attn_exact_gpu.py holds the plan's xcd_mode against, case by case: 1 for 8 pairs in one launch, 2 for 9 and 12 pairs, 0 under
    attn4_xcd = 0 and below 8 pairs; 2 for both launches of a planned pair of launches"""
    modes = {c["id"]: X.expected_xcd_mode(c["B"] * c["H"], c["opts"]) for c in X.G4_CASES}
    assert modes["g4-xcd2-b3h3"] == modes["g4-xcd2-b2h6-raw"] == 2 and modes["g4-xcd-off"] == 0
    assert [m for i, m in modes.items() if "-b2h4" in i] == [1, 1]
    assert all(m == 0 for i, m in modes.items() if "-b2h4" not in i and "xcd2" not in i)
    assert X.expected_xcd_mode(9, {}, 2) == X.expected_xcd_mode(8, {}, 2) == 2 and X.expected_xcd_mode(1, {}, 2) == 0


def test_the_self_attention_route_table():
    """both sides of every boundary of attn_choose (csrc/attn.hip), by kernel name without a plan; kernel_name asserts that scail_flash_attn_kernel_for
    agrees, except at the grid limit, which the seven-argument query cannot see: it says 4 on both sides"""
    name = lambda *a, **kw: X.kernel_name(*a, **kw)
    for pre in (False, True):                                                                # `prescaled` does not change any answer
        assert name(128, 128, 128, 1, 1, 256, 511, False, pre) == X.W8 and name(128, 128, 128, 1, 1, 256, 512, False, pre) == X.GEN          # key count
        assert name(128, 128, 128, 1, 1, 256, 512, True, pre) == X.W8                                                                        # accumulate
        assert X.with_options({"attn4": 1}, lambda: name(128, 128, 128, 1, 1, 256, 512, False, pre)) == X.GEN                                # option attn4
        assert X.with_options({"attn4": 0}, lambda: name(128, 128, 128, 1, 1, 256, 512, False, pre)) == X.W8
        # 32-bit byte offsets inside a slice: 69 905 x 15 360 = 1 073 740 800 < 2^30 <= 69 906 x 15 360, for each of the three row strides
        assert 69905 * 15360 == 1073740800 < 2 ** 30 <= 69906 * 15360
        for i in range(3):
            rs = [128, 128, 128]
            rs[i] = 15360
            lens = dict(Lq=256, Lk=512)
            for n, want in ((69905, X.GEN), (69906, X.W8)):
                lens["Lk" if i == 1 else "Lq"] = n
                assert name(*rs, 1, 1, lens["Lq"], lens["Lk"], False, pre) == want, (rs, lens)
        # the V^T image: 128 (Lk + 63) reaches 2^30 at Lk = 8 388 545 (k_rs = 128: the K offsets stay below it up to Lk = 8 388 607, so this term decides)
        assert 128 * (8388544 + 63) < 2 ** 30 <= 128 * (8388545 + 63) and 8388544 * 128 < 2 ** 30
        assert name(128, 128, 128, 1, 1, 256, 8388544, False, pre) == X.GEN and name(128, 128, 128, 1, 1, 256, 8388545, False, pre) == X.W8
        # the workgroup-id decode: 32 768 heads
        assert name(128, 128, 128, 1, 32767, 1, 512, False, pre, agree=False) == X.GEN and name(128, 128, 128, 1, 32768, 1, 512, False, pre, agree=False) == X.W8
        assert name(128, 128, 128, 32767, 1, 1, 512, False, pre, agree=False) == X.GEN and name(128, 128, 128, 32768, 1, 1, 512, False, pre, agree=False) == X.W8
        assert X.flash_route(128, 128, 128, 1, 512, False, pre) == 4                          # ... the blind spot of the seven-argument query, pinned


def test_the_cross_attention_route_table():
    """both sides of every boundary of cross_choose, by kernel name; cross_kernel_name asserts that scail_cross_attn2_kernel_for agrees"""
    name = lambda *a, **o: X.with_options(o, lambda: X.cross_kernel_name(*a))
    D = 256
    assert name(D, D, D, D, 300, 1024, 256, 2, 2) == X.X_HIP and name(D, D, D, D, 300, 1024, 257, 2, 2) == X.X_GEN          # cross4 = 2 (default): 20 / 21 key tiles
    assert name(D, D, D, D, 300, 1024, 256, 2, 2, cross4=2) == X.X_HIP and name(D, D, D, D, 300, 1024, 257, 2, 2, cross4=2) == X.X_GEN
    assert name(D, D, D, D, 300, 1024, 257, 2, 2, cross4=0) == X.X_HIP and name(D, D, D, D, 300, 1024, 256, 2, 2, cross4=1) == X.X_GEN       # option cross4
    for a, b in ((63, 64), (64, 63)):                                                        # at least one whole key tile per set
        assert name(D, D, D, D, 300, a, b, 2, 2, cross4=1) == X.X_HIP
    assert name(D, D, D, D, 300, 64, 64, 2, 2, cross4=1) == X.X_GEN
    assert name(D, D, 2 * D, D, 300, 1024, 257, 2, 2) == X.X_HIP and name(D, 2 * D, 2 * D, D, 300, 1024, 257, 2, 2) == X.X_GEN            # one K row stride for both sets
    for cross4 in (0, 1, 2):                                                                 # option attn4 = 0: no generated kernel at all
        assert name(D, D, D, D, 300, 1024, 257, 2, 2, attn4=0, cross4=cross4) == X.X_HIP
    assert name(D, D, D, D, 300, 1024, 257, 1, 32767) == X.X_GEN and name(D, D, D, D, 300, 1024, 257, 1, 32768) == X.X_HIP                # the workgroup-id decode
    # the hipcc kernel's workgroup count needs no device: one per (128-row query block, head, batch element)
    assert X.cross_kernel_name(D, D, D, D, 300, 512, 257, 2, 2, want_grid=True) == (X.X_HIP, 3 * 2 * 2)


def test_name_queries_reject_bad_buffers_and_write_nothing():
    import ctypes as C
    from scail_amd import lib as L
    L.load()
    small, plan, wg = C.create_string_buffer(b"\x55" * 8, 8), (C.c_int64 * 9)(*([77] * 9)), C.c_int64(77)
    self_args, cross_args = (128, 128, 128, 1, 1, 256, 64, 0, 1), (256, 256, 256, 256, 300, 512, 257, 2, 2)
    for fn, args, extra in (("scail_flash_attn_kernel_name_for", self_args, plan), ("scail_cross_attn2_kernel_name_for", cross_args, C.byref(wg))):
        for e in (None, C.cast(extra, C.c_void_p)):
            with pytest.raises(L.ScailHipError, match="null argument"):
                L.call(fn, *args, None, 128, e)
            with pytest.raises(L.ScailHipError, match="buffer too small"):
                L.call(fn, *args, small, len(small), e)
            with pytest.raises(L.ScailHipError, match="buffer too small"):
                L.call(fn, *args, small, 0, e)
    assert small.raw == b"\x55" * 8 and list(plan) == [77] * 9 and wg.value == 77
    with pytest.raises(L.ScailHipError, match="at least one"):
        L.call("scail_flash_attn_kernel_name_for", 128, 128, 128, 0, 1, 256, 64, 0, 1, small, len(small), None)
    # the 8-wave kernel's plan needs no device: one launch, a workgroup per (256-row query block, head, batch element)
    assert X.kernel_name(128, 128, 128, 2, 3, 300, 64, False, True, plan=True) == (X.W8, dict(n_launch=1, launches=[dict(rows=256, item0=0, n_items=12, xcd_mode=0)]))
    # ... and a forced height's neither
    got = X.with_options({"attn4_rows": 192}, lambda: X.kernel_name(128, 128, 128, 2, 4, 300, 512, False, True, plan=True))
    assert got == (X.GEN + "_q3", dict(n_launch=1, launches=[dict(rows=192, item0=0, n_items=16, xcd_mode=1)]))


# ---- the fp32 restatements pass --------------------------------------------------------------------------------------------------------------
def _restate(case, d, mode, **kw):
    return X.online_fp32(d["q"], d["k"].expand(case["B"], -1, -1), d["v"].expand(case["B"], -1, -1), case["H"], X.sl2_of(case), case["n_seg"], mode=mode,
                         old=d["old"], **kw)


@pytest.mark.parametrize("case", SELF_CASES, ids=lambda c: c["id"])
def test_fp32_restatements_pass(case):
    d = X.self_case(case)
    r = d["r"]
    modes = [("tile", {})] + ([("lazy", {"thr": float(case["opts"].get("attn4_thr", 8))}), ("opt", {"rows": 256}), ("opt", {"rows": 192})] if case["route"] == 4 else [])
    outs = []
    for mode, kw in modes:
        o = _restate(case, d, mode, **kw)
        if mode == "opt":
            o, restarts = o
            wgs = len({t // kw["rows"] for t in X.TARGETS if t < case["Lq"]}) if case["form"] == "restart" else 0
            assert restarts.tolist() == [[wgs] * case["H"]] * case["B"], (mode, kw)
        X.check_interval_bf16(o, r["ref"], r["lo"], r["hi"], f"{case['id']} fp32 {mode} {kw}")
        outs.append(o)
    dec = X.decided(r["lo"], r["hi"])
    assert all(torch.equal(o.double()[dec], outs[0].double()[dec]) for o in outs)


@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("case", X.X_CASES, ids=lambda c: c["id"])
def test_fp32_cross_restatements_pass(case, raw):
    d = X.cross_case(case, raw)
    for mode in ("tile", "lazy"):
        o = X.cross_fp32(d["q"], d["k1"], d["v1"], d["k2"], d["v2"], case["H"], X.sl2_of(raw), mode=mode)
        X.check_interval_bf16(o, d["ref"], d["lo"], d["hi"], f"{case['id']} raw={raw} fp32 {mode}")


def test_small_attention_reference():
    g = torch.Generator().manual_seed(3)
    v = torch.randint(-7, 8, (2, 50, 160), generator=g).float()
    r = X.small_reference(v, 2, 80, [50, 17])
    o = (v[1, :17].sum(0) * (torch.tensor(1.0) / torch.tensor(17.0))).to(X.BF16)
    X.check(o, dict(ref=r["ref"][1], budget=r["budget"][1]), "mean of 17 rows, fp32")
    assert X.undecided_share(r["ref"] - r["budget"], r["ref"] + r["budget"]) <= X.UNDECIDED_CAP


# ---- the checker rejects seeded faults ---------------------------------------------------------------------------------------------------------
def _small(form="plain", raw=False, n_seg=1, Lk=145, spike=None):
    q, k, v = X.exact_qkv("sparse_q", 1, 2, 130, Lk * n_seg, 11, raw, spike)
    r = X.reference(q, k, v, 2, X.sl2_of(raw), n_seg)
    old = None
    if form == "accumulate":
        old = torch.randint(-3, 4, q.shape, generator=torch.Generator().manual_seed(12)).float()
        ref, lo, hi = X.accumulate_bounds(r, old)
    else:
        ref, lo, hi = r["ref"], r["ref"] - r["budget"], r["ref"] + r["budget"]
    return dict(q=q, k=k, v=v, old=old, ref=ref, lo=lo, hi=hi, raw=raw, n_seg=n_seg)


FAULTS = [("drop_tile", {}), ("pad_counted", {}), ("l_2m8", {}), ("l_5pc", {}), ("weight_doubled", {}), ("v_unpermuted", {}), ("skip_segment", dict(n_seg=3, Lk=100)),
          ("no_o_rescale", dict(spike=(140, X.SPIKE_C))), ("truncated", {}), ("old_ignored", dict(form="accumulate")), ("old_after_rounding", dict(form="accumulate")),
          ("scale_twice", dict(raw=True)), ("scale_missing", dict(raw=True))]


@pytest.mark.parametrize("fault,kw", FAULTS, ids=[f for f, _ in FAULTS])
def test_checker_rejects_seeded_faults(fault, kw):
    """on a small case (2 heads x 130 rows x 145 keys: three tiles, the last ragged) the sound chain passes and the faulty one has DECIDED elements
    that are wrong"""
    d = _small(**kw)
    run = lambda f: X.online_fp32(d["q"], d["k"], d["v"], 2, X.sl2_of(d["raw"]), d["n_seg"], mode="tile", old=d["old"], fault=f, fault_tile=2)
    X.check_interval_bf16(run(None), d["ref"], d["lo"], d["hi"], "sound")
    with pytest.raises(AssertionError, match="although fp32 arithmetic decides it"):
        X.check_interval_bf16(run(fault), d["ref"], d["lo"], d["hi"], fault)


def test_checker_rejects_cross_attention_without_its_bf16_intermediate():
    c = X.X_CASES[0]
    d = X.cross_case(c, False)
    with pytest.raises(AssertionError, match="although fp32 arithmetic decides it"):
        X.check_interval_bf16(X.cross_fp32(d["q"], d["k1"], d["v1"], d["k2"], d["v2"], c["H"], fault="set1_unrounded"), d["ref"], d["lo"], d["hi"], "set 1 unrounded")


def test_transpose_v_reference_is_the_emulator_tools():
    from tools import attn4_emu_run as R
    g = torch.Generator().manual_seed(2)
    for Lk, H in ((1, 1), (63, 3), (65, 1), (257, 3)):
        v = torch.randint(-7, 8, (2, Lk, H * 128), generator=g).float()
        mine = X.transpose_v_ref(v, H)
        theirs = R.from_bf16_bits(R.transpose_v(R.to_bf16_bits(v.numpy()), H))
        assert np.array_equal(mine.float().numpy(), theirs)
    p = X.transpose_v_perm(64)
    assert torch.equal(p[p], torch.arange(64)) and p[4] == 8 and p[8] == 4 and p[12] == 12


# ---- the generated kernels in the CPU emulator --------------------------------------------------------------------------------------------------
def _emu_self(cfg, Lq, Lk, raw=False, spike=None, thr=8.0, restart=False, kind="sparse_q", lazy_key=None):
    from tools import attn4_emu_run as R
    q, k, v = X.exact_qkv(kind, 1, 1, Lq, Lk, 1000 + Lk + Lq, raw, spike, lazy_key=lazy_key)
    r = X.reference(q, k, v, 1, X.sl2_of(raw), restart_key=spike[0] if restart else None)
    o, st = R.run(cfg, q.numpy(), [k.numpy()], [v.numpy()], 1, thr_log2=thr, sl2=X.sl2_of(raw))
    o = torch.from_numpy(o).to(X.BF16)
    X.check(o, r, f"emulator {cfg.rows} rows, Lq {Lq}, Lk {Lk}, raw {raw}, spike {spike}, lazy key {lazy_key}, thr {thr}")
    want = X.online_fp32(q, k, v, 1, X.sl2_of(raw), mode="tile")
    dec = X.decided(r["ref"] - r["budget"], r["ref"] + r["budget"])
    assert torch.equal(o.double()[dec], want.double()[dec])
    return st


def _height(rows):
    from scail_amd.asmgen import attn4
    return attn4.M16F if rows == 256 else attn4.M16F_Q3


@pytest.mark.parametrize("rows", X.HEIGHTS)
@pytest.mark.parametrize("Lk", [64, 128, 320, 576, 145])
def test_emulator_m16f_exact_operands(rows, Lk):
    """1, 2, 5 and 9 key tiles and a ragged count (2 tiles + 17 keys), both heights, alternating operand kinds and scales"""
    i = [64, 128, 320, 576, 145].index(Lk)
    _emu_self(_height(rows), rows, Lk, raw=bool(i & 1), kind=("sparse_q", "sparse_k")[(i >> 1) & 1])


@pytest.mark.parametrize("rows", X.HEIGHTS)
def test_emulator_m16f_spike_stays_inside_the_first_pass_headroom(rows):
    """a +12 spike is 28 below the first pass's reference point (first tile's maximum + 40): exact, and the same instructions whatever attn4_thr is --
    the first pass never reaches the rescale subroutine on these operands (the restart test below does)"""
    base = _emu_self(_height(rows), rows, 320)["instr"]
    for thr in (8.0, 0.0, 2.0):
        assert _emu_self(_height(rows), rows, 320, spike=(64 * 4 + 9, X.SPIKE_C), thr=thr)["instr"] == base


@pytest.mark.parametrize("rows", X.HEIGHTS)
def test_emulator_m16f_restart_runs_the_lazy_rescale_on_exact_rows(rows):
    """the c = 64 key restarts the workgroup; in the lazy-maximum loop that follows the reference point is the running maximum, so the lazy rows' +12
    key calls the rescale subroutine at thr 8, the riser rows' +4 key (two tiles earlier) calls it too at thr 2, and thr 0 calls it also where
    ordinary maxima rise.  Proof that it EXECUTED: wave 0 (the statistics are its; it holds lazy row 20 and riser row 25) runs more instructions
    with the two keys than without at thr 8, more again at thr 2 and more again at thr 0; every row -- the rescaled ones included -- is held
    exactly"""
    cfg, spike, lk = _height(rows), (64 * 3 + 7, X.RESTART_C), 64 * 8 + 5
    without = _emu_self(cfg, rows, 64 * 11, spike=spike, restart=True)
    n = {thr: _emu_self(cfg, rows, 64 * 11, spike=spike, restart=True, thr=thr, lazy_key=lk) for thr in (8.0, 2.0, 0.0)}
    assert without["restarts"] == 1 and all(st["restarts"] == 1 for st in n.values())
    assert all(st["mfma"] == without["mfma"] for st in n.values())
    print(f"{rows} rows, wave 0 instructions: without the two keys {without['instr']}, thr 8 {n[8.0]['instr']}, thr 2 {n[2.0]['instr']}, thr 0 {n[0.0]['instr']}")
    assert without["instr"] < n[8.0]["instr"] < n[2.0]["instr"] < n[0.0]["instr"]


def test_emulator_x2_exact_operands():
    from scail_amd.asmgen import attn4
    from tools import attn4_emu_run as R
    c = dict(id="emu-x2", B=1, H=1, Lq=256, Lk1=128, Lk2=65, shared2=True, route=4)
    q, k1, v1 = X.exact_qkv("sparse_q", 1, 1, 256, 128, 77)
    _, k2, v2 = X.exact_qkv("sparse_q", 1, 1, 256, 65, 78)
    ref, lo, hi = X.cross_bounds(X.reference(q, k1, v1, 1), X.reference(q, k2, v2, 1))
    o, _ = R.run_x2(attn4.X2, q.numpy(), k1.numpy(), v1.numpy(), k2.numpy(), v2.numpy(), 1, n_wgs=1, sl2=1.0)
    o = torch.from_numpy(o).to(X.BF16)
    X.check_interval_bf16(o, ref, lo, hi, "emulator scail_attn4_x2, 128 + 65 keys")
    dec = X.decided(lo, hi)
    assert torch.equal(o.double()[dec], X.cross_fp32(q, k1, v1, k2, v2, 1).double()[dec])


def test_emulator_x2_restart_runs_the_lazy_rescale_on_exact_rows():
    """scail_attn4_x2 has the same first pass (reference point = first tile's maximum + 40 per set): the c = 64 key in set 1 restarts that set's pass,
    and the lazy-maximum loop that follows rescales at the lazy rows' +12 key (more instructions than without it); every row is held exactly"""
    from scail_amd.asmgen import attn4
    from tools import attn4_emu_run as R
    _, k2, v2 = X.exact_qkv("sparse_q", 1, 1, 256, 65, 78)
    instr = []
    for lazy_key in (None, 64 * 8 + 5):
        q, k1, v1 = X.exact_qkv("sparse_q", 1, 1, 256, 64 * 11, 79, spike=(64 * 3 + 7, X.RESTART_C), lazy_key=lazy_key)
        ref, lo, hi = X.cross_bounds(X.reference(q, k1, v1, 1, restart_key=64 * 3 + 7), X.reference(q, k2, v2, 1))
        o, st = R.run_x2(attn4.X2, q.numpy(), k1.numpy(), v1.numpy(), k2.numpy(), v2.numpy(), 1, n_wgs=1, sl2=1.0)
        X.check_interval_bf16(torch.from_numpy(o).to(X.BF16), ref, lo, hi, f"emulator scail_attn4_x2, restart in set 1, lazy key {lazy_key}")
        assert st[0]["mfma"] == 136 * (11 + 2) + 136 * 11                                    # set 1 ran twice
        instr.append(st[0]["instr"])
    print(f"scail_attn4_x2, wave 0 instructions: no +12 key {instr[0]}, with it {instr[1]}")
    assert instr[0] < instr[1]
