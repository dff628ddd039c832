"""The operands, references, budgets and restatements of tests/softmax_exact.py, proven on the CPU before a GPU sees them: every case of
tests/test_softmax_exact_gpu.py keeps the conditions on its inputs (integer scores, the exactness bounds, bf16 operands, a bias table that tells a
wrong-head and a transposed lookup apart) and stays under the undecided cap for the reference alone; an IEEE fp32 restatement of each kernel's chain
passes the checker; and the checker rejects seven seeded faults of each kernel: the ragged tail counted as score 0, a wave's partial sum dropped,
the last register chunk skipped, columns >= 8192 left untouched, natural instead of base-2 scaling, a 2^-8 error of the row sum, truncation;
the neighbouring head's bias through a transposed table index, batch 0's mask for batch 1, keys >= 64 dropped, the last key missing from P . V,
the previous row's Q, a 2^-8 error of the row sum, truncation.  Needs no GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import softmax_exact as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


# ---- scail_softmax_rows: the inputs ---------------------------------------------------------------------------------------------------------------
def test_constants_and_case_tables():
    assert X.SLACK == 2.0 and X.UNDECIDED_CAP == 0.05 and X.U == 2.0 ** -24
    assert {X.maxv_of(n) for n in X.SM_EXACT_N if n <= 8192} == {4} and {X.maxv_of(n) for n in X.SM_EXACT_N if n > 8192} == {16}
    assert set(X.SM_EXACT_N) == {1, 7, 8, 9, 2047, 2048, 2056, 8191, 8192, 8193, 8200, 24584, 32767, 32768}
    assert {n for n, _ in X.SM_GENERAL} == {35, 81, 7168, 8200} and {C for _, C in X.SM_GENERAL} == {384, 128}
    assert X.vae_scale(384) == float(np.float32(1.0 / np.sqrt(384.0))) and X.vae_scale(128) == float(np.float32(1.0 / np.sqrt(128.0)))
    ids = [c["id"] for c in X.A_CASES]
    assert len(set(ids)) == len(ids)
    shapes = {(c["B"], c["H"], c["Lq"], c["Lk"], c["hd"]) for c in X.A_CASES}
    assert shapes >= {(2, 3, 130, 130, 64), (1, 2, 512, 512, 64), (2, 2, 257, 257, 80), (1, 2, 33, 297, 128), (2, 3, 5, 65, 64)}
    assert {(c["Lq"], c["Lk"]) for c in X.A_CASES if c["id"].startswith("edge")} == {(a, b) for a in (1, 33) for b in (1, 63, 64, 65)}
    assert all(c["signed_v"] == (c["Lk"] <= 65) for c in X.A_CASES)
    assert any(c["valid"] == [1] and c["Lk"] == 512 for c in X.A_CASES) and any(c["real_scale"] and c["hd"] == 80 for c in X.A_CASES)
    # the LDS boundary of head_dim 128, and UMT5's 512 keys inside it
    assert X.lds_bytes(297, 128) == 544 * 297 + 2048 <= 160 * 1024 < 544 * 298 + 2048 == X.lds_bytes(298, 128)
    assert X.lds_bytes(512, 64) == 148480 <= 160 * 1024
    assert X.LDS_REFUSED["Lk"] == 298 and X.LDS_REFUSED["hd"] == 128


@pytest.mark.parametrize("n", X.SM_EXACT_N)
def test_softmax_exact_case_inputs(n):
    """softmax_exact_reference asserts sl2 = 2^-3, (s - mx) sl2 = k and the exactness bound; here: where the maxima lie, the buffer, the cap"""
    r = X.softmax_exact_reference(n)
    s = r["s"]
    mx = s.amax(-1)
    assert int((s[0] == mx[0]).sum()) == 1 and s[0, n - 1] == mx[0] and int((s[1] == mx[1]).sum()) == 1 and s[1, 0] == mx[1]
    assert torch.equal(torch.log2(r["ref"] / r["ref"].amax(-1, keepdim=True)).round(), ((s - mx[:, None]) / 8).double())             # powers of two over one sum
    buf = X.softmax_buffer(s, n)
    n8 = X.ceil8(n)
    assert buf.shape[1] > n8 and buf.shape[1] % 8 == 0 and bool(torch.isnan(buf[:, n8:].float()).all())
    if n % 8:
        assert float(buf[0, n]) > 2.9e38 and bool(torch.isnan(buf[1, n].float())) and float(buf[2, n]) == float("-inf")
    share = X.undecided_share(r["ref"] - r["budget"], r["ref"] + r["budget"])
    print(f"softmax exact n={n}: undecided share {share:.4%}")
    assert share <= X.UNDECIDED_CAP


@pytest.mark.parametrize("n,C", X.SM_GENERAL)
def test_softmax_general_case_inputs(n, C):
    r = X.softmax_general_reference(n, C)
    share = X.undecided_share(r["ref"] - r["budget"], r["ref"] + r["budget"])
    print(f"softmax general n={n} C={C}: undecided share {share:.4%}, largest relative budget {float(r['rel'].max()):.0f} u, smallest t {r['t_min']:.1f}")
    assert share <= X.UNDECIDED_CAP
    assert float(r["rel"].max()) < 2 ** 15 / 16                                               # far below a bf16 half ulp (32 768 u)
    assert r["t_min"] < -8                                                                   # ... on weights that span many binades


def test_softmax_budgets_are_derived_not_measured():
    r = X.softmax_exact_reference(9)
    assert torch.equal(r["budget"], 2.0 * 6 * 2.0 ** -24 * r["ref"])
    for n, C, maxv in ((35, 128, 4), (8200, 384, 16)):
        r = X.softmax_general_reference(n, C)
        z = (r["s"].double() - r["s"].double().amax(-1, keepdim=True)) * X.vae_scale(C)
        w = torch.softmax(z, -1)
        e = 3 * np.log(2.0) * (z * X.LOG2E).abs() + 2
        want = 2.0 * 2.0 ** -24 * w * (e + (w * e).sum(-1, keepdim=True) + 8 * maxv + 8 + 2)
        assert torch.allclose(r["budget"], want, rtol=1e-12, atol=0) and torch.allclose(r["ref"], w, rtol=1e-12, atol=0)


# ---- scail_softmax_rows: the restatement passes, the faults do not ----------------------------------------------------------------------------------
def _sm(regime, n, C=128):
    if regime == "exact":
        return X.softmax_exact_reference(n), X.raw_scale()
    return X.softmax_general_reference(n, C), X.vae_scale(C)


@pytest.mark.parametrize("n", X.SM_EXACT_N)
def test_softmax_fp32_restatement_passes_exact(n):
    r, scale = _sm("exact", n)
    buf = X.softmax_buffer(r["s"], n)
    X.check_softmax_output(X.softmax_fp32(buf, n, scale), buf, r, n, f"softmax fp32 exact n={n}")


@pytest.mark.parametrize("n,C", X.SM_GENERAL)
def test_softmax_fp32_restatement_passes_general(n, C):
    r, scale = _sm("general", n, C)
    buf = X.softmax_buffer(r["s"], n)
    X.check_softmax_output(X.softmax_fp32(buf, n, scale), buf, r, n, f"softmax fp32 general n={n} C={C}")


SM_FAULTS = [("tail_zero", "exact", 9), ("wave_dropped", "exact", 2056), ("last_chunk", "general", 7168), ("maxv_mixup", "exact", 8200), ("natural", "general", 81),
             ("sum_2m8", "general", 35), ("truncated", "general", 81)]


@pytest.mark.parametrize("fault,regime,n", SM_FAULTS, ids=[f for f, _, _ in SM_FAULTS])
def test_softmax_checker_rejects_seeded_faults(fault, regime, n):
    r, scale = _sm(regime, n)
    buf = X.softmax_buffer(r["s"], n)
    X.check_softmax_output(X.softmax_fp32(buf, n, scale), buf, r, n, "sound")
    with pytest.raises(AssertionError, match="although fp32 arithmetic decides it"):
        X.check_softmax_output(X.softmax_fp32(buf, n, scale, fault=fault), buf, r, n, fault)


# ---- scail_attn_small: the inputs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [2, 3])
def test_bias_table_tells_the_lookups_apart(H):
    tab = X.bias_table(H)
    assert tab.dtype == torch.float32 and tab.shape == (X.N_BUCKETS, H) and torch.equal(tab, tab.round()) and float(tab.abs().max()) <= 2
    for b in range(X.N_BUCKETS):
        assert len(set(tab[b].tolist())) == H                                                # another head's column
        for h in range(H):
            t = X.transposed_index(b, h, H)
            assert t == (b, h) or tab[t] != tab[b, h]                                        # the transposed index
    from scail_amd.umt5 import relative_position_bucket
    bk = relative_position_bucket(5, 65)
    assert bk.shape == (5, 65) and bk.dtype == torch.int32 and int(bk.min()) >= 0 and int(bk.max()) < X.N_BUCKETS and len(bk.unique()) > 16


@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("case", X.A_CASES, ids=lambda c: c["id"])
def test_attn_small_case_inputs(case, kind):
    """integer scores or the bound on sum|q k| (asserted by small_reference()), bf16 operands (small_qkv()), the V operand's sign, the masks, the cap"""
    d = X.small_case(case, kind)
    q, k, v, r = d["q"], d["k"], d["v"], d["r"]
    qm = 8.0 if case["scale"] == 0.125 else 1.0
    assert set(q.unique().tolist()) <= {-qm, 0.0, qm} and set(k.unique().tolist()) <= {-1.0, 0.0, 1.0}
    sp = (q if kind == "sparse_q" else k).view(-1, case["hd"])
    assert bool(((sp != 0).sum(-1) == 4).all()) and bool(((sp.view(-1, 4, case["hd"] // 4) != 0).sum(-1) == 1).all())
    assert torch.equal(v, v.round()) and float(v.abs().max()) <= 7 and (float(v.min()) >= 1 or case["signed_v"]) and (not case["signed_v"] or float(v.min()) < 0)
    assert case["scale"] in (1.0, 0.125) or case["real_scale"]
    assert float(np.float32(case["scale"])) == case["scale"]
    if case["valid"] is not None:
        assert d["mask"].sum(-1).tolist() == case["valid"] and min(case["valid"]) >= 1
    if case["bias"]:
        assert d["bucket"].shape == (case["Lq"], case["Lk"]) and d["tab"].shape == (X.N_BUCKETS, case["H"])
    share = X.undecided_share(r["ref"] - r["budget"], r["ref"] + r["budget"])
    print(f"{case['id']} {kind}: undecided share {share:.4%}, smallest x {r['x_min']:.2f}")
    assert share <= X.UNDECIDED_CAP
    assert bool((r["budget"] >= 0).all())
    if case["valid"] is not None and 1 in case["valid"]:                                     # one unmasked key: its v row and no budget
        b = case["valid"].index(1)
        assert torch.equal(r["ref"][b], v[b, :1].double().expand(case["Lq"], -1)) and float(r["budget"][b].max()) == 0


def test_attn_small_budget_is_derived_not_measured():
    q, k, v = X.small_qkv("sparse_q", 1, 1, 3, 70, 64, 21)
    r = X.small_reference(q, k, v, 1, 1.0)
    s = q[0].double() @ k[0].double().t()
    x = s - s.amax(-1, keepdim=True)
    w = torch.softmax(x, -1)
    e = 2 * x.abs() + 2
    va = v[0].double().abs()
    want = 2.0 * 2.0 ** -24 * ((w * e) @ va + 70 * (w @ va) + (w @ v[0].double()).abs() * ((w * e).sum(-1, keepdim=True) + 2 + 6 + 2))
    assert torch.allclose(r["budget"][0], want, rtol=1e-12, atol=0)
    # the real scale widens every weight's error by 2 E + u |x|, E = (head_dim + 1) 4 scale
    q, k, v = X.small_qkv("sparse_k", 1, 1, 3, 70, 80, 22)
    a = X.small_reference(q, k, v, 1, X.REAL_SCALE_80, real_scale=True)
    s = q[0].double() @ k[0].double().t() * X.REAL_SCALE_80
    x = s - s.amax(-1, keepdim=True)
    w = torch.softmax(x, -1)
    e = 2 * x.abs() + 2 + 2 * 81 * 4 * X.REAL_SCALE_80 + x.abs()
    va = v[0].double().abs()
    want = 2.0 * 2.0 ** -24 * ((w * e) @ va + 70 * (w @ va) + (w @ v[0].double()).abs() * ((w * e).sum(-1, keepdim=True) + 2 + 6 + 2))
    assert torch.allclose(a["budget"][0], want, rtol=1e-12, atol=0)


# ---- scail_attn_small: the restatement passes, the faults do not ----------------------------------------------------------------------------------
def _restate(case, d, fault=None):
    return X.attn_small_fp32(d["q"], d["k"], d["v"], case["H"], case["scale"], d["bucket"], d["tab"], d["mask"], fault=fault)


@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("case", X.A_CASES, ids=lambda c: c["id"])
def test_attn_small_fp32_restatement_passes(case, kind):
    d = X.small_case(case, kind)
    r = d["r"]
    o = _restate(case, d)
    X.check_interval_bf16(o, r["ref"], r["ref"] - r["budget"], r["ref"] + r["budget"], f"{case['id']} {kind} fp32")
    if case["valid"] is not None and 1 in case["valid"]:
        X.assert_bits(o, d["v"][:, :1].expand(-1, case["Lq"], -1).to(X.BF16), "one unmasked key")


A_FAULTS = ["bias_transposed", "mask_batch0", "keys_ge64_dropped", "pv_last_key", "prev_row_q", "sum_2m8", "truncated"]


@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("fault", A_FAULTS)
def test_attn_small_checker_rejects_seeded_faults(fault, kind):
    """on the UMT5-like case (2 x 3 heads x 130 rows x 130 keys, bias, batch 1 with 70 unmasked keys) the sound chain passes and the faulty one has
    DECIDED elements that are wrong"""
    case = X.A_CASES[0]
    assert case["id"] == "umt5-130"
    d = X.small_case(case, kind)
    r = d["r"]
    X.check_interval_bf16(_restate(case, d), r["ref"], r["ref"] - r["budget"], r["ref"] + r["budget"], "sound")
    with pytest.raises(AssertionError, match="although fp32 arithmetic decides it"):
        X.check_interval_bf16(_restate(case, d, fault), r["ref"], r["ref"] - r["budget"], r["ref"] + r["budget"], fault)
