"""The references and the checker of tests/conv_exact.py, proven on the CPU before a GPU sees them: the exact sum is order-independent in fp32 and
equal to the oracle's convolution; the margin of check_rounded_bf16 passes an IEEE fp32 restatement of the norm + SiLU chain; the inputs of every
norm case of tests/test_conv_exact_gpu.py keep the undecided share under its cap and t above T_NEG_MIN; the checks reject a truncating pack, one
dropped (tap, channel) pair at a border voxel, a bias added after the rounding, sqrt(C - 1) for sqrt(C) and a norm of the unrounded sum; and the
case table names every convolution kernel of csrc/conv.hip (a host-only query).  Needs no GPU."""
import pytest
import torch
import torch.nn.functional as F

import conv_exact as E
from oracle import wan_vae_oracle as V


def _case(id):
    return next(c for c in E.PLAIN_CASES + E.NORM_CASES + E.RESID_NORM_CASES if c["id"] == id)


def _taps_fp32(case, o, reverse):
    """the sum accumulated tap by tap and 32-channel slice by slice in fp32 (forward, or the slices of every tap in reverse order)"""
    x, w = o["x"], o["w"] if o["w"].dim() == 5 else o["w"].unsqueeze(2)
    kt, kh, kw = w.shape[2:]
    pad = case["pad"] if case["pad"] is not None else (kt - 1, kh // 2, kw // 2)
    st = case["stride"]
    if case["ups"]:
        x = F.interpolate(x.permute(1, 0, 2, 3), scale_factor=(2.0, 2.0), mode="nearest-exact").permute(1, 0, 2, 3)
    s2 = st[1] == 2
    xp = F.pad(x, (pad[2], 1 if s2 else pad[2], pad[1], 1 if s2 else pad[1], pad[0], 0))
    To, Ho, Wo = E.out_thw(case)
    acc = torch.zeros(To, Ho, Wo, w.shape[0], dtype=torch.float32)
    slices = [slice(c, min(c + 32, x.shape[0])) for c in range(0, x.shape[0], 32)]
    taps = [(dt, dh, dw) for dt in range(kt) for dh in range(kh) for dw in range(kw)]
    for dt, dh, dw in taps:
        for sl in (slices[::-1] if reverse else slices):
            win = xp[sl, dt:dt + st[0] * (To - 1) + 1:st[0], dh:dh + st[1] * (Ho - 1) + 1:st[1], dw:dw + st[2] * (Wo - 1) + 1:st[2]]
            acc = acc + torch.einsum("cthw,oc->thwo", win, w[:, sl, dt, dh, dw])
    return acc


@pytest.mark.parametrize("id", ["conv4c-96", "s2-1-32-96", "conv4u-192-96-ups"])
def test_fp32_accumulation_is_exact_in_any_order(id):
    case = _case(id)
    o = E.operands(case)
    want = E.conv_sum(o["x"], o["w"], None, None, case["stride"], case["pad"], case["ups"])
    assert tuple(want.shape[:3]) == E.out_thw(case)
    for reverse in (False, True):
        acc = _taps_fp32(case, o, reverse)
        assert torch.equal(acc.double(), want), f"fp32 accumulation ({'reversed slices' if reverse else 'forward'}) is not the exact sum"
    full = acc + o["bias"] + o["resid"]                      # bias and residual in fp32: still exact
    assert torch.equal(full.double(), E.conv_sum(o["x"], o["w"], o["bias"], o["resid"], case["stride"], case["pad"], case["ups"]))
    assert float(want.abs().max()) * 8 + 64 + 512 < 2 ** 24


@pytest.mark.parametrize("id", ["conv4c-96", "igemm-16-32", "direct-shortcut"])
def test_conv_ref_equals_the_oracle_in_fp64(id):
    case = _case(id)
    o = E.operands(case)
    want = V.causal_conv3d(o["x"].double()[None], o["w"].double(), o["bias"].double())[0].permute(1, 2, 3, 0)
    assert torch.equal(E.conv_sum(o["x"], o["w"], o["bias"]), want)
    assert torch.equal(E.conv_ref(o["x"], o["w"], o["bias"]).double(), want.float().to(torch.bfloat16).double())


def _rows(C, silu):
    x, gamma = E.integer_rows(E.RMS_SILU_ROWS, C, seed=C + (1 if silu else 0))
    s = x.to(torch.bfloat16)
    return s, gamma, E.norm_silu_ref(s, gamma, silu)


def test_margin_is_derived_not_measured():
    assert E.MARGIN == 4 * (38.5 + 34.5 * 4.0) * 2.0 ** -24 and 2.0 ** -15 < E.MARGIN < 2.0 ** -14
    assert 38.5 + 34.5 * -E.T_NEG_MIN <= E.MARGIN / E.U          # the worst case of the most negative t the inputs may hold
    assert E.UNDECIDED_CAP == 0.03


@pytest.mark.parametrize("id", [c["id"] for c in E.NORM_CASES + E.RESID_NORM_CASES])
def test_norm_case_inputs_and_margin(id):
    """on the inputs the GPU file uses: the undecided share is under its cap, no t is below T_NEG_MIN, and IEEE fp32 arithmetic passes the checker"""
    case = _case(id)
    s, ref = E.norm_reference(case)
    gamma = E.operands(case)["gamma"]
    assert float(E.norm_t(s, gamma).min()) >= E.T_NEG_MIN
    share = E.check_rounded_bf16(E.norm_silu_fp32(s, gamma).to(torch.bfloat16), ref, E.MARGIN, id + " (IEEE fp32)")
    assert share <= E.UNDECIDED_CAP, share


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("C", E.RMS_SILU_CHANNELS)
def test_rms_silu_rows_inputs_and_margin(C, silu):
    s, gamma, ref = _rows(C, silu)
    assert float(s[0].abs().max()) == 0 and int((s[1] != 0).sum()) == 1 and float(ref[0].abs().max()) == 0
    assert float(E.norm_t(s, gamma).min()) >= E.T_NEG_MIN
    share = E.check_rounded_bf16(E.norm_silu_fp32(s, gamma, silu).to(torch.bfloat16), ref, E.MARGIN, f"rows C={C} silu={silu} (IEEE fp32)")
    assert share <= E.UNDECIDED_CAP, share


# ---- the checks reject wrong results ------------------------------------------------------------------------------------------------------
def _truncate(v64):
    lo, _, _ = E.bf16_neighbours(v64)
    return lo.to(torch.bfloat16)


def test_rejects_truncation_instead_of_rne():
    case = _case("norm-conv4c_e4")
    o = E.operands(case)
    s64 = E.conv_sum(o["x"], o["w"], o["bias"])
    with pytest.raises(AssertionError, match="differ"):
        E.assert_bits(_truncate(s64), E.round_bf16(s64), "truncated pack")
    s, ref = E.norm_reference(case)
    with pytest.raises(AssertionError, match="not the correctly rounded"):
        E.check_rounded_bf16(_truncate(ref), ref, E.MARGIN, "truncated pack")


def test_rejects_one_dropped_tap_channel_pair_at_a_border_voxel():
    case = _case("conv4c-96")
    o = E.operands(case)
    s64 = E.conv_sum(o["x"], o["w"], o["bias"])
    T, H, W = case["thw"]
    t, h, wv, n = T - 1, H - 1, W - 1, 1                              # the last voxel of the ragged last tile; tap (2, 1, 1) reads the voxel itself
    c = int((o["x"][:, t, h, wv] * o["w"][n, :, 2, 1, 1]).abs().argmax())
    term = float(o["x"][c, t, h, wv] * o["w"][n, c, 2, 1, 1])
    assert term != 0
    bad = s64.clone()
    bad[t, h, wv, n] -= term
    assert abs(float(s64[t, h, wv, n])) < 64, "one product (>= 1/8) survives the rounding only where the bf16 step is <= 1/4"
    with pytest.raises(AssertionError, match="1 of .* elements differ"):
        E.assert_bits(E.round_bf16(bad), E.round_bf16(s64), "dropped pair")


def test_rejects_a_bias_added_after_the_rounding():
    case = _case("conv4c-96")
    o = E.operands(case)
    twice = (E.conv_ref(o["x"], o["w"]).float() + o["bias"]).to(torch.bfloat16)
    with pytest.raises(AssertionError, match="differ"):
        E.assert_bits(twice, E.conv_ref(o["x"], o["w"], o["bias"]), "bias after the rounding")


def test_rejects_sqrt_of_c_minus_one():
    case = _case("norm-conv4c_e4")
    s, ref = E.norm_reference(case)
    C = s.shape[-1]
    t = E.norm_t(s, E.operands(case)["gamma"]) * ((C - 1) / C) ** 0.5
    with pytest.raises(AssertionError, match="not the correctly rounded|no bf16 neighbour"):
        E.check_rounded_bf16(E.round_bf16(t / (1 + torch.exp(-t))), ref, E.MARGIN, "sqrt(C - 1)")


def test_rejects_the_norm_of_the_unrounded_sum():
    case = _case("norm-conv4c_e4")
    o = E.operands(case)
    s, ref = E.norm_reference(case)
    s64 = E.conv_sum(o["x"], o["w"], o["bias"])
    assert not torch.equal(s.double(), s64)
    with pytest.raises(AssertionError, match="not the correctly rounded|no bf16 neighbour"):
        E.check_rounded_bf16(E.round_bf16(E.norm_silu_ref(s64, o["gamma"])), ref, E.MARGIN, "norm of the unrounded sum")


def test_checker_accepts_the_correctly_rounded_value_and_counts_the_undecided():
    ref = torch.tensor([1.0, 1.00390625, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.015625 + 2.0 ** -12, 0.0], dtype=torch.float64)
    rne = torch.tensor([1.0, 1.0, 1.0078125, -3.015625, 0.0]).to(torch.bfloat16)
    assert E.check_rounded_bf16(rne, ref, 2.0 ** -15, "rne") == pytest.approx(2 / 5)      # the tie and 1 + 2^-8 + 2^-20 lie inside the margin
    other = torch.tensor([1.0, 1.0078125, 1.0, -3.015625, 0.0]).to(torch.bfloat16)          # the other neighbour of the two undecided ones: allowed
    E.check_rounded_bf16(other, ref, 2.0 ** -15, "other neighbour")
    with pytest.raises(AssertionError, match="not the correctly rounded"):
        E.check_rounded_bf16(other, ref, 2.0 ** -22, "margin below the distance")
    with pytest.raises(AssertionError, match="no bf16 neighbour"):
        E.check_rounded_bf16(torch.tensor([1.0, 1.0, 1.015625, -3.015625, 0.0]).to(torch.bfloat16), ref, 2.0 ** -15, "two steps away")


# ---- the case table against the dispatch (host-only queries of the built library) ----------------------------------------------------------
def test_case_table_names_every_convolution_kernel():
    from scail_amd import build
    build.build(verbose=False)
    named = []
    for c in E.PLAIN_CASES:
        N = (c["cout"] + 7) // 8 * 8
        got = E.with_options(c["opts"], lambda: (E.kernel_name(c, 0, N + 32, 0, 2, 1), E.kernel_name(c, 0, N + 32, N + 8, 2, 1)))
        assert got[0] == c["plain"] and (c["resid"] is None or got[1] == c["resid"]), (c["id"], got)
        named += [c["plain"], c["resid"] or ""]
    for c in E.NORM_CASES:
        assert E.with_options(c["opts"], lambda: E.kernel_name(c, 1, c["cout"], 0)) == c["plain"], c["id"]
        named.append(c["plain"])
    for c in E.RESID_NORM_CASES:
        N = c["cout"]
        got = E.with_options(c["opts"], lambda: E.kernel_name(c, 2 if c["want_raw"] else 3, N, N if c["with_resid"] else 0))
        assert got == c["plain"], (c["id"], got)
        named.append(c["plain"])
    for k in E.KERNELS:
        assert any(n.startswith(k) for n in named), f"no case runs {k}"
    for form in ("<0, 32, 1, false, 96, 2>", "<0, 32, 1, false, 96>", "<0, 32, 1, false, 32>", "<0, 32, 1, false, 96, 2, 1, true>", "<4, 32, 1, false, 96, 2>",
                 "<4, 32, 1, false, 96>", "<4, 32, 1, false, 32>"):
        assert "conv_halo_kernel" + form in named
    for form in ("<14, 3>", "<6, 3>", "<6, 6>", "<6, 6> x 2", "<14, 3, true>"):
        assert "conv_direct_kernel" + form in named
    for bn in ("64, 4, 1", "96, 4, 1", "128, 2, 2"):
        assert f"conv_igemm_kernel<0, {bn}>" in named and f"conv_igemm_kernel<3, {bn}>" in named
