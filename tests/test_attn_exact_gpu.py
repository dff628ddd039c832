"""Every attention kernel and its V staging on operands for which softmax attention is exact in fp32 (tests/attn_exact.py): scail_transpose_v bit
for bit against a Python permutation; flash_attn_swp_kernel (and, in the measurement build, every schedule variant of the 8-wave family),
scail_attn4_m16f at both tile heights and in its planned two-launch form, cross_attn2_kernel, scail_attn4_x2 and scail_attn_small against the fp64
reference: correctly rounded wherever fp32 arithmetic can decide it, inside the derived budget elsewhere.  Outputs go into NaN-filled buffers; slack
of the layouts must stay NaN; every case asserts its kernel through the host queries.  tests/test_attn_exact_cpu.py proves the inputs and the
checker."""
import pytest
import torch

import attn_exact as X

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from scail_amd import lib, ops as _ops
    lib.load()          # loud failure when the HIP library is missing
    assert torch.cuda.is_available()
    return _ops


# the schedules of the 8-wave family (tests/test_kernels_gpu.py ATTN_VARIANTS): the first is the product's kernel
ATTN_VARIANTS = [8 | (2 << 12), 2, 258, 66, 8 | (1 << 12), 8 | (6 << 12)]


@pytest.fixture(params=ATTN_VARIANTS)
def attn_variant(request):
    from scail_amd import lib as L
    if request.param == ATTN_VARIANTS[0]:
        yield request.param
        return
    if not L.ABLATIONS:
        pytest.skip("kernel variant of the measurement build (run with SCAIL_ABLATIONS=1)")
    L.tune_set("attn_variant", request.param)
    yield request.param
    L.tune_set("attn_variant", ATTN_VARIANTS[0])


def nan_buf(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=BF16)


def column_view(x, col, cols=3):
    """x (B, L, D) as columns [col D, (col + 1) D) of a NaN-filled (B, L, cols D) buffer"""
    B, L, D = x.shape
    buf = nan_buf(B, L, cols * D)
    buf[..., col * D:(col + 1) * D] = x.to(BF16).to(DEV)
    return buf[..., col * D:(col + 1) * D]


def transpose_v_into_nan(ops, v, H):
    """the V^T image of v, written by scail_transpose_v into a NaN-filled target: whatever it left unwritten poisons the attention that reads it"""
    return ops.transpose_v(v, H, out=nan_buf(v.shape[0], H, X.HD, (v.shape[1] + 63) // 64 * 64))


def all_nan(t):
    return bool(torch.isnan(t.float()).all())


def assert_choice(case, opts, args, variant=None):
    """the kernels and launches the library says the call runs (the name query with a plan) against the case: the kernel by name, and for the generated
    kernel the plan -- the forced height, every (pair, query block) item once, the workgroup-id decode -- and scail_flash_attn_rows_for's agreement
    with it.  Returns the plan."""
    from scail_amd import lib as L
    B, H, Lq = case["B"], case["H"], case["Lq"]
    name, plan = X.kernel_name(*args, plan=True)
    first = plan["launches"][0]
    if opts.get("attn4", 1) == 0 or case["route"] == 8:
        assert name == X.expected_name(dict(case, route=8), variant=variant), name
        qblk = 128 if variant == 66 else 256
        assert plan == dict(n_launch=1, launches=[dict(rows=qblk, item0=0, n_items=B * H * -(-Lq // qblk), xcd_mode=0)]), plan
        return plan
    rows = L.load().scail_flash_attn_rows_for(B, H, Lq)
    assert rows == (448 if plan["n_launch"] == 2 else first["rows"]) and name == X.expected_name(case, rows), (name, rows, plan)
    forced = opts.get("attn4_rows", 0)
    if forced:
        assert plan["n_launch"] == 1 and first["rows"] == forced
    if plan["n_launch"] == 1:
        assert first["item0"] == 0 and first["n_items"] == B * H * -(-Lq // first["rows"]), plan
    assert all(l["xcd_mode"] == X.expected_xcd_mode(B * H, opts, plan["n_launch"]) for l in plan["launches"]), plan
    return plan


def run_self(ops, case, d, opts=None, variant=None):
    """one scail_flash_attn_bf16 call of a case under its options (+ opts): the output (B, Lq, D) bf16 on the CPU; asserts the route, the kernel name
    (variant: the attn_variant code in force), the launch plan and the slack"""
    B, H, Lq, Ls, S = case["B"], case["H"], case["Lq"], case["Lk"], case["n_seg"]
    D = H * X.HD
    strided, acc = case["form"] == "strided", case["form"] == "accumulate"
    q = column_view(d["q"], 0) if strided else d["q"].to(BF16).to(DEV)
    Bk = d["k"].shape[0]
    if strided:                                                                              # k and v are columns 1 and 2 of one buffer
        kv = nan_buf(Bk, Ls, 3 * D)
        kv[..., D:2 * D], kv[..., 2 * D:] = d["k"].to(BF16).to(DEV), d["v"].to(BF16).to(DEV)
        kseg, vseg = kv[None, :, :, D:2 * D], kv[None, :, :, 2 * D:]
    else:
        kseg = d["k"].view(Bk, S, Ls, D).permute(1, 0, 2, 3).contiguous().to(BF16).to(DEV)   # (S, Bk, Ls, D)
        vseg = d["v"].view(Bk, S, Ls, D).permute(1, 0, 2, 3).contiguous().to(BF16).to(DEV)
    vt = torch.stack([transpose_v_into_nan(ops, vseg[s], H) for s in range(S)])
    obuf = nan_buf(B, Lq, D + 64) if strided else nan_buf(B, Lq, D)
    out = obuf[..., :D]
    if acc:
        out.copy_(d["old"].to(BF16).to(DEV))
    all_opts = dict(case["opts"], **(opts or {}))

    def call():
        assert X.flash_route(q.stride(1), kseg.stride(2), out.stride(1), Lq, Ls, acc, not case["raw"]) == (8 if all_opts.get("attn4", 1) == 0 else case["route"]), case["id"]
        assert_choice(case, all_opts, (q.stride(1), kseg.stride(2), out.stride(1), B, H, Lq, Ls, acc, not case["raw"]), variant)
        kw = dict(scale=X.raw_scale()) if case["raw"] else dict(q_prescaled=True)
        ops.flash_attn(q, kseg[0], vt[0], out=out, accumulate=acc, n_seg=S, k_seg_stride=kseg.stride(0) if S > 1 else 0, vt_seg_stride=vt.stride(0) if S > 1 else 0,
                       k_broadcast=case["form"] == "bcast", **kw)
        torch.cuda.synchronize()

    X.with_options(all_opts, call)
    if strided:
        assert all_nan(obuf[..., D:]), "the slack between output rows was written"
    return out.cpu()


def check_self(o, d, what):
    r = d["r"]
    return X.check_interval_bf16(o, r["ref"], r["lo"], r["hi"], what)


# ---- scail_transpose_v -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("Lk", [1, 63, 64, 65, 257])
def test_transpose_v_is_the_permutation(ops, Lk, heads):
    """bit-exact against the Python permutation (keys permuted inside each group of 16: bits 2 and 3 swapped), from a strided v view, into a NaN-filled
    target: the padding up to the next multiple of 64 must be written, with zeros"""
    B, D = 2, heads * X.HD
    g = torch.Generator().manual_seed(Lk * 10 + heads)
    v = torch.randint(-7, 8, (B, Lk, D), generator=g).float()
    assert X._is_bf16(v)
    out = nan_buf(B, heads, X.HD, (Lk + 63) // 64 * 64)
    ops.transpose_v(column_view(v, 2), heads, out=out)
    X.assert_bits(out, X.transpose_v_ref(v, heads), f"transpose_v Lk={Lk} heads={heads}")


# ---- the 8-wave kernel --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.W8_CASES, ids=lambda c: c["id"])
def test_8wave_kernel_exact(ops, attn_variant, case):
    d = X.self_case(case)
    o = run_self(ops, case, d, variant=attn_variant)
    check_self(o, d, f"{case['id']} variant {attn_variant}")
    if case["Lk"] == 1 and case["n_seg"] == 1:                                               # one key: o = v, bit for bit
        X.assert_bits(o, d["v"].expand(case["B"], 1, -1).expand(-1, case["Lq"], -1).to(BF16), "one key")


# ---- scail_attn4_m16f ---------------------------------------------------------------------------------------------------------------------
def _restart_counter(L, fn):
    ctr = torch.zeros(1, device=DEV, dtype=torch.int32)
    L.call("scail_flash_attn_count_restarts", ctr.data_ptr())
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        L.call("scail_flash_attn_count_restarts", None)
    return out, int(ctr.item())


@pytest.mark.parametrize("case", X.G4_CASES, ids=lambda c: c["id"])
def test_attn4_m16f_exact_at_both_heights_and_equal_to_the_8wave_kernel(ops, case):
    from scail_amd import lib as L
    d = X.self_case(case)
    dec = X.decided(d["r"]["lo"], d["r"]["hi"])
    outs = {}
    for rows in X.HEIGHTS:
        assert X.with_options({"attn4_rows": rows}, lambda: L.load().scail_flash_attn_rows_for(case["B"], case["H"], case["Lq"])) == rows
        o, restarts = _restart_counter(L, lambda: run_self(ops, case, d, {"attn4_rows": rows}))
        want = len({t // rows for t in X.TARGETS if t < case["Lq"]}) * case["B"] * case["H"] if case["form"] == "restart" else 0
        print(f"{case['id']} {rows} rows: {restarts} workgroups restarted")
        assert restarts == want, (rows, restarts, want)
        check_self(o, d, f"{case['id']} {rows} rows")
        outs[rows] = o
    o8 = run_self(ops, case, d, {"attn4": 0})
    check_self(o8, d, f"{case['id']} 8-wave kernel")
    for rows in X.HEIGHTS:
        assert torch.equal(outs[rows].double()[dec], o8.double()[dec]), f"{rows}-row launch against the 8-wave kernel"
    assert torch.equal(outs[256].double()[dec], outs[192].double()[dec])


@pytest.mark.parametrize("B,H,Lq0", [(1, 1, 64), (3, 3, 256)], ids=["one-pair", "nine-pairs"])
def test_attn4_m16f_planned_two_launch_shape(ops, B, H, Lq0):
    """scail_flash_attn_bf16's mixed launch (whole rounds of 256-row tiles, then 192-row tiles from a 768-row boundary on): option "attn4_cus" makes
    the plan count on a few CUs only, the smallest Lq (from Lq0 on) for which scail_flash_attn_rows_for answers 448 is searched with the host query,
    and that shape runs on exact operands -- every row exactly once, equal to the single 256-row launch on every decided element.  One pair: the
    split lies INSIDE the pair, at a 768-row boundary.  Nine pairs: both launches decode their workgroup ids in 8 runs of the item list (XCD mode
    2: padded grid, and the 192-row launch starts at its item0)"""
    from scail_amd import lib as L
    lib = L.load()

    def search():
        for Lq in range(Lq0, 4097, 64):
            for cus in range(1, 17):
                L.set_option("attn4_cus", cus)
                if lib.scail_flash_attn_rows_for(B, H, Lq) == 448:
                    return cus, Lq
        return None

    try:
        found = search()
    finally:
        L.set_option("attn4_cus", 0)
    assert found is not None, "no planned two-launch shape up to 4096 rows"
    cus, Lq = found
    assert Lq > 768 or B * H >= 8
    print(f"two-launch shape: attn4_cus {cus}, batch {B}, {H} heads, {Lq} query rows")
    case = X._c(f"g4-two-launch-{B}x{H}x{Lq}", B, H, Lq, 512, route=4)
    q, k, v = X.exact_qkv("sparse_q", B, H, Lq, 512, 4242)
    r = X.reference(q, k, v, H)
    d = dict(q=q, k=k, v=v, old=None, r=dict(r, lo=r["ref"] - r["budget"], hi=r["ref"] + r["budget"]))

    def planned():
        assert lib.scail_flash_attn_rows_for(B, H, Lq) == 448
        name, plan = X.kernel_name(H * X.HD, H * X.HD, H * X.HD, B, H, Lq, 512, False, True, plan=True)
        print(f"{name}: {plan}")
        assert name == "scail_attn4_m16f + scail_attn4_m16f_q3" and plan["n_launch"] == 2
        first, second = plan["launches"]
        n4, n3 = -(-Lq // 256), -(-Lq // 192)
        assert (first["rows"], first["item0"], second["rows"]) == (256, 0, 192) and 0 < first["n_items"] < B * H * n4
        # launch 0 ends, and launch 1 starts, at the same query row of the same pair, a multiple of 768 rows: every row exactly once
        pair, row = first["n_items"] // n4, first["n_items"] % n4 * 256
        assert (second["item0"] // n3, second["item0"] % n3 * 192) == (pair, row) and row % 768 == 0
        assert second["item0"] + second["n_items"] == B * H * n3
        assert [l["xcd_mode"] for l in plan["launches"]] == ([2, 2] if B * H >= 8 else [0, 0])
        return run_self(ops, case, d)

    o = X.with_options({"attn4_cus": cus}, planned)
    check_self(o, d, case["id"])
    o256 = run_self(ops, case, d, {"attn4_rows": 256})
    dec = X.decided(d["r"]["lo"], d["r"]["hi"])
    assert torch.equal(o.double()[dec], o256.double()[dec])


# ---- cross attention ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raw", [False, True], ids=["prescaled", "raw"])
@pytest.mark.parametrize("case", X.X_CASES, ids=lambda c: c["id"])
def test_cross_attention_exact_on_both_kernels(ops, case, raw):
    B, H, Lq = case["B"], case["H"], case["Lq"]
    D = H * X.HD
    d = X.cross_case(case, raw)
    q = column_view(d["q"], 0)
    k1, k2 = d["k1"].to(BF16).to(DEV), d["k2"].to(BF16).to(DEV)
    vt1, vt2 = transpose_v_into_nan(ops, d["v1"].to(BF16).to(DEV), H), transpose_v_into_nan(ops, d["v2"].to(BF16).to(DEV), H)
    kw = dict(scale=X.raw_scale()) if raw else dict(q_prescaled=True)
    outs = []
    for cross4 in (0, 1):
        obuf = nan_buf(B, Lq, D + 64)

        def call():
            assert X.cross_route(q.stride(1), D, D, D + 64, Lq, case["Lk1"], case["Lk2"], B, H) == (case["route"] if cross4 else 2)
            name, wgs = X.cross_kernel_name(q.stride(1), D, D, D + 64, Lq, case["Lk1"], case["Lk2"], B, H, want_grid=True)
            assert name == (X.expected_name(case) if cross4 else X.X_HIP)
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            assert wgs == (min(cus, B * H * -(-Lq // 256)) if name == X.X_GEN else B * H * -(-Lq // 128)), (name, wgs)
            ops.cross_attn2(q, k1, vt1, k2, vt2, out=obuf[..., :D], **kw)
            torch.cuda.synchronize()

        X.with_options({"cross4": cross4}, call)
        assert all_nan(obuf[..., D:]), "the slack between output rows was written"
        o = obuf[..., :D].cpu()
        X.check_interval_bf16(o, d["ref"], d["lo"], d["hi"], f"{case['id']} raw={raw} cross4={cross4}")
        outs.append(o)
    dec = X.decided(d["lo"], d["hi"])
    assert torch.equal(outs[0].double()[dec], outs[1].double()[dec])


# ---- scail_attn_small ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [64, 80])
def test_attn_small_masked_mean(ops, hd):
    """all scores zero (q = 0), no bias, a key mask with ragged valid counts: o is the correctly rounded mean of the unmasked v rows within the
    division's budget (the biased softmax uses natural exp, is not exact and stays with tests/test_encoders_gpu.py)"""
    B, heads, Lq, Lk, valid = 2, 2, 37, 50, [50, 17]
    g = torch.Generator().manual_seed(hd)
    v = torch.randint(-7, 8, (B, Lk, heads * hd), generator=g).float()
    k = torch.randint(-1, 2, (B, Lk, heads * hd), generator=g).float()
    mask = torch.zeros(B, Lk, dtype=torch.int32)
    for b in range(B):
        mask[b, :valid[b]] = 1
    r = X.small_reference(v, heads, hd, valid)
    out = nan_buf(B, Lq, heads * hd)
    ops.attn_small(torch.zeros(B, Lq, heads * hd, device=DEV, dtype=BF16), k.to(BF16).to(DEV), v.to(BF16).to(DEV), heads, key_mask=mask.to(DEV), out=out)
    ref, bud = r["ref"][:, None].expand(B, Lq, -1).contiguous(), r["budget"][:, None].expand(B, Lq, -1).contiguous()
    share = X.check(out.cpu(), dict(ref=ref, budget=bud), f"attn_small head_dim {hd}")
    assert share <= X.UNDECIDED_CAP
