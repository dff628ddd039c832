"""The row kernels of csrc/rowops.hip against fp64 references rounded once (tests/row_exact.py): LayerNorm + modulate and affine LayerNorm on the block
kernel (one chunk, a partial wave, one full register pass plus a chunk, a third pass with one chunk, the maximum D) and on all five wave
instantiations, the persistent row loops and the batch split, the executor's calling forms; RMSNorm with and without RoPE on the block kernel, both
wave forms (head_dim 128 and not), in place, strided, batched tables, an offset table view, the slab layout, the plain copy; bit-exact properties that
need no margin; scail_small_linear, scail_mul_bf16 and scail_row_affine.  Every element has to be the round-to-nearest-even bf16 of something inside
the derived per-element margin around the reference.  Every case first asserts its kernel by name and its workgroup count
(scail_row_kernel_name_for), writes into a NaN-filled tensor wider than the result and asserts that nothing else was written.
tests/test_row_exact_cpu.py proves that these checks reject the faults listed there."""
import pytest
import torch

import row_exact as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def cus():
    from scail_amd import lib as L
    L.load()
    return torch.cuda.get_device_properties(0).multi_processor_count


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan_out(rows, ld):
    """rows + 1 rows of ld columns, NaN everywhere: one guard row, and guard columns where ld > D"""
    return torch.full((rows + 1, ld), NAN, dtype=BF16, device=DEV)


def _untouched(out, rows, D, what):
    o = out.float()
    assert bool(torch.isnan(o[rows:]).all()) and bool(torch.isnan(o[:rows, D:]).all()), f"{what}: written outside the result"


def _route(c, form, n_batch, rows_out, cus, hd=128):
    """asserts the kernel by name and the workgroup count; -> (name, workgroups)"""
    name, wg = E.kernel_name(form, n_batch, rows_out, c["D"], hd, want_grid=True)
    assert name == E.expected_name(c), (c["id"], name)
    rows = n_batch * rows_out
    if "wave" not in name:
        want = rows
    elif form in ("mod", "aff"):
        want = n_batch * max(1, min((rows_out + 3) // 4, (3 * cus + n_batch - 1) // n_batch))
    else:
        want = max(1, min((rows + 3) // 4, 3 * cus))
    assert wg == want, (c["id"], name, wg, want)
    print(f"{c['id']}: {name}, {wg} workgroups for {rows} rows")
    return name, wg


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------
def _run_ln(c, inp, cus, rows_launch=None):
    """one launch: the whole case, or (n_batch = 1, no row offset) its first rows_launch rows alone.  -> (rows, D) bf16 on the CPU"""
    from scail_amd import lib as L
    D, B = c["D"], inp["n_batch"]
    ro = inp["rows_out"] if rows_launch is None else rows_launch
    src_rows = inp["src_rows"] if rows_launch is None else rows_launch
    assert rows_launch is None or (B == 1 and c["src_off"] == 0)
    x = inp["x_src"].to(DEV)
    ldx, ldy = x.shape[-1], D + 8
    out = _nan_out(B * ro, ldy)
    name, wg = _route(c, c["form"], B, ro, cus)
    if c["loops"]:
        assert ro > 4 * (wg // B), "the case is meant to take the persistent row loop more than once"
    if c["form"] == "mod":
        if c["mod"] == "plain":
            sh, sc, stride = inp["shift"].to(DEV), inp["scale"].to(DEV), D
            psh, psc = sh.data_ptr(), sc.data_ptr()
        else:
            tab = inp["table"].to(DEV)
            psh, psc, stride = tab.data_ptr(), tab.data_ptr() + 4 * D, c["mod"] * D
        L.call("scail_ln_modulate", x.data_ptr(), ldx, out.data_ptr(), ldy, psh, psc, stride, B, ro, src_rows, c["src_off"], D, c["eps"], _stream())
    else:
        w, b = inp["w"].to(DEV), inp["b"].to(DEV)
        L.call("scail_layernorm_affine", x.data_ptr(), ldx, out.data_ptr(), ldy, w.data_ptr(), b.data_ptr(), B * ro, D, c["eps"], _stream())
    torch.cuda.synchronize()
    _untouched(out, B * ro, D, c["id"])
    return out[:B * ro, :D].cpu()


@pytest.mark.parametrize("id", [c["id"] for c in E.LN_CASES])
def test_layernorm(id, cus):
    c = E.case_of(id)
    inp = E.ln_inputs(c, cus)

    def run():
        return _run_ln(c, inp, cus), [(k, _run_ln(c, inp, cus, k)) for k in c["launches"]]

    got, small = E.with_options(E.options_of(c), run)
    E.check_case(got, inp["ref"], inp["margin"], inp["n_special"], id)
    k = got.shape[0] - E.N_SPECIAL                                   # the all-zero row: bf16(shift) | bf16(b), bit for bit
    E.assert_bits(got[k], E.rne_bf16(inp["add"][k]).float().to(BF16), id + " zero row")
    for n, g in small:
        E.check_margin_bf16(g, inp["ref"][:n], inp["margin"][:n], f"{id} [{n} rows]")


# ---- RMSNorm + RoPE -----------------------------------------------------------------------------------------------------------
def _run_rms(c, inp, cus, rows_launch=None, tables=True, entry="scaled", out_scale=None, cos=None, sin=None):
    """one launch in the case's calling form -> (rows, D) bf16 on the CPU.  tables False: the call without RoPE tables; entry "plain": scail_rmsnorm_rope"""
    from scail_amd import lib as L
    D, hd, call = c["D"], c["hd"], c["call"]
    rows = inp["rows"] if rows_launch is None else rows_launch
    rpb = inp["rpb"] if rows_launch is None else rows
    os_ = c["out_scale"] if out_scale is None else out_scale
    rope = c["rope"] and tables
    w = inp["w"].to(DEV)
    pc = ps = None
    if rope:
        cf = (inp["cos_full"] if cos is None else cos).to(DEV)
        sf = (inp["sin_full"] if sin is None else sin).to(DEV)
        pc, ps = cf.data_ptr() + 4 * inp["row0"] * (hd // 2), sf.data_ptr() + 4 * inp["row0"] * (hd // 2)
    if rope:
        _route(c, "rope", 1, rows, cus, hd)
    else:
        name, wg = E.kernel_name("rms", 1, rows, D, hd, want_grid=True)
        assert (name, wg) == ("rmsnorm_rope_kernel", rows)
        print(f"{c['id']}: {name}, {wg} workgroups for {rows} rows (no tables)")
    x = inp["x"][:rows]
    if call == "inplace3":
        g = torch.Generator().manual_seed(7)
        buf = E.regular_rows(rows, 3 * D, g)
        buf[:, D:2 * D] = x
        dbuf = buf.to(DEV)
        p = dbuf.data_ptr() + 2 * D
        L.call("scail_rmsnorm_rope_scaled", p, 3 * D, p, 3 * D, w.data_ptr(), pc, ps, rows, rpb, D, hd, E.f32(E.EPS), os_, _stream())
        torch.cuda.synchronize()
        res = dbuf.cpu()
        E.assert_bits(res[:, :D], buf[:, :D], c["id"] + " left third")
        E.assert_bits(res[:, 2 * D:], buf[:, 2 * D:], c["id"] + " right third")
        return res[:, D:2 * D].contiguous()
    xd = x.to(DEV)
    if call == "slab":
        n_slabs = 4
        sw = D // n_slabs
        msg = torch.full((n_slabs, rows, 3 * sw), NAN, dtype=BF16, device=DEV)      # q | k | v side by side: this call fills the middle third
        L.call("scail_rmsnorm_rope_slabs", xd.data_ptr(), D, msg.data_ptr() + 2 * sw, sw, 3 * sw, rows * 3 * sw, w.data_ptr(), pc, ps, rows, rpb, D, hd,
               E.f32(E.EPS), os_, _stream())
        torch.cuda.synchronize()
        m = msg.float()
        assert bool(torch.isnan(m[:, :, :sw]).all()) and bool(torch.isnan(m[:, :, 2 * sw:]).all()), c["id"] + ": written outside the slab third"
        return msg[:, :, sw:2 * sw].permute(1, 0, 2).reshape(rows, D).cpu()
    ldy = 2 * D if call == "ldy2" else D + 8
    out = _nan_out(rows, ldy)
    if entry == "plain":
        L.call("scail_rmsnorm_rope", xd.data_ptr(), D, out.data_ptr(), ldy, w.data_ptr(), pc, ps, rows, rpb, D, hd, E.f32(E.EPS), _stream())
    else:
        L.call("scail_rmsnorm_rope_scaled", xd.data_ptr(), D, out.data_ptr(), ldy, w.data_ptr(), pc, ps, rows, rpb, D, hd, E.f32(E.EPS), os_, _stream())
    torch.cuda.synchronize()
    _untouched(out, rows, D, c["id"])
    return out[:rows, :D].cpu()


@pytest.mark.parametrize("id", [c["id"] for c in E.RMS_CASES])
def test_rmsnorm_rope(id, cus):
    c = E.case_of(id)
    inp = E.rms_inputs(c, cus)

    def run():
        if c["loops"]:
            _, wg = E.kernel_name("rope", 1, inp["rows"], c["D"], c["hd"], want_grid=True)
            assert inp["rows"] > 4 * wg, "the case is meant to take the persistent row loop more than once"
        return _run_rms(c, inp, cus), [(k, _run_rms(c, inp, cus, k)) for k in c["launches"]]

    got, small = E.with_options(E.options_of(c), run)
    E.check_case(got, inp["ref"], inp["margin"], inp["n_special"], id)
    assert float(got[inp["rows"] - E.N_SPECIAL].float().abs().max()) == 0.0, "the all-zero row"
    for n, g in small:                                               # (rows_per_batch = n: the same table rows)
        E.check_margin_bf16(g, inp["ref"][:n], inp["margin"][:n], f"{id} [{n} rows]")


@pytest.mark.parametrize("id", ["rms-wave-1536-hd128", "rms-wave-1536-hd64", "rms-block-256-hd64", "rms-block-128-hd128", "rms-block-5120-rope"])
def test_rope_bit_exact_properties(id, cus):
    """no margin: identity tables (cos = 1, sin = 0) give the bits of the call without tables; quarter-turn tables give the identity result with the
    pairs swapped and signed; out_scale = 1.0 gives the bits of the unscaled entry point.  A call without tables always runs the block kernel, so the
    first property is bit for bit only where the call with tables runs it too; on a wave kernel, whose fp32 sums have another order, the
    identity-table result is held to the reference of the call without tables instead, under the wave kernel's margin."""
    c = E.case_of(id)
    inp = E.rms_inputs(c, cus)
    g = torch.Generator().manual_seed(11)
    shape = inp["cos_full"].shape
    one, zero = torch.ones(shape), torch.zeros(shape)
    q = torch.randint(0, 4, shape, generator=g)
    qc, qs = torch.tensor([1.0, 0.0, -1.0, 0.0])[q], torch.tensor([0.0, 1.0, 0.0, -1.0])[q]

    def run():
        return (_run_rms(c, inp, cus, tables=False), _run_rms(c, inp, cus, cos=one, sin=zero), _run_rms(c, inp, cus, cos=qc, sin=qs),
                _run_rms(c, inp, cus, out_scale=1.0), _run_rms(c, inp, cus, entry="plain"))

    plain, ident, quarter, scale1, unscaled = E.with_options(E.options_of(c), run)
    if E.expected_name(c) == "rmsnorm_rope_kernel":
        E.assert_bits(ident, plain, id + ": cos = 1, sin = 0")
    else:
        ref, margin = E.rms_reference(inp["x"], inp["w"], E.f32(E.EPS), E.depth("wave", c["D"]), out_scale=c["out_scale"])
        E.check_case(ident, ref, margin, inp["n_special"], id + ": cos = 1, sin = 0 against the reference without tables")
    tok = torch.arange(inp["rows"]) % inp["rpb"] + inp["row0"]
    p = E.rope_pairs(c["D"], c["hd"])
    cc, ss = qc[tok][:, p].to(BF16), qs[tok][:, p].to(BF16)          # 0, +-1: exact
    n0, n1 = ident[:, 0::2], ident[:, 1::2]
    want = torch.stack((n0 * cc - n1 * ss, n1 * cc + n0 * ss), -1).reshape(ident.shape)      # one term is +-0, the other +-n: exact in bf16
    E.assert_bits(quarter, want, id + ": quarter turns")
    E.assert_bits(scale1, unscaled, id + ": out_scale = 1.0")


def test_slab_copy_without_weight(cus):
    """w == NULL: a plain copy into the slab layout, and nothing else written"""
    from scail_amd import lib as L
    c = E.case_of("rms-block-slab-norope")
    inp = E.rms_inputs(c, cus)
    rows, D = inp["rows"], c["D"]
    sw = D // 4
    assert E.kernel_name("copy", 1, rows, D, 128, want_grid=True) == ("rmsnorm_rope_kernel", rows)
    x = inp["x"].to(DEV)
    msg = torch.full((4, rows, 3 * sw), NAN, dtype=BF16, device=DEV)
    L.call("scail_rmsnorm_rope_slabs", x.data_ptr(), D, msg.data_ptr() + 4 * sw, sw, 3 * sw, rows * 3 * sw, None, None, None, rows, rows, D, 128, E.f32(E.EPS),
           1.0, _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(msg[:, :, :2 * sw].float()).all())
    E.assert_bits(msg[:, :, 2 * sw:].permute(1, 0, 2).reshape(rows, D).cpu(), inp["x"], "slab copy")


def test_rmsnorm_rope_on_the_models_tables(cus):
    """the oracle's own rope_tables (3 x 6 x 4 latent grid, 12 heads), passed as the executor passes them: cos[:, 0::2]"""
    from scail_amd import lib as L
    from oracle import scail_oracle as O
    cos, sin = O.rope_tables(O.DiTConfig(hidden_size=1536, num_attention_heads=12, latent_height=32, latent_width=32, num_frames=13), 3, 6, 4)
    cos, sin = cos[:, 0::2].contiguous(), sin[:, 0::2].contiguous()
    ref, margin, x, w = E.table_case(cos, sin, 1536)
    rows, D = x.shape
    name, wg = E.kernel_name("rope", 1, rows, D, 128, want_grid=True)
    assert name == "rmsnorm_rope_wave_kernel<3, true>" and wg == min((rows + 3) // 4, 3 * cus)
    out = _nan_out(rows, D + 8)
    xd, wd, cd, sd = x.to(DEV), w.to(DEV), cos.to(DEV), sin.to(DEV)
    L.call("scail_rmsnorm_rope", xd.data_ptr(), D, out.data_ptr(), D + 8, wd.data_ptr(), cd.data_ptr(), sd.data_ptr(), rows, rows, D, 128, E.f32(E.EPS), _stream())
    torch.cuda.synchronize()
    _untouched(out, rows, D, "oracle tables")
    E.check_case(out[:rows, :D].cpu(), ref, margin, 0, "rms-wave-oracle-tables")


# ---- the small kernels next to them ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 264, 520, 1032])
@pytest.mark.parametrize("N", [5, 64])
@pytest.mark.parametrize("M", [1, 8])
def test_small_linear_exact(M, N, K):
    """integer x, integer bf16 weights, integer bias, no activation: every fp32 partial sum is exact, so the fp32 output IS the fp64 sum"""
    from scail_amd import lib as L
    x, w, b, y64 = E.small_linear_operands(M, N, K)
    assert float((x.double().abs() @ w.double().abs().t()).max()) + 8 < 2 ** 24, "exactness bound: every partial sum is an integer below 2^24"
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    y = torch.full((M * N + 8,), NAN, device=DEV)
    L.call("scail_small_linear", xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), M, N, K, L.ACT_NONE, L.ACT_NONE, _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[M * N:]).all())
    assert torch.equal(y[:M * N].cpu().double().reshape(M, N), y64)
    y0 = torch.full((M * N + 8,), NAN, device=DEV)
    L.call("scail_small_linear", xd.data_ptr(), wd.data_ptr(), None, y0.data_ptr(), M, N, K, L.ACT_NONE, L.ACT_NONE, _stream())
    assert torch.equal(y0[:M * N].cpu().double().reshape(M, N), y64 - b.double()[None])


@pytest.mark.parametrize("act_in,act_out", [(1, 0), (2, 0), (0, 1), (0, 2), (1, 1)])
@pytest.mark.parametrize("K", [8, 520])
def test_small_linear_activations(K, act_in, act_out):
    """SiLU / tanh-GELU on the input and on the output, under the margin of row_exact.small_linear_margin"""
    from scail_amd import lib as L
    M, N = 8, 5
    x, w, b, ref, margin = E.small_linear_act_case(M, N, K, act_in, act_out)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    y = torch.full((M * N + 8,), NAN, device=DEV)
    L.call("scail_small_linear", xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), M, N, K, act_in, act_out, _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[M * N:]).all())
    err = (y[:M * N].cpu().double().reshape(M, N) - ref).abs()
    print(f"small_linear K={K} act_in={act_in} act_out={act_out}: max err / margin {float((err / margin.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= margin).all()), (float(err.max()), float((err / margin.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("n", [8, 8 * (3 * 256 + 5)])
def test_mul_bf16_is_the_product_rounded_once(n):
    """the product of two bf16 values is exact in fp32; n = 8: one thread; the other: a ragged fourth workgroup"""
    from scail_amd import lib as L
    g = torch.Generator().manual_seed(n)
    a, b = E.regular_rows(1, n, g)[0], E.regular_rows(1, n, g)[0]
    ad, bd = a.to(DEV), b.to(DEV)
    y = torch.full((n + 8,), NAN, dtype=BF16, device=DEV)
    L.call("scail_mul_bf16", ad.data_ptr(), bd.data_ptr(), y.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    want = torch.full((n + 8,), NAN, dtype=BF16)
    want[:n] = E.rne_bf16(a.double() * b.double()).float().to(BF16)
    E.assert_bits(y.cpu(), want, f"mul_bf16 n={n}")


@pytest.mark.parametrize("form", ["rowscale", "addrow", "both", "both-broadcast"])
def test_row_affine(form):
    """y[r] = x[r] * rowscale[r] + addrow[r % add_rows]: two fp32 roundings (one under contraction), margin u |x s| + u |ref|.  Without a row scale the
    product is exact and so is the fp32 sum of two bf16 values of similar size -- many of them exact ties between two bf16 values: there the margin is 0
    and the output is the sum rounded once, ties to even, bit for bit."""
    from scail_amd import lib as L
    rows, D = 37, 264                                                # 1221 chunks: four full workgroups and a ragged fifth
    g = torch.Generator().manual_seed(5 + len(form))
    x = E.regular_rows(rows, D, g)
    s = torch.randn(rows, generator=g) if form != "addrow" else None
    add_rows = {"rowscale": 0, "addrow": rows, "both": rows, "both-broadcast": 5}[form]
    a = E.regular_rows(add_rows, D, g) if add_rows else None
    prod = x.double() * (s.double()[:, None] if s is not None else 1.0)
    ref = prod + (a.double()[torch.arange(rows) % add_rows] if a is not None else 0.0)
    margin = E.SLACK * E.U * (prod.abs() + ref.abs())
    if s is None:
        margin = torch.where((x.float() + a.float()).double() == ref, 0.0, E.U * ref.abs())
        assert float((margin == 0).double().mean()) > 0.99
    xd, sd, ad = x.to(DEV), None if s is None else s.to(DEV), None if a is None else a.to(DEV)
    y = torch.full((rows * D + 8,), NAN, dtype=BF16, device=DEV)
    L.call("scail_row_affine", xd.data_ptr(), y.data_ptr(), None if sd is None else sd.data_ptr(), None if ad is None else ad.data_ptr(), add_rows, rows, D,
           _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[rows * D:].float()).all()), "written behind the output"
    share, _ = E.check_margin_bf16(y[:rows * D].cpu().reshape(rows, D), ref, margin, f"row_affine {form}")
    assert share <= E.UNDECIDED_CAP
