"""The token, sampler and layout kernels against the exact references of tests/layout_exact.py, bit for bit: scail_patchify, scail_patchify_chars,
scail_unpatchify, scail_f32_to_bf16, scail_bf16_to_f32, scail_adaln_table, scail_from_channels_last (+ _frames), scail_transpose2d and
scail_slabs_to_rows have ONE reference; scail_cfg_euler and scail_to_channels_last (+ _frames), whose multiply-adds the compiler may contract, must
give one of the four (two) candidates on every element, and the counts are printed; scail_timestep_embedding must give the correctly rounded fp32 of
the fp64 reference on every element (the inputs leave none undecided).  Every result is written into a larger sentinel-filled buffer, every strided
input is a window of one, and every word outside the result must keep its bits.  tests/test_layout_exact_cpu.py proves the inputs and the checkers."""
import pytest
import torch

import layout_exact as X

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def L():
    from scail_amd import lib
    lib.load()          # loud failure when the HIP library is missing
    assert torch.cuda.is_available()
    return lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def d16(bits):
    """int64 bit patterns -> bf16 tensor on the device (a copy of the bits: no conversion touches a NaN payload)"""
    return X.bf16_of(bits).to(DEV)


def d32(words):
    return X.f32_of(words).to(DEV)


def h16(t):
    torch.cuda.synchronize()
    return X.bits_of(t.cpu())


def h32(t):
    torch.cuda.synchronize()
    return X.words_of(t.cpu())


# ---- 1. token assembly --------------------------------------------------------------------------------------------------------------------------------
def _run_patchify(L, c, name):
    inp = X.patchify_inputs(c)
    before, want, inside = X.framed(X.patchify_reference(c, inp).view(-1, c["kpad"]))
    x, ref, pose, tok = d32(inp["xw"]), d16(inp["ref"]), d16(inp["pose"]), d16(before)
    shape = (c["B"], c["n_ref"], c["n_pose"]) + ((c["n_char"],) if name == "scail_patchify_chars" else ()) + (c["T"], c["H"], c["W"], c["kpad"])
    L.call(name, x.data_ptr(), ref.data_ptr(), pose.data_ptr(), tok.data_ptr(), *shape, stream())
    got = h16(tok)
    X.check_buffer(got, before, inside, [want], f"{name} {c['id']}")
    assert torch.equal(h32(x), inp["xw"]) and torch.equal(h16(ref), inp["ref"]) and torch.equal(h16(pose), inp["pose"])
    return got


@pytest.mark.parametrize("c", X.PATCHIFY_CASES, ids=lambda c: c["id"])
def test_patchify_is_the_token_layout(L, c):
    _run_patchify(L, c, "scail_patchify")


@pytest.mark.parametrize("c", X.CHARS_CASES, ids=lambda c: c["id"])
def test_patchify_chars_is_the_token_layout(L, c):
    """n_char = 1 through lib.call (ops.patchify routes it to the other kernel): the reference, and bit for bit scail_patchify's buffer"""
    got = _run_patchify(L, c, "scail_patchify_chars")
    if c["n_char"] == 1:
        assert torch.equal(got, _run_patchify(L, c, "scail_patchify"))


@pytest.mark.parametrize("B,T,H,W", X.UNPATCHIFY_CASES)
def test_unpatchify_is_the_permutation(L, B, T, H, W):
    tok = X.unpatchify_tokens(B, T, H, W)
    before, want, inside = X.framed(X.unpatchify_reference(tok, B, T, H, W).reshape(-1, W), sentinel=X.SENT32)
    out, td = d32(before), d16(tok)
    L.call("scail_unpatchify", td.data_ptr(), out.data_ptr(), B, T, H, W, stream())
    X.check_buffer(h32(out), before, inside, [want], f"unpatchify B={B} T={T} {H}x{W}")


# ---- 2. conversions -----------------------------------------------------------------------------------------------------------------------------------
def test_bf16_to_f32_on_every_pattern(L):
    p = X.all_bf16_patterns()
    before, want, inside = X.framed((p << 16)[None], rows_after=0, cols_after=64, sentinel=X.SENT32)
    out, pd = d32(before), d16(p)
    L.call("scail_bf16_to_f32", pd.data_ptr(), out.data_ptr(), p.numel(), stream())
    X.check_buffer(h32(out), before, inside, [want], "bf16_to_f32, all 65 536 patterns")


def test_f32_to_bf16_rounds_to_nearest_even_on_every_tie_and_denormal(L):
    """every bf16 pattern p, the words (p << 16) + d for d in {0, 1, 0x7fff, 0x8000, 0x8001, 0xffff}: every tie and both sides of it at every exponent,
    denormal inputs and outputs, overflow to infinity, every NaN class.  A device that flushed denormals here would fail this test."""
    w = X.all_conversion_words()
    before, _, inside = X.framed(X.rne_bits(w)[None], rows_after=0, cols_after=64)
    out, wd = d16(before), d32(w)
    L.call("scail_f32_to_bf16", wd.data_ptr(), out.data_ptr(), w.numel(), stream())
    got = h16(out)
    assert torch.equal(got[~inside], before[~inside]), "words behind the result were written"
    den_in, den_out = X.check_f32_to_bf16(got[0, :w.numel()], w, "f32_to_bf16")
    print(f"f32_to_bf16: {w.numel()} words bit for bit; denormals are NOT flushed: {den_in} fp32 denormal inputs, {den_out} of them with a bf16 denormal result, "
          f"all rounded to nearest even")


@pytest.mark.parametrize("n", X.WRAPPER_N)
def test_to_bf16_and_to_f32_wrappers(L, n):
    from scail_amd import ops
    w = X.rounding_words(n, 11 + n)
    X.check_f32_to_bf16(h16(ops.to_bf16(d32(w))), w, f"ops.to_bf16 n={n}")
    p = X.patterns([n], 5 + n)[0]
    assert torch.equal(h32(ops.to_f32(d16(p))), p << 16)


# ---- 3. sampler scalars -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", X.TS_CASES)
def test_timestep_embedding_is_the_rounded_fp64_reference(L, dim, n):
    t = X.timestep_values(n)
    ref, m, _ = X.timestep_reference(t, dim)
    before, _, inside = X.framed(X.words_of(ref.float()), sentinel=X.SENT32)
    out, td = d32(before), t.to(DEV)
    L.call("scail_timestep_embedding", td.data_ptr(), out.data_ptr(), n, dim, stream())
    got = h32(out)
    assert torch.equal(got[~inside], before[~inside]), "the guard row was written"
    assert X.check_timestep(got[:n], ref, m, f"timestep_embedding dim={dim} n={n}") == 0


@pytest.mark.parametrize("layers,B,width", X.ADALN_CASES)
def test_adaln_table_is_one_fp32_addition(L, layers, B, width):
    emb, table = X.adaln_inputs(layers, B, width)
    before, want, inside = X.framed(X.words_of(emb[None] + table[:, None]).view(layers * B, width), sentinel=X.SENT32)
    out, ed, tb = d32(before), emb.to(DEV), table.to(DEV)
    L.call("scail_adaln_table", ed.data_ptr(), tb.data_ptr(), out.data_ptr(), layers, B, width, stream())
    X.check_buffer(h32(out), before, inside, [want], f"adaln_table {layers}x{B}x{width}")


@pytest.mark.parametrize("n", X.CFG_EULER_N)
def test_cfg_euler_is_one_of_the_contraction_candidates(L, n):
    """x + ds * (vu + cfg * (vc - vu)): each multiply-add fused or not; v's second half starts exactly at v + n"""
    x, v = X.cfg_euler_inputs(n)
    frames = [X.framed(c[None], rows_after=0, cols_after=64, sentinel=X.SENT32) for c in X.cfg_euler_candidates(x, v)]
    before, _, inside = frames[0]
    xb = d32(before)
    xb[0, :n] = x.to(DEV)
    before = h32(xb)
    vb = torch.cat([X.words_of(v), torch.full((64,), X.SENT32)])
    vd = d32(vb)
    L.call("scail_cfg_euler", xb.data_ptr(), vd.data_ptr(), n, float(X.CFG), float(X.DSIGMA), stream())
    counts = X.check_buffer(h32(xb), before, inside, [f[1] for f in frames], f"cfg_euler n={n}")
    assert torch.equal(h32(vd), vb)
    print(f"cfg_euler n={n}: elements equal to each candidate: " + ", ".join(f"{k} {c}" for k, c in zip(X.CFG_EULER_NAMES, counts)))


# ---- 4. VAE layouts -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Cc,batch", X.TRANSPOSE_CASES)
def test_transpose2d_is_the_transpose(L, R, Cc, batch):
    """the input a window of a wider, taller sentinel-filled tensor (ldi = C + 3, batch stride (R + 2) ldi), the output rows ldo = R + 5 long with
    one guard row per matrix: columns from R on and the guard rows keep their bits"""
    x = X.transpose_input(R, Cc, batch)
    src = torch.full((batch, R + 2, Cc + 3), X.SENT16, dtype=torch.int64)
    src[:, :R, :Cc] = x
    before, want, inside = X.framed(x.transpose(1, 2), rows_after=1, cols_after=5)
    sd, out = d16(src), d16(before)
    L.call("scail_transpose2d", sd.data_ptr(), Cc + 3, (R + 2) * (Cc + 3), out.data_ptr(), R + 5, (Cc + 1) * (R + 5), R, Cc, batch, stream())
    X.check_buffer(h16(out), before, inside, [want], f"transpose2d {R}x{Cc} batch {batch}")
    assert torch.equal(h16(sd), src)


def _ptr(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("has_a,has_b", X.CL_AB)
@pytest.mark.parametrize("C,Cpad", X.CL_SHAPES)
def test_to_channels_last_is_one_of_the_contraction_candidates(L, C, Cpad, has_a, has_b):
    """bf16(x * a + b) with a general a, fused or not; a == NULL and b == NULL; the pad channels are +0"""
    a, b = X.cl_scale_shift(C, has_a, has_b)
    ad, bd = (None if v is None else v.to(DEV) for v in (a, b))
    total = [0, 0]
    for N in X.CL_N:
        x = X.cl_planar_input(C, N, a, b)
        frames = [X.framed(c) for c in X.to_channels_last_candidates(x, a, b, Cpad)]
        before, _, inside = frames[0]
        y, xd = d16(before), x.to(DEV)
        L.call("scail_to_channels_last", xd.data_ptr(), y.data_ptr(), _ptr(ad), _ptr(bd), C, Cpad, N, stream())
        got = h16(y)
        counts = X.check_buffer(got, before, inside, [f[1] for f in frames], f"to_channels_last C={C} Cpad={Cpad} N={N} a={has_a} b={has_b}")
        assert bool((got[:N, C:] == 0).all())
        total = [t + c for t, c in zip(total, counts)]
    n_el = sum(X.CL_N) * Cpad
    print(f"to_channels_last C={C} Cpad={Cpad} a={has_a} b={has_b}: of {n_el} elements, equal to the separate result {total[0]}, to the fused result {total[1]}")


@pytest.mark.parametrize("lo,hi", X.CL_CLAMPS)
@pytest.mark.parametrize("has_a,has_b", X.CL_AB)
def test_from_channels_last_is_the_fp32_expression(L, has_a, has_b, lo, hi):
    """clamp((x + b) * a, lo, hi) cannot contract: bit for bit; rows of ldx = Cpad + 8 with sentinel columns from C on; a NaN input comes out as lo"""
    for C, Cpad in X.CL_SHAPES:
        a, b = X.cl_scale_shift(C, has_a, has_b)
        ad, bd = (None if v is None else v.to(DEV) for v in (a, b))
        for N in X.CL_N:
            buf = X.cl_rows_input(C, N, Cpad + 8)
            before, want, inside = X.framed(X.from_channels_last_reference(buf, C, a, b, lo, hi), sentinel=X.SENT32)
            y, xd = d32(before), d16(buf)
            L.call("scail_from_channels_last", xd.data_ptr(), Cpad + 8, y.data_ptr(), _ptr(ad), _ptr(bd), C, N, lo, hi, stream())
            X.check_buffer(h32(y), before, inside, [want], f"from_channels_last C={C} ldx={Cpad + 8} N={N} a={has_a} b={has_b} clamp ({lo}, {hi})")


@pytest.mark.parametrize("hw", X.FRAMES_HW)
def test_frame_window_kernels_with_a_general_scale(L, hw):
    """hw = 48: the float4 form of the windowed kernels; hw = 45: the dword form.  The windowed and the whole-tensor kernel each satisfy the
    two-candidate rule on the way in (they need not agree with each other) and give the one fp32 expression on the way back"""
    fc = X.FRAMES_CASE
    C, Cpad, T, t0, n = fc["C"], fc["Cpad"], fc["T"], fc["t0"], fc["n"]
    a, b = X.cl_scale_shift(C, True, True)
    ad, bd = a.to(DEV), b.to(DEV)
    x = X.cl_planar_input(C, T * hw, a, b, seed=1)
    x[:, t0 * hw:t0 * hw + X.CL_TIES] = x[:, :X.CL_TIES]                # the tie inputs inside the window as well
    xd = x.to(DEV)
    win = slice(t0 * hw, (t0 + n) * hw)
    for what, xs, call in (("to_channels_last_frames", x[:, win].contiguous(), lambda y: L.call("scail_to_channels_last_frames", xd.data_ptr(), y.data_ptr(), ad.data_ptr(), bd.data_ptr(),
                                                                                             C, Cpad, T * hw, t0 * hw, n * hw, stream())),
                           ("to_channels_last", x, lambda y: L.call("scail_to_channels_last", xd.data_ptr(), y.data_ptr(), ad.data_ptr(), bd.data_ptr(), C, Cpad, T * hw, stream()))):
        cands = X.to_channels_last_candidates(xs, a, b, Cpad)
        assert int((cands[0] != cands[1]).sum()) > 0
        frames = [X.framed(c) for c in cands]
        before, _, inside = frames[0]
        y = d16(before)
        call(y)
        counts = X.check_buffer(h16(y), before, inside, [f[1] for f in frames], f"{what} hw={hw}")
        print(f"{what} hw={hw}: of {int(inside.sum())} elements, equal to the separate result {counts[0]}, to the fused result {counts[1]}")
    # the way back: the window of a sentinel-filled planar tensor with one guard plane behind it
    lo, hi = X.CL_CLAMPS[0]
    rows = X.cl_rows_input(Cpad, n * hw, Cpad)                          # the windowed kernel reads whole 16-byte groups: all Cpad columns hold values
    ref = X.from_channels_last_reference(rows, C, a, b, lo, hi)
    before = torch.full((C + 1, T * hw), X.SENT32, dtype=torch.int64)
    inside = torch.zeros(before.shape, dtype=torch.bool)
    inside[:C, win] = True
    want = before.clone()
    want[:C, win] = ref
    y, rd = d32(before), d16(rows)
    L.call("scail_from_channels_last_frames", rd.data_ptr(), Cpad, y.data_ptr(), ad.data_ptr(), bd.data_ptr(), C, T * hw, t0 * hw, n * hw, lo, hi, stream())
    X.check_buffer(h32(y), before, inside, [want], f"from_channels_last_frames hw={hw}")
    before, want, inside = X.framed(ref, sentinel=X.SENT32)
    y = d32(before)
    L.call("scail_from_channels_last", rd.data_ptr(), Cpad, y.data_ptr(), ad.data_ptr(), bd.data_ptr(), C, n * hw, lo, hi, stream())
    X.check_buffer(h32(y), before, inside, [want], f"from_channels_last hw={hw}")


# ---- 5. scail_slabs_to_rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,D,w", X.SLAB_CASES)
def test_slabs_to_rows_is_the_concatenation(L, rows, D, w):
    """slab stride rows w + 24 with sentinel gaps, output rows ldy = D + 8 with a guard row"""
    buf, slabs = X.slab_input(rows, D, w)
    before, want, inside = X.framed(X.slab_reference(slabs), rows_after=1, cols_after=8)
    xd, y = d16(buf), d16(before)
    L.call("scail_slabs_to_rows", xd.data_ptr(), w, rows * w + X.SLAB_GAP, y.data_ptr(), D + 8, rows, D, stream())
    X.check_buffer(h16(y), before, inside, [want], f"slabs_to_rows rows={rows} D={D} slab_w={w}")
    assert torch.equal(h16(xd), buf)
