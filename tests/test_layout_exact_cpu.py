"""What tests/test_layout_exact_gpu.py rests on, checked without a GPU (tests/layout_exact.py): the permutation inputs are distinct; the torch-index
reference of the token layout, pushed through the tiny config's patch embedding in fp64, is the oracle's patch_embed; the timestep reference is the
oracle's and leaves NO element of any case undecided; the integer RNE formula is torch's conversion; the fused multiply-add is the exact one; the
inputs separate the contraction candidates; the checkers reject every seeded fault; and the older entry points refuse bad arguments on the host."""
import fractions

import numpy as np
import pytest
import torch

import layout_exact as X

ALL_TOKEN_CASES = X.PATCHIFY_CASES + X.CHARS_CASES


def case(id):
    return next(c for c in ALL_TOKEN_CASES if c["id"] == id)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------------
def test_permutation_inputs_are_distinct_and_sizes_sit_off_the_block():
    """every source element of a data-movement case is its own bit pattern, none of them a NaN, +-0 or 1; thread counts are off the 256-thread block
    wherever the shapes leave the choice (16 H W of unpatchify at 8 x 12 is 6 blocks whatever B and T are)"""
    for c in ALL_TOKEN_CASES:
        inp = X.patchify_inputs(c)
        srcs = (inp["ref"], inp["pose"]) if c["rounding"] else (inp["ref"], inp["pose"], inp["xw"] >> 16)
        assert X.all_distinct(*srcs), c["id"]
        for s in srcs:
            assert not bool((X.nan_bits(s) | (s == 0) | (s == 0x8000) | (s == X.ONE16)).any()), c["id"]
        if c["rounding"]:
            assert not bool(X.nan_word(inp["xw"]).any())
            w = inp["xw"]
            assert bool(((w & 0xFFFF) == 0x8000).any()) and bool(((w & 0x7F800000) == 0).any()) and bool((w == 0x7F7FFFFF).any()) and bool((w == 0x80000000).any())
        else:
            assert bool(((inp["xw"] & 0xFFFF) == 0).all())
        assert X.patchify_threads(c) % X.BLOCK != 0, c["id"]
    assert min(X.patchify_threads(c) for c in X.PATCHIFY_CASES) < X.BLOCK < max(X.patchify_threads(c) for c in X.PATCHIFY_CASES)
    assert min(X.patchify_threads(c) for c in X.CHARS_CASES) < X.BLOCK < max(X.patchify_threads(c) for c in X.CHARS_CASES)
    for u in X.UNPATCHIFY_CASES:
        assert X.all_distinct(X.unpatchify_tokens(*u))
    assert any(b * t * 16 * h * w < X.BLOCK for b, t, h, w in X.UNPATCHIFY_CASES) and any((b * t * 16 * h * w) % X.BLOCK for b, t, h, w in X.UNPATCHIFY_CASES)
    for t in X.TRANSPOSE_CASES:
        assert X.all_distinct(X.transpose_input(*t))
    for s in X.SLAB_CASES:
        buf, slabs = X.slab_input(*s)
        assert X.all_distinct(slabs) and not bool((slabs == X.SENT16).any()) and (s[0] * s[1] // 8) % X.BLOCK != 0
    assert X.all_bf16_patterns()[:65536].unique().numel() == 65536 and X.all_bf16_patterns().numel() % X.BLOCK == X.CONV_TAIL
    w = X.all_conversion_words()
    assert w.numel() == 6 * 65536 + X.CONV_TAIL and w.numel() % X.BLOCK != 0 and all(n % X.BLOCK != 0 for n in X.WRAPPER_N + X.CFG_EULER_N + X.CL_N)
    for layers, B, width in X.ADALN_CASES[:3]:
        assert (layers * B * width) % X.BLOCK != 0


# ---- the token layout is the model's ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", ["8x12x3-b3-BB-k128", "12x20x2-b3-1B-k80", "4x4x1-b1-k80"])
def test_token_reference_through_the_patch_embedding_is_the_oracles(id):
    """moderate random values in place of the bit patterns (those span 76 orders of magnitude, which an fp64 sum cannot resolve element by element);
    the SAME reference function; x is general fp32, so the rounding of the noise tokens is tied too"""
    from oracle import scail_oracle as O
    c = case(id)
    g = torch.Generator().manual_seed(len(id))
    shapes = {k: v.shape for k, v in X.patchify_inputs(c).items()}
    inp = dict(xw=X.words_of(torch.randn(shapes["xw"], generator=g)), ref=X.bits_of(torch.randn(shapes["ref"], generator=g).to(X.BF16)),
               pose=X.bits_of(torch.randn(shapes["pose"], generator=g).to(X.BF16)))
    cfg = O.DiTConfig(**O.TINY)
    sd = {k: v.double() for k, v in O.make_state_dict(cfg).items() if "patch_embed" in k}
    D = cfg.hidden_size
    tok = X.bf16_of(X.patchify_reference(c, inp)).double()
    assert float(tok[..., 80:].abs().max()) == 0 if c["kpad"] > 80 else True
    n = (1 + c["T"]) * (c["H"] // 2) * (c["W"] // 2)
    got = torch.cat([tok[:, sl, :80] @ sd[f"mixins.patch_embed.{name}.weight"].reshape(D, 80).t() + sd[f"mixins.patch_embed.{name}.bias"]
                     for name, sl in (("proj", slice(0, n)), ("proj_pose", slice(n, None)))], 1)
    want = O.patch_embed(cfg, sd, *X.patchify_model_view(c, inp))
    assert want.dtype == torch.float64 and got.shape == want.shape
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)


def _token_buffers(c, inp):
    return X.framed(X.patchify_reference(c, inp).view(-1, c["kpad"]))


@pytest.mark.parametrize("fault,id", [("pq_swapped", "4x4x1-b1-k80"), ("pose_w2", "8x12x3-b3-11-k128"), ("ref_broadcast", "8x12x3-b3-B1-k80"),
                                      ("mask_on_noise", "4x4x1-b3-BB-k88"), ("pad_nonzero", "12x20x2-b1-k88"),
                                      ("char_frame_swapped", "c2-8x12x3-b3-B1-k88"), ("truncate", "8x12x3-b3-B1-k88-rounding"),
                                      ("truncate", "c2-8x12x3-b3-1B-k80-rounding")])
def test_token_checker_rejects_seeded_faults(fault, id):
    """7 faults: p and q swapped, the pose tokens indexed with w2 where w4 belongs, the ref batch broadcast although n_ref == B, the mask set on noise
    tokens, a non-zero pad column, the character and frame order of the pose swapped, truncation instead of RNE; and the reference itself passes"""
    c = case(id)
    inp = X.patchify_inputs(c)
    before, want, inside = _token_buffers(c, inp)
    assert X.check_buffer(want, before, inside, [want], id) == [int(inside.sum())]
    bad = before.clone()
    bad[inside] = X.patchify_reference(c, inp, fault).flatten()
    assert X.rejects(bad, before, inside, [want]), f"{fault} passes on {id}"


def test_buffer_checker_sees_the_guards_and_the_sentinel():
    """3 faults: a guard row written, a guard column written, a result word left at the sentinel"""
    res = X.patterns([6 * 8], 1)[0].view(6, 8)
    before, want, inside = X.framed(res, rows_after=1, cols_after=3)
    assert before.shape == (7, 11) and int(inside.sum()) == 48
    for pos in ((6, 0), (2, 9)):
        bad = want.clone()
        bad[pos] = 0
        assert X.rejects(bad, before, inside, [want])
    bad = want.clone()
    bad[3, 3] = X.SENT16
    assert X.rejects(bad, before, inside, [want])
    other = want.clone()
    other[0, 0] += 1
    assert X.check_buffer(other, before, inside, [want, other], "two candidates") == [47, 48]


def test_unpatchify_reference_is_the_final_layers_rearrangement():
    """the (o p q c) columns of dit...:764-784 as the existing test states them, on distinct patterns"""
    for B, T, H, W in X.UNPATCHIFY_CASES:
        tok = X.unpatchify_tokens(B, T, H, W)
        want = tok.reshape(B, T, H // 2, W // 2, 1, 2, 2, 16).permute(0, 1, 4, 7, 2, 5, 3, 6).reshape(B, T, 16, H, W) << 16
        assert torch.equal(X.unpatchify_reference(tok, B, T, H, W), want)
        assert torch.equal(X.unpatchify_reference(tok, B, T, H, W)[0, 0, 5, 1, 0], tok[0, 0, 32 + 5] << 16)


# ---- conversions --------------------------------------------------------------------------------------------------------------------------------------
def test_integer_rne_formula_is_torchs_conversion():
    """on all 393 221 conversion words and the rounding words of the token cases; 2 faults rejected by the checker: truncation, denormals flushed"""
    for w in (X.all_conversion_words(), X.rounding_words(20000, 3)):
        ok = ~X.nan_word(w)
        assert torch.equal(X.bits_of(X.f32_of(w).to(X.BF16))[ok], X.rne_bits(w)[ok])
        assert bool(X.nan_bits(X.bits_of(X.f32_of(w).to(X.BF16))[~ok]).all())
    w = X.all_conversion_words()
    den_in, den_out = X.check_f32_to_bf16(torch.where(X.nan_word(w), torch.full_like(w, 0x7FC0), X.rne_bits(w)), w, "the formula")
    assert den_in > 700 and den_out > 700
    # ties at every exponent, both ways; overflow to infinity
    assert int(X.rne_bits(torch.tensor(0x3F808000))) == 0x3F80 and int(X.rne_bits(torch.tensor(0x3F818000))) == 0x3F82
    assert int(X.rne_bits(torch.tensor(0x7F7F8000))) == 0x7F80 and int(X.rne_bits(torch.tensor(0xFF7FFFFF))) == 0xFF80
    assert int(X.rne_bits(torch.tensor(0x00008000))) == 0 and int(X.rne_bits(torch.tensor(0x00008001))) == 1 and int(X.rne_bits(torch.tensor(0x80000000))) == 0x8000
    for faulty in (X.trunc_bits(w), torch.where((w & 0x7F800000) == 0, w >> 16 & 0x8000, X.rne_bits(w))):
        with pytest.raises(AssertionError, match="not rounded to nearest even"):
            X.check_f32_to_bf16(faulty, w, "fault")
    with pytest.raises(AssertionError, match="NaN word"):
        X.check_f32_to_bf16(X.rne_bits(w), w, "NaN to number")          # the formula carries 0x7f80ffff over into 0x7f81, but 0x7fffffff into 0x8000 = -0


# ---- timestep embedding -------------------------------------------------------------------------------------------------------------------------------
def test_timestep_reference_is_the_oracles_and_decides_every_element():
    from oracle import scail_oracle as O
    assert X.sampler_timesteps().shape == (50,) and X.sampler_timesteps().dtype == torch.float32
    assert float(X.sampler_timesteps()[0]) == 1000.0 and bool((X.sampler_timesteps()[1:] < X.sampler_timesteps()[:-1]).all())
    for dim, n in X.TS_CASES:
        t = X.timestep_values(n)
        ref, m, m0 = X.timestep_reference(t, dim)
        assert ref.shape == (n, dim) and torch.equal(ref.float(), O.timestep_embedding(t, dim))
        assert bool((m <= m0).all())
        und, und0 = int((~X.timestep_decided(ref, m)).sum()), int((~X.timestep_decided(ref, m0)).sum())
        print(f"timestep dim={dim} n={n}: undecided {und} of {ref.numel()} (with the margin 8 * 2^-52 (|t f| + 1): {und0})")
        assert und == 0, (dim, n)
        assert X.check_timestep(X.words_of(ref.float()), ref, m, "the reference") == 0
    # the two replaced steps of the schedule: the only ones whose reference has an undecided element, and the replacement is the neighbouring fp32
    t50, sched = X.timestep_values(50), X.sampler_timesteps()
    changed = (t50 != sched).nonzero().flatten().tolist()
    assert changed == list(X.TS_REPLACED) and torch.equal(t50[changed], torch.nextafter(sched[changed], torch.tensor(2000.0)))
    und_steps = set()
    for dim in X.TS_DIMS:
        ref, m, _ = X.timestep_reference(sched, dim)
        und_steps |= set((~X.timestep_decided(ref, m)).any(1).nonzero().flatten().tolist())
    assert und_steps == set(X.TS_REPLACED)
    assert 300 // 2 > 128                                            # dim 300 takes two passes of the kernel's 128-thread loop


@pytest.mark.parametrize("fault,dim,n", [("cos_sin_swapped", 256, 50), ("f32_frequency", 256, 50), ("j_over_dim", 256, 50), ("last_column", 7, 3),
                                         ("cos_sin_swapped", 6, 1), ("f32_frequency", 300, 3), ("j_over_dim", 513, 1)])
def test_timestep_checker_rejects_seeded_faults(fault, dim, n):
    """4 faults: cos and sin swapped, the frequency rounded to fp32, j / dim in place of j / half, a non-zero last column at an odd dim"""
    t = X.timestep_values(n)
    ref, m, _ = X.timestep_reference(t, dim)
    bad, _, _ = X.timestep_reference(t, dim, fault)
    with pytest.raises(AssertionError, match="not the correctly rounded value"):
        X.check_timestep(X.words_of(bad.float()), ref, m, fault)


# ---- multiply-adds that may contract ------------------------------------------------------------------------------------------------------------------
def test_fma32_is_the_exact_fused_multiply_add():
    """against exact rationals on the elements of a cfg_euler case and of a channels-last case; and on a constructed operand triple where the fp64
    sum rounded a second time gives another fp32 value"""
    a, b, c = np.float32(1 + 2.0 ** -23), np.float32(1 - 2.0 ** -23), np.float32(2.0 ** 24 + 2)
    assert float(X.fma32(a, b, c).reshape(-1)[0]) == X.fma32_exact(float(a), float(b), float(c)) == 2.0 ** 24 + 2
    assert float(np.float32(np.float64(a) * np.float64(b) + np.float64(c))) == 2.0 ** 24 + 4          # the double rounding the helper avoids
    assert X.round_fraction_f32(fractions.Fraction(2 ** 24 + 1)) == 2.0 ** 24 and X.round_fraction_f32(fractions.Fraction(2 ** 24 + 3)) == 2.0 ** 24 + 4
    assert X.round_fraction_f32(fractions.Fraction(-3, 8)) == -0.375 and X.round_fraction_f32(fractions.Fraction(1, 3)) == float(np.float32(1 / 3))
    x, v = X.cfg_euler_inputs(255)
    d = (v[255:] - v[:255]).numpy()
    got = X.fma32(X.CFG, d, v[:255].numpy())
    assert all(float(got[i]) == X.fma32_exact(float(X.CFG), float(d[i]), float(v[i])) for i in range(255))
    sa, sb = X.cl_scale_shift(12, True, True)
    xs = X.cl_planar_input(12, 45, sa, sb)
    got = X.fma32(xs.numpy(), sa[:, None].numpy(), sb[:, None].numpy())
    assert got.shape == (12, 45) and got.dtype == np.float32
    assert all(float(got[i, j]) == X.fma32_exact(float(xs[i, j]), float(sa[i]), float(sb[i])) for i in range(12) for j in range(45))


def test_cfg_euler_inputs_separate_the_candidates_and_the_checker_rejects_faults():
    """cfg = 3.7, ds = -0.0371 as fp32 values; every pair of the four candidates differs somewhere at the two larger sizes.  3 faults: vc and vu
    swapped, cfg * vc - vu, the expression accumulated in fp64"""
    assert float(X.CFG) == float(np.float32(3.7)) and float(X.DSIGMA) == float(np.float32(-0.0371))
    for n in X.CFG_EULER_N:
        x, v = X.cfg_euler_inputs(n)
        cands = X.cfg_euler_candidates(x, v)
        assert len(cands) == 4 and all(c.shape == (n,) for c in cands)
        sep = {(i, j): int((cands[i] != cands[j]).sum()) for i in range(4) for j in range(i + 1, 4)}
        print(f"cfg_euler n={n}: elements on which two candidates differ {sep}")
        if n > 1:
            assert all(k > 0 for k in sep.values()), sep
        before, want, inside = X.framed(cands[0][None], rows_after=0, cols_after=64, sentinel=X.SENT32)
        for k, cand in enumerate(cands):
            buf = before.clone()
            buf[0, :n] = cand
            counts = X.check_buffer(buf, before, inside, [X.framed(cc[None], 0, 64, X.SENT32)[1] for cc in cands], "candidate")
            assert counts[k] == n
        if n > 1:
            for fault in ("swapped", "no_parentheses", "fp64"):
                buf = before.clone()
                buf[0, :n] = X.cfg_euler_candidates(x, v, fault)[0]
                assert X.rejects(buf, before, inside, [X.framed(cc[None], 0, 64, X.SENT32)[1] for cc in cands]), (fault, n)


def test_channels_last_inputs_separate_the_candidates():
    """a general a: the separate and the fused x * a + b differ after the rounding to bf16 on a non-zero count of elements wherever both a and b are
    given (at every N with more than a handful of elements: the tie inputs of layout_exact._tie_inputs), and coincide where one of them is missing
    (x * 1 + b and x * a + 0 are one rounding either way).  1 fault: (x + b) * a"""
    for C, Cpad in X.CL_SHAPES:
        for has_a, has_b in X.CL_AB:
            a, b = X.cl_scale_shift(C, has_a, has_b)
            if a is not None:
                fr, ex = torch.frexp(a)
                assert not bool((fr == 0.5).any()), "a power of two"
            diff = []
            for N in X.CL_N:
                sep, fused = X.to_channels_last_candidates(X.cl_planar_input(C, N, a, b), a, b, Cpad)
                assert sep.shape == (N, Cpad) and bool((sep[:, C:] == 0).all()) and bool((fused[:, C:] == 0).all())
                diff.append(int((sep != fused).sum()))
            print(f"to_channels_last C={C} Cpad={Cpad} a={has_a} b={has_b}: separate and fused differ on {diff} elements at N = {X.CL_N}")
            assert all((d > 0) == (has_a and has_b) for d in diff[1:]) and (has_a and has_b or diff[0] == 0)
    for hw in X.FRAMES_HW:
        fc = X.FRAMES_CASE
        a, b = X.cl_scale_shift(fc["C"], True, True)
        sep, fused = X.to_channels_last_candidates(X.cl_planar_input(fc["C"], fc["T"] * hw, a, b, seed=1), a, b, fc["Cpad"])
        assert int((sep != fused).sum()) > 0
    C, Cpad, N = 12, 16, X.CL_N[2]
    a, b = X.cl_scale_shift(C, True, True)
    x = X.cl_planar_input(C, N, a, b)
    cands = X.to_channels_last_candidates(x, a, b, Cpad)
    wrong = torch.zeros(N, Cpad, dtype=torch.int64)
    wrong[:, :C] = X.rne_bits(X.words_of((x + b[:, None]) * a[:, None])).t()
    before, _, inside = X.framed(cands[0])
    buf = before.clone()
    buf[:N] = wrong
    assert X.rejects(buf, before, inside, [X.framed(cc)[1] for cc in cands])


def test_from_channels_last_reference_pins_the_clamp_and_the_nan():
    """the NaN of the input comes out as lo, the infinities as hi and lo; lo == hi gives that value everywhere; sentinel columns are not read"""
    C, N, ldx = 3, 45, 16
    buf = X.cl_rows_input(C, N, ldx)
    assert bool((buf[:, C:] == X.SENT16).all()) and int(X.nan_bits(buf[:, :C]).sum()) == 1
    a, b = X.cl_scale_shift(C, True, True)
    for lo, hi in X.CL_CLAMPS:
        y = X.f32_of(X.from_channels_last_reference(buf, C, a, b, lo, hi))
        assert not bool(torch.isnan(y).any()) and float(y.min()) >= np.float32(lo) and float(y.max()) <= np.float32(hi)
        assert float(y.t().flatten()[2]) == float(np.float32(lo))       # the NaN
        assert float(y.t().flatten()[9]) == float(np.float32(hi)) and float(y.t().flatten()[16]) == float(np.float32(lo))    # +inf, -inf
    y = X.f32_of(X.from_channels_last_reference(buf, C, None, None, -0.75, 0.75))
    plain = X.bf16_of(buf[:, :C]).float().t()
    ok = ~torch.isnan(plain)
    assert torch.equal(y[ok], plain.clamp(-0.75, 0.75)[ok])


def test_slab_and_transpose_references():
    buf, slabs = X.slab_input(37, 64, 16)
    want = X.slab_reference(slabs)
    assert want.shape == (37, 64) and torch.equal(want[5, 16:32], buf[1, 5 * 16:6 * 16]) and bool((buf[:, 37 * 16:] == X.SENT16).all())
    t = X.transpose_input(65, 130, 3)
    assert t.transpose(1, 2).shape == (3, 130, 65)


# ---- host-side refusals -------------------------------------------------------------------------------------------------------------------------------
A = 1 << 20                                     # a 256-byte aligned non-null address: the checks fire before anything is dereferenced
BIG = 1 << 14
REFUSALS = [
    ("scail_unpatchify", (A, A, -1, 1, 2, 2, None)), ("scail_unpatchify", (A, A, 1, 1, 3, 2, None)), ("scail_unpatchify", (A, A, 1, 1, 2, 3, None)),
    ("scail_unpatchify", (None, A, 1, 1, 2, 2, None)), ("scail_unpatchify", (A, None, 1, 1, 2, 2, None)),
    ("scail_unpatchify", (A, A, BIG, BIG, BIG, BIG, None)), ("scail_unpatchify", (A, A, 1, 1, 1 << 31, 2, None)),
    ("scail_patchify", (A, A, A, A, -1, 1, 1, 1, 8, 8, 128, None)), ("scail_patchify", (A, A, A, A, 1, 1, 1, -1, 8, 8, 128, None)),
    ("scail_patchify", (None, A, A, A, 1, 1, 1, 1, 8, 8, 128, None)), ("scail_patchify", (A, None, A, A, 1, 1, 1, 1, 8, 8, 128, None)),
    ("scail_patchify", (A, A, None, A, 1, 1, 1, 1, 8, 8, 128, None)), ("scail_patchify", (A, A, A, None, 1, 1, 1, 1, 8, 8, 128, None)),
    ("scail_patchify", (A + 2, A, A, A, 1, 1, 1, 1, 8, 8, 128, None)), ("scail_patchify", (A, A + 1, A, A, 1, 1, 1, 1, 8, 8, 128, None)),
    ("scail_patchify", (A, A, A + 1, A, 1, 1, 1, 1, 8, 8, 128, None)), ("scail_patchify", (A, A, A, A + 8, 1, 1, 1, 1, 8, 8, 128, None)),
    ("scail_patchify", (A, A, A, A, 32767, 1, 1, 32767, 32764, 32764, 128, None)),
    ("scail_timestep_embedding", (A, A, 1, 0, None)), ("scail_timestep_embedding", (A, A, -1, 256, None)),
    ("scail_timestep_embedding", (None, A, 1, 256, None)), ("scail_timestep_embedding", (A, None, 1, 256, None)),
    ("scail_timestep_embedding", (A, A, 1 << 31, 256, None)),
    ("scail_adaln_table", (A, A, A, -1, 1, 8, None)), ("scail_adaln_table", (A, A, A, 1, 1, -8, None)), ("scail_adaln_table", (None, A, A, 1, 1, 8, None)),
    ("scail_adaln_table", (A, None, A, 1, 1, 8, None)), ("scail_adaln_table", (A, A, None, 1, 1, 8, None)),
    ("scail_adaln_table", (A, A, A, (1 << 20) - 1, (1 << 20) - 1, (1 << 20) - 1, None)),
    ("scail_cfg_euler", (A, A, -1, 3.7, -0.03, None)), ("scail_cfg_euler", (A, A, 1 << 39, 3.7, -0.03, None)),
    ("scail_cfg_euler", (None, A, 8, 3.7, -0.03, None)), ("scail_cfg_euler", (A, None, 8, 3.7, -0.03, None)),
    ("scail_f32_to_bf16", (A, A, -1, None)), ("scail_f32_to_bf16", (A, A, 1 << 39, None)), ("scail_f32_to_bf16", (None, A, 8, None)),
    ("scail_f32_to_bf16", (A, None, 8, None)),
    ("scail_bf16_to_f32", (A, A, -1, None)), ("scail_bf16_to_f32", (A, A, 1 << 39, None)), ("scail_bf16_to_f32", (None, A, 8, None)),
    ("scail_bf16_to_f32", (A, None, 8, None)),
    ("scail_transpose2d", (A, 8, 64, A, 8, 64, -1, 8, 1, None)), ("scail_transpose2d", (A, 8, 64, A, 8, 64, 8, 8, -1, None)),
    ("scail_transpose2d", (A, 8, 64, A, 64 * 65535 + 1, 64, 64 * 65535 + 1, 8, 1, None)), ("scail_transpose2d", (A, 8, 64, A, 8, 64, 8, 8, 65536, None)),
    ("scail_transpose2d", (None, 8, 64, A, 8, 64, 8, 8, 1, None)), ("scail_transpose2d", (A, 8, 64, None, 8, 64, 8, 8, 1, None)),
    ("scail_transpose2d", (A, 7, 64, A, 8, 64, 8, 8, 1, None)), ("scail_transpose2d", (A, 8, 64, A, 7, 64, 8, 8, 1, None)),
    ("scail_to_channels_last", (A, A, None, None, 0, 8, 4, None)), ("scail_to_channels_last", (A, A, None, None, 9, 8, 4, None)),
    ("scail_to_channels_last", (A, A, None, None, 16, 16, 1 << 39, None)), ("scail_to_channels_last", (None, A, None, None, 3, 8, 4, None)),
    ("scail_to_channels_last", (A, None, None, None, 3, 8, 4, None)), ("scail_to_channels_last", (A, A, None, None, 3, 8, -4, None)),
    ("scail_from_channels_last", (A, 8, A, None, None, 0, 4, -1.0, 1.0, None)), ("scail_from_channels_last", (A, 8, A, None, None, 9, 4, -1.0, 1.0, None)),
    ("scail_from_channels_last", (A, 16, A, None, None, 16, 1 << 39, -1.0, 1.0, None)),
    ("scail_from_channels_last", (None, 8, A, None, None, 3, 4, -1.0, 1.0, None)), ("scail_from_channels_last", (A, 8, None, None, None, 3, 4, -1.0, 1.0, None)),
    ("scail_from_channels_last", (A, 8, A, None, None, 3, -4, -1.0, 1.0, None)),
]
EMPTY_CALLS = [
    ("scail_unpatchify", (None, None, 0, 1, 2, 2, None)), ("scail_patchify", (None, None, None, None, 0, 1, 1, 1, 8, 8, 128, None)),
    ("scail_timestep_embedding", (None, None, 0, 256, None)), ("scail_adaln_table", (None, None, None, 0, 1, 8, None)),
    ("scail_cfg_euler", (None, None, 0, 3.7, -0.03, None)), ("scail_f32_to_bf16", (None, None, 0, None)), ("scail_bf16_to_f32", (None, None, 0, None)),
    ("scail_transpose2d", (None, 8, 64, None, 8, 64, 0, 8, 1, None)), ("scail_to_channels_last", (None, None, None, None, 3, 8, 0, None)),
    ("scail_from_channels_last", (None, 8, None, None, None, 3, 0, -1.0, 1.0, None)),
]


def test_older_entry_points_refuse_bad_arguments_without_gpu():
    """every bad call returns 1 before any launch (this machine has no device: a launch would fail with 2) and the message names the function;
    an empty call returns 0 before the pointers are looked at"""
    from scail_amd import lib as L
    lib = L.load()
    for name, args in REFUSALS:
        rc = getattr(lib, name)(*args)
        msg = lib.scail_last_error().decode()
        assert rc == 1, (name, args, rc, msg)
        assert msg.startswith(name + ":"), (name, args, msg)
        with pytest.raises(L.ScailHipError, match=name):
            L.call(name, *args)
    for name, args in EMPTY_CALLS:
        assert getattr(lib, name)(*args) == 0, (name, args)
    assert {n for n, _ in REFUSALS} == {n for n, _ in EMPTY_CALLS} and len({n for n, _ in REFUSALS}) == 10
