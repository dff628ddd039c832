"""Exact-arithmetic helpers for the VAE convolution tests (tests/test_conv_exact_cpu.py, tests/test_conv_exact_gpu.py).

Operands.  x = (integers in [-3, 3]) / 2, w = (integers in [-2, 2]) / 4, bias = integers in [-8, 8], residual = integers in [-64, 64]: all exact in
bf16.  In units of 2^-3 every product is an integer of magnitude <= 6, so a convolution with K = taps x Cin <= 27 x 384 terms has
sum |x w| <= 6 K <= 62 208 units; with the bias (<= 64 units) and the residual (<= 512 units) every partial sum stays below 2^24 units: EVERY fp32
partial sum is exact, in any order and for any MFMA shape.  A kernel therefore has to reproduce conv_ref -- the fp64 convolution + bias (+ residual),
rounded ONCE to bf16 -- bit for bit.

Norm epilogues.  SiLU(RMS_norm(s) * gamma) of the bf16-rounded sum s is not exact in fp32, so the kernels are held to "correctly rounded wherever
fp32 arithmetic can decide it": check_rounded_bf16 wants every element to be one of the two bf16 neighbours of the fp64 reference, and to BE the
round-to-nearest-even one wherever the reference is farther than MARGIN x |ref| from a rounding boundary.

MARGIN, from the operation chain of rms_silu_kernel (csrc/conv.hip; the fused epilogues of conv_halo_kernel<4, ..>, conv_direct_kernel<.., true>
and asmgen/conv4.py norm_silu run the same chain), first-order relative errors in units of u = 2^-24 (one fp32 rounding):
  q = sum of C squares (96 to 384 terms; the squares of bf16 values are exact).  A term takes part in at most D additions: 24 serial + 4 butterfly
      steps in rms_silu_kernel, 24 + 2 in the generated epilogue, 48 + 1 in the hipcc fused epilogues.  All terms are >= 0, so |dq| <= D u q, D <= 49;
  sqrt(q): halves it ............................ 24.5        v_sqrt, 1 ulp = 2 u ............ 2
  v_rcp, 1 ulp .................................. 2           sqrtf(C), rounded constant ..... 1
  three multiplications (sqrt(C) r, s inv, gamma) 3           => t = s sqrt(C) / ||s|| gamma : 32.5 u   (the whole chain when SiLU is off)
  a = -1.4427 t: the rounded constant 1 + the multiplication 1 + t's 32.5 = 34.5 u relative on a, i.e. |a| 34.5 u absolute;
  e = exp2(a): ln 2 |a| 34.5 u = |t| 34.5 u from its argument, + v_exp 1 ulp = 2 u;
  d = 1 + e: 1 u of its own + e / (1 + e) (34.5 |t| + 2) u inherited;   v_rcp: 2 u;   t * r: 1 u.
  SiLU(t): 32.5 + 1 + 2 + 1 + sigmoid(-t) (34.5 |t| + 2)  <=  (38.5 + 34.5 |t|) u for t < 0, and <= 48 u for t > 0 (sigmoid(-t) t <= 0.2785).
|t| = |s| sqrt(C) / ||s|| |gamma| is the size of a unit-variance sample times gamma: |t| <= 4 for all but ~1e-4 of the elements, where the BUDGET is
(38.5 + 138) u = 176.5 u = 1.05e-5 = 2^-16.5.  MARGIN = 4 x BUDGET = 706 u = 4.21e-5 = 2^-14.5.  The factor 4 also covers the worst case of every
element with t >= -19.3 (38.5 + 34.5 x 19.3 = 706); T_NEG_MIN = -19 is a condition on the inputs that the CPU tests assert.  A bf16 significand
f in [1, 2) has rounding boundaries 2^-7 / f apart in relative terms, so the share of elements inside the margin is about
2 x MARGIN x 2^7 x E[f] = 369 x MARGIN = 1.6 %; UNDECIDED_CAP = 3 % is again a condition on the inputs, not a tolerance on a kernel.

The module reads nothing outside tests/ and scail_amd/."""
import functools

import torch
import torch.nn.functional as F

U = 2.0 ** -24
BUDGET = (38.5 + 34.5 * 4.0) * U
MARGIN = 4.0 * BUDGET                      # 706 u = 4.21e-5
T_NEG_MIN = -19.0                          # most negative t = RMS_norm(s) * gamma the margin covers in the worst case (docstring)
UNDECIDED_CAP = 0.03
BF16 = torch.bfloat16


# ---- operands -----------------------------------------------------------------------------------------------------------------
def _is_bf16(t):
    return torch.equal(t.to(BF16).to(t.dtype), t)


def exact_operands(cin, cout, k, thw, seed, out_thw=None):
    """x (cin, T, H, W), w (cout, cin, *k), bias (cout), resid (To, Ho, Wo, cout) channels-last, gamma (cout): fp32 tensors on the CPU.  x, w, bias and
    resid are exact in bf16 (module docstring); output channel 0 of w is structured and asymmetric; gamma = 1 + 0.1 randn."""
    g = torch.Generator().manual_seed(seed)
    T, H, W = thw
    x = torch.randint(-3, 4, (cin, T, H, W), generator=g).float() * 0.5
    w = torch.randint(-2, 3, (cout, cin) + tuple(k), generator=g).float()
    nk = w[0].numel()
    w[0] = (torch.arange(nk).remainder(5).float() - 2).reshape(w[0].shape)      # a structured, non-symmetric row
    w = w * 0.25
    bias = torch.randint(-8, 9, (cout,), generator=g).float()
    resid = torch.randint(-64, 65, tuple(out_thw or thw) + (cout,), generator=g).float()
    gamma = 1 + 0.1 * torch.randn(cout, generator=g)
    assert all(_is_bf16(t) for t in (x, w, bias, resid))
    assert 6 * nk * 8 + 64 + 512 < 2 ** 24, "exactness bound: every fp32 partial sum is an integer below 2^24 in units of 2^-3"
    return dict(x=x, w=w, bias=bias, resid=resid, gamma=gamma)


def integer_rows(rows, C, seed):
    """rows x C integers in [-3, 3] for scail_rms_silu alone: row 0 all zero, row 1 one non-zero element -- negative where t = -sqrt(C) gamma stays above
    T_NEG_MIN (C <= 96), positive else -- and gamma = 1 + 0.1 randn."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (rows, C), generator=g).float()
    x[0] = 0
    x[1] = 0
    x[1, C // 3] = -3.0 if C <= 96 else 3.0
    return x, 1 + 0.1 * torch.randn(C, generator=g)


# ---- references ---------------------------------------------------------------------------------------------------------------
def conv_sum(x, w, bias=None, resid=None, stride=(1, 1, 1), pad=None, ups=False):
    """The exact sum in fp64, channels-last (To, Ho, Wo, cout): the geometry vocabulary of ops.conv3d_cl.  pad = (pt, ph, pw) zero frames / rows / columns
    in FRONT (default: causal 'same', (kt - 1, kh // 2, kw // 2)); behind: none in time, ph / pw in space -- or, with a spatial stride of 2, the one row and
    column of ZeroPad2d((0, 1, 0, 1)); ups: the nearest-exact 2x upsample in front of the convolution."""
    x, w = x.double(), w.double()
    if w.dim() == 4:
        w = w.unsqueeze(2)
    kt, kh, kw = w.shape[2:]
    if pad is None:
        pad = (kt - 1, kh // 2, kw // 2)
    if ups:
        x = F.interpolate(x.permute(1, 0, 2, 3), scale_factor=(2.0, 2.0), mode="nearest-exact").permute(1, 0, 2, 3)
    s2 = stride[1] == 2
    xp = F.pad(x, (pad[2], 1 if s2 else pad[2], pad[1], 1 if s2 else pad[1], pad[0], 0))
    y = F.conv3d(xp[None], w, None, stride=stride)[0].permute(1, 2, 3, 0)
    if bias is not None:
        y = y + bias.double()
    if resid is not None:
        y = y + resid.double()
    return y.contiguous()


def round_bf16(v64):
    """ONE rounding, to nearest even: the fp32 value of an exact sum is exact."""
    return v64.float().to(BF16)


def conv_ref(x, w, bias=None, resid=None, stride=(1, 1, 1), pad=None, ups=False, ot_mul=1, ot_off=0, frames=None, ldc=None):
    """conv_sum rounded once to bf16.  With ``frames`` / ``ldc``: the whole output tensor (frames, Ho, Wo, ldc) a kernel should leave behind -- result
    frame t in slot t * ot_mul + ot_off, channels [0, cout), NaN wherever nothing may be written."""
    r = round_bf16(conv_sum(x, w, bias, resid, stride, pad, ups))
    if frames is None and ldc is None:
        assert ot_mul == 1 and ot_off == 0
        return r
    To, Ho, Wo, N = r.shape
    out = torch.full((frames or To, Ho, Wo, ldc or N), float("nan"), dtype=BF16)
    out[ot_off::ot_mul][:To, :, :, :N] = r
    return out


def norm_silu_ref(s_bf16, gamma, silu=True):
    """fp64: t = s sqrt(C) / max(||s||_2, 1e-12) gamma over the last (channel) dimension of the bf16-ROUNDED sum, then t / (1 + exp(-t))."""
    s = s_bf16.double()
    C = s.shape[-1]
    t = s * (float(C) ** 0.5) / s.norm(dim=-1, keepdim=True).clamp_min(1e-12) * gamma.double()
    return t / (1 + torch.exp(-t)) if silu else t


def norm_t(s_bf16, gamma):
    return norm_silu_ref(s_bf16, gamma, silu=False)


def norm_silu_fp32(s_bf16, gamma, silu=True):
    """the kernels' chain restated with IEEE fp32 operations (torch on the CPU)"""
    s = s_bf16.float()
    q = (s * s).sum(-1, keepdim=True)
    inv = torch.tensor(float(s.shape[-1])).sqrt() * (1.0 / q.sqrt().clamp_min(1e-12))
    t = s * inv * gamma.float()
    return t * (1.0 / (1.0 + torch.exp2(torch.tensor(-1.4426950408889634) * t))) if silu else t


# ---- checker ------------------------------------------------------------------------------------------------------------------
def bf16_neighbours(ref64):
    """(lo, hi, ulp) in fp64: the bf16 values of the same sign with |lo| <= |ref| <= |hi| (lo == hi where ref is a bf16 value)."""
    a = ref64.abs()
    _, e = torch.frexp(a)                                     # a = m 2^e, m in [0.5, 1): 8 significant bits -> ulp 2^(e - 8)
    ulp = torch.ldexp(torch.ones_like(a), (e - 8).clamp_min(-133))
    lo = torch.floor(a / ulp) * ulp
    hi = torch.where(lo == a, lo, lo + ulp)
    sgn = torch.where(ref64 < 0, -1.0, 1.0).to(a.dtype)
    return sgn * lo, sgn * hi, ulp


def check_rounded_bf16(got, ref64, margin, what=""):
    """got (bf16) against the fp64 reference: every element is one of the two bf16 neighbours of ref64, and every element whose ref64 is farther than
    margin x |ref64| from the rounding boundary between them IS the round-to-nearest-even value.  Returns the share of elements inside the margin
    (undecided); prints it and the number of elements that are not RNE(ref64).  Raises AssertionError."""
    assert got.dtype == BF16 and got.shape == ref64.shape and ref64.dtype == torch.float64
    g = got.double().cpu()
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite output"
    lo, hi, _ = bf16_neighbours(ref64)
    mid = (lo.abs() + hi.abs()) / 2
    a = ref64.abs()
    rne = torch.where(a < mid, lo, hi)                        # (a tie lies inside any margin: which side it goes to is not asked)
    rne = torch.where(lo == hi, lo, rne)
    undecided = (lo != hi) & ((a - mid).abs() <= margin * a)
    neighbour = (g == lo) | (g == hi)
    inexact = g != rne
    wrong = inexact & ~undecided
    share = float(undecided.double().mean())
    print(f"{what}: undecided share {share:.4%}, not RNE but allowed {int((inexact & undecided & neighbour).sum())} of {g.numel()}")
    if not bool(neighbour.all()):
        i = int((~neighbour).flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int((~neighbour).sum())} elements are no bf16 neighbour of the reference; first at {i}: "
                             f"got {float(g.flatten()[i])!r}, ref {float(ref64.flatten()[i])!r}")
    if bool(wrong.any()):
        i = int(wrong.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(wrong.sum())} elements are not the correctly rounded value although the reference is outside the margin; "
                             f"first at {i}: got {float(g.flatten()[i])!r}, ref {float(ref64.flatten()[i])!r}")
    return share


def assert_bits(got, want, what=""):
    """bit for bit as VALUES (+0 == -0), NaN == NaN: ``want`` carries NaN wherever nothing may be written"""
    assert got.dtype == BF16 and want.dtype == BF16 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    g, w = got.float().cpu(), want.float()
    gn, wn = torch.isnan(g), torch.isnan(w)
    assert bool((gn | ~wn).all()), f"{what}: {int((wn & ~gn).sum())} elements were written outside the output"
    assert not bool((gn & ~wn).any()), f"{what}: {int((gn & ~wn).sum())} output elements are NaN / were not written"
    bad = (g != w) & ~wn
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {int((~wn).sum())} elements differ; first at {tuple(int(v) for v in torch.unravel_index(torch.tensor(i), g.shape))}: "
                             f"got {float(g.flatten()[i])!r}, want {float(w.flatten()[i])!r}; max |d| {float((g - w)[bad].abs().max())}")


# ---- the cases of tests/test_conv_exact_gpu.py (the CPU file checks the conditions on their inputs) -----------------------------------
HALO0, HALO3, HALO4 = "conv_halo_kernel<0, 32, 1, false, ", "conv_halo_kernel<3, 32, 1, false, ", "conv_halo_kernel<4, 32, 1, false, "
K333, K133, K111 = (3, 3, 3), (3, 3), (1, 1, 1)


def _c(id, cin, cout, k, thw, plain, resid=None, opts=None, **kw):
    """plain / resid: the kernel scail_conv3d_kernel_name_for must name without / with a residual (None: that form is not run)"""
    return dict(id=id, cin=cin, cout=cout, k=k, thw=thw, plain=plain, resid=resid, opts=opts or {}, stride=kw.pop("stride", (1, 1, 1)),
                pad=kw.pop("pad", None), ups=kw.pop("ups", False), **kw)


# plain and residual epilogues: bit-exact against conv_ref
PLAIN_CASES = [
    _c("conv4c-96", 96, 96, K333, (5, 33, 40), "scail_conv4c_e0", "scail_conv4c_e3"),
    _c("conv4c-96-chunk", 96, 96, K333, (5, 33, 40), "scail_conv4c_e0", "scail_conv4c_e3", pad=(0, 1, 1)),       # two cache frames in front, no padding
    _c("conv4-96", 96, 96, K333, (5, 33, 40), "scail_conv4_e0", "scail_conv4_e3", {"conv4_cont": 0}),
    _c("conv4-96-chunk", 96, 96, K333, (5, 33, 40), "scail_conv4_e0", "scail_conv4_e3", {"conv4_cont": 0}, pad=(0, 1, 1)),
    _c("conv4-224-192", 224, 192, K333, (4, 16, 50), "scail_conv4_e0", "scail_conv4_e3"),                       # 7 slices: the frame-slot ring wraps; 2 n tiles
    _c("conv4-384", 384, 384, K333, (3, 17, 20), "scail_conv4_e0", "scail_conv4_e3"),                           # 12 slices, 4 n tiles
    _c("conv4cn-96-3", 96, 3, K333, (3, 19, 33), "scail_conv4cn_e0"),
    _c("conv4cn-64-16", 64, 16, K333, (3, 19, 33), "scail_conv4cn_e0"),
    _c("conv4n-96-3", 96, 3, K333, (3, 19, 33), "scail_conv4n_e0", None, {"conv4_cont": 0}),
    _c("conv4n-64-16", 64, 16, K333, (3, 19, 33), "scail_conv4n_e0", None, {"conv4_cont": 0}),
    _c("conv4u-192-96-ups", 192, 96, K133, (3, 12, 20), "scail_conv4u_e0", pad=(0, 1, 1), ups=True),
    _c("conv4u-384-192-ups", 384, 192, K133, (4, 17, 23), "scail_conv4u_e0", pad=(0, 1, 1), ups=True),
    _c("conv4u-96", 96, 96, K133, (2, 32, 48), "scail_conv4u_e0", pad=(0, 1, 1)),
    _c("halo-96", 96, 96, K333, (5, 10, 12), HALO0 + "96, 2>", HALO3 + "96, 2>", {"conv4": 0}),
    _c("halo-192-96", 192, 96, K333, (3, 17, 35), HALO0 + "96, 2>", HALO3 + "96, 2>", {"conv4": 0}),
    _c("halo-96-oneframe", 96, 96, K333, (1, 10, 12), HALO0 + "96>", HALO3 + "96>", {"conv4": 0}),
    _c("halo-32-24", 32, 24, K333, (2, 8, 16), HALO0 + "32>", HALO3 + "32>", {"conv4": 0}),
    _c("halo-96-200", 96, 200, K333, (2, 8, 16), HALO0 + "96, 2>", HALO3 + "96, 2>"),                           # a ragged third n tile (8 of 96 channels)
    _c("halo-ups-192-96", 192, 96, K133, (3, 12, 20), HALO0 + "96, 2, 1, true>", None, {"conv4": 0}, pad=(0, 1, 1), ups=True),
    _c("s2-1-32-96", 32, 96, K133, (3, 17, 35), "conv_s2_kernel<1>", None, {"conv_s2": 1}, stride=(1, 2, 2), pad=(0, 0, 0)),
    _c("s2-1-64-384", 64, 384, K133, (2, 16, 16), "conv_s2_kernel<1>", None, {"conv_s2": 1}, stride=(1, 2, 2), pad=(0, 0, 0)),
    _c("s2-2-32-96", 32, 96, K133, (3, 17, 35), "conv_s2_kernel<2>", None, {"conv_s2": 2}, stride=(1, 2, 2), pad=(0, 0, 0)),
    _c("s2-2-64-384", 64, 384, K133, (2, 16, 16), "conv_s2_kernel<2>", None, {"conv_s2": 2}, stride=(1, 2, 2), pad=(0, 0, 0)),
    _c("direct-stem", 3, 96, K333, (5, 40, 56), "conv_direct_kernel<14, 3>"),                                    # Cin padded to 8; M = 11 200 >= 4096
    _c("direct-temporal-s2", 32, 96, (3, 1, 1), (9, 31, 40), "conv_direct_kernel<6, 3>", stride=(2, 1, 1), pad=(0, 0, 0)),
    _c("direct-shortcut", 96, 192, K111, (3, 40, 41), "conv_direct_kernel<6, 6>"),
    _c("direct-64-384", 64, 384, K111, (2, 48, 50), "conv_direct_kernel<6, 6> x 2"),
    _c("igemm-16-32", 16, 32, K333, (5, 10, 12), "conv_igemm_kernel<0, 64, 4, 1>", "conv_igemm_kernel<3, 64, 4, 1>"),
    _c("igemm-8-96", 8, 96, K333, (5, 10, 12), "conv_igemm_kernel<0, 96, 4, 1>", "conv_igemm_kernel<3, 96, 4, 1>"),
    _c("igemm-192-384-1x1x1", 192, 384, K111, (5, 10, 12), "conv_igemm_kernel<0, 128, 2, 2>", "conv_igemm_kernel<3, 128, 2, 2>"),
    _c("igemm-40-200", 40, 200, K333, (2, 8, 16), "conv_igemm_kernel<0, 128, 2, 2>", "conv_igemm_kernel<3, 128, 2, 2>"),   # ragged second n tile (72 of 128)
]

# scail_conv3d_cl_norm (form 1): conv -> RMS_norm -> SiLU in one kernel
NORM_CASES = [
    _c("norm-conv4c_e4", 96, 96, K333, (5, 33, 40), "scail_conv4c_e4"),
    _c("norm-conv4f_e4", 96, 96, K333, (5, 33, 40), "scail_conv4f_e4", None, {"conv4_cont": 0}),
    _c("norm-halo-96", 96, 96, K333, (5, 33, 40), HALO4 + "96, 2>", None, {"conv4": 0}),
    _c("norm-halo-32", 32, 32, K333, (4, 9, 17), HALO4 + "32>", None, {"conv4": 0}),
    _c("norm-halo-oneframe", 96, 96, K333, (1, 10, 12), HALO4 + "96>", None, {"conv4": 0}),
]

# scail_conv3d_cl_resid_norm (form 2 with the raw output, 3 without): `plain` is the name for the form the case runs
RESID_NORM_CASES = [
    _c("rn-conv4c_e5", 96, 96, K333, (5, 48, 80), "scail_conv4c_e5", want_raw=True, with_resid=True),
    _c("rn-conv4c_e6", 96, 96, K333, (3, 50, 70), "scail_conv4c_e6", want_raw=False, with_resid=True),
    _c("rn-conv4u_e7", 192, 96, K133, (3, 24, 40), "scail_conv4u_e7", pad=(0, 1, 1), ups=True, want_raw=True, with_resid=False),
    _c("rn-direct-stem", 3, 96, K333, (5, 40, 56), "conv_direct_kernel<14, 3, true>", want_raw=True, with_resid=False),
    _c("rn-two-calls", 96, 96, K333, (5, 48, 80), "scail_conv4c_e3 + scail_rms_silu", None, {"conv4_resnorm": 0}, want_raw=True, with_resid=True),
]

RMS_SILU_CHANNELS = (32, 96, 192, 384)
RMS_SILU_ROWS = 77                           # an odd count: the last voxel group of rms_silu_kernel (two voxels per lane group) is ragged

KERNELS = ["conv_halo_kernel", "conv_s2_kernel<1>", "conv_s2_kernel<2>", "conv_direct_kernel", "conv_igemm_kernel",
           "scail_conv4_e0", "scail_conv4_e3", "scail_conv4c_e0", "scail_conv4c_e3", "scail_conv4c_e4", "scail_conv4c_e5", "scail_conv4c_e6",
           "scail_conv4f_e4", "scail_conv4u_e0", "scail_conv4u_e7", "scail_conv4n_e0", "scail_conv4cn_e0"]      # five hipcc templates (both s2 forms) + eleven generated


def seed_of(case):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case["id"])) % 100003


def out_thw(case):
    """(To, Ho, Wo) of a case, from its geometry"""
    T, H, W = case["thw"]
    k = case["k"] if len(case["k"]) == 3 else (1,) + tuple(case["k"])
    pad = case["pad"] if case["pad"] is not None else (k[0] - 1, k[1] // 2, k[2] // 2)
    st = case["stride"]
    if case["ups"]:
        H, W = 2 * H, 2 * W
    To = (T + pad[0] - k[0]) // st[0] + 1
    if st[1] == 2:
        return To, (H + 1 - k[1]) // 2 + 1, (W + 1 - k[2]) // 2 + 1
    return To, H + 2 * pad[1] - k[1] + 1, W + 2 * pad[2] - k[2] + 1


@functools.lru_cache(maxsize=None)
def _operands(id):
    case = next(c for c in PLAIN_CASES + NORM_CASES + RESID_NORM_CASES if c["id"] == id)
    return exact_operands(case["cin"], case["cout"], case["k"], case["thw"], seed_of(case), out_thw=out_thw(case))


def operands(case):
    """the case's operands: computed once, shared, never modified"""
    return _operands(case["id"])


@functools.lru_cache(maxsize=None)
def _norm_reference(id):
    case = next(c for c in NORM_CASES + RESID_NORM_CASES if c["id"] == id)
    o = operands(case)
    s = conv_ref(o["x"], o["w"], o["bias"], o["resid"] if case.get("with_resid") else None, case["stride"], case["pad"], case["ups"])
    return s, norm_silu_ref(s, o["gamma"])


def norm_reference(case):
    """(the bf16-rounded sum, fp64 SiLU(RMS_norm(it) gamma)) of a norm case: computed once, shared, never modified"""
    return _norm_reference(case["id"])


def geometry(case, N, Kpad, cin_pad, ot_mul=1, ot_off=0):
    """the 21 int32 of scail_conv3d_cl's geometry argument"""
    import ctypes as C
    T, H, W = case["thw"]
    To, Ho, Wo = out_thw(case)
    k = case["k"] if len(case["k"]) == 3 else (1,) + tuple(case["k"])
    pad = case["pad"] if case["pad"] is not None else (k[0] - 1, k[1] // 2, k[2] // 2)
    return (C.c_int32 * 21)(T, H, W, cin_pad, To, Ho, Wo, *k, *case["stride"], *pad, 1 if case["ups"] else 0, ot_mul, ot_off, N, Kpad)


def kernel_name(case, form, ldc, ldr, ot_mul=1, ot_off=0):
    """what scail_conv3d_kernel_name_for says the case runs under the options in force"""
    import ctypes as C
    from scail_amd import lib as L
    cin_pad, N = (case["cin"] + 7) // 8 * 8, (case["cout"] + 7) // 8 * 8
    k = case["k"] if len(case["k"]) == 3 else (1,) + tuple(case["k"])
    Kpad = (k[0] * k[1] * k[2] * cin_pad + 63) // 64 * 64
    buf = C.create_string_buffer(128)
    L.call("scail_conv3d_kernel_name_for", C.cast(geometry(case, N, Kpad, cin_pad, ot_mul, ot_off), C.c_void_p), ldc, ldr, form, buf, len(buf))
    return buf.value.decode()


OPTION_DEFAULTS = {"conv4": 1, "conv4_cont": 1, "conv4_resnorm": 1, "conv_direct": 1, "conv_s2": 1}


def with_options(opts, fn, defaults=OPTION_DEFAULTS):
    """fn() under the library options ``opts``; the defaults (everything on, conv_s2 = 1) are back afterwards, whatever happens"""
    from scail_amd import lib as L
    try:
        for name, v in opts.items():
            L.set_option(name, v)
        return fn()
    finally:
        for name in opts:
            L.set_option(name, defaults[name])
