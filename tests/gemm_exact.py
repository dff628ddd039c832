"""Exact-arithmetic helpers for the bf16 GEMM tests (tests/test_gemm_exact_cpu.py, tests/test_gemm_exact_gpu.py); the rounding helpers and
assert_bits come from tests/conv_exact.py.

Operands.  x = ix / 4 and w = iw / 8 * 2^-s with integers |ix|, |iw| <= A (A = 31 for K <= 320, 7 above: at most 5 + 5 significant bits), bias =
integers in [-8, 8] (GELU cases: / 8), residual = integers in [-64, 64], gate = (integers in [-4, 4]) / 2: x, w and the residual are exact in bf16, bias
and gate in fp32.  In units of 2^-(5+s) every product is an integer of magnitude <= A^2, so a dot product of K terms stays below A^2 K <= 677 376
units (K = 13 824, A = 7) and, with the bias (<= 8 x 2^(5+s) units), below V units; the gated residual epilogue r + g v is, in HALF units, an integer
below 4 V + 64 x 2^(6+s).  exact_operands asserts 4 V + 64 x 2^(6+s) < 2^24: EVERY fp32 partial sum is exact, in any order and for any MFMA shape, and so
are acc + bias, g * v, r + g * v and fma(g, v, r).  A kernel therefore has to reproduce exact_ref -- the fp64 value rounded ONCE to bf16 -- bit for
bit.  s is chosen per case so that the pre-activation v = x . w + bias has a standard deviation of about 8 (exact epilogues: the sums carry 11 to 14
significant bits against the 8 of bf16, and are of the size of the bias and the residual) or about 1 (GELU).  Row 0 of w is structured and asymmetric
(k mod 13 - 6); the "identity" operands (x = 7/4 where k == m mod K, else 0) make y[m, n] = 7/4 w[n, m mod K], which a transposed result cannot match.

GELU epilogues.  GELU of the exact v is not exact in fp32, so the kernels are held to "correctly rounded wherever fp32 arithmetic can decide it":
check_budget_bf16 wants round_bf16(ref - B(v)) <= y <= round_bf16(ref + B(v)) in value order; where the two ends coincide the element is decided and
must be that value, and the share of elements where they differ is the undecided share (a condition on the INPUTS, at most UNDECIDED_CAP = 5 % per
case, asserted on the CPU for the reference alone).

B(v), first-order absolute error bounds in units of u = 2^-24 (one fp32 rounding is <= u relative).  Instruction accuracies: the kernel guides this
project follows give none, so the figures are the ISA manual's -- v_exp_f32 and v_rcp_f32 1 ulp = 2 u; the division 2.0f / (e + 1.0f) of common.h is
IEEE-correct (u): scail_amd/build.py compiles with -O3 only, no -ffast-math and nothing that switches hipcc's default correctly rounded fp32 division
off; erff: no accuracy statement for the ROCm device library exists in the installed ROCm documentation, so the OpenCL bound of 16 ulp = 32 u is
used.  A rounded constant costs u.  Contraction of a * b + c into an fma only removes a rounding.
With U = k0 (v + k1 v^3), s = sigmoid(2 U) = (1 + tanh U) / 2, ref = v s:
  gelu_tanh_f (csrc/common.h): k1 v v v: constant + 3 products = 4 u; v + .: 1 more on a sum of equal signs = 5 u; k0 .: constant + product = 7 u;
      * 2 log2(e): 9 u on the argument of exp2, i.e. 2 |U| 9 u = 18 |U| u on e = exp(2 U), + v_exp 2 u;  e + 1: u + s (2 + 18 |U|) u;  2 / .: + u;
      q = 2 (1 - s) thus carries q (2 + s (2 + 18 |U|)) u ABSOLUTE, which t = 1 - q (u |t|, t = 2 s - 1) and g = 1 + t (u g, g = 2 s) inherit unchanged:
      for v < 0, g is small and the error of q is not -- the cancellation that makes the budget absolute and a function of v.  0.5 v is exact, the
      last product costs u |ref|:      |v| (1 - s) (2 + s (2 + 18 |U|)) + 0.5 |v| (2 s + |2 s - 1|) + |ref|.
  the e1 epilogue of asmgen/gemm4.py: v - v / (exp2(((k0 k1 c) v^2 + k0 c) v) + 1), c = 2 log2(e): v^2 u, two constants and the fma 3 u, * v: 4 u on
      the argument, 8 |U| u on e, + v_exp 2 u;  1 + e: u + s (2 + 8 |U|) u;  v_rcp: + 2 u;  the final fma rounds once:
      |v| (1 - s) (3 + s (2 + 8 |U|)) + |ref|.
  Both are covered by  TANH_FIRST(v) = |v| (1 - s) (3 + s (2 + 18 |U|)) + 0.5 |v| (2 s + |2 s - 1|) + |ref|.
  gelu_erf_f: z = v / sqrt 2 (constant + product, 2 u), E = erff(z): 32 u |E| + erf'(z) |z| 2 u = (4 / sqrt pi) |z| exp(-z^2) u;  g = 1 + E: + u g, again
      absolute and large against g for v < 0;  0.5 v g: + u |ref|:      ERF_FIRST(v) = 0.5 |v| (g + 32 |E| + (4 / sqrt pi) |z| exp(-z^2)) + |ref|.
B = SLACK x FIRST x u with SLACK = 2 for the second-order terms; V_ABS_MAX = 8 bounds |v| (a condition on the inputs, asserted on the CPU), so that
they stay far below the first-order ones and exp2 stays far from its flush-to-zero range.  Sizes: at v = 1 B is 9.5 (tanh) / 26 (erf) u on a
reference of 0.84, at v = -2 it is 17 / 62 u on -0.045, at v = -4 28 / 128 u on -7e-5 / -1.3e-4; the undecided share of the cases below, v ~ N(0, 1.1
to 1.4) + bias, is 0.1 to 1.3 % (tanh) and 0.3 to 2.6 % (erf).

The module reads nothing outside tests/ and scail_amd/."""
import functools
import math

import torch

import conv_exact
from conv_exact import BF16, U, _is_bf16, assert_bits, bf16_neighbours, round_bf16, seed_of      # noqa: F401  (re-exported for the two test files)

EPI_BIAS, EPI_GELU_TANH, EPI_GELU_ERF, EPI_RESID = 0, 1, 2, 3
SLACK = 2.0
V_ABS_MAX = 8.0
UNDECIDED_CAP = 0.05
K0, K1 = math.sqrt(2.0 / math.pi), 0.044715
EXACT_FORMS = ("bias", "nobias", "resid_alias", "resid_sep", "gated")
GELU_FORMS = ("gelu_tanh", "gelu_erf")
FORMS = ("bias", "nobias", "gelu_tanh", "gelu_erf", "resid_alias", "resid_sep", "gated")
EPI_OF = {"bias": EPI_BIAS, "nobias": EPI_BIAS, "gelu_tanh": EPI_GELU_TANH, "gelu_erf": EPI_GELU_ERF, "resid_alias": EPI_RESID, "resid_sep": EPI_RESID,
          "gated": EPI_RESID}


# ---- operands -----------------------------------------------------------------------------------------------------------------
def grid_of(K):
    return 31 if K <= 320 else 7


def scale_of(K, gelu):
    """s of w = iw / 8 * 2^-s: the sum of K products of two uniform integers in [-A, A] has a standard deviation of A (A + 1) / 3 sqrt(K) units of
    2^-(5+s); s brings it to about 8 (exact epilogues) or 1 (GELU)"""
    A = grid_of(K)
    return round(math.log2(A * (A + 1) / 3.0 * math.sqrt(K) / (1.0 if gelu else 8.0))) - 5


def rows_per_batch(M):
    """a gate batch length that is no multiple of 32 (so of no tile) and gives at least 3 batches"""
    rpb = (M + 2) // 3
    return rpb if rpb % 32 else rpb - 1


def exact_operands(M, N, K, seed, gelu=False, kind="random"):
    """x (M, K), w (N, K), bias (N), resid (M, N), gate table (B, 6 N) of which columns [2 N, 3 N) are the gate, rpb, s: fp32 tensors on the CPU (module
    docstring)"""
    g = torch.Generator().manual_seed(seed)
    A, s = grid_of(K), scale_of(K, gelu)
    if kind == "identity":
        ix = torch.zeros(M, K)
        ix[torch.arange(M), torch.arange(M) % K] = 7.0
    else:
        ix = torch.randint(-A, A + 1, (M, K), generator=g).float()
    iw = torch.randint(-A, A + 1, (N, K), generator=g).float()
    iw[0] = torch.arange(K).remainder(13).float() - 6                       # a structured, non-symmetric row
    x, w = ix * 0.25, iw * 0.125 * 2.0 ** -s
    bias = torch.randint(-8, 9, (N,), generator=g).float() * (0.125 if gelu else 1.0)
    resid = torch.randint(-64, 65, (M, N), generator=g).float()
    rpb = rows_per_batch(M)
    nb = (M + rpb - 1) // rpb
    table = torch.randint(-4, 5, (nb, 6 * N), generator=g).float() * 0.5
    assert all(_is_bf16(t) for t in (x, w, resid)) and nb >= 3 and rpb % 32 != 0
    bias_units = 8 * 2.0 ** (5 + s) * (0.125 if gelu else 1.0)
    assert bias_units == int(bias_units) and bias_units >= 1, "the bias is a whole number of product units"
    V = A * A * K + bias_units
    assert 4 * V + 64 * 2.0 ** (6 + s) < 2 ** 24, "exactness bound: every fp32 partial sum, and r + g v, is an integer below 2^24 in (half) units of 2^-(5+s)"
    return dict(x=x, w=w, bias=bias, resid=resid, table=table, gate=table[:, 2 * N:3 * N], rpb=rpb, s=s)


# ---- references ---------------------------------------------------------------------------------------------------------------
def dot64(x, w):
    return x.double() @ w.double().t()


def gate_rows(o, M):
    """the gate row of every output row, fp64 (M, N)"""
    return o["gate"].double()[torch.arange(M) // o["rpb"]]


def value64(acc64, o, form):
    """the exact value of an exact epilogue, or the pre-activation v of a GELU one, in fp64, from acc64 = dot64(x, w)"""
    v = acc64 if form == "nobias" else acc64 + o["bias"].double()
    if form in ("resid_alias", "resid_sep"):
        return o["resid"].double() + v
    if form == "gated":
        return o["resid"].double() + gate_rows(o, acc64.shape[0]) * v
    return v


def gelu_tanh64(v):
    return v / (1 + torch.exp(-2 * K0 * (v + K1 * v ** 3)))                # 0.5 v (1 + tanh U) = v sigmoid(2 U), without the cancellation


def gelu_erf64(v):
    return 0.5 * v * torch.special.erfc(-v / math.sqrt(2.0))               # 1 + erf(z) = erfc(-z)


def budget_tanh(v):
    Uv = K0 * (v + K1 * v ** 3)
    s = torch.sigmoid(2 * Uv)
    a = v.abs()
    first = a * (1 - s) * (3 + s * (2 + 18 * Uv.abs())) + 0.5 * a * (2 * s + (2 * s - 1).abs()) + (v * s).abs()
    return SLACK * first * U


def budget_erf(v):
    z = v / math.sqrt(2.0)
    g = torch.special.erfc(-z)
    first = 0.5 * v.abs() * (g + 32 * torch.erf(z).abs() + 4 / math.sqrt(math.pi) * z.abs() * torch.exp(-z * z)) + (0.5 * v * g).abs()
    return SLACK * first * U


GELU64 = {"gelu_tanh": gelu_tanh64, "gelu_erf": gelu_erf64}
BUDGET = {"gelu_tanh": budget_tanh, "gelu_erf": budget_erf}


# the kernels' chains restated with IEEE fp32 operations (torch on the CPU)
def _f(c):
    return torch.tensor(c, dtype=torch.float32)


def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def gelu_tanh_hip_fp32(v, k0=None):
    """gelu_tanh_f of csrc/common.h (k0: another constant in place of the correctly rounded sqrt(2 / pi), for the tests of the checker)"""
    x = v.float()
    u = _f(0.7978845608028654 if k0 is None else k0) * (x + _f(0.044715) * x * x * x)
    e = torch.exp2(u * _f(2.8853900817779268))
    t = 1.0 - 2.0 / (e + 1.0)
    return 0.5 * x * (1.0 + t)


def gelu_tanh_e1_fp32(v):
    """the e1 epilogue of scail_amd/asmgen/gemm4.py"""
    x = v.float()
    sc = 2.0 * 1.4426950408889634
    u = _fma32(x * x, _f(0.7978845608028654 * 0.044715 * sc), _f(0.7978845608028654 * sc)) * x
    r = 1.0 / (1.0 + torch.exp2(u))
    return _fma32(-x, r, x)


def gelu_erf_fp32(v, c=None):
    """gelu_erf_f of csrc/common.h"""
    x = v.float()
    return 0.5 * x * (1.0 + torch.erf(x * _f(0.7071067811865476 if c is None else c)))


# ---- checkers -----------------------------------------------------------------------------------------------------------------
_DROP = 45                                     # fp64 keeps 52 fraction bits, bf16 7
_MAG = 0x7FFFFFFFFFFFFFFF


def _round_bits(v64, add_half, tie_even):
    v64 = v64.contiguous()
    mag = v64.view(torch.int64) & _MAG
    # (the bit arithmetic is right for zero and for normal bf16 magnitudes; the references here are zero or far above 2^-120)
    assert bool(((mag == 0) | (mag >= (1023 - 120) << 52)).all()), "magnitude below the range the bit rounding covers"
    if add_half:
        mag = mag + (((1 << (_DROP - 1)) - 1 + ((mag >> _DROP) & 1)) if tie_even else (1 << (_DROP - 1)))
    r = ((mag >> _DROP) << _DROP).view(torch.float64)
    return torch.where(v64 < 0, -r, r)


def rne_bf16(v64):
    """fp64 -> the nearest bf16 VALUE (as fp64), ties to even, in ONE rounding (round_bf16 goes through fp32: right for the exact sums only)"""
    return _round_bits(v64, True, True)


def truncate_bf16(v64):
    return _round_bits(v64, False, False)


def away_bf16(v64):
    """nearest, ties AWAY from zero"""
    return _round_bits(v64, True, False)


def rne_bf16_slow(v64):
    """rne_bf16 stated with the neighbour arithmetic of conv_exact.py (the CPU tests hold the two against each other)"""
    lo, hi, ulp = bf16_neighbours(v64)
    a = v64.abs()
    dl, dh = a - lo.abs(), hi.abs() - a
    lo_even = torch.remainder(torch.round(lo.abs() / ulp), 2) == 0
    return torch.where((dl < dh) | ((dl == dh) & lo_even), lo, hi)


def even_away_ties(v64):
    """the number of exact ties whose even and away roundings differ"""
    return int((rne_bf16(v64) != away_bf16(v64)).sum())


def check_budget_bf16(got, ref64, budget64, what=""):
    """got (bf16) against the fp64 reference and its absolute error budget: rne(ref - B) <= got <= rne(ref + B) everywhere.  Returns the share of
    elements whose two ends differ (undecided); prints it, the number of elements that are not RNE(ref) but allowed, and the number of DECIDED
    elements that are not RNE(ref), which raises AssertionError like any element outside its interval."""
    assert got.dtype == BF16 and got.shape == ref64.shape == budget64.shape and ref64.dtype == torch.float64
    g = got.double().cpu()
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite output"
    lo, hi = rne_bf16(ref64 - budget64), rne_bf16(ref64 + budget64)
    undecided = lo != hi
    inside = (g >= lo) & (g <= hi)
    share = float(undecided.double().mean())
    off = int(((g != rne_bf16(ref64)) & inside).sum())
    decided_wrong = ~inside & ~undecided
    print(f"{what}: undecided share {share:.4%}, decided but not RNE {int(decided_wrong.sum())}, not RNE but allowed {off} of {g.numel()}")
    if bool(decided_wrong.any()):
        i = int(decided_wrong.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(decided_wrong.sum())} elements are not the correctly rounded value although fp32 arithmetic decides it; "
                             f"first at {i}: got {float(g.flatten()[i])!r}, ref {float(ref64.flatten()[i])!r}")
    if not bool(inside.all()):
        i = int((~inside).flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int((~inside).sum())} elements are outside [rne(ref - B), rne(ref + B)]; first at {i}: got {float(g.flatten()[i])!r}, "
                             f"ref {float(ref64.flatten()[i])!r}, B {float(budget64.flatten()[i])!r}")
    return share


# ---- the cases of tests/test_gemm_exact_gpu.py (the CPU file checks the conditions on their inputs and the route table) ----------------------
T128, T256, T256_DMA, Q8 = "gemm_bf16_kernel<128, 128, 2, 2, {e}, false>", "gemm_bf16_kernel<256, 256, 2, 4, {e}, false>", "gemm_bf16_kernel<256, 256, 2, 4, {e}, true>", "gemm_bf16_q8_kernel<{e}>"
GEN = "scail_gemm4_e{g}"
FORCED = {256: T256, 257: T256_DMA, 260: "gemm_bf16_kernel<256, 256, 2, 4, {e}, true, 4>", 261: Q8, 262: "gemm_bf16_q8_kernel<{e}, 32>"}
KERNELS = ["gemm_bf16_kernel<128, 128, 2, 2, ", "gemm_bf16_q8_kernel<", "scail_gemm4_e0", "scail_gemm4_e1", "scail_gemm4_e3", "scail_gemm4_e4"]


def _c(id, M, N, K, route, forms=FORMS, erf_route=None, opts=None, kind="random"):
    """route: the kernel of every form but GELU-erf, erf_route: GELU-erf's (the generated kernels have none)"""
    return dict(id=id, M=M, N=N, K=K, route=route, erf_route=erf_route or route, forms=tuple(forms), opts=opts or {}, kind=kind)


CASES = [
    # the 128 tile: one ragged tile, N % 32 != 0, 1 / 3 / 216 k-tiles; 3 x 2 tiles with ragged edges, 2 k-tiles
    _c("t128-77x72x64", 77, 72, 64, T128), _c("t128-77x72x192", 77, 72, 192, T128), _c("t128-77x72x13824", 77, 72, 13824, T128),
    _c("t128-300x136x128", 300, 136, 128, T128), _c("t128-identity", 300, 136, 128, T128, ("bias",), kind="identity"),
    # q8: a 3-row tail (clamped rows), a ragged fifth n-tile, 45 tiles (the XCD remainder and the last group of 4 m-tiles are partial); 1, 2 and >= 3 k-tiles
    _c("q8-2051x1032x64", 2051, 1032, 64, Q8), _c("q8-2051x1032x128", 2051, 1032, 128, Q8), _c("q8-2051x1032x320", 2051, 1032, 320, Q8),
    _c("q8-identity", 2051, 1032, 128, Q8, ("bias",), kind="identity"),
    _c("q8-erf-2048x1024", 2048, 1024, 128, Q8, ("gelu_erf",)),                                                  # every other form of this shape is a generated kernel's
    _c("q8-gemm4-off", 2048, 1024, 192, Q8, [f for f in FORMS if f != "gelu_erf"], opts={"gemm4": 0}),              # ... which option "gemm4" = 0 sends to q8
    # generated: an 8-row tail, 1 and 2 n-tiles, 2 / 3 / 216 k-tiles; GELU-erf at these shapes is the 128 tile's (N < 1024)
    _c("gen-2056x256x128", 2056, 256, 128, GEN, erf_route=T128), _c("gen-2056x256x192", 2056, 256, 192, GEN, erf_route=T128),
    _c("gen-2056x256x13824", 2056, 256, 13824, GEN, erf_route=T128), _c("gen-2056x512x128", 2056, 512, 128, GEN, erf_route=T128),
    _c("gen-2056x512x192", 2056, 512, 192, GEN, erf_route=T128), _c("gen-2056x512x13824", 2056, 512, 13824, GEN, erf_route=T128),
    _c("gen-identity", 2056, 256, 128, GEN, ("bias",), erf_route=T128, kind="identity"),
    _c("gen-small-m-512x16384", 512, 16384, 128, GEN, erf_route=T128),                                           # 512 <= M < 2048 with 128 tiles
]
CASE_FORMS = [(c["id"], f) for c in CASES for f in c["forms"]]


def case_of(id):
    return next(c for c in CASES if c["id"] == id)


def expected_name(case, form, tile=0):
    """the name scail_gemm_kernel_name_for must give: by shape, or under a forced tile of the measurement build"""
    e = EPI_OF[form]
    if tile:
        return f"gemm_tile {tile}: " + FORCED[tile].format(e=e)
    return (case["erf_route"] if form == "gelu_erf" else case["route"]).format(e=e, g={"resid_alias": 4, "resid_sep": 4, "gated": 3}.get(form, e))


def other_route(case, form):
    """(options, kernel name) of the second route that accepts the case, or None: option "gemm4" = 0 sends a generated kernel's shape to a hipcc kernel
    (the one GELU-erf runs at that shape), and the case that runs under that option is a generated kernel's without it"""
    if form == "gelu_erf" or not (case["route"] == GEN or case["opts"]):
        return None
    if case["opts"]:
        return {}, expected_name(dict(case, route=GEN), form)
    return {"gemm4": 0}, case["erf_route"].format(e=EPI_OF[form])


@functools.lru_cache(maxsize=2)
def _operands(id, gelu):
    c = case_of(id)
    return exact_operands(c["M"], c["N"], c["K"], seed_of(c) + (1 if gelu else 0), gelu, c["kind"])


def operands(case, form):
    """the operands of a case -- one set for its exact forms, one (v of O(1)) for its GELU forms: computed once, shared, never modified"""
    return _operands(case["id"], form in GELU_FORMS)


@functools.lru_cache(maxsize=2)
def _acc(id, gelu):
    o = _operands(id, gelu)
    return dot64(o["x"], o["w"])


def reference(case, form):
    """(fp64 reference, budget): the exact value and None for an exact form -- the kernel must give round_bf16(reference) --, GELU(v) and B(v) else"""
    o = operands(case, form)
    v = value64(_acc(case["id"], form in GELU_FORMS), o, form)
    if form in GELU_FORMS:
        return GELU64[form](v), BUDGET[form](v)
    return v, None


def pre_activation(case, form):
    return value64(_acc(case["id"], True), operands(case, form), form)


def kernel_name(lda, ldc, ldr, M, N, K, epilogue, gated):
    """what scail_gemm_kernel_name_for says the call runs under the options in force; scail_gemm_kernel_for must agree"""
    import ctypes as C
    from scail_amd import lib as L
    buf = C.create_string_buffer(128)
    L.call("scail_gemm_kernel_name_for", lda, ldc, ldr, M, N, K, epilogue, 1 if gated else 0, buf, len(buf))
    name = buf.value.decode()
    assert L.load().scail_gemm_kernel_for(lda, ldc, ldr, M, N, K, epilogue) == (4 if name.startswith("scail_gemm4_e") else 0), name
    return name


OPTION_DEFAULTS = {"gemm4": 1}


def with_options(opts, fn):
    """fn() under the library options ``opts``; the defaults are back afterwards, whatever happens"""
    return conv_exact.with_options(opts, fn, OPTION_DEFAULTS)
