"""Exact-arithmetic helpers for the row kernels of csrc/rowops.hip (tests/test_row_exact_cpu.py, tests/test_row_exact_gpu.py): LayerNorm + modulate,
affine LayerNorm, RMSNorm (+ interleaved RoPE, + out_scale), and the small kernels next to them (scail_small_linear, scail_mul_bf16, scail_row_affine).

References are fp64 functions of the bf16 inputs and the fp32 parameters AS THE KERNEL RECEIVES THEM, rounded once to bf16:
  LayerNorm   ((x - mean) / sqrt(var + eps)) (1 + scale) + shift   |   ... w + b      (population variance, eps the fp32 value)
  RMSNorm     n = w x / sqrt(mean(x^2) + eps)
  RoPE        o[2i] = n[2i] c - n[2i+1] s,  o[2i+1] = n[2i+1] c + n[2i] s,  (c, s) = tables[r % rows_per_batch, i];  then * out_scale.
A kernel is held to "the round-to-nearest-even bf16 of SOME real number in [ref - m, ref + m]" (check_margin_bf16), m a per-element ABSOLUTE margin that
is a function of reference quantities only.  Where m is below the bf16 spacing this is conv_exact.check_rounded_bf16's rule: a neighbour of the
reference, and the RNE one wherever the reference is farther than m from the rounding boundary.  The margin has to be absolute because the mean
subtraction and the RoPE sum cancel: their error scales with rstd |d mean| and |n0 c| + |n1 s|, not with |ref|.

The margin, first-order, in units of u = 2^-24 (one fp32 rounding is a relative error <= u), from the operation chains of csrc/rowops.hip.
  Sums.  A term takes part in at most A additions: block kernels (ln_kernel, rmsnorm_rope_kernel) 8 x 3 serial + 6 butterfly steps + 3 = 33, wave
      kernels 8 x CPL serial + 6 butterfly, CPL = D / 512 (30 .. 102).  |dS| <= A u sum|x|; for a sum of non-negative terms that is A u relative.
  LayerNorm.  mean = S / D is one rounding, S * (1 / D) (wave form) two: |d mean| <= Em = (A mean|x| + 2 |mean|) u.   d_i = x_i - mean carries Em and its
      own rounding u |d_i|.   q = sum d_i^2: the common part of the error drops out at first order (sum d_i = 0), the own roundings give 2 u, each
      square 1 u, the sum A u, / D again <= 2 u: (A + 5) u relative on var -- plus the SECOND-order dmean^2 that the kernel's variance really
      contains (var^ = var + dmean^2): it is kept, as Em^2 / (var + eps), because on a constant row it is all there is.   t = var + eps: the inherited
      (A + 5) rho u with rho = var / (var + eps), + 1 u.   rsqrtf is held to v_rsq_f32's documented 1 ulp = 2 u and halves its argument's error:
          R = ((A + 5) rho + 1) / 2 + 2 + Em^2 / (2 u (var + eps))          [u, relative, on rstd]
      o = (d rstd) M + a with M = 1.0f + scale (rounded: 1 u) or w (exact): d rstd 1 u, (.) M 1 u  =>  (R + 4) u relative on the product for the
      modulate form, (R + 3) u for the affine form, + |M| rstd Em from the mean, + u |ref| for the last addition:
          m_LN = |M| rstd (Em + |d| (R + 4) u) + u |ref|                      (R + 4 is used for both forms)
  RMSNorm.  x^2 is exact in fp32 (8-bit significands), q = sum x^2 has A u relative, / D <= 2 u, + eps 1 u, rsqrt as above:
          R = ((A + 2) rho + 1) / 2 + 2,  rho = ms / (ms + eps)
      n = w (x rstd): two multiplications, (R + 2) u.  Without RoPE: * out_scale 1 u  =>  m = (R + 3) u |ref|.  With RoPE every product is rounded (1 u on
      top of n's R + 2), the sum is rounded (u |o|) and so is * out_scale (u |ref|):
          m_RoPE = |out_scale| (R + 3) u (|n0 c| + |n1 s|) + 2 u |ref|
  Three multiplications at most lie on any chain.  build.py passes no -ffp-contract, so hipcc may or may not contract a * b + c into an fma: an fma
  only removes one of the roundings counted above, the margin holds either way.
  SLACK = 1.125 on top: it covers the second-order terms (the largest relative first-order term is about 110 u = 7e-6, so they are below 1e-5 of the
  margin) and the fp64 reference's own error; it is not a worst-case allowance -- every term above is already a worst-case bound, not a typical size.
Sizes: for rows of 2 randn + 0.5 the margin is about 50 u (block) to 130 u (wave, D = 6144) on values of order 1, 3e-6 to 8e-6 absolute, against a
bf16 spacing of 2^-8 |ref| or more: 0.05 to 1.2 % of the elements have a rounding boundary inside their interval.  UNDECIDED_CAP = 3 % over the regular
rows of a case is a condition on the inputs, not a tolerance on a kernel; the special rows (zero, constant, one-hot, 2^10, 2^-10) are checked by the
same rule, counted apart and carry no cap -- on a constant row d = 0 and the margin, |M| rstd Em with rstd = eps^-1/2, can exceed a bf16 step.

scail_small_linear (one wave per output column, lane l holds the 8-element chunks l, l + 64, ..): a term takes part in A_sl = 8 ceil(K / 512) + 6
additions, + 1 for the bias.  With integer operands below 2^24 every partial sum is exact and the fp32 output IS the fp64 sum.  With activations:
  silu_f(x) = x / (1 + __expf(-x)): the argument of exp2 carries the rounded constant and the product (2 u, i.e. 2 |x| u on e), v_exp_f32 1 ulp = 2 u;
      1 + e: u + sigmoid(-x) (2 + 2 |x|) u; the division is IEEE (u):  b_silu(x) = (2 + sigmoid(-x) (2 + 2 |x|)) u |silu(x)|;
  gelu_tanh_f: gemm_exact.budget_tanh, the same chain (it carries that module's SLACK = 2 already; b_silu gets the same factor 2);
  act on the input: sum |w_i| b(x_i) from the activations, + (A_sl + 2) u (sum |act(x_i) w_i| + |bias|) for the products, the sum and the bias;
  act on the output: 1.2 x the error of its argument (|silu'|, |gelu'| <= 1.13) + b(v).  |x|, |v| <= 8 as in gemm_exact (asserted).
scail_mul_bf16: a product of two bf16 values is exact in fp32: the output is the fp64 product rounded once, bit for bit.
scail_row_affine: x s + a is two fp32 roundings, one under contraction: m = u |x s| + u |ref|.

The module reads nothing outside tests/ and scail_amd/."""
import functools
import math

import torch

from conv_exact import BF16, U, assert_bits, seed_of          # noqa: F401  (re-exported for the two test files)
from gemm_exact import rne_bf16, truncate_bf16                # noqa: F401

SLACK = 1.125
UNDECIDED_CAP = 0.03
EPS = 1e-6
NOMINAL_CUS = 256                      # the CPU file builds the CU-dependent cases for this count (an MI355X has 256)
ATTN_LOG2_SCALE = 1.4426950408889634 / math.sqrt(128.0)
N_SPECIAL = 6
SPECIAL = ("zero", "constant", "one-hot", "2^10", "2^-10 a", "2^-10 b")
F64, F32 = torch.float64, torch.float32


def f32(v):
    """the fp32 value of a Python float, as fp64 (what a kernel receives for eps / out_scale)"""
    return float(torch.tensor(v, dtype=F32))


def depth(kind, D):
    """additions a term of a row sum takes part in, at most (module docstring)"""
    return 8 * 3 + 6 + 3 if kind == "block" else 8 * ((D + 511) // 512) + 6          # (the restatement runs the wave order at any D)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def special_rows(D, g):
    """the six special rows: zero, constant, one-hot, magnitude 2^10, and two of magnitude 2^-10 whose variance (1e-6, 2.5e-7) is comparable to eps"""
    s = torch.zeros(N_SPECIAL, D)
    s[1] = 1.5
    s[2, D // 3] = 3.0
    s[3] = (2.0 * torch.randn(D, generator=g) + 0.5) * 1024.0
    s[4] = torch.randn(D, generator=g) * 2.0 ** -10
    s[5] = (torch.randn(D, generator=g) + 0.5) * 2.0 ** -11
    return s.to(BF16)


def regular_rows(rows, D, g):
    return (2.0 * torch.randn(rows, D, generator=g) + 0.5).to(BF16)


def rope_tables(n, half, g):
    """n x half DISTINCT angles, uniform over the full circle: the golden-ratio sequence from a random start, so that two angles are at least
    2 pi / (sqrt(5) n half) apart and stay distinct as fp32 (cos, sin) pairs.  cos and sin in fp64, rounded to fp32.  Token 0 is not special."""
    k = torch.arange(n * half, dtype=F64).reshape(n, half)
    ang = torch.frac(float(torch.rand(1, generator=g, dtype=F64)) + k * ((math.sqrt(5.0) - 1) / 2)) * (2 * math.pi)
    return torch.cos(ang).float(), torch.sin(ang).float()


# ---- references and margins ---------------------------------------------------------------------------------------------------
def ln_reference(X, mult, add, eps, A):
    """X (rows, D) bf16; mult, add (rows, D) or (D,) fp64 -- 1 + scale | w, and shift | b; eps the fp32 value.  -> (ref, margin), fp64"""
    x = X.double()
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    ref = d * rstd * mult + add
    Em = (A * x.abs().mean(-1, keepdim=True) + 2 * mean.abs()) * U
    R = ((A + 5) * var / (var + eps) + 1) / 2 + 2 + Em * Em / (2 * U * (var + eps))
    m = mult.abs() * rstd * (Em + d.abs() * (R + 4) * U) + U * ref.abs()
    return ref, SLACK * m


def rope_pairs(D, hd):
    """pair index inside the head of every even column"""
    return (torch.arange(0, D, 2) % hd) // 2


def rms_reference(X, w, eps, A, cos=None, sin=None, tok=None, hd=128, out_scale=1.0):
    """X (rows, D) bf16, w (D,) fp32, cos / sin (n, hd / 2) fp32 with tok (rows,) the table row of every row; out_scale the fp32 value.  -> (ref, margin)"""
    x = X.double()
    ms = (x * x).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(ms + eps)
    R = ((A + 2) * ms / (ms + eps) + 1) / 2 + 2
    n = w.double() * x * rstd
    if cos is None:
        ref = n * out_scale
        return ref, SLACK * (R + 3) * U * ref.abs()
    p = rope_pairs(X.shape[1], hd)
    c, s = cos.double()[tok][:, p], sin.double()[tok][:, p]                  # (rows, D / 2)
    n0, n1 = n[:, 0::2], n[:, 1::2]
    ref = torch.stack((n0 * c - n1 * s, n1 * c + n0 * s), -1).reshape(x.shape) * out_scale
    mag = torch.stack((n0.abs() * c.abs() + n1.abs() * s.abs(), n1.abs() * c.abs() + n0.abs() * s.abs()), -1).reshape(x.shape)
    return ref, SLACK * (abs(out_scale) * (R + 3) * U * mag + 2 * U * ref.abs())


# ---- checker ------------------------------------------------------------------------------------------------------------------
def check_margin_bf16(got, ref64, margin64, what=""):
    """got (bf16) is accepted iff every element is the RNE bf16 of some real number in [ref - m, ref + m], i.e. rne(ref - m) <= got <= rne(ref + m).
    Returns (undecided share, count "not RNE but allowed") and prints them; the share is that of the elements whose interval contains a rounding
    boundary.  Raises AssertionError."""
    assert got.dtype == BF16 and got.shape == ref64.shape == margin64.shape and ref64.dtype == F64, (got.dtype, got.shape, ref64.shape, margin64.shape)
    g = got.double().cpu()
    assert bool(torch.isfinite(g).all()), f"{what}: {int((~torch.isfinite(g)).sum())} non-finite (or unwritten) output elements"
    lo, hi = rne_bf16(ref64 - margin64), rne_bf16(ref64 + margin64)
    undecided = lo != hi
    inside = (g >= lo) & (g <= hi)
    share = float(undecided.double().mean()) if g.numel() else 0.0
    allowed = int(((g != rne_bf16(ref64)) & inside).sum())
    print(f"{what}: undecided share {share:.4%}, not RNE but allowed {allowed} of {g.numel()}")
    if not bool(inside.all()):
        bad = ~inside
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements ({int((bad & ~undecided).sum())} of them decided by fp32 arithmetic) are not the rounding of "
                             f"anything in [ref - m, ref + m]; first at {i}: got {float(g.flatten()[i])!r}, ref {float(ref64.flatten()[i])!r}, "
                             f"m {float(margin64.flatten()[i])!r}")
    return share, allowed


def check_case(got, ref, margin, n_special, what):
    """regular rows under the cap, special rows (the last n_special) apart and without one.  -> dict of the four figures"""
    rows = ref.shape[0]
    k = rows - n_special
    share, allowed = check_margin_bf16(got[:k], ref[:k], margin[:k], what)
    out = dict(share=share, allowed=allowed, special_share=0.0, special_allowed=0)
    if n_special:
        out["special_share"], out["special_allowed"] = check_margin_bf16(got[k:], ref[k:], margin[k:], what + " [special rows]")
    assert share <= UNDECIDED_CAP, (what, share)
    return out


# ---- the kernels' chains restated with IEEE fp32 operations (torch on the CPU), in block and in wave order ----------------------------
def row_sum_fp32(v, kind, drop_chunk=None):
    """sum over the last dim of v (rows, D) fp32 in the order of block_sum_256 after the per-thread serial loop ("block": thread t holds the 8-element
    chunks t, t + 256, t + 512) or of wave_sum ("wave": lane l holds chunks l, l + 64, ..).  drop_chunk: a chunk left out (a seeded fault)."""
    rows, D = v.shape
    nvec = D // 8
    T = 256 if kind == "block" else 64
    per = (nvec + T - 1) // T
    ch = torch.zeros(rows, per * T, 8, dtype=F32)                            # absent chunks add +0: exact
    ch[:, :nvec] = v.reshape(rows, nvec, 8)
    if drop_chunk is not None:
        ch[:, drop_chunk] = 0
    ch = ch.reshape(rows, per, T, 8)
    s = torch.zeros(rows, T, dtype=F32)
    for j in range(per):
        for e in range(8):
            s = s + ch[:, j, :, e]
    s = s.reshape(rows, T // 64, 64)
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, lanes ^ o]
    s = s[:, :, 0]
    r = s[:, 0]
    for w in range(1, s.shape[1]):
        r = r + s[:, w]
    return r[:, None]


def _store(o32, fault):
    if fault == "truncate":
        return truncate_bf16(o32.double()).float().to(BF16)
    return o32.to(BF16)


def ln_fp32(c, inp, kind, fault=None):
    """ln_kernel / ln_wave_kernel on the case's raw inputs -> (n_batch * rows_out, D) bf16.  fault: one of LN_FAULTS"""
    D, B, ro = c["D"], inp["n_batch"], inp["rows_out"]
    off = 0 if fault == "src_row_offset ignored" else c["src_off"]
    xs = inp["x_src"][:, off:off + ro, :D].reshape(B * ro, D).float()
    eps = torch.tensor({"eps 1e-5": 1e-5, "eps dropped": 0.0}.get(fault, c["eps"]), dtype=F32)
    Df = torch.tensor(float(D), dtype=F32)
    inv = (1.0 / Df) if kind == "wave" else None
    S = row_sum_fp32(xs, kind, 1 if fault == "chunk left out of the mean" else None)
    mean = S * inv if kind == "wave" else S / Df
    d = xs - mean
    Q = row_sum_fp32(d * d, kind, 1 if fault == "chunk left out of the sum of squares" else None)
    if fault == "variance over D - 1":
        var = Q / (Df - 1)
    else:
        var = Q * inv if kind == "wave" else Q / Df
    rstd = torch.rsqrt(var + eps)
    b_of = torch.arange(B * ro) // ro
    if fault == "batch 0's modulation":
        b_of = b_of * 0
    if c["form"] == "mod":
        sc = inp["scale"][b_of]
        M, Ad = (sc if fault == "scale instead of 1 + scale" else 1.0 + sc), inp["shift"][b_of]
    else:
        M, Ad = inp["w"][None], inp["b"][None]
    o = d * rstd * M + Ad
    out = _store(o, fault)
    if fault == "output row unwritten":
        out[B * ro // 2] = float("nan")
    return out


def rms_fp32(c, inp, kind, fault=None):
    """rmsnorm_rope_kernel / rmsnorm_rope_wave_kernel on the case's raw inputs -> (rows, D) bf16.  fault: one of RMS_FAULTS"""
    D, hd, rows = c["D"], c["hd"], inp["rows"]
    x = inp["x"].float()
    eps = torch.tensor({"eps 1e-5": 1e-5, "eps dropped": 0.0}.get(fault, EPS), dtype=F32)
    Df = torch.tensor(float(D), dtype=F32)
    Q = row_sum_fp32(x * x, kind, 1 if fault == "chunk left out of the sum of squares" else None)
    var = Q * (1.0 / Df) if kind == "wave" else Q / Df
    rstd = torch.rsqrt(var + eps)
    n = inp["w"][None] * (x * rstd)
    os_ = torch.tensor(c["out_scale"], dtype=F32)
    if not c["rope"]:
        o = n
    else:
        half = hd // 2
        cos, sin = inp["cos_full"].reshape(-1), inp["sin_full"].reshape(-1)           # the whole allocation, flat: a wrong index reads what lies there
        r = torch.arange(rows)
        tok = {"table row r": r, "table row r + 1": (r + 1) % inp["rpb"]}.get(fault, r % inp["rpb"]) + inp["row0"]
        chunk = torch.arange(D // 8)
        p0 = ((chunk * 8) % hd) // 2
        if fault == "pair index shifted by one chunk":
            p0 = (p0 + 4) % half
        base = tok[:, None] * half + p0[None]
        if fault == "HD128 shortcut at another head_dim":
            base = tok[:, None] * 64 + ((chunk % 64) & 15)[None] * 4
        idx = ((base[:, :, None] + torch.arange(4)[None, None]) % cos.numel()).reshape(rows, D // 2)
        C, S = cos[idx], sin[idx]
        if fault == "sine sign flipped":
            S = -S
        n0, n1 = n[:, 0::2], n[:, 1::2]
        o = torch.stack((n0 * C - n1 * S, n1 * C + n0 * S), -1).reshape(rows, D)
    if fault == "out_scale after a bf16 rounding":
        return (o.to(BF16).float() * os_).to(BF16)
    return _store(o * os_, fault)


LN_FAULTS = ("variance over D - 1", "eps 1e-5", "eps dropped", "chunk left out of the mean", "chunk left out of the sum of squares",
             "scale instead of 1 + scale", "batch 0's modulation", "src_row_offset ignored", "truncate", "output row unwritten")
RMS_FAULTS = ("sine sign flipped", "pair index shifted by one chunk", "table row r", "table row r + 1", "HD128 shortcut at another head_dim",
              "out_scale after a bf16 rounding", "truncate", "eps dropped", "chunk left out of the sum of squares")


# ---- cases --------------------------------------------------------------------------------------------------------------------
def _ln(id, form, D, kind, launches=(), n_batch=1, rows=None, src_rows=None, src_off=0, ldx_pad=0, mod="plain", eps=EPS, loops=False):
    """form "mod" | "aff"; kind the kernel family the case must run ("block" cases run under option row_wave = 0 where D has a wave kernel); rows: regular
    rows per batch element, a number or a function of the CU count; launches: extra launches on the first k regular rows alone (n_batch = 1 only);
    mod: "plain" (shift, scale dense (B, D)) | 6 | 2 (views into one (B, k D) table, mod_stride = k D); loops: assert rows_out > 4 x workgroups per batch"""
    return dict(id=id, form=form, D=D, kind=kind, launches=tuple(launches), n_batch=n_batch, rows=rows if rows is not None else 37, src_rows=src_rows,
                src_off=src_off, ldx_pad=ldx_pad, mod=mod, eps=f32(eps), loops=loops)


LN_CASES = []
for _f in ("mod", "aff"):
    LN_CASES += [_ln(f"ln-{_f}-block-{D}", _f, D, "block", (1, 3)) for D in (8, 264, 1280, 2056, 4104, 6144)]
    LN_CASES += [_ln(f"ln-{_f}-wave-{D}", _f, D, "wave", (1, 3, 5)) for D in (1536, 2048, 4096, 5120, 6144)]
    LN_CASES += [_ln(f"ln-{_f}-wave-persistent", _f, 1536, "wave", rows=lambda cus: 12 * cus + 5, loops=True)]
LN_CASES += [
    _ln("ln-mod-wave-5-batches", "mod", 1536, "wave", n_batch=5, rows=lambda cus: 4 * ((3 * cus + 4) // 5) + 3, loops=True),
    _ln("ln-mod-wave-3cus-batches", "mod", 1536, "wave", n_batch=lambda cus: 3 * cus, rows=9, loops=True),      # one workgroup per batch element, three ragged rounds
    # the executor's calling forms (csrc/dit_step.hip): modulation rows inside one table, a row slice of every batch element, a view into a wider buffer
    _ln("ln-mod-wave-table6-slice-ldx", "mod", 1536, "wave", n_batch=2, rows=20, src_rows=50, src_off=5, ldx_pad=64, mod=6),
    _ln("ln-mod-block-table2-slice-ldx", "mod", 264, "block", n_batch=3, rows=20, src_rows=50, src_off=5, ldx_pad=64, mod=2),
    _ln("ln-aff-block-eps1e-5-ldx", "aff", 1280, "block", ldx_pad=8, eps=1e-5),
    _ln("ln-aff-wave-eps1e-5-ldx", "aff", 2048, "wave", ldx_pad=8, eps=1e-5),
]


def _rms(id, D, hd, kind, rope=True, out_scale=1.0, rows=37, launches=(), call="plain", loops=False):
    """call: plain (separate output, ldy = D + 8) | inplace3 (the middle third of a (rows, 3 D) buffer) | ldy2 | batch3 (three batch elements share one
    table) | row0 (a table view offset by row0 rows, rows_per_batch = rows) | slab (slab_ld = 3 slab_w) | copy (w == NULL, slab layout)"""
    return dict(id=id, D=D, hd=hd, kind=kind, rope=rope, out_scale=f32(out_scale), rows=rows, launches=tuple(launches), call=call, loops=loops)


RMS_CASES = (
    [_rms(f"rms-block-{D}-hd{hd}", D, hd, "block", launches=(1, 5)) for D, hd in ((128, 128), (256, 64), (1280, 80), (4104, 216))] +
    [_rms("rms-block-4096-norope", 4096, 128, "block", rope=False), _rms("rms-block-5120-norope-scaled", 5120, 128, "block", rope=False, out_scale=ATTN_LOG2_SCALE),
     _rms("rms-block-5120-rope", 5120, 128, "block-forced", out_scale=ATTN_LOG2_SCALE)] +
    [_rms(f"rms-wave-{D}-hd128", D, 128, "wave", launches=(1, 5), out_scale=ATTN_LOG2_SCALE if D == 5120 else 1.0) for D in (1536, 2048, 4096, 5120, 6144)] +
    [_rms(f"rms-wave-{D}-hd{hd}", D, hd, "wave", launches=(1, 5)) for D, hd in ((1536, 64), (1536, 96), (2048, 256), (1536, 1536))] +
    [_rms("rms-wave-persistent", 1536, 128, "wave", rows=lambda cus: 12 * cus + 5, loops=True),
     _rms("rms-wave-inplace3", 1536, 128, "wave", call="inplace3"), _rms("rms-wave-ldy2", 1536, 128, "wave", call="ldy2"),
     _rms("rms-wave-batch3", 1536, 128, "wave", rows=39, call="batch3"), _rms("rms-block-batch3", 256, 64, "block", rows=39, call="batch3"),
     _rms("rms-wave-row0", 1536, 128, "wave", call="row0", out_scale=ATTN_LOG2_SCALE), _rms("rms-block-row0", 256, 64, "block", call="row0"),
     _rms("rms-wave-slab", 1536, 128, "wave", call="slab", out_scale=ATTN_LOG2_SCALE), _rms("rms-block-slab", 256, 64, "block", call="slab"),
     _rms("rms-block-slab-norope", 1536, 128, "block", rope=False, call="slab")])
ROW0 = 11                                      # the table offset of the "row0" cases


def case_of(id):
    return next(c for c in LN_CASES + RMS_CASES if c["id"] == id)


def _n(v, cus):
    return v(cus) if callable(v) else v


@functools.lru_cache(maxsize=None)
def _ln_inputs(id, cus):
    c = case_of(id)
    g = torch.Generator().manual_seed(seed_of(c))
    D, B, rows = c["D"], _n(c["n_batch"], cus), _n(c["rows"], cus)
    n_special = N_SPECIAL
    rows_out = rows + N_SPECIAL if B == 1 else rows          # one batch element: the special rows are appended; more: they are the last six of the last element
    assert rows_out > N_SPECIAL
    src_rows = c["src_rows"] or rows_out
    X = regular_rows(B * rows_out, D, g).reshape(B, rows_out, D)
    X[B - 1, rows_out - N_SPECIAL:] = special_rows(D, g)
    x_src = regular_rows(B * src_rows, D + c["ldx_pad"], g).reshape(B, src_rows, D + c["ldx_pad"])     # other values around the rows the call reads
    x_src[:, c["src_off"]:c["src_off"] + rows_out, :D] = X
    inp = dict(x_src=x_src, X=X.reshape(B * rows_out, D), rows_out=rows_out, src_rows=src_rows, n_batch=B, n_special=n_special)
    A = depth(c["kind"], D)
    if c["form"] == "mod":
        k = 1 if c["mod"] == "plain" else c["mod"]
        table = torch.randn(B, k * D, generator=g) * (0.3 if k == 1 else 1.0)
        scale_table = torch.randn(B, k * D, generator=g) * 0.3
        if k == 1:
            shift, scale = torch.randn(B, D, generator=g), scale_table
        else:                                               # shift | scale are chunks 0 | 1 of every batch element's row of ONE table
            table[:, D:2 * D] = scale_table[:, :D]
            shift, scale = table[:, :D], table[:, D:2 * D]
        inp.update(table=table, shift=shift, scale=scale)
        b_of = torch.arange(B * rows_out) // rows_out
        mult, add = (1.0 + scale.double())[b_of], shift.double()[b_of]
    else:
        inp.update(w=1 + 0.3 * torch.randn(D, generator=g), b=torch.randn(D, generator=g))
        mult, add = inp["w"].double()[None].expand(B * rows_out, D), inp["b"].double()[None].expand(B * rows_out, D)
    inp["ref"], inp["margin"] = ln_reference(inp["X"], mult, add, c["eps"], A)
    inp["add"] = add
    return inp


def ln_inputs(c, cus=NOMINAL_CUS):
    """the case's inputs, fp64 reference and margin: computed once, shared, never modified"""
    return _ln_inputs(c["id"], cus)


@functools.lru_cache(maxsize=None)
def _rms_inputs(id, cus):
    c = case_of(id)
    g = torch.Generator().manual_seed(seed_of(c))
    D, hd = c["D"], c["hd"]
    rows = _n(c["rows"], cus) + N_SPECIAL
    x = torch.cat((regular_rows(rows - N_SPECIAL, D, g), special_rows(D, g)))
    w = 1 + 0.3 * torch.randn(D, generator=g)
    rpb = rows // 3 if c["call"] == "batch3" else rows
    row0 = ROW0 if c["call"] == "row0" else 0
    inp = dict(x=x, w=w, rows=rows, rpb=rpb, row0=row0, n_special=N_SPECIAL)
    kind = "block" if c["kind"].startswith("block") else "wave"
    if c["rope"]:
        n_tab = rows + row0 + 1                              # a table larger than the call needs: a wrong row index reads other angles, not outside
        cos, sin = rope_tables(n_tab, hd // 2, g)
        inp.update(cos_full=cos, sin_full=sin, cos=cos[row0:], sin=sin[row0:])
        inp["ref"], inp["margin"] = rms_reference(x, w, f32(EPS), depth(kind, D), inp["cos"], inp["sin"], torch.arange(rows) % rpb, hd, c["out_scale"])
    else:
        inp["ref"], inp["margin"] = rms_reference(x, w, f32(EPS), depth(kind, D), out_scale=c["out_scale"])
    return inp


def rms_inputs(c, cus=NOMINAL_CUS):
    return _rms_inputs(c["id"], cus)


# ---- the route ----------------------------------------------------------------------------------------------------------------
FORM_CODE = {"mod": 0, "aff": 1, "rms": 2, "rope": 3, "copy": 4}             # include/scail_hip.h SCAIL_ROW_*


def expected_name(c):
    """the kernel the case must run, by the rule of csrc/rowops.hip row_choose"""
    cpl = c["D"] // 512
    if "form" in c:
        m = "0" if c["form"] == "mod" else "1"
        return f"ln_wave_kernel<{m}, {cpl}>" if c["kind"] == "wave" else f"ln_kernel<{m}>"
    return f"rmsnorm_rope_wave_kernel<{cpl}, {'true' if c['hd'] == 128 else 'false'}>" if c["kind"] == "wave" else "rmsnorm_rope_kernel"


def options_of(c):
    """block cases at a D the wave kernels cover run under row_wave = 0 -- except the RMSNorm without RoPE, which takes the block kernel by the rule"""
    wave_D = c["D"] // 512 in (3, 4, 8, 10, 12) and c["D"] % 512 == 0
    if "form" in c:
        return {"row_wave": 0} if c["kind"] == "block" and wave_D else {}
    return {"row_wave": 0} if c["kind"] == "block-forced" else {}


def kernel_name(form, n_batch, rows_out, D, hd=128, want_grid=False):
    """(name, workgroups or None) from scail_row_kernel_name_for under the options in force"""
    import ctypes as C
    from scail_amd import lib as L
    buf, wg = C.create_string_buffer(128), C.c_int64(-1)
    L.call("scail_row_kernel_name_for", FORM_CODE[form], n_batch, rows_out, D, hd, buf, len(buf), C.cast(C.byref(wg), C.c_void_p) if want_grid else None)
    return buf.value.decode(), (wg.value if want_grid else None)


def with_options(opts, fn):
    """fn() under the library options ``opts``; the default (row_wave = 1) is back afterwards, whatever happens"""
    from scail_amd import lib as L
    try:
        for name, v in opts.items():
            L.set_option(name, v)
        return fn()
    finally:
        for name in opts:
            L.set_option(name, 1)


# ---- one case on tables handed in (the test files take them from the oracle's rope_tables) ----------------------------------------------
def table_case(cos, sin, D, seed=1536):
    """regular rows only, one per table row, head_dim 128, the wave kernel's depth.  -> (ref, margin, x, w)"""
    g = torch.Generator().manual_seed(seed)
    rows = cos.shape[0]
    x, w = regular_rows(rows, D, g), 1 + 0.3 * torch.randn(D, generator=g)
    ref, margin = rms_reference(x, w, f32(EPS), depth("wave", D), cos, sin, torch.arange(rows), 128, 1.0)
    return ref, margin, x, w


# ---- scail_small_linear -------------------------------------------------------------------------------------------------------
def small_linear_operands(M, N, K):
    """integer x (fp32) in [-3, 3], integer bf16 weights in [-2, 2], integer bias in [-8, 8]; y64 = x w^T + b in fp64"""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    x = torch.randint(-3, 4, (M, K), generator=g).float()
    w = torch.randint(-2, 3, (N, K), generator=g).float().to(BF16)
    b = torch.randint(-8, 9, (N,), generator=g).float()
    return x, w, b, x.double() @ w.double().t() + b.double()[None]


def silu64(x):
    return x / (1 + torch.exp(-x))


def budget_silu(x):
    return 2.0 * (2 + torch.sigmoid(-x) * (2 + 2 * x.abs())) * U * silu64(x).abs()


def small_linear_act_case(M, N, K, act_in, act_out):
    """-> x fp32 (M, K), w bf16 (N, K), b fp32 (N), the fp64 reference and the absolute margin (module docstring).  Without an input activation the
    operands are multiples of 1/4 and 1/2 in 12 columns, so that the pre-activation is exact and |v| <= 7."""
    import gemm_exact
    act64 = {0: lambda v: v, 1: silu64, 2: gemm_exact.gelu_tanh64}
    budget = {1: budget_silu, 2: gemm_exact.budget_tanh}
    g = torch.Generator().manual_seed(100 * K + 10 * act_in + act_out)
    A = 8 * ((K + 511) // 512) + 6
    if act_in:
        x = (1.5 * torch.randn(M, K, generator=g)).clamp(-6, 6)
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(BF16)
        b = torch.randn(N, generator=g)
        a = act64[act_in](x.double())
        aw = a.abs() @ w.double().abs().t()
        v = a @ w.double().t() + b.double()[None]
        m_pre = budget[act_in](x.double()) @ w.double().abs().t() + (A + 2) * U * (aw + b.double().abs()[None])
    else:
        x = torch.zeros(M, K)
        cols = torch.randperm(K, generator=g)[:min(K, 12)]
        x[:, cols] = torch.randint(-2, 3, (M, len(cols)), generator=g).float() / 4
        w = (torch.randint(-2, 3, (N, K), generator=g).float() / 2).to(BF16)
        b = torch.randint(-4, 5, (N,), generator=g).float() / 4
        v = x.double() @ w.double().t() + b.double()[None]
        m_pre = torch.zeros_like(v)                          # multiples of 1/8 below 2^24 / 8: every partial sum is exact
    assert float(x.abs().max()) <= 8 and float(v.abs().max()) <= 8
    if not act_out:
        return x, w, b, v, SLACK * m_pre
    return x, w, b, act64[act_out](v), SLACK * 1.2 * m_pre + budget[act_out](v)
