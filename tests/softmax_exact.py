"""Exact-arithmetic helpers for the two softmax kernels outside the flash-attention family (tests/test_softmax_exact_cpu.py,
tests/test_softmax_exact_gpu.py): softmax_rows_kernel<4> / <16> (csrc/conv.hip, the VAE's mid-block attention) and attn_small_kernel
(csrc/rowops.hip, every attention of the UMT5 and CLIP encoders).  The rounding helpers, the checker (check_budget_bf16 / check_interval_bf16:
rne(ref - B) <= o <= rne(ref + B), and where the two ends coincide the element is decided and must be that value), raw_scale(), SLACK = 2 and
UNDECIDED_CAP = 5 % come from tests/gemm_exact.py and tests/attn_exact.py.  The share of undecided elements is a condition on the INPUTS, asserted
on the CPU for the reference alone.

Every budget B is a first-order absolute error bound in units of u = 2^-24, times SLACK for the second-order terms, built from the kernel's
operation chain and the ISA manual's figures that the sibling modules use (not measured): v_exp_f32 and v_rcp_f32 1 ulp = 2 u, an IEEE division
or product u (scail_amd/build.py compiles with -O3 only), an addition u of its result, a contraction only removes a rounding.  No budget is taken
from what a kernel returns.

1. scail_softmax_rows (in place, n valid columns of a row of ld >= ceil8(n) elements).  The chain of softmax_rows_kernel<MAXV>, MAXV = 4 for
   n <= 8192 and 16 above: 256 threads, thread t holds the 8-column chunks t + 256 j (j < MAXV); columns n .. ceil8(n) are replaced with -inf
   before anything reads them; mx = row maximum (exact); sl2 = fl(scale * fl(log2 e)); p = v_exp_f32(fl((s - mx) * sl2)); the row sum: each
   thread adds its 8 MAXV values one after the other (the first to 0.0), a 6-step butterfly inside each wave, then red[0] + red[1] + red[2] +
   red[3]: an element passes through at most 8 MAXV - 1 + 6 + 3 = 8 MAXV + 8 additions, every partial sum is at most the row sum (p >= 0);
   inv = 1.0f / sum (IEEE); o = bf16(p * inv); the columns n .. ceil8(n) are written as p = v_exp_f32(-inf) = +0.
   Exact regime: scale = raw_scale(), whose sl2 -- the same single fp32 product -- is exactly 2^-3; scores 8 (k + c) with k an integer in
   [-9, 0], at least one k = 0 per row, and a per-row integer c with |k + c| <= 255, so that every score is a bf16 value.  Then (s - mx) sl2 = k
   exactly, every p is a power of two, and with 2^9 sum p < 2^24 (asserted per row; true up to n = 32768) every partial sum is an integer
   multiple of 2^-9 below 2^15: exact in fp32 in any order.  What is left is bf16(p * (1.0f / sum)): the numerator's v_exp 2 u, the denominator's
   v_exp results 2 u (a weighted mean of relative errors of at most 2 u each), the division u, the product u:
       B = SLACK (2 + 2 + 2) u |ref|.
   General regime (scale = float(1 / sqrt(C)), C = 384 and 128: what the VAE passes): scores are bf16 multiples of 2^-6 below 2^8, so s - mx is
   exact in fp32 (asserted), and t = (s - mx) scale log2(e) stays above -60 (asserted): no p is near the denormal range of the raw v_exp_f32.
   The reference is softmax(scale * s) in fp64 with the fp32 value of scale.  Per element j, relative to ref_j = w_j = p_j / sum p:
       sl2: fl(log2 e) u and the product u = 2 u; the product (s - mx) * sl2: u; together 3 u |t_j| on the argument in log2 units, which is
           3 ln 2 |t_j| u = 2.08 |t_j| u on the weight;  v_exp_f32: 2 u;       e_j = (3 ln 2 |t_j| + 2) u
       the row sum: sum_i w_i e_i from its terms, (8 MAXV + 8) u from its additions;  the division: u;  the final product: u
       B_j = SLACK u ref_j (e_j + sum_i w_i e_i + 8 MAXV + 8 + 2).
   The largest relative budget is a few hundred u, against a bf16 half ulp of 2^-9 = 32 768 u.

2. scail_attn_small.  The chain of attn_small_kernel: Q[d] = fl(bf16 q * scale); s = sum over head_dim of Q[d] * k[d] (one after the other,
   possibly fused) [+ bias_tab[bucket[i, j] * heads + h]] [= -inf where the key mask is 0]; mx = row maximum; P_j = __expf(s_j - mx);
   sum: each lane adds its ceil(Lk / 64) values one after the other, then a 6-step butterfly; inv = 1.0f / sum; acc_d = sum over ALL Lk keys, one
   after the other, of P_j * v_j[d]; o = bf16(acc * inv).
   __expf(x) is __builtin_amdgcn_exp2f(0x1.715476p+0f * x) -- read in clang's HIP device header __clang_hip_math.h, not in a disassembly -- so it is
   v_exp_f32 of a ROUNDED product and not exact at integers: this is a margin test, not a bit test.
   Operands: the sparse / dense integer construction of attn_exact.exact_qkv for head_dim 64, 80 and 128: one of q, k has four +-1 per (row, head),
   one in each quarter of the head, the other is dense in {-1, 0, 1}, both roles run; the bias table holds fp32 integers in [-2, 2] (bias_table():
   every entry differs from the other heads' entries of its bucket and from the entry a transposed index h * buckets + bucket would fetch); the
   bucket matrix is umt5.relative_position_bucket; scale is 1.0, or 2^-3 with q holding +-8.  Then Q is exact, every score is an integer, exact in
   fp32 in any order, and x_j = s_j - mx is an integer <= 0 (asserted).  The case with CLIP's real scale 80^-1/2 keeps q in {-1, 0, 1}: Q is +-scale
   exactly, and the score carries at most E = (head_dim + 1) u scale sum|q k| <= 4 (head_dim + 1) u scale (one rounding for Q, head_dim fused
   products); there x_j is off by at most 2 E + u |x_j| (both scores and the subtraction), which enters the weight 1 : 1.
       weight j: the argument fl(x * fl(log2 e)) is off by 2 u |x| log2 e, which is 2 |x| u on the weight; v_exp_f32 2 u:
           e_j = (2 |x_j| + 2) u  [+ 2 E + u |x_j| under the real scale]
       row sum: sum_j w_j e_j from its terms, (ceil(Lk / 64) + 6) u from its additions;  1.0f / sum: u;  acc * inv: u
       acc: sum_j w_j e_j |v_j| from the weights; Lk products and additions one after the other: Lk u sum_j w_j |v_j| = Lk u A
       B = SLACK u (sum_j w_j e_j |v_j| + Lk A + |ref| (sum_j w_j e_j + ceil(Lk / 64) + 6 + 2)).
   A row with ONE unmasked key (the unconditional prompt) has P = v_exp_f32(+-0) = 1 for that key (the ISA manual's functional examples, on which
   the sibling modules rely as well) and v_exp_f32(-inf) = 0 for the others, sum 1 and acc = that key's v row: B = 0, bit for bit.
   The cap decides the V operand: Lk u A against |ref| is small only without cancellation, so v holds integers in [1, 7] wherever Lk > 65 and
   signed integers in [-7, 7] in the cases with Lk <= 65, which is where a sign error would show.

The module also restates both chains with IEEE fp32 operations in torch (softmax_fp32, attn_small_fp32) with the seeded faults the CPU tests want
rejected.  It reads nothing outside tests/ and scail_amd/."""
import functools
import math

import numpy as np
import torch

from attn_exact import SLACK, UNDECIDED_CAP, check_interval_bf16, decided, raw_scale, undecided_share      # noqa: F401  (re-exported)
from conv_exact import BF16, U, _is_bf16, assert_bits, seed_of                                             # noqa: F401
from gemm_exact import check_budget_bf16, rne_bf16, truncate_bf16                                          # noqa: F401

LOG2E = 1.4426950408889634
LOG2E_F32 = np.float32(LOG2E)
LN2 = math.log(2.0)
T_MIN = -60.0


def ceil8(n):
    return (n + 7) // 8 * 8


# ================================================================================================================================================
# 1. scail_softmax_rows
# ================================================================================================================================================
SM_ROWS = 3
SM_OFFSETS = (0, 100, -200)                                   # the per-row integer c: |k + c| <= 255
SM_EXACT_N = (1, 7, 8, 9, 2047, 2048, 2056, 8191, 8192, 8193, 8200, 24584, 32767, 32768)
SM_GENERAL = [(n, C) for n in (35, 81, 7168, 8200) for C in (384, 128)]
SM_SIGMA = 24.0
SM_POISON = (3.0e38, float("nan"), float("-inf"))             # columns n .. ceil8(n) before the call, one row each


def maxv_of(n):
    return 4 if n <= 8192 else 16


def vae_scale(C):
    """what wan_vae.py and csrc/vae_exec.hip hand the kernel: 1 / sqrt(C) in double, rounded once"""
    return float(np.float32(1.0 / math.sqrt(C)))


def softmax_exact_scores(n):
    """(SM_ROWS, n) fp32 scores 8 (k + c): row 0 has its only k = 0 in the last valid column, row 1 its only one in column 0, row 2 at a seeded place"""
    g = torch.Generator().manual_seed(7000 + n)
    k = torch.randint(-9, 1, (SM_ROWS, n), generator=g)
    k[0] = torch.randint(-9, 0, (n,), generator=g)
    k[1] = torch.randint(-9, 0, (n,), generator=g)
    k[0, n - 1] = 0
    k[1, 0] = 0
    k[2, int(torch.randint(0, n, (1,), generator=g))] = 0
    s = 8.0 * (k + torch.tensor(SM_OFFSETS)[:, None]).float()
    assert _is_bf16(s)
    return s, k


def softmax_exact_reference(n):
    """dict(s, ref, budget): the exact regime (module docstring); asserts its conditions"""
    s, k = softmax_exact_scores(n)
    assert bool((k.amax(-1) == 0).all()) and int(k.min()) >= -9
    assert float(np.float32(np.float32(raw_scale()) * LOG2E_F32)) == 0.125
    assert bool(((s.double() - s.double().amax(-1, keepdim=True)) * 0.125 == k.double()).all())
    p = torch.exp2(k.double())
    l = p.sum(-1, keepdim=True)
    assert bool((2 ** 9 * l < 2 ** 24).all()), "exactness bound: 2^9 sum p < 2^24 in every row"
    ref = p / l
    return dict(s=s, ref=ref, budget=SLACK * (2 + 2 + 2) * U * ref)


def softmax_general_scores(n, C):
    g = torch.Generator().manual_seed(9000 + n + C)
    s = (torch.round(torch.randn(SM_ROWS, n, generator=g) * SM_SIGMA * 64) / 64).to(BF16).float()
    return s


def softmax_general_reference(n, C):
    """dict(s, ref, budget, rel): the general regime (module docstring); rel = budget / (u ref)"""
    s = softmax_general_scores(n, C)
    assert bool((s * 64 == (s * 64).round()).all()) and float(s.abs().max()) < 256
    mx = s.amax(-1, keepdim=True)
    assert bool(((s - mx).double() == s.double() - mx.double()).all()), "s - mx is exact in fp32"
    z = (s.double() - mx.double()) * vae_scale(C)
    t = z * LOG2E
    assert float(t.min()) > T_MIN
    p = torch.exp(z)
    w = p / p.sum(-1, keepdim=True)
    e = 3 * LN2 * t.abs() + 2
    first = e + (w * e).sum(-1, keepdim=True) + 8 * maxv_of(n) + 8 + 2
    return dict(s=s, ref=w, budget=SLACK * U * w * first, rel=SLACK * first, t_min=float(t.min()))


def softmax_buffer(s, n):
    """the scores in a NaN-filled (rows, ld) bf16 buffer, ld = ceil8(n) + 24, with the poisoned columns n .. ceil8(n)"""
    buf = torch.full((s.shape[0], ceil8(n) + 24), float("nan"), dtype=BF16)
    buf[:, :n] = s.to(BF16)
    for r in range(s.shape[0]):
        buf[r, n:ceil8(n)] = SM_POISON[r % 3]
    return buf


def check_softmax_output(got, before, r, n, what):
    """got, before: the (rows, ld) bf16 buffer after and before the call: the poisoned columns came back as +0 bits, the columns from ceil8(n) on
    kept their bits, the valid columns are inside the budget; returns the undecided share"""
    got, n8 = got.cpu(), ceil8(n)
    share = check_budget_bf16(got[:, :n].contiguous(), r["ref"], r["budget"], what)
    assert bool((got[:, n:n8].contiguous().view(torch.int16) == 0).all()), f"{what}: columns n .. ceil8(n) are not +0"
    assert torch.equal(got[:, n8:].contiguous().view(torch.int16), before[:, n8:].contiguous().view(torch.int16)), f"{what}: columns from ceil8(n) on were written"
    assert bool(torch.isnan(got[:, n8:].float()).all())
    return share


def softmax_fp32(buf, n, scale, fault=None):
    """softmax_rows_kernel's chain in IEEE fp32 on the (rows, ld) bf16 buffer of softmax_buffer(): the buffer after the call.  Seeded faults:
    tail_zero (the ragged tail counted as score 0), wave_dropped (wave 1's partial sum), last_chunk (the last register chunk left out of the sum),
    maxv_mixup (the MAXV = 4 kernel above 8192: columns >= 8192 neither read nor written), natural (sl2 without log2 e), sum_2m8, truncated"""
    f32 = torch.float32
    rows, n8 = buf.shape[0], ceil8(n)
    maxv = 4 if fault == "maxv_mixup" else maxv_of(n)
    cols = maxv * 2048
    m = min(n8, cols)
    v = torch.full((rows, cols), float("-inf"), dtype=f32)
    v[:, :m] = buf[:, :m].float()
    if n < m:
        v[:, n:m] = 0.0 if fault == "tail_zero" else float("-inf")
    mx = v.amax(-1, keepdim=True)
    sl2 = torch.tensor(scale, dtype=f32) * (1.0 if fault == "natural" else torch.tensor(LOG2E, dtype=f32))
    p = torch.exp2((v - mx) * sl2)
    pt = p.view(rows, maxv, 256, 8)                                                          # column (t + 256 j) 8 + e
    acc = torch.zeros(rows, 256, dtype=f32)
    for j in range(maxv):
        if fault == "last_chunk" and j == maxv - 1:
            continue
        for e in range(8):
            acc = acc + pt[:, j, :, e]
    w = acc.view(rows, 4, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, lane ^ o]
    red = w[:, :, 0].clone()
    if fault == "wave_dropped":
        red[:, 1] = 0
    total = (((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3])[:, None]
    if fault == "sum_2m8":
        total = total * (1 + 2.0 ** -8)
    y = p * (1.0 / total)
    out = buf.clone()
    out[:, :m] = (truncate_bf16(y[:, :m].double()).float() if fault == "truncated" else y[:, :m]).to(BF16)
    return out


# ================================================================================================================================================
# 2. scail_attn_small
# ================================================================================================================================================
N_BUCKETS = 32
REAL_SCALE_80 = float(np.float32(80 ** -0.5))


def _sparse(rows, hd, g, mag):
    """(rows, hd): 4 non-zeros +-mag, one at a seeded position in each quarter of the head"""
    pos = torch.randint(0, hd // 4, (rows, 4), generator=g) + torch.arange(4) * (hd // 4)
    sign = torch.randint(0, 2, (rows, 4), generator=g).float() * 2 - 1
    return torch.zeros(rows, hd).scatter_(1, pos, sign * mag)


def _dense(rows, hd, g, mag):
    return torch.randint(-1, 2, (rows, hd), generator=g).float() * mag


def small_qkv(kind, B, H, Lq, Lk, hd, seed, qmag=1.0, signed_v=False):
    """q (B, Lq, H hd), k, v (B, Lk, H hd) fp32 on the CPU: attn_exact.exact_qkv for any head_dim, without its reserved dimensions"""
    assert kind in ("sparse_q", "sparse_k") and hd % 4 == 0
    g = torch.Generator().manual_seed(seed)
    q = (_sparse if kind == "sparse_q" else _dense)(B * Lq * H, hd, g, qmag).view(B, Lq, H * hd)
    k = (_dense if kind == "sparse_q" else _sparse)(B * Lk * H, hd, g, 1.0).view(B, Lk, H * hd)
    v = torch.randint(-7 if signed_v else 1, 8, (B, Lk, H * hd), generator=g).float()
    assert all(_is_bf16(t) for t in (q, k, v))
    return q, k, v


def transposed_index(bucket, h, H):
    """the (bucket', head') a transposed flat index h * N_BUCKETS + bucket lands on in the (N_BUCKETS, H) table"""
    f = h * N_BUCKETS + bucket
    return f // H, f % H


@functools.lru_cache(maxsize=4)
def bias_table(H, seed=5):
    """(N_BUCKETS, H) fp32 integers in [-2, 2]: entry (b, h) differs from every other head's entry of bucket b and from the entry the transposed
    index fetches -- a greedy colouring: an entry has at most H - 1 + 2 <= 4 constraints (H <= 3) and five values to choose from"""
    assert H <= 3
    g = torch.Generator().manual_seed(seed)
    entries = [(b, h) for b in range(N_BUCKETS) for h in range(H)]
    tab = torch.full((N_BUCKETS, H), float("nan"))                                           # NaN: not chosen yet, equal to nothing
    for b, h in entries:
        rivals = [(b, o) for o in range(H) if o != h] + [transposed_index(b, h, H)] + [e for e in entries if transposed_index(*e, H) == (b, h)]
        banned = {float(tab[e]) for e in rivals if e != (b, h)}
        free = [x for x in (-2.0, -1.0, 0.0, 1.0, 2.0) if x not in banned]
        tab[b, h] = free[int(torch.randint(0, len(free), (1,), generator=g))]
    return tab


def _heads(x, H):
    B, L, D = x.shape
    return x.view(B, L, H, D // H).permute(0, 2, 1, 3)


def _merge(x):
    B, H, L, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, L, H * hd)


def key_mask(B, Lk, valid):
    """int32 (B, Lk), the first valid[b] keys of batch element b unmasked; None for no mask"""
    if valid is None:
        return None
    m = torch.zeros(B, Lk, dtype=torch.int32)
    for b in range(B):
        m[b, :valid[b]] = 1
    return m


def bucket_of(Lq, Lk):
    from scail_amd.umt5 import relative_position_bucket
    return relative_position_bucket(Lq, Lk, N_BUCKETS)


def small_reference(q, k, v, H, scale, bucket=None, tab=None, mask=None, real_scale=False):
    """fp64 softmax attention of scail_attn_small on exact operands and its budget (module docstring).  Asserts integer scores (an exact scale) or
    sum|q k| <= 4 (the real scale).  Returns dict(ref, budget, A, x_min) with (B, Lq, H hd) fp64 tensors."""
    B, Lq, D = q.shape
    Lk, hd = k.shape[1], D // H
    qh, kh, vh = _heads(q.double(), H), _heads(k.double(), H), _heads(v.double(), H)
    s = qh @ kh.transpose(-1, -2) * scale
    E = 0.0
    if real_scale:
        assert float((qh.abs() @ kh.abs().transpose(-1, -2)).max()) <= 4 and float(qh.abs().max()) <= 1
        E = (hd + 1) * 4 * scale                                                             # in units of u
    if tab is not None:
        s = s + tab.double()[bucket.long()].permute(2, 0, 1)[None]
    if not real_scale:
        assert bool((s == s.round()).all()), "scores are integers"
    if mask is not None:
        assert bool((mask.sum(-1) >= 1).all()), "a fully masked row is outside the kernel's precondition"
        s = s.masked_fill(mask.view(B, 1, 1, Lk) == 0, float("-inf"))
    x = s - s.amax(-1, keepdim=True)
    p = torch.exp(x)
    w = p / p.sum(-1, keepdim=True)
    xa = x.abs().masked_fill(p == 0, 0.0)                                                    # masked keys: P = 0 exactly
    e = (2 * xa + 2 + (2 * E + xa if real_scale else 0.0)).masked_fill(p == 0, 0.0)
    ref = w @ vh
    A = w @ vh.abs()
    WE = (w * e).sum(-1, keepdim=True)
    first = (w * e) @ vh.abs() + Lk * A + ref.abs() * (WE + (Lk + 63) // 64 + 6 + 2)
    budget = SLACK * U * first
    one = (mask.sum(-1) == 1) if mask is not None else torch.full((B,), Lk == 1)
    budget[one] = 0.0                                                                        # one unmasked key: its v row, bit for bit
    return dict(ref=_merge(ref).contiguous(), budget=_merge(budget).contiguous(), A=_merge(A).contiguous(), x_min=float(x[p > 0].min()))


def attn_small_fp32(q, k, v, H, scale, bucket=None, tab=None, mask=None, fault=None):
    """attn_small_kernel's chain in IEEE fp32 (torch on the CPU).  Seeded faults: bias_transposed (the table read at h * buckets + bucket: another
    head's column), mask_batch0 (batch 0's mask for every batch element), keys_ge64_dropped (the lane loop's first trip only), pv_last_key (the last
    key missing from P . V), prev_row_q (the previous row's Q), sum_2m8, truncated"""
    f32 = torch.float32
    B, Lq, D = q.shape
    Lk, hd = k.shape[1], D // H
    Q = _heads(q.float(), H) * torch.tensor(scale, dtype=f32)
    if fault == "prev_row_q":
        Q = torch.cat([Q[:, :, :1], Q[:, :, :-1]], 2)
    kh, vh = _heads(k.float(), H), _heads(v.float(), H)
    s = Q @ kh.transpose(-1, -2)
    if tab is not None:
        bl = bucket.long()
        if fault == "bias_transposed":
            bias = torch.stack([tab.flatten()[h * N_BUCKETS + bl] for h in range(H)])
        else:
            bias = tab[bl].permute(2, 0, 1)
        s = s + bias[None]
    if mask is not None:
        mk = mask[:1].expand(B, -1) if fault == "mask_batch0" else mask
        s = s.masked_fill(mk.view(B, 1, 1, Lk) == 0, float("-inf"))
    if fault == "keys_ge64_dropped":
        s[..., 64:] = float("-inf")
    mx = s.amax(-1, keepdim=True)
    P = torch.exp2((s - mx) * torch.tensor(LOG2E, dtype=f32))
    trips = (Lk + 63) // 64
    pl = torch.cat([P, torch.zeros(B, H, Lq, trips * 64 - Lk)], -1).view(B, H, Lq, trips, 64)
    w = torch.zeros(B, H, Lq, 64, dtype=f32)
    for t in range(trips):
        w = w + pl[..., t, :]
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lane ^ o]
    total = w[..., :1]
    if fault == "sum_2m8":
        total = total * (1 + 2.0 ** -8)
    acc = torch.zeros(B, H, Lq, hd, dtype=f32)
    for j in range(Lk - 1 if fault == "pv_last_key" else Lk):
        acc = acc + P[..., j:j + 1] * vh[:, :, j:j + 1, :]
    y = _merge(acc * (1.0 / total))
    return (truncate_bf16(y.double()).float() if fault == "truncated" else y).to(BF16)


# ---- the cases of tests/test_softmax_exact_gpu.py (the CPU file checks the conditions on their inputs) ---------------------------------------------
def _a(id, B, H, Lq, Lk, hd, scale=1.0, bias=False, valid=None, real_scale=False):
    """scale: 1.0, 0.125 (q holds +-8) or the real 80^-1/2; valid: unmasked keys per batch element (None: no mask); v is signed where Lk <= 65"""
    return dict(id=id, B=B, H=H, Lq=Lq, Lk=Lk, hd=hd, scale=scale, bias=bias, valid=valid, real_scale=real_scale, signed_v=Lk <= 65)


A_CASES = [
    _a("umt5-130", 2, 3, 130, 130, 64, bias=True, valid=[130, 70]),
    _a("umt5-512", 1, 2, 512, 512, 64, bias=True, valid=[300]),
    _a("uncond-512", 1, 2, 512, 512, 64, bias=True, valid=[1]),
    _a("clip-257", 2, 2, 257, 257, 80, scale=0.125),
    _a("clip-257-real-scale", 2, 2, 257, 257, 80, scale=REAL_SCALE_80, real_scale=True),
    _a("hd128-297", 1, 2, 33, 297, 128),
    _a("bucket-5x65", 2, 3, 5, 65, 64, bias=True, valid=[65, 40]),
] + [_a(f"edge-{Lq}x{Lk}", 2, 2, Lq, Lk, 64, valid=None if Lk == 1 else [Lk, Lk - 3]) for Lk in (1, 63, 64, 65) for Lq in (1, 33)]
KINDS = ("sparse_q", "sparse_k")
LDS_REFUSED = dict(B=1, H=2, Lq=33, Lk=298, hd=128)                                          # 544 * 298 + 2048 > 163 840


def lds_bytes(Lk, hd):
    """the dynamic LDS of one attn_small workgroup (scail_attn_small in csrc/rowops.hip)"""
    return Lk * (hd + 8) * 2 + Lk * hd * 2 + 4 * Lk * 4 + 4 * hd * 4


@functools.lru_cache(maxsize=4)
def _small_case(id, kind):
    c = next(x for x in A_CASES if x["id"] == id)
    q, k, v = small_qkv(kind, c["B"], c["H"], c["Lq"], c["Lk"], c["hd"], seed_of(c) + KINDS.index(kind), qmag=8.0 if c["scale"] == 0.125 else 1.0,
                        signed_v=c["signed_v"])
    bucket = bucket_of(c["Lq"], c["Lk"]) if c["bias"] else None
    tab = bias_table(c["H"]) if c["bias"] else None
    mask = key_mask(c["B"], c["Lk"], c["valid"])
    r = small_reference(q, k, v, c["H"], c["scale"], bucket, tab, mask, c["real_scale"])
    return dict(q=q, k=k, v=v, bucket=bucket, tab=tab, mask=mask, r=r)


def small_case(case, kind):
    """operands and the reference dict of a case: computed once, shared, never modified"""
    return _small_case(case["id"], kind)
