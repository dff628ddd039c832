"""Exact-arithmetic helpers for the attention tests (tests/test_attn_exact_cpu.py, tests/test_attn_exact_gpu.py); the rounding helpers and the
checker come from tests/gemm_exact.py and tests/conv_exact.py.

Operands.  Every attention kernel works in log2 units, p = exp2(s sl2 - m sl2), with sl2 = 1 for queries that arrive in log2 units
(SCAIL_ATTN_Q_PRESCALED).  The operands make every score q . k a small integer: "sparse_q" gives each query row (per head) 4 non-zeros +-1 at seeded
positions and keys dense in {-1, 0, 1}, "sparse_k" swaps the roles (so neither operand's fragment layout hides behind zeros); scores lie in [-4, 4];
v holds integers in [-7, 7].  The last 4 dimensions of every head are RESERVED: zero in every ordinary query row and key.  "Target" rows (TARGETS:
at least one in each of the four waves of a 256-row and of a 192-row workgroup) carry +1 there; a "spike" key carries c there and nothing else, so
it scores 4 c for the target rows and 0 for all others.  The sparse operand has one non-zero in each quarter of the ordinary dimensions and a target
row is zero on the upper two quarters: its ordinary scores lie in [-2, 2].
  c = 3 (+12, "spike"): at least 10 above the row's running maximum.  The 8-wave kernels rescale there.  scail_attn4_m16f and scail_attn4_x2 do NOT
      on their first pass: its reference point is the first tile's maximum + 40 (S_HEAD of asmgen/attn4.py, whatever the key count), the lazy check
      of the later tiles is relative to THAT, and +12 stays 28 below it -- the spike cases hold the optimistic pass exact with an outlier in it, and
      option attn4_thr changes nothing in them.
  c = 64 (+256, "restart"): the optimistic pass overflows, the workgroup restarts and runs the lazy-maximum loop, whose reference point is the
      running maximum (S_HEAD = 0).  THERE the rescale subroutine runs on rows that are held exactly: a restart case also has "lazy" rows (LAZY_ROWS,
      again one per wave of both heights, in the restarted workgroups) that carry (+1, -1, +1, -1) on the reserved dimensions -- orthogonal to the
      target rows' (+1, +1, +1, +1), so they score 0 on the restart key -- and a second spike key carrying 3 x (+1, -1, +1, -1): +12 for the lazy
      rows, 0 for everyone else.  "Riser" rows (RISER_ROWS) are zero on every ordinary dimension and carry (+1, +1, -1, -1), orthogonal to both;
      a third key, two tiles before the lazy rows', carries the same pattern: their scores are 0 everywhere and +4 there.  With attn4_thr 8 the
      subroutine fires on the lazy rows' waves at their key; with thr 2 also at the riser key; with thr 0 also wherever an ordinary row's maximum
      rises.  tests/test_attn_exact_cpu.py proves in the emulator that it executed each time.
Raw-scale callers: raw_scale() searches the fp32 `scale` for which the host's fl32(scale * fl32(log2 e)) is exactly 2^-3; q then holds +-8 instead
of +-1, so that s sl2 (hipcc kernels, per score) and bf16(sl2 q) (generated kernels, prologue) are the same integers.

Then s - M is an integer for every reference point M a kernel uses (running maximum, lazily raised maximum, first tile's maximum + 40), every p and
every alpha = exp2(m_old - m_new) is a power of two -- exact in fp32 and in the bf16 that feeds the P . V MFMA --, and the numerator sum p v and the
row sum l are sums of integers times ONE power of two.  reference() asserts, per row, 7 sum_j 2^(s_j - min_j s) < 2^24: every partial sum is exact
in fp32, in any order, for any MFMA shape and any tile split.  (Rows of a restart case that see the c = 64 spike are outside the bound: every other
key weighs less than 2^-240 of the spike, which underflows to 0 in fp32 and in the rescale of what was accumulated before it, so their exact answer
is the spike key's v row, bit for bit; reference() gives them that row and a budget of 0.)

What is left is o = bf16(acc (1 / l)): one division or v_rcp_f32, one product, one rounding.  The kernels are held to "correctly rounded wherever
fp32 arithmetic can decide it": rne(ref - B) <= o <= rne(ref + B), and where the two ends coincide the element is decided and must be that value
(check_interval_bf16: the rule of gemm_exact.check_budget_bf16 for an interval given by its two ends).  The share of undecided elements is a
condition on the INPUTS (at most UNDECIDED_CAP = 5 % per case, asserted on the CPU for the reference alone).

B, first-order absolute error bounds in units of u = 2^-24.  The hardware is expected to return exact powers of two from v_exp_f32 at integer
arguments, but nothing documents it, so B is built from the ISA manual's figures, the ones gemm_exact.py uses: v_exp_f32 and v_rcp_f32 1 ulp = 2 u,
the IEEE division 1.0f / l of csrc/attn.hip u (scail_amd/build.py compiles with -O3 only), a product u, a contraction only removes a rounding.
  weights: the weight of key j in the numerator and in l is one v_exp result p_j times one alpha = exp2(m_old - m_new) per LATER move of the row's
      reference point.  An alpha whose maximum did not move is exp2(+-0), which the ISA manual's functional examples give as exactly 1 (as they
      give exp2(-inf) = 0, on which the masks and the first tile rely); every kernel moves a row's reference point only in a tile in which the
      row's running maximum rises (flash_attn_swp_kernel and cross_attn2_kernel in each such tile, the lazy loops of the generated kernels in some
      of them, the optimistic loop never).  With R_j = the number of later 64-key tiles in which the row's running maximum rises (every
      segment's tiles counted), the weight carries c_j = 1 + R_j v_exp results: 2 c_j u relative.  With w_j = p_j / l:
      numerator 2 u sum_j c_j w_j |v_j| = 2 u AC,  denominator 2 u |ref| sum_j c_j w_j = 2 u |ref| LC;
  1 / l: v_rcp_f32 2 u |ref| (asmgen/attn4.py epilogue; the division's u is below it);  acc * inv: u |ref|.
  FIRST = 2 AC + (2 LC + 3) |ref|,  B = SLACK x FIRST x u, SLACK = 2 for the second-order terms.
  Where the maximum never moves after the first tile (LC = 1, AC = A = sum w |v|): 2 A + 5 |ref|; integer scores in [-4, 4] move it a few times at
  most, LC <= 2 or so.  A bf16 half ulp is 2^-9 |ref| = 32 768 u |ref|, so an element is undecided only where |ref| is small against A (bf16 is
  fine-grained near o ~ 0).
Two-step forms, every step monotone, so the lower and upper end are pushed through each step (check_interval_bf16, the same decision logic):
  accumulate: bf16(acc inv + o_old): ends ref1 -+ B1 + o_old, widened by the sum's rounding SLACK u |ref1 + o_old| (an fma has none);
  cross attention: bf16(bf16(O1) + O2): a1 in [rne(ref1 - B1), rne(ref1 + B1)], then a1 + ref2 -+ B2, widened by SLACK u |.| for the sum.
      A set of ONE key has O2 = its v row, an integer: bf16(O1) + integer is an exact tie of the coarser bf16 grid of the sum for 16 % of the
      elements (one to three dropped bits reading 1, 10 or 100), and a tie is undecided under any budget above zero.  The v row of a one-key set
      therefore keeps one element in four and is zero elsewhere, where the sum is bf16(O1) itself.
scail_attn_small (all scores zero, key mask): p = __expf(0) per unmasked key, c_j = 1: the one-tile budget on the mean of the unmasked v rows.

The module also restates each kernel family's chain with IEEE fp32 operations in torch (online_fp32: per-tile alpha / lazy threshold / first pass
at M + 40 with its restart into the lazy loop; cross_fp32 with the bf16 intermediate), with the seeded faults the CPU tests want rejected.

The module reads nothing outside tests/ and scail_amd/."""
import functools
import math

import numpy as np
import torch

import conv_exact
from conv_exact import BF16, U, _is_bf16, assert_bits, seed_of                                  # noqa: F401  (re-exported for the two test files)
from gemm_exact import rne_bf16, truncate_bf16

HD = 128
RES = 4                                    # reserved dimensions at the end of every head
QUARTER = (HD - RES) // 4                  # the sparse operand has one non-zero in each quarter of the ordinary dimensions
SLACK = 2.0
UNDECIDED_CAP = 0.05
TARGETS = (3, 70, 133, 150, 200)           # waves 0, 1, 2, 2, 3 of a 256-row workgroup; waves 0, 1, 2, 3 of a 192-row one and wave 0 of the next
LAZY_ROWS = (20, 90, 140, 170, 230)        # the same waves
LAZY_SIGNS = (1.0, -1.0, 1.0, -1.0)
RISER_ROWS = tuple(r + 5 for r in LAZY_ROWS)
RISER_SIGNS = (1.0, 1.0, -1.0, -1.0)       # orthogonal to the target rows' and to the lazy rows' pattern
RISER_BACK = 128                           # the riser key lies two tiles before the lazy key
SPIKE_C, RESTART_C = 3, 64
LOG2E_F32 = np.float32(1.4426950408889634)


# ---- operands -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def raw_scale():
    """the fp32 scale whose fl32(scale * fl32(log2 e)) -- the host's sl2 -- is exactly 2^-3: searched among the neighbours of 0.125 / log2(e)"""
    s = np.float32(0.125 / 1.4426950408889634)
    for _ in range(8):
        s = np.nextafter(s, np.float32(0))
    for _ in range(17):
        if np.float32(s * LOG2E_F32) == np.float32(0.125):
            return float(s)
        s = np.nextafter(s, np.float32(1))
    raise AssertionError("no fp32 scale gives sl2 = 2^-3")


def _sparse(rows, g, mag):
    """(rows, HD): 4 non-zeros +-mag, one at a seeded position in each quarter (QUARTER dimensions) of the ordinary dimensions"""
    pos = torch.randint(0, QUARTER, (rows, 4), generator=g) + torch.arange(4) * QUARTER
    sign = torch.randint(0, 2, (rows, 4), generator=g).float() * 2 - 1
    return torch.zeros(rows, HD).scatter_(1, pos, sign * mag)


def _dense(rows, g, mag):
    x = torch.randint(-1, 2, (rows, HD), generator=g).float() * mag
    x[:, HD - RES:] = 0
    return x


def exact_qkv(kind, B, H, Lq, Lk, seed, raw=False, spike=None, kv_batch=None, lazy_key=None):
    """q (B, Lq, H HD), k, v (kv_batch or B, Lk, H HD): fp32 tensors on the CPU (module docstring).  raw: q holds +-8 (for sl2 = 2^-3).
    spike = (key, c): the target rows (those below Lq) carry +1 (+8) on the reserved dimensions, key `key` of every batch element and head carries c;
    lazy_key: the lazy rows and their +12 key (module docstring)"""
    assert kind in ("sparse_q", "sparse_k")
    g = torch.Generator().manual_seed(seed)
    Bk = kv_batch or B
    qm = 8.0 if raw else 1.0
    q = (_sparse if kind == "sparse_q" else _dense)(B * Lq * H, g, qm).view(B, Lq, H * HD)
    k = (_dense if kind == "sparse_q" else _sparse)(Bk * Lk * H, g, 1.0).view(Bk, Lk, H * HD)
    v = torch.randint(-7, 8, (Bk, Lk, H * HD), generator=g).float()
    if spike is not None:
        key, c = spike
        rows = [r for r in TARGETS if r < Lq]
        assert rows and 0 <= key < Lk
        qv, kv = q.view(B, Lq, H, HD), k.view(Bk, Lk, H, HD)
        qv[:, rows, :, 2 * QUARTER:] = 0                                                     # ordinary scores of a target row: [-2, 2]
        qv[:, rows, :, HD - RES:] = qm
        kv[:, key] = 0
        kv[:, key, :, HD - RES:] = float(c)
    if lazy_key is not None:
        rows = [r for r in LAZY_ROWS if r < Lq]
        assert rows and spike is not None and 0 <= lazy_key < Lk and lazy_key != spike[0]
        qv, kv = q.view(B, Lq, H, HD), k.view(Bk, Lk, H, HD)
        qv[:, rows, :, 2 * QUARTER:] = 0
        qv[:, rows, :, HD - RES:] = torch.tensor(LAZY_SIGNS) * qm
        kv[:, lazy_key] = 0
        kv[:, lazy_key, :, HD - RES:] = torch.tensor(LAZY_SIGNS) * SPIKE_C
        rows, rkey = [r for r in RISER_ROWS if r < Lq], lazy_key - RISER_BACK
        assert rows and 64 <= rkey != spike[0]
        qv[:, rows] = 0                                                                      # ordinary scores of a riser row: 0
        qv[:, rows, :, HD - RES:] = torch.tensor(RISER_SIGNS) * qm
        kv[:, rkey] = 0
        kv[:, rkey, :, HD - RES:] = torch.tensor(RISER_SIGNS)
    assert all(_is_bf16(t) for t in (q, k, v))
    return q, k, v


def _heads(x, H):
    B, L, D = x.shape
    return x.view(B, L, H, HD).permute(0, 2, 1, 3)


def _merge(x):
    B, H, L, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, L, H * HD)


def tile_of_keys(Ls, n_seg=1):
    """the 64-key tile index of every key of n_seg segments of Ls keys, and the number of tiles"""
    tps = (Ls + 63) // 64
    t = torch.arange(Ls) // 64
    return torch.cat([t + s * tps for s in range(n_seg)]), tps * n_seg


# ---- references ---------------------------------------------------------------------------------------------------------------
def reference(q, k, v, H, sl2=1.0, n_seg=1, restart_key=None):
    """fp64 softmax attention in log2 units on exact operands: p = 2^(s - max), o = (p @ v) / sum p.  k, v: (B | 1, n_seg * Ls, H HD), the segments
    one behind the other.  Asserts that the scores are integers and the exactness bound of every row (module docstring); restart_key: the key
    that carries the c = 64 spike -- the target rows get its v row and a budget of 0.  Returns dict(ref, budget, A) of (B, Lq, H HD) fp64 tensors."""
    B, Lq, _ = q.shape
    Lk = k.shape[1]
    qh, kh, vh = _heads(q.double(), H), _heads(k.double(), H), _heads(v.double(), H)
    s = qh @ kh.transpose(-1, -2) * sl2                                                      # (B, H, Lq, Lk), broadcast over a shared K / V
    assert bool((s == s.round()).all()), "scores are integers"
    span = s - s.amin(-1, keepdim=True)
    rows_ok = 7 * torch.exp2(span).sum(-1) < 2 ** 24
    hot = torch.zeros(Lq, dtype=torch.bool)
    if restart_key is not None:
        hot[[r for r in TARGETS if r < Lq]] = True
        top2 = s[:, :, hot].topk(2, dim=-1).values
        assert bool((s[:, :, hot].argmax(-1) == restart_key).all()) and bool((top2[..., 0] - top2[..., 1] >= 240).all()), "the spike outweighs everything by 2^240"
    assert bool(rows_ok[:, :, ~hot].all()), "exactness bound: 7 sum 2^(s - min s) < 2^24 in every row"
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    tile, T = tile_of_keys(Lk // n_seg, n_seg)
    run = torch.stack([s[..., tile == t].amax(-1) for t in range(T)], -1).cummax(-1).values       # the running maximum after every tile
    inc = torch.cat([torch.zeros_like(run[..., :1]), (run[..., 1:] > run[..., :-1]).double()], -1)
    later = inc.flip(-1).cumsum(-1).flip(-1) - inc                                            # R: rises in the tiles after tile t
    c = 1 + later[..., tile]
    ref = (p @ vh) / l
    A = (p @ vh.abs()) / l
    AC = ((p * c) @ vh.abs()) / l
    LC = (p * c).sum(-1, keepdim=True) / l
    budget = SLACK * U * (2 * AC + (2 * LC + 3) * ref.abs())
    if restart_key is not None:
        ref[:, :, hot] = vh[:, :, restart_key].unsqueeze(2).expand(ref.shape[0], -1, int(hot.sum()), -1)
        budget[:, :, hot] = 0
    return dict(ref=_merge(ref).contiguous(), budget=_merge(budget).contiguous(), A=_merge(A).contiguous(), span_max=float(span[:, :, ~hot].max()))


def accumulate_bounds(r, old):
    """(ref, lo, hi) of bf16(acc inv + o_old)"""
    ref = r["ref"] + old.double()
    w = r["budget"] + SLACK * U * ref.abs()
    return ref, ref - w, ref + w


def cross_bounds(r1, r2):
    """(ref, lo, hi) of bf16(bf16(O1) + O2): the ends of the first rounding pushed through the sum"""
    ref = rne_bf16(r1["ref"]) + r2["ref"]
    lo = rne_bf16(r1["ref"] - r1["budget"]) + r2["ref"] - r2["budget"]
    hi = rne_bf16(r1["ref"] + r1["budget"]) + r2["ref"] + r2["budget"]
    return ref, lo - SLACK * U * lo.abs(), hi + SLACK * U * hi.abs()


def small_reference(v, heads, hd, valid):
    """scail_attn_small with all scores zero: the mean of the first valid[b] v rows; v (B, Lk, heads hd), valid: list of counts"""
    B, Lk, D = v.shape
    ref = torch.stack([v[b, :valid[b]].double().mean(0) for b in range(B)])
    A = torch.stack([v[b, :valid[b]].double().abs().mean(0) for b in range(B)])
    assert 7 * max(valid) < 2 ** 24
    return dict(ref=ref, budget=SLACK * U * (2 * A + 5 * ref.abs()))


# ---- checker ------------------------------------------------------------------------------------------------------------------
def check_interval_bf16(got, ref64, lo64, hi64, what=""):
    """gemm_exact.check_budget_bf16 for an interval that is not symmetric about the reference (the two-step forms): rne(lo) <= got <= rne(hi)
    everywhere; returns the undecided share, prints the same three figures, raises AssertionError.  check() goes through it too."""
    assert got.dtype == BF16 and got.shape == ref64.shape == lo64.shape == hi64.shape and ref64.dtype == torch.float64
    g = got.double().cpu()
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite output"
    assert bool((lo64 <= ref64).all() and (ref64 <= hi64).all())
    lo, hi = rne_bf16(lo64), rne_bf16(hi64)
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
        raise AssertionError(f"{what}: {int((~inside).sum())} elements are outside [rne(lo), rne(hi)]; first at {i}: got {float(g.flatten()[i])!r}, "
                             f"ref {float(ref64.flatten()[i])!r}")
    return share


def undecided_share(lo64, hi64):
    return float((rne_bf16(lo64) != rne_bf16(hi64)).double().mean())


def decided(lo64, hi64):
    return rne_bf16(lo64) == rne_bf16(hi64)


def check(got, r, what=""):
    """a one-step result against reference()'s dict"""
    return check_interval_bf16(got, r["ref"], r["ref"] - r["budget"], r["ref"] + r["budget"], what)


# ---- the kernels' chains restated with IEEE fp32 operations (torch on the CPU) -----------------------------------------------------------
def transpose_v_perm(n):
    """scail_transpose_v: position p of the padded key axis holds key (p with bits 2 and 3 swapped)"""
    p = torch.arange(n)
    return (p & ~12) | (((p >> 3) & 1) << 2) | (((p >> 2) & 1) << 3)


def transpose_v_ref(v, H):
    """the V^T image (B, H, HD, ceil64(Lk)) bf16 of v (B, Lk, H HD): keys permuted inside each group of 16, zero padding"""
    B, Lk, _ = v.shape
    Lkp = (Lk + 63) // 64 * 64
    key = transpose_v_perm(Lkp)
    ok = key < Lk
    out = torch.zeros(B, H, HD, Lkp, dtype=BF16)
    out[:, :, :, ok] = _heads(v.to(BF16), H).transpose(-1, -2)[:, :, :, key[ok]]
    return out


def _bf(x):
    return x.to(BF16).float()


def online_fp32(q, k, v, H, sl2=1.0, n_seg=1, mode="tile", thr=8.0, old=None, fault=None, rows=256, final=True, fault_tile=None):
    """One kernel family's chain in IEEE fp32: 64-key tiles (every segment's last tile ragged, its padded keys masked with -inf), P rounded to bf16 for
    P . V, o = bf16(acc * (1 / l) [+ old]).
    mode "tile": flash_attn_swp_kernel / cross_attn2_kernel -- running maximum, alpha = exp2((m_old - m_new) sl2) for l every tile, l summed from the
        unrounded p;
    mode "lazy": the generated kernels' loop after a restart -- the reference point rises (to the running maximum) only where a tile's maximum
        exceeds it by more than thr; p up to 2^thr; l summed from the bf16 p (matrix pipe);
    mode "opt": the generated kernels as launched -- the first tile puts the reference point at its maximum + 40 and it stays there (the hot loop
        tracks no maximum; the remainder tiles check theirs against THAT point, which only a score more than 40 + thr above the first tile's
        maximum passes: none of the exact operands has one outside the hot loop); a workgroup (`rows` query rows) with a non-finite or zero row
        sum runs again in mode "lazy".  Returns (o, restarted workgroups per (batch, head)) in this mode.
    fault: a seeded fault (tests/test_attn_exact_cpu.py).  final=False returns the fp32 acc * inv without the rounding (cross_fp32)."""
    B, Lq, _ = q.shape
    Lk = k.shape[1]
    Ls = Lk // n_seg
    f32 = torch.float32
    qh, kh, vh = _heads(q.float(), H), _heads(k.float(), H), _heads(v.float(), H)
    sl2f = torch.tensor(sl2, dtype=f32)
    if fault == "scale_twice":
        sl2f = sl2f * sl2f
    if fault == "scale_missing":
        sl2f = torch.tensor(1.0)
    if fault == "v_unpermuted":                                                              # V^T read as if scail_transpose_v had not swapped bits 2 and 3
        n = Lk // 16 * 16
        vh = torch.cat([vh[:, :, transpose_v_perm(n)], vh[:, :, n:]], 2)
    acc = torch.zeros(B, H, Lq, HD, dtype=f32)
    l = torch.zeros(B, H, Lq, 1, dtype=f32)
    m = torch.full((B, H, Lq, 1), float("-inf"), dtype=f32)
    tiles = [(sg, t0) for sg in range(n_seg) for t0 in range(0, Ls, 64)]
    for ti, (sg, t0) in enumerate(tiles):
        if (fault == "drop_tile" and ti == len(tiles) // 2) or (fault == "skip_segment" and sg == 1):
            continue
        n = min(64, Ls - t0)
        ks, vs = kh[:, :, sg * Ls + t0:sg * Ls + t0 + n], vh[:, :, sg * Ls + t0:sg * Ls + t0 + n]
        s = qh @ ks.transpose(-1, -2)                                                        # exact integers (times 8 for raw-scale queries)
        if fault == "pad_counted" and n < 64:
            s = torch.cat([s, torch.zeros(*s.shape[:-1], 64 - n)], -1)
            vs = torch.cat([vs, torch.zeros(*vs.shape[:-2], 64 - n, HD)], -2)
        mx = s.amax(-1, keepdim=True)
        if mode == "tile":
            m_new = torch.maximum(m, mx)
        elif mode == "lazy":
            m_new = torch.where((ti == 0) | (mx * sl2f > m * sl2f + thr), torch.maximum(m, mx), m)
        else:
            m_new = mx + 40.0 / sl2f if ti == 0 else m
        alpha = torch.exp2((m - m_new) * sl2f)
        p = torch.exp2(s * sl2f - m_new * sl2f)
        if fault == "weight_doubled" and ti == 0:
            p[..., 5] *= 2
        l = l * alpha + (p if mode == "tile" else _bf(p)).sum(-1, keepdim=True)
        if not (fault == "no_o_rescale" and ti == fault_tile):
            acc = acc * alpha
        acc = acc + _bf(p) @ vs
        m = m_new
    if fault == "l_2m8":
        l = l * (1 + 2.0 ** -8)
    if fault == "l_5pc":
        l = l * 1.05
    restarted = None
    if mode == "opt":
        restarted = torch.zeros(B, H, dtype=torch.int64)
        bad = ~torch.isfinite(l) | (l == 0) | ~torch.isfinite(acc).all(-1, keepdim=True)
        if bool(bad.any()):
            again = online_fp32(q, k, v, H, sl2, n_seg, "lazy", thr, final=False)
            y = acc * (1.0 / l)
            for r0 in range(0, Lq, rows):
                wg = bad[:, :, r0:r0 + rows].any(2).squeeze(-1)                              # (B, H)
                restarted += wg.long()
                y[:, :, r0:r0 + rows] = torch.where(wg[:, :, None, None], _heads(again, H)[:, :, r0:r0 + rows], y[:, :, r0:r0 + rows])
            y = _merge(y)
        else:
            y = _merge(acc * (1.0 / l))
    else:
        y = _merge(acc * (1.0 / l))
    if not final:
        return y
    if old is not None:
        if fault == "old_ignored":
            pass
        elif fault == "old_after_rounding":
            y = _bf(y) + old.float()
        else:
            y = y + old.float()
    out = truncate_bf16(y.double()).float().to(BF16) if fault == "truncated" else y.to(BF16)
    return (out, restarted) if mode == "opt" else out


def cross_fp32(q, k1, v1, k2, v2, H, sl2=1.0, mode="tile", fault=None):
    """bf16(bf16(O1) + O2) with both sets through online_fp32 (cross_attn2_kernel: mode "tile"; scail_attn4_x2: "lazy")"""
    B = q.shape[0]
    o1 = online_fp32(q, k1.expand(B, -1, -1), v1.expand(B, -1, -1), H, sl2, mode=mode, final=False)
    o2 = online_fp32(q, k2.expand(B, -1, -1), v2.expand(B, -1, -1), H, sl2, mode=mode, final=False)
    return ((o1 if fault == "set1_unrounded" else _bf(o1)) + o2).to(BF16)


# ---- the cases of tests/test_attn_exact_gpu.py (the CPU file checks the conditions on their inputs and the routes) ------------------------------
def _c(id, B, H, Lq, Lk, kind="sparse_q", raw=False, form="plain", route=8, opts=None, n_seg=1, spike_key=None, lazy_key=None):
    """form: plain | accumulate | bcast (batch-broadcast K / V) | strided (q, k column views of a qkv buffer, o_rs with slack) | spike | restart;
    Lk: keys per segment; route: scail_flash_attn_kernel_for's answer under opts"""
    return dict(id=id, B=B, H=H, Lq=Lq, Lk=Lk, kind=kind, raw=raw, form=form, route=route, opts=opts or {}, n_seg=n_seg, spike_key=spike_key, lazy_key=lazy_key)


# the 8-wave kernel (product: flash_attn_swp_kernel<4, 4, 0, 1>; every variant of the measurement build)
W8_CASES = [
    _c("w8-one-key", 1, 1, 40, 1),                                                          # o = v exactly
    _c("w8-130x64", 2, 2, 130, 64), _c("w8-130x64-raw", 2, 2, 130, 64, "sparse_k", raw=True),
    _c("w8-300x65", 1, 2, 300, 65, "sparse_k"), _c("w8-300x65-acc", 1, 2, 300, 65, form="accumulate"),
    _c("w8-300x257", 2, 2, 300, 257), _c("w8-300x257-raw", 2, 2, 300, 257, raw=True), _c("w8-300x257-bcast", 2, 2, 300, 257, "sparse_k", form="bcast"),
    _c("w8-300x257-acc-raw", 2, 2, 300, 257, "sparse_k", raw=True, form="accumulate"), _c("w8-300x257-strided", 2, 2, 300, 257, form="strided"),
    _c("w8-256x512-attn4-off", 1, 1, 256, 512, opts={"attn4": 0}),
    _c("w8-seg-3x100", 1, 2, 130, 100, n_seg=3), _c("w8-spike", 2, 2, 300, 257, form="spike", spike_key=200),
]

# scail_attn4_m16f (route 4): every Lk, Lq and (B, H) of the issue once, both operand kinds, both scales, both heights
_LK, _LQ, _BH = (512, 576, 832, 1088, 513, 849), (256, 130, 300, 520), ((1, 1), (2, 2), (1, 3), (2, 4))
G4_CASES = [_c(f"g4-{Lq}x{Lk}-b{b}h{h}" + ("-raw" if i % 2 else ""), b, h, Lq, Lk, ("sparse_q", "sparse_k")[(i // 2) % 2], raw=bool(i % 2), route=4)
            for i, (Lk, Lq, (b, h)) in enumerate(zip(_LK, _LQ + _LQ[:2], _BH + _BH[2:]))] + [
    _c("g4-xcd-off", 2, 4, 300, 576, route=4, opts={"attn4_xcd": 0}),
    _c("g4-strided", 2, 2, 300, 513, "sparse_k", form="strided", route=4),
    _c("g4-seg-3x512", 1, 2, 200, 512, route=4, n_seg=3),
    _c("g4-spike-thr8", 1, 2, 300, 832, form="spike", route=4, spike_key=700), _c("g4-spike-thr0", 1, 2, 300, 832, form="spike", route=4, opts={"attn4_thr": 0}, spike_key=700),
    _c("g4-spike-thr2", 1, 2, 300, 832, "sparse_k", form="spike", route=4, opts={"attn4_thr": 2}, spike_key=700),
    # 11 tiles; restart key in tile 3, the lazy rows' +12 key in tile 8: the restarted workgroups run the lazy-maximum loop under each threshold
    _c("g4-restart-thr8", 1, 1, 300, 704, form="restart", route=4, spike_key=64 * 3 + 7, lazy_key=64 * 8 + 5),
    _c("g4-restart-thr0", 1, 2, 300, 704, "sparse_k", form="restart", route=4, opts={"attn4_thr": 0}, spike_key=64 * 3 + 7, lazy_key=64 * 8 + 5),
    _c("g4-restart-thr2", 1, 1, 300, 704, form="restart", route=4, opts={"attn4_thr": 2}, spike_key=64 * 3 + 7, lazy_key=64 * 8 + 5),
    # 9 and 12 pairs: XCD decode mode 2 (8 equal runs of the item list, padded grid)
    _c("g4-xcd2-b3h3", 3, 3, 300, 512, route=4), _c("g4-xcd2-b2h6-raw", 2, 6, 130, 513, "sparse_k", raw=True, route=4),
]
HEIGHTS = (256, 192)

# cross attention: (B, H, Lq, Lk1, Lk2, set 2 shared by the batch); route under option cross4 = 1 (cross4 = 0: cross_attn2_kernel, 2, for all)
X_CASES = [dict(id="x-300x512+257", B=2, H=2, Lq=300, Lk1=512, Lk2=257, shared2=True, route=4), dict(id="x-515x64+320", B=2, H=1, Lq=515, Lk1=64, Lk2=320, shared2=False, route=4),
           dict(id="x-128x77+1", B=1, H=3, Lq=128, Lk1=77, Lk2=1, shared2=False, route=2)]

OPTION_DEFAULTS = {"attn4": 1, "attn4_rows": 0, "attn4_xcd": 1, "attn4_cus": 0, "attn4_thr": 8, "cross4": 2}


def with_options(opts, fn):
    """fn() under the library options ``opts``; the defaults are back afterwards, whatever happens"""
    return conv_exact.with_options(opts, fn, OPTION_DEFAULTS)


def sl2_of(case_or_raw):
    raw = case_or_raw["raw"] if isinstance(case_or_raw, dict) else case_or_raw
    return 0.125 if raw else 1.0


@functools.lru_cache(maxsize=4)
def _self_case(id):
    c = next(x for x in W8_CASES + G4_CASES if x["id"] == id)
    spike = None if c["spike_key"] is None else (c["spike_key"], RESTART_C if c["form"] == "restart" else SPIKE_C)
    Bk = 1 if c["form"] == "bcast" else c["B"]
    q, k, v = exact_qkv(c["kind"], c["B"], c["H"], c["Lq"], c["Lk"] * c["n_seg"], seed_of(c), c["raw"], spike, kv_batch=Bk, lazy_key=c["lazy_key"])
    r = reference(q, k, v, c["H"], sl2_of(c), c["n_seg"], restart_key=c["spike_key"] if c["form"] == "restart" else None)
    old = None
    if c["form"] == "accumulate":
        old = torch.randint(-3, 4, q.shape, generator=torch.Generator().manual_seed(seed_of(c) + 1)).float()
        r["ref"], r["lo"], r["hi"] = accumulate_bounds(r, old)
    else:
        r["lo"], r["hi"] = r["ref"] - r["budget"], r["ref"] + r["budget"]
    return dict(q=q, k=k, v=v, old=old, r=r)


def self_case(case):
    """operands (q, k, v with the segments one behind the other, old) and the reference dict (ref, lo, hi, budget) of a case: computed once, shared,
    never modified"""
    return _self_case(case["id"])


@functools.lru_cache(maxsize=4)
def _cross_case(id, raw):
    c = next(x for x in X_CASES if x["id"] == id)
    kind = "sparse_k" if raw else "sparse_q"                                                 # one q for both sets, so both sets are of its kind
    q, k1, v1 = exact_qkv(kind, c["B"], c["H"], c["Lq"], c["Lk1"], seed_of(c) + raw, raw)
    _, k2, v2 = exact_qkv(kind, c["B"], c["H"], c["Lq"], c["Lk2"], seed_of(c) + 7 + raw, raw, kv_batch=1 if c["shared2"] else None)
    if c["Lk2"] == 1:                                                                        # (module docstring: exact ties of bf16(O1) + integer)
        v2 = v2 * (torch.rand(v2.shape, generator=torch.Generator().manual_seed(seed_of(c) + 11)) < 0.25).float()
    r1, r2 = reference(q, k1, v1, c["H"], sl2_of(raw)), reference(q, k2, v2, c["H"], sl2_of(raw))
    ref, lo, hi = cross_bounds(r1, r2)
    return dict(q=q, k1=k1, v1=v1, k2=k2, v2=v2, ref=ref, lo=lo, hi=hi)


def cross_case(case, raw):
    return _cross_case(case["id"], bool(raw))


def flash_route(q_rs, k_rs, o_rs, Lq, Lk, accumulate, prescaled):
    from scail_amd import lib as L
    return L.load().scail_flash_attn_kernel_for(q_rs, k_rs, o_rs, Lq, Lk, 1 if accumulate else 0, 1 if prescaled else 0)


def cross_route(q_rs, k1_rs, k2_rs, o_rs, Lq, Lk1, Lk2, B, H):
    from scail_amd import lib as L
    return L.load().scail_cross_attn2_kernel_for(q_rs, k1_rs, k2_rs, o_rs, Lq, Lk1, Lk2, B, H)


GEN, W8 = "scail_attn4_m16f", "flash_attn_swp_kernel<4, 4, 0, 1>"
X_GEN, X_HIP = "scail_attn4_x2", "cross_attn2_kernel"
# the measurement build's attn_variant codes that the GPU tests force (ATTN_VARIANTS there), by kernel
VARIANT_KERNELS = {2: "flash_attn_kernel<2, 8>", 258: "flash_attn_kernel<258, 8>", 66: "flash_attn_kernel<2, 4>", 8 | (1 << 12): "flash_attn_swp_kernel<5, 5>",
                   8 | (6 << 12): "flash_attn_swp_kernel<4, 4>"}


def kernel_name(q_rs, k_rs, o_rs, B, H, Lq, Lk, accumulate, prescaled, plan=False, agree=True):
    """what scail_flash_attn_kernel_name_for says the call runs under the options in force; scail_flash_attn_kernel_for must agree (agree=False:
    a grid the seven-argument query cannot see).  plan=True (needs the device unless option attn4_rows forces a height): (name, dict(n_launch,
    launches=[dict(rows, item0, n_items, xcd_mode)]))"""
    import ctypes as C
    from scail_amd import lib as L
    buf, pl = C.create_string_buffer(128), (C.c_int64 * 9)()
    L.call("scail_flash_attn_kernel_name_for", q_rs, k_rs, o_rs, B, H, Lq, Lk, 1 if accumulate else 0, 1 if prescaled else 0, buf, len(buf),
           C.cast(pl, C.c_void_p) if plan else None)
    name = buf.value.decode()
    if agree:
        assert flash_route(q_rs, k_rs, o_rs, Lq, Lk, accumulate, prescaled) == (4 if name.startswith("scail_attn4") else 8), name
    if not plan:
        return name
    launches = [dict(zip(("rows", "item0", "n_items", "xcd_mode"), pl[1 + 4 * i:5 + 4 * i])) for i in range(2)]
    assert pl[0] in (1, 2) and all(v == 0 for l in launches[pl[0]:] for v in l.values()), list(pl)
    return name, dict(n_launch=pl[0], launches=launches[:pl[0]])


def cross_kernel_name(q_rs, k1_rs, k2_rs, o_rs, Lq, Lk1, Lk2, B, H, want_grid=False):
    """what scail_cross_attn2_kernel_name_for says the call runs under the options in force (want_grid: (name, workgroups), which needs the device
    for the generated kernel); scail_cross_attn2_kernel_for must agree"""
    import ctypes as C
    from scail_amd import lib as L
    buf, wg = C.create_string_buffer(128), C.c_int64(-1)
    L.call("scail_cross_attn2_kernel_name_for", q_rs, k1_rs, k2_rs, o_rs, Lq, Lk1, Lk2, B, H, buf, len(buf), C.cast(C.byref(wg), C.c_void_p) if want_grid else None)
    name = buf.value.decode()
    assert cross_route(q_rs, k1_rs, k2_rs, o_rs, Lq, Lk1, Lk2, B, H) == {X_GEN: 4, X_HIP: 2}[name], name
    return (name, wg.value) if want_grid else name


def expected_name(case, rows=None, variant=None):
    """the name the queries must give for a case under its options: a self-attention case by its route -- rows: the generated kernel's launches, 256 / 192
    = one of that height, 448 = both, None = the base symbol (no plan asked for); variant: the attn_variant code the measurement build forces on the
    8-wave family -- and a cross-attention case by its route under option cross4 = 1"""
    if "Lk1" in case:
        return X_GEN if case["route"] == 4 else X_HIP
    if case["route"] == 8 or case["opts"].get("attn4", 1) == 0:
        return f"attn_variant {variant}: {VARIANT_KERNELS[variant]}" if variant in VARIANT_KERNELS else W8
    return {None: GEN, 256: GEN, 192: GEN + "_q3", 448: GEN + " + " + GEN + "_q3"}[rows]


def expected_xcd_mode(pairs, opts, n_launch=1):
    """the workgroup-id decode of a generated launch: plain below 8 (batch, head) pairs or under attn4_xcd = 0, pairs dealt round-robin for one launch
    of a multiple of 8 pairs, 8 runs of the item list otherwise"""
    if opts.get("attn4_xcd", 1) == 0 or pairs < 8:
        return 0
    return 1 if pairs % 8 == 0 and n_launch == 1 else 2


def strides_of(case):
    """(q_rs, k_rs, o_rs) of a case's call: the strided form takes q and k as column views of a qkv buffer and writes rows with 64 elements of slack"""
    D = case["H"] * HD
    return (3 * D, 3 * D, D + 64) if case["form"] == "strided" else (D, D, D)
