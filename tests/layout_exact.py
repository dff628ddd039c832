"""Exact references for the token, sampler and layout kernels (tests/test_layout_exact_cpu.py, tests/test_layout_exact_gpu.py): scail_patchify,
scail_patchify_chars, scail_unpatchify, scail_f32_to_bf16, scail_bf16_to_f32, scail_timestep_embedding, scail_adaln_table, scail_cfg_euler,
scail_transpose2d, scail_to_channels_last / scail_from_channels_last and their _frames forms, scail_slabs_to_rows.  All of them are pure data movement,
where a wrong index is a wrong bit, or one to four fp32 operations: every reference here is exact and every check is on BITS.  No tolerance anywhere.

How a GPU case is held.  The CPU builds the whole buffer the kernel writes into, sentinel included (bf16 0x7fc0 / fp32 0x7fc0a5a5, both NaNs), as an
integer tensor of bit patterns: `before`, and what it must look like afterwards: `want`, or a list of candidates where the language allows more than
one result.  check_buffer() asserts that every word outside the result kept its bits and that every word inside equals (one of) the reference(s).

1. Data movement (patchify, patchify_chars, unpatchify, transpose2d, slabs_to_rows, bf16 -> fp32).  The inputs are PERMUTATION inputs: every element
   of every source of a case is a distinct bf16 bit pattern (patterns(): all 65 536 without the NaNs, +0.0, -0.0 and 1.0, the values the mask and the
   padding use; fp32 sources hold them exactly), so equal bits prove the index map element by element.  The references are torch indexing statements
   of the layouts of include/scail_hip.h: tokens [ref_0.. | noise | pose_0..], each (t h w) row-major, column 4 c + 2 p + q below 80, channels
   16 .. 19 the mask (1 on ref / pose tokens, 0 on noise tokens), columns 80 .. kpad zero; out[b, t, c, 2 h + p, 2 w + q] = tok[b, (t h w),
   32 p + 16 q + c] for unpatchify.
2. fp32 -> bf16 (scail_f32_to_bf16, the noise tokens of patchify, the channels-last store): round to nearest even as the integer formula on the bits,
   rne_bits(); the CPU file shows the formula equal to torch's .to(bfloat16) on every word the tests use.  A NaN word must come back as some NaN.
3. scail_timestep_embedding: [cos | sin] of a = t f_j in fp64, f_j = exp(-ln(1e4) j / half), rounded once to fp32; a trailing zero for odd dim.  The
   device's fp64 exp, log, cos and sin are not correctly rounded, so the kernel is held to "the RNE fp32 of some real within m of the reference".
   The issue's margin is m0 = 8 * 2^-52 (|a| + 1): a few double ulps on the frequency scale with the argument, a few on the result (|result| <= 1).
   Where the reference itself is tiny -- sin(a) for a small a, and sin(0) = 0 at t = 0 -- m0 spans many fp32 values and decides nothing; so the
   margin used is the same statement with the result's own magnitude in place of its bound 1:
       m = 8 * 2^-52 (|a| + |ref|) <= m0,       and m = 0 where a == 0 (sin(+0) = +0 and cos(0) = 1 exactly, C Annex F).
   An element is decided where rne32(ref - m) == rne32(ref + m); the CPU file asserts that EVERY element of every case is decided (cap 0), from the
   reference alone.  m <= m0, so this asks no less than the issue's rule.
4. scail_adaln_table: one fp32 addition, torch's on the CPU.  scail_from_channels_last: (x + b) * a cannot contract; fmaxf / fminf return their
   other argument for a NaN, so a NaN input comes out as lo: torch.fmin(torch.fmax(v, lo), hi).
5. scail_cfg_euler, x + ds * (vu + cfg * (vc - vu)), and scail_to_channels_last, bf16(x * a + b): the header lets their multiply-adds contract, so a
   result is one of four (two) candidates.  A fused multiply-add is computed without double rounding: the product of two fp32 values is exact in
   fp64, the sum with the fp32 addend is taken with its exact error term (two-sum) and the sticky bit is put into the fp64 sum's last place
   (round to odd), which makes the final rounding to fp32 the single correct one (53 >= 24 + 2 bits).  The CPU file proves fma32() against exact
   rationals, and that the fp64 sum rounded twice is NOT the same function on these inputs.

The module also restates each reference with the seeded faults that the CPU file wants rejected.  It reads nothing outside tests/ and scail_amd/."""
import fractions
import functools
import math

import numpy as np
import torch

BF16 = torch.bfloat16
SENT16 = 0x7FC0                                   # bf16 sentinel (a NaN)
SENT32 = 0x7FC0A5A5                               # fp32 sentinel (a NaN no bf16 widens to)
ONE16 = 0x3F80
BLOCK = 256


# ================================================================================================================================================
# bits
# ================================================================================================================================================
def words_of(x):
    """fp32 tensor -> int64 tensor of its words in [0, 2^32)"""
    assert x.dtype == torch.float32
    return x.contiguous().view(torch.int32).long() & 0xFFFFFFFF


def f32_of(w):
    """int64 words -> fp32 tensor"""
    w = w.long() & 0xFFFFFFFF
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).view(torch.float32)


def bits_of(x):
    """bf16 tensor -> int64 tensor of its bit patterns in [0, 65536)"""
    assert x.dtype == BF16
    return x.contiguous().view(torch.int16).long() & 0xFFFF


def bf16_of(b):
    """int64 bit patterns -> bf16 tensor"""
    b = b.long() & 0xFFFF
    return torch.where(b >= 2 ** 15, b - 2 ** 16, b).to(torch.int16).view(BF16)


def nan_word(w):
    return (w & 0x7FFFFFFF) > 0x7F800000


def nan_bits(b):
    return (b & 0x7FFF) > 0x7F80


def rne_bits(w):
    """round to nearest even, fp32 word -> bf16 bits, by the integer formula (not meaningful for NaN words)"""
    return ((w + 0x7FFF + ((w >> 16) & 1)) >> 16) & 0xFFFF


def trunc_bits(w):
    return (w >> 16) & 0xFFFF


@functools.lru_cache(maxsize=1)
def _all_patterns():
    p = torch.arange(65536)
    keep = ~nan_bits(p) & (p != 0) & (p != 0x8000) & (p != ONE16)
    return p[keep]


def patterns(counts, seed):
    """disjoint tensors of distinct bf16 bit patterns, one per entry of counts, in a seeded order"""
    pool = _all_patterns()
    assert sum(counts) <= pool.numel(), (counts, pool.numel())
    perm = pool[torch.randperm(pool.numel(), generator=torch.Generator().manual_seed(seed))]
    out, o = [], 0
    for n in counts:
        out.append(perm[o:o + n].clone())
        o += n
    return out


def all_distinct(*tensors):
    v = torch.cat([t.flatten() for t in tensors])
    return v.unique().numel() == v.numel()


def rounding_words(n, seed):
    """n general fp32 words for the rounding cases: for seeded bf16 patterns p the words (p << 16) + d, d in CONV_D (ties, both neighbours of ties,
    exact values), with every special first: fp32 denormals, the largest finite values (they round up to infinity), -0.0, +-inf; no NaN"""
    special = [0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x007FFFFF, 0x80000001, 0x80008000, 0x807F8000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000,
               0x7F7F7FFF, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000]
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(0, 65536, (n,), generator=g)
    d = torch.tensor(CONV_D)[torch.randint(0, len(CONV_D), (n,), generator=g)]
    w = (p << 16) + d
    w[:min(n, len(special))] = torch.tensor(special)[:n]
    w = torch.where(nan_word(w), w & 0x807FFFFF | 0x3F000000, w)           # a NaN word: the same fraction at exponent 126
    assert not bool(nan_word(w).any())
    return w


def check_buffer(got, before, inside, cands, what):
    """got, before, every candidate: integer tensors of bit patterns of one shape; inside: bool mask of the result.  Outside, every word kept its
    bits; inside, every word equals one of the candidates.  Returns how many words each candidate matches."""
    got, before = got.cpu().long(), before.long()
    assert got.shape == before.shape == inside.shape
    out = ~inside
    moved = out & (got != before)
    assert not bool(moved.any()), f"{what}: {int(moved.sum())} words outside the result were written; first at {tuple(int(v[0]) for v in moved.nonzero(as_tuple=True))}"
    ok = torch.zeros_like(inside)
    counts = []
    for c in cands:
        eq = inside & (got == c.long())
        counts.append(int(eq.sum()))
        ok |= eq
    bad = inside & ~ok
    if bool(bad.any()):
        i = tuple(int(v[0]) for v in bad.nonzero(as_tuple=True))
        raise AssertionError(f"{what}: {int(bad.sum())} of {int(inside.sum())} words differ from the reference; first at {i}: got {int(got[i]):#x}, "
                             f"want {' or '.join(f'{int(c[i]):#x}' for c in cands)}")
    return counts


def rejects(got, before, inside, cands):
    try:
        check_buffer(got, before, inside, cands, "")
    except AssertionError:
        return True
    return False


def framed(result, rows_after=1, cols_after=0, sentinel=SENT16):
    """the (..., R, C) result inside a sentinel-filled (..., R + rows_after, C + cols_after) buffer: (before, want, inside)"""
    *l, R, Cc = result.shape
    before = torch.full((*l, R + rows_after, Cc + cols_after), sentinel, dtype=torch.int64)
    inside = torch.zeros(before.shape, dtype=torch.bool)
    inside[..., :R, :Cc] = True
    want = before.clone()
    want[..., :R, :Cc] = result
    return before, want, inside


# ================================================================================================================================================
# 1. token assembly
# ================================================================================================================================================
def _p(id, H, W, T, B, n_ref, n_pose, kpad, n_char=1, rounding=False):
    return dict(id=id, H=H, W=W, T=T, B=B, n_ref=n_ref, n_pose=n_pose, kpad=kpad, n_char=n_char, rounding=rounding)


PATCHIFY_CASES = [
    _p("4x4x1-b1-k80", 4, 4, 1, 1, 1, 1, 80),
    _p("4x4x1-b3-BB-k88", 4, 4, 1, 3, 3, 3, 88),
    _p("8x12x3-b3-11-k128", 8, 12, 3, 3, 1, 1, 128),
    _p("8x12x3-b3-B1-k80", 8, 12, 3, 3, 3, 1, 80),
    _p("8x12x3-b3-1B-k88", 8, 12, 3, 3, 1, 3, 88),
    _p("8x12x3-b3-BB-k128", 8, 12, 3, 3, 3, 3, 128),
    _p("12x20x2-b1-k88", 12, 20, 2, 1, 1, 1, 88),
    _p("12x20x2-b3-BB-k128", 12, 20, 2, 3, 3, 3, 128),
    _p("12x20x2-b3-1B-k80", 12, 20, 2, 3, 1, 3, 80),
    _p("8x12x3-b3-B1-k88-rounding", 8, 12, 3, 3, 3, 1, 88, rounding=True),
]
CHARS_CASES = [
    _p("c1-4x4x1-b1-k80", 4, 4, 1, 1, 1, 1, 80, 1),
    _p("c1-8x12x3-b3-BB-k128", 8, 12, 3, 3, 3, 3, 128, 1),
    _p("c1-12x20x2-b3-1B-k88", 12, 20, 2, 3, 1, 3, 88, 1),
    _p("c2-4x4x1-b3-11-k128", 4, 4, 1, 3, 1, 1, 128, 2),
    _p("c2-8x12x3-b3-B1-k88", 8, 12, 3, 3, 3, 1, 88, 2),
    _p("c3-12x20x2-b1-k80", 12, 20, 2, 1, 1, 1, 80, 3),
    _p("c3-8x12x3-b3-BB-k128", 8, 12, 3, 3, 3, 3, 128, 3),
    _p("c2-8x12x3-b3-1B-k80-rounding", 8, 12, 3, 3, 1, 3, 80, 2, rounding=True),
]


def patchify_tokens(c):
    nc, T, H, W = c["n_char"], c["T"], c["H"], c["W"]
    return (nc + T) * (H // 2) * (W // 2) + nc * T * (H // 4) * (W // 4)


def patchify_threads(c):
    return c["B"] * patchify_tokens(c) * (c["kpad"] // 8)


@functools.lru_cache(maxsize=None)
def _patchify_inputs(id):
    c = next(x for x in PATCHIFY_CASES + CHARS_CASES if x["id"] == id)
    nc, T, H, W, B = c["n_char"], c["T"], c["H"], c["W"], c["B"]
    sx, sr, sp = (B, T, 16, H, W), (c["n_ref"], nc, 16, H, W), (c["n_pose"], nc * T, 16, H // 2, W // 2)
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(id))
    if c["rounding"]:
        r, p = patterns([math.prod(sr), math.prod(sp)], seed)
        xw = rounding_words(math.prod(sx), seed)
    else:
        r, p, xb = patterns([math.prod(sr), math.prod(sp), math.prod(sx)], seed)
        xw = xb << 16
    return dict(xw=xw.view(sx), ref=r.view(sr), pose=p.view(sp))


def patchify_inputs(c):
    """dict(xw: fp32 words (B, T, 16, H, W), ref: bf16 bits (n_ref, n_char, 16, H, W), pose: bf16 bits (n_pose, n_char T, 16, H/2, W/2)): computed
    once, shared, never modified"""
    return _patchify_inputs(c["id"])


def _patches(z, swap_pq=False):
    """(N, F, 16, h, w) -> (N, F (h/2) (w/2), 64): token (f, hh, ww), column 4 c + 2 p + q = element (c, 2 hh + p, 2 ww + q)"""
    N, F, C, h, w = z.shape
    z = z.reshape(N, F, C, h // 2, 2, w // 2, 2)                       # n f c hh p ww q
    z = z.permute(0, 1, 3, 5, 2, 6, 4) if swap_pq else z.permute(0, 1, 3, 5, 2, 4, 6)
    return z.reshape(N, F * (h // 2) * (w // 2), C * 4)


def patchify_reference(c, inp, fault=None):
    """(B, L, kpad) bf16 bits.  Seeded faults: pq_swapped, pose_w2 (the pose token's (hh, ww) taken with the row length of the noise tokens),
    ref_broadcast (batch 0's ref for every batch element), mask_on_noise, pad_nonzero, char_frame_swapped (the pose read as [T, n_char]), truncate"""
    nc, T, H, W, B, kpad = c["n_char"], c["T"], c["H"], c["W"], c["B"], c["kpad"]
    xw, ref, pose = inp["xw"], inp["ref"], inp["pose"]
    if fault == "ref_broadcast":
        ref = ref[:1]
    if fault == "char_frame_swapped":
        pose = pose.reshape(pose.shape[0], T, nc, *pose.shape[2:]).transpose(1, 2).reshape(pose.shape)
    ref, pose = ref.expand(B, -1, -1, -1, -1), pose.expand(B, -1, -1, -1, -1)
    xb = trunc_bits(xw) if fault == "truncate" else rne_bits(xw)
    sw = fault == "pq_swapped"
    t_ref, t_noise, t_pose = _patches(ref, sw), _patches(xb, sw), _patches(pose, sw)
    if fault == "pose_w2":
        h2, w2, h4, w4 = H // 2, W // 2, H // 4, W // 4
        rem, k = torch.arange(h4 * w4)[:, None], torch.arange(64)[None]
        hh, ww, ch, p, q = rem // w2, rem % w2, k // 4, (k // 2) % 2, k % 2
        addr = ((ch * h2 + 2 * hh + p) * w2 + 2 * ww + q) % (16 * h2 * w2)
        t_pose = pose.reshape(B, nc * T, 16 * h2 * w2)[:, :, addr].reshape(B, -1, 64)
    tok = torch.zeros(B, patchify_tokens(c), kpad, dtype=torch.int64)
    data = torch.cat([t_ref, t_noise, t_pose], 1)
    assert data.shape[1] == tok.shape[1]
    tok[:, :, :64] = data
    n0, n1 = t_ref.shape[1], t_ref.shape[1] + t_noise.shape[1]
    tok[:, :n0, 64:80] = ONE16
    tok[:, n1:, 64:80] = ONE16
    if fault == "mask_on_noise":
        tok[:, n0:n1, 64:80] = ONE16
    if fault == "pad_nonzero":
        tok[:, :, 80:81] = ONE16
    return tok


def patchify_model_view(c, inp):
    """the same inputs as the (B, F, 20, h, w) fp64 tensors oracle.scail_oracle.patch_embed takes (n_char == 1): the mask channels appended"""
    B, T, H, W = c["B"], c["T"], c["H"], c["W"]
    val = lambda bits: bf16_of(bits).double()
    x = val(rne_bits(inp["xw"]))
    ref, pose = val(inp["ref"]).expand(B, -1, -1, -1, -1), val(inp["pose"]).expand(B, -1, -1, -1, -1)
    one = lambda z: torch.ones(z.shape[0], z.shape[1], 4, z.shape[3], z.shape[4], dtype=torch.float64)
    return torch.cat([x, 0 * one(x)], 2), torch.cat([ref, one(ref)], 2), torch.cat([pose, one(pose)], 2)


UNPATCHIFY_CASES = [(B, T, H, W) for (T, H, W) in ((1, 2, 2), (3, 8, 12), (2, 6, 10)) for B in (1, 2)]


@functools.lru_cache(maxsize=None)
def unpatchify_tokens(B, T, H, W):
    n = B * T * (H // 2) * (W // 2) * 64
    return patterns([n], 77 + n)[0].view(B, T * (H // 2) * (W // 2), 64)


def unpatchify_reference(tok, B, T, H, W):
    """(B, T, 16, H, W) fp32 words: out[b, t, c, 2 h + p, 2 w + q] = tok[b, (t, h, w), 32 p + 16 q + c]"""
    z = tok.reshape(B, T, H // 2, W // 2, 2, 2, 16)                    # b t h w p q c
    return z.permute(0, 1, 6, 2, 4, 3, 5).reshape(B, T, 16, H, W) << 16


# ================================================================================================================================================
# 2. conversions
# ================================================================================================================================================
CONV_D = (0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF)
CONV_TAIL = 5                                       # the word counts are 65 536 + 5 and 6 * 65 536 + 5: off the block size
WRAPPER_N = (1, BLOCK * 3 + 5)


def all_bf16_patterns():
    return torch.cat([torch.arange(65536), torch.arange(CONV_TAIL) + 0x4000])


def all_conversion_words():
    p = torch.arange(65536)
    w = torch.cat([(p << 16) + d for d in CONV_D])
    return torch.cat([w, w[:CONV_TAIL] + 0x3F800001])


def check_f32_to_bf16(got_bits, w, what):
    """non-NaN words: the integer RNE formula, bit for bit; NaN words: some NaN.  Returns the number of denormal inputs and outputs checked."""
    got_bits = got_bits.cpu().long()
    nan = nan_word(w)
    want = rne_bits(w)
    bad = ~nan & (got_bits != want)
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        den = bad & ((w & 0x7F800000) == 0)
        raise AssertionError(f"{what}: {int(bad.sum())} words are not rounded to nearest even ({int(den.sum())} of them fp32 denormals); first: "
                             f"{int(w[i]):#010x} -> {int(got_bits[i]):#06x}, want {int(want[i]):#06x}")
    assert bool(nan_bits(got_bits[nan]).all()), f"{what}: a NaN word came back as a number"
    den_in = ~nan & ((w & 0x7F800000) == 0) & ((w & 0x7FFFFFFF) != 0)
    den_out = den_in & ((want & 0x7F80) == 0) & ((want & 0x7FFF) != 0)
    return int(den_in.sum()), int(den_out.sum())


# ================================================================================================================================================
# 3. sampler scalars
# ================================================================================================================================================
TS_DIMS = (256, 2, 6, 7, 300, 513)
TS_MARGIN_ULPS = 8
# steps of the 50-step schedule whose reference has an element within the margin of an fp32 rounding boundary (step 12: sin(t f_4) at dim 256; step
# 23: cos(t f_9); found from the reference alone, tests/test_layout_exact_cpu.py): replaced by the next fp32 value above, which has none
TS_REPLACED = (12, 23)


def sampler_timesteps():
    """the 50 timesteps of the sampler's default schedule (RFScaling: c_noise = 1000 sigma, in fp32 as RFSampler.sample_hip forms it)"""
    from scail_amd.sampler import make_flow_timesteps
    sig = make_flow_timesteps(0, 50)
    return torch.stack([sig[i] * 1000.0 for i in range(50)])


def timestep_values(n):
    if n == 1:
        return torch.tensor([1000.0])
    if n == 3:
        return torch.tensor([0.0, 1e-3, 999.999])
    assert n == 50
    t = sampler_timesteps()
    for i in TS_REPLACED:
        t[i] = torch.nextafter(t[i], torch.tensor(2000.0))
    return t


TS_CASES = [(dim, n) for dim in TS_DIMS for n in (1, 3, 50)]


def timestep_reference(t, dim, fault=None):
    """(ref fp64 (n, dim), margin fp64, issue's margin fp64).  Seeded faults: cos_sin_swapped, f32_frequency, j_over_dim, last_column"""
    half = dim // 2
    j = torch.arange(half, dtype=torch.float64)
    f = torch.exp(-math.log(10000.0) * j / (dim if fault == "j_over_dim" else half))
    if fault == "f32_frequency":
        f = f.float().double()
    a = t.float().double()[:, None] * f[None]
    parts = [torch.sin(a), torch.cos(a)] if fault == "cos_sin_swapped" else [torch.cos(a), torch.sin(a)]
    args = [a, a]
    if dim % 2:
        parts.append(torch.full_like(a[:, :1], 2.0 ** -30 if fault == "last_column" else 0.0))
        args.append(torch.zeros_like(a[:, :1]))
    ref, a = torch.cat(parts, 1), torch.cat(args, 1).abs()
    eps = TS_MARGIN_ULPS * 2.0 ** -52
    m = torch.where(a == 0, torch.zeros_like(a), eps * (a + ref.abs()))
    return ref, m, eps * (a + 1)


def timestep_decided(ref, m):
    lo, hi = words_of((ref - m).float()), words_of((ref + m).float())
    return (lo == hi) | ((ref - m).float() == (ref + m).float())       # (+0 and -0 are one value)


def check_timestep(got_words, ref, m, what):
    """every decided element is the RNE fp32 of the reference (as a value: the sign of a zero is not held); returns the number of undecided ones"""
    got = f32_of(got_words.cpu())
    dec = timestep_decided(ref, m)
    bad = dec & ~(got == ref.float())
    if bool(bad.any()):
        i = tuple(int(v[0]) for v in bad.nonzero(as_tuple=True))
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} elements are not the correctly rounded value; first at {i}: got {float(got[i])!r}, "
                             f"ref {float(ref[i])!r}")
    lo, hi = (ref - m).float(), (ref + m).float()
    assert bool(((got >= lo) & (got <= hi))[~dec].all()), f"{what}: an undecided element is outside its interval"
    return int((~dec).sum())


ADALN_CASES = [(1, 1, 1), (5, 2, 96), (3, 3, 100), (40, 2, 6 * 128)]


def adaln_inputs(layers, B, width):
    g = torch.Generator().manual_seed(layers * 1000 + width)
    return torch.randn(B, width, generator=g), torch.randn(layers, width, generator=g) * 3


# ---- fused multiply-add without double rounding ---------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """rne32(a * b + c) for fp32 numpy arrays of finite values: one rounding (module docstring, 5.)"""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    p = a * b                                                          # exact: 48 bits
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                                    # exact: s + err == p + c
    odd = (np.ascontiguousarray(s).view(np.int64) & 1) == 1
    toward = np.where(err > 0, np.inf, -np.inf)                        # the neighbour of s on err's side
    fix = (err != 0) & ~odd
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def fma32_exact(a, b, c):
    """the same for three Python floats holding fp32 values, with exact rationals"""
    v = fractions.Fraction(a) * fractions.Fraction(b) + fractions.Fraction(c)
    return round_fraction_f32(v)


def round_fraction_f32(v):
    """a Fraction in the normal range of fp32 -> the nearest fp32 (ties to even), as a Python float"""
    if v == 0:
        return 0.0
    s, v = (-1 if v < 0 else 1), abs(v)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if fractions.Fraction(2) ** e > v:
        e -= 1
    assert fractions.Fraction(2) ** e <= v < fractions.Fraction(2) ** (e + 1) and -126 <= e <= 127
    q = v / fractions.Fraction(2) ** (e - 23)                          # in [2^23, 2^24)
    n = q.numerator // q.denominator
    r = q - n
    if r > fractions.Fraction(1, 2) or (r == fractions.Fraction(1, 2) and n % 2 == 1):
        n += 1
    return s * float(n) * 2.0 ** (e - 23)


CFG, DSIGMA = np.float32(3.7), np.float32(-0.0371)
CFG_EULER_N = (1, 255, BLOCK * 5 + 17)
CFG_EULER_NAMES = ("separate", "inner fused", "outer fused", "both fused")


def cfg_euler_inputs(n):
    g = torch.Generator().manual_seed(4100 + n)
    return torch.randn(n, generator=g), torch.randn(2 * n, generator=g)


def cfg_euler_candidates(x, v, fault=None):
    """the four results of x + ds * (vu + cfg * (vc - vu)) in fp32, as int64 words, in the order of CFG_EULER_NAMES.  Seeded faults (one result):
    swapped (vc and vu), no_parentheses (cfg * vc - vu), fp64 (the whole expression in fp64, rounded once)"""
    n = x.numel()
    x, vu, vc = x.numpy(), v[:n].numpy(), v[n:].numpy()
    if fault == "swapped":
        vu, vc = vc, vu
    if fault == "fp64":
        r = x.astype(np.float64) + np.float64(DSIGMA) * (vu.astype(np.float64) + np.float64(CFG) * (vc.astype(np.float64) - vu.astype(np.float64)))
        return [words_of(torch.from_numpy(r.astype(np.float32)))]
    if fault == "no_parentheses":
        u = vu + (CFG * vc - vu)
        return [words_of(torch.from_numpy(x + DSIGMA * u))]
    d = vc - vu
    inner = (vu + CFG * d, fma32(CFG, d, vu))
    out = [x + DSIGMA * inner[0], x + DSIGMA * inner[1], fma32(DSIGMA, inner[0], x), fma32(DSIGMA, inner[1], x)]
    assert all(o.dtype == np.float32 for o in out)
    return [words_of(torch.from_numpy(o)) for o in out]


# ================================================================================================================================================
# 4. VAE layouts
# ================================================================================================================================================
TRANSPOSE_CASES = [(R, Cc, batch) for (R, Cc) in ((1, 1), (63, 65), (64, 64), (65, 130), (200, 96)) for batch in (1, 3)]


@functools.lru_cache(maxsize=None)
def transpose_input(R, Cc, batch):
    return patterns([batch * R * Cc], 31 * R + Cc + batch)[0].view(batch, R, Cc)


CL_SHAPES = ((16, 16), (3, 8), (12, 16))            # (C, Cpad); the way back reads rows of ldx = Cpad + 8 with sentinel columns from C on
CL_N = (1, 45, BLOCK * 2 + 3)
CL_AB = ((False, False), (True, False), (False, True), (True, True))
CL_CLAMPS = ((-0.75, 0.75), (-3.0e38, 3.0e38), (0.25, 0.25))
CL_NAMES = ("separate", "fused")


def cl_scale_shift(C, has_a, has_b):
    """general per-channel factors (no power of two) and shifts, fp32"""
    g = torch.Generator().manual_seed(50 + C)
    a = torch.rand(C, generator=g) * 1.7 + 0.31
    b = (1 + torch.rand(C, generator=g)) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()      # 1 <= |b| < 2
    return (a if has_a else None), (b if has_b else None)


CL_TIES = 64                                        # the first columns of every channel of a scale-and-shift input are tie inputs


def _tie_inputs(a, b, n, g):
    """(x (C, n) fp32, found): where found, rne32(x a) + b is EXACTLY a bf16 tie T = +-(257 + 2 j) 2^-17 (no rounding in the addition: |T| << |b|, and
    T is a multiple of the fp32 spacing at |b| < 4), which bf16 rounds to even, while the unrounded product x a is off rne32(x a) by up to half an fp32
    ulp at |b|, about 2^-16 |T|: the fused result is off the tie and bf16 rounds it to the side the product's error points to.  These are the
    elements on which a contracted and a separate x * a + b can differ after the rounding to bf16; random inputs have none in a few thousand."""
    C = a.numel()
    j = torch.randint(0, 128, (C, n), generator=g)
    sign = (torch.randint(0, 2, (C, n), generator=g) * 2 - 1).double()
    target = sign * (257 + 2 * j).double() * 2.0 ** -17 - b.double()[:, None]
    assert bool((target.float().double() == target).all())
    ad = a.double()[:, None]
    x0 = (target / ad).float()
    best, found = x0.clone(), torch.zeros(C, n, dtype=torch.bool)
    for k in (0, 1, -1, 2, -2):
        xk = f32_of(words_of(x0) + k)
        ok = ((xk.double() * ad).float().double() == target) & ~found
        best = torch.where(ok, xk, best)
        found |= ok
    return best, found


def cl_planar_input(C, N, a=None, b=None, seed=0):
    """(C, N) fp32: random normals; with both a scale and a shift the first CL_TIES columns are tie inputs for them (_tie_inputs)"""
    g = torch.Generator().manual_seed(600 + 7 * C + N + seed)
    x = torch.randn(C, N, generator=g) * 2.5
    if a is not None and b is not None:
        n = min(N, CL_TIES)
        t, found = _tie_inputs(a, b, n, g)
        x[:, :n] = torch.where(found, t, x[:, :n])
    return x


def to_channels_last_candidates(x, a, b, Cpad):
    """[separate, fused]: (N, Cpad) bf16 bits of bf16(x * a + b); pad channels +0"""
    C, N = x.shape
    av = (a if a is not None else torch.ones(C))[:, None].expand(C, N).contiguous().numpy()
    bv = (b if b is not None else torch.zeros(C))[:, None].expand(C, N).contiguous().numpy()
    xs = x.numpy()
    out = []
    for v in (xs * av + bv, fma32(xs, av, bv)):
        assert v.dtype == np.float32
        y = torch.zeros(N, Cpad, dtype=torch.int64)
        y[:, :C] = rne_bits(words_of(torch.from_numpy(v))).t()
        out.append(y)
    return out


def cl_rows_input(C, N, ldx):
    """(N, ldx) bf16 bits: random values with a NaN and both infinities among them in the first C columns, the sentinel from column C on"""
    g = torch.Generator().manual_seed(900 + 11 * C + N)
    x = bits_of((torch.randn(N, C, generator=g) * 1.5).to(BF16))
    flat = x.view(-1)
    for k, special in enumerate((0x7FC1, 0x7F80, 0xFF80, 0x8000)):
        if k * 7 + 2 < flat.numel():
            flat[k * 7 + 2] = special
    buf = torch.full((N, ldx), SENT16, dtype=torch.int64)
    buf[:, :C] = x
    return buf


def from_channels_last_reference(buf, C, a, b, lo, hi):
    """(C, N) fp32 words of clamp((x + b) * a, lo, hi) with fmaxf / fminf: a NaN comes out as lo"""
    x = bf16_of(buf[:, :C]).float().t().contiguous()
    v = (x + (b if b is not None else torch.zeros(C))[:, None]) * (a if a is not None else torch.ones(C))[:, None]
    y = torch.fmin(torch.fmax(v, torch.tensor(lo, dtype=torch.float32)), torch.tensor(hi, dtype=torch.float32))
    return words_of(y)


FRAMES_CASE = dict(C=12, Cpad=16, T=3, t0=1, n=1)
FRAMES_HW = (48, 45)                                # 48: plane, offset and window are multiples of 4 (float4 on the planar side); 45: dwords

# ================================================================================================================================================
# 5. scail_slabs_to_rows
# ================================================================================================================================================
SLAB_CASES = [(rows, D, w) for rows in (1, 37) for (D, w) in ((64, 8), (64, 16), (64, 64), (1536, 384))]
SLAB_GAP = 24                                       # sentinel elements between two slabs (a multiple of 8: 16-byte slabs)


@functools.lru_cache(maxsize=None)
def slab_input(rows, D, w):
    """(before: the (D / w, rows w + SLAB_GAP) slab buffer as bf16 bits, slabs: (D / w, rows, w))"""
    n = D // w
    slabs = patterns([rows * D], 13 * rows + D + w)[0].view(n, rows, w)
    buf = torch.full((n, rows * w + SLAB_GAP), SENT16, dtype=torch.int64)
    buf[:, :rows * w] = slabs.reshape(n, rows * w)
    return buf, slabs


def slab_reference(slabs):
    return torch.cat(list(slabs), 1)
