"""softmax_rows_kernel<4> / <16> and attn_small_kernel on operands for which their softmax is exact, or bounded by a derived budget, in fp32
(tests/softmax_exact.py): correctly rounded wherever fp32 arithmetic can decide it, inside the budget elsewhere.  scail_softmax_rows: on both sides of
every boundary of the kernel (8 columns per chunk, 2048 columns per register pass, MAXV 4 / 16 at 8192), with poisoned columns n .. ceil8(n) that must
come back as +0 and NaN slack that must stay.  scail_attn_small: live scores with the real bucket matrix, key masks, head_dim 64 / 80 / 128, the real
lengths (512 and 257 keys), Lq != Lk, one unmasked key, the LDS boundary of head_dim 128 (297 keys run, 298 are refused on the host), from column
views of NaN-filled fused buffers into NaN-filled outputs.  The VAE's mid-block attention around scail_softmax_rows at token counts that are no
multiple of 8: against the fp64 oracle, bit for bit independent of the next frame's keys, and the C executor bit for bit equal to the layer path.
tests/test_softmax_exact_cpu.py proves the inputs and the checker."""
import pytest
import torch

import softmax_exact as X

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from scail_amd import lib, ops as _ops
    lib.load()          # loud failure when the HIP library is missing
    assert torch.cuda.is_available()
    return _ops


def nan_buf(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=BF16)


def all_nan(t):
    return bool(torch.isnan(t.float()).all())


# ---- scail_softmax_rows -----------------------------------------------------------------------------------------------------------------------------
def _run_softmax(ops, r, n, scale, what):
    before = X.softmax_buffer(r["s"], n)
    buf = before.to(DEV)
    ops.softmax_rows_(buf, n, scale)
    torch.cuda.synchronize()
    return X.check_softmax_output(buf, before, r, n, what)


@pytest.mark.parametrize("n", X.SM_EXACT_N)
def test_softmax_rows_exact_regime(ops, n):
    """sl2 = 2^-3 and scores 8 k: every p is a power of two and the row sum is exact in any order; in effect bit for bit"""
    share = _run_softmax(ops, X.softmax_exact_reference(n), n, X.raw_scale(), f"softmax_rows exact n={n} MAXV={X.maxv_of(n)}")
    assert share <= X.UNDECIDED_CAP


@pytest.mark.parametrize("n,C", X.SM_GENERAL)
def test_softmax_rows_general_regime(ops, n, C):
    """the scale the VAE passes, random scores: inside the margin derived from the kernel's chain"""
    share = _run_softmax(ops, X.softmax_general_reference(n, C), n, X.vae_scale(C), f"softmax_rows general n={n} C={C}")
    assert share <= X.UNDECIDED_CAP


# ---- scail_attn_small -------------------------------------------------------------------------------------------------------------------------------
def _fused(q, k, v):
    """q, k, v as column views of NaN-filled fused buffers: one (B, L, 3 D) buffer where Lq = Lk (what umt5.py and clip.py pass), else q in the
    first column of its own buffer and k, v in the second and third of theirs"""
    D = q.shape[-1]
    kv = nan_buf(k.shape[0], k.shape[1], 3 * D)
    kv[..., D:2 * D], kv[..., 2 * D:] = k.to(BF16).to(DEV), v.to(BF16).to(DEV)
    qb = kv if q.shape[1] == k.shape[1] else nan_buf(q.shape[0], q.shape[1], 3 * D)
    qb[..., :D] = q.to(BF16).to(DEV)
    return qb[..., :D], kv[..., D:2 * D], kv[..., 2 * D:]


@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("case", X.A_CASES, ids=lambda c: c["id"])
def test_attn_small_live_scores(ops, case, kind):
    d = X.small_case(case, kind)
    r, B, Lq, D = d["r"], case["B"], case["Lq"], case["H"] * case["hd"]
    q, k, v = _fused(d["q"], d["k"], d["v"])
    obuf = nan_buf(B, Lq, D + 64)
    dev = lambda t: None if t is None else t.to(DEV)
    ops.attn_small(q, k, v, case["H"], scale=case["scale"], bucket=dev(d["bucket"]), bias_tab=dev(d["tab"]), key_mask=dev(d["mask"]), out=obuf[..., :D])
    torch.cuda.synchronize()
    assert all_nan(obuf[..., D:]), "the slack between output rows was written"
    o = obuf[..., :D].cpu()
    share = X.check_interval_bf16(o, r["ref"], r["ref"] - r["budget"], r["ref"] + r["budget"], f"attn_small {case['id']} {kind}")
    assert share <= X.UNDECIDED_CAP
    if case["valid"] is not None and 1 in case["valid"] or case["Lk"] == 1:                  # one unmasked key: its v row, bit for bit
        rows = [b for b in range(B) if case["Lk"] == 1 or case["valid"][b] == 1]
        X.assert_bits(o[rows], d["v"][rows, :1].expand(-1, Lq, -1).to(BF16), "one unmasked key")


def test_attn_small_refuses_what_does_not_fit_in_lds(ops):
    """head_dim 128: 544 Lk + 2048 bytes; 298 keys are refused on the host before any launch and the output stays untouched"""
    from scail_amd import lib as L
    c = X.LDS_REFUSED
    D = c["H"] * c["hd"]
    q, k, v = X.small_qkv("sparse_q", c["B"], c["H"], c["Lq"], c["Lk"], c["hd"], 3)
    out = nan_buf(c["B"], c["Lq"], D)
    with pytest.raises(L.ScailHipError, match="must fit in LDS"):
        ops.attn_small(q.to(BF16).to(DEV), k.to(BF16).to(DEV), v.to(BF16).to(DEV), c["H"], out=out)
    torch.cuda.synchronize()
    assert all_nan(out)


# ---- the mid-block attention around scail_softmax_rows at ragged token counts -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def vae32():
    """WanVAE_(dim=32): 128 channels in the mid block; random weights, biases and norm weights from the oracle's generator"""
    from oracle import wan_vae_oracle as V
    from scail_amd.wan_vae import WanVAE_
    sd = V.make_state_dict(V.VAEConfig(dim=32, z_dim=16), seed=11)
    m = WanVAE_(dim=32, z_dim=16, device=DEV)
    missing, unexpected = m.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    return m, {k: v.double() for k, v in sd.items()}


def _mid_input(T, H, Wd, seed, C=128):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T, H, Wd, C, generator=g).to(BF16)


@pytest.mark.parametrize("T,H,Wd", [(2, 5, 7), (1, 9, 9)], ids=["nt35", "nt81"])
@pytest.mark.parametrize("block", ["encoder.middle.1", "decoder.middle.1"])
def test_mid_block_attention_at_ragged_token_counts(vae32, block, T, H, Wd):
    """35 tokens (ceil8 = 40: the five extra score columns of frame 0 are frame 1's first keys) and 81 (ceil8 = 88, ceil64 = 128: the pad rows, and
    the memset columns of S and V^T): the layer path against the fp64 oracle at the standing tolerance of multi-rounding bf16 chains"""
    from oracle import wan_vae_oracle as V
    m, sd = vae32
    assert (H * Wd) % 8 != 0
    x = _mid_input(T, H, Wd, 100 + H * Wd)
    got = m._attn(m.prepare(), block, x.to(DEV)).float().cpu()
    want = V.attention_block(sd, block, x.double().permute(3, 0, 1, 2)[None])[0].permute(1, 2, 3, 0)
    print(f"{block} T={T} nt={H * Wd}: max abs err {float((got.double() - want).abs().max()):.4g}")
    torch.testing.assert_close(got.double(), want, rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("block", ["encoder.middle.1", "decoder.middle.1"])
def test_mid_block_attention_ignores_the_next_frames_keys(vae32, block):
    """T = 2, 35 tokens: frame 0's score GEMM writes 40 columns, the last five from frame 1's keys.  With frame 1 replaced by other data (x 64; the
    block's RMS norm takes the factor out again, the keys still differ throughout) frame 0 comes back bit for bit: nothing of those columns
    survives the softmax.  Same T and shapes in both calls, so every GEMM takes the same kernel."""
    m, _ = vae32
    W = m.prepare()
    x = _mid_input(2, 5, 7, 135)
    x2 = x.clone()
    x2[1] = (_mid_input(1, 5, 7, 136)[0].float() * 64).to(BF16)
    a, b = m._attn(W, block, x.to(DEV)), m._attn(W, block, x2.to(DEV))
    assert not torch.equal(a[1], b[1])
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))


@pytest.mark.parametrize("shape", [(1, 3, 5, 40, 56), (1, 3, 1, 72, 72)], ids=["nt35", "nt81"])
def test_c_executor_equals_layerwise_path_at_ragged_token_counts(shape):
    """test_vae_gpu.py::test_c_executor_equals_layerwise_path at 5 x 7 = 35 and 9 x 9 = 81 mid-block tokens per frame: the executor's score GEMM reads
    pad rows it does not clear, and both paths rely on one memset for the columns up to ceil64 of S and V^T"""
    from scail_amd.wan_vae import WanVAE_
    m = WanVAE_(dim=32, z_dim=16, device=DEV)
    vid = (torch.rand(*shape, generator=torch.Generator().manual_seed(shape[3])) * 2 - 1).to(DEV)
    assert m.use_c_exec
    z_c = m.encode(vid)
    x_c = m.decode(z_c)
    assert m._cvae is not None
    m.use_c_exec = False
    z_p = m.encode(vid)
    x_p = m.decode(z_p)
    assert z_c.shape == (1, 16, 1 + (shape[2] - 1) // 4, shape[3] // 8, shape[4] // 8) and x_c.shape == shape
    assert bool(torch.isfinite(z_c).all()) and bool(torch.isfinite(x_c).all())
    assert torch.equal(z_c, z_p) and torch.equal(x_c, x_p)
