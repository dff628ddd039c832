"""The step cache on the GPU (include/scail_dit.h "step cache"): the three row kernels against torch on the CPU and numpy, the executor's
FILL / REUSE modes and the cached sampler loop against compositions the test makes itself through ``ops`` and the per-layer seam.

No tolerance except where a sum of fp64 roundings is compared with another order of the same sum (scail_abs_diff_sums on random data,
bound n * 2^-52 * sum): everything else is bit equality.  Toy networks (3 layers, D 512 / 256), latents of Ltok 190 and one of 882."""
import types

import numpy as np
import pytest
import torch

import ws_contract as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
bf16 = torch.bfloat16

TOY = dict(hidden_size=512, num_attention_heads=4, inner_hidden_size=1024, text_dim=64, time_freq_dim=256, time_embed_dim=512)   # test_ws_contract_gpu.TOY
TINY2 = dict(hidden_size=256, num_attention_heads=2, inner_hidden_size=512, text_dim=64, time_freq_dim=256, time_embed_dim=256)  # test_ws_contract_gpu.TINY2
SMALL = (3, 8, 20)              # T, H, W: Ltok 190, Lnoise 120
LARGE = (2, 28, 36)             # Ltok 882, Lnoise 504

_nets = {}


def _net(kind="toy", layers=3, **kw):
    import test_parallel_gpu as P
    key = (kind, layers) + tuple(sorted(kw.items()))
    if key not in _nets:
        _nets[key] = P._mk(dict(TOY if kind == "toy" else TINY2, **kw), layers, seed=77)
    return _nets[key]


def _inputs(shape, n_char=1, pair=False, seed=11, t=700.0):
    import test_parallel_gpu as P
    x, ts, ctx, ref, pose, clip = P._inputs(*shape, n_char, 64, 12, 5, seed=seed)
    if pair:
        x = torch.cat([x[:1], x[:1]]).contiguous()
    return x, torch.full_like(ts, t), ctx, ref, pose, clip


def _fwd(net, inputs, **kw):
    x, t, ctx, ref, pose, clip = inputs
    return net.forward_f32(x, t, ctx, None, concat_images=torch.zeros(1, device=DEV), image_clip_features=clip, ref_concat=ref,
                           concat_smpl_render=pose, **kw)


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu()


def _same_bf16(got, want, what):
    """bit equality of two bf16 tensors, a NaN compared as NaN-ness"""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype == bf16, what
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f"{what}: NaN in {int((gn != wn).sum())} different places"
    bad = (_bits(got) != _bits(want)) & ~wn
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} values differ, first at flat index {int(bad.flatten().nonzero()[0])}"


# ---- 1. scail_resid_store / scail_resid_apply ---------------------------------------------------------------------------------------------
# the second operand of the exhaustive run: zeros, subnormals, the edges of the normal range, infinities, NaNs (quiet, signalling, negative),
# powers of two that are half an ulp of their neighbours below (ties of the rounding), odd and even last bits, and ordinary values
CHOSEN = [0x0000, 0x8000, 0x0001, 0x8001, 0x0040, 0x8040, 0x007f, 0x807f, 0x0080, 0x8080, 0x0081, 0x0100, 0x7f7f, 0xff7f, 0x7f7e, 0xff7e,
          0x7f00, 0x7e80, 0x7f80, 0xff80, 0x7fc0, 0xffc1, 0x7f81, 0x7fff, 0x3f80, 0xbf80, 0x3f81, 0xbf81, 0x3f7f, 0x3f00, 0x3b80, 0xbb80,
          0x3bc0, 0x3c00, 0x4000, 0xc000, 0x4380, 0xc380, 0x4381, 0x4049, 0xc0ad, 0x3eaa, 0x5555, 0xaaaa, 0x1234, 0x9abc, 0x4b00, 0x3780]
assert len(CHOSEN) == 48 and len(set(CHOSEN)) == 48


@pytest.fixture(scope="module")
def exhaustive():
    """every bf16 value against each chosen value, as (B 2, rows 3072, D 512) operands; the torch expressions on the CPU, once"""
    every = torch.tensor(np.arange(65536, dtype=np.uint16).view(np.int16)).view(bf16)
    chosen = torch.tensor(np.array(CHOSEN, dtype=np.uint16).view(np.int16)).view(bf16)
    x = every.repeat(48).view(2, 3072, 512).contiguous()
    y = chosen.repeat_interleave(65536).view(2, 3072, 512).contiguous()
    return dict(x=x, y=y, x_minus_y=(x.float() - y.float()).bfloat16(), y_minus_x=(y.float() - x.float()).bfloat16(),
                x_plus_y=(x.float() + y.float()).bfloat16())


def test_resid_kernels_every_value(exhaustive):
    from scail_amd import ops
    e = exhaustive
    x, y = e["x"].to(DEV), e["y"].to(DEV)
    xb, yb = _bits(x), _bits(y)
    assert torch.isnan(e["x_minus_y"]).any() and torch.isinf(e["x_plus_y"]).any() and (e["x_minus_y"] == 0).any()
    _same_bf16(ops.resid_store(x, y), e["x_minus_y"], "resid_store(x, y)")
    _same_bf16(ops.resid_store(y, x), e["y_minus_x"], "resid_store(y, x)")
    _same_bf16(ops.resid_apply(x, y), e["x_plus_y"], "resid_apply(x, y)")
    _same_bf16(ops.resid_apply(y, x), e["x_plus_y"], "resid_apply(y, x)")
    torch.cuda.synchronize()
    assert torch.equal(_bits(x), xb) and torch.equal(_bits(y), yb), "an input was changed"


def _rand_bf16(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (3.0 * torch.randn(*shape, generator=g)).to(bf16)


@pytest.mark.parametrize("D", [128, 384])
@pytest.mark.parametrize("shared_in", [False, True], ids=["in_bs", "in_bs0"])
def test_resid_kernels_shapes(D, shared_in):
    """rows 37 (no multiple of anything), B 2, a row window [5, 42) of a 50-row matrix, the input's batch stride zero and non-zero, outputs
    between 0xA5 bands"""
    from scail_amd import ops
    B, R, Ltot, r0 = 2, 37, 50, 5
    big_out, big_in = _rand_bf16(B, Ltot, D, seed=1), _rand_bf16(1 if shared_in else B, Ltot, D, seed=2)
    res = _rand_bf16(B, R, D, seed=3)
    go, gi, gr = big_out.to(DEV), big_in.to(DEV), res.to(DEV)
    win_out = go[:, r0:r0 + R]
    win_in = gi[:, r0:r0 + R].expand(B, R, D) if shared_in else gi[:, r0:r0 + R]
    cpu_in = big_in[:, r0:r0 + R].expand(B, R, D)
    # store into a guarded dense r
    r_buf, r_check = W.guarded_like(torch.empty(B, R, D, dtype=bf16, device=DEV), 0x47)
    ops.resid_store(win_out, win_in, out=r_buf)
    r_check("resid_store r")
    _same_bf16(r_buf, (big_out[:, r0:r0 + R].float() - cpu_in.float()).bfloat16(), "resid_store window")
    # apply into a guarded dense h
    h_buf, h_check = W.guarded_like(torch.empty(B, R, D, dtype=bf16, device=DEV), 0x47)
    ops.resid_apply(win_in, gr, out=h_buf)
    h_check("resid_apply h")
    want = (cpu_in.float() + res.float()).bfloat16()
    _same_bf16(h_buf, want, "resid_apply window")
    # apply into the row window of a larger guarded matrix: the rows around the window keep their bits
    m_buf, m_check = W.guarded_like(torch.empty(B, Ltot, D, dtype=bf16, device=DEV), 0x47)
    before = _bits(m_buf)
    ops.resid_apply(win_in, gr, out=m_buf[:, r0:r0 + R])
    m_check("resid_apply into a window")
    _same_bf16(m_buf[:, r0:r0 + R], want, "resid_apply into a window")
    after = _bits(m_buf)
    assert torch.equal(after[:, :r0], before[:, :r0]) and torch.equal(after[:, r0 + R:], before[:, r0 + R:]), "rows outside the window were written"
    torch.cuda.synchronize()
    assert torch.equal(_bits(go), _bits(big_out)) and torch.equal(_bits(gi), _bits(big_in)) and torch.equal(_bits(gr), _bits(res)), "an input was changed"


@pytest.mark.parametrize("D", [128, 384])
@pytest.mark.parametrize("shared_in", [False, True], ids=["in_bs", "in_bs0"])
def test_resid_apply_in_place(D, shared_in):
    """h IS h_in: element for element, and (in_bs == 0) element 0 as the one input of both elements and an output -- the executor's
    REUSE under SCAIL_DIT_CFG_PAIR.  In a row window of a guarded matrix."""
    from scail_amd import ops
    B, R, Ltot, r0 = 2, 37, 50, 5
    big, res = _rand_bf16(B, Ltot, D, seed=4), _rand_bf16(B, R, D, seed=5)
    m_buf, m_check = W.guarded_like(torch.empty(B, Ltot, D, dtype=bf16, device=DEV), 0x47)
    m_buf.copy_(big.to(DEV))
    gr = res.to(DEV)
    win = m_buf[:, r0:r0 + R]
    h_in = m_buf[:1, r0:r0 + R].expand(B, R, D) if shared_in else win
    cpu_in = big[:1, r0:r0 + R].expand(B, R, D) if shared_in else big[:, r0:r0 + R]
    out = ops.resid_apply(h_in, gr, out=win)
    assert out.data_ptr() == h_in.data_ptr()
    m_check("resid_apply in place")
    _same_bf16(win, (cpu_in.float() + res.float()).bfloat16(), "resid_apply in place")
    after, before = _bits(m_buf), _bits(big)
    assert torch.equal(after[:, :r0], before[:, :r0]) and torch.equal(after[:, r0 + R:], before[:, r0 + R:]), "rows outside the window were written"
    assert torch.equal(_bits(gr), _bits(res))


def test_resid_kernels_grid_stride():
    """more 8-column chunks than the capped grid has threads (2048 workgroups x 256): the loop's second trip"""
    from scail_amd import ops
    B, R, D = 1, 2 * 2048 * 256 * 8 // 4096 + 3, 4096          # 1027 rows: 525 824 chunks > 524 288 threads
    a, b = _rand_bf16(B, R, D, seed=6), _rand_bf16(B, R, D, seed=7)
    ga, gb = a.to(DEV), b.to(DEV)
    _same_bf16(ops.resid_store(ga, gb), (a.float() - b.float()).bfloat16(), "resid_store, second trip")
    _same_bf16(ops.resid_apply(ga, gb), (a.float() + b.float()).bfloat16(), "resid_apply, second trip")


# ---- 2. scail_abs_diff_sums ---------------------------------------------------------------------------------------------------------------
SIZES = [1, 255, 256, 257, 1536, 30720]


@pytest.mark.parametrize("n", SIZES)
def test_abs_diff_sums_exact_on_dyadic_inputs(n):
    """integers x 2^-10 below 2^13: every term and every partial sum is an integer multiple of 2^-10 below 2^53 of them, so the fp64 sums
    are exact in any order and the result must be THE sum"""
    from scail_amd import ops
    g = torch.Generator().manual_seed(n)
    ia, ib = torch.randint(-(1 << 12), 1 << 12, (n,), generator=g), torch.randint(-(1 << 12), 1 << 12, (n,), generator=g)
    a, b = (ia.double() / 1024).float(), (ib.double() / 1024).float()
    want = torch.tensor([float((ia - ib).abs().sum()) / 1024, float(ib.abs().sum()) / 1024], dtype=torch.float64)
    out, check = W.guarded_like(torch.empty(2, dtype=torch.float64, device=DEV), 0xFF)
    ga, gb = a.to(DEV), b.to(DEV)
    ops.abs_diff_sums(ga, gb, out=out)
    check("abs_diff_sums out")
    assert torch.equal(out.cpu(), want), (out.cpu(), want)
    again = ops.abs_diff_sums(ga, gb)
    assert torch.equal(again.view(torch.int64).cpu(), out.view(torch.int64).cpu()), "two calls, two results"
    assert torch.equal(ga.cpu(), a) and torch.equal(gb.cpu(), b)


@pytest.mark.parametrize("n", SIZES)
def test_abs_diff_sums_random(n):
    """random fp32 data: each term is exact in fp64 up to one rounding, the sum is n - 1 more: within n * 2^-52 * sum of numpy's fp64 sum,
    and the same bits on a second call"""
    from scail_amd import ops
    g = torch.Generator().manual_seed(100 + n)
    a, b = torch.randn(n, generator=g) * 37.0, torch.randn(n, generator=g) * 0.01 + 2.0
    a64, b64 = a.numpy().astype(np.float64), b.numpy().astype(np.float64)
    want = np.array([np.abs(a64 - b64).sum(), np.abs(b64).sum()])
    ga, gb = a.to(DEV), b.to(DEV)
    got = ops.abs_diff_sums(ga, gb)
    again = ops.abs_diff_sums(ga, gb)
    g64 = got.cpu().numpy()
    print(f"abs_diff_sums n {n}: got {g64}, numpy {want}, |d| / sum {np.abs(g64 - want) / want}, bound {n * 2.0 ** -52}")
    assert np.all(np.abs(g64 - want) <= n * 2.0 ** -52 * want), (g64, want)
    assert torch.equal(again.view(torch.int64), got.view(torch.int64))


# ---- 3. scail_dit_time_distances ------------------------------------------------------------------------------------------------------------
def _time_signal(net, ts, signal):
    """the step's own time embedding of every timestep, through ops, in the executor's chunks of 8"""
    from scail_amd import lib as L, ops
    Wt = net.prepare()
    rows = []
    for s0 in range(0, ts.numel(), 8):
        temb = ops.timestep_embedding(ts[s0:s0 + 8].contiguous(), net.time_freq_dim)
        e1 = ops.small_linear(temb, Wt["time_embed.0.w"], Wt["time_embed.0.b"], act_out=L.ACT_SILU)
        emb = ops.small_linear(e1, Wt["time_embed.2.w"], Wt["time_embed.2.b"])
        v = emb if signal == "time" else ops.small_linear(emb, Wt["adaln_projection.1.w"], Wt["adaln_projection.1.b"], act_in=L.ACT_SILU)
        rows.extend(v[j].contiguous() for j in range(v.shape[0]))
    return rows


@pytest.mark.parametrize("signal", ["time", "modulation"])
@pytest.mark.parametrize("n_steps", [1, 2, 9, 50])
def test_time_distances(n_steps, signal):
    from scail_amd import ops
    from scail_amd.sampler import make_flow_timesteps
    net = _net()
    ts = (make_flow_timesteps(0, n_steps, shift_scale=5)[:-1] * 1000.0).to(DEV).contiguous()
    assert ts.numel() == n_steps
    rows = _time_signal(net, ts, signal)
    assert len(rows) == n_steps and rows[0].numel() == (net.time_embed_dim if signal == "time" else 6 * net.hidden_size)
    want = torch.zeros(n_steps, 2, dtype=torch.float64)
    for i in range(1, n_steps):
        want[i] = ops.abs_diff_sums(rows[i], rows[i - 1]).cpu()
    got = net.time_distances(ts, signal)
    assert got.shape == (n_steps, 2) and got.dtype == torch.float64 and got.device.type == "cpu"
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)), (got, want)
    if n_steps > 1:
        assert bool((got[1:] > 0).all()) and bool(torch.isfinite(got).all())
    with W.poisoned(0xFF) as s:                                  # the scratch and the table come out of guarded, NaN-filled memory
        again = net.time_distances(ts, signal)
        assert len(s.outs) == 2, "scratch and table"
        s.workspaces.append(("(none: the call has a scratch of its own, no workspace)", None))
        s.check()
    assert torch.equal(again.view(torch.int64), want.view(torch.int64))


# ---- 4. FILL --------------------------------------------------------------------------------------------------------------------------------
def _lens(shape, n_char):
    T, H, Wd = shape
    hp, wp = H // 2, Wd // 2
    return n_char * hp * wp, T * hp * wp


def _tables(net, t):
    """(mod (layers, B, 6D), fin (B, 2D)) of the timesteps, as the per-op path forms them"""
    from scail_amd import lib as L, ops
    Wt = net.prepare()
    temb = ops.timestep_embedding(t, net.time_freq_dim)
    e1 = ops.small_linear(temb, Wt["time_embed.0.w"], Wt["time_embed.0.b"], act_out=L.ACT_SILU)
    emb = ops.small_linear(e1, Wt["time_embed.2.w"], Wt["time_embed.2.b"])
    adaln = ops.small_linear(emb, Wt["adaln_projection.1.w"], Wt["adaln_projection.1.b"], act_in=L.ACT_SILU)
    return ops.adaln_table(adaln, Wt["adaln_tables"]), ops.adaln_table(emb.repeat(1, 2).contiguous(), Wt["final_table"])[0]


def _per_layer_hidden(net, inputs, shape, n_char):
    """(embedded noise rows, noise rows after the last block), bf16 (B, Lnoise, D): patch embedding through ops, then CStep.block per layer"""
    from scail_amd import ops
    x, t, ctx, ref, pose, clip = inputs
    Wt, ex, D = net.prepare(), net._executor(), net.hidden_size
    B = x.shape[0]
    Lref, Lnoise = _lens(shape, n_char)
    Lrn = Lref + Lnoise
    mod, _ = _tables(net, t)
    tok = ops.patchify(x, ref, pose, kpad=128, n_char=n_char)
    h = torch.empty(B, tok.shape[1], D, device=DEV, dtype=bf16)
    for b in range(B):
        ops.gemm(tok[b, :Lrn], Wt["patch_w"], Wt["patch_b"], out=h[b, :Lrn])
        ops.gemm(tok[b, Lrn:], Wt["pose_w"], Wt["pose_b"], out=h[b, Lrn:])
    h_in = h[:, Lref:Lrn].clone()
    cond = net._conditioning(ctx, clip)
    cos, sin = net._rope(shape[0], shape[1] // 2, shape[2] // 2, 0, 0, x.device, n_char)
    for i in range(net.num_layers):
        ex.block(i, h, mod[i].contiguous(), cond, cos, sin)
    return h_in, h[:, Lref:Lrn].clone()


def _check_fill(net, inputs, shape, n_char=1, cfg_pair=False):
    x = inputs[0]
    B, D = x.shape[0], net.hidden_size
    plain = _fwd(net, inputs, cfg_pair=cfg_pair).clone()
    ex = net._executor()
    ex._cache = None
    out = _fwd(net, inputs, cfg_pair=cfg_pair, step_cache="fill")
    assert torch.equal(out, plain), f"FILL changed the result in {int((out != plain).sum())} values"
    assert bool(torch.isfinite(out).all())
    assert ex._cache[1].numel() == ex.step_cache_bytes(B, *shape) and ex._cache[1].data_ptr() % 256 == 0
    r = ex.step_cache_residual(B, *shape, D).clone()
    h_in, h_out = _per_layer_hidden(net, inputs, shape, n_char)
    assert r.shape == h_in.shape == (B, _lens(shape, n_char)[1], D)
    _same_bf16(r, (h_out.cpu().float() - h_in.cpu().float()).bfloat16(), "r at offset 0 of the cache")
    assert not torch.equal(_bits(h_out), _bits(h_in))
    return out, r


def test_fill_cfg_pair():
    _check_fill(_net(), _inputs(SMALL, pair=True), SMALL, cfg_pair=True)


def test_fill_cfg_pair_large():
    _check_fill(_net(), _inputs(LARGE, pair=True), LARGE, cfg_pair=True)


def test_fill_batch_one():
    x, t, ctx, ref, pose, clip = _inputs(SMALL)
    _check_fill(_net(), (x[:1].contiguous(), t[:1].contiguous(), ctx[:1].contiguous(), ref, pose, clip), SMALL)


def test_fill_batch_two_own_ref_and_pose():
    x, t, ctx, ref, pose, clip = _inputs(SMALL)
    ref2, pose2 = torch.cat([ref, ref.flip(-1)]).contiguous(), torch.cat([pose, pose.flip(-1)]).contiguous()
    _, r = _check_fill(_net(), (x, t, ctx, ref2, pose2, clip), SMALL)
    assert not torch.equal(_bits(r[0]), _bits(r[1]))


def test_fill_two_characters():
    inputs = _inputs(SMALL, n_char=2, pair=True)
    assert inputs[3].shape[1] == 2
    net = _net("tiny2")
    _check_fill(net, inputs, SMALL, n_char=2, cfg_pair=True)
    ex = net._executor()
    assert ex.step_cache_bytes(2, *SMALL) == 2 * ((2 * 120 * 256 * 2 + 255) // 256 * 256), "the cache does not depend on n_char: r + the kept embedding"


def test_fill_one_layer_network():
    """one layer: the pair sharing switches itself off (it needs a layer after layer 0), and that layer is the row-pruned last one"""
    _check_fill(_net(layers=1), _inputs(SMALL, pair=True), SMALL, cfg_pair=True)


def test_fill_fp8():
    net = _net(gemm_precision="fp8", fp8_scaling="row")
    _check_fill(net, _inputs(SMALL, pair=True), SMALL, cfg_pair=True)
    assert net._cstep._fp8_buf is not None


# ---- 5. REUSE -------------------------------------------------------------------------------------------------------------------------------
def _reuse_reference(net, inputs, shape, r, n_char=1):
    """what a REUSE evaluation is, through ops: patchify, the patch GEMM on the noise rows, r added, the final layer"""
    from scail_amd import ops
    x, t, ctx, ref, pose, clip = inputs
    Wt, D = net.prepare(), net.hidden_size
    B = x.shape[0]
    Lref, Lnoise = _lens(shape, n_char)
    _, fin = _tables(net, t)
    tok = ops.patchify(x, ref, pose, kpad=128, n_char=n_char)
    e = torch.empty(B, Lnoise, D, device=DEV, dtype=bf16)
    for b in range(B):
        ops.gemm(tok[b, Lref:Lref + Lnoise], Wt["patch_w"], Wt["patch_b"], out=e[b])
    h = ops.resid_apply(e, r)
    xf = ops.ln_modulate(h, fin[:, :D], fin[:, D:], eps=net.layernorm_epsilon)
    tokout = ops.gemm(xf, Wt["final_w"], Wt["final_b"])
    return ops.unpatchify(tokout.contiguous(), *shape)


@pytest.mark.parametrize("case", ["pair", "pair_large", "plain", "two_characters", "batch_one"])
def test_reuse(case):
    shape = LARGE if case == "pair_large" else SMALL
    n_char = 2 if case == "two_characters" else 1
    pair = case != "plain" and case != "batch_one"
    net = _net("tiny2" if n_char == 2 else "toy")
    first, second = _inputs(shape, n_char, pair=pair, seed=11, t=700.0), _inputs(shape, n_char, pair=pair, seed=12, t=350.0)
    if case == "batch_one":
        first, second = (tuple(v[:1].contiguous() if i < 3 else v for i, v in enumerate(inp)) for inp in (first, second))
    assert not torch.equal(first[0], second[0])
    ex = net._executor()
    ex._cache = None
    _fwd(net, first, cfg_pair=pair, step_cache="fill")
    cache = ex._cache[1]
    kept = cache.clone()
    r = ex.step_cache_residual(second[0].shape[0], *shape, net.hidden_size).clone()
    snap = W.snapshot(dict(net=net, prepared=net._prepared, inputs=second))
    out = _fwd(net, second, cfg_pair=pair, step_cache="reuse").clone()
    torch.cuda.synchronize()
    assert torch.equal(cache, kept), "REUSE wrote into the cache"
    W.assert_unchanged(snap)
    want = _reuse_reference(net, second, shape, r, n_char)
    assert out.shape == want.shape == second[0].shape and bool(torch.isfinite(out).all())
    assert torch.equal(out, want), f"REUSE differs from its composition in {int((out != want).sum())} values"
    if second[0].shape[0] == 2:
        assert not torch.equal(out[0], out[1]), "the two elements carry different residuals"
    assert not torch.equal(out, _fwd(net, second, cfg_pair=pair)), "a REUSE evaluation is not a full evaluation"
    # REUSE does not read the conditioning: the binding passes NULL for None
    x, t, ctx, rf, ps, clip = second
    cos, sin = net._rope(shape[0], shape[1] // 2, shape[2] // 2, 0, 0, x.device, n_char)
    bare = ex.step_cached(x, t, None, rf, ps, cos, sin, "reuse", cfg_pair=pair, n_char=n_char)
    assert torch.equal(bare, want)


@pytest.mark.parametrize("case", ["pair", "plain"])
def test_fill_and_reuse_on_poisoned_guarded_buffers(case):
    """FILL then REUSE with the workspaces, the cache and the outputs handed out at exactly the queried size between guard bands, once per
    fill pattern: the same bits as on ordinary buffers, bands intact, the cache untouched by REUSE"""
    pair = case == "pair"
    net = _net()
    first, second = _inputs(SMALL, pair=pair, seed=11, t=700.0), _inputs(SMALL, pair=pair, seed=12, t=350.0)
    ex = net._executor()

    def run():
        ex._cache = None
        o1 = _fwd(net, first, cfg_pair=pair, step_cache="fill").clone()
        kept = ex._cache[1].clone()
        o2 = _fwd(net, second, cfg_pair=pair, step_cache="reuse").clone()
        torch.cuda.synchronize()
        assert torch.equal(ex._cache[1], kept), "REUSE wrote into the cache"
        return o1, o2

    plain = run()
    snap = W.snapshot(dict(net=net, prepared=net._prepared, first=first, second=second))
    for name, fill in W.FILLS.items():
        with W.poisoned(fill) as s:
            got = run()
            s.check()
            whats = [what for what, _ in s.workspaces]
            assert any("scail_dit_step_cache_bytes" in w for w in whats) and any("scail_dit_chars_workspace_bytes" in w for w in whats), whats
            cache_ws = [ws for what, ws in s.workspaces if "scail_dit_step_cache_bytes" in what]
            assert len(cache_ws) == 1 and cache_ws[0].numel() == ex.step_cache_bytes(2, *SMALL), "one cache, at exactly the queried size"
        for g, p in zip(got, plain):
            assert bool(torch.isfinite(g).all()), f"fill {name}: non-finite output"
            assert torch.equal(g, p), f"fill {name}: differs from the plain run in {int((g != p).sum())} values"
    ex._cache = None
    W.assert_unchanged(snap)


# ---- 6. scail_dit_sample_cached -----------------------------------------------------------------------------------------------------------
SIG6 = torch.tensor([1.0, 0.9, 0.75, 0.6, 0.4, 0.2, 0.0])
MASK6 = [0, 1, 0, 1, 1, 0]


@pytest.mark.parametrize("n_char", [1, 2])
def test_sample_cached_all_zero_mask_is_the_plain_sampler(n_char):
    net = _net("toy" if n_char == 1 else "tiny2")
    x, t, ctx, ref, pose, clip = _inputs(SMALL, n_char=n_char)
    plain = net.sample_c(x[:1], SIG6, 4.0, ctx, ref, pose, clip).clone()
    net._executor()._cache = None
    got = net.sample_c(x[:1], SIG6, 4.0, ctx, ref, pose, clip, reuse=[0] * 6)
    assert torch.equal(got, plain) and bool(torch.isfinite(got).all())


def _host_loop(net, x0, sig, cfg, ctx, ref, pose, clip, mask):
    from scail_amd import ops
    x = x0.float().contiguous().clone()
    for i in range(len(sig) - 1):
        t = (sig[i] * 1000.0).repeat(2).to(DEV)
        v = net.forward_f32(torch.cat([x, x], 0), t, ctx, None, concat_images=torch.zeros(1, device=DEV), image_clip_features=clip,
                            ref_concat=ref, concat_smpl_render=pose, cfg_pair=True, step_cache="reuse" if mask[i] else "fill")
        ops.cfg_euler_(x, v, cfg, float(sig[i + 1] - sig[i]))
    return x


@pytest.mark.parametrize("n_char", [1, 2])
def test_sample_cached_mask_is_the_host_loop(n_char):
    net = _net("toy" if n_char == 1 else "tiny2")
    x, t, ctx, ref, pose, clip = _inputs(SMALL, n_char=n_char)
    net._executor()._cache = None
    want = _host_loop(net, x[:1], SIG6, 4.0, ctx, ref, pose, clip, MASK6)
    net._executor()._cache = None
    with W.poisoned(0xFF) as s:
        got = net.sample_c(x[:1], SIG6, 4.0, ctx, ref, pose, clip, reuse=MASK6).clone()
        s.check()
    net._executor()._cache = None
    assert torch.equal(got, want), f"differs from the host loop in {int((got != want).sum())} values"
    assert bool(torch.isfinite(got).all())
    assert not torch.equal(got, net.sample_c(x[:1], SIG6, 4.0, ctx, ref, pose, clip)), "the mask skipped nothing"


@pytest.mark.parametrize("n_char", [1, 2])
@pytest.mark.parametrize("option", [dict(mask=MASK6), dict(threshold=1e30, signal="modulation"), dict(threshold=0.0)], ids=["mask", "huge", "zero"])
def test_sample_hip_routes_agree(option, n_char):
    """RFSampler.sample_hip: the one-call route and the host loop (a step callback forces it) take the same plan and give the same bits"""
    from scail_amd.sampler import RFSampler
    net = _net("toy" if n_char == 1 else "tiny2")
    x, t, ctx, ref, pose, clip = _inputs(SMALL, n_char=n_char)
    shared = dict(concat_images=torch.zeros(1, device=DEV), ref_concat=ref, concat_smpl_render=pose, image_clip_features=clip)
    c, uc = dict(crossattn=ctx[1:2], **shared), dict(crossattn=ctx[0:1], **shared)
    s = RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=6)
    net._executor()._cache = None
    one = s.sample_hip(net, x[:1], c, uc, scale=4.0, step_cache=dict(option)).clone()
    plan = list(s.last_step_cache_plan)
    assert plan == {"mask": MASK6, "huge": [0, 1, 1, 1, 1, 0], "zero": [0] * 6}["mask" if "mask" in option else "huge" if option["threshold"] else "zero"]
    seen = []
    net._executor()._cache = None
    loop = s.sample_hip(net, x[:1], c, uc, scale=4.0, step_cache=dict(option), step_callback=lambda i, xx: seen.append(i))
    assert seen == list(range(6)) and s.last_step_cache_plan == plan
    assert torch.equal(one, loop), f"the two routes differ in {int((one != loop).sum())} values"
    if not any(plan):
        assert torch.equal(one, s.sample_hip(net, x[:1], c, uc, scale=4.0)), "a plan without reuse is the uncached sampler"
    net._executor()._cache = None


# ---- 7. refusals that need a handle ---------------------------------------------------------------------------------------------------------
def test_cache_one_byte_short():
    from scail_amd import lib as L
    net, inputs = _net(), _inputs(SMALL, pair=True)
    ex = net._executor()
    need = ex.step_cache_bytes(2, *SMALL)
    assert need == 2 * 2 * 120 * 512 * 2 and ex.step_cache_bytes(1, *SMALL) == need // 2
    assert L.load().scail_dit_step_cache_bytes(ex._h, 2, 3, 8, 18) == -1 and L.load().scail_dit_step_cache_bytes(ex._h, 0, 3, 8, 20) == -1
    buf, check = W.guarded(need, 0x47, DEV)
    for mode in ("fill", "reuse"):
        ex._cache = ((2, *SMALL, inputs[0].device), buf[:need - 1])
        with pytest.raises(L.ScailHipError, match=rf"cache too small: {need - 1} bytes, needs {need}"):
            _fwd(net, inputs, cfg_pair=True, step_cache=mode)
    x, t, ctx, ref, pose, clip = inputs
    with pytest.raises(L.ScailHipError, match=rf"cache too small: {need - 1} bytes, needs {need}"):
        net.sample_c(x[:1], SIG6, 4.0, ctx, ref, pose, clip, reuse=MASK6)
    check("a refused cache")
    assert W.holds_fill(buf, 0x47), "a refused call wrote into the cache"
    ex._cache = None


def test_python_refusals():
    from scail_amd import lib as L
    from scail_amd.sampler import RFSampler, RFSamplerLong
    net, inputs = _net(), _inputs(SMALL, pair=True)
    x, t, ctx, ref, pose, clip = inputs
    ex = net._executor()
    ex._cache = None
    with pytest.raises(L.ScailHipError, match="needs a 'fill' evaluation"):
        _fwd(net, inputs, cfg_pair=True, step_cache="reuse")
    with pytest.raises(L.ScailHipError, match="mode must be one of"):
        _fwd(net, inputs, cfg_pair=True, step_cache="refill")
    with pytest.raises(L.ScailHipError, match="one entry per step"):
        net.sample_c(x[:1], SIG6, 4.0, ctx, ref, pose, clip, reuse=[0, 1])
    with pytest.raises(L.ScailHipError, match=r"reuse\[0\] = 1"):
        net.sample_c(x[:1], SIG6, 4.0, ctx, ref, pose, clip, reuse=[1, 0, 0, 0, 0, 0])
    ex._cache = None                                         # (the binding had a cache ready for the call the library refused)
    shared = dict(concat_images=torch.zeros(1, device=DEV), ref_concat=ref, concat_smpl_render=pose, image_clip_features=clip)
    c, uc = dict(crossattn=ctx[1:2], **shared), dict(crossattn=ctx[0:1], **shared)
    # tiled
    long = RFSamplerLong(hunyuan_schedule=True, shift_scale=5, num_steps=2)
    with pytest.raises(NotImplementedError, match="step_cache"):
        long.sample_hip(net, x[:1], dict(c, smpl_tiled=pose[:, None]), uc, tile_indices=[[0, 1], [1, 2]], step_cache=dict(threshold=0.1))
    # sequence-parallel ranks, SCAIL_C_STEP=0, _tap, kernel_timer, the per-block seam: refused by the network and by the sampler
    s = RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=2)
    settings = [("sp", types.SimpleNamespace(size=2, rank=0)), ("use_c_step", False), ("_tap", lambda i, h: None), ("kernel_timer", {}), ("_c_blocks", True)]
    for attr, value in settings:
        old = getattr(net, attr)
        setattr(net, attr, value)
        try:
            with pytest.raises(NotImplementedError, match="step_cache"):
                _fwd(net, inputs, cfg_pair=True, step_cache="fill")
            with pytest.raises(NotImplementedError, match="step_cache"):
                net.sample_c(x[:1], SIG6, 4.0, ctx, ref, pose, clip, reuse=MASK6)
            if attr != "_c_blocks":
                with pytest.raises(NotImplementedError, match="step_cache"):
                    s.sample_hip(net, x[:1], c, uc, scale=4.0, step_cache=dict(mask=[0, 1]))
        finally:
            setattr(net, attr, old)
    assert ex._cache is None, "a refused request allocated a cache"
    assert torch.equal(_fwd(net, inputs, cfg_pair=True, step_cache="fill"), _fwd(net, inputs, cfg_pair=True))
    ex._cache = None
