"""GPU tests of the per-layer fp8 selection and the on-device GEMM error probe (include/scail_dit.h scail_dit_fp8_select_layers /
scail_dit_fp8_probe, include/scail_hip.h scail_rel_err_rows): the kernel bit for bit on exact-integer operands, the probe leaving the
network's result alone, a table entry against an fp64 restatement, a planted outlier channel found and routed around exactly, the
selection's semantics, and the CLI / engine calibration.  Network: hidden 256, 2 heads, FF 512, 3 layers; 2 x 224 token rows."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

from test_fp8_gpu import _fwd, _inputs, _mk

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFGD = dict(hidden_size=256, num_attention_heads=2, inner_hidden_size=512, text_dim=64, time_freq_dim=256, time_embed_dim=256)
D, FF, LAYERS, LTOK = 256, 512, 3, 224           # Ltok of a (T, H, W) = (2, 16, 16) latent: 64 ref + 128 noise + 32 pose rows
QKV, O, CQ, CO, W1, W2 = range(6)                 # table columns = bit indices of lib.FP8_GEMMS


@pytest.fixture(scope="module")
def inputs():
    return _inputs(2, 16, 16, 64, 12, 5)


@pytest.fixture(scope="module")
def plain(inputs):
    """(bf16 step output, all-fp8 step output) of the seed-1234 network: computed once, read by several tests, never written"""
    o16 = _fwd(_mk(CFGD, LAYERS), inputs)
    o8 = _fwd(_mk(CFGD, LAYERS, gemm_precision="fp8"), inputs)
    assert torch.isfinite(o16).all() and not torch.equal(o16, o8)
    return o16, o8


# ---- 1. the kernel on exact integers ----------------------------------------------------------------------------------------------
def _restate(a, b):
    """numpy restatement of scail_rel_err_rows on fp32 copies of the operands; small integers: every fp32 sum below is exact"""
    d = (b - a).astype(np.float32)
    err = (d * d).sum(1, dtype=np.float32)
    pw = (a * a).sum(1, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(pw == 0, np.where(err == 0, np.float32(0), np.float32(np.inf)), err / pw).astype(np.float32)   # an fp32 division
    return float(err.astype(np.float64).sum()), float(pw.astype(np.float64).sum()), float(ratio.max())


def _padded(x, ld):
    """x (rows, cols) as a bf16 device view with row stride ld; the padding holds a value that would show in every sum"""
    buf = torch.full((x.shape[0], ld), 7.0, dtype=torch.bfloat16)
    buf[:, :x.shape[1]] = torch.from_numpy(x).to(torch.bfloat16)
    return buf.to(DEV)[:, :x.shape[1]]


# the issue's grid, and 2050 rows: more than 1024 rows puts two rows into one workgroup's range
@pytest.mark.parametrize("rows,cols", [(r, c) for r in (1, 97, 513) for c in (128, 384, 5120)] + [(2050, 128)])
def test_rel_err_rows_exact_integers(rows, cols):
    from scail_amd import ops
    rng = np.random.default_rng(rows * 7 + cols)
    a1 = rng.integers(-3, 4, (rows, cols)).astype(np.float32)
    b1 = rng.integers(-3, 4, (rows, cols)).astype(np.float32)
    a2 = rng.integers(-3, 4, (rows, cols)).astype(np.float32)
    b2 = rng.integers(-3, 4, (rows, cols)).astype(np.float32)
    if rows >= 3:
        a1[0] = b1[0] = 0.0                      # an all-zero row: ratio 0
        b1[rows // 2] = a1[rows // 2]            # a == b: err 0
        a1[rows - 1, : cols // 2] = 0.0          # a sparse row: the largest finite ratio is likely here
    a2[rows - 1] = 0.0                           # a == 0, b != 0: +inf (second call only, so that the first checks a finite maximum)
    b2[rows - 1, cols - 1] = 2.0
    assert 36 * cols < 2 ** 24
    acc = torch.zeros(4, device=DEV, dtype=torch.float64)
    ops.rel_err_rows(_padded(a1, cols + 8), _padded(b1, cols + 16), acc)
    e1, p1, m1 = _restate(a1, b1)
    got = acc.cpu().tolist()
    assert got == [e1, p1, m1, float(rows)], (got, [e1, p1, m1, rows])
    assert math.isfinite(m1) and (rows < 3 or m1 > 0.0)
    # a second call accumulates: sums add up, the maximum is kept or raised, rows add up
    ops.rel_err_rows(_padded(a2, cols + 8), _padded(b2, cols + 16), acc)
    e2, p2, m2 = _restate(a2, b2)
    assert m2 == math.inf
    assert acc.cpu().tolist() == [e1 + e2, p1 + p2, math.inf, float(2 * rows)]
    # the same inputs give the same bits, and a finite maximum is not lowered by a later, smaller one
    acc3 = torch.zeros(4, device=DEV, dtype=torch.float64)
    ops.rel_err_rows(_padded(a1, cols + 8), _padded(b1, cols + 16), acc3)
    ops.rel_err_rows(_padded(a1, cols + 8), _padded(a1, cols + 16), acc3)
    assert acc3.cpu().tolist() == [e1, 2 * p1, m1, float(2 * rows)]


# ---- 2. the probe does not change the result -----------------------------------------------------------------------------------------
def test_probe_leaves_the_bf16_result_and_off_is_plain_fp8(inputs, plain):
    from scail_amd import lib as L
    o16, o8 = plain
    net = _mk(CFGD, LAYERS, gemm_precision="fp8")
    assert torch.equal(_fwd(net, inputs), o8)
    ex = net._executor()
    table = ex.fp8_probe_on(2, LTOK, DEV)
    o_probe = _fwd(net, inputs)
    assert torch.equal(o_probe, o16), f"the probe changed the bf16 result: max |d| {float((o_probe - o16).abs().max())}"
    t = table.cpu()
    assert bool((t[..., 0] > 0).all()) and bool((t[..., 1] > 0).all()) and bool((t[..., 2] > 0).all())
    # rows seen = rows the real GEMM ran on: every row in layers 0 and 1, the noise rows only past the last layer's q | k | v
    assert t[:2, :, 3].eq(2 * LTOK).all() and float(t[2, QKV, 3]) == 2 * LTOK and t[2, 1:, 3].eq(2 * 128).all()
    # a call with more rows than the scratch covers is refused before anything is enqueued
    ex.fp8_probe_on(1, LTOK, DEV)
    with pytest.raises(L.ScailHipError, match="the probe's scratch covers 224"):
        _fwd(net, inputs)
    ex.fp8_probe_off()
    assert torch.equal(_fwd(net, inputs), o8), "probe off is not the plain fp8 result"
    # the CFG-pair form probes layer 0's self-attention part once (element 0's rows) and gives the same result
    x, tt, ctx, ref, pose, clip = inputs
    pair = (torch.cat([x[:1], x[:1]]).contiguous(), tt, ctx, ref, pose, clip)
    ref16 = _fwd(_mk(CFGD, LAYERS), pair)
    table = ex.fp8_probe_on(2, LTOK, DEV)
    assert torch.equal(_fwd(net, pair, cfg_pair=True), ref16)
    ex.fp8_probe_off()
    t = table.cpu()
    assert t[0, :2, 3].eq(LTOK).all() and t[0, 2:, 3].eq(2 * LTOK).all() and t[1, :, 3].eq(2 * LTOK).all()


# ---- 3. the table means what it says -----------------------------------------------------------------------------------------------
def test_table_entry_equals_fp64_restatement(inputs):
    """(layer 0, QKV) after one scail_dit_block on a hidden state and modulation of the test's own, against the same three library calls
    made from here and summed in fp64.  Tolerance: the kernel sums a row of cols = 3 D = 768 squares in fp32, so a row sum -- and with it
    the total -- is within cols * 2^-24 = 4.6e-5 relative of the exact one (the fp64 sum over rows adds nothing at this scale)."""
    from scail_amd import ops
    _, _, ctx, _, _, clip = inputs
    net = _mk(CFGD, LAYERS, gemm_precision="fp8")
    W, ex = net.prepare(), net._executor()
    cond = net._conditioning(ctx, clip, None)
    cos, sin = net._rope(2, 8, 8, 0, 0, DEV)
    g = torch.Generator(device=DEV).manual_seed(11)
    h0 = torch.randn(2, LTOK, D, device=DEV, generator=g).to(torch.bfloat16)
    mod = (torch.randn(2, 6 * D, device=DEV, generator=g) * 0.1).contiguous()
    table = ex.fp8_probe_on(2, LTOK, DEV)
    ex.block(0, h0.clone(), mod, cond, cos, sin)
    ex.fp8_probe_off()
    got = table.cpu()[0, QKV].tolist()
    lw = W["layers"][0]
    xn = ops.ln_modulate(h0, mod[:, :D], mod[:, D:2 * D], eps=net.layernorm_epsilon)
    y16 = ops.gemm(xn, lw["qkv_w"], lw["qkv_b"]).reshape(-1, 3 * D)
    xq, sx = ops.quant_fp8_rows(xn.reshape(-1, D))
    wq, sw = ops.quant_fp8_rows(lw["qkv_w"])
    y8 = ops.gemm_fp8(xq, sx, wq, sw, lw["qkv_b"])
    a, b = y16.double().cpu(), y8.double().cpu()
    err_r, pow_r = ((b - a) ** 2).sum(1), (a ** 2).sum(1)
    num, den, worst = float(err_r.sum()), float(pow_r.sum()), float((err_r / pow_r).max())
    tol = 3 * D * 2.0 ** -24
    print(f"\n(0, qkv): num {got[0]:.9e} vs {num:.9e}, den {got[1]:.9e} vs {den:.9e}, worst {got[2]:.9e} vs {worst:.9e}, rel err {math.sqrt(num / den):.4e}")
    assert abs(got[0] - num) <= tol * num and abs(got[1] - den) <= tol * den
    assert abs(got[2] - worst) <= (2 * tol + 2.0 ** -23) * worst           # two row sums and one fp32 division
    assert got[3] == 2 * LTOK and 0.0 < num < den


# ---- 4. planted outlier ------------------------------------------------------------------------------------------------------------
CSTAR = 137                                       # the planted channel of layer 1's MLP
P = "transformer.layers.1.mlp."


def _planted(b1_cstar=None, **kw):
    """The control net (layer 1: W2[:, c*] = 0, b2 = 0) and, with b1_cstar, the planted one (b1[c*] on top)"""
    net = _mk(CFGD, LAYERS, **kw)
    p = dict(net.named_parameters())
    with torch.no_grad():
        p[P + "dense_4h_to_h.weight"][:, CSTAR] = 0
        p[P + "dense_4h_to_h.bias"].zero_()
        if b1_cstar is not None:
            p[P + "dense_h_to_4h.bias"][CSTAR] = b1_cstar
            assert float(p[P + "dense_h_to_4h.bias"][CSTAR]) == b1_cstar          # representable in bf16
    return net


def test_planted_outlier_is_found_and_routed_around_exactly(inputs):
    """One channel of layer 1's MLP activation is made huge (b1[c*] = 2^20 * max |ff| of the control, rounded UP to a power of two so that
    the bf16 parameter holds it exactly); W2's column c* is zero, so the bf16 network does not notice, while the per-token e4m3 scale
    flushes every other entry of each ff row to code 0 (448 x / amax < 2^-10, below half of e4m3's smallest subnormal).

    One entry of the issue's list cannot hold as written and is checked differently: "every table entry except (1, W2) is bit-identical
    between the two nets" also covers (1, W1), but the probe measures the bias-only GEMM, and b1[c*] IS W1's bias: column c* of Y16 is
    2^20 max |ff| in the planted net, so that entry's denominator differs by construction (its numerator loses column c*'s term, where
    both GEMMs round to the bias itself).  Checked instead for (1, W1): den = rows * b1[c*]^2 up to fp32 rounding, num no larger than the
    control's up to the fp32 row-sum bound.  The other 16 entries are compared bit for bit as the issue asks."""
    from scail_amd import lib as L
    from scail_amd.dit import choose_fp8_layers
    # max |ff| of the control's layer 1, from the bf16 per-op path (its MLP buffer still holds layer 1's activation when the tap fires)
    ctl16 = _planted()
    seen = []
    ctl16._tap = lambda i, h: seen.append(float(next(iter(ctl16._ws.values()))["ff"].abs().max())) if i == 1 else None
    _fwd(ctl16, inputs)
    ctl16._tap = None
    o16 = _fwd(ctl16, inputs)
    ff_max = seen[0]
    big = 2.0 ** 20 * 2.0 ** math.ceil(math.log2(ff_max))
    assert 0.0 < ff_max and big >= 2.0 ** 20 * ff_max
    ctl, pl = _planted(gemm_precision="fp8"), _planted(big, gemm_precision="fp8")
    assert torch.equal(_fwd(_planted(big), inputs), o16), "the bf16 network must not see the planted channel"
    t_ctl, t_pl = [], []
    for net, out in ((ctl, t_ctl), (pl, t_pl)):
        rel, worst = net.fp8_probe(*inputs[:3], None, concat_images=torch.zeros(1, device=DEV), image_clip_features=inputs[5],
                                   ref_concat=inputs[3], concat_smpl_render=inputs[4])
        out += [net.fp8_probe_table, rel, worst]
    tc, tp = t_ctl[0], t_pl[0]
    names = list(L.FP8_GEMMS)
    for i in range(LAYERS):
        print(f"\nlayer {i}: control " + " ".join(f"{n} {float(t_ctl[1][i, g]):.4f}" for g, n in enumerate(names)) +
              " | planted " + " ".join(f"{n} {float(t_pl[1][i, g]):.4f}" for g, n in enumerate(names)), end="")
    for i in range(LAYERS):
        for g in range(6):
            if (i, g) not in ((1, W2), (1, W1)):
                assert torch.equal(tc[i, g], tp[i, g]), f"entry ({i}, {names[g]}) differs: {tc[i, g].tolist()} vs {tp[i, g].tolist()}"
    # (1, W2) of the planted net: Y8 == 0, so num == den bit for bit and the relative error is exactly 1, in total and in every row
    assert float(tp[1, W2, 0]) == float(tp[1, W2, 1]) > 0.0 and float(tp[1, W2, 2]) == 1.0 and float(t_pl[1][1, W2]) == 1.0
    assert float(tp[1, W2, 1]) == float(tc[1, W2, 1]), "Y16 of the planted W2 GEMM is the control's"
    # (1, W1) of the planted net: column c* holds the bias itself in both results (see the docstring)
    rows, tol = 2 * LTOK, FF * 2.0 ** -24
    assert rows * big ** 2 <= float(tp[1, W1, 1]) <= rows * big ** 2 * (1 + 2.0 ** -20)
    assert float(tp[1, W1, 0]) <= float(tc[1, W1, 0]) * (1 + 2 * tol) and float(tp[1, W1, 3]) == rows
    # every other entry is below the loose cap 0.25 (e4m3 keeps 3 mantissa bits: each normal operand element is off by at most 2^-4)
    for rel in (t_ctl[1], t_pl[1]):
        for i in range(LAYERS):
            for g in range(6):
                assert (rel is t_pl[1] and (i, g) == (1, W2)) or 0.0 < float(rel[i, g]) < 0.25, (i, names[g], float(rel[i, g]))
    masks = choose_fp8_layers(t_pl[1], 0.5, L.FP8_ALL)
    assert masks == [63, 63 - L.FP8_GEMMS["w2"], 63]
    assert choose_fp8_layers(t_ctl[1], 0.5, L.FP8_ALL) == [63, 63, 63]
    # all-fp8, the planted net is off; under the selection it gives the control's bits
    o_pl_all = _fwd(pl, inputs)
    pl.select_fp8_layers(masks)
    ctl.select_fp8_layers(masks)
    o_pl_sel, o_ctl_sel = _fwd(pl, inputs), _fwd(ctl, inputs)
    assert torch.equal(o_pl_sel, o_ctl_sel), f"max |d| {float((o_pl_sel - o_ctl_sel).abs().max())}"
    e_sel, e_all = float((o_pl_sel - o16).abs().max()), float((o_pl_all - o16).abs().max())
    print(f"\nplanted net, max |out - bf16|: all fp8 {e_all:.5f}, layer 1 W2 left in bf16 {e_sel:.5f} (ff max {ff_max:.3f}, b1[c*] {big:g})")
    assert e_sel < e_all


# ---- 5. selection semantics ----------------------------------------------------------------------------------------------------------
class _Chain:
    """scail_dit_block per layer: layers 0 and 2 on a bf16 handle, layer 1 on an fp8 handle"""

    def __init__(self, ex16, ex8):
        self.ex16, self.ex8 = ex16, ex8

    def block(self, i, *a):
        return (self.ex8 if i == 1 else self.ex16).block(i, *a)


def test_selection_semantics(inputs, plain):
    from scail_amd import lib as L
    o16, o8 = plain
    net = _mk(CFGD, LAYERS, gemm_precision="fp8")
    net.select_fp8_layers([L.FP8_ALL] * LAYERS)
    assert torch.equal(_fwd(net, inputs), o8), "all-ALL masks are not the plain fp8 bits"
    net.select_fp8_layers([0] * LAYERS)
    assert torch.equal(_fwd(net, inputs), o16), "all-zero masks are not the bf16 bits"
    # the option at construction reaches a fresh handle
    assert torch.equal(_fwd(_mk(CFGD, LAYERS, gemm_precision="fp8", fp8_layers=[0, 0, 0]), inputs), o16)
    # only layer 1 in fp8 == the block-wise chain bf16, fp8, bf16 (the same weights behind two handles)
    net.select_fp8_layers([0, L.FP8_ALL, 0])
    o_sel = _fwd(net, inputs)
    assert not torch.equal(o_sel, o16) and not torch.equal(o_sel, o8)
    net16, net8 = _mk(CFGD, LAYERS), _mk(CFGD, LAYERS, gemm_precision="fp8")
    net16.prepare()
    ex16 = net16._executor()
    net16._cstep, net16._c_blocks = _Chain(ex16, net8._executor()), True
    o_chain = _fwd(net16, inputs)
    net16._cstep = ex16
    assert torch.equal(o_sel, o_chain), f"max |d| {float((o_sel - o_chain).abs().max())}"
    # None = uniform again
    net.select_fp8_layers(None)
    assert torch.equal(_fwd(net, inputs), o8)
    # a bit outside the enabled set is an error that names the layer and the bit; the selection in force is kept
    part = _mk(CFGD, LAYERS, gemm_precision="fp8", fp8_gemms=["qkv", "w1"])
    o_part = _fwd(part, inputs)
    with pytest.raises(L.ScailHipError, match=r"layer 1 selects bit 32 \(w2\).*mask 17"):
        part._executor().select_fp8_layers([17, 17 | 32, 0])
    with pytest.raises(L.ScailHipError, match="layer 2 selects bit 64"):
        part._executor().select_fp8_layers([17, 1, 64])
    assert torch.equal(_fwd(part, inputs), o_part)
    # scail_dit_enable_fp8(h, 0, ..) clears the selection: enabling again starts uniform
    ex = net._executor()
    ex.select_fp8_layers([0] * LAYERS)
    assert torch.equal(_fwd(net, inputs), o16)
    ex.enable_fp8(0, DEV)
    assert torch.equal(_fwd(net, inputs), o16)
    ex.enable_fp8(L.FP8_ALL, DEV)
    assert torch.equal(_fwd(net, inputs), o8), "scail_dit_enable_fp8 did not reset the per-layer selection"
    # a sequence-parallel call on a handle with a selection (even an all-zero one) still fails with today's message
    ex.select_fp8_layers([0] * LAYERS)
    a = ctypes.c_void_p(1 << 20)
    with pytest.raises(L.ScailHipError, match="fp8 GEMMs are enabled"):
        L.call("scail_dit_step_sp", ex._h, a, a, a, a, 1, a, 1, a, a, a, 2, 2, 16, 16, a, 0, a, 1 << 30, None)


# ---- 6. CLI and engine ---------------------------------------------------------------------------------------------------------------
def test_cli_calibration_inf_is_plain_fp8_and_zero_is_bf16(capsys):
    from scail_amd import cli, lib as L
    cfg8 = copy.deepcopy(cli.TINY)
    cfg8["model"]["network_config"]["params"]["gemm_precision"] = "fp8"
    e16, e8 = cli.build_engine(cli.TINY), cli.build_engine(cfg8)
    v16, z16, _ = cli.run(cli.TINY, engine=e16)
    v8, z8, _ = cli.run(cfg8, engine=e8)
    assert not torch.equal(z16, z8)
    capsys.readouterr()
    # inf keeps every GEMM: the bits of the plain fp8 run, so the calibration did not disturb the request's noise
    v, z, _ = cli.run(cfg8, engine=e8, fp8_max_error=math.inf)
    out = capsys.readouterr().out
    assert torch.equal(z, z8) and torch.equal(v, v8)
    assert e8.network.fp8_layer_masks == [L.FP8_ALL] * 2 and "left in bf16: none" in out and out.count("e-0") >= 12
    # 0 keeps none: the bits of the bf16 run
    v, z, _ = cli.run(cfg8, engine=e8, fp8_max_error=0.0)
    out = capsys.readouterr().out
    assert torch.equal(z, z16) and torch.equal(v, v16)
    assert e8.network.fp8_layer_masks == [0, 0] and "(0, qkv)" in out and "(1, w2)" in out
    # the engine call itself returns the table it selected from
    cal = e8.calibrate_fp8(*_tiny_conds(e8), (4, 16, 8, 8), 0.5)
    assert cal["rel_err"].shape == (2, 6) and bool((cal["rel_err"] > 0).all()) and bool((cal["worst"] >= cal["rel_err"]).all())
    assert cal["masks"] == e8.network.fp8_layer_masks and cal["enabled"] == L.FP8_ALL
    # a clip longer than one window (25 frames, three windows of 4 latent frames): calibrated on the first window, the same two identities
    e8.network.select_fp8_layers(None)
    _, zt16, _ = cli.run(cli.TINY, engine=e16, frames=25)
    _, zt8, _ = cli.run(cfg8, engine=e8, frames=25)
    assert zt8.shape == (1, 16, 7, 8, 8) and not torch.equal(zt8, zt16)
    assert torch.equal(cli.run(cfg8, engine=e8, frames=25, fp8_max_error=math.inf)[1], zt8)
    assert torch.equal(cli.run(cfg8, engine=e8, frames=25, fp8_max_error=0.0)[1], zt16)
    assert e8.network.fp8_layer_masks == [0, 0] and type(e8.sampler).__name__ == "RFSampler"


def _tiny_conds(engine):
    """c / uc of a synthetic request for the tiny engine (the dictionaries cli.run builds), latent (4, 16, 8, 8)"""
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    shared = dict(concat_images=torch.zeros(1, device=DEV), ref_concat=r(1, 1, 16, 8, 8).to(torch.bfloat16),
                  concat_smpl_render=r(1, 4, 16, 4, 4).to(torch.bfloat16), image_clip_features=r(1, 257, 1280).to(torch.bfloat16))
    return dict(crossattn=r(1, 12, 64), **shared), dict(crossattn=r(1, 12, 64), **shared)
