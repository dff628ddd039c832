"""GPU tests of the fp8 (e4m3) per-token GEMM path: scail_quant_fp8_rows bit for bit against the tests' reference quantizer
(tests/test_fp8_cpu.py), scail_gemm_fp8 bit for bit on exact-integer operands (every epilogue, against the fp32 product and against
scail_gemm_bf16 on the same, exactly representable, dequantized operands: both kernels share gemm_epi.h), within bf16 rounding on
random data at the 14B shapes, the executor's fp8 mode (CFG-pair and last-layer pruning exactness, determinism, enable / disable,
sequence-parallel refusal) and its accuracy against bf16 and the reference goldens."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import scail_oracle as O
from test_fp8_cpu import e4m3_value, quant_fp8_rows_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
P14B = dict(hidden_size=5120, num_attention_heads=40, inner_hidden_size=13824, text_dim=4096, time_freq_dim=256, time_embed_dim=5120)


def _cos(a, b):
    a, b = a.flatten().double(), b.flatten().double()
    return float((a @ b) / (a.norm() * b.norm()))


def _load(golden_dir, name):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(golden_dir, name)).items()}


# ---- scail_quant_fp8_rows ---------------------------------------------------------------------------------------------------
def test_quant_matches_reference_bit_exactly():
    from scail_amd import ops
    g = torch.Generator().manual_seed(3)
    for rows, cols, ld in ((257, 5120, 5120), (64, 13824, 13824 + 64), (7, 128, 136), (1, 8, 8)):
        x = torch.randn(rows, cols, generator=g) * torch.logspace(-20, 20, rows)[:, None]
        x[0] = 0.0                                          # zero row
        if rows > 2:
            x[1] = 0.0
            x[1, cols // 2] = -3.0e30                       # one huge element
            x[2] = torch.randn(cols, generator=g) * 1e-30   # tiny row
        if rows > 4:
            x[3] = -0.0
            x[4, :] = 448.0                                 # the saturation value itself
        xb = x.to(torch.bfloat16)
        buf = torch.zeros(rows, ld, dtype=torch.bfloat16)
        buf[:, :cols] = xb
        src = buf.to(DEV)[:, :cols]
        q, s = ops.quant_fp8_rows(src)
        torch.cuda.synchronize()
        qr, sr = quant_fp8_rows_ref(xb)
        assert torch.equal(s.cpu(), sr), (rows, cols)
        mism = (q.cpu() != qr).sum()
        assert int(mism) == 0, f"{int(mism)} codes differ at {(rows, cols)}"


# ---- scail_gemm_fp8: exact-integer operands -----------------------------------------------------------------------------------
def _int_operands(M, N, K, lda, g, vmax=3):
    """e4m3 codes of small integers (exact), power-of-two scales, an ASYMMETRIC W (random per element)."""
    xi = torch.randint(-vmax, vmax + 1, (M, K), generator=g).float()
    wi = torch.randint(-vmax, vmax + 1, (N, K), generator=g).float()
    wi[0, :] = torch.arange(K).remainder(7).float() - 3          # a structured, non-symmetric row
    sx = torch.pow(2.0, torch.randint(-3, 3, (M,), generator=g).float())
    sw = torch.pow(2.0, torch.randint(-3, 3, (N,), generator=g).float())
    xq = torch.zeros(M, lda, dtype=torch.uint8)
    xq[:, :K] = xi.to(torch.float8_e4m3fn).view(torch.uint8)
    wq = wi.to(torch.float8_e4m3fn).view(torch.uint8).contiguous()
    return xi, wi, sx, sw, xq, wq


@pytest.mark.parametrize("M,N,K", [(1, 128, 128), (97, 384, 256), (300, 256, 640), (513, 15360, 5120), (260, 5120, 13824)])
def test_gemm_fp8_exact_integer_every_epilogue(M, N, K):
    from scail_amd import lib as L, ops
    g = torch.Generator().manual_seed(M * 7 + N + K)
    lda = K + 16
    xi, wi, sx, sw, xq, wq = _int_operands(M, N, K, lda, g)
    acc = (xi.double() @ wi.double().T)                           # exact
    v = (acc * sx.double()[:, None] * sw.double()[None, :]).float()
    bias = torch.randint(-8, 9, (N,), generator=g).float()
    xq_d, wq_d = xq.to(DEV)[:, :K], wq.to(DEV)
    sx_d, sw_d, b_d = sx.to(DEV), sw.to(DEV), bias.to(DEV)
    # the bf16 GEMM on the dequantized operands (exact in bf16: small integers times powers of two)
    xd = (xi * sx[:, None]).to(torch.bfloat16).to(DEV)
    wd = (wi * sw[:, None]).to(torch.bfloat16).to(DEV).contiguous()
    assert torch.equal(xd.float().cpu(), xi * sx[:, None]) and torch.equal(wd.float().cpu(), wi * sw[:, None])

    # BIAS: bit-exact against the fp32 product (+ integer bias, exact) rounded to bf16
    y = ops.gemm_fp8(xq_d, sx_d, wq_d, sw_d, b_d)
    want = (v + bias).to(torch.bfloat16)
    assert torch.equal(y.cpu(), want), f"max |d| {float((y.float().cpu() - want.float()).abs().max())}"
    assert torch.equal(y, ops.gemm(xd, wd, b_d))
    # no bias
    assert torch.equal(ops.gemm_fp8(xq_d, sx_d, wq_d, sw_d).cpu(), v.to(torch.bfloat16))
    # GELU-tanh: the same epilogue code as the bf16 kernel on the same fp32 values
    yg = ops.gemm_fp8(xq_d, sx_d, wq_d, sw_d, b_d, epilogue=L.EPI_GELU_TANH)
    assert torch.equal(yg, ops.gemm(xd, wd, b_d, epilogue=L.EPI_GELU_TANH))
    ref = torch.nn.functional.gelu((v + bias).double(), approximate="tanh")
    torch.testing.assert_close(yg.double().cpu(), ref, rtol=8e-3, atol=1e-3)
    # RESID ungated, resid aliasing y, output with a row stride > N
    r0 = torch.randint(-64, 65, (M, N), generator=g).float().to(torch.bfloat16)
    out = torch.zeros(M, N + 128, dtype=torch.bfloat16, device=DEV)[:, :N]
    out.copy_(r0.to(DEV))
    ops.gemm_fp8(xq_d, sx_d, wq_d, sw_d, b_d, out=out, epilogue=L.EPI_RESID, resid=out)
    want = (r0.float() + (v + bias)).to(torch.bfloat16)
    assert torch.equal(out.cpu(), want)
    # RESID gated, rows_per_batch: gate[(m / rpb), n]; both kernels share the epilogue -> same bits as the bf16 kernel
    rpb = max(1, (M + 1) // 2)
    nb = (M + rpb - 1) // rpb
    gate = torch.randn(nb, 2 * N, generator=g).to(DEV)[:, :N]
    o8 = r0.to(DEV).clone()
    ob = r0.to(DEV).clone()
    ops.gemm_fp8(xq_d, sx_d, wq_d, sw_d, b_d, out=o8, epilogue=L.EPI_RESID, resid=o8, gate=gate, rows_per_batch=rpb)
    ops.gemm(xd, wd, b_d, out=ob, epilogue=L.EPI_RESID, resid=ob, gate=gate, rows_per_batch=rpb)
    assert torch.equal(o8, ob)
    gm = gate.cpu().repeat_interleave(rpb, 0)[:M]
    torch.testing.assert_close(o8.float().cpu(), r0.float() + gm * (v + bias), rtol=8e-3, atol=1e-2)


# ---- scail_gemm_fp8: random data at the 14B shapes ----------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(15360, 5120), (5120, 5120), (13824, 5120), (5120, 13824)])
def test_gemm_fp8_random_matches_dequantized_product(N, K):
    from scail_amd import ops
    M = 4099
    g = torch.Generator(device=DEV).manual_seed(N + K)
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV, generator=g) * 0.02).to(torch.bfloat16)
    b = torch.randn(N, device=DEV, generator=g)
    xq, sx = ops.quant_fp8_rows(x)
    wq, sw = ops.quant_fp8_rows(w)
    y = ops.gemm_fp8(xq, sx, wq, sw, b)
    rows = torch.tensor([0, 1, 255, 256, 2047, 4000, M - 1])
    xd = e4m3_value(xq[rows].cpu()).double() * sx[rows].cpu().double()[:, None]
    wd = e4m3_value(wq.cpu()).double() * sw.cpu().double()[:, None]
    ref = xd @ wd.T + b.cpu().double()
    mag = xd.abs() @ wd.abs().T
    err = (y[rows].double().cpu() - ref).abs()
    # bf16 output rounding (2^-9 relative, with margin) + fp32 accumulation over K (measured up to ~2e-6 of sum |a b|)
    assert bool((err <= 2.0 ** -8 * ref.abs() + 1e-5 * mag + 1e-6).all()), float((err - 2.0 ** -8 * ref.abs() - 1e-5 * mag).max())


# ---- executor ---------------------------------------------------------------------------------------------------------------
def _mk(params, layers, seed=1234, **kw):
    from scail_amd.dit import DiffusionTransformer
    return DiffusionTransformer(transformer_args=dict(model_parallel_size=1), num_frames=81, latent_width=300, latent_height=300,
                                share_adaln=True, use_i2v_clip=True, device=DEV, init_seed=seed, num_layers=layers, **params, **kw)


def _inputs(T, H, W, text_dim, Lt, Lc, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, T, 16, H, W, generator=g).to(DEV)
    ref = torch.randn(1, 1, 16, H, W, generator=g).to(DEV).to(torch.bfloat16)
    pose = torch.randn(1, T, 16, H // 2, W // 2, generator=g).to(DEV).to(torch.bfloat16)
    ctx = torch.randn(2, Lt, text_dim, generator=g).to(DEV).to(torch.bfloat16)
    clip = torch.randn(1, Lc, 1280, generator=g).to(DEV).to(torch.bfloat16)
    t = torch.tensor([700.0, 700.0], device=DEV)
    return x, t, ctx, ref, pose, clip


def _fwd(net, inputs, **kw):
    x, t, ctx, ref, pose, clip = inputs
    return net.forward_f32(x, t, ctx, None, concat_images=torch.zeros(1, device=DEV), image_clip_features=clip, ref_concat=ref,
                           concat_smpl_render=pose, **kw)


def test_fp8_cfg_pair_is_bit_identical_at_full_size():
    """fp8 keeps SCAIL_DIT_CFG_PAIR exact (per-token activation scales): 14B width, L = 48 832, 3 layers (layer 0, a middle layer and the
    row-pruned last layer run in fp8)."""
    x, t, ctx, ref, pose, clip = _inputs(21, 64, 112, 4096, 512, 257, seed=5)
    x = torch.cat([x[:1], x[:1]]).contiguous()
    inputs = (x, t, ctx, ref, pose, clip)
    net = _mk(P14B, 3, gemm_precision="fp8")
    outs = [_fwd(net, inputs, cfg_pair=pair) for pair in (False, True)]
    assert net._cstep is not None and net._cstep._fp8_buf is not None
    assert torch.isfinite(outs[0]).all() and float(outs[0].abs().mean()) > 1e-3
    assert not torch.equal(outs[0][0], outs[0][1])
    assert torch.equal(outs[0], outs[1]), f"cfg_pair changed the fp8 result: max |d| {float((outs[0] - outs[1]).abs().max())}"


def _net_golden(cfgd, seed, **kw):
    from scail_amd.dit import DiffusionTransformer
    cfg = O.DiTConfig(**cfgd)
    net = DiffusionTransformer(
        transformer_args=dict(model_parallel_size=1, is_decoder=True), num_frames=cfg.num_frames, time_compressed_rate=4,
        latent_width=cfg.latent_width, latent_height=cfg.latent_height, hidden_size=cfg.hidden_size, text_dim=cfg.text_dim,
        num_layers=cfg.num_layers, num_attention_heads=cfg.num_attention_heads, time_freq_dim=cfg.time_freq_dim,
        time_embed_dim=cfg.time_embed_dim, share_adaln=True, inner_hidden_size=cfg.inner_hidden_size, use_i2v_clip=True, device=DEV,
        **kw)
    net.load_state_dict(O.make_state_dict(cfg, seed=seed), strict=True)
    return net


def _golden_kw(g):
    return dict(concat_images=torch.zeros(1, *g["x"].shape[1:], device=DEV), ref_concat=g["ref"].to(DEV),
                concat_smpl_render=g["pose"].to(DEV), image_clip_features=g["clip"].to(DEV))


def test_fp8_step_equals_blockwise_determinism_enable_disable(golden_dir, capsys):
    from scail_amd import lib as L
    g = _load(golden_dir, "dit_tiny.npz")
    seed = int(g["seed"])
    x, t, ctx = g["x"].to(DEV), g["t"].to(DEV), g["ctx"].to(DEV)
    kw = _golden_kw(g)
    net = _net_golden(O.TINY, seed, gemm_precision="fp8")
    o_step = net.forward_f32(x, t, ctx, None, **kw)
    o_step2 = net.forward_f32(x, t, ctx, None, **kw)
    assert torch.equal(o_step, o_step2), "two fp8 runs differ"
    # the same network driven block by block through scail_dit_block (the last layer then runs all rows: the step's row pruning is exact)
    net._c_blocks = True
    o_blocks = net.forward_f32(x, t, ctx, None, **kw)
    net._c_blocks = False
    assert torch.equal(o_step, o_blocks), f"max |d| {float((o_step - o_blocks).abs().max())}"
    # enable -> disable gives the bits of a handle that never enabled fp8
    ref = _net_golden(O.TINY, seed)
    o_bf16 = ref.forward_f32(x, t, ctx, None, **kw)
    assert not torch.equal(o_bf16, o_step)
    net._cstep.enable_fp8(0, DEV)
    assert torch.equal(net.forward_f32(x, t, ctx, None, **kw), o_bf16)
    net._cstep.enable_fp8(L.FP8_ALL, DEV)
    assert torch.equal(net.forward_f32(x, t, ctx, None, **kw), o_step)
    # accuracy (one step on the dit_tiny inputs): against bf16 and against the real reference's output
    c_bf16, c_gold = _cos(o_step.cpu(), o_bf16.cpu()), _cos(o_step.cpu(), g["out"])
    with capsys.disabled():
        print(f"\nfp8 one step (dit_tiny): cosine vs bf16 {c_bf16:.6f}, vs reference golden {c_gold:.6f}, bf16 vs golden "
              f"{_cos(o_bf16.cpu(), g['out']):.6f}")
    assert c_bf16 >= 0.995 and c_gold >= 0.995


def test_fp8_refuses_sequence_parallel_and_the_per_op_path():
    from scail_amd import lib as L
    from scail_amd.parallel import SequenceParallel
    cfgd = dict(hidden_size=256, num_attention_heads=2, inner_hidden_size=512, text_dim=64, time_freq_dim=256, time_embed_dim=256)
    net = _mk(cfgd, 1, gemm_precision="fp8")
    inputs = _inputs(2, 16, 16, 64, 12, 5)
    out = _fwd(net, inputs)
    assert torch.isfinite(out).all()
    # the executor itself: an SP call on a handle with fp8 enabled returns an error before anything runs
    a = ctypes.c_void_p(1 << 20)
    with pytest.raises(L.ScailHipError, match="fp8 GEMMs are enabled"):
        L.call("scail_dit_block_sp", net._cstep._h, 0, a, a, a, a, a, 2, 16, a, a, 1 << 30, None)
    with pytest.raises(L.ScailHipError, match="fp8 GEMMs are enabled"):
        L.call("scail_dit_step_sp", net._cstep._h, a, a, a, a, 1, a, 1, a, a, a, 2, 2, 16, 16, a, 0, a, 1 << 30, None)

    class TwoRanks:
        rank, size = 0, 2

    net.sp = SequenceParallel(TwoRanks(), mode="allgather")
    with pytest.raises(NotImplementedError, match="sequence-parallel"):
        _fwd(net, inputs)
    net.sp = None
    net.use_c_step = False
    with pytest.raises(NotImplementedError, match="per-op path"):
        _fwd(net, inputs)


def test_fp8_full_size_block_accuracy(capsys):
    """one 14B block (L = 48 832) in fp8 against the same block in bf16 (scail_dit_block through CStep.block)"""
    from scail_amd import lib as L
    from scail_amd.cstep import CStep
    T, H, W = 21, 64, 112
    net = _mk(P14B, 1)
    _, _, ctx, _, _, clip = _inputs(T, H, W, 4096, 512, 257, seed=7)
    ctx = ctx[:1].contiguous()
    cs = CStep(net, net.prepare())
    cond = net._conditioning(ctx, clip, None)
    cos, sin = net._rope(T, H // 2, W // 2, 0, 0, DEV)
    Ltok = (H // 2) * (W // 2) * (1 + T) + T * (H // 4) * (W // 4)
    assert Ltok == 48832
    gg = torch.Generator(device=DEV).manual_seed(11)
    h0 = torch.randn(1, Ltok, 5120, device=DEV, generator=gg).to(torch.bfloat16)
    mod = (torch.randn(1, 6 * 5120, device=DEV, generator=gg) * 0.1).contiguous()
    hb = cs.block(0, h0.clone(), mod, cond, cos, sin)
    cs.enable_fp8(L.FP8_ALL, DEV)
    h8 = cs.block(0, h0.clone(), mod, cond, cos, sin)
    torch.cuda.synchronize()
    assert torch.isfinite(h8.float()).all()
    c = _cos((h8.float() - h0.float()).cpu(), (hb.float() - h0.float()).cpu())
    c_full = _cos(h8.float().cpu(), hb.float().cpu())
    with capsys.disabled():
        print(f"\nfp8 14B block (L = 48 832): cosine vs bf16 of the block's update {c:.6f}, of the output {c_full:.6f}")
    assert c >= 0.99
    cs.close()


def test_fp8_sampler_fifty_steps_vs_reference_golden(golden_dir, capsys):
    from scail_amd import sampler as S
    g = _load(golden_dir, "sampler_tiny_50.npz")
    net = _net_golden(O.CONFIG1, int(g["seed"]), gemm_precision="fp8")
    smp = S.RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=50,
                      guider_config={"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": 4}})
    shared = dict(concat_images=torch.zeros(1, *g["x0"].shape[1:], device=DEV), ref_concat=g["ref"].to(DEV),
                  concat_smpl_render=g["pose"].to(DEV), image_clip_features=g["clip"].to(DEV))
    xT = smp.sample_hip(net, g["x0"].to(DEV), dict(crossattn=g["c_ctx"].to(DEV), **shared), dict(crossattn=g["uc_ctx"].to(DEV), **shared))
    assert net._cstep is not None and net._cstep._fp8_buf is not None
    c = _cos(xT.cpu(), g["xT"])
    with capsys.disabled():
        print(f"\nfp8 50-step sampler (config 1): final latent cosine vs the reference golden {c:.6f}, max |d| "
              f"{float((xT.cpu() - g['xT']).abs().max()):.4f}")
    assert c >= 0.98
