"""Wiring tests of the DiT step on the GPU: every route through scail_amd/dit.py and csrc/dit_step.hip runs the PLANTED network on
the planted inputs (tests/dit_wiring.py) and is compared with the fp32 oracle by e(a, b) = ||a - b||_2 / ||b||_2 at every observation
point the route exposes.  The bound at point p is T_p = 2 N_p, N_p being the distance of the CPU bf16-storage model from the oracle
(dit_wiring.bounds: derived on the CPU, proven discriminating by tests/test_dit_wiring_cpu.py -- every catalogue mutant moves some point
by >= 4 T_p -- and never taken from a GPU result).  A value over T_p is a finding: a store point the model misses, or a wrong wire.

Every test prints its figures (route, point, N_p, T_p, measured) before it asserts; profiles/dit_wiring.log is that output."""
import pytest
import torch

import dit_wiring as DW
from oracle import scail_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _net():
    from scail_amd.dit import DiffusionTransformer
    cfg = DW.planted_config()
    net = DiffusionTransformer(
        transformer_args=dict(model_parallel_size=1, is_decoder=True), num_frames=cfg.num_frames, time_compressed_rate=4,
        latent_width=cfg.latent_width, latent_height=cfg.latent_height, patch_size=[1, 2, 2], in_channels=20, out_channels=16,
        hidden_size=cfg.hidden_size, text_dim=cfg.text_dim, num_layers=cfg.num_layers, num_attention_heads=cfg.num_attention_heads,
        elementwise_affine=False, time_freq_dim=cfg.time_freq_dim, time_embed_dim=cfg.time_embed_dim, share_adaln=True,
        inner_hidden_size=cfg.inner_hidden_size, use_i2v_clip=True, dtype="bf16", device=DEV,
        modules={"pos_embed_config": {"params": {"hidden_size_head": 128, "interleaved_rope": True}},
                 "adaln_layer_config": {"params": {"qk_ln": True, "hidden_size_head": cfg.hidden_size}}})
    missing, unexpected = net.load_state_dict(DW.planted_state_dict(cfg), strict=True)
    assert not missing and not unexpected
    return net


@pytest.fixture(scope="module")
def planted():
    """config, weights, inputs, the oracle's observation points (computed once, never written to) and the CPU-derived bounds"""
    cfg = DW.planted_config()
    sd = DW.planted_state_dict(cfg)
    inp = DW.planted_inputs()
    ref = DW.oracle_points(cfg, sd, inp)
    bi = DW.block_inputs_of(cfg, ref)
    ref = DW.oracle_points(cfg, sd, inp, bi)
    return dict(cfg=cfg, sd=sd, inp=inp, ref=ref, block_inputs=bi, bounds=DW.bounds())


def _kw(inp):
    return dict(concat_images=torch.zeros(1, device=DEV), ref_concat=inp["ref"].to(DEV), concat_smpl_render=inp["pose"].to(DEV),
                image_clip_features=inp["clip"].to(DEV))


def _check(capsys, route, bounds, got, want):
    """print every figure of the route, then assert all of them"""
    rows = [(p, bounds["N"][p], bounds["T"][p], DW.e(got[p].float().cpu(), want[p])) for p in got]
    with capsys.disabled():
        print()
        for p, n, t, m in rows:
            print("wiring  %-44s %-6s N_p %.3e  T_p %.3e  measured %.3e  (%.2f N_p)%s" % (route, p, n, t, m, m / n, "" if m <= t else "   OVER"))
    over = [(p, m, t) for p, _, t, m in rows if not m <= t]
    assert not over, f"{route}: over T_p at {over}"


def test_per_op_path(planted, capsys):
    """use_c_step = False: the host-driven kernel sequence, hidden states through net._tap"""
    inp, net = planted["inp"], _net()
    net.use_c_step = False
    taps = {}
    net._tap = lambda i, h: taps.__setitem__("emb" if i < 0 else f"h{i + 1}", h.float().cpu().clone())
    out = net.forward_f32(inp["x"].to(DEV), inp["t"].to(DEV), inp["ctx"].to(DEV), None, **_kw(inp))
    assert net._cstep is None and set(taps) == {"emb", "h1", "h2"}
    _check(capsys, "per-op path (use_c_step = False)", planted["bounds"], dict(taps, out=out), planted["ref"])


@pytest.mark.parametrize("cfg_pair", [False, True])
def test_c_step(planted, capsys, cfg_pair):
    """scail_dit_step (one C call), without and with the CFG-pair pruning"""
    inp, net = planted["inp"], _net()
    out = net.forward_f32(inp["x"].to(DEV), inp["t"].to(DEV), inp["ctx"].to(DEV), None, cfg_pair=cfg_pair, **_kw(inp))
    assert net._cstep is not None, "the C executor was not used"
    _check(capsys, f"scail_dit_step (cfg_pair = {cfg_pair})", planted["bounds"], dict(out=out), planted["ref"])


def test_c_block_local(planted, capsys):
    """scail_dit_block through CStep.block, layer by layer on the oracle's bf16-rounded block inputs: the block-local points"""
    from scail_amd import lib as L
    from scail_amd import ops
    from scail_amd.cstep import CStep
    from scail_amd.dit import _as_bf16
    cfg, inp, net = planted["cfg"], planted["inp"], _net()
    W = net.prepare()
    cs = CStep(net, W)
    temb = ops.timestep_embedding(inp["t"].to(DEV).float(), net.time_freq_dim)
    e1 = ops.small_linear(temb, W["time_embed.0.w"], W["time_embed.0.b"], act_out=L.ACT_SILU)
    emb = ops.small_linear(e1, W["time_embed.2.w"], W["time_embed.2.b"])
    adaln = ops.small_linear(emb, W["adaln_projection.1.w"], W["adaln_projection.1.b"], act_in=L.ACT_SILU)
    mod = ops.adaln_table(adaln, W["adaln_tables"])
    cond = net._conditioning(_as_bf16(inp["ctx"], DEV), _as_bf16(inp["clip"], DEV))
    cos, sin = net._rope(DW.T, DW.H // 2, DW.W // 2, 0, 0, torch.device(DEV))
    got = {}
    for i in range(cfg.num_layers):
        h = planted["block_inputs"][i].to(DEV).to(torch.bfloat16).contiguous()
        assert torch.equal(h.float().cpu(), planted["block_inputs"][i])
        got[f"blk{i}"] = cs.block(i, h, mod[i].contiguous(), cond, cos, sin)
    _check(capsys, "scail_dit_block (CStep.block)", planted["bounds"], got, planted["ref"])


def test_c_step_two_characters(capsys):
    """scail_dit_step_chars with two characters against the multi-character branch of the oracle (rope_tables_multi)"""
    cfg = DW.planted_config()
    sd, inp = DW.planted_state_dict(cfg), DW.planted_inputs(n_char=2)
    want = O.dit_forward(cfg, sd, inp["x"], inp["t"], inp["ctx"], inp["ref"], inp["pose"], inp["clip"])
    one = DW.planted_inputs()
    assert float((want - O.dit_forward(cfg, sd, one["x"], one["t"], one["ctx"], one["ref"], one["pose"], one["clip"])).abs().max()) > 0.1
    net = _net()
    out = net.forward_f32(inp["x"].to(DEV), inp["t"].to(DEV), inp["ctx"].to(DEV), None, **_kw(inp))
    assert net._cstep is not None
    _check(capsys, "scail_dit_step_chars (2 characters)", DW.bounds(n_char=2), dict(out=out), dict(out=want))


@pytest.mark.parametrize("mode", ["allgather", "ulysses"])
def test_sequence_parallel_virtual_ranks(planted, capsys, mode):
    """two virtual ranks (tests/test_parallel_gpu.py _run_ranks: H-chunked latents, rank-shifted RoPE, the executor's sequence-parallel
    step), gathered on rank 0"""
    from scail_amd.dit import _as_bf16
    from test_parallel_gpu import _run_ranks
    inp = planted["inp"]
    inputs = (inp["x"].to(DEV), inp["t"].to(DEV)) + tuple(_as_bf16(inp[k], DEV) for k in ("ctx", "ref", "pose", "clip"))
    out = _run_ranks(2, mode, _net, inputs, 3, use_c=True)
    _check(capsys, f"scail_dit_step_sp, 2 ranks {mode}", planted["bounds"], dict(out=out), planted["ref"])


def test_c_step_cached_fill(planted, capsys):
    """scail_dit_step_cached in FILL mode: the full evaluation that also leaves the block residual in the cache"""
    inp, net = planted["inp"], _net()
    out = net.forward_f32(inp["x"].to(DEV), inp["t"].to(DEV), inp["ctx"].to(DEV), None, step_cache="fill", **_kw(inp))
    _check(capsys, "scail_dit_step_cached (fill)", planted["bounds"], dict(out=out), planted["ref"])


def test_c_sample_two_steps(planted, capsys):
    """scail_dit_sample: two Euler steps with CFG 4 against O.sample at the final latent; the bound comes from the storage model run
    through the same two steps"""
    from scail_amd import sampler as S
    cfg, sd, inp, net = planted["cfg"], planted["sd"], planted["inp"], _net()
    b = DW.bounds(sampler=True)
    want = DW.oracle_sample(cfg, sd, inp)
    smp = S.RFSampler(hunyuan_schedule=True, shift_scale=int(DW.SHIFT_SCALE), num_steps=DW.SAMPLE_STEPS,
                      guider_config={"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": DW.CFG_SCALE}})
    assert torch.equal(smp.sigmas(), O.flow_sigmas(DW.SAMPLE_STEPS, DW.SHIFT_SCALE))
    x0, c_ctx, uc_ctx = DW.sample_args(inp)
    shared = _kw(inp)
    xT = smp.sample_hip(net, x0.to(DEV), dict(crossattn=c_ctx.to(DEV), **shared), dict(crossattn=uc_ctx.to(DEV), **shared))
    assert net._cstep is not None
    _check(capsys, "scail_dit_sample (2 steps, CFG 4)", b, dict(sample=xT), dict(sample=want))
