"""Tiled long-clip sampling (RFSamplerLong, temporal tiling; reference sampling.py:986-1085) in ONE executor call: the three fp32 row
kernels (include/scail_hip.h scail_tile_*) against the torch expressions they replace, scail_dit_sample_tiled (include/scail_dit.h)
against the host loop of scail_amd/sampler.py -- the same kernels in the same order with every elementwise operation rounded on its own,
so the yardstick is EQUALITY -- and against the reference's golden, and the CLI's route for a pose clip longer than one window."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import scail_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUIDER = {"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": 4}}


def _load(golden_dir, name):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(golden_dir, name)).items()}


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


def _cos(a, b):
    a, b = a.flatten().double(), b.flatten().double()
    return float((a @ b) / (a.norm() * b.norm()))


class _Calls:
    """counts the calls of CStep methods (which executor entry points a request reached)"""

    def __init__(self, monkeypatch, *names):
        from scail_amd.cstep import CStep
        self.n = {k: 0 for k in names}
        for k in names:
            monkeypatch.setattr(CStep, k, self._wrap(k, getattr(CStep, k)))

    def _wrap(self, name, orig):
        def f(cs, *a, **kw):
            self.n[name] += 1
            return orig(cs, *a, **kw)
        return f


def _sampler(steps, shift=5):
    from scail_amd import sampler as S
    return S.RFSamplerLong(hunyuan_schedule=True, shift_scale=shift, num_steps=steps, guider_config=GUIDER)


def _both_routes(smp, net, x0, c, uc, tiles, calls, steps):
    """(one-call result, host-loop result); the host loop is forced with a step_callback"""
    before = dict(calls.n)
    xT = smp.sample_hip(net, x0, c, uc, tile_indices=tiles)
    assert calls.n["sample_tiled"] == before["sample_tiled"] + 1 and calls.n["step"] == before["step"], "the one-call route was not taken"
    seen = []
    xT_loop = smp.sample_hip(net, x0, c, uc, tile_indices=tiles, step_callback=lambda i, xx: seen.append(i))
    assert seen == list(range(steps)) and calls.n["sample_tiled"] == before["sample_tiled"] + 1
    assert calls.n["step"] == before["step"] + steps * len(tiles)
    return xT, xT_loop


# ---- 1. the operators against the torch expressions of RFSamplerLong.sample_hip ---------------------------------------------------------
def test_tile_operators_equal_the_torch_expressions():
    from scail_amd import ops
    from scail_amd.sampler import RFSamplerLong as R
    g = torch.Generator().manual_seed(5)
    # a frame of 16 * 5 * 7 = 560 floats: neither F nor T * F is a multiple of the 256-thread block
    T, Tt, C, H, W = 9, 5, 16, 5, 7
    assert (C * H * W) % 256 != 0 and (T * C * H * W) % 256 != 0
    x = torch.randn(1, T, C, H, W, generator=g).to(DEV)
    idx = [7, 2, 8, 0, 4]                                  # unsorted
    it = torch.as_tensor(idx, device=DEV, dtype=torch.long)
    # gather (+ the CFG twin)
    xt = x[:, it]
    assert torch.equal(ops.tile_gather(x, idx), torch.cat([xt, xt], 0))
    # blend-accumulate: cfg and the weights are not powers of two, so a contracted multiply-add would show
    cfg = 3.7
    weight = R.tile_weight(Tt, DEV)[:, None, None, None]
    v = torch.randn(2, Tt, C, H, W, generator=g).to(DEV)
    den0 = torch.randn(1, T, C, H, W, generator=g).to(DEV)
    n_diff_fma = 0
    for m in (1, 2):
        want = den0.clone()
        d = v[0:1] + cfg * (v[1:2] - v[0:1])
        want[:, it] += (m * weight) * d
        got = ops.tile_blend_acc_(den0.clone(), v, idx, (m * weight).flatten().cpu(), cfg)
        assert torch.equal(got, want), f"blend-accumulate (m = {m}): max |d| {float((got - want).abs().max())}"
        untouched = [f for f in range(T) if f not in idx]
        assert torch.equal(got[:, untouched], den0[:, untouched])
        # what contraction would give (the data must be able to tell): a * b + c in one rounding, emulated in fp64
        fma = (v[0:1].double() + float(np.float32(cfg)) * (v[1:2] - v[0:1]).double()).float()
        n_diff_fma += int((fma != d).sum())
    assert n_diff_fma > 0, "the data cannot tell a contracted multiply-add from separate roundings"
    # finish: x + dsigma * (den * inv), and den left zeroed
    wsum = torch.zeros(T, device=DEV)
    for k, t in enumerate(([0, 1, 2, 3, 4], [2, 3, 4, 5, 6], [4, 5, 6, 7, 8])):
        wsum[torch.as_tensor(t, device=DEV)] += R._mult(k, 3) * weight[:, 0, 0, 0]
    inv = (1.0 / wsum)[:, None, None, None]
    ds = -0.0371
    den = torch.randn(1, T, C, H, W, generator=g).to(DEV)
    want = x + float(np.float32(ds)) * (den * inv)
    xg, dg = x.clone(), den.clone()
    ops.tile_finish_(xg, dg, inv.flatten().cpu(), float(np.float32(ds)))
    assert torch.equal(xg, want), f"finish: max |d| {float((xg - want).abs().max())}"
    assert int(dg.count_nonzero()) == 0
    # more than 64 frames: the finish pass goes in launches of 64 frames' factors
    T2 = 70
    x2, d2 = torch.randn(1, T2, 3, 5, generator=g).to(DEV), torch.randn(1, T2, 3, 5, generator=g).to(DEV)
    inv2 = (torch.rand(T2, generator=g) + 0.3).to(DEV)
    want2 = x2 + float(np.float32(ds)) * (d2 * inv2[:, None, None])
    ops.tile_finish_(x2, d2, inv2.cpu(), float(np.float32(ds)))
    assert torch.equal(x2, want2) and int(d2.count_nonzero()) == 0
    # the weights of the one-call route are the host loop's, formed on the device: fetched values are those bits
    assert torch.equal(weight.flatten().cpu().to(DEV), weight.flatten())


# ---- 2. the golden's inputs: 6-frame latent, three 4-frame tiles, 2 steps --------------------------------------------------------------
def _golden_request(golden_dir, **kw):
    g = _load(golden_dir, "sampler_long_tiny.npz")
    d = _load(golden_dir, "dit_tiny.npz")
    net = _net_golden(O.TINY, int(d["seed"]), **kw)
    tiles = [list(map(int, r)) for r in g["tiles"]]
    shared = dict(concat_images=torch.zeros(1, 4, 16, 8, 8, device=DEV), ref_concat=d["ref"].to(DEV), smpl_tiled=g["smpl_tiled"].to(DEV),
                  image_clip_features=d["clip"].to(DEV))
    c = dict(crossattn=g["c_ctx"].to(DEV), **shared)
    uc = dict(crossattn=g["uc_ctx"].to(DEV), **shared)
    return g, net, tiles, c, uc


def test_one_call_equals_the_host_loop_and_the_reference_golden(golden_dir, monkeypatch, capsys):
    calls = _Calls(monkeypatch, "sample_tiled", "sample", "step")
    g, net, tiles, c, uc = _golden_request(golden_dir)
    assert g["x0"].shape[1] == 6 and len(tiles) == 3 and len(tiles[0]) == 4
    xT, xT_loop = _both_routes(_sampler(2), net, g["x0"].to(DEV), c, uc, tiles, calls, 2)
    with capsys.disabled():
        print(f"\ntiled one-call vs host loop: max |d| {float((xT - xT_loop).abs().max()):.3e}; vs the reference golden: max |d| "
              f"{float((xT.cpu() - g['xT']).abs().max()):.4f} mean |d| {float((xT.cpu() - g['xT']).abs().mean()):.5f} cosine {_cos(xT.cpu(), g['xT']):.6f}")
    assert torch.isfinite(xT).all() and not torch.equal(xT.cpu(), g["x0"])
    assert torch.equal(xT, xT_loop), f"max |d| {float((xT - xT_loop).abs().max())}"
    # the bars of tests/test_dit_gpu.py test_sampler_long_vs_reference_golden
    torch.testing.assert_close(xT.cpu(), g["xT"], rtol=3e-2, atol=0.14)
    assert _cos(xT.cpu(), g["xT"]) >= 0.999
    assert float((xT.cpu() - g["xT"]).abs().mean()) < 1.5e-2
    # a real handle: the workspace check names both sizes
    from scail_amd import lib as L
    need = net._cstep.sample_tiled_workspace_bytes(6, 4, 8, 8)
    assert need > net._cstep.workspace_bytes(2, 4, 8, 8)
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    a = ctypes.c_void_p(ws.data_ptr())
    fr, tw, iw = net._cstep.tile_tables(tiles, torch.ones(3, 4), torch.ones(6))
    with pytest.raises(L.ScailHipError, match=rf"workspace too small: {need - 1} bytes, needs {need}\b"):
        L.call("scail_dit_sample_tiled", net._cstep._h, a, a, a, 2, 4.0, a, a, a, fr, tw, iw, 3, 6, 4, a, a, 8, 8, a, need - 1, None)


def test_one_call_with_interleaved_index_lists_equals_the_host_loop(golden_dir, monkeypatch):
    """tile_indices are arbitrary index lists in the reference: interleaved, unsorted frames"""
    calls = _Calls(monkeypatch, "sample_tiled", "sample", "step")
    g, net, _, c, uc = _golden_request(golden_dir)
    tiles = [[4, 0, 2, 5], [1, 3, 5, 0], [5, 2, 4, 1]]
    xT, xT_loop = _both_routes(_sampler(2), net, g["x0"].to(DEV), c, uc, tiles, calls, 2)
    assert torch.isfinite(xT).all()
    assert torch.equal(xT, xT_loop), f"max |d| {float((xT - xT_loop).abs().max())}"


def test_one_call_fp8_equals_the_host_loop(golden_dir, monkeypatch, capsys):
    calls = _Calls(monkeypatch, "sample_tiled", "sample", "step")
    g, net, tiles, c, uc = _golden_request(golden_dir, gemm_precision="fp8")
    xT, xT_loop = _both_routes(_sampler(2), net, g["x0"].to(DEV), c, uc, tiles, calls, 2)
    assert net._cstep is not None and net._cstep._fp8_buf is not None
    cs = _cos(xT.cpu(), g["xT"])
    with capsys.disabled():
        print(f"\nfp8 tiled one-call: cosine vs the reference golden {cs:.6f}, max |d| {float((xT.cpu() - g['xT']).abs().max()):.4f}")
    assert torch.equal(xT, xT_loop), f"max |d| {float((xT - xT_loop).abs().max())}"
    assert cs >= 0.98          # the bar tests/test_fp8_gpu.py sets for an fp8-sampled latent against a reference golden


# ---- 3. a wider case on BASELINE config 1's network ---------------------------------------------------------------------------------------
def test_one_call_equals_the_host_loop_config1_four_tiles(monkeypatch):
    from scail_amd.cli import plan_tiles
    calls = _Calls(monkeypatch, "sample_tiled", "sample", "step")
    net = _net_golden(O.CONFIG1, 77)
    T, Tt, H, W, steps = 9, 3, 16, 24, 3                 # Tt = 3: the triangular weights are not dyadic
    tiles = plan_tiles(T, Tt, 1)
    assert len(tiles) == 4
    gg = torch.Generator().manual_seed(9)
    r = lambda *s: torch.randn(*s, generator=gg)
    shared = dict(concat_images=torch.zeros(1, device=DEV), ref_concat=r(1, 1, 16, H, W).to(DEV).to(torch.bfloat16),
                  smpl_tiled=r(1, len(tiles), Tt, 16, H // 2, W // 2).to(DEV).to(torch.bfloat16),
                  image_clip_features=r(1, 5, 1280).to(DEV).to(torch.bfloat16))
    c = dict(crossattn=r(1, 12, 64).to(DEV).to(torch.bfloat16), **shared)
    uc = dict(crossattn=r(1, 12, 64).to(DEV).to(torch.bfloat16), **shared)
    x0 = r(1, T, 16, H, W).to(DEV)
    xT, xT_loop = _both_routes(_sampler(steps), net, x0, c, uc, tiles, calls, steps)
    assert torch.isfinite(xT).all() and not torch.equal(xT, x0)
    assert torch.equal(xT, xT_loop), f"max |d| {float((xT - xT_loop).abs().max())}"


def test_two_characters_with_tiles_keep_the_host_loop(monkeypatch):
    """tiles combined with several characters are outside scail_dit_sample_tiled: such a request runs the Python loop, as it did before
    the one-call route existed (one scail_dit_step_chars evaluation per tile and step)"""
    from scail_amd.dit import DiffusionTransformer
    calls = _Calls(monkeypatch, "sample_tiled", "sample", "step")
    net = DiffusionTransformer(transformer_args=dict(model_parallel_size=1), num_frames=81, latent_width=300, latent_height=300, share_adaln=True,
                               use_i2v_clip=True, device=DEV, init_seed=78, num_layers=2, hidden_size=256, num_attention_heads=2,
                               inner_hidden_size=512, text_dim=64, time_freq_dim=256, time_embed_dim=256)
    T, Tt, H, W, C, steps = 5, 3, 8, 20, 2, 2
    tiles = [[0, 1, 2], [2, 3, 4]]
    gg = torch.Generator().manual_seed(13)
    r = lambda *s: torch.randn(*s, generator=gg)
    shared = dict(concat_images=torch.zeros(1, device=DEV), ref_concat=r(1, C, 16, H, W).to(DEV).to(torch.bfloat16),
                  smpl_tiled=r(1, len(tiles), C * Tt, 16, H // 2, W // 2).to(DEV).to(torch.bfloat16),
                  image_clip_features=r(1, 5, 1280).to(DEV).to(torch.bfloat16))
    c = dict(crossattn=r(1, 12, 64).to(DEV).to(torch.bfloat16), **shared)
    uc = dict(crossattn=r(1, 12, 64).to(DEV).to(torch.bfloat16), **shared)
    x0 = r(1, T, 16, H, W).to(DEV)
    smp = _sampler(steps)
    xT = smp.sample_hip(net, x0, c, uc, tile_indices=tiles)
    assert calls.n == {"sample_tiled": 0, "sample": 0, "step": steps * len(tiles)}
    assert xT.shape == x0.shape and torch.isfinite(xT).all() and not torch.equal(xT, x0)
    # the same request with the loop forced: the same bits
    assert torch.equal(xT, smp.sample_hip(net, x0, c, uc, tile_indices=tiles, step_callback=lambda i, xx: None))


# ---- 4. capture --------------------------------------------------------------------------------------------------------------------------
def test_one_call_replays_from_a_graph(golden_dir):
    from scail_amd import lib as L
    from scail_amd.cstep import _cond_struct
    from scail_amd.sampler import RFSamplerLong as R
    g, net, tiles, c, uc = _golden_request(golden_dir)
    steps, T, Tt, H, W = 2, 6, 4, 8, 8
    smp = _sampler(steps)
    x0 = g["x0"].to(DEV)
    xT = smp.sample_hip(net, x0, c, uc, tile_indices=tiles)           # eager (also the warm-up of every kernel and table)
    cs = net._cstep
    sig = smp.sigmas(steps).float().cpu()
    ts = (sig[:-1] * 1000.0).repeat_interleave(2).to(DEV).contiguous()
    dsa = (ctypes.c_float * steps)(*[float(v) for v in (sig[1:] - sig[:-1])])
    weight = R.tile_weight(Tt, DEV)
    tile_w = torch.stack([R._mult(k, 3) * weight for k in range(3)])
    wsum = torch.zeros(T, device=DEV)
    for k in range(3):
        wsum[torch.as_tensor(tiles[k], device=DEV)] += tile_w[k]
    fr, tw, iw = cs.tile_tables(tiles, tile_w, 1.0 / wsum)
    ctx = torch.cat((uc["crossattn"], c["crossattn"]), 0).to(torch.bfloat16).contiguous()
    cond = net._conditioning(ctx, c["image_clip_features"].to(torch.bfloat16).contiguous(), None)
    cc = _cond_struct(cond)
    cos, sin = net._rope(Tt, H // 2, W // 2, 0, 0, torch.device(DEV), 1)
    ref = c["ref_concat"].to(torch.bfloat16).contiguous()
    pose = c["smpl_tiled"].to(torch.bfloat16).contiguous()
    ws = torch.empty(cs.sample_tiled_workspace_bytes(T, Tt, H, W), device=DEV, dtype=torch.uint8)
    xg = x0.clone()

    def run():
        L.call("scail_dit_sample_tiled", cs._h, xg.data_ptr(), ts.data_ptr(), ctypes.cast(dsa, ctypes.c_void_p), steps, 4.0, ctypes.byref(cc),
               ref.data_ptr(), pose.data_ptr(), fr, tw, iw, 3, T, Tt, cos.data_ptr(), sin.data_ptr(), H, W, ws.data_ptr(), ws.numel(),
               torch.cuda.current_stream().cuda_stream)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                  # warm-up on the capture stream
    torch.cuda.synchronize()
    assert torch.equal(xg, xT)
    xg.copy_(x0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        run()
    for n in (1, 2):
        xg.copy_(x0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(xg, xT), f"graph replay {n}: max |d| {float((xg - xT).abs().max())}"


# ---- 5. the request path -----------------------------------------------------------------------------------------------------------------
def _write_request(tmp_path, frames, seed=0):
    from PIL import Image
    g = np.random.default_rng(seed)
    Image.fromarray(g.integers(0, 255, (80, 120, 3), dtype=np.uint8)).save(tmp_path / "ref.jpg")
    np.save(tmp_path / f"rendered{frames}.npy", g.integers(0, 255, (frames, 70, 90, 3), dtype=np.uint8))
    return str(tmp_path / "ref.jpg"), str(tmp_path / f"rendered{frames}.npy")


def test_cli_long_clip_end_to_end(tmp_path, monkeypatch):
    """--tiny (13-frame window = 4 latent frames): a 25-frame pose clip is sampled in three windows through the one-call route, the
    latent equals the same request assembled by hand on the host loop; the video has 25 frames"""
    from scail_amd import cli, sampler as S, video_io
    calls = _Calls(monkeypatch, "sample_tiled", "sample", "step")
    ref, pose = _write_request(tmp_path, 25)
    cli.main(["--tiny", "--ref-image", ref, "--pose-video", pose, "--tile-frames", "13", "--tile-overlap", "8", "--steps", "2",
              "--out", str(tmp_path / "out.pt"), "--save-dir", str(tmp_path / "vid"), "--format", ".npy"])
    assert calls.n == {"sample_tiled": 1, "sample": 0, "step": 0}
    out = torch.load(tmp_path / "out.pt")
    z_cli, video = out["latent"], out["video"]
    assert z_cli.shape == (1, 16, 7, 8, 8) and video.shape == (1, 3, 25, 64, 64)
    assert torch.isfinite(video).all() and 0.0 <= float(video.min()) and float(video.max()) <= 1.0
    back = video_io.load_video_for_pose_sample(str(tmp_path / "vid" / "0_output_000000.npy"))
    assert back.shape[0] == 25
    # the same request by hand: windows [0..3], [2..5], [3..6] in latent frames, each window's pose frames encoded on its own,
    # engine.sample with tile_indices on the HOST LOOP (forced with a step callback)
    tiles = cli.plan_tiles(7, 4, 2)
    assert tiles == [[0, 1, 2, 3], [2, 3, 4, 5], [3, 4, 5, 6]]
    cfg = copy.deepcopy(cli.TINY)
    engine = cli.build_engine(cfg)
    req = cli.request_from_files(ref, pose, cfg, seed=1234, text_dim=engine.network.text_dim)[0]          # the CLI's default --seed
    enc = lambda v: engine.encode_first_stage(v.unsqueeze(0), None, force_encode=True).permute(0, 2, 1, 3, 4).contiguous().to(torch.bfloat16)
    smpl_tiled = torch.stack([enc(req["pose"][:, 4 * t[0]:4 * t[-1] + 1]) for t in tiles], 1)
    assert smpl_tiled.shape == (1, 3, 4, 16, 4, 4)
    shared = dict(concat_images=torch.zeros(1, device=DEV), ref_concat=enc(req["ref"]), smpl_tiled=smpl_tiled,
                  image_clip_features=req["clip"].to(torch.bfloat16))
    c, uc = dict(crossattn=req["context"], **shared), dict(crossattn=req["uncond_context"], **shared)

    class HostLoop(S.RFSamplerLong):
        def sample_hip(self, *a, **kw):
            return super().sample_hip(*a, step_callback=lambda i, x: None, **kw)

    params = dict(cfg["model"]["sampler_config"]["params"])
    engine.sampler = HostLoop(**params)
    torch.manual_seed(1234)
    z = engine.sample(c, uc=uc, batch_size=1, shape=(7, 16, 8, 8), num_steps=2, tile_indices=tiles)
    assert calls.n == {"sample_tiled": 1, "sample": 0, "step": 2 * 3}
    z = z.permute(0, 2, 1, 3, 4).contiguous().cpu()
    assert torch.equal(z_cli, z), f"max |d| {float((z_cli.float() - z.float()).abs().max())}"


def test_cli_clip_of_one_window_takes_the_plain_path(tmp_path, monkeypatch):
    """a 13-frame clip with a 13-frame window: no tiling, no sampler swap -- the bits of the plain request path"""
    from scail_amd import cli, sampler as S
    calls = _Calls(monkeypatch, "sample_tiled", "sample", "step")
    ref, pose = _write_request(tmp_path, 13)
    cfg = copy.deepcopy(cli.TINY)
    engine = cli.build_engine(cfg)
    plain = engine.sampler
    assert type(plain) is S.RFSampler
    req = cli.request_from_files(ref, pose, cfg, text_dim=engine.network.text_dim)[0]
    video, z, _ = cli.run(cfg, dict(req), steps=2, engine=engine, tile_frames=13, tile_overlap=8)
    assert engine.sampler is plain and calls.n == {"sample_tiled": 0, "sample": 1, "step": 0}
    assert z.shape == (1, 16, 4, 8, 8) and video.shape == (1, 3, 13, 64, 64)
    # the plain path by hand (the body of cli.run before this route existed)
    enc = lambda v: engine.encode_first_stage(v.unsqueeze(0), None, force_encode=True).permute(0, 2, 1, 3, 4).contiguous().to(torch.bfloat16)
    ref_concat, pose_latent = enc(req["ref"]), enc(req["pose"])
    shared = dict(concat_images=torch.zeros(1, device=DEV), ref_concat=ref_concat, concat_pose=pose_latent, concat_smpl_render=pose_latent,
                  image_clip_features=req["clip"].to(torch.bfloat16))
    torch.manual_seed(1234)
    z2 = engine.sample(dict(crossattn=req["context"], **shared), uc=dict(crossattn=req["uncond_context"], **shared), batch_size=1,
                       shape=(4, 16, 8, 8), num_steps=2)
    assert torch.equal(z, z2.permute(0, 2, 1, 3, 4).contiguous())
    # after a tiled request on the same engine the configured sampler is back
    ref25, pose25 = _write_request(tmp_path, 25, seed=1)
    req25 = cli.request_from_files(ref25, pose25, cfg, text_dim=engine.network.text_dim)[0]
    video25, z25, _ = cli.run(cfg, req25, steps=2, engine=engine)          # defaults: the network's 13-frame window, half overlap
    assert engine.sampler is plain and calls.n["sample_tiled"] == 1
    assert z25.shape == (1, 16, 7, 8, 8) and video25.shape == (1, 3, 25, 64, 64) and torch.isfinite(video25).all()
