"""The step cache for clips longer than one window (include/scail_dit.h scail_dit_sample_tiled_cached): one plan for every temporal tile,
one block residual per tile, one shared embedding region.

Every comparison is bit equality.  The comparison is built here from entry points that exist without the tiled cache: ops.tile_gather,
CStep.step_cached (cfg_pair, on a cache of its own per tile) in "fill" / "reuse" mode, ops.tile_blend_acc_, ops.tile_finish_, with the
schedule values the binding hands the library.  Toy networks (3 layers, D 512 / 256); tiles of Ltok 190 and one of 882."""
import copy
import ctypes

import pytest
import torch

import ws_contract as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
bf16 = torch.bfloat16

TOY = dict(hidden_size=512, num_attention_heads=4, inner_hidden_size=1024, text_dim=64, time_freq_dim=256, time_embed_dim=512)   # test_ws_contract_gpu.TOY
TINY2 = dict(hidden_size=256, num_attention_heads=2, inner_hidden_size=512, text_dim=64, time_freq_dim=256, time_embed_dim=256)  # test_ws_contract_gpu.TINY2
SIG4 = torch.tensor([1.0, 0.8, 0.55, 0.3, 0.0])
SIG6 = torch.tensor([1.0, 0.9, 0.75, 0.6, 0.4, 0.2, 0.0])
CFG = 4.0

# name -> (network, T, H, W, tiles); a tile of (3, 8, 20) has Ltok 190, one of (2, 28, 36) Ltok 882 (above the 768-row boundary of the
# attention plan)
CASES = {
    "small": ("toy", 5, 8, 20, [[0, 1, 2], [1, 2, 3], [2, 3, 4]]),
    "interleaved": ("tiny2", 5, 8, 20, [[4, 0, 2], [1, 3, 0], [2, 4, 1]]),          # unordered index lists, as the reference allows
    "four": ("tiny2", 6, 8, 20, [[0, 1, 2], [1, 2, 3], [2, 3, 4], [3, 4, 5]]),
    "large": ("toy", 3, 28, 36, [[0, 1], [1, 2]]),
}
MASKS = {"0101": [0, 1, 0, 1], "0110": [0, 1, 1, 0], "001110": [0, 0, 1, 1, 1, 0], "0000": [0, 0, 0, 0]}
# every mask on the smallest shape; the other shapes under one mask each
RUNS = [("small", m) for m in MASKS] + [("interleaved", "0110"), ("four", "0101"), ("large", "0110")]

_nets = {}


def _net(kind="toy", **kw):
    import test_parallel_gpu as P
    key = (kind,) + tuple(sorted(kw.items()))
    if key not in _nets:
        _nets[key] = P._mk(dict(TOY if kind == "toy" else TINY2, **kw), 3, seed=77)
    return _nets[key]


def _sig(mask):
    return SIG4 if len(mask) == 4 else SIG6


def _request(case, seed=21):
    """(x0 (1,T,16,H,W) fp32, ctx (2,12,64), ref (1,1,16,H,W), pose_tiles (1,n_tiles,Tt,16,H/2,W/2) -- random, so every tile has its own --,
    clip (1,5,1280), tiles, tile_w (n_tiles,Tt) and inv_wsum (T) as RFSamplerLong forms them)"""
    from scail_amd.sampler import RFSamplerLong
    _, T, H, Wd, tiles = CASES[case]
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    x0 = r(1, T, 16, H, Wd).to(DEV)
    ctx = r(2, 12, 64).to(DEV).to(bf16)
    ref = r(1, 1, 16, H, Wd).to(DEV).to(bf16)
    pose = r(1, len(tiles), len(tiles[0]), 16, H // 2, Wd // 2).to(DEV).to(bf16)
    clip = r(1, 5, 1280).to(DEV).to(bf16)
    _, tile_w, inv_wsum = RFSamplerLong(hunyuan_schedule=True)._tile_table(tiles, T, DEV)
    return x0, ctx, ref, pose, clip, tiles, tile_w.cpu(), inv_wsum.cpu()


def _compose(net, req, sig, mask):
    """The comparison: the tiled loop on the host, tile k's evaluation a CStep.step_cached on a cache that belongs to tile k alone.
    -> (final latent, [cache of tile k])"""
    from scail_amd import ops
    x0, ctx, ref, pose, clip, tiles, tile_w, inv_wsum = req
    ex = net._executor()
    Tt, H, Wd = len(tiles[0]), x0.shape[3], x0.shape[4]
    cond = net._conditioning(ctx, clip, None)
    cos, sin = net._rope(Tt, H // 2, Wd // 2, 0, 0, torch.device(DEV), 1)
    need = ex.step_cache_bytes(2, Tt, H, Wd)
    caches = [torch.full((need,), 0xFF, device=DEV, dtype=torch.uint8) for _ in tiles]
    sig = sig.float().cpu()
    x = x0.clone()
    den = torch.zeros_like(x)
    for i in range(len(mask)):
        t = (sig[i] * 1000.0).repeat(2).to(DEV)
        for k, fr in enumerate(tiles):
            xin = ops.tile_gather(x, fr)
            v = ex.step_cached(xin, t, cond, ref, pose[:, k].contiguous(), cos, sin, "reuse" if mask[i] else "fill", cfg_pair=True,
                               cache=caches[k])
            ops.tile_blend_acc_(den, v, fr, tile_w[k], CFG)
        ops.tile_finish_(x, den, inv_wsum, float(sig[i + 1] - sig[i]))
    torch.cuda.synchronize()
    return x, caches


def _cached_call(net, req, sig, mask):
    x0, ctx, ref, pose, clip, tiles, tile_w, inv_wsum = req
    return net.sample_tiled_c(x0, sig, CFG, ctx, ref, pose, clip, tiles, tile_w, inv_wsum, reuse=mask)


def _slabs(net, req):
    x0, _, _, _, _, tiles, _, _ = req
    ex = net._executor()
    return [ex.tile_cache_residual(k, len(tiles), len(tiles[0]), x0.shape[3], x0.shape[4], net.hidden_size).clone() for k in range(len(tiles))]


_results = {}


def _result(case, mask_name, **kw):
    """one cached call and its comparison per (case, mask, network options), shared by the tests below and left unchanged:
    dict(got, slabs, want, want_r, req, net)"""
    key = (case, mask_name) + tuple(sorted(kw.items()))
    if key not in _results:
        net, req, mask = _net(CASES[case][0], **kw), _request(case), MASKS[mask_name]
        want, caches = _compose(net, req, _sig(mask), mask)
        net._executor()._tile_cache = None
        got = _cached_call(net, req, _sig(mask), mask).clone()
        torch.cuda.synchronize()
        n = 2 * len(req[5][0]) * (req[0].shape[3] // 2) * (req[0].shape[4] // 2) * net.hidden_size
        want_r = [c[:2 * n].view(bf16).view(2, -1, net.hidden_size).clone() for c in caches]
        _results[key] = dict(got=got, slabs=_slabs(net, req), want=want, want_r=want_r, req=req, net=net)
        net._executor()._tile_cache = None
    return _results[key]


def _bits(t):
    return t.detach().contiguous().view(torch.int16)


# ---- 1. a plan without reuse is scail_dit_sample_tiled ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_all_zero_mask_is_the_uncached_tiled_sampler(case):
    net, req = _net(CASES[case][0]), _request(case)
    x0, ctx, ref, pose, clip, tiles, tile_w, inv_wsum = req
    plain = net.sample_tiled_c(x0, SIG4, CFG, ctx, ref, pose, clip, tiles, tile_w, inv_wsum).clone()
    got = _cached_call(net, req, SIG4, [0, 0, 0, 0])
    net._executor()._tile_cache = None
    assert bool(torch.isfinite(got).all()) and not torch.equal(got, x0)
    assert torch.equal(got, plain), f"differs from scail_dit_sample_tiled in {int((got != plain).sum())} values"


# ---- 2. every mask against the composition ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mask_name", RUNS)
def test_final_latent_equals_the_composition(case, mask_name):
    r = _result(case, mask_name)
    assert bool(torch.isfinite(r["got"]).all()) and not torch.equal(r["got"], r["req"][0])
    assert torch.equal(r["got"], r["want"]), f"differs from the composition in {int((r['got'] != r['want']).sum())} values"
    if any(MASKS[mask_name]):
        x0, ctx, ref, pose, clip, tiles, tile_w, inv_wsum = r["req"]
        plain = r["net"].sample_tiled_c(x0, _sig(MASKS[mask_name]), CFG, ctx, ref, pose, clip, tiles, tile_w, inv_wsum)
        assert not torch.equal(r["got"], plain), "the mask skipped nothing"


# ---- 3. slab k holds tile k's residual --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mask_name", RUNS)
def test_residual_slabs_equal_the_compositions_caches(case, mask_name):
    r = _result(case, mask_name)
    n = len(r["slabs"])
    assert n == len(CASES[case][4]) == len(r["want_r"])
    for k in range(n):
        assert bool(torch.isfinite(r["slabs"][k].float()).all())
        assert torch.equal(_bits(r["slabs"][k]), _bits(r["want_r"][k])), f"slab {k} is not the residual of tile {k}"
    for k in range(n):
        for j in range(k + 1, n):
            assert not torch.equal(_bits(r["want_r"][k]), _bits(r["want_r"][j])), f"tiles {k} and {j} have the same residual: the data cannot tell a swapped slab"


# ---- 4. quantised GEMMs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp8", "fp6"])
def test_quantised_gemms_equal_the_composition(precision):
    r = _result("small", "0110", gemm_precision=precision)
    assert r["net"]._cstep._fp8_buf is not None
    assert bool(torch.isfinite(r["got"]).all())
    assert torch.equal(r["got"], r["want"]), f"differs from the composition in {int((r['got'] != r['want']).sum())} values"
    for k in range(len(r["slabs"])):
        assert torch.equal(_bits(r["slabs"][k]), _bits(r["want_r"][k])), f"slab {k}"
    assert not torch.equal(r["got"], _result("small", "0110")["got"]), "the quantised network gave the bf16 bits"


# ---- 5. the guarded-workspace contract --------------------------------------------------------------------------------------------------------
def test_poisoned_guarded_workspace_and_cache():
    """workspace and cache at exactly the queried sizes between guard bands, once per fill: were a slab read before its FILL wrote it, or the
    shared embedding region before its copy, the fills would differ"""
    net, req = _net("toy"), _request("small")
    ex = net._executor()
    x0, ctx, ref, pose, clip, tiles, tile_w, inv_wsum = req
    mask = MASKS["001110"]

    def run():
        ex._tile_cache = None
        out = _cached_call(net, req, SIG6, mask).clone()
        torch.cuda.synchronize()
        return out

    before = W.snapshot(dict(net=net, req=list(req)))
    plain = run()
    W.assert_unchanged(before)
    snap = W.snapshot(dict(net=net, prepared=net._prepared, cond=net._cond_cache, rope=net._rope_cache, req=list(req)))
    got = {}
    for name, fill in W.FILLS.items():
        with W.poisoned(fill) as s:
            got[name] = run()
            s.check()
            cache_ws = [ws for what, ws in s.workspaces if "scail_dit_sample_tiled_cache_bytes" in what]
            step_ws = [ws for what, ws in s.workspaces if "scail_dit_sample_tiled_workspace_bytes" in what]
            assert len(cache_ws) == 1 and cache_ws[0].numel() == ex.sample_tiled_cache_bytes(3, 3, 8, 20), "one cache, at exactly the queried size"
            assert len(step_ws) == 1 and step_ws[0].numel() == ex.sample_tiled_workspace_bytes(5, 3, 8, 20)
            assert len(s.workspaces) == 2
    ex._tile_cache = None
    for name, o in got.items():
        assert bool(torch.isfinite(o).all()), f"fill {name}: non-finite output"
        assert torch.equal(o, got["zero"]), f"fill {name} differs from fill zero in {int((o != got['zero']).sum())} values"
        assert torch.equal(o, plain), f"fill {name} differs from the plain run in {int((o != plain).sum())} values"
    assert torch.equal(plain, _result("small", "001110")["want"])
    W.assert_unchanged(snap)


# ---- 6. refusals leave everything as it was ---------------------------------------------------------------------------------------------------
def test_refused_calls_touch_nothing():
    from scail_amd import lib as L
    net, req = _net("toy"), _request("small")
    ex = net._executor()
    x0, ctx, ref, pose, clip, tiles, tile_w, inv_wsum = req
    cond = net._conditioning(ctx, clip, None)
    cos, sin = net._rope(3, 4, 10, 0, 0, torch.device(DEV), 1)
    need = ex.sample_tiled_cache_bytes(3, 3, 8, 20)
    key = (3, 3, 8, 20, torch.device(DEV, torch.cuda.current_device()))
    x = x0.clone()
    call = lambda m: ex.sample_tiled_cached(x, SIG4, CFG, cond, ref, pose, tiles, tile_w, inv_wsum, cos, sin, m)
    # no cache held: a refused plan leaves none behind
    ex._tile_cache = None
    with pytest.raises(L.ScailHipError, match=r"scail_dit_sample_tiled_cached: reuse\[0\] = 1"):
        call([1, 0, 0, 0])
    assert ex._tile_cache is None, "a refused call left a new cache in the binding"
    with pytest.raises(L.ScailHipError, match=r"reuse\[2\] = 2"):
        call([0, 1, 2, 0])
    assert ex._tile_cache is None
    with pytest.raises(L.ScailHipError, match="one entry per step"):
        call([0, 1])
    # a pre-filled cache: one byte short, and a bad plan on a full-size one
    buf, check = W.guarded(need, 0x47, DEV)
    held = (key, buf[:need - 1])
    ex._tile_cache = held
    with pytest.raises(L.ScailHipError, match=rf"cache too small: {need - 1} bytes, needs {need} \(scail_dit_sample_tiled_cache_bytes\)"):
        call([0, 1, 1, 0])
    assert ex._tile_cache is held
    ex._tile_cache = (key, buf)
    with pytest.raises(L.ScailHipError, match=r"reuse\[0\] = 1"):
        call([1, 1, 1, 0])
    torch.cuda.synchronize()
    check("a refused cache")
    assert W.holds_fill(buf, 0x47), "a refused call wrote into the cache"
    assert torch.equal(x, x0), "a refused call changed the latent"
    ex._tile_cache = None
    # the network's own refusals come first (the per-block seam has no cached form)
    net._c_blocks = True
    try:
        with pytest.raises(NotImplementedError, match="step_cache"):
            _cached_call(net, req, SIG4, [0, 1, 1, 0])
    finally:
        net._c_blocks = False
    assert ex._tile_cache is None


# ---- 7. capture -------------------------------------------------------------------------------------------------------------------------------
def test_cached_call_replays_from_a_graph():
    from scail_amd import lib as L
    from scail_amd.cstep import _cond_struct
    r = _result("small", "0110")
    net, (x0, ctx, ref, pose, clip, tiles, tile_w, inv_wsum) = r["net"], r["req"]
    cs = net._executor()
    steps, T, Tt, H, Wd = 4, 5, 3, 8, 20
    sig = SIG4.float().cpu()
    ts = (sig[:-1] * 1000.0).repeat_interleave(2).to(DEV).contiguous()
    dsa = (ctypes.c_float * steps)(*[float(v) for v in (sig[1:] - sig[:-1])])
    fr, tw, iw = cs.tile_tables(tiles, tile_w, inv_wsum)
    cond = net._conditioning(ctx, clip, None)
    cc = _cond_struct(cond)
    cos, sin = net._rope(Tt, H // 2, Wd // 2, 0, 0, torch.device(DEV), 1)
    ws = torch.empty(cs.sample_tiled_workspace_bytes(T, Tt, H, Wd), device=DEV, dtype=torch.uint8)
    cache = torch.empty(cs.sample_tiled_cache_bytes(3, Tt, H, Wd), device=DEV, dtype=torch.uint8)
    reuse = (ctypes.c_uint8 * steps)(*MASKS["0110"])
    xg = x0.clone()

    def run():
        L.call("scail_dit_sample_tiled_cached", cs._h, xg.data_ptr(), ts.data_ptr(), ctypes.cast(dsa, ctypes.c_void_p), steps, CFG, ctypes.byref(cc),
               ref.data_ptr(), pose.data_ptr(), fr, tw, iw, 3, T, Tt, cos.data_ptr(), sin.data_ptr(), H, Wd, ws.data_ptr(), ws.numel(),
               reuse, cache.data_ptr(), cache.numel(), torch.cuda.current_stream().cuda_stream)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                  # warm-up on the capture stream
    torch.cuda.synchronize()
    assert torch.equal(xg, r["got"])
    xg.copy_(x0)
    cache.fill_(0xFF)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        run()
    xg.copy_(x0)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(xg, r["got"]), f"graph replay: max |d| {float((xg - r['got']).abs().max())}"


# ---- 8. the query -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,D", [("toy", 512), ("tiny2", 256)])
def test_cache_query_is_n_tiles_R_plus_E(kind, D):
    from scail_amd import lib as L
    ex = _net(kind)._executor()
    q = L.load().scail_dit_sample_tiled_cache_bytes
    for n_tiles, Tt, H, Wd in [(3, 3, 8, 20), (4, 3, 8, 20), (2, 2, 28, 36), (2, 1, 4, 4), (7, 64, 8, 8)]:
        Lnoise = Tt * (H // 2) * (Wd // 2)
        R = (2 * Lnoise * D * 2 + 255) // 256 * 256                     # r: bf16 [2][Lnoise][D], rounded to 256
        E = ex.step_cache_bytes(2, Tt, H, Wd) - R                       # what the step cache holds behind r: the embedding region
        assert E == R
        assert ex.sample_tiled_cache_bytes(n_tiles, Tt, H, Wd) == n_tiles * R + E
        assert n_tiles * R + E < n_tiles * (R + E), "the embedding region is shared, not stacked"
    assert q(None, 3, 3, 8, 20) == -1
    for bad in [(1, 3, 8, 20), (0, 3, 8, 20), (3, 0, 8, 20), (3, 65, 8, 20), (3, 3, 8, 18), (3, 3, 6, 20), (3, 3, 0, 20)]:
        assert q(ex._h, *bad) == -1, bad
        with pytest.raises(L.ScailHipError, match="scail_dit_sample_tiled_cache_bytes: bad shape"):
            ex.sample_tiled_cache_bytes(*bad)


# ---- 9. the sampler, the engine and the command line -----------------------------------------------------------------------------------------
def test_sampler_route_takes_the_plan(monkeypatch):
    """RFSamplerLong.sample_hip with the option: the one-call cached entry, the plan kept; a threshold plans from the network's own signal"""
    import test_longclip_gpu as LC
    from scail_amd.sampler import RFSamplerLong
    calls = LC._Calls(monkeypatch, "sample_tiled", "sample_tiled_cached", "step", "step_cached", "time_distances")
    r = _result("small", "0110")
    net, (x0, ctx, ref, pose, clip, tiles, tile_w, inv_wsum) = r["net"], r["req"]
    shared = dict(concat_images=torch.zeros(1, device=DEV), ref_concat=ref, smpl_tiled=pose, image_clip_features=clip)
    c, uc = dict(crossattn=ctx[1:2], **shared), dict(crossattn=ctx[0:1], **shared)
    smp = RFSamplerLong(hunyuan_schedule=True, shift_scale=5, num_steps=4)
    sig = smp.sigmas(4)
    got = smp.sample_hip(net, x0, c, uc, scale=CFG, tile_indices=tiles, step_cache=dict(mask=[0, 1, 1, 0]))
    assert smp.last_step_cache_plan == [0, 1, 1, 0]
    assert calls.n == {"sample_tiled": 0, "sample_tiled_cached": 1, "step": 0, "step_cached": 0, "time_distances": 0}
    net._executor()._tile_cache = None
    want, _ = _compose(net, r["req"], sig, [0, 1, 1, 0])
    assert torch.equal(got, want)
    huge = smp.sample_hip(net, x0, c, uc, scale=CFG, tile_indices=tiles, step_cache=dict(threshold=1e30, signal="modulation"))
    assert smp.last_step_cache_plan == [0, 1, 1, 0] and calls.n["time_distances"] == 1 and calls.n["sample_tiled_cached"] == 2
    assert torch.equal(huge, want)
    zero = smp.sample_hip(net, x0, c, uc, scale=CFG, tile_indices=tiles, step_cache=dict(threshold=0.0))
    assert smp.last_step_cache_plan == [0, 0, 0, 0]
    assert torch.equal(zero, smp.sample_hip(net, x0, c, uc, scale=CFG, tile_indices=tiles)) and calls.n["sample_tiled"] == 1
    with pytest.raises(NotImplementedError, match="step_cache"):
        smp.sample_hip(net, x0, c, uc, scale=CFG, tile_indices=tiles, step_cache=dict(mask=[0, 1, 1, 0]), step_callback=lambda i, xx: None)
    net._executor()._tile_cache = None


def test_cli_long_clip_with_a_plan_end_to_end(tmp_path, monkeypatch, capsys):
    """--tiny, a 25-frame pose clip in three windows of 4 latent frames, 3 steps, an explicit plan: the CLI's latent is
    engine.sample(tile_indices, step_cache), the plan is printed; without the option the bits are those of the uncached route"""
    import test_longclip_gpu as LC
    from scail_amd import cli, sampler as S
    calls = LC._Calls(monkeypatch, "sample_tiled", "sample_tiled_cached", "sample", "step")
    ref, pose = LC._write_request(tmp_path, 25)
    cfg = copy.deepcopy(cli.TINY)
    engine = cli.build_engine(cfg)
    plain = engine.sampler
    req = cli.request_from_files(ref, pose, cfg, seed=1234, text_dim=engine.network.text_dim)[0]
    plan = [0, 1, 0]
    capsys.readouterr()
    video, z_cli, _ = cli.run(cfg, dict(req), steps=3, engine=engine, tile_frames=13, tile_overlap=8, step_cache=dict(mask=plan))
    out = capsys.readouterr().out
    assert cli.format_step_cache_plan(plan) in out and "2 of 3 steps compute the blocks (0, 2)" in out
    assert calls.n == {"sample_tiled": 0, "sample_tiled_cached": 1, "sample": 0, "step": 0} and engine.sampler is plain
    assert z_cli.shape == (1, 16, 7, 8, 8) and video.shape == (1, 3, 25, 64, 64) and bool(torch.isfinite(video).all())
    # the same request through the engine
    tiles = cli.plan_tiles(7, 4, 2)
    enc = lambda v: engine.encode_first_stage(v.unsqueeze(0), None, force_encode=True).permute(0, 2, 1, 3, 4).contiguous().to(bf16)
    smpl_tiled = torch.stack([enc(req["pose"][:, 4 * t[0]:4 * t[-1] + 1]) for t in tiles], 1)
    shared = dict(concat_images=torch.zeros(1, device=DEV), ref_concat=enc(req["ref"]), smpl_tiled=smpl_tiled,
                  image_clip_features=req["clip"].to(bf16))
    c, uc = dict(crossattn=req["context"], **shared), dict(crossattn=req["uncond_context"], **shared)
    engine.sampler = S.RFSamplerLong(**dict(cfg["model"]["sampler_config"]["params"]))
    try:
        torch.manual_seed(1234)
        z = engine.sample(c, uc=uc, batch_size=1, shape=(7, 16, 8, 8), num_steps=3, tile_indices=tiles, step_cache=dict(mask=plan))
        assert engine.sampler.last_step_cache_plan == plan
        torch.manual_seed(1234)
        z_plain = engine.sample(c, uc=uc, batch_size=1, shape=(7, 16, 8, 8), num_steps=3, tile_indices=tiles)
    finally:
        engine.sampler = plain
    assert torch.equal(z_cli, z.permute(0, 2, 1, 3, 4).contiguous()), "the CLI's latent is not engine.sample's"
    assert not torch.equal(z, z_plain), "the plan skipped nothing"
    # without the option: today's route, today's bits
    before = dict(calls.n)
    _, z_off, _ = cli.run(cfg, dict(req), steps=3, engine=engine, tile_frames=13, tile_overlap=8)
    assert calls.n["sample_tiled"] == before["sample_tiled"] + 1 and calls.n["sample_tiled_cached"] == before["sample_tiled_cached"]
    assert torch.equal(z_off, z_plain.permute(0, 2, 1, 3, 4).contiguous())
    assert "step cache:" not in capsys.readouterr().out
    engine.network._executor()._tile_cache = None
