"""Multi-character requests (n_char reference frames + n_char pose streams, tokens [ref_0.. | noise | pose_0..]; BASELINE config 5, an
extension of the reference) through the ONE-CALL executor and sampler: scail_patchify_chars, scail_dit_step_chars / _sp_chars,
scail_dit_sample_chars (include/scail_dit.h).  The yardsticks are this project's own per-block / per-op path (same kernels in the same
order: identical bits) and the oracle extended the same way."""
import ctypes
import os
import threading

import numpy as np
import pytest
import torch

from oracle import scail_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"

P14B = dict(hidden_size=5120, num_attention_heads=40, inner_hidden_size=13824, text_dim=4096, time_freq_dim=256, time_embed_dim=5120)
TINY2 = dict(hidden_size=256, num_attention_heads=2, inner_hidden_size=512, text_dim=64, time_freq_dim=256, time_embed_dim=256)
TINY4 = dict(hidden_size=512, num_attention_heads=4, inner_hidden_size=1024, text_dim=64, time_freq_dim=256, time_embed_dim=512)


def _mk(params, layers, seed=1234, **kw):
    """random-weight network whose RoPE table extent (latent_width 300) has room for three characters"""
    from scail_amd.dit import DiffusionTransformer
    return DiffusionTransformer(transformer_args=dict(model_parallel_size=1), num_frames=81, latent_width=300, latent_height=300,
                                share_adaln=True, use_i2v_clip=True, device=DEV, init_seed=seed, num_layers=layers, **params, **kw)


def _inputs(T, H, W, n_char, text_dim, Lt, Lc, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, T, 16, H, W, generator=g).to(DEV)
    ref = torch.randn(1, n_char, 16, H, W, generator=g).to(DEV).to(torch.bfloat16)
    pose = torch.randn(1, n_char * T, 16, H // 2, W // 2, generator=g).to(DEV).to(torch.bfloat16)
    ctx = torch.randn(2, Lt, text_dim, generator=g).to(DEV).to(torch.bfloat16)
    clip = torch.randn(1, Lc, 1280, generator=g).to(DEV).to(torch.bfloat16)
    t = torch.tensor([700.0, 700.0], device=DEV)
    return x, t, ctx, ref, pose, clip


def _fwd(net, inputs, **kw):
    x, t, ctx, ref, pose, clip = inputs
    return net.forward_f32(x, t, ctx, None, concat_images=torch.zeros(1, device=DEV), image_clip_features=clip, ref_concat=ref,
                           concat_smpl_render=pose, **kw)


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
    sd = O.make_state_dict(cfg, seed=seed)
    net.load_state_dict(sd, strict=True)
    return cfg, sd, net


def _cos(a, b):
    a, b = a.flatten().double(), b.flatten().double()
    return float((a @ b) / (a.norm() * b.norm()))


class _Calls:
    """counts the calls of CStep methods (which executor entry points a request reached)"""

    def __init__(self, monkeypatch, *names):
        from scail_amd.cstep import CStep
        self.n = {k: 0 for k in names}
        self.kw = {k: [] for k in names}
        for k in names:
            monkeypatch.setattr(CStep, k, self._wrap(k, getattr(CStep, k)))

    def _wrap(self, name, orig):
        def f(cs, *a, **kw):
            self.n[name] += 1
            self.kw[name].append(kw)
            return orig(cs, *a, **kw)
        return f


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------
def _patchify_chars(x, ref, pose, n_char, kpad=128, out=None):
    """scail_patchify_chars itself (ops.patchify routes n_char == 1 to the single-character kernel)"""
    from scail_amd import lib as L
    B, T, _, H, W = x.shape
    Ltok = (n_char + T) * (H // 2) * (W // 2) + n_char * T * (H // 4) * (W // 4)
    if out is None:
        out = torch.full((B, Ltok, kpad), float("nan"), device=DEV, dtype=torch.bfloat16)
    L.call("scail_patchify_chars", x.data_ptr(), ref.data_ptr(), pose.data_ptr(), out.data_ptr(), B, ref.shape[0], pose.shape[0], n_char,
           T, H, W, kpad, torch.cuda.current_stream().cuda_stream)
    return out


def _patchify_loop(x, ref, pose, n_char):
    """the per-character token assembly this kernel replaces: one scail_patchify per character into a temporary + three copies"""
    from scail_amd import ops
    B, T, _, H, W = x.shape
    Lref1, Lnoise, Lpose1 = (H // 2) * (W // 2), T * (H // 2) * (W // 2), T * (H // 4) * (W // 4)
    Lref, Lpose = n_char * Lref1, n_char * Lpose1
    tok = torch.full((B, Lref + Lnoise + Lpose, 128), float("nan"), device=DEV, dtype=torch.bfloat16)
    for c in range(n_char):
        tk = ops.patchify(x, ref[:, c:c + 1].contiguous(), pose[:, c * T:(c + 1) * T].contiguous(), kpad=128)
        tok[:, c * Lref1:(c + 1) * Lref1].copy_(tk[:, :Lref1])
        if c == 0:
            tok[:, Lref:Lref + Lnoise].copy_(tk[:, Lref1:Lref1 + Lnoise])
        tok[:, Lref + Lnoise + c * Lpose1:Lref + Lnoise + (c + 1) * Lpose1].copy_(tk[:, Lref1 + Lnoise:])
    return tok


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("n_char", [1, 2, 3])
@pytest.mark.parametrize("B,n_ref,n_pose", [(1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 1, 2), (2, 2, 2)])
def test_patchify_chars_equals_the_per_character_loop(n_char, B, n_ref, n_pose):
    from scail_amd import ops
    T, H, W = 3, 8, 20
    g = torch.Generator().manual_seed(100 * n_char + 10 * B + n_ref + 2 * n_pose)
    x = torch.randn(B, T, 16, H, W, generator=g).to(DEV)
    ref = torch.randn(n_ref, n_char, 16, H, W, generator=g).to(DEV).to(torch.bfloat16)
    pose = torch.randn(n_pose, n_char * T, 16, H // 2, W // 2, generator=g).to(DEV).to(torch.bfloat16)
    got = _patchify_chars(x, ref, pose, n_char)
    want = _patchify_loop(x, ref, pose, n_char)
    assert got.shape == want.shape
    assert torch.equal(_bits(got), _bits(want))          # bit patterns: every element written (no NaN of the fill left), none differs
    assert not torch.isnan(got.float()).any()
    if n_char == 1:
        assert torch.equal(_bits(got), _bits(ops.patchify(x, ref, pose, kpad=128)))
    else:
        assert torch.equal(_bits(ops.patchify(x, ref, pose, kpad=128, n_char=n_char)), _bits(want))
    # another padded width (the mask channels and the zero padding move with it)
    if n_char == 2 and B == 2 and n_ref == 1 and n_pose == 1:
        assert torch.equal(_bits(_patchify_chars(x, ref, pose, 2, kpad=96)), _bits(want[..., :96].contiguous()))


def test_patchify_chars_bad_arguments_launch_nothing():
    from scail_amd import lib as L
    T, H, W = 2, 8, 8
    x = torch.randn(2, T, 16, H, W, device=DEV)
    ref = torch.randn(1, 2, 16, H, W, device=DEV).to(torch.bfloat16)
    pose = torch.randn(1, 2 * T, 16, H // 2, W // 2, device=DEV).to(torch.bfloat16)
    out = torch.full((2, (2 + T) * 16 + 2 * T * 4, 128), 7.0, device=DEV, dtype=torch.bfloat16)
    s = torch.cuda.current_stream().cuda_stream
    args = lambda **k: (x.data_ptr() + k.get("xo", 0), ref.data_ptr(), pose.data_ptr(), out.data_ptr(), 2, k.get("n_ref", 1), 1, k.get("n_char", 2), T,
                        k.get("H", H), W, k.get("kpad", 128), s)
    for needle, k in (("n_char must be 1..64, got 0", dict(n_char=0)), ("multiples of 4", dict(H=6)), ("kpad must be", dict(kpad=100)),
                      ("cond batch", dict(n_ref=3)), ("pointer alignment", dict(xo=4))):
        with pytest.raises(L.ScailHipError, match=needle.replace(".", r"\.")):
            L.call("scail_patchify_chars", *args(**k))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote to the output"


# ---- 2. one call == the per-block path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_char", [2, 3])
def test_one_call_step_equals_the_host_driven_paths(n_char, monkeypatch):
    """flags 0: scail_dit_step_chars through forward_f32 against (a) the same executor driven block by block from the host
    (scail_dit_block per layer, token assembly / embeddings / final layer as ops.* calls) and (b) the per-op path."""
    calls = _Calls(monkeypatch, "step", "block")
    inputs = _inputs(3, 8, 20, n_char, 64, 12, 5, seed=20 + n_char)
    net = _mk(TINY2, 3, seed=77)
    one = _fwd(net, inputs)
    assert net._cstep is not None and calls.n == {"step": 1, "block": 0}
    assert calls.kw["step"][0]["n_char"] == n_char
    net._c_blocks = True
    blocks = _fwd(net, inputs)
    net._c_blocks = False
    assert calls.n == {"step": 1, "block": 3}
    net.use_c_step = False
    per_op = _fwd(net, inputs)
    net.use_c_step = True
    assert calls.n == {"step": 1, "block": 3}
    assert torch.isfinite(one).all() and float(one.abs().mean()) > 1e-3
    assert torch.equal(one, blocks), f"one call vs scail_dit_block per layer: max |d| {float((one - blocks).abs().max())}"
    assert torch.equal(one, per_op), f"one call vs per-op path: max |d| {float((one - per_op).abs().max())}"
    # the characters matter: dropping the last one changes the result
    x, t, ctx, ref, pose, clip = inputs
    fewer = _fwd(net, (x, t, ctx, ref[:, :-1].contiguous(), pose[:, :-x.shape[1]].contiguous(), clip))
    assert (fewer - one).abs().max() > 1e-3


# ---- 3. the prunings stay exact at full size ---------------------------------------------------------------------------------------
def test_cfg_pair_is_bit_identical_with_two_characters_at_full_size():
    """the shape of test_cfg_pair_is_bit_identical_at_full_size with two characters: 14B width, L = 60 032, 3 layers (layer 0, a middle
    layer and the row-pruned last layer, whose noise rows now start at 2 (H/2)(W/2))"""
    T, H, W = 21, 64, 112
    x, t, ctx, ref, pose, clip = _inputs(T, H, W, 2, 4096, 512, 257, seed=5)
    assert (2 + T) * (H // 2) * (W // 2) + 2 * T * (H // 4) * (W // 4) == 60032
    x = torch.cat([x[:1], x[:1]]).contiguous()
    inputs = (x, t, ctx, ref, pose, clip)
    net = _mk(P14B, 3)
    outs = [_fwd(net, inputs, cfg_pair=pair) for pair in (False, True)]
    assert net._cstep is not None
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all() and float(outs[0].abs().mean()) > 1e-3
    assert not torch.equal(outs[0][0], outs[0][1]), "the two elements must differ (different text conditioning)"
    assert torch.equal(outs[0], outs[1]), f"cfg_pair changed the result: max |d| {float((outs[0] - outs[1]).abs().max())}"


# ---- 4. against the oracle ------------------------------------------------------------------------------------------------------------
def test_one_call_multi_character_step_vs_oracle(golden_dir, monkeypatch, n_char=2):
    """the inputs and the bar of tests/test_dit_gpu.py::test_multi_character_extension_vs_oracle, on the one-call path"""
    calls = _Calls(monkeypatch, "step", "block")
    g = _load(golden_dir, "dit_tiny.npz")
    cfg, sd, net = _net_golden(O.TINY, int(g["seed"]))
    T = g["x"].shape[1]
    gen = torch.Generator().manual_seed(77)
    refs = torch.cat([g["ref"]] + [torch.randn(g["ref"].shape, generator=gen) for _ in range(n_char - 1)], 1)
    poses = torch.cat([g["pose"]] + [torch.randn(g["pose"].shape, generator=gen) for _ in range(n_char - 1)], 1)
    assert refs.shape[1] == n_char and poses.shape[1] == n_char * T
    want = O.dit_forward(cfg, sd, g["x"], g["t"], g["ctx"], refs, poses, g["clip"])
    kw = dict(concat_images=torch.zeros(1, *g["x"].shape[1:], device=DEV), image_clip_features=g["clip"].to(DEV))
    out = net.forward_f32(g["x"].to(DEV), g["t"].to(DEV), g["ctx"].to(DEV), None, ref_concat=refs.to(DEV),
                          concat_smpl_render=poses.to(DEV), **kw)
    assert net._cstep is not None and calls.n == {"step": 1, "block": 0}, "the one-call path must have run"
    assert out.shape == g["out"].shape
    torch.testing.assert_close(out.cpu(), want, rtol=2e-2, atol=2e-2)
    assert _cos(out.cpu(), want) >= 0.999
    one = net.forward_f32(g["x"].to(DEV), g["t"].to(DEV), g["ctx"].to(DEV), None, ref_concat=g["ref"].to(DEV),
                          concat_smpl_render=g["pose"].to(DEV), **kw)
    torch.testing.assert_close(one.cpu(), g["out"], rtol=2e-2, atol=2e-2)
    assert (one - out).abs().max() > 1e-2
    with pytest.raises(Exception, match="frames"):
        net.forward_f32(g["x"].to(DEV), g["t"].to(DEV), g["ctx"].to(DEV), None, ref_concat=refs.to(DEV),
                        concat_smpl_render=g["pose"].to(DEV), **kw)
    # the executor's own check of the same thing (the Python layer above answers first in the product)
    from scail_amd import lib as L
    a = ctypes.c_void_p(1 << 20)
    with pytest.raises(L.ScailHipError, match=r"n_char \* T = 2 \* 4 frames, got 4"):
        L.call("scail_dit_step_chars", net._cstep._h, a, a, a, a, 1, a, 1, 2, 4, a, a, a, 2, 4, 8, 8, 0, a, 1 << 30, None)
    with pytest.raises(L.ScailHipError, match="n_char must be 1..64, got 0"):
        L.call("scail_dit_step_chars", net._cstep._h, a, a, a, a, 1, a, 1, 0, 0, a, a, a, 2, 4, 8, 8, 0, a, 1 << 30, None)
    with pytest.raises(L.ScailHipError, match="fewer than 2\\^31 - 64 keys, got Ltok = "):
        L.call("scail_dit_step_chars", net._cstep._h, a, a, a, a, 1, a, 1, 64, 64 * 30000, a, a, a, 2, 30000, 1024, 1024, 0, a, 1 << 30, None)
    assert L.load().scail_dit_chars_workspace_bytes(net._cstep._h, 2, 30000, 1024, 1024, 64) == -1
    assert L.load().scail_dit_chars_workspace_bytes(net._cstep._h, 2, 4, 8, 8, 0) == -1
    assert L.load().scail_dit_chars_workspace_bytes(net._cstep._h, 2, 4, 8, 8, 2) > L.load().scail_dit_workspace_bytes(net._cstep._h, 2, 4, 8, 8) > 0


# ---- 5. the sampler ------------------------------------------------------------------------------------------------------------------
def test_sampler_one_call_equals_the_python_loop_and_replays_from_a_graph(monkeypatch):
    from scail_amd import lib as L, sampler as S
    from scail_amd.cstep import DitCond
    calls = _Calls(monkeypatch, "sample", "step", "block")
    T, H, W, n_char, steps = 3, 8, 20, 2, 5
    x, t, ctx, ref, pose, clip = _inputs(T, H, W, n_char, 64, 12, 5, seed=31)
    x0 = x[:1].contiguous()
    net = _mk(TINY2, 3, seed=78)
    smp = S.RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=steps,
                      guider_config={"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": 4}})
    shared = dict(concat_images=torch.zeros(1, device=DEV), ref_concat=ref, concat_smpl_render=pose, image_clip_features=clip)
    c, uc = dict(crossattn=ctx[1:2], **shared), dict(crossattn=ctx[0:1], **shared)
    xT = smp.sample_hip(net, x0, c, uc)
    assert calls.n == {"sample": 1, "step": 0, "block": 0}, "two reference frames must take scail_dit_sample_chars"
    seen = []
    xT_loop = smp.sample_hip(net, x0, c, uc, step_callback=lambda i, xx: seen.append(i))      # the Python loop: forward_f32 + cfg_euler_
    assert seen == list(range(steps)) and calls.n == {"sample": 1, "step": steps, "block": 0}
    assert torch.isfinite(xT).all() and not torch.equal(xT, x0)
    assert torch.equal(xT, xT_loop), f"max |d| {float((xT - xT_loop).abs().max())}"
    # one capture of the whole run (scail_dit_sample_chars enqueues without synchronising), one replay: the same bits
    cs = net._cstep
    sig = smp.sigmas(steps).float().cpu()
    ts = (sig[:-1] * 1000.0).repeat_interleave(2).to(DEV).contiguous()
    dsa = (ctypes.c_float * steps)(*[float(v) for v in (sig[1:] - sig[:-1])])
    cond = net._conditioning(torch.cat((uc["crossattn"], c["crossattn"]), 0), clip, None)
    cc = DitCond(cond["k_text"].data_ptr(), cond["vt_text"].data_ptr(), cond["k_clip"].data_ptr(), cond["vt_clip"].data_ptr(),
                 cond["k_text"].shape[2], cond["k_clip"].shape[2], cond["k_clip"].shape[1])
    cos, sin = net._rope(T, H // 2, W // 2, 0, 0, torch.device(DEV), n_char)
    need = L.load().scail_dit_sample_chars_workspace_bytes(cs._h, T, H, W, n_char)
    assert need > 0
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    xg = x0.clone()

    def run():
        L.call("scail_dit_sample_chars", cs._h, xg.data_ptr(), ts.data_ptr(), ctypes.cast(dsa, ctypes.c_void_p), steps, 4.0, ctypes.byref(cc),
               ref.data_ptr(), pose.data_ptr(), n_char, pose.shape[1], cos.data_ptr(), sin.data_ptr(), T, H, W, ws.data_ptr(), ws.numel(),
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
    xg.copy_(x0)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(xg, xT), f"graph replay: max |d| {float((xg - xT).abs().max())}"


def test_engine_request_with_two_reference_frames_reaches_the_one_call_sampler(monkeypatch):
    import copy
    from scail_amd import cli
    from scail_amd.engine import SATVideoDiffusionEngine
    calls = _Calls(monkeypatch, "sample", "step", "block")
    mc = copy.deepcopy(cli.TINY["model"])
    mc["build_first_stage"] = False
    eng = SATVideoDiffusionEngine(mc, device=DEV)
    p = mc["network_config"]["params"]
    g = torch.Generator().manual_seed(3)
    shared = dict(concat_images=torch.zeros(1, device=DEV), image_clip_features=torch.randn(1, 5, 1280, generator=g).to(DEV).to(torch.bfloat16),
                  ref_concat=torch.randn(1, 2, 16, 8, 8, generator=g).to(DEV).to(torch.bfloat16),
                  concat_smpl_render=torch.randn(1, 2 * 4, 16, 4, 4, generator=g).to(DEV).to(torch.bfloat16))
    c = dict(crossattn=torch.randn(1, 12, p["text_dim"], generator=g).to(DEV).to(torch.bfloat16), **shared)
    uc = dict(crossattn=torch.zeros(1, 12, p["text_dim"], device=DEV, dtype=torch.bfloat16), **shared)
    z = eng.sample(c, uc=uc, batch_size=1, shape=(4, 16, 8, 8), num_steps=2)
    assert z.shape == (1, 4, 16, 8, 8) and torch.isfinite(z.float()).all()
    assert calls.n == {"sample": 1, "step": 0, "block": 0}
    assert calls.kw["sample"][0]["n_char"] == 2


# ---- 6. sequence parallel ---------------------------------------------------------------------------------------------------------------
def _run_ranks(world, mode, mk, inputs, chunk_dim, setup, expect):
    """one network evaluation on `world` virtual ranks (ThreadBackend); `setup(net)` selects the path; returns rank 0's gathered result"""
    from scail_amd.cstep import CStep
    from scail_amd.parallel import SequenceParallel, ThreadBackend
    x, t, ctx, ref, pose, clip = inputs
    shared = ThreadBackend.Shared(world)
    outs, errs = [None] * world, []
    counts, lock = {"step_sp": 0, "block_sp": 0}, threading.Lock()
    orig = {k: getattr(CStep, k) for k in counts}

    def counted(name):
        def f(cs, *a, **kw):
            with lock:
                counts[name] += 1
            return orig[name](cs, *a, **kw)
        return f

    def run(rk):
        try:
            torch.cuda.set_device(0)
            n = mk()
            setup(n)
            sp = SequenceParallel(ThreadBackend(shared, rk), mode=mode)
            n.sp = sp
            sp.check_latent(x.shape[3], x.shape[4], chunk_dim)
            ch = lambda tt: sp.chunk(tt, chunk_dim)
            o = n.forward_f32(ch(x), t, ctx, None, concat_images=torch.zeros(1, device=DEV), image_clip_features=clip,
                              ref_concat=ch(ref), concat_smpl_render=ch(pose), chunk_dim=chunk_dim)
            outs[rk] = sp.gather_to_rank0(o, chunk_dim)
        except Exception as e:  # pragma: no cover
            errs.append(e)
            shared.barrier.abort()

    for k in counts:
        setattr(CStep, k, counted(k))
    try:
        th = [threading.Thread(target=run, args=(rk,)) for rk in range(world)]
        [tt.start() for tt in th]
        [tt.join() for tt in th]
    finally:
        for k, v in orig.items():
            setattr(CStep, k, v)
    assert not errs, errs
    torch.cuda.synchronize()
    assert counts == expect, counts
    return outs[0]


@pytest.mark.parametrize("world,mode,chunk_dim", [(2, "allgather", 3), (4, "ulysses", 4)])
def test_sequence_parallel_one_call_equals_per_block_and_single_rank(world, mode, chunk_dim):
    n_char, layers = 2, 3
    T, H, W = (2, 16, 32) if chunk_dim == 3 else (2, 32, 16)
    inputs = _inputs(T, H, W, n_char, 64, 12, 5, seed=11)
    mk = lambda: _mk(TINY4, layers, seed=77)
    one = _run_ranks(world, mode, mk, inputs, chunk_dim, lambda n: None, {"step_sp": world, "block_sp": 0})

    def blocks(n):
        n._c_blocks = True

    def per_op(n):
        n.use_c_step = False

    by_block = _run_ranks(world, mode, mk, inputs, chunk_dim, blocks, {"step_sp": 0, "block_sp": world * layers})
    host = _run_ranks(world, mode, mk, inputs, chunk_dim, per_op, {"step_sp": 0, "block_sp": 0})
    assert torch.equal(one, by_block), f"scail_dit_step_sp_chars vs scail_dit_block_sp per layer: max |d| {float((one - by_block).abs().max())}"
    assert torch.equal(one, host), f"scail_dit_step_sp_chars vs per-op host path: max |d| {float((one - host).abs().max())}"
    single = _fwd(mk(), inputs)
    d = (one - single).abs()
    scale = float(single.abs().mean())
    print(f"SP {world} x {mode}, {n_char} characters: max |d| {float(d.max()):.4f}, mean |d| {float(d.mean()):.5f}, |ref| mean {scale:.3f}")
    # the bar of test_sequence_parallel_fullsize_virtual_ranks for n_char = 2 (bf16 re-association: rank-major key order, per-rank tiling)
    assert torch.isfinite(one).all()
    assert float(d.mean()) <= 6e-3 * max(scale, 1.0) and float(d.max()) <= 0.125
    assert _cos(one, single) >= 0.9999


# ---- 7. fp8 ----------------------------------------------------------------------------------------------------------------------------
def test_fp8_one_call_equals_blockwise_with_two_characters_and_sp_still_refuses(monkeypatch):
    from scail_amd import lib as L
    calls = _Calls(monkeypatch, "step", "block")
    inputs = _inputs(3, 8, 20, 2, 64, 12, 5, seed=41)
    net = _mk(TINY2, 3, seed=79, gemm_precision="fp8")
    o_step = _fwd(net, inputs)
    assert net._cstep is not None and net._cstep._fp8_buf is not None and calls.n == {"step": 1, "block": 0}
    net._c_blocks = True
    o_blocks = _fwd(net, inputs)
    net._c_blocks = False
    assert calls.n == {"step": 1, "block": 3}
    assert torch.isfinite(o_step).all()
    assert torch.equal(o_step, o_blocks), f"max |d| {float((o_step - o_blocks).abs().max())}"
    bf16 = _fwd(_mk(TINY2, 3, seed=79), inputs)
    assert not torch.equal(bf16, o_step) and _cos(bf16, o_step) >= 0.995
    # the sequence-parallel entry points, old and new, refuse a handle with fp8 enabled before anything runs
    a = ctypes.c_void_p(1 << 20)
    with pytest.raises(L.ScailHipError, match="fp8 GEMMs are enabled"):
        L.call("scail_dit_step_sp", net._cstep._h, a, a, a, a, 1, a, 1, a, a, a, 2, 2, 16, 16, a, 0, a, 1 << 30, None)
    with pytest.raises(L.ScailHipError, match="fp8 GEMMs are enabled"):
        L.call("scail_dit_step_sp_chars", net._cstep._h, a, a, a, a, 1, a, 1, 2, 4, a, a, a, 2, 2, 16, 16, a, 0, a, 1 << 30, None)
    with pytest.raises(L.ScailHipError, match="fp8 GEMMs are enabled"):
        L.call("scail_dit_block_sp", net._cstep._h, 0, a, a, a, a, a, 2, 16, a, a, 1 << 30, None)


# ---- 8. one character is untouched -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 1])
def test_step_chars_with_one_character_equals_scail_dit_step(golden_dir, flags):
    from scail_amd import lib as L
    from scail_amd.cstep import DitCond
    g = _load(golden_dir, "dit_tiny.npz")
    cfg, sd, net = _net_golden(O.TINY, int(g["seed"]))
    x, t, ctx = g["x"].to(DEV).float().contiguous(), g["t"].to(DEV).float().contiguous(), g["ctx"].to(DEV).to(torch.bfloat16)
    ref, pose, clip = (g[k].to(DEV).to(torch.bfloat16).contiguous() for k in ("ref", "pose", "clip"))
    B, T, _, H, W = x.shape
    assert B == 2 and ref.shape[0] == 1 and pose.shape[0] == 1
    if flags:                                   # SCAIL_DIT_CFG_PAIR: one latent and one timestep twice
        x, t = torch.cat([x[:1], x[:1]]).contiguous(), torch.cat([t[:1], t[:1]]).contiguous()
    kw = dict(concat_images=torch.zeros(1, device=DEV), ref_concat=ref, concat_smpl_render=pose, image_clip_features=clip)
    through_python = net.forward_f32(x, t, ctx, None, cfg_pair=bool(flags), **kw)        # scail_dit_step_chars(n_char = 1)
    cs = net._cstep
    cond = net._conditioning(ctx, clip, None)
    cc = DitCond(cond["k_text"].data_ptr(), cond["vt_text"].data_ptr(), cond["k_clip"].data_ptr(), cond["vt_clip"].data_ptr(),
                 cond["k_text"].shape[2], cond["k_clip"].shape[2], cond["k_clip"].shape[1])
    cos, sin = net._rope(T, H // 2, W // 2, 0, 0, torch.device(DEV))
    lib = L.load()
    need = lib.scail_dit_workspace_bytes(cs._h, B, T, H, W)
    assert need == lib.scail_dit_chars_workspace_bytes(cs._h, B, T, H, W, 1) > 0
    assert lib.scail_dit_sample_workspace_bytes(cs._h, T, H, W) == lib.scail_dit_sample_chars_workspace_bytes(cs._h, T, H, W, 1)
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    s = torch.cuda.current_stream().cuda_stream
    outs = []
    for name, extra in (("scail_dit_step", ()), ("scail_dit_step_chars", (1, T))):
        out = torch.full((B, T, 16, H, W), float("nan"), device=DEV)
        L.call(name, cs._h, x.data_ptr(), t.data_ptr(), ctypes.byref(cc), ref.data_ptr(), 1, pose.data_ptr(), 1, *extra, cos.data_ptr(),
               sin.data_ptr(), out.data_ptr(), B, T, H, W, flags, ws.data_ptr(), ws.numel(), s)
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], through_python)
    if not flags:
        torch.testing.assert_close(outs[0].cpu(), g["out"], rtol=2e-2, atol=2e-2)
