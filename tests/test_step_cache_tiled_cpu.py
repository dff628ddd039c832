"""The step cache for clips longer than one window, without a GPU: which entry of the network a tiled request with the ``step_cache`` option
reaches (RFSamplerLong.sample_hip on a fake network), what stays refused and that the refusal comes before any call into the network, the
command line's route, and the refusals of scail_dit_sample_tiled_cached / scail_dit_sample_tiled_cache_bytes that need no handle."""
import ctypes as C
import os

import pytest
import torch


class _FakeNet:
    """stands in for DiffusionTransformer: records which entry of the binding a tiled request would reach"""

    def __init__(self, takes_loop=True):
        self.calls, self.takes_loop = [], takes_loop

    def executor_ok(self, whole_loop=False):
        return self.takes_loop

    def sample_tiled_c(self, *args, **kw):
        self.calls.append(("sample_tiled_c", args, kw))
        return args[0]

    def time_distances(self, timesteps, signal="time"):
        self.calls.append(("time_distances", signal, int(timesteps.numel())))
        return [(0.0, 0.0)] + [(0.5, 4.0)] * (int(timesteps.numel()) - 1)

    def forward_f32(self, xin, t, ctx, y, **kw):
        self.calls.append(("forward_f32", kw.get("step_cache", "absent")))
        return torch.zeros_like(xin)


TILES = [[0, 1], [1, 2]]


def _request(n_tiles=2, Tt=2, n_char=1, T=3):
    c = dict(crossattn=torch.zeros(1, 4, 8), ref_concat=torch.zeros(1, n_char, 16, 8, 8), smpl_tiled=torch.zeros(1, n_tiles, Tt, 16, 4, 4),
             image_clip_features=torch.zeros(1, 3, 8))
    return torch.zeros(1, T, 16, 8, 8), c, dict(c)


def _sampler():
    from scail_amd.sampler import RFSamplerLong
    return RFSamplerLong(hunyuan_schedule=True, shift_scale=5, num_steps=6)


def _same(a, b):
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def test_a_mask_reaches_sample_tiled_c_with_that_plan():
    net, (x, c, uc) = _FakeNet(), _request()
    s = _sampler()
    s.sample_hip(net, x, c, uc, tile_indices=TILES, step_cache=dict(mask=[0, 1, 0, 1, 1, 0]))
    assert [k[0] for k in net.calls] == ["sample_tiled_c"], "an explicit plan needs no distance run and no forward"
    assert net.calls[0][2]["reuse"] == [0, 1, 0, 1, 1, 0] and s.last_step_cache_plan == [0, 1, 0, 1, 1, 0]


def test_a_threshold_plans_once_then_reaches_sample_tiled_c():
    net, (x, c, uc) = _FakeNet(), _request()
    s = _sampler()
    s.sample_hip(net, x, c, uc, tile_indices=TILES, step_cache=dict(threshold=0.3, signal="modulation"))
    assert net.calls[0] == ("time_distances", "modulation", 6) and [k[0] for k in net.calls] == ["time_distances", "sample_tiled_c"]
    assert net.calls[1][2]["reuse"] == [0, 1, 1, 0, 1, 0] == s.last_step_cache_plan          # d_i = 0.125, threshold 0.3 (plan_step_cache's example)


def test_without_the_option_the_call_is_todays():
    """argument for argument what RFSamplerLong.sample_hip hands sample_tiled_c without the option: no ``reuse`` key at all"""
    net, (x, c, uc) = _FakeNet(), _request()
    s = _sampler()
    s.sample_hip(net, x, c, uc, tile_indices=TILES)
    s.sample_hip(net, x, c, uc, tile_indices=TILES, step_cache=None)
    s.sample_hip(net, x, c, uc, tile_indices=TILES, step_cache=dict(mask=[0, 1, 0, 1, 1, 0]))
    assert [k[0] for k in net.calls] == ["sample_tiled_c"] * 3
    (_, a0, k0), (_, a1, k1), (_, a2, k2) = net.calls
    assert sorted(k0) == sorted(k1) == ["cond_key"] and k0["cond_key"] == ("sample_hip", id(c))
    assert len(a0) == 10 and _same(a0, a1), "step_cache=None changed the call"
    # the arguments themselves: latent, schedule, scale, [uncond; cond], ref, pose tiles, clip, tiles, weights
    idxs, tile_w, inv_wsum = s._tile_table(TILES, 3, x.device)
    want = (x, s.sigmas(None), float(s.guider.scale), torch.cat((uc["crossattn"], c["crossattn"]), 0), c["ref_concat"], c["smpl_tiled"],
            c["image_clip_features"], [[0, 1], [1, 2]], tile_w.cpu(), inv_wsum.cpu())
    assert _same(a0, want)
    # and with the option the same arguments plus the plan
    assert _same(a2, a0) and sorted(k2) == ["cond_key", "reuse"] and k2["cond_key"] == k0["cond_key"]


@pytest.mark.parametrize("what", ["callback", "chunk_dim", "host_loop", "two_characters", "tile_of_65", "no_smpl_tiled", "smpl_tiled_tiles",
                                  "smpl_tiled_frames", "smpl_tiled_rank"])
def test_uncovered_requests_are_refused_before_any_network_call(what):
    net, (x, c, uc) = _FakeNet(takes_loop=what != "host_loop"), _request()
    kw, tiles = {}, TILES
    if what == "callback":
        kw["step_callback"] = lambda i, xx: None
    elif what == "chunk_dim":
        kw["chunk_dim"] = 3
    elif what == "two_characters":
        x, c, uc = _request(n_char=2)
    elif what == "tile_of_65":
        x, c, uc = _request(Tt=65, T=66)
        tiles = [list(range(65)), list(range(1, 66))]
    elif what == "no_smpl_tiled":
        c = {k: v for k, v in c.items() if k != "smpl_tiled"}
    elif what == "smpl_tiled_tiles":
        c = dict(c, smpl_tiled=torch.zeros(1, 3, 2, 16, 4, 4))
    elif what == "smpl_tiled_frames":
        c = dict(c, smpl_tiled=torch.zeros(1, 2, 3, 16, 4, 4))
    elif what == "smpl_tiled_rank":
        c = dict(c, smpl_tiled=torch.zeros(2, 2, 16, 4, 4))
    for option in (dict(threshold=0.1), dict(mask=[0, 1, 0, 1, 1, 0])):
        with pytest.raises(NotImplementedError, match="step_cache"):
            _sampler().sample_hip(net, x, c, uc, tile_indices=tiles, step_cache=option, **kw)
    assert net.calls == [], "the refusal came after a call into the network (time_distances included)"


def test_a_malformed_option_is_a_value_error_and_reaches_nothing():
    net, (x, c, uc) = _FakeNet(), _request()
    for bad in ({}, dict(threshold=0.1, foo=1), dict(mask=[0, 1], threshold=0.1), dict(mask=[1, 0, 0, 0, 0, 0]), dict(mask=[0, 1]), dict(signal="time")):
        with pytest.raises(ValueError, match="step_cache"):
            _sampler().sample_hip(net, x, c, uc, tile_indices=TILES, step_cache=bad)
    assert net.calls == []


# ---- the command line ---------------------------------------------------------------------------------------------------------------------------
class _FakeEngine:
    """stands in for SATVideoDiffusionEngine in cli.run: records what engine.sample is asked, runs nothing"""

    def __init__(self):
        from scail_amd import sampler as S
        self.network = type("N", (), dict(num_frames=13, text_dim=64))()
        self.sampler = S.RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=3)
        self.sp = None
        self.asked = []

    def encode_first_stage(self, v, *a, **kw):
        return torch.zeros(1, 16, (v.shape[2] - 1) // 4 + 1, v.shape[3] // 8, v.shape[4] // 8)

    def sample(self, c, uc=None, batch_size=1, shape=None, num_steps=None, **extra):
        self.asked.append(dict(extra, sampler=type(self.sampler).__name__, shape=tuple(shape), num_steps=num_steps, smpl_tiled=tuple(c["smpl_tiled"].shape)))
        if "step_cache" in extra:
            self.sampler.last_step_cache_plan = self.sampler.step_cache_plan(None, self.sampler.sigmas(num_steps), extra["step_cache"])
        return torch.zeros(batch_size, *shape)

    def decode_first_stage(self, z, chunk_frames=None):
        return torch.zeros(z.shape[0], 3, 4 * (z.shape[2] - 1) + 1, 8 * z.shape[3], 8 * z.shape[4])


def test_cli_takes_step_cache_with_tiles(monkeypatch, capsys):
    """a 25-frame pose clip with a 13-frame window: three tiles AND the step cache -- no longer refused, the option travels with the tiles and
    the plan is printed; without the option engine.sample is asked exactly what it was asked before"""
    from scail_amd import cli
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    assert cli.step_cache_args(0.2, None, "1,1", "time") == dict(threshold=0.2, signal="time", keep_first=1, keep_last=1)
    assert cli.tile_args(13, 8, 13) == (4, 2)
    req = cli.synthetic_request(64, 64, 25, 64, 12, "cpu", 0)
    eng = _FakeEngine()
    plain = eng.sampler
    video, z, _ = cli.run(cli.TINY, dict(req), steps=3, device="cpu", engine=eng, tile_frames=13, tile_overlap=8, step_cache=dict(mask=[0, 1, 0]))
    assert eng.sampler is plain
    assert eng.asked == [dict(tile_indices=[[0, 1, 2, 3], [2, 3, 4, 5], [3, 4, 5, 6]], step_cache=dict(mask=[0, 1, 0]), sampler="RFSamplerLong",
                              shape=(7, 16, 8, 8), num_steps=3, smpl_tiled=(1, 3, 4, 16, 4, 4))]
    assert cli.format_step_cache_plan([0, 1, 0]) in capsys.readouterr().out
    cli.run(cli.TINY, dict(req), steps=3, device="cpu", engine=eng, tile_frames=13, tile_overlap=8)
    assert eng.asked[1] == dict(tile_indices=[[0, 1, 2, 3], [2, 3, 4, 5], [3, 4, 5, 6]], sampler="RFSamplerLong", shape=(7, 16, 8, 8), num_steps=3,
                                smpl_tiled=(1, 3, 4, 16, 4, 4)), "without the option no step_cache key travels"
    assert "step cache:" not in capsys.readouterr().out
    # the help texts no longer speak of one window
    text = cli.build_parser().format_help()
    assert "Single GPU, one window" not in " ".join(text.split()) and "one plan for all of them" in " ".join(text.split())


# ---- the library's refusals that need no handle -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from scail_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libscail_hip.so is not built")
    return L


A = 0x1000        # a fake, 256-byte aligned device address: every refusal below comes before it is dereferenced


def _tiled_cached(L, n_tiles=3, T=5, Tt=3, n_steps=4, reuse=(0, 1, 1, 0), cache=A, cache_bytes=1 << 30, tiles=((0, 1, 2), (1, 2, 3), (2, 3, 4)),
                  ws_bytes=1 << 30, handle=None):
    fr = (C.c_int32 * (len(tiles) * len(tiles[0])))(*[f for t in tiles for f in t])
    tw = (C.c_float * len(fr))(*[1.0] * len(fr))
    iw = (C.c_float * max(T, 1))(*[1.0] * max(T, 1))
    dsa = (C.c_float * max(n_steps, 1))(*[-0.25] * max(n_steps, 1))
    mask = None if reuse is None else (C.c_uint8 * max(len(reuse), 1))(*reuse)
    L.call("scail_dit_sample_tiled_cached", handle, A, A, C.cast(dsa, C.c_void_p), n_steps, 4.0, A, A, A, fr, tw, iw, n_tiles, T, Tt, A, A, 8, 20,
           A, ws_bytes, mask, cache, cache_bytes, None)


def test_library_refusals_without_a_handle(lib):
    L = lib
    who = "scail_dit_sample_tiled_cached: "
    with pytest.raises(L.ScailHipError, match=who + r"needs at least 2 tiles .* got n_tiles = 1\b"):
        _tiled_cached(L, n_tiles=1, tiles=((0, 1, 2),))
    with pytest.raises(L.ScailHipError, match=who + r"the tile length Tt must be 1..min\(T, 64\), got Tt = 65 with T = 70"):
        _tiled_cached(L, T=70, Tt=65, tiles=(tuple(range(65)),) * 3)
    with pytest.raises(L.ScailHipError, match=who + r"frame 4 of \[0, T = 5\) is covered by no tile"):
        _tiled_cached(L, tiles=((0, 1, 2), (1, 2, 3), (2, 3, 1)))
    with pytest.raises(L.ScailHipError, match=who + r"reuse\[0\] = 1: the first step has nothing to reuse"):
        _tiled_cached(L, reuse=(1, 0, 0, 0))
    with pytest.raises(L.ScailHipError, match=who + r"reuse\[2\] = 2 \(an entry is 0 = compute or 1 = reuse\)"):
        _tiled_cached(L, reuse=(0, 1, 2, 0))
    with pytest.raises(L.ScailHipError, match=who + r"null reuse mask with n_steps = 4"):
        _tiled_cached(L, reuse=None)
    with pytest.raises(L.ScailHipError, match=who + r"null cache \(cache_bytes 4096; scail_dit_sample_tiled_cache_bytes\)"):
        _tiled_cached(L, cache=None, cache_bytes=4096)
    with pytest.raises(L.ScailHipError, match=who + r"the cache must be 256-byte aligned, got an address that is 128 past a multiple of 256"):
        _tiled_cached(L, cache=A + 128)
    # the tiling is judged before the plan and the plan before the cache; only then is the handle missed
    with pytest.raises(L.ScailHipError, match="n_tiles = 1"):
        _tiled_cached(L, n_tiles=1, tiles=((0, 1, 2),), reuse=(1, 0, 0, 0), cache=None)
    with pytest.raises(L.ScailHipError, match=r"reuse\[0\] = 1"):
        _tiled_cached(L, reuse=(1, 0, 0, 0), cache=None)
    with pytest.raises(L.ScailHipError, match=who + "null handle"):
        _tiled_cached(L)
    # the uncached entry keeps its own name in the same refusals
    fr = (C.c_int32 * 3)(0, 1, 2)
    one = (C.c_float * 5)(*[1.0] * 5)
    with pytest.raises(L.ScailHipError, match=r"scail_dit_sample_tiled: needs at least 2 tiles .* got n_tiles = 1\b"):
        L.call("scail_dit_sample_tiled", None, A, A, A, 2, 4.0, A, A, A, fr, one, one, 1, 5, 3, A, A, 8, 20, A, 1 << 30, None)


def test_cache_query_without_a_handle(lib):
    q = lib.load().scail_dit_sample_tiled_cache_bytes
    assert q(None, 3, 3, 8, 20) == -1 and q(None, 1, 65, 8, 18) == -1
    assert q.restype is C.c_int64
