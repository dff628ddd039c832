"""Tiled long-clip sampling (RFSamplerLong, temporal tiling) through the one-call executor, the part that needs no GPU: the new symbols of
the C ABI (include/scail_hip.h scail_tile_*, include/scail_dit.h scail_dit_sample_tiled), the refusals of the entry point -- host-side
returns that name the value, before any device call --, the tile planner of the request path and the CLI's argument checks."""
import ctypes as C
import re

import pytest
import torch

TILE_SYMBOLS = ["scail_tile_gather", "scail_tile_blend_acc", "scail_tile_finish", "scail_dit_sample_tiled_workspace_bytes",
                "scail_dit_sample_tiled"]
A = 0x1000       # a fake, suitably aligned device address: validation fails before it is ever dereferenced


@pytest.fixture(scope="module")
def L():
    from scail_amd import build, lib
    build.build(verbose=False)
    lib.load()
    return lib


def test_tiled_entry_points_are_declared_bound_and_exported(L):
    import os
    lib = L.load()
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    header = open(os.path.join(inc, "scail_hip.h")).read() + open(os.path.join(inc, "scail_dit.h")).read()
    for name in TILE_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in L.SIGNATURES, name
        assert hasattr(lib, name), name
    assert L.ABI_VERSION == 8 and lib.scail_abi_version() == 8
    assert lib.scail_dit_sample_tiled_workspace_bytes.restype is L._i64
    assert len(L.SIGNATURES["scail_dit_sample_tiled"]) == 22
    assert lib.scail_dit_sample_tiled_workspace_bytes(None, 6, 4, 8, 8) == -1           # no handle
    from scail_amd import ops
    from scail_amd.cstep import CStep
    from scail_amd.dit import DiffusionTransformer
    assert all(hasattr(ops, n) for n in ("tile_gather", "tile_blend_acc_", "tile_finish_"))
    assert hasattr(CStep, "sample_tiled") and hasattr(DiffusionTransformer, "sample_tiled_c")


def _sample_tiled(L, tiles, T, inv=None, tile_w=None, n_tiles=None, Tt=None, ws_bytes=1 << 40, **ptr):
    """scail_dit_sample_tiled on fake pointers and NO handle: every check of the tiling runs before the handle is looked at"""
    n = len(tiles)
    tt = len(tiles[0]) if n else 0
    fr = (C.c_int32 * max(1, n * tt))(*[f for t in tiles for f in t])
    tw = (C.c_float * max(1, n * tt))(*([1.0] * (n * tt) if tile_w is None else tile_w))
    iw = (C.c_float * max(1, T))(*([0.5] * T if inv is None else inv))
    p = dict(h=None, x=A, ts=A, ds=A, cond=A, ref=A, pose=A, fr=fr, tw=tw, iw=iw, cos=A, sin=A, ws=A)
    p.update(ptr)
    L.call("scail_dit_sample_tiled", p["h"], p["x"], p["ts"], p["ds"], 2, 4.0, p["cond"], p["ref"], p["pose"], p["fr"], p["tw"], p["iw"],
           n if n_tiles is None else n_tiles, T, tt if Tt is None else Tt, p["cos"], p["sin"], 8, 8, p["ws"], ws_bytes, None)


GOOD = [[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 5]]


def test_sample_tiled_refusals_name_the_value(L):
    who = "scail_dit_sample_tiled: "
    with pytest.raises(L.ScailHipError, match=who + r"needs at least 2 tiles .* got n_tiles = 1\b"):
        _sample_tiled(L, GOOD[:1], 4)
    with pytest.raises(L.ScailHipError, match=r"n_tiles = 0\b"):
        _sample_tiled(L, GOOD, 6, n_tiles=0)
    # Tt outside 1..min(T, 64)
    with pytest.raises(L.ScailHipError, match=who + r"the tile length Tt must be 1\.\.min\(T, 64\), got Tt = 0 with T = 6"):
        _sample_tiled(L, GOOD, 6, Tt=0)
    with pytest.raises(L.ScailHipError, match=r"got Tt = 4 with T = 3\b"):
        _sample_tiled(L, GOOD, 3)
    with pytest.raises(L.ScailHipError, match=who + r"the latent must have fewer than 32768 frames, got T = 32768\b"):
        _sample_tiled(L, GOOD, 32768)
    with pytest.raises(L.ScailHipError, match=r"got Tt = 65 with T = 100\b"):
        _sample_tiled(L, [list(range(65)), list(range(35, 100))], 100)
    # a frame index outside [0, T)
    with pytest.raises(L.ScailHipError, match=r"tile 2: frame index 6 \(tile frame 3\) is outside \[0, T = 6\)"):
        _sample_tiled(L, [GOOD[0], GOOD[1], [2, 3, 4, 6]], 6)
    with pytest.raises(L.ScailHipError, match=r"tile 0: frame index -1 "):
        _sample_tiled(L, [[0, -1, 2, 3], GOOD[1], GOOD[2]], 6)
    # a repeated index inside one tile
    with pytest.raises(L.ScailHipError, match=r"tile 1: frame index 2 is repeated inside one tile \(tile frames 1 and 3\)"):
        _sample_tiled(L, [GOOD[0], [1, 2, 3, 2], GOOD[2]], 6)
    # a frame covered by no tile
    with pytest.raises(L.ScailHipError, match=r"frame 6 of \[0, T = 7\) is covered by no tile"):
        _sample_tiled(L, GOOD, 7)
    # inv_wsum: non-finite / non-positive
    for bad, shown in ((0.0, "0.0"), (-1.0, "-1.0"), (float("inf"), "inf"), (float("nan"), "nan")):
        with pytest.raises(L.ScailHipError, match=r"inv_wsum\[2\] = -?" + re.escape(shown.lstrip("-")) + r"\S* must be finite and positive"):
            _sample_tiled(L, GOOD, 6, inv=[0.5, 0.5, bad, 0.5, 0.5, 0.5])
    # null pointers: the host arrays first, then the handle / device pointers, each by name
    for key, name in (("fr", "tile_frames"), ("tw", "tile_w"), ("iw", "inv_wsum")):
        with pytest.raises(L.ScailHipError, match="null pointer: " + name):
            _sample_tiled(L, GOOD, 6, **{key: None})
    with pytest.raises(L.ScailHipError, match="null pointer: handle"):
        _sample_tiled(L, GOOD, 6)
    # a workspace that is too small: the pair buffers and den alone (2 * 2 * 4 * 1024 * 4 + 6 * 1024 * 4 bytes at H = W = 8) do not fit
    with pytest.raises(L.ScailHipError, match=r"workspace too small: 1000 bytes cannot hold .* \(90112 bytes\)"):
        _sample_tiled(L, GOOD, 6, ws_bytes=1000)


def test_tile_operator_refusals_are_host_side(L):
    fr = (C.c_int32 * 4)(0, 5, 2, 2)
    w = (C.c_float * 4)(1, 1, 1, 1)
    with pytest.raises(L.ScailHipError, match=r"scail_tile_blend_acc: frame index 2 is repeated inside one tile"):
        L.call("scail_tile_blend_acc", A, A, fr, w, 4, 6, 64, 4.0, None)
    with pytest.raises(L.ScailHipError, match=r"scail_tile_gather: frame index 5 \(tile frame 1\) is outside \[0, T = 5\)"):
        L.call("scail_tile_gather", A, A, fr, 4, 5, 64, None)
    with pytest.raises(L.ScailHipError, match=r"scail_tile_gather: the tile length Tt must be 1\.\.min\(T, 64\), got Tt = 4 with T = 3"):
        L.call("scail_tile_gather", A, A, fr, 4, 3, 64, None)
    L.call("scail_tile_gather", A, A, fr, 4, 6, 0, None)          # an empty frame is accepted and launches nothing
    L.call("scail_tile_finish", A, A, w, 4, 0, -0.5, None)


# ---- the planner ----------------------------------------------------------------------------------------------------------------------
def test_plan_tiles_grid():
    from scail_amd.cli import plan_tiles
    from scail_amd.sampler import RFSamplerLong as R
    n_cases = 0
    for Tt in (2, 3, 4, 5, 8, 21):
        for overlap in range(1, Tt):
            for T in list(range(1, 3 * Tt + 3)) + [41, 100]:
                tiles = plan_tiles(T, Tt, overlap)
                if T <= Tt:
                    assert tiles is None, (T, Tt, overlap)
                    continue
                n_cases += 1
                assert len(tiles) >= 2
                assert all(len(t) == Tt and t == list(range(t[0], t[0] + Tt)) for t in tiles), (T, Tt, overlap)
                assert tiles[0][0] == 0 and tiles[-1][-1] == T - 1
                assert sorted(set(f for t in tiles for f in t)) == list(range(T))
                starts = [t[0] for t in tiles]
                assert all(b - a == Tt - overlap for a, b in zip(starts[:-2], starts[1:-1]))          # regular stride up to the final tile
                assert 0 < starts[-1] - starts[-2] <= Tt - overlap
                # the weight sums RFSamplerLong forms from the plan
                wsum = torch.zeros(T)
                for k, t in enumerate(tiles):
                    wsum[torch.tensor(t)] += R._mult(k, len(tiles)) * R.tile_weight(Tt)
                assert bool((wsum > 0).all()) and bool(torch.isfinite(1.0 / wsum).all())
    assert n_cases > 500
    assert plan_tiles(7, 4, 2) == [[0, 1, 2, 3], [2, 3, 4, 5], [3, 4, 5, 6]]
    assert [t[0] for t in plan_tiles(41, 21, 10)] == [0, 11, 20]
    for T, Tt, ov in ((9, 4, 0), (9, 4, 4), (9, 4, -1), (9, 1, 1)):
        with pytest.raises(ValueError, match="overlap"):
            plan_tiles(T, Tt, ov)


def test_tile_args_and_cli_argument_checks(capsys):
    from scail_amd import cli
    assert cli.tile_args(None, None, 81) == (21, 10) and cli.tile_args(None, None, 13) == (4, 2)
    assert cli.tile_args(13, 4, 81) == (4, 1) and cli.tile_args(81, 44, 13) == (21, 11)
    with pytest.raises(ValueError, match="multiple of 4"):
        cli.tile_args(13, 6, 13)
    with pytest.raises(ValueError, match="smaller than the window"):
        cli.tile_args(13, 16, 13)
    with pytest.raises(ValueError, match="4n \\+ 1"):
        cli.tile_args(14, None, 13)
    # the same through the command line: an argparse error (exit status 2) before any model is built
    for argv, msg in ((["--tiny", "--tile-overlap", "6"], "multiple of 4"),
                      (["--tiny", "--tile-frames", "13", "--tile-overlap", "16"], "smaller than the window"),
                      (["--tiny", "--tile-overlap", "16"], "smaller than the window"),          # --tiny's window: 13 frames
                      (["--tiny", "--tile-frames", "12"], "4n \\+ 1")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2
        assert re.search(msg, capsys.readouterr().err)


# ---- which requests take the one call ------------------------------------------------------------------------------------------------
def test_one_call_route_declines_what_the_entry_point_does_not_cover():
    """scail_dit_sample_tiled is one character, tiles of at most 64 latent frames, one rank: everything else the Python loop of
    RFSamplerLong.sample_hip ran before must keep running there"""
    from types import SimpleNamespace
    from scail_amd.dit import DiffusionTransformer
    from scail_amd.sampler import RFSamplerLong as R

    def mk(**kw):
        """a stand-in network that answers with DiffusionTransformer's own rule from these attributes"""
        fake = SimpleNamespace(**dict(dict(use_c_step=True, kernel_timer=None, _tap=None, sp=None), **kw))
        fake.executor_ok = lambda **k: DiffusionTransformer.executor_ok(fake, **k)
        return fake

    net = mk()
    T, Tt, n = 9, 4, 3
    tiles = [[0, 1, 2, 3], [3, 4, 5, 6], [5, 6, 7, 8]]
    x = torch.zeros(1, T, 16, 8, 8)
    ref = torch.zeros(1, 1, 16, 8, 8)
    smpl = torch.zeros(1, n, Tt, 16, 4, 4)
    ok = lambda **kw: R._one_call_ok(**dict(dict(network=net, x=x, ref_concat=ref, smpl_tiled=smpl, tile_indices=tiles, step_callback=None,
                                                 chunk_dim=None), **kw))
    assert ok() is True
    # several characters with tiles: two reference frames, pose tiles of 2 * Tt frames
    assert ok(ref_concat=torch.zeros(1, 2, 16, 8, 8), smpl_tiled=torch.zeros(1, n, 2 * Tt, 16, 4, 4)) is False
    assert ok(ref_concat=torch.zeros(1, 2, 16, 8, 8)) is False
    assert ok(smpl_tiled=torch.zeros(1, n, 2 * Tt, 16, 4, 4)) is False
    # tiles longer than the 64 frames whose indices fit the kernel arguments
    long_tiles = [list(range(0, 65)), list(range(35, 100))]
    assert ok(x=torch.zeros(1, 100, 16, 4, 4), tile_indices=long_tiles, smpl_tiled=torch.zeros(1, 2, 65, 16, 2, 2)) is False
    edge = [list(range(0, 64)), list(range(36, 100))]
    assert ok(x=torch.zeros(1, 100, 16, 4, 4), tile_indices=edge, smpl_tiled=torch.zeros(1, 2, 64, 16, 2, 2)) is True
    # RFSampler's own conditions
    assert ok(step_callback=lambda i, xx: None) is False and ok(chunk_dim=3) is False
    assert ok(x=torch.zeros(2, T, 16, 8, 8)) is False and ok(ref_concat=torch.zeros(2, 1, 16, 8, 8)) is False
    assert ok(smpl_tiled=torch.zeros(2, n, Tt, 16, 4, 4)) is False and ok(smpl_tiled=torch.zeros(1, n + 1, Tt, 16, 4, 4)) is False
    for kw in (dict(use_c_step=False), dict(kernel_timer=object()), dict(_tap=object()), dict(sp=SimpleNamespace(size=2))):
        assert ok(network=mk(**kw)) is False
    assert ok(network=mk(sp=SimpleNamespace(size=1))) is True
    # a network that does not state the rule (any other nn.Module) keeps the generic loop
    assert ok(network=SimpleNamespace(use_c_step=True, kernel_timer=None, _tap=None, sp=None)) is False


def test_cli_run_refuses_a_long_clip_that_is_not_4n_plus_1_before_sampling():
    """n_pix beyond the window and not 4n + 1: an error that names the frame count (checked right after the reference frame's encode)"""
    from types import SimpleNamespace
    from scail_amd import cli
    engine = SimpleNamespace(network=SimpleNamespace(num_frames=13, text_dim=64), encode_first_stage=lambda *a, **k: torch.zeros(1, 16, 1, 8, 8))
    req = dict(ref=torch.zeros(3, 1, 64, 64), pose=torch.zeros(3, 26, 32, 32))
    with pytest.raises(ValueError, match=r"longer than one window needs 4n \+ 1 frames .* got 26\b"):
        cli.run(cli.TINY, req, engine=engine, device="cpu")
