"""Host-side checks of the uint8 output route (include/scail_hip.h scail_frames_u8, include/scail_vae.h scail_vae_decode_u8 /
scail_vae_decode_stream_u8, ``cli.run(postprocess="hip")``, ``video_io.save_multi_video_grid`` with uint8 clips): the entry points are
declared, exported and bound; bad arguments are refused before anything touches a device, naming the value; the writer makes the same files
of uint8 clips as of the float clips they were quantised from.  The arithmetic itself is tests/test_postprocess_gpu.py's."""
import os
import re

import numpy as np
import pytest
import torch

from postprocess_ref import quantise
from test_vae_stream_cpu import handle  # noqa: F401  (the null-weight scail_vae handle of the shipped architecture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("scail_frames_u8", "scail_vae_decode_u8", "scail_vae_decode_stream_u8")


@pytest.fixture(scope="module")
def L():
    from scail_amd import build, lib
    build.build(verbose=False)
    lib.load()
    return lib


def test_entry_points_are_declared_bound_and_exported(L):
    lib = L.load()
    header = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("scail_hip.h", "scail_vae.h"))
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in L.SIGNATURES, name
        assert hasattr(lib, name), name
    assert len(L.SIGNATURES["scail_frames_u8"]) == 9
    assert L.SIGNATURES["scail_vae_decode_u8"] == L.SIGNATURES["scail_vae_decode"]
    assert L.SIGNATURES["scail_vae_decode_stream_u8"] == L.SIGNATURES["scail_vae_decode_stream"]
    assert lib.scail_abi_version() == L.ABI_VERSION          # entry points were added, none changed (include/scail_hip.h scail_abi_version)
    from scail_amd import cvae, engine, wan_vae
    assert hasattr(cvae.CVae, "decode_u8") and hasattr(wan_vae.WanVAE_, "decode_u8") and hasattr(wan_vae.WanVAE, "decode_u8")
    assert hasattr(engine.SATVideoDiffusionEngine, "decode_first_stage_u8")


def test_frames_u8_refusals_without_gpu(L):
    A = 0x1000        # a fake 16-byte aligned device address: the checks fail before it is ever dereferenced
    H, W = 6, 10
    dense = dict(x=A, ldx=8, out=A, row=3 * W, frame=3 * W * H, n=2, H=H, W=W)

    def call(**kw):
        p = dict(dense, **kw)
        L.call("scail_frames_u8", p["x"], p["ldx"], p["out"], p["row"], p["frame"], p["n"], p["H"], p["W"], None)

    cases = [
        (f"row_bytes = {3 * W - 1}", dict(row=3 * W - 1)),
        (f"frame_bytes = {H * 3 * W - 1}", dict(frame=H * 3 * W - 1)),
        (f"frame_bytes = {H * (3 * W + 7) - 1}", dict(row=3 * W + 7, frame=H * (3 * W + 7) - 1)),
        ("ldx = 12", dict(ldx=12)),
        ("ldx = 0", dict(ldx=0)),
        ("null pointer: out", dict(out=None)),
        ("null pointer: x", dict(x=None)),
        ("16-byte aligned rows.*ends in 8", dict(x=A + 8)),
        ("n_frames = -1", dict(n=-1)),
        ("W = -2", dict(W=-2, row=0)),
    ]
    for needle, kw in cases:
        with pytest.raises(L.ScailHipError, match=needle):
            call(**kw)
    # the empty problem is accepted and launches nothing (no device is needed), whichever size is zero; `out` needs no alignment
    call(n=0)
    call(H=0, frame=0)
    call(W=0, out=A + 3)


def test_decode_u8_refusals_are_those_of_the_fp32_calls(L, handle):  # noqa: F811
    lib = L.load()
    A = 0x10000       # a fake 256-byte aligned device address
    need = lib.scail_vae_decode_stream_workspace_bytes(handle, 4, 6, 8)

    def message(fn, *args):
        with pytest.raises(L.ScailHipError) as e:
            L.call(fn, *args)
        msg = str(e.value).split(" failed ", 1)[1]            # the library's message behind the binding's "<entry point> failed "
        assert f": {fn}: " in msg, msg                        # it names the entry point that was called ...
        return msg.replace(f": {fn}: ", ": ")                 # ... and is otherwise the same text

    for args, needle in (((handle, A, A, 7, 6, 8, 1, A, need, None), "chunk must be at least 2 latent frames.*got 1"),
                         ((handle, A, A, 7, 6, 8, 4, A, need - 1, None), f"workspace too small.*need {need} bytes, got {need - 1}"),
                         ((handle, A, None, 7, 6, 8, 4, A, need, None), "null argument"),
                         ((handle, A, A, 7, 6, 8, 4, A + 16, need, None), "not 256-byte aligned")):
        got = message("scail_vae_decode_stream_u8", *args)
        assert re.search(needle, got), got
        assert got == message("scail_vae_decode_stream", *args)
    whole = lib.scail_vae_workspace_bytes(handle, 25, 48, 64)
    for args, needle in (((handle, A, A, 7, 6, 8, A, whole - 1, None), "workspace too small"), ((handle, None, A, 7, 6, 8, A, whole, None), "null argument"),
                         ((handle, A, A, 0, 6, 8, A, whole, None), "bad latent shape")):
        got = message("scail_vae_decode_u8", *args)
        assert re.search(needle, got), got
        assert got == message("scail_vae_decode", *args)


def _clips(seed, B=1, T=3, H=6, W=10):
    """a float clip (B, T, C, H, W) whose values are clamp((bf16 + 1) / 2, 0, 1) for random bf16 values in [-1.5, 1.5] -- what the default route
    hands the writer -- and its uint8 form (B, T, H, W, C) by the restatement above"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, T, 3, H, W, generator=g) * 3.0 - 1.5).to(torch.bfloat16)
    x[0, 0, :, 0, :4] = torch.tensor([-1.5, -1.0, 1.0, 1.5], dtype=torch.bfloat16)            # both clamps and both ends of the range
    fl = torch.clamp((x.float() + 1.0) / 2.0, 0.0, 1.0)
    u8 = torch.from_numpy(quantise(x.float().numpy())).permute(0, 1, 3, 4, 2).contiguous()
    return fl, u8


@pytest.mark.parametrize("ext", [".npy", "", ".webp"])
@pytest.mark.parametrize("n_clips", [1, 2])
def test_save_multi_video_grid_writes_the_same_files_for_uint8_clips(tmp_path, ext, n_clips):
    from scail_amd import video_io
    pairs = [_clips(11 + k, B=2) for k in range(n_clips)]
    pf = video_io.save_multi_video_grid([p[0] for p in pairs], str(tmp_path / "float"), fps=8, key="k", ext=ext)
    pu = video_io.save_multi_video_grid([p[1] for p in pairs], str(tmp_path / "u8"), fps=8, key="k", ext=ext)
    assert [os.path.basename(p) for p in pf] == [os.path.basename(p) for p in pu] == [f"k_{i:06d}{ext}" for i in range(2)]
    for i, (a, b) in enumerate(zip(pf, pu)):
        want = torch.cat([p[1][i] for p in pairs], dim=2)                                       # T H (n W) C: "h (n w) c" per frame
        if ext == ".npy":
            assert open(a, "rb").read() == open(b, "rb").read()
            assert np.array_equal(np.load(b), want.numpy())
        elif ext == "":
            assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == [f"{t:06d}.png" for t in range(want.shape[0])]
            for n in os.listdir(a):
                assert open(os.path.join(a, n), "rb").read() == open(os.path.join(b, n), "rb").read(), n
            assert torch.equal(video_io.load_video_for_pose_sample(b), want)
        else:
            fa, fb = video_io.load_video_for_pose_sample(a), video_io.load_video_for_pose_sample(b)       # lossless: the decoded pixels
            assert torch.equal(fa, fb) and torch.equal(fb, want)


def test_save_multi_video_grid_refuses_mixed_and_misshapen_uint8(tmp_path):
    from scail_amd import video_io
    fl, u8 = _clips(3)
    with pytest.raises(ValueError, match="all float .* or all uint8"):
        video_io.save_multi_video_grid([fl, u8], str(tmp_path), ext=".npy")
    with pytest.raises(ValueError, match="one shape"):
        video_io.save_multi_video_grid([u8, u8[:, :2]], str(tmp_path), ext=".npy")


def test_cli_arguments():
    from scail_amd import cli
    ap = cli.build_parser()
    assert ap.parse_args(["--tiny"]).postprocess == "torch"
    assert ap.parse_args(["--tiny", "--postprocess", "hip"]).postprocess == "hip"
    with pytest.raises(SystemExit):
        ap.parse_args(["--tiny", "--postprocess", "numpy"])
    with pytest.raises(ValueError, match="postprocess must be one of"):
        cli.run(cli.TINY, postprocess="numpy")


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_hip_route_has_no_host_fallback():
    from scail_amd import cli, lib
    with pytest.raises(lib.ScailHipError, match="GPU"):
        cli.run(cli.TINY, steps=2, postprocess="hip", device="cpu")


def test_layer_path_has_no_uint8_route():
    from scail_amd.wan_vae import WanVAE_
    m = WanVAE_(dim=32, z_dim=16, device="cpu")
    m._prepared, m.use_c_exec = {}, False
    with pytest.raises(NotImplementedError, match="C executor"):
        m.decode_u8(torch.zeros(1, 16, 7, 6, 8))
    with pytest.raises(NotImplementedError, match="C executor"):
        m.decode_u8(torch.zeros(1, 16, 7, 6, 8), chunk_frames=4)
