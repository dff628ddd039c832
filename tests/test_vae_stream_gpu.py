"""GPU tests of the streamed VAE decode (include/scail_vae.h scail_vae_decode_stream; WanVAE_.decode(z, chunk_frames=N)).

Streamed and whole-sequence decode compute every output voxel from the same inputs through the same kernels, so they are compared BITWISE
-- after asserting, on the host (tests/vae_stream_dispatch.py), that every launch picks the same kernel for the chunk's geometry as for the
clip's: a shape that straddles a dispatch threshold would read as wrong arithmetic otherwise.  Against the reference: the goldens and
tolerances of tests/test_vae_gpu.py test_vae_decode_vs_reference_golden, copied verbatim."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import wan_vae_oracle as V

import vae_stream_dispatch as D

pytestmark = pytest.mark.gpu
DEV = "cuda"

_models, _whole = {}, {}


def _model(dim):
    from scail_amd.wan_vae import WanVAE_
    if dim not in _models:
        _models[dim] = WanVAE_(dim=dim, z_dim=16, device=DEV)
    return _models[dim]


def _latent(Tl, hl, wl):
    g = torch.Generator().manual_seed(1000 * Tl + 10 * hl + wl)
    return torch.randn(1, 16, Tl, hl, wl, generator=g).to(DEV)


def _whole_decode(dim, Tl, hl, wl):
    """the whole-sequence decode of the case's latent, computed once and shared"""
    key = (dim, Tl, hl, wl)
    if key not in _whole:
        _whole[key] = _model(dim).decode(_latent(Tl, hl, wl))
    return _whole[key]


def _cos(a, b):
    a, b = a.flatten().double(), b.flatten().double()
    return float((a @ b) / (a.norm() * b.norm()))


# Tl = 7 at 6 x 8: chunks 3 and 6 merge a one-frame remainder (3 + 4; 7 = chunk + 1 is ONE chunk), chunk 2 leaves the first chunk's time
# convolutions a one-frame tail, chunks 4 and 5 end on a short chunk; Tl = 2 is a single chunk; 5 x 9 has ragged 16 x 16 tiles at every stage
CASES = [(7, 6, 8, c) for c in (2, 3, 4, 5, 6)] + [(2, 6, 8, 2), (7, 5, 9, 2), (7, 5, 9, 3)]


@pytest.mark.parametrize("dim", [32, 96])
@pytest.mark.parametrize("Tl,hl,wl,chunk", CASES)
def test_streamed_equals_whole_bitwise(dim, Tl, hl, wl, chunk):
    m = _model(dim)
    diffs = D.dispatch_differences(m, Tl, hl, wl, chunk)
    assert not diffs, f"chunk and clip geometry pick different kernels (a dispatch difference, not arithmetic): {diffs}"
    whole = _whole_decode(dim, Tl, hl, wl)
    got = m.decode(_latent(Tl, hl, wl), chunk_frames=chunk)
    assert got.shape == whole.shape == (1, 3, 1 + 4 * (Tl - 1), 8 * hl, 8 * wl)
    assert bool(torch.isfinite(got).all())
    print(f"dim {dim} Tl {Tl} {hl}x{wl} chunk {chunk} plan {D.chunk_plan(Tl, chunk)}: max |streamed - whole| = {float((got - whole).abs().max()):.3e}")
    assert torch.equal(got, whole)


def _golden(golden_dir, name):
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(golden_dir, name)).items()}
    from scail_amd.wan_vae import WanVAE_
    cfg = V.VAEConfig(dim=int(g["dim"]), z_dim=16)
    sd = V.make_state_dict(cfg, seed=int(g["seed"]))
    m = WanVAE_(dim=cfg.dim, z_dim=16, device=DEV)
    missing, unexpected = m.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    return g, m


# vae_tiny.npz and vae_dim96.npz hold 3 latent frames: with chunk_frames = 2 that is Tl <= chunk + 1, ONE chunk -- the whole-sequence launches
# through the streamed entry point, no streaming coverage (test_streamed_equals_whole_bitwise carries that for both widths).  vae_tiny2.npz
# holds 4: two chunks of two.
@pytest.mark.parametrize("name,chunks", [("vae_tiny.npz", 1), ("vae_tiny2.npz", 2), ("vae_dim96.npz", 1)])
def test_streamed_decode_vs_reference_golden(golden_dir, name, chunks):
    g, m = _golden(golden_dir, name)
    assert len(D.chunk_plan(g["z_in"].shape[2], 2)) == chunks
    rec = m.decode(g["z_in"].to(DEV), chunk_frames=2).clamp(-1, 1).cpu()
    assert rec.shape == g["rec"].shape
    torch.testing.assert_close(rec, g["rec"], rtol=3e-2, atol=3e-2)
    assert _cos(rec, g["rec"]) >= 0.999


def test_memory_is_bounded_by_the_chunk():
    """dim 32, 6 x 8, chunk_frames = 4: the workspace CVae allocates is the same for a 5-frame and a 41-frame latent, and the 41-frame result
    equals the whole-sequence decode."""
    m = _model(32)
    c = m._c()
    m.decode(_latent(5, 6, 8), chunk_frames=4)
    ws5 = c._ws.numel()
    got = m.decode(_latent(41, 6, 8), chunk_frames=4)
    ws41 = c._ws.numel()
    assert ws5 == ws41 == __import__("scail_amd.lib", fromlist=["load"]).load().scail_vae_decode_stream_workspace_bytes(c._h, 4, 6, 8)
    whole = _whole_decode(32, 41, 6, 8)
    assert c._ws.numel() > ws41            # the whole-sequence workspace of the same clip is the larger one
    diffs = D.dispatch_differences(m, 41, 6, 8, 4)
    print(f"Tl 41: workspace {ws41} B streamed, {c._ws.numel()} B whole; max |streamed - whole| = {float((got - whole).abs().max()):.3e}; "
          f"dispatch differences: {sorted(set((n, a, b) for _, n, a, b in diffs))}")
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, whole)


def test_refusals_enqueue_nothing():
    from scail_amd import lib as L
    m = _model(32)
    z = _latent(7, 6, 8)
    with pytest.raises(ValueError, match="at least 2 latent frames, got 1"):
        m.decode(z, chunk_frames=1)
    c = m._c()
    need = L.load().scail_vae_decode_stream_workspace_bytes(c._h, 4, 6, 8)
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    out = torch.full((3, 25, 48, 64), 7.0, device=DEV)
    zz = z[0].contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(L.ScailHipError, match="chunk must be at least 2 latent frames.*got 1"):
        L.call("scail_vae_decode_stream", c._h, zz.data_ptr(), out.data_ptr(), 7, 6, 8, 1, ws.data_ptr(), need, stream)
    with pytest.raises(L.ScailHipError, match=f"workspace too small.*need {need} bytes, got {need - 1}"):
        L.call("scail_vae_decode_stream", c._h, zz.data_ptr(), out.data_ptr(), 7, 6, 8, 4, ws.data_ptr(), need - 1, stream)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())         # nothing was enqueued: the output is untouched
    m.use_c_exec = False
    try:
        with pytest.raises(NotImplementedError, match="chunk_frames"):
            m.decode(z, chunk_frames=4)
    finally:
        m.use_c_exec = True
    # and the same buffers with a full workspace do run
    L.call("scail_vae_decode_stream", c._h, zz.data_ptr(), out.data_ptr(), 7, 6, 8, 4, ws.data_ptr(), need, stream)
    assert torch.equal(out, _whole_decode(32, 7, 6, 8)[0])


@pytest.mark.parametrize("T,hw,t0,n", [(7, 45, 2, 3), (7, 45, 0, 7), (5, 48, 1, 3), (3, 45, 2, 1)])
def test_frame_window_layout_kernels(T, hw, t0, n):
    """scail_to_channels_last_frames / scail_from_channels_last_frames: a window of frames out of a planar tensor and back, against torch
    indexing, bitwise; hl * wl = 45 puts offset and length off every multiple of the vector width (dword path), 48 on it (float4 path)."""
    from scail_amd import lib as L
    g = torch.Generator().manual_seed(T * 100 + hw + t0)
    stream = torch.cuda.current_stream().cuda_stream
    for Cc, Cpad in ((16, 16), (3, 8)):
        x = torch.randn(Cc, T, hw, generator=g).to(DEV)
        # scales that are powers of two: x * a is exact, so the result does not depend on whether the compiler fuses the multiply and the add
        a, b = (2.0 ** torch.randint(-1, 2, (Cc,), generator=g)).to(DEV), torch.randn(Cc, generator=g).to(DEV)
        y = torch.full((n * hw + 3, Cpad), -5.0, device=DEV, dtype=torch.bfloat16)[:n * hw]      # (guard rows behind the window)
        L.call("scail_to_channels_last_frames", x.data_ptr(), y.data_ptr(), a.data_ptr(), b.data_ptr(), Cc, Cpad, T * hw, t0 * hw, n * hw, stream)
        ref = torch.zeros(n * hw, Cpad, device=DEV)
        ref[:, :Cc] = (x[:, t0:t0 + n].reshape(Cc, n * hw) * a[:, None] + b[:, None]).t()
        assert torch.equal(y, ref.to(torch.bfloat16))
        back = torch.full((Cc, T, hw), 9.0, device=DEV)
        L.call("scail_from_channels_last_frames", y.data_ptr(), Cpad, back.data_ptr(), a.data_ptr(), b.data_ptr(), Cc, T * hw, t0 * hw, n * hw,
               -0.75, 0.75, stream)
        want = torch.full((Cc, T, hw), 9.0, device=DEV)               # frames outside the window stay untouched
        want[:, t0:t0 + n] = ((y[:, :Cc].float() + b) * a).clamp(-0.75, 0.75).t().reshape(Cc, n, hw)
        assert torch.equal(back, want)
        # the whole tensor as one window equals the whole-tensor kernels
        if t0 == 0 and n == T:
            y0 = torch.empty(n * hw, Cpad, device=DEV, dtype=torch.bfloat16)
            L.call("scail_to_channels_last", x.data_ptr(), y0.data_ptr(), a.data_ptr(), b.data_ptr(), Cc, Cpad, T * hw, stream)
            assert torch.equal(y, y0)
