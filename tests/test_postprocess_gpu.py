"""GPU tests of the uint8 output route: scail_frames_u8 (include/scail_hip.h), scail_vae_decode_u8 / scail_vae_decode_stream_u8
(include/scail_vae.h; WanVAE_.decode_u8) and ``cli.run(postprocess="hip")``.

The kernel's arithmetic is the default route's, operation by operation in fp32 (tests/postprocess_ref.py restates it in numpy), and its input
is the bf16 tensor the fp32 decode widens exactly -- so everything here is compared BITWISE: every bf16 bit pattern through the kernel, and
every decode against the quantised fp32 decode of the same chunking (the same launches up to the last one, so the comparison does not lean on
streamed and whole-sequence decodes picking the same kernels)."""
import numpy as np
import pytest
import torch

from postprocess_ref import quantise

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = 0xA5

_models, _fp32 = {}, {}


def _model(dim):
    from scail_amd.wan_vae import WanVAE_
    if dim not in _models:
        _models[dim] = WanVAE_(dim=dim, z_dim=16, device=DEV)
    return _models[dim]


def _latent(Tl, hl, wl):
    g = torch.Generator().manual_seed(1000 * Tl + 10 * hl + wl)
    return torch.randn(1, 16, Tl, hl, wl, generator=g).to(DEV)


def _quantised_decode(dim, Tl, hl, wl, chunk=None):
    """the fp32 decode of the case's latent (whole sequence, or streamed with ``chunk``), quantised on the host and moved to (1, T, H, W, 3);
    computed once and shared"""
    key = (dim, Tl, hl, wl, chunk)
    if key not in _fp32:
        x = _model(dim).decode(_latent(Tl, hl, wl), chunk_frames=chunk)
        assert bool(torch.isfinite(x).all())
        _fp32[key] = torch.from_numpy(quantise(x.cpu().numpy())).permute(0, 2, 3, 4, 1).contiguous()
    return _fp32[key]


def _bf16_from_bits(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(bits.astype(np.uint16).view(np.int16)).view(torch.bfloat16)


def _frames_u8(x, out, offset, row_bytes, frame_bytes, n, H, W):
    from scail_amd import lib as L
    L.call("scail_frames_u8", x.data_ptr(), x.shape[1], out.data_ptr() + offset, row_bytes, frame_bytes, n, H, W,
           torch.cuda.current_stream().cuda_stream)


def test_every_bf16_value():
    """8 frames of 64 x 64, ldx = 8: channels 0..2 hold all 65 536 bf16 bit patterns (and random ones in the remaining slots), channels 3..7
    NaN patterns that must never be read as pixels.  Finite and infinite values: the numpy restatement, exactly; NaN: 0."""
    n, H, W = 8, 64, 64
    rng = np.random.default_rng(5)
    slots = n * H * W * 3
    bits = np.concatenate([np.arange(65536, dtype=np.uint32), rng.integers(0, 65536, slots - 65536, dtype=np.uint32)])
    bits = bits[rng.permutation(slots)].reshape(n * H * W, 3)
    assert len(np.unique(bits)) == 65536
    rows = np.empty((n * H * W, 8), dtype=np.uint32)
    rows[:, :3] = bits
    rows[:, 3:] = rng.choice(np.array([0x7FC0, 0xFFC0, 0x7F81, 0xFFFF, 0x7FFF], dtype=np.uint32), size=(n * H * W, 5))
    x = _bf16_from_bits(rows).to(DEV)
    out = torch.full((n, H, W, 3), FILL, dtype=torch.uint8, device=DEV)
    _frames_u8(x, out, 0, 3 * W, 3 * W * H, n, H, W)
    got = out.cpu().numpy().reshape(-1, 3)
    v = (bits << 16).astype(np.uint32).view(np.float32)
    nan = np.isnan(v)
    assert nan.sum() >= 2 * 127 and np.isinf(v).sum() >= 2
    want = np.where(nan, np.uint8(0), quantise(np.where(nan, np.float32(0), v)))
    bad = np.nonzero(got != want)
    assert bad[0].size == 0, [(hex(int(bits[i, c])), int(got[i, c]), int(want[i, c])) for i, c in zip(bad[0][:8], bad[1][:8])]
    assert np.array_equal(got[np.isposinf(v)], np.full(np.isposinf(v).sum(), 255)) and not got[np.isneginf(v)].any()


# (name, offset of `out` in the buffer, row_bytes - 3 W, frame_bytes - H * row_bytes, frames in the buffer, first frame, ldx)
LAYOUTS = [("offset 1", 1, 0, 0, 3, 0, 8), ("offset 3", 3, 0, 0, 3, 0, 8), ("padded rows and frames", 0, 7, 5, 3, 0, 8),
           ("padded frames", 2, 0, 5, 3, 0, 8), ("frames 2-4 of 7", 0, 0, 0, 7, 2, 16)]


@pytest.mark.parametrize("H,W", [(40, 72), (3, 5)])
@pytest.mark.parametrize("name,offset,row_pad,frame_pad,n_buf,first,ldx", LAYOUTS)
def test_layout(H, W, name, offset, row_pad, frame_pad, n_buf, first, ldx):
    """3 frames whose pixel counts are off every vector width, written at odd addresses, with gaps behind rows and frames, and as a window of a
    longer clip: the pixels equal a dense call's (itself checked against the restatement) and every other byte keeps its fill value."""
    n = 3
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.full((n * H * W, ldx), float("nan"), dtype=torch.bfloat16)
    x[:, :3] = (torch.rand(n * H * W, 3, generator=g) * 3.0 - 1.5).to(torch.bfloat16)
    want = quantise(x[:, :3].float().numpy()).reshape(n, H, 3 * W)
    x = x.to(DEV)
    dense = torch.full((n, H, W, 3), FILL, dtype=torch.uint8, device=DEV)
    _frames_u8(x, dense, 0, 3 * W, 3 * W * H, n, H, W)
    assert np.array_equal(dense.cpu().numpy().reshape(n, H, 3 * W), want)
    row_bytes = 3 * W + row_pad
    frame_bytes = H * row_bytes + frame_pad
    size = offset + n_buf * frame_bytes + 64
    buf = torch.full((size,), FILL, dtype=torch.uint8, device=DEV)
    _frames_u8(x, buf, offset + first * frame_bytes, row_bytes, frame_bytes, n, H, W)
    exp = np.full(size, FILL, dtype=np.uint8)
    for t in range(n):
        for y in range(H):
            at = offset + (first + t) * frame_bytes + y * row_bytes
            exp[at:at + 3 * W] = want[t, y]
    got = buf.cpu().numpy()
    assert np.array_equal(got, exp), f"{name}: first differing byte {int(np.nonzero(got != exp)[0][0])} of {size}"


SHAPES = [(7, 6, 8), (7, 5, 9)]            # the latents of tests/test_vae_stream_gpu.py: 5 x 9 has ragged tiles at every stage


@pytest.mark.parametrize("dim", [32, 96])
@pytest.mark.parametrize("Tl,hl,wl", SHAPES)
def test_decode_u8_equals_the_quantised_decode(dim, Tl, hl, wl):
    got = _model(dim).decode_u8(_latent(Tl, hl, wl))
    assert got.dtype == torch.uint8 and got.is_cuda and got.shape == (1, 1 + 4 * (Tl - 1), 8 * hl, 8 * wl, 3)
    want = _quantised_decode(dim, Tl, hl, wl)
    assert len(torch.unique(want)) > 16                 # a picture, not a constant
    assert torch.equal(got.cpu(), want)


# chunk 2: the first chunk's time convolutions see a one-frame tail; 3: a one-frame remainder joins the last chunk; 6: Tl = chunk + 1 is ONE chunk
@pytest.mark.parametrize("dim", [32, 96])
@pytest.mark.parametrize("Tl,hl,wl", SHAPES)
@pytest.mark.parametrize("chunk", [2, 3, 6])
def test_streamed_decode_u8_equals_the_quantised_streamed_decode(dim, Tl, hl, wl, chunk):
    got = _model(dim).decode_u8(_latent(Tl, hl, wl), chunk_frames=chunk)
    assert got.dtype == torch.uint8 and got.shape == (1, 1 + 4 * (Tl - 1), 8 * hl, 8 * wl, 3)
    assert torch.equal(got.cpu(), _quantised_decode(dim, Tl, hl, wl, chunk))


def test_memory_is_the_workspace_and_the_uint8_clip():
    """dim 32, 6 x 8, chunk_frames = 4, a 41-frame latent: the call allocates the streamed workspace, of exactly the query's size, and the
    T * H * W * 3-byte result -- nothing else is alive at its peak, an fp32 clip (4 x the result) least of all.  torch's allocator rounds a
    request up to 512 bytes and hands out a cached or fresh block whole when what would remain of it is under 1 MiB: that much per allocation
    is the only slack."""
    from scail_amd import lib as L
    m = _model(32)
    c = m._c()
    Tl, hl, wl = 41, 6, 8
    T, H, W = 1 + 4 * (Tl - 1), 8 * hl, 8 * wl
    z = _latent(Tl, hl, wl)
    c._ws = None
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = m.decode_u8(z, chunk_frames=4)
    torch.cuda.synchronize()
    peak, after = torch.cuda.max_memory_allocated(), torch.cuda.memory_allocated()
    need = L.load().scail_vae_decode_stream_workspace_bytes(c._h, 4, hl, wl)
    assert c._ws.numel() == need
    assert got.shape == (1, T, H, W, 3) and got.numel() == T * H * W * 3
    total = need + T * H * W * 3
    print(f"workspace {need} B + result {T * H * W * 3} B = {total} B; allocated by the call {after - base} B, peak {peak - base} B")
    assert peak == after                               # nothing beyond what the call leaves alive: the workspace and the result
    assert total <= after - base <= total + 2 * ((1 << 20) + 512)
    assert torch.equal(got.cpu(), _quantised_decode(32, Tl, hl, wl, 4))


def test_refusals_enqueue_nothing():
    from scail_amd import lib as L
    m = _model(32)
    Tl, hl, wl = 7, 6, 8
    T, H, W = 25, 48, 64
    c = m._c()
    zz = _latent(Tl, hl, wl)[0].contiguous()
    need = L.load().scail_vae_decode_stream_workspace_bytes(c._h, 4, hl, wl)
    whole = L.load().scail_vae_workspace_bytes(c._h, T, H, W)
    ws = torch.empty(max(need, whole), device=DEV, dtype=torch.uint8)
    frames = torch.full((T, H, W, 3), 7, device=DEV, dtype=torch.uint8)
    x = torch.zeros(T * H * W, 8, device=DEV, dtype=torch.bfloat16)
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(ValueError, match="at least 2 latent frames, got 1"):
        m.decode_u8(zz, chunk_frames=1)
    for needle, fn, args in [
            ("chunk must be at least 2 latent frames.*got 1", "scail_vae_decode_stream_u8", (c._h, zz.data_ptr(), frames.data_ptr(), Tl, hl, wl, 1, ws.data_ptr(), need, stream)),
            (f"workspace too small.*need {need} bytes, got {need - 1}", "scail_vae_decode_stream_u8", (c._h, zz.data_ptr(), frames.data_ptr(), Tl, hl, wl, 4, ws.data_ptr(), need - 1, stream)),
            ("workspace too small", "scail_vae_decode_u8", (c._h, zz.data_ptr(), frames.data_ptr(), Tl, hl, wl, ws.data_ptr(), whole - 1, stream)),
            ("null argument", "scail_vae_decode_u8", (c._h, None, frames.data_ptr(), Tl, hl, wl, ws.data_ptr(), whole, stream)),
            (f"row_bytes = {3 * W - 1}", "scail_frames_u8", (x.data_ptr(), 8, frames.data_ptr(), 3 * W - 1, 3 * W * H, T, H, W, stream)),
            (f"frame_bytes = {3 * W * H - 1}", "scail_frames_u8", (x.data_ptr(), 8, frames.data_ptr(), 3 * W, 3 * W * H - 1, T, H, W, stream)),
            ("ldx = 12", "scail_frames_u8", (x.data_ptr(), 12, frames.data_ptr(), 3 * W, 3 * W * H, T, H, W, stream)),
            ("ends in 2", "scail_frames_u8", (x.data_ptr() + 2, 8, frames.data_ptr(), 3 * W, 3 * W * H, T, H, W, stream))]:
        with pytest.raises(L.ScailHipError, match=needle):
            L.call(fn, *args)
    torch.cuda.synchronize()
    assert bool((frames == 7).all())                   # nothing was enqueued: the frames are untouched
    # and the same buffers with valid arguments do run
    L.call("scail_vae_decode_stream_u8", c._h, zz.data_ptr(), frames.data_ptr(), Tl, hl, wl, 4, ws.data_ptr(), need, stream)
    assert torch.equal(frames.cpu(), _quantised_decode(32, Tl, hl, wl, 4)[0])
    frames.fill_(7)
    L.call("scail_vae_decode_u8", c._h, zz.data_ptr(), frames.data_ptr(), Tl, hl, wl, ws.data_ptr(), whole, stream)
    assert torch.equal(frames.cpu(), _quantised_decode(32, Tl, hl, wl)[0])


def test_through_the_cli():
    from scail_amd import cli
    engine = cli.build_engine(cli.TINY)
    video, z, _ = cli.run(cli.TINY, steps=2, engine=engine, postprocess="hip")
    B, C, Tl, h, w = z.shape
    assert video.dtype == torch.uint8 and video.is_cuda and video.shape == (1, 1 + 4 * (Tl - 1), 8 * h, 8 * w, 3)
    x = engine.decode_first_stage(z.float())                                # fp32 (1, 3, T, H, W) in [-1, 1]: the default route's decode
    want = torch.from_numpy(quantise(x.cpu().numpy())).permute(0, 2, 3, 4, 1).contiguous()
    assert len(torch.unique(want)) > 16
    assert torch.equal(video.cpu(), want)
