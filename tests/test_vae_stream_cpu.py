"""Host-side checks of the streamed VAE decode (include/scail_vae.h scail_vae_decode_stream): its workspace does not depend on the clip
length and is smaller than the whole-sequence decode's by the ratio of the frames their slots hold; bad arguments are refused before
anything touches a device.  The header / ctypes / export consistency of the new symbols is tests/test_abi.py's."""
import ctypes as C

import pytest

HL, WL = 64, 112          # 512 x 896


@pytest.fixture(scope="module")
def handle():
    """a scail_vae handle of the shipped architecture (dim 96) with null weight pointers: the workspace queries read channel widths, kernel
    extents and the stage table only"""
    from scail_amd import build
    build.build(verbose=False)
    from scail_amd import cvae, lib as L
    from scail_amd.wan_vae import WanVAE_
    m = WanVAE_(dim=96, z_dim=16, device="cpu")
    spec = m.param_spec()

    def conv(n, cout=None):
        if n + ".weight" not in spec:
            return cvae.ConvW(None, None, 0, 0, 0, 0, 0, 0)
        co, ci, *k = spec[n + ".weight"]
        k = tuple(k) if len(k) == 3 else (1, *k)
        co = cout or co
        ci8 = (ci + 7) // 8 * 8
        return cvae.ConvW(None, None, ci8, (co + 7) // 8 * 8, (k[0] * k[1] * k[2] * ci8 + 63) // 64 * 64, *k)

    def res(n):
        return cvae.Res(None, conv(n + ".residual.2"), None, conv(n + ".residual.6"), conv(n + ".shortcut"))

    plan = m.decoder_plan()
    dec = (cvae.Stage * len(plan))()
    for i, (kind, n, a, b) in enumerate(plan):
        if kind == "res":
            dec[i].kind, dec[i].res = 0, res(n)
        else:
            dec[i].kind, dec[i].temporal, dec[i].resample = 2, int(bool(b)), conv(n + ".resample.1")
            if b:
                dec[i].time_conv0 = dec[i].time_conv1 = conv(n + ".time_conv", cout=a)
    top = 96 * 4
    w = cvae.Weights()
    w.z_dim = 16
    w.enc_conv1 = conv("encoder.conv1")
    w.enc_attn.C = w.dec_attn.C = top
    w.conv2, w.dec_conv1 = conv("conv2"), conv("decoder.conv1")
    w.dec_mid0, w.dec_mid2 = res("decoder.middle.0"), res("decoder.middle.2")
    w.dec, w.n_dec = dec, len(plan)
    w.dec_head = conv("decoder.head.2")
    h = C.c_void_p()
    L.call("scail_vae_create", C.byref(w), C.byref(h))
    yield h
    L.load().scail_vae_destroy(h)


def test_stream_workspace_is_independent_of_the_clip_and_smaller_by_the_frame_ratio(handle):
    from scail_amd import lib as L
    lib = L.load()
    chunk, Tl = 4, 41
    T = 1 + 4 * (Tl - 1)
    stream = lib.scail_vae_decode_stream_workspace_bytes(handle, chunk, HL, WL)
    whole = lib.scail_vae_workspace_bytes(handle, T, 8 * HL, 8 * WL)
    assert stream > 0 and whole > 0
    # the query has no clip-length argument: one value serves every Tl (a 2-frame, a 41-frame and a 1001-frame latent alike)
    assert lib.scail_vae_decode_stream_workspace_bytes.argtypes == [C.c_void_p, C.c_int64, C.c_int64, C.c_int64]
    assert stream == lib.scail_vae_decode_stream_workspace_bytes(handle, chunk, HL, WL)
    # frames a slot holds: whole sequence, all T = 161 full-resolution frames; streamed, the largest chunk -- chunk + 1 latent frames (a
    # one-frame remainder joins the last chunk) = 4 (chunk + 1) frames -- behind the 2 carried frames of a causal convolution
    slot_frames_stream, slot_frames_whole = 4 * (chunk + 1) + 2, T
    assert (slot_frames_stream, slot_frames_whole) == (22, 161)
    print(f"stream {stream} B, whole {whole} B, ratio {stream / whole:.4f}, bound {slot_frames_stream / slot_frames_whole:.4f}")
    assert stream * slot_frames_whole <= whole * slot_frames_stream
    # and it grows with the chunk, not with anything else
    assert lib.scail_vae_decode_stream_workspace_bytes(handle, 8, HL, WL) > stream > lib.scail_vae_decode_stream_workspace_bytes(handle, 2, HL, WL)


def test_stream_refusals_without_gpu(handle):
    from scail_amd import lib as L
    lib = L.load()
    A = 0x10000       # a fake 256-byte aligned device address: the checks fail before it is ever dereferenced
    assert lib.scail_vae_decode_stream_workspace_bytes(handle, 1, HL, WL) == -1
    assert lib.scail_vae_decode_stream_workspace_bytes(None, 4, HL, WL) == -1
    need = lib.scail_vae_decode_stream_workspace_bytes(handle, 4, 6, 8)
    with pytest.raises(L.ScailHipError, match="chunk must be at least 2 latent frames.*got 1"):
        L.call("scail_vae_decode_stream", handle, A, A, 7, 6, 8, 1, A, need, None)
    with pytest.raises(L.ScailHipError, match="null argument"):
        L.call("scail_vae_decode_stream", handle, None, A, 7, 6, 8, 4, A, need, None)
    with pytest.raises(L.ScailHipError, match=f"workspace too small.*need {need} bytes, got {need - 1}"):
        L.call("scail_vae_decode_stream", handle, A, A, 7, 6, 8, 4, A, need - 1, None)
    with pytest.raises(L.ScailHipError, match="not 256-byte aligned"):
        L.call("scail_vae_decode_stream", handle, A, A, 7, 6, 8, 4, A + 16, need, None)
    with pytest.raises(L.ScailHipError, match="must lie inside a plane"):
        L.call("scail_to_channels_last_frames", A, A, None, None, 16, 16, 90, 60, 45, None)
    with pytest.raises(L.ScailHipError, match="row stride"):
        L.call("scail_from_channels_last_frames", A, 12, A, None, None, 3, 90, 0, 45, -1.0, 1.0, None)


def test_cli_and_layer_path_arguments():
    """--vae-chunk-frames is refused below 2 before any model is built; the layer-by-layer path has no streamed form"""
    import torch
    from scail_amd import cli
    from scail_amd.wan_vae import WanVAE_
    with pytest.raises(SystemExit):
        cli.main(["--tiny", "--vae-chunk-frames", "1"])
    m = WanVAE_(dim=32, z_dim=16, device="cpu")
    m._prepared, m.use_c_exec = {}, False
    with pytest.raises(NotImplementedError, match="chunk_frames"):
        m.decode(torch.zeros(1, 16, 7, 6, 8), chunk_frames=4)
