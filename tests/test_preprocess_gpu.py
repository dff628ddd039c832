"""The HIP route of request preprocessing on the GPU (include/scail_hip.h scail_resize_crop_aa / scail_pose_half, scail_amd/preprocess.py
``*_hip``, ``request_from_files(..., preprocess="hip")``) against the fp64 restatement of tests/test_preprocess_hip_cpu.py: the bound B,
the rounding cap and the shapes are stated there."""
import numpy as np
import pytest
import torch

from test_preprocess_hip_cpu import (F32_CASE, HALF_TOL, MAX_AMBIGUOUS, U8_CASES, check_rounded, f32_image, half_bounds, restate_request,
                                     rounded_bounds, textured_image_u8, u8_clip)

pytestmark = pytest.mark.gpu

SMALL = [c for c in U8_CASES if c[0] != "identity"]


def _mean4(p):
    """((a + b) + (c + d)) * 0.25 in fp32, the order include/scail_hip.h documents for scail_pose_half."""
    a, b, c, d = p[..., 0::2, 0::2], p[..., 0::2, 1::2], p[..., 1::2, 0::2], p[..., 1::2, 1::2]
    return ((a + b) + (c + d)) * 0.25


@pytest.fixture(scope="module")
def first_case():
    """5 frames of the first case, its restatement and the one-chunk result: shared, never modified."""
    from scail_amd import preprocess
    name, shape, size = U8_CASES[0]
    clip = u8_clip((5,) + shape[1:], 21)
    expected, B = restate_request(clip.permute(0, 3, 1, 2).numpy(), size)
    pose, smpl = preprocess.prepare_pose_video_hip(clip, size, chunk_frames=5, want_full=True)
    return clip, size, expected, B, pose.cpu(), smpl.cpu()


@pytest.mark.parametrize("name,shape,size", SMALL, ids=[c[0] for c in SMALL])
def test_ops_against_the_restatement_u8(name, shape, size):
    from scail_amd import ops, preprocess
    clip = u8_clip(shape, 11)
    expected, B = restate_request(clip.permute(0, 3, 1, 2).numpy(), size)
    (hr, wr), top, left = preprocess.crop_geometry(shape[1], shape[2], size)
    px = ops.resize_crop_aa(clip.cuda(), (hr, wr), top, left, size)
    assert px.dtype == torch.float32 and tuple(px.shape) == expected.shape
    check_rounded(px.cpu().numpy(), expected, B, name)
    half, full = ops.pose_half(px, want_full=True)
    x = px.cpu()
    assert torch.equal(full.cpu(), (x - 127.5) / 127.5)                     # the bits of the torch expression
    assert torch.equal(half.cpu(), _mean4(full.cpu()))
    lo, hi = half_bounds(expected, B)
    h = half.cpu().double().numpy()
    assert (h >= lo).all() and (h <= hi).all()


@pytest.mark.parametrize("name,shape,size", SMALL, ids=[c[0] for c in SMALL])
def test_prepare_pose_video_hip_against_the_restatement(name, shape, size):
    from scail_amd import preprocess
    clip = u8_clip(shape, 11)
    expected, B = restate_request(clip.permute(0, 3, 1, 2).numpy(), size)
    pose, smpl = preprocess.prepare_pose_video_hip(clip, size, want_full=True)
    T = shape[0]
    assert tuple(pose.shape) == (T, 3) + tuple(size) and tuple(smpl.shape) == (3, T, size[0] // 2, size[1] // 2) and smpl.is_contiguous()
    check_rounded(np.rint(pose.cpu().double().numpy() * 127.5 + 127.5), expected, B, name)
    lo, hi = half_bounds(expected, B)
    s = smpl.permute(1, 0, 2, 3).cpu().double().numpy()
    assert (s >= lo).all() and (s <= hi).all()
    assert preprocess.prepare_pose_video_hip(clip, size)[0] is None         # the full-size frames are optional


def test_identity_is_exact():
    from scail_amd import ops, preprocess
    name, shape, size = U8_CASES[4]
    clip = u8_clip(shape, 11)
    want = clip.permute(0, 3, 1, 2).float()
    assert torch.equal(ops.resize_crop_aa(clip.cuda(), size, 0, 0, size).cpu(), want)
    pose, smpl = preprocess.prepare_pose_video_hip(clip, size, want_full=True)
    assert torch.equal(pose.cpu(), (want - 127.5) / 127.5)
    assert torch.equal(smpl.cpu(), _mean4(pose.cpu()).permute(1, 0, 2, 3))
    img = f32_image((1, 3) + tuple(size), 5)
    assert torch.equal(preprocess.prepare_reference_image_hip(img, size).cpu(), img)


def test_f32_planar_source_is_not_rounded():
    from scail_amd import ops, preprocess
    name, shape, size = F32_CASE
    img = f32_image(shape, 12)
    expected, B = restate_request(img.numpy(), size)
    (hr, wr), top, left = preprocess.crop_geometry(shape[2], shape[3], size)
    a = ops.resize_crop_aa(img.cuda(), (hr, wr), top, left, size).cpu()
    err = float(np.abs(a.double().numpy() - expected).max())
    print(f"{name}: max error {err:.3e}, B = {B:.3e}")
    assert tuple(a.shape) == expected.shape and err <= B
    assert torch.equal(preprocess.prepare_reference_image_hip(img, size).cpu(), a)


def test_chunk_independence(first_case):
    from scail_amd import preprocess
    clip, size, expected, B, pose5, smpl5 = first_case
    check_rounded(np.rint(pose5.double().numpy() * 127.5 + 127.5), expected, B, "5 frames, one chunk")
    for chunk in (2, 16):                                                   # 5 is no multiple of 2: the last chunk is short
        pose, smpl = preprocess.prepare_pose_video_hip(clip, size, chunk_frames=chunk, want_full=True)
        assert torch.equal(pose.cpu(), pose5) and torch.equal(smpl.cpu(), smpl5), chunk
    with pytest.raises(ValueError, match="chunk_frames must be positive"):
        preprocess.prepare_pose_video_hip(clip, size, chunk_frames=0)


def test_half_resolution_into_a_strided_slot():
    """scail_pose_half on GIVEN integer pixels: within HALF_TOL of the fp64 mean, the documented fp32 order bit for bit, and written into
    frames 1..2 of a (C, 4, h/2, w/2) tensor with the neighbouring frames' slots untouched."""
    from scail_amd import ops
    x = torch.from_numpy(np.random.default_rng(31).integers(0, 256, (2, 3, 16, 24)).astype(np.float32))
    dense, full = ops.pose_half(x.cuda(), want_full=True)
    p64 = (x.double() - 127.5) / 127.5
    want = p64.reshape(2, 3, 8, 2, 12, 2).mean((3, 5))
    assert float((dense.cpu().double() - want).abs().max()) <= HALF_TOL
    assert torch.equal(full.cpu(), (x - 127.5) / 127.5) and torch.equal(dense.cpu(), _mean4(full.cpu()))
    big = torch.full((3, 4, 8, 12), 7.0, device="cuda")
    out, none = ops.pose_half(x.cuda(), out_half=big[:, 1:3].permute(1, 0, 2, 3))
    assert none is None and out.data_ptr() == big[:, 1:3].data_ptr()
    b = big.cpu()
    assert torch.equal(b[:, 1:3], dense.cpu().permute(1, 0, 2, 3)) and bool((b[:, 0] == 7.0).all()) and bool((b[:, 3] == 7.0).all())


def test_ops_refuse_what_the_library_refuses():
    from scail_amd import ops
    from scail_amd.lib import ScailHipError
    clip = u8_clip((1, 45, 80, 3), 0).cuda()
    with pytest.raises(ScailHipError, match="outside the resized image"):
        ops.resize_crop_aa(clip, (16, 28), 0, 5, (16, 24))
    with pytest.raises(ScailHipError, match="above the cap"):
        ops.resize_crop_aa(clip, (2, 28), 0, 0, (2, 24))
    with pytest.raises(ScailHipError, match="must be even"):
        ops.pose_half(torch.zeros(1, 3, 15, 24, device="cuda"))


def test_route_agreement_and_a_run_on_the_hip_request(tmp_path):
    """request_from_files with preprocess="hip" against "torch": same shapes and layout, the reference image within B, the pose equal
    wherever the rounding is decided and within one uint8 step (through / 127.5 and the 2 x 2 mean) where it is not; then a tiny run.
    The clip is white noise; the image is textured_image_u8, where today's torch route is itself within B (the reason is stated there)."""
    from PIL import Image
    from scail_amd import cli, video_io
    g = np.random.default_rng(0)
    Image.fromarray(textured_image_u8((90, 160), 0)).save(tmp_path / "ref.png")
    np.save(tmp_path / "rendered.npy", g.integers(0, 255, (5, 90, 160, 3), dtype=np.uint8))
    files = (str(tmp_path / "ref.png"), str(tmp_path / "rendered.npy"), cli.TINY)
    rt, size_t = cli.request_from_files(*files, text_dim=64, preprocess="torch")
    rh, size_h = cli.request_from_files(*files, text_dim=64, preprocess="hip")
    assert size_t == size_h == (64, 64)
    for k in rt:
        assert rh[k].shape == rt[k].shape and rh[k].stride() == rt[k].stride() and rh[k].dtype == rt[k].dtype and rh[k].device == rt[k].device, k
    assert rt["ref"].shape == (3, 1, 64, 64) and rt["pose"].shape == (3, 5, 32, 32)
    for k in ("context", "uncond_context", "clip"):
        assert torch.equal(rh[k], rt[k])
    # the reference image: an fp32 source, not rounded
    img = video_io.load_image_to_tensor_chw_normalized(files[0])
    expected, B = restate_request(img.numpy(), (64, 64))
    e = expected.transpose(1, 0, 2, 3)
    err_h = float(np.abs(rh["ref"].cpu().double().numpy() - e).max())
    err_t = float(np.abs(rt["ref"].cpu().double().numpy() - e).max())
    diff = float((rh["ref"] - rt["ref"]).abs().max())
    print(f"ref: hip {err_h:.3e}, torch {err_t:.3e} from the restatement, hip - torch {diff:.3e}, B = {B:.3e}")
    assert err_h <= B and err_t <= B and diff <= B
    # the pose: a uint8 source
    clip = video_io.load_video_for_pose_sample(files[1]).permute(0, 3, 1, 2)
    expected, B = restate_request(clip.numpy(), (64, 64))
    lo, hi, amb = rounded_bounds(expected, B)
    assert float(amb.mean()) <= MAX_AMBIGUOUS
    blo, bhi = half_bounds(expected, B)
    for r in (rh, rt):
        s = r["pose"].permute(1, 0, 2, 3).cpu().double().numpy()
        assert (s >= blo).all() and (s <= bhi).all()
    undecided = amb.reshape(5, 3, 32, 2, 32, 2).sum((3, 5)).transpose(1, 0, 2, 3)          # ambiguous pixels per 2 x 2 block
    d = (rh["pose"] - rt["pose"]).abs().cpu().double().numpy()
    print(f"pose: B = {B:.3e}, ambiguous {float(amb.mean()):.4%}, blocks that differ {int((d > 2 * HALF_TOL).sum())} of {d.size}")
    assert (d <= undecided / (4 * 127.5) + 2 * HALF_TOL).all()
    video, z, _ = cli.run(cli.TINY, rh, steps=2)
    assert video.shape == (1, 3, 5, 64, 64) and bool(torch.isfinite(video).all())
