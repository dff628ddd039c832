"""The pinned resize arithmetic of request preprocessing, and the host side of its HIP route (scail_amd/preprocess.py ``*_hip``,
include/scail_hip.h scail_resize_crop_aa / scail_pose_half) -- everything that needs no GPU.

The yardstick is the fp64 RESTATEMENT below, never the code under test: two 1-D weight matrices built from the formula the header
states (cubic a = -0.5, align_corners = False, support widened by the scale), ``expected = Wh . X . Ww^T``, then the crop.  It is tied
to today's torch route here and the kernels are held to it in tests/test_preprocess_gpu.py.

Tolerance (derived, not tuned): a float result may differ from ``expected`` by at most

    B = (taps_h + taps_w + 4) * 2^-23 * A * max_rows sum|w_h| * max_rows sum|w_w|,    A = the input's largest magnitude

(one rounding per tap of each fp32 pass plus the weights' own rounding, each relative to the largest partial sum).  A uint8 source is
rounded half-to-even: the result must equal ``rint(expected)`` except where ``expected`` lies within B of a half-integer, where either
neighbour is accepted; such pixels must be at most 2 % of the outputs (about 2 B of them are expected for random pixels)."""
import os

import numpy as np
import pytest
import torch

from scail_amd import preprocess
from scail_amd.lib import ScailHipError

# (name, source (T, H, W, 3) uint8, target): the smallest shapes that take every branch of the kernels
U8_CASES = [
    ("down_crop_w", (3, 45, 80, 3), (16, 24)),      # resized 16 x 28, left = 2, non-integer scale 2.81
    ("down_crop_h", (2, 50, 40, 3), (16, 24)),      # resized 30 x 24, top = 7
    ("upscale", (1, 9, 13, 3), (16, 24)),           # support clipped and renormalised at the borders
    ("large_scale", (1, 128, 224, 3), (16, 24)),    # scale 8, about 33 taps per axis
    ("identity", (2, 64, 112, 3), (64, 112)),
]
F32_CASE = ("f32_planar", (1, 3, 45, 80), (16, 24))
MAX_AMBIGUOUS = 0.02
# scail_pose_half against the fp64 mean of the four normalised pixels: each |p| <= 1 carries <= 2^-25 from its division, a + b and c + d
# (<= 2) round by <= 2^-24 each, their sum (<= 4) by <= 2^-23, the factor 0.25 is exact: 0.25 * 3 * 2^-23 < 2^-23
HALF_TOL = 2.0 ** -23


def cubic(x):
    """Keys' cubic, a = -0.5."""
    x = abs(x)
    if x < 1.0:
        return 1.5 * x ** 3 - 2.5 * x ** 2 + 1.0
    if x < 2.0:
        return -0.5 * x ** 3 + 2.5 * x ** 2 - 4.0 * x + 2.0
    return 0.0


def weight_matrix(n_in, n_out):
    """(W (n_out, n_in) fp64, taps per output): row i holds k((j - c + 0.5) / max(s, 1)) over the taps
    [max(0, floor(c - sup + 0.5)), min(n_in, floor(c + sup + 0.5))), s = n_in / n_out, sup = 2 max(s, 1), c = s (i + 0.5), normalised."""
    s = n_in / n_out
    sc = max(s, 1.0)
    sup = 2.0 * sc
    W = np.zeros((n_out, n_in), np.float64)
    taps = np.zeros(n_out, np.int64)
    for i in range(n_out):
        c = s * (i + 0.5)
        lo, hi = max(0, int(np.floor(c - sup + 0.5))), min(n_in, int(np.floor(c + sup + 0.5)))
        w = np.array([cubic((j - c + 0.5) / sc) for j in range(lo, hi)], np.float64)
        W[i, lo:hi] = w / w.sum()
        taps[i] = hi - lo
    return W, taps


def restate(x, resized_hw, top, left, out_hw):
    """x (..., H, W) -> (expected (..., Ho, Wo) fp64, B)."""
    x = np.asarray(x, np.float64)
    Wh, th = weight_matrix(x.shape[-2], resized_hw[0])
    Ww, tw = weight_matrix(x.shape[-1], resized_hw[1])
    Wh, th = Wh[top:top + out_hw[0]], th[top:top + out_hw[0]]
    Ww, tw = Ww[left:left + out_hw[1]], tw[left:left + out_hw[1]]
    expected = Wh @ x @ Ww.T
    B = (th.max() + tw.max() + 4) * 2.0 ** -23 * np.abs(x).max() * np.abs(Wh).sum(1).max() * np.abs(Ww).sum(1).max()
    return expected, float(B)


def restate_request(x, size_hw):
    """The restatement with the geometry of resize_for_rectangle_crop, written out: scale so the frame covers the target, centre crop."""
    H, W = x.shape[-2], x.shape[-1]
    th, tw = size_hw
    hr, wr = (th, int(W * th / H)) if W / H > tw / th else (int(H * tw / W), tw)
    return restate(x, (hr, wr), (hr - th) // 2, (wr - tw) // 2, (th, tw))


def rounded_bounds(expected, B):
    """(lo, hi, ambiguous): the accepted uint8 values of every pixel -- rint(expected) clamped, or both neighbours where expected is
    within B of a half-integer."""
    r = np.clip(np.rint(expected), 0, 255)
    amb = np.abs(expected - (np.floor(expected) + 0.5)) <= B
    lo = np.where(amb, np.clip(np.floor(expected), 0, 255), r)
    hi = np.where(amb, np.clip(np.ceil(expected), 0, 255), r)
    return lo, hi, amb


def check_rounded(got, expected, B, what=""):
    got = np.asarray(got, np.float64)
    lo, hi, amb = rounded_bounds(expected, B)
    share = float(amb.mean())
    print(f"{what}: B = {B:.3e}, ambiguous {share:.4%}, off {int(((got != lo) & (got != hi)).sum())} of {got.size}")
    assert share <= MAX_AMBIGUOUS, (what, share)
    assert ((got == lo) | (got == hi)).all(), (what, int(((got != lo) & (got != hi)).sum()))
    return amb


def half_bounds(expected, B):
    """Bounds of the half-resolution render: the 2 x 2 mean of (v - 127.5) / 127.5 over the lowest / highest accepted pixels, +- HALF_TOL."""
    lo, hi, _ = rounded_bounds(expected, B)
    m = lambda v: ((v - 127.5) / 127.5).reshape(*v.shape[:-2], v.shape[-2] // 2, 2, v.shape[-1] // 2, 2).mean((-3, -1))
    return m(lo) - HALF_TOL, m(hi) + HALF_TOL


def u8_clip(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8))


def f32_image(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32))


def textured_image_u8(hw, seed, texture=16):
    """(H, W, 3) uint8 over the full range 0..255: a smooth colour field plus white texture of +-``texture`` levels -- the reference
    image of the route-agreement test (tests/test_preprocess_gpu.py).  Why not white noise at full amplitude, as the clip is: B bounds
    the ROUNDING of exact weights, relative to the largest magnitude A.  ATen evaluates the tap positions ``j - s (i + 0.5) + 0.5`` in
    fp32, so a weight carries an absolute error of about ulp(coordinate) = 2^-23 * 160 here, which B does not cover; the weights still
    sum to one, so that error multiplies the CONTRAST inside the support, not A.  A loaded image in [-1, 1] made of full-amplitude
    noise has contrast 2 A inside every support (a uint8 clip, A = 255, has only A), and today's torch route is then 4.1e-6 .. 4.8e-6
    from the restatement against B = 2.7e-6 at 90 x 160 -> 64 x 113, on the CPU, for every seed tried; no image that a request
    carries looks like that.  With +-16 levels of texture on a smooth field the torch route is within 1e-6 (test below)."""
    h, w = hw
    y, x = np.mgrid[0:h, 0:w]
    g = np.random.default_rng(seed)
    field = np.stack([127.5 + (127.5 - texture) * np.sin(2 * np.pi * (c + 1) * x / w + np.pi * y / h) for c in range(3)], -1)
    return np.clip(np.rint(field + g.integers(-texture, texture + 1, field.shape)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_matches_the_torch_route_on_the_request_image(seed):
    """The 90 x 160 reference image of the route-agreement test, normalised as the image loader does: today's torch route is within B."""
    u = textured_image_u8((90, 160), seed)
    assert u.min() == 0 and u.max() == 255
    img = (torch.from_numpy(u).permute(2, 0, 1)[None].float() - 127.5) / 127.5
    expected, B = restate_request(img.numpy(), (64, 64))
    err = float(np.abs(preprocess.prepare_reference_image(img, (64, 64)).double().numpy() - expected).max())
    print(f"request image, seed {seed}: max error {err:.3e}, B = {B:.3e}")
    assert err <= B


@pytest.mark.parametrize("name,shape,size", U8_CASES, ids=[c[0] for c in U8_CASES])
def test_restatement_matches_the_torch_route_u8(name, shape, size):
    clip = u8_clip(shape, 11)                                               # (T, H, W, C)
    tchw = clip.permute(0, 3, 1, 2)
    expected, B = restate_request(tchw.numpy(), size)
    got = preprocess.resize_for_rectangle_crop(tchw, size)
    assert got.dtype == torch.uint8 and tuple(got.shape) == expected.shape
    check_rounded(got.numpy(), expected, B, name)
    pose, smpl = preprocess.prepare_pose_video(tchw, size)
    assert np.array_equal(np.rint(pose.double().numpy() * 127.5 + 127.5), got.numpy().astype(np.float64))
    lo, hi = half_bounds(expected, B)
    s = smpl.double().numpy()
    assert (s >= lo).all() and (s <= hi).all()
    (hr, wr), top, left = preprocess.crop_geometry(shape[1], shape[2], size)
    assert 0 <= top and top + size[0] <= hr and 0 <= left and left + size[1] <= wr and (hr == size[0] or wr == size[1])


def test_restatement_matches_the_torch_route_f32():
    name, shape, size = F32_CASE
    img = f32_image(shape, 12)
    expected, B = restate_request(img.numpy(), size)
    got = preprocess.prepare_reference_image(img, size).double().numpy()
    err = float(np.abs(got - expected).max())
    print(f"{name}: max error {err:.3e}, B = {B:.3e}")
    assert got.shape == expected.shape and err <= B


def test_exact_2x_weights_are_the_closed_form():
    """(8, 12) -> (4, 6): scale 2, taps at -1.75 .. 1.75 in steps of 0.5.  k(0.25) = 111/128, k(0.75) = 29/128, k(1.25) = -9/128,
    k(1.75) = -3/128; the eight sum to 2, so an interior row is exactly these over 2."""
    k = np.array([-3.0, -9.0, 29.0, 111.0, 111.0, 29.0, -9.0, -3.0]) / 128.0
    assert [cubic(v) for v in (1.75, 1.25, 0.75, 0.25)] == [-3 / 128, -9 / 128, 29 / 128, 111 / 128] and k.sum() == 2.0
    Ww, tw = weight_matrix(12, 6)
    for i in (2, 3):                                                        # interior: taps 2i - 3 .. 2i + 4 all inside [0, 12)
        assert tw[i] == 8 and np.array_equal(Ww[i, 2 * i - 3:2 * i + 5], k / 2.0) and np.count_nonzero(Ww[i]) == 8
    Wh, th = weight_matrix(8, 4)                                            # no row of 8 -> 4 is interior: clipped and renormalised
    for i in range(4):
        lo, hi = max(0, 2 * i - 3), min(8, 2 * i + 5)
        part = k[lo - (2 * i - 3):hi - (2 * i - 3)]
        assert th[i] == hi - lo and np.allclose(Wh[i, lo:hi], part / part.sum(), rtol=0, atol=1e-16)
    assert np.allclose(Wh.sum(1), 1.0, atol=1e-15) and np.allclose(Ww.sum(1), 1.0, atol=1e-15)
    x = u8_clip((1, 3, 8, 12), 3)
    expected, B = restate(x.numpy(), (4, 6), 0, 0, (4, 6))
    check_rounded(preprocess._resize_bicubic_u8(x, (4, 6)).numpy(), expected, B, "exact 2x")


def test_identity_returns_the_input():
    Wh, th = weight_matrix(64, 64)
    assert np.array_equal(Wh, np.eye(64)) and th.max() <= 4
    x = u8_clip((2, 64, 112, 3), 4).permute(0, 3, 1, 2)
    expected, _ = restate_request(x.numpy(), (64, 112))
    assert np.array_equal(expected, x.numpy().astype(np.float64))
    assert torch.equal(preprocess.resize_for_rectangle_crop(x, (64, 112)), x)


@pytest.fixture(scope="module")
def L():
    from scail_amd import build, lib
    build.build(verbose=False)
    lib.load()
    return lib


def test_host_side_validation_without_a_gpu(L):
    """Every refusal of the two entry points is decided on the host before a launch, so it is testable here; on the parent commit the
    symbols do not exist."""
    A = 0x1000       # a fake, aligned device address: validation fails (or n = 0 returns) before it is dereferenced
    cases = [
        ("vertical scale 1700 / 100 is above the cap of 16", "scail_resize_crop_aa", (A, 0, A, 1, 3, 1700, 64, 100, 64, 0, 0, 100, 64, None)),
        ("horizontal scale 3300 / 200 is above the cap", "scail_resize_crop_aa", (A, 0, A, 1, 3, 64, 3300, 64, 200, 0, 0, 64, 200, None)),
        (r"window \[5, 5 \+ 60\) x \[0, 0 \+ 24\) is outside the resized image 64 x 28", "scail_resize_crop_aa",
         (A, 0, A, 1, 3, 180, 80, 64, 28, 5, 0, 60, 24, None)),
        ("outside the resized image", "scail_resize_crop_aa", (A, 0, A, 1, 3, 180, 80, 64, 28, 0, -1, 60, 24, None)),
        ("C must be 1..4, got 5", "scail_resize_crop_aa", (A, 0, A, 1, 5, 45, 80, 16, 28, 0, 2, 16, 24, None)),
        ("unknown source kind 7", "scail_resize_crop_aa", (A, 7, A, 1, 3, 45, 80, 16, 28, 0, 2, 16, 24, None)),
        ("null pointer", "scail_resize_crop_aa", (None, 0, A, 1, 3, 45, 80, 16, 28, 0, 2, 16, 24, None)),
        ("null pointer", "scail_resize_crop_aa", (A, 0, None, 1, 3, 45, 80, 16, 28, 0, 2, 16, 24, None)),
        ("H and W must be even .*got 15 x 16", "scail_pose_half", (A, A, 64, 64, None, 1, 3, 15, 16, None)),
        ("H and W must be even .*got 16 x 23", "scail_pose_half", (A, A, 88, 88, None, 1, 3, 16, 23, None)),
        ("null pointer", "scail_pose_half", (None, A, 64, 64, None, 1, 3, 16, 16, None)),
        ("null pointer", "scail_pose_half", (A, None, 64, 64, None, 1, 3, 16, 16, None)),
        ("strides must hold a plane of 64 pixels", "scail_pose_half", (A, A, 63, 64, None, 1, 3, 16, 16, None)),
        ("8-byte aligned", "scail_pose_half", (A + 4, A, 64, 64, None, 1, 3, 16, 16, None)),
    ]
    for needle, fn, args in cases:
        with pytest.raises(L.ScailHipError, match=needle):
            L.call(fn, *args)
    # n = 0 is accepted and launches nothing (no device needed); 2160 -> 256 is inside the cap
    L.call("scail_resize_crop_aa", A, 0, A, 0, 3, 45, 80, 16, 28, 0, 2, 16, 24, None)
    L.call("scail_resize_crop_aa", A, 1, A, 0, 3, 2160, 3840, 256, 455, 0, 3, 256, 448, None)
    L.call("scail_pose_half", A, A, 64, 64, None, 0, 3, 16, 16, None)
    assert L.RESIZE_MAX_SCALE == 16 and 2160 / 256 <= L.RESIZE_MAX_SCALE
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "scail_hip.h")).read()
    assert "#define SCAIL_RESIZE_MAX_SCALE 16" in hdr and "#define SCAIL_SRC_U8_NHWC 0" in hdr and "#define SCAIL_SRC_F32_NCHW 1" in hdr


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_hip_route_has_no_cpu_fallback():
    from scail_amd import ops
    with pytest.raises(ScailHipError, match="GPU"):
        preprocess.prepare_pose_video_hip(u8_clip((2, 45, 80, 3), 0), (16, 24))
    with pytest.raises(ScailHipError, match="GPU"):
        preprocess.prepare_reference_image_hip(f32_image((1, 3, 45, 80), 0), (16, 24))
    with pytest.raises(ScailHipError, match="GPU"):
        ops.resize_crop_aa(u8_clip((2, 45, 80, 3), 0), (16, 28), 0, 2, (16, 24))
    with pytest.raises(ScailHipError, match="GPU"):
        ops.pose_half(torch.zeros(1, 3, 16, 24))


def test_hip_route_refuses_a_cpu_device_and_other_reshape_modes():
    with pytest.raises(ScailHipError, match="needs a GPU"):
        preprocess.prepare_pose_video_hip(u8_clip((2, 45, 80, 3), 0), (16, 24), device="cpu")
    with pytest.raises(ScailHipError, match="needs a GPU"):
        preprocess.prepare_reference_image_hip(f32_image((1, 3, 45, 80), 0), (16, 24), device="cpu")
    with pytest.raises(NotImplementedError, match="center"):
        preprocess.crop_geometry(45, 80, (16, 24), "random")


def test_cli_preprocess_option(tmp_path, capsys):
    from PIL import Image
    from scail_amd import cli
    ap = cli.build_parser()
    assert ap.parse_args(["--tiny"]).preprocess == "torch" and ap.parse_args(["--tiny", "--preprocess", "hip"]).preprocess == "hip"
    with pytest.raises(SystemExit):                                         # an argparse error, before any model is built
        cli.main(["--tiny", "--preprocess", "nope"])
    assert "invalid choice: 'nope'" in capsys.readouterr().err
    g = np.random.default_rng(0)
    Image.fromarray(g.integers(0, 255, (90, 160, 3), dtype=np.uint8)).save(tmp_path / "ref.png")
    np.save(tmp_path / "rendered.npy", g.integers(0, 255, (5, 90, 160, 3), dtype=np.uint8))
    files = (str(tmp_path / "ref.png"), str(tmp_path / "rendered.npy"), cli.TINY)
    with pytest.raises(ScailHipError, match="needs a GPU"):
        cli.request_from_files(*files, device="cpu", text_dim=64, preprocess="hip")
    with pytest.raises(ValueError, match="preprocess must be one of"):
        cli.request_from_files(*files, device="cpu", text_dim=64, preprocess="nope")
    req = cli.request_from_files(*files, device="cpu", text_dim=64)[0]       # the default route is unchanged
    assert req["ref"].shape == (3, 1, 64, 64) and req["pose"].shape == (3, 5, 32, 32)
