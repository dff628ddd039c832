"""Request preprocessing of the reference CLI (sample_video.py:325-351, data_video.py:141-170), as tensor ops.

    resize_for_rectangle_crop   data_video.py:141-170: scale so the frame covers the target, centre crop
    prepare_pose_video          sample_video.py:340-351: crop, (x - 127.5) / 127.5, optional 0.5x bilinear
    prepare_reference_image     sample_video.py:343 (+ the [-1, 1] normalisation of the image loader)
    target_size                 sample_video.py:325-328: sampling_image_size is (H, W) for landscape, swapped for portrait

    prepare_pose_video_hip      the same on the library's kernels (scail_resize_crop_aa + scail_pose_half), a chunk of frames at a time
    prepare_reference_image_hip the same for the reference image (fp32 source, not rounded)

The reference resizes with torchvision ``resize(..., BICUBIC)`` on uint8 tensors; torchvision is not available
offline, so the resize is restated with ``torch.nn.functional.interpolate(mode="bicubic", antialias=True)`` followed
by the uint8 round + clamp torchvision applies (its tensor path calls exactly that op).  No reference OUTPUT could be generated
here, but the resize arithmetic is pinned: the antialiased cubic (a = -0.5, align_corners = False) is written out as two fp64 weight
matrices in tests/test_preprocess_hip_cpu.py -- taps and weights as include/scail_hip.h scail_resize_crop_aa states them, a
hand-checkable exact-2x case -- and both routes, this module's torch functions and the ``*_hip`` ones, are held to it within a derived
fp32 bound; the geometry (sizes, crop offsets, value ranges) is tested as before.
The ``*_hip`` route is opt-in (``request_from_files(..., preprocess="hip")``, ``--preprocess hip``): the clip crosses to the device as
uint8, ``chunk_frames`` frames at a time, so neither host nor device ever holds it as fp32 (the torch route's ``arr.float()`` of a
401-frame 1080p clip is 10 GB of host memory); there is no fallback -- without a GPU it raises ``ScailHipError``.
Video decoding (decord) and mp4 writing (imageio) need packages that are absent offline; ``scail_amd/video_io.py`` fills
those roles with Pillow containers (frame directories, arrays, animated WebP / PNG / GIF)."""
from __future__ import annotations

from typing import Sequence, Tuple

import torch
import torch.nn.functional as F

from .lib import ScailHipError


def target_size(image_hw: Tuple[int, int], sampling_image_size: Sequence[int]) -> Tuple[int, int]:
    """(target_H, target_W): sample_video.py:325-328."""
    h, w = image_hw
    a, b = sampling_image_size
    return (a, b) if h < w else (b, a)


def _resize_bicubic_u8(arr: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    dt = arr.dtype
    out = F.interpolate(arr.float(), size=size, mode="bicubic", align_corners=False, antialias=True)
    if dt == torch.uint8:
        out = out.round().clamp_(0, 255).to(torch.uint8)
    return out


def resize_for_rectangle_crop(arr: torch.Tensor, image_size: Sequence[int], reshape_mode: str = "center") -> torch.Tensor:
    """arr (T, C, H, W).  data_video.py:141-170; only the deterministic 'center' mode the CLI uses."""
    H, W = arr.shape[2], arr.shape[3]
    th, tw = int(image_size[0]), int(image_size[1])
    if W / H > tw / th:
        arr = _resize_bicubic_u8(arr, (th, int(W * th / H)))
    else:
        arr = _resize_bicubic_u8(arr, (int(H * tw / W), tw))
    h, w = arr.shape[2], arr.shape[3]
    if reshape_mode != "center":
        raise NotImplementedError("only reshape_mode='center' (the sampling CLI); 'random' is a training augmentation")
    top, left = (h - th) // 2, (w - tw) // 2
    return arr[:, :, top:top + th, left:left + tw]


def prepare_pose_video(pose_u8: torch.Tensor, size_hw: Sequence[int], downsample: bool = True):
    """pose_u8 (T, C, H, W) 0..255 -> (pose [-1,1] at full size, smpl render at half size if ``downsample``),
    sample_video.py:340-351."""
    pose = resize_for_rectangle_crop(pose_u8, size_hw, "center").float()
    pose = (pose - 127.5) / 127.5
    smpl = F.interpolate(pose, scale_factor=0.5, mode="bilinear", align_corners=False) if downsample else pose
    return pose, smpl


def prepare_reference_image(img: torch.Tensor, size_hw: Sequence[int]) -> torch.Tensor:
    """img (1, C, H, W) already in [-1, 1] (the reference's loader normalises) -> centre-cropped to size."""
    return resize_for_rectangle_crop(img, size_hw, "center")


# ---- the same on the library's kernels (include/scail_hip.h scail_resize_crop_aa / scail_pose_half) ----
def crop_geometry(H: int, W: int, image_size: Sequence[int], reshape_mode: str = "center"):
    """((Hr, Wr) resized size, top, left) of ``resize_for_rectangle_crop`` for an H x W source -- its sizes and offsets, stated once more
    for the route that computes only the crop window."""
    th, tw = int(image_size[0]), int(image_size[1])
    if reshape_mode != "center":
        raise NotImplementedError("only reshape_mode='center' (the sampling CLI); 'random' is a training augmentation")
    h, w = (th, int(W * th / H)) if W / H > tw / th else (int(H * tw / W), tw)
    return (h, w), (h - th) // 2, (w - tw) // 2


def _hip_device(device, who: str) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise ScailHipError(f"{who}: needs a GPU (device = {device!r}, torch.cuda.is_available() = {torch.cuda.is_available()}); "
                            "scail_amd has no CPU path -- the torch route is prepare_pose_video / prepare_reference_image")
    return dev


def prepare_pose_video_hip(pose_u8_thwc: torch.Tensor, size_hw: Sequence[int], chunk_frames: int = 16, device="cuda", want_full: bool = False):
    """pose_u8_thwc (T, H, W, C) uint8 on the HOST, as ``video_io.load_video_for_pose_sample`` returns it -> (pose, smpl) on ``device``:
    ``smpl`` (C, T, h/2, w/2) fp32, the half-resolution render in the request's layout; ``pose`` (T, C, h, w) in [-1, 1] when
    ``want_full``, else None.  ``chunk_frames`` frames at a time cross to the device as uint8 and go through scail_resize_crop_aa
    (resize + crop, uint8 rounding) and scail_pose_half (normalise + 2 x 2 mean, written into the chunk's slot of ``smpl``); every frame
    is computed on its own, so the result does not depend on ``chunk_frames``."""
    from . import ops
    dev = _hip_device(device, "prepare_pose_video_hip")
    if pose_u8_thwc.dtype != torch.uint8 or pose_u8_thwc.dim() != 4:
        raise ScailHipError(f"prepare_pose_video_hip: expected a uint8 (T, H, W, C) clip, got {pose_u8_thwc.dtype} {tuple(pose_u8_thwc.shape)}")
    if chunk_frames < 1:
        raise ValueError(f"prepare_pose_video_hip: chunk_frames must be positive, got {chunk_frames}")
    T, H, W, C = pose_u8_thwc.shape
    th, tw = int(size_hw[0]), int(size_hw[1])
    (hr, wr), top, left = crop_geometry(H, W, (th, tw))
    smpl = torch.empty((C, T, th // 2, tw // 2), device=dev, dtype=torch.float32)
    pose = torch.empty((T, C, th, tw), device=dev, dtype=torch.float32) if want_full else None
    n = max(1, min(chunk_frames, T))
    with torch.cuda.device(dev):
        u8 = torch.empty((n, H, W, C), device=dev, dtype=torch.uint8)
        px = torch.empty((n, C, th, tw), device=dev, dtype=torch.float32)
        for t0 in range(0, T, n):
            m = min(n, T - t0)
            u8[:m].copy_(pose_u8_thwc[t0:t0 + m])
            ops.resize_crop_aa(u8[:m], (hr, wr), top, left, (th, tw), out=px[:m])
            ops.pose_half(px[:m], out_half=smpl[:, t0:t0 + m].permute(1, 0, 2, 3), out_full=pose[t0:t0 + m] if want_full else None)
    return pose, smpl


def prepare_reference_image_hip(img: torch.Tensor, size_hw: Sequence[int], device="cuda") -> torch.Tensor:
    """img (1, C, H, W) fp32 already in [-1, 1] (host or device) -> centre-cropped to size, (1, C, h, w) on ``device``; not rounded."""
    from . import ops
    dev = _hip_device(device, "prepare_reference_image_hip")
    th, tw = int(size_hw[0]), int(size_hw[1])
    (hr, wr), top, left = crop_geometry(img.shape[2], img.shape[3], (th, tw))
    with torch.cuda.device(dev):
        return ops.resize_crop_aa(img.to(dev, torch.float32).contiguous(), (hr, wr), top, left, (th, tw))
