"""Driver mirroring the hot-path part of the reference CLI (sample_video.py:219-507):

    python -m scail_amd.cli --base <model.yaml> [<sampling.yaml>] [--load DIR] [--steps N] [--out out.pt]
    python -m scail_amd.cli --tiny          # BASELINE.json configs[0] shape: 2-layer / 128-dim DiT, 4x8x8 latent, 2 steps
    python -m scail_amd.cli --base ... --request "the girl is dancing@@examples/001" [--input-file requests.txt]

Order of work per request (same as the reference): VAE-encode the reference frame and the half-resolution
pose video (:355-391), build c / uc (:433-470), ``engine.sample`` (:476-483), VAE-decode (:491-494).
The reference's first VAE encode of [ref + zeros] (:362-365) is skipped: ``concat_images`` only gates a
branch and is never read by the network -- a zero-size placeholder is passed.

Requests: ``--ref-image ref.jpg --pose-video <frames dir | .npy | animated .webp/.png/.gif | Motion-JPEG .mp4> [--conditioning c.pt]`` runs
the reference's preprocessing (centre crop, [-1, 1], half-resolution pose; scail_amd/preprocess.py; ``--preprocess hip`` = on the GPU
with the library's kernels, chunked; ``--postprocess hip`` = the VAE decoder's last kernel writes the uint8 frames the file writers take, so no
fp32 video exists on either side) on files, or
``--inputs file.pt`` passes tensors directly: ref (3,1,H,W) in [-1,1], pose (3,T,H,W), context (1,Lt,4096),
uncond_context (1,Lt,4096), clip (1,257,1280); without either synthetic inputs are drawn.  ``--save-dir`` writes
``0_output_000000.webp`` (lossless animated WebP; ``--format`` for APNG / GIF / .npy / frames, or ``.mp4`` = the reference's
file name with Motion-JPEG samples, container written by scail_amd/video_io.py) where the reference writes H.264 mp4.  ``--prompt TEXT --tokenizer <HF dir | spiece.model> [--t5-ckpt ..] [--clip-ckpt ..]`` runs the UMT5 and CLIP encoders
(scail_amd/umt5.py, clip.py) on the prompt and the reference image.  Offline limits of this image: no H.264 / HEVC codec (decord,
imageio, ffmpeg, cv2 are absent: an .mp4 with such a track is rejected by the name of its codec), no tokenizer files and no checkpoints -- hence the container formats above, the tokenizer as a path
argument, and random-init weights unless checkpoints are given.

Clips longer than one window (an EXTENSION: the reference CLI has no such route, it only ships the sampler): a pose clip with more latent
frames than ``--tile-frames`` covers is sampled with ``RFSamplerLong`` (temporal tiling, sampling.py:986-1085) over the windows of
``plan_tiles`` -- each window's pose frames VAE-encoded on their own, noise and decode for the whole latent.  A clip that fits one window
takes the plain path above, unchanged."""
from __future__ import annotations

import argparse
import copy
import math
import os
import time

# the host driver supports only dmabuf IPC: RCCL between the ranks of one node fails without this (set before HIP starts)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402

from . import lib
from .config import load_yaml_configs
from .engine import SATVideoDiffusionEngine

TINY = {
    "model": {
        "use_i2v_clip": True, "scale_factor": 1.0, "build_first_stage": True,
        "network_config": {"target": "dit_video_crossattn_sc_xc.DiffusionTransformer", "params": dict(
            time_freq_dim=256, time_embed_dim=128, share_adaln=True, elementwise_affine=False, num_frames=13,
            time_compressed_rate=4, latent_width=32, latent_height=32, num_layers=2, patch_size=[1, 2, 2], in_channels=20,
            out_channels=16, text_dim=64, hidden_size=128, inner_hidden_size=256, num_attention_heads=1,
            transformer_args=dict(model_parallel_size=1, is_decoder=True),
            modules={"pos_embed_config": {"params": {"hidden_size_head": 128, "interleaved_rope": True}},
                     "adaln_layer_config": {"params": {"qk_ln": True, "hidden_size_head": 128}}})},
        "first_stage_config": {"target": "sgm.models.wan_vae.WanVAE", "params": {"vae_pth": None, "dtype": "torch.bfloat16", "dim": 32}},
        "sampler_config": {"target": "sgm.modules.diffusionmodules.sampling.RFSampler", "params": dict(
            hunyuan_schedule=True, shift_scale=5, num_steps=2,
            guider_config={"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": 4}})},
    },
    "args": {"sampling_image_size": [64, 64], "sampling_fps": 16},
}


def synthetic_request(H, W, frames, text_dim, Lt, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    ctx = r(1, Lt, text_dim)
    ctx[:, Lt // 8:] = 0
    uc = torch.zeros(1, Lt, text_dim)
    uc[:, :1] = r(1, 1, text_dim)
    return dict(ref=(torch.rand(3, 1, H, W, generator=g) * 2 - 1).to(device), pose=(torch.rand(3, frames, H // 2, W // 2, generator=g) * 2 - 1).to(device),
                context=ctx.to(device), uncond_context=uc.to(device), clip=r(1, 257, 1280).to(device))


def plan_tiles(T: int, Tt: int, overlap: int):
    """Temporal windows of a T-frame latent for RFSamplerLong: contiguous tiles of Tt latent frames whose neighbours share ``overlap``
    frames (1 <= overlap < Tt).  None when one window holds the clip (T <= Tt: the plain path).  Otherwise the tiles start at 0, s, 2s, ..
    (s = Tt - overlap) while start + Tt < T, and a final tile ends at T: at least two tiles, every frame covered."""
    if T < 1 or Tt < 1:
        raise ValueError(f"plan_tiles: T and Tt must be positive, got T = {T}, Tt = {Tt}")
    if T <= Tt:
        return None
    if not 1 <= overlap < Tt:
        raise ValueError(f"plan_tiles: the overlap must be 1..Tt - 1 = {Tt - 1} latent frames, got {overlap}")
    starts, s = [], 0
    while s + Tt < T:
        starts.append(s)
        s += Tt - overlap
    starts.append(T - Tt)
    return [list(range(a, a + Tt)) for a in starts]


def tile_args(tile_frames, tile_overlap, num_frames):
    """``--tile-frames`` / ``--tile-overlap`` (pixel frames) -> (Tt, overlap) in latent frames.  Defaults: the network's window
    (``num_frames``) and half of its latent frames."""
    tf = num_frames if tile_frames is None else tile_frames
    if tf < 5 or (tf - 1) % 4:
        raise ValueError(f"--tile-frames must be 4n + 1 pixel frames with n >= 1 (the causal VAE's frame groups), got {tf}")
    Tt = (tf - 1) // 4 + 1
    if tile_overlap is None:
        return Tt, max(1, Tt // 2)
    if tile_overlap % 4 or tile_overlap < 4:
        raise ValueError(f"--tile-overlap must be a positive multiple of 4 pixel frames (whole latent frames), got {tile_overlap}")
    if tile_overlap // 4 >= Tt:
        raise ValueError(f"--tile-overlap = {tile_overlap} pixel frames ({tile_overlap // 4} latent frames) must be smaller than the window of "
                         f"{tf} pixel frames ({Tt} latent frames)")
    return Tt, tile_overlap // 4


REF_IMAGE_PATTERNS = ["ref.jpg", "ref.png", "ref_image.jpg", "ref_image.png"]                # sample_video.py:289
# the reference looks for rendered_aligned.mp4 / rendered.mp4 (:296); the containers this image can decode come first
POSE_PATTERNS = [stem + ext for stem in ("rendered_aligned", "rendered") for ext in ("", ".webp", ".png", ".gif", ".npy", ".pt", ".mp4")]      # (.mp4 last: the reference's own examples are H.264, which nothing here decodes)


def find_file_with_patterns(directory: str, patterns):
    """sample_video.py:64-70."""
    import os
    for pat in patterns:
        p = os.path.join(directory, pat)
        if os.path.exists(p):
            return p
    return None


def parse_request(line: str):
    """One request line of the reference CLI, ``<prompt>@@<example_dir>`` (sample_video.py:76, :284-300): the directory holds
    the reference image and the rendered pose video.  -> (prompt, example_dir, image_path, pose_path)."""
    parts = line.strip().split("@@")
    if len(parts) != 2:
        raise ValueError(f"expected '<prompt>@@<example_dir>', got {line!r}")
    text, input_dir = parts[0], parts[1]
    if text == "None":
        text = ""
    image_path = find_file_with_patterns(input_dir, REF_IMAGE_PATTERNS)
    if image_path is None:
        raise FileNotFoundError(f"Reference image not found in {input_dir}. Tried: {REF_IMAGE_PATTERNS}")
    pose_path = find_file_with_patterns(input_dir, POSE_PATTERNS)
    if pose_path is None:
        raise FileNotFoundError(f"Pose video not found in {input_dir}. Tried: {POSE_PATTERNS}")
    return text, input_dir, image_path, pose_path


def read_from_file(path: str, rank: int = 0, world_size: int = 1):
    """sample_video.py:82-91: request lines of a text file, dealt round-robin to the data-parallel ranks."""
    with open(path) as f:
        for cnt, line in enumerate(f):
            if cnt % world_size == rank and line.strip():
                yield line.strip(), cnt


def encode_conditioning(prompt: str, negative_prompt: str, ref: torch.Tensor, text_dim: int, tokenizer_path: str,
                        t5_ckpt: str = None, clip_ckpt: str = None, device="cuda", max_length: int = 512):
    """Prompt + reference image -> the conditioning tensors of the request (sample_video.py:397-400, :416-438): UMT5
    states of the prompt and of the negative prompt (padded rows zeroed), CLIP ViT-H penultimate features of the reference
    frame.  Both encoders run once and are released (the reference moves them back to the CPU).  Checkpoints are optional
    (random init without them -- there are none offline); a text width other than 4096 builds a 2-layer encoder of that
    width, for plumbing tests against small networks."""
    from .clip import CLIPModel
    from .tokenizer import HuggingfaceTokenizer
    from .umt5 import T5EncoderModel
    kw = {}
    if text_dim != 4096:
        if text_dim % 128:
            raise ValueError("the plumbing-size text encoder needs a text width that is a multiple of 128")
        vocab = HuggingfaceTokenizer(tokenizer_path).vocab_size
        kw = dict(vocab=(vocab + 63) // 64 * 64, dim=text_dim, dim_attn=text_dim, dim_ffn=2 * text_dim,
                  num_heads=max(1, text_dim // 64), num_layers=2)
    t5 = T5EncoderModel(max_length=max_length, checkpoint_path=t5_ckpt, device=device, tokenizer_path=tokenizer_path, **kw)
    ctx = t5.encode_text([prompt, negative_prompt])
    del t5
    clip = CLIPModel(device=device, checkpoint_path=clip_ckpt)
    feats = clip.visual([ref.to(device)])                                               # (1, 257, 1280)
    del clip
    torch.cuda.empty_cache()
    return dict(context=ctx[0:1].contiguous(), uncond_context=ctx[1:2].contiguous(), clip=feats)


PREPROCESS_ROUTES = ("torch", "hip")
POSTPROCESS_ROUTES = ("torch", "hip")


def request_from_files(ref_image: str, pose_video: str, cfg, conditioning: str = None, device="cuda", seed=0, text_dim=4096,
                       preprocess="torch"):
    """The reference's request assembly from files (sample_video.py:300-351): reference image + driving (pose) video ->
    centre-cropped, [-1, 1], pose at half resolution (``smpl_downsample``).  Text / CLIP conditioning comes from
    ``conditioning`` (a .pt with context, uncond_context, clip) -- the T5 tokenizer files are not available offline --
    or is drawn synthetically.  ``preprocess``: "torch" (default) resizes on the host with torch over the whole clip; "hip" sends the
    clip to ``device`` as uint8, a chunk of frames at a time, and resizes / crops / halves it with the library's kernels
    (scail_amd/preprocess.py ``*_hip``; needs a GPU)."""
    from . import preprocess as pp, video_io
    if preprocess not in PREPROCESS_ROUTES:
        raise ValueError(f"preprocess must be one of {PREPROCESS_ROUTES}, got {preprocess!r}")
    img = video_io.load_image_to_tensor_chw_normalized(ref_image)                       # (1, 3, H, W) in [-1, 1]
    H, W = pp.target_size((img.shape[2], img.shape[3]), cfg.get("args", {}).get("sampling_image_size", [512, 896]))
    if preprocess == "hip":
        img = pp.prepare_reference_image_hip(img, (H, W), device=device)
        smpl = pp.prepare_pose_video_hip(video_io.load_video_for_pose_sample(pose_video), (H, W), device=device)[1]   # (3, T, H/2, W/2)
        n_frames = smpl.shape[1]
    else:
        img = pp.prepare_reference_image(img, (H, W))
        pose = video_io.load_video_for_pose_sample(pose_video).permute(0, 3, 1, 2)     # T H W C -> T C H W (:339)
        smpl = pp.prepare_pose_video(pose, (H, W), downsample=True)[1].permute(1, 0, 2, 3).contiguous().to(device)   # (3, T, H/2, W/2)
        n_frames = smpl.shape[1]
    req = synthetic_request(H, W, n_frames, text_dim, 512 if text_dim == 4096 else 12, device, seed)
    if conditioning:
        req.update({k: v.to(device) for k, v in torch.load(conditioning, map_location="cpu").items()
                    if k in ("context", "uncond_context", "clip")})
    req["ref"] = img[0].unsqueeze(1).contiguous().to(device)                            # (1, 3, H, W) -> (3, 1, H, W), dense strides on either route
    req["pose"] = smpl
    return req, (H, W)


def lora_arg(value):
    """``--lora FILE[:STRENGTH]`` -> (path, strength): what follows the LAST colon is the strength when it reads as a number (so a path
    with colons works as long as a strength is given), else the whole value is the path and the strength is 1"""
    path, sep, tail = str(value).rpartition(":")
    if sep and path:
        try:
            strength = float(tail)
        except ValueError:
            return str(value), 1.0
        if not math.isfinite(strength):
            raise ValueError(f"--lora {value}: the strength must be finite")
        return path, strength
    return str(value), 1.0


def apply_loras(engine, loras):
    """Merge the adapters [(path, strength), ...] into the engine's network, in order (engine.load_lora), and print one table each"""
    from . import lora
    for path, strength in loras or ():
        print(lora.format_table(path, strength, engine.load_lora(path, strength)))


def build_engine(cfg, load=None, device="cuda", loras=None):
    """Under ``python -m torch.distributed.run`` the whole world is one sequence-parallel group (the reference's CLI: dp = 1,
    sample_video.py:229): every rank builds the engine, encodes the request and joins ``engine.sample``; SP rank 0 decodes
    and saves (:484-507)."""
    lib.load()
    mc = dict(cfg["model"])
    mc["build_first_stage"] = True
    sp = None
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        from . import parallel
        backend = os.environ.get("SCAIL_DIST_BACKEND", "nccl")          # "gloo": ranks sharing one GPU (tests only)
        if backend == "nccl":
            device = f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}"
        sp = parallel.init_from_env(backend)
    engine = SATVideoDiffusionEngine(mc, device=device, sp=sp)
    if load:
        from .checkpoint import load_checkpoint
        load_checkpoint(engine, load, force_inference=cfg.get("args", {}).get("force_inference", True))
    apply_loras(engine, loras)                                             # after --load: an adapter goes onto the checkpoint's weights
    return engine


def fp8_max_error_arg(value, gemm_precision):
    """``--fp8-max-error`` checked against the network's GEMM precision: a number >= 0 (inf allowed), and only with quantised (fp8 or fp6) GEMMs."""
    if value is None:
        return None
    value = float(value)
    if not value >= 0.0:
        raise ValueError(f"--fp8-max-error must be a number >= 0, got {value}")
    if gemm_precision not in lib.GEMM_PRECISIONS:
        raise ValueError("--fp8-max-error needs --gemm-precision fp8 (or gemm_precision: fp8 in the network's yaml): it chooses which fp8 GEMMs to keep")
    return value


def fp8_scaling_arg(value, gemm_precision):
    """``--fp8-scaling`` checked against the network's GEMM precision: "row" or "mx" (lib.FP8_SCALINGS), "mx" only with fp8 GEMMs."""
    if value is None:
        return None
    if value not in lib.FP8_SCALINGS:
        raise ValueError(f"--fp8-scaling must be one of {sorted(lib.FP8_SCALINGS)}, got {value!r}")
    if value != "row" and gemm_precision != "fp8":
        raise ValueError(f"--fp8-scaling {value} needs --gemm-precision fp8 (or gemm_precision: fp8 in the network's yaml): it scales the fp8 GEMMs")
    return value


def step_cache_args(threshold, coefficients=None, keep=None, signal=None):
    """``--step-cache-threshold`` / ``--step-cache-coefficients`` / ``--step-cache-keep`` / ``--step-cache-signal`` -> the ``step_cache`` option
    of RFSampler.sample_hip, or None when no threshold is given (the other three only shape the plan a threshold makes)."""
    if threshold is None:
        if coefficients is not None or keep is not None or signal is not None:
            raise ValueError("--step-cache-coefficients / --step-cache-keep / --step-cache-signal need --step-cache-threshold (they shape its plan)")
        return None
    threshold = float(threshold)
    if not threshold >= 0.0:
        raise ValueError(f"--step-cache-threshold must be a number >= 0, got {threshold}")
    opt = {"threshold": threshold, "signal": "time" if signal is None else signal}
    if opt["signal"] not in lib.CACHE_SIGNALS:
        raise ValueError(f"--step-cache-signal must be one of {sorted(lib.CACHE_SIGNALS)}, got {signal!r}")
    if coefficients is not None:
        try:
            opt["coefficients"] = [float(v) for v in str(coefficients).split(",")]
        except ValueError:
            raise ValueError(f"--step-cache-coefficients must be numbers separated by commas, highest degree first, got {coefficients!r}")
        if not opt["coefficients"]:
            raise ValueError("--step-cache-coefficients must hold at least one number")
    if keep is not None:
        try:
            first, last = (int(v) for v in str(keep).split(","))
        except ValueError:
            raise ValueError(f"--step-cache-keep must be FIRST,LAST (two integers), got {keep!r}")
        if first < 1 or last < 0:
            raise ValueError(f"--step-cache-keep needs FIRST >= 1 (step 0 has nothing to reuse) and LAST >= 0, got {keep!r}")
        opt["keep_first"], opt["keep_last"] = first, last
    return opt


def guidance_args(interval=None, every=None, plan=None, tile_frames=None):
    """``--cfg-interval LO HI`` / ``--cfg-delta-every K`` / ``--cfg-plan 0,2,1,...`` -> the ``guidance`` option of RFSampler.sample_hip, or None
    when none of the three is given.  An explicit plan stands alone; none of them goes with ``--tile-frames``."""
    if interval is None and every is None and plan is None:
        return None
    if tile_frames is not None:
        raise ValueError("--cfg-interval / --cfg-delta-every / --cfg-plan do not go with --tile-frames: the tiled loops keep no delta per temporal window")
    if plan is not None:
        if interval is not None or every is not None:
            raise ValueError("--cfg-plan stands alone: --cfg-interval and --cfg-delta-every make a plan from the schedule")
        try:
            modes = [int(v) for v in str(plan).split(",")]
        except ValueError:
            raise ValueError(f"--cfg-plan must be entries 0 / 1 / 2 separated by commas, one per step, got {plan!r}")
        from .sampler import check_guidance_plan
        return {"modes": check_guidance_plan(modes, what="--cfg-plan")}
    opt = {}
    if interval is not None:
        lo, hi = (float(v) for v in interval)
        if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi:
            raise ValueError(f"--cfg-interval needs finite LO <= HI (sigma runs from 1 down to 0), got {lo} {hi}")
        opt["interval"] = (lo, hi)
    if every is not None:
        if int(every) < 1:
            raise ValueError(f"--cfg-delta-every must be an integer >= 1, got {every}")
        opt["every"] = int(every)
    return opt


def format_guidance_plan(plan):
    """The plan as text: which steps run the pair, and k of n"""
    pair = [i for i, v in enumerate(plan) if v == 0]
    n_delta, n_cond = sum(1 for v in plan if v == 1), sum(1 for v in plan if v == 2)
    return (f"guidance plan: {len(pair)} of {len(plan)} steps run the uncond / cond pair ({', '.join(map(str, pair))}); {n_delta} run the cond "
            f"branch with the last stored delta, {n_cond} the cond branch without guidance")


SOLVER_CHOICES = ("euler", "dpmpp2m")


def solver_args(solver, step_cache=None, guidance=None):
    """``--solver`` -> the ``solver`` option of RFSampler.sample_hip: None for "euler" (the route as it was), else the name.  A solver
    goes with neither the step cache nor the guidance plan."""
    if solver is None or solver == "euler":
        return None
    if solver not in SOLVER_CHOICES:
        raise ValueError(f"--solver must be one of {SOLVER_CHOICES}, got {solver!r}")
    if step_cache is not None:
        raise ValueError(f"--solver {solver} does not go with --step-cache-threshold: the solver's pass takes the pair of a full step")
    if guidance is not None:
        raise ValueError(f"--solver {solver} does not go with --cfg-interval / --cfg-delta-every / --cfg-plan: the solver's pass takes the "
                         "pair of a full step")
    return solver


def format_solver_plan(plan, solver="dpmpp2m"):
    """The table as text: which steps are second order, and k of n"""
    second = [i for i, row in enumerate(plan) if row[2] != 0.0]
    return (f"solver plan ({solver}): {len(second)} of {len(plan)} steps are second order ({', '.join(map(str, second))}); the others are "
            "first order (no usable history, or a step that starts at sigma = 1 or ends at sigma = 0)")


def format_step_cache_plan(plan):
    """The plan as text: which steps compute, and k of n"""
    computed = [i for i, v in enumerate(plan) if not v]
    return f"step cache: {len(computed)} of {len(plan)} steps compute the blocks ({', '.join(map(str, computed))}); the others reuse the last computed residual"


def format_fp8_table(cal, max_rel_err):
    """The probe's result as text: a heading that names the scaling probed (cal["scaling"]; "row" when absent), one row per layer, one
    column per GEMM, then the (layer, GEMM) pairs left in bf16."""
    names = list(lib.FP8_GEMMS)
    rel, masks = cal["rel_err"], cal["masks"]
    head = "fp6 probe (MXFP6 e2m3)" if cal.get("precision", "fp8") == "fp6" else f"fp8 probe ({cal.get('scaling', 'row')} scaling)"
    kind = cal.get("precision", "fp8")
    out = [f"{head}: relative error of each {kind} GEMM against its bf16 twin (first evaluation), threshold {max_rel_err:g}",
           "layer " + " ".join(f"{n:>8}" for n in names)]
    for i in range(rel.shape[0]):
        out.append(f"{i:5d} " + " ".join(f"{float(rel[i, g]):8.2e}" for g in range(len(names))))
    left = [f"({i}, {n})" for i in range(rel.shape[0]) for g, n in enumerate(names) if (cal["enabled"] >> g) & 1 and not (masks[i] >> g) & 1]
    out.append("left in bf16: " + (", ".join(left) if left else "none"))
    return "\n".join(out)


def _calibrate(engine, c, uc, shape, steps, fp8_max_error):
    """--fp8-max-error: once per request, before sampling (its noise comes from a generator of its own)"""
    if fp8_max_error is None:
        return
    cal = engine.calibrate_fp8(c, uc, shape, fp8_max_error, num_steps=steps)
    print(format_fp8_table(cal, fp8_max_error))


def run(cfg, inputs=None, steps=None, load=None, seed=1234, device="cuda", frames=None, engine=None, tile_frames=None, tile_overlap=None,
        vae_chunk_frames=None, postprocess="torch", fp8_max_error=None, step_cache=None, guidance=None, solver=None, loras=None):
    """``loras``: None, or [(path, strength), ...] -- LoRA adapters merged into the network's weights in this order after ``load``
    (scail_amd/lora.py; an extension), when this call builds the engine; an ``engine`` that is passed in is merged by its owner
    (engine.load_lora), once.  One table per adapter is printed.
    ``solver``: None (the Euler loop as it was), or "dpmpp2m" (solver_args; RFSampler.sample_hip / RFSamplerLong.sample_hip): a second-order
    multistep update in the data prediction, still one executor call: one window, several characters, temporal tiles.  One rank; not with
    ``step_cache`` or ``guidance``.  The plan is printed.
    ``guidance``: None, or the guidance option (guidance_args; RFSampler.sample_hip): which steps run the CFG pair, the cond branch with
    the stored delta, or the cond branch alone.  One rank, one window.  The plan is printed.
    ``fp8_max_error`` (fp8 networks only): probe the request's first evaluation and keep in bf16 every (layer, GEMM) whose fp8 result is
    further than this from bf16 (engine.calibrate_fp8).
    ``step_cache``: None, or the step-cache option (step_cache_args; RFSampler.sample_hip): steps whose time embedding moved little reuse the
    block residual of the last computed step.  One rank; a clip longer than one window keeps one residual per temporal tile under one
    plan.  The plan is printed.
    ``postprocess``: "torch" (default) returns the video as fp32 (B, 3, T, H, W) in [0, 1]; "hip" returns it as the file writers' pixels,
    uint8 (B, T, H, W, 3) on the device, written by the VAE decoder's last kernel (engine.decode_first_stage_u8; needs a GPU)."""
    if postprocess not in POSTPROCESS_ROUTES:
        raise ValueError(f"postprocess must be one of {POSTPROCESS_ROUTES}, got {postprocess!r}")
    if postprocess == "hip" and not torch.cuda.is_available():
        raise lib.ScailHipError("postprocess='hip' writes the uint8 frames with the library's kernels and needs a GPU; there is no host fallback")
    fp8_max_error = fp8_max_error_arg(fp8_max_error, cfg["model"]["network_config"].get("params", {}).get("gemm_precision", "bf16"))
    if loras and engine is not None:
        raise ValueError("loras go with the engine this call builds; merge them into a passed engine once, with engine.load_lora")
    engine = engine or build_engine(cfg, load, device, loras=loras)
    H, W = cfg.get("args", {}).get("sampling_image_size", [512, 896])
    net = engine.network
    frames = frames or min(81, net.num_frames)
    if callable(inputs):                                      # file-based request: needs the network's text width
        inputs = inputs(net.text_dim)
    req = inputs or synthetic_request(H, W, frames, net.text_dim, 512 if net.text_dim == 4096 else 12, device, seed)
    t0 = time.perf_counter()
    # model.encode_first_stage(..., force_encode=True): VAE mean x scale_factor (sample_video.py:366, :381; diffusion_video.py:311-331)
    ref_lat = engine.encode_first_stage(req["ref"].unsqueeze(0), None, force_encode=True)
    n_pix = req["pose"].shape[1]
    if n_pix > (net.num_frames if tile_frames is None else tile_frames):      # longer than one window: temporal tiles (an extension)
        if (n_pix - 1) % 4:
            raise ValueError(f"a pose clip longer than one window needs 4n + 1 frames (the causal VAE's frame groups), got {n_pix}")
        Tt, overlap = tile_args(tile_frames, tile_overlap, net.num_frames)
        tiles = plan_tiles((n_pix - 1) // 4 + 1, Tt, overlap)
        if guidance is not None:
            raise NotImplementedError("guidance with temporal tiles is out of scope: this pose clip is longer than one window and the tiled loops "
                                      "keep no delta per temporal window")
        return _run_tiled(cfg, engine, req, ref_lat, tiles, steps, seed, device, t0, vae_chunk_frames, postprocess, fp8_max_error, step_cache,
                          solver)
    pose_lat = engine.encode_first_stage(req["pose"].unsqueeze(0), None, force_encode=True)   # already half resolution (:350-351)
    ref_concat = ref_lat.permute(0, 2, 1, 3, 4).contiguous().to(torch.bfloat16)      # B C T H W -> B T C H W
    pose_latent = pose_lat.permute(0, 2, 1, 3, 4).contiguous().to(torch.bfloat16)
    T, C, h, w = pose_latent.shape[1], ref_concat.shape[2], ref_concat.shape[3], ref_concat.shape[4]
    shared = dict(concat_images=torch.zeros(1, device=device), ref_concat=ref_concat, concat_pose=pose_latent,
                  concat_smpl_render=pose_latent, image_clip_features=req["clip"].to(torch.bfloat16))
    c = dict(crossattn=req["context"], **shared)
    uc = dict(crossattn=req["uncond_context"], **shared)
    _calibrate(engine, c, uc, (T, C, h, w), steps, fp8_max_error)
    torch.manual_seed(seed)
    opts = {k: v for k, v in (("step_cache", step_cache), ("guidance", guidance), ("solver", solver)) if v is not None}
    z = engine.sample(c, uc=uc, batch_size=1, shape=(T, C, h, w), num_steps=steps, **opts)
    if step_cache is not None:
        print(format_step_cache_plan(engine.sampler.last_step_cache_plan))
    if guidance is not None:
        print(format_guidance_plan(engine.sampler.last_guidance_plan))
    if solver is not None:
        print(format_solver_plan(engine.sampler.last_solver_plan, solver))
    return _finish(engine, z, t0, vae_chunk_frames, postprocess)


def _finish(engine, z, t0, vae_chunk_frames=None, postprocess="torch"):
    """sampled latent (B T C H W) -> (video in [0, 1], latent (B C T H W), seconds); (None, None, seconds) off sequence-parallel rank 0.
    ``postprocess`` "hip": the video is uint8 (B, T, H, W, 3) instead, the same pixels the writers make of the fp32 one."""
    if engine.sp is not None and engine.sp.size > 1 and engine.sp.rank != 0:
        torch.cuda.synchronize()
        return None, None, time.perf_counter() - t0                         # only SP rank 0 holds the gathered latent (:484)
    z = z.permute(0, 2, 1, 3, 4).contiguous()                               # B T C H W -> B C T H W (:484-485)
    if postprocess == "hip":
        video = engine.decode_first_stage_u8(z.float(), chunk_frames=vae_chunk_frames)
        torch.cuda.synchronize()
        return video, z, time.perf_counter() - t0
    x = engine.decode_first_stage(z.float(), chunk_frames=vae_chunk_frames)
    video = torch.clamp((x + 1.0) / 2.0, 0.0, 1.0)                          # (:494)
    torch.cuda.synchronize()
    return video, z, time.perf_counter() - t0


def _run_tiled(cfg, engine, req, ref_lat, tiles, steps, seed, device, t0, vae_chunk_frames=None, postprocess="torch", fp8_max_error=None,
               step_cache=None, solver=None):
    """A pose clip longer than one window (an extension, see the module docstring): RFSamplerLong with the configured sampler's
    parameters over ``tiles``; every window's pose frames [4 start, 4 (start + Tt - 1)] are VAE-encoded on their own (the causal VAE treats
    a window's first frame as a clip's first frame, which is how ``smpl_tiled[:, k]`` is used); noise and decode for the whole latent.
    ``step_cache``: as for ``run`` -- one plan shared by the tiles, one residual per tile (RFSamplerLong.sample_hip); the plan is printed.
    ``solver``: as for ``run`` -- one update of the whole latent per step, one history for every tile; the plan is printed."""
    from . import sampler as S
    Tt = len(tiles[0])
    ref_concat = ref_lat.permute(0, 2, 1, 3, 4).contiguous().to(torch.bfloat16)
    wins = []
    for t in tiles:
        lat = engine.encode_first_stage(req["pose"][:, 4 * t[0]:4 * (t[0] + Tt - 1) + 1].unsqueeze(0), None, force_encode=True)
        wins.append(lat.permute(0, 2, 1, 3, 4).contiguous().to(torch.bfloat16))
    smpl_tiled = torch.stack(wins, 1)                                       # (1, n_tiles, Tt, 16, h/2, w/2)
    T, C, h, w = tiles[-1][-1] + 1, ref_concat.shape[2], ref_concat.shape[3], ref_concat.shape[4]
    shared = dict(concat_images=torch.zeros(1, device=device), ref_concat=ref_concat, smpl_tiled=smpl_tiled,
                  image_clip_features=req["clip"].to(torch.bfloat16))
    c = dict(crossattn=req["context"], **shared)
    uc = dict(crossattn=req["uncond_context"], **shared)
    params = dict(cfg["model"]["sampler_config"].get("params", {}))
    params["device"] = device
    plain, engine.sampler = engine.sampler, S.RFSamplerLong(**params)
    try:
        _calibrate(engine, c, uc, (T, C, h, w), steps, fp8_max_error)       # the first window
        torch.manual_seed(seed)
        if solver is not None:
            z = engine.sample(c, uc=uc, batch_size=1, shape=(T, C, h, w), num_steps=steps, tile_indices=tiles, solver=solver,
                              **({} if step_cache is None else {"step_cache": step_cache}))
            print(format_solver_plan(engine.sampler.last_solver_plan, solver))
        elif step_cache is None:
            z = engine.sample(c, uc=uc, batch_size=1, shape=(T, C, h, w), num_steps=steps, tile_indices=tiles)
        else:
            z = engine.sample(c, uc=uc, batch_size=1, shape=(T, C, h, w), num_steps=steps, tile_indices=tiles, step_cache=step_cache)
            print(format_step_cache_plan(engine.sampler.last_step_cache_plan))
    finally:
        engine.sampler = plain
    return _finish(engine, z, t0, vae_chunk_frames, postprocess)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", nargs="*", default=[])
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--inputs", default=None)
    ap.add_argument("--load", default=None)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ref-image", default=None, help="reference image file (any Pillow format)")
    ap.add_argument("--pose-video", default=None, help="driving video: directory of frames, .npy/.pt (T,H,W,3) or animated WebP/PNG/GIF")
    ap.add_argument("--conditioning", default=None, help=".pt with context / uncond_context / clip tensors")
    ap.add_argument("--prompt", default=None, help="text prompt (needs --tokenizer; UMT5 / CLIP run on the GPU, random-init without --t5-ckpt / --clip-ckpt)")
    ap.add_argument("--negative-prompt", default="")
    ap.add_argument("--tokenizer", default=None, help="Hugging Face tokenizer directory or SentencePiece .model file of umt5-xxl")
    ap.add_argument("--t5-ckpt", default=None)
    ap.add_argument("--clip-ckpt", default=None)
    ap.add_argument("--save-dir", default=None, help="write <key>_000000.<ext> like the reference's save_multi_video_grid_and_mp4")
    ap.add_argument("--format", default=".webp", help=".webp (lossless) | .png (APNG) | .gif | .npy | .mp4 (Motion JPEG) | '' (directory of PNG frames)")
    ap.add_argument("--request", action="append", default=[], help="'<prompt>@@<example_dir>' (the reference's cli input line); repeatable")
    ap.add_argument("--input-file", default=None, help="text file of request lines (the reference's --input-type txt)")
    ap.add_argument("--output-dir", default="outputs", help="results of --request / --input-file go to <output-dir>/<example>/")
    ap.add_argument("--gemm-precision", choices=("bf16",) + lib.GEMM_PRECISIONS, default=None,
                    help="precision of the six per-token GEMMs of every block (default: the config's, bf16); fp8 = e4m3 with per-token / "
                         "per-channel scales, single GPU; fp6 = OCP MXFP6 e2m3, 6-bit codes with one power-of-two scale per block of 32 "
                         "along K (--fp8-max-error works under it; --fp8-scaling does not apply), single GPU")
    ap.add_argument("--fp8-scaling", choices=tuple(lib.FP8_SCALINGS), default=None,
                    help="scaling of the fp8 GEMMs (default: the config's fp8_scaling, row): row = one fp32 scale per token / output "
                         "channel; mx = OCP MX, one power-of-two scale per block of 32 along K in the matrix instruction, so an outlier "
                         "channel costs its own block and not its whole row.  Not yet measured on a real checkpoint: compare the "
                         "--fp8-max-error table under both")
    ap.add_argument("--fp8-max-error", type=float, default=None,
                    help="with fp8 GEMMs: before sampling, run the request's first network evaluation through the executor's error probe "
                         "and keep in bf16 every (layer, GEMM) whose fp8 result is further than this (relative error against its bf16 "
                         "twin) from bf16; prints the table.  No measured table of a real checkpoint exists yet: choose the value from "
                         "the printed table of your own weights")
    ap.add_argument("--step-cache-threshold", type=float, default=None,
                    help="opt-in step cache (an extension): a sampler step reuses the change the blocks made to the hidden states at the last "
                         "computed step, and runs only the patch embedding and the final layer, while the accumulated relative change of the "
                         "time embedding since that step stays below this number; 0 computes every step.  The plan is printed.  No value is "
                         "recommended: nothing has been measured on real weights, and random-init weights say nothing about quality.  "
                         "Single GPU.  A pose clip longer than one window (--tile-frames) keeps one such change per temporal window under "
                         "one plan for all of them")
    ap.add_argument("--step-cache-coefficients", default=None,
                    help="with --step-cache-threshold: polynomial applied to each step's relative change before it is accumulated, "
                         "comma-separated, highest degree first (default 1,0: the identity).  No fitted values are shipped")
    ap.add_argument("--step-cache-keep", default=None,
                    help="with --step-cache-threshold: FIRST,LAST = steps at the start (>= 1) and at the end that always compute (default 1,1)")
    ap.add_argument("--step-cache-signal", choices=tuple(lib.CACHE_SIGNALS), default=None,
                    help="with --step-cache-threshold: what is compared between steps: time = the timestep embedding (default), "
                         "modulation = its AdaLN projection, the 6 D values every block is modulated with")
    ap.add_argument("--cfg-interval", type=float, nargs=2, metavar=("LO", "HI"), default=None,
                    help="opt-in guidance plan (an extension): classifier-free guidance only on the steps whose starting sigma lies in "
                         "[LO, HI] (sigma runs from 1 down to 0); the other steps run the cond branch alone, about half the work of a step "
                         "by FLOP count.  The plan is printed.  No interval is recommended: nothing has been measured on real weights.  "
                         "One GPU and a clip of one window (not with --tile-frames); combines with --step-cache-threshold")
    ap.add_argument("--cfg-delta-every", type=int, metavar="K", default=None,
                    help="opt-in guidance plan: inside the interval (every step without --cfg-interval) only every K-th step runs the uncond / "
                         "cond pair; the steps between run the cond branch alone and reuse v_c - v_u of the last pair step.  No K is recommended")
    ap.add_argument("--cfg-plan", default=None,
                    help="opt-in guidance plan, spelled out: one entry per step, comma-separated: 0 = the pair, 1 = cond branch + stored delta, "
                         "2 = cond branch without guidance.  Stands alone; with --step-cache-threshold it must agree with that plan as it stands")
    ap.add_argument("--solver", choices=SOLVER_CHOICES, default="euler",
                    help="opt-in solver plan (an extension): dpmpp2m = DPM-Solver++(2M), a second-order multistep update in the data prediction "
                         "that needs no further network evaluation per step (one fp32 pass and one fp32 latent of history); euler (default) "
                         "is the route as it was.  The plan is printed.  No step count is recommended: nothing has been measured on real "
                         "weights.  One GPU; one window, several characters and --tile-frames clips; not with --step-cache-threshold or the "
                         "--cfg-* plans")
    ap.add_argument("--lora", action="append", default=[], metavar="FILE[:STRENGTH]",
                    help="merge a LoRA adapter into the DiT's weights on the GPU (an extension): .safetensors or a torch.load-able file with "
                         "lora_A / lora_B or lora_down / lora_up pairs, alpha, diff and diff_b keys under the native or Wan2.1 module "
                         "names; repeatable, applied in order after --load; STRENGTH defaults to 1.  One table per adapter is printed.  "
                         "The Wan2.1 names could not be checked against a real adapter file")
    ap.add_argument("--tile-frames", type=int, default=None,
                    help="pixel frames per temporal window, 4n + 1 (default: the network's num_frames); a pose clip with more frames is sampled "
                         "in overlapping windows (RFSamplerLong), an extension of the reference CLI; such a clip needs 4n + 1 frames")
    ap.add_argument("--tile-overlap", type=int, default=None,
                    help="pixel frames shared by neighbouring windows, a multiple of 4 and smaller than the window (default: half of the "
                         "window's latent frames, e.g. 40 for an 81-frame window)")
    ap.add_argument("--vae-chunk-frames", type=int, default=None,
                    help="decode the sampled latent in chunks of this many latent frames (>= 2; one latent frame is four pixel frames): "
                         "the VAE workspace then depends on this number and the frame size instead of the clip length (512x896: 10.9 GB with 4 instead of 85 GB "
                         "for 161 frames), at the price of smaller launches and two frame copies per causal convolution and chunk; same video. "
                         "Unset: one pass over the whole clip")
    ap.add_argument("--preprocess", choices=PREPROCESS_ROUTES, default="torch",
                    help="where the reference image and the driving video are resized, cropped and halved: torch = on the host, the whole clip "
                         "at once as fp32; hip = on the GPU with the library's kernels, the clip crossing as uint8 a chunk of frames at a time "
                         "(bounded host and device memory for long clips)")
    ap.add_argument("--postprocess", choices=POSTPROCESS_ROUTES, default="torch",
                    help="where the decoded clip becomes the writers' 8-bit pixels: torch = the decoder returns fp32, clamp and scaling run as "
                         "torch ops and the writer quantises on the host; hip = the decoder's last kernel writes uint8 (T, H, W, 3) frames, "
                         "which cross to the host once (no fp32 video on either side; --out then holds the uint8 tensor)")
    return ap


def _save(video_io, video, save_dir, fps, key, ext):
    """the clip of ``run`` to files: fp32 (B, 3, T, H, W) goes to the writer as (B, T, 3, H, W), uint8 (B, T, H, W, 3) as it is"""
    samples = video.cpu() if video.dtype == torch.uint8 else video.permute(0, 2, 1, 3, 4).contiguous().cpu()      # B C T H W -> B T C H W (:493)
    return video_io.save_multi_video_grid([samples], save_dir, fps=fps, key=key, ext=ext)


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.vae_chunk_frames is not None and a.vae_chunk_frames < 2:
        ap.error(f"--vae-chunk-frames must be at least 2 latent frames, got {a.vae_chunk_frames}")
    cfg = TINY if a.tiny or not a.base else load_yaml_configs(*a.base)
    if a.tile_frames is not None or a.tile_overlap is not None:         # argument errors before any model is built
        try:
            tile_args(a.tile_frames, a.tile_overlap, cfg["model"]["network_config"].get("params", {}).get("num_frames", 81))
        except ValueError as e:
            ap.error(str(e))
    tk = dict(tile_frames=a.tile_frames, tile_overlap=a.tile_overlap, vae_chunk_frames=a.vae_chunk_frames, postprocess=a.postprocess)
    if a.gemm_precision is not None:
        cfg = copy.deepcopy(cfg)
        cfg["model"]["network_config"].setdefault("params", {})["gemm_precision"] = a.gemm_precision
    try:                                                                # an argument error before any model is built
        params = cfg["model"]["network_config"].get("params", {})
        if fp8_scaling_arg(a.fp8_scaling, params.get("gemm_precision", "bf16")) is not None:
            if a.gemm_precision is None:
                cfg = copy.deepcopy(cfg)
            cfg["model"]["network_config"].setdefault("params", {})["fp8_scaling"] = a.fp8_scaling
        tk["fp8_max_error"] = fp8_max_error_arg(a.fp8_max_error, cfg["model"]["network_config"].get("params", {}).get("gemm_precision", "bf16"))
        sc = step_cache_args(a.step_cache_threshold, a.step_cache_coefficients, a.step_cache_keep, a.step_cache_signal)
        if sc is not None:
            tk["step_cache"] = sc
        gd = guidance_args(a.cfg_interval, a.cfg_delta_every, a.cfg_plan, a.tile_frames)
        if gd is not None:
            tk["guidance"] = gd
        sv = solver_args(a.solver, sc, gd)
        if sv is not None:
            tk["solver"] = sv
        loras = [lora_arg(v) for v in a.lora]
    except ValueError as e:
        ap.error(str(e))
    lines = [(r, i) for i, r in enumerate(a.request)] + (list(read_from_file(a.input_file)) if a.input_file else [])
    if lines:
        import os
        from . import video_io
        engine = build_engine(cfg, a.load, loras=loras)
        td = engine.network.text_dim
        for line, cnt in lines:
            text, input_dir, image_path, pose_path = parse_request(line)
            print(cnt, ": ", text)
            req = request_from_files(image_path, pose_path, cfg, a.conditioning, seed=a.seed, text_dim=td, preprocess=a.preprocess)[0]
            if a.tokenizer:
                req.update(encode_conditioning(text, a.negative_prompt, req["ref"], td, a.tokenizer, a.t5_ckpt, a.clip_ckpt,
                                               max_length=512 if td == 4096 else 16))
            video, z, dt = run(cfg, req, a.steps, seed=a.seed, engine=engine, **tk)
            if video is None:
                continue
            save_dir = os.path.join(a.output_dir, os.path.basename(os.path.normpath(input_dir)))
            os.makedirs(save_dir, exist_ok=True)
            with open(os.path.join(save_dir, "text.txt"), "w") as f:                   # sample_video.py:413-414
                f.write(text)
            paths = _save(video_io, video, save_dir, cfg.get("args", {}).get("sampling_fps", 16),
                          f"{os.path.basename(os.path.normpath(input_dir))}_output", a.format)
            print(f"  latent {tuple(z.shape)} -> video {tuple(video.shape)} in {dt:.2f} s; wrote {', '.join(paths)}")
        return
    inputs = torch.load(a.inputs) if a.inputs else None
    if a.ref_image or a.pose_video:
        if not (a.ref_image and a.pose_video):
            ap.error("--ref-image and --pose-video go together")
        def inputs(text_dim):
            req = request_from_files(a.ref_image, a.pose_video, cfg, a.conditioning, seed=a.seed, text_dim=text_dim, preprocess=a.preprocess)[0]
            if a.prompt is not None:
                if not a.tokenizer:
                    ap.error("--prompt needs --tokenizer (tokenizer files are not bundled)")
                req.update(encode_conditioning(a.prompt, a.negative_prompt, req["ref"], text_dim, a.tokenizer, a.t5_ckpt, a.clip_ckpt,
                                               max_length=512 if text_dim == 4096 else 16))
            return req
    video, z, dt = run(cfg, inputs, a.steps, a.load, a.seed, loras=loras, **tk)
    if video is None:
        return
    print(f"sampled latent {tuple(z.shape)} -> video {tuple(video.shape)} in {dt:.2f} s")
    if a.out:
        torch.save({"video": video.cpu(), "latent": z.cpu()}, a.out)
    if a.save_dir:
        from . import video_io
        paths = _save(video_io, video, a.save_dir, cfg.get("args", {}).get("sampling_fps", 16), "0_output", a.format)
        print("wrote", ", ".join(paths))


if __name__ == "__main__":
    main()
