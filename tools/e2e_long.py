"""Long-video request at full size: RFSamplerLong temporal tiling (reference sampling.py:986-1085) over a 41-frame latent
(161 video frames, 512x896) in 21-frame windows planned by scail_amd.cli.plan_tiles (overlap 10: three tiles), SCAIL-14B shapes,
random-init weights, N sampler steps (default 1), then VAE decode of the 161 frames.  Checks shapes and finiteness; prints times.

    python tools/e2e_long.py [steps] [--route onecall|host|both] [--reps R] [--latent-frames T] [--no-decode]

--route onecall (default): the whole loop in ONE executor call (scail_dit_sample_tiled).  host: the Python loop of
RFSamplerLong.sample_hip (forced with a step callback).  both: the two routes ALTERNATE R times in this process (same noise, same
conditioning), per-step times of every repetition, their spread and whether the two latents are equal are printed."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scail_amd import sampler as S
from scail_amd.cli import plan_tiles
from scail_amd.engine import SATVideoDiffusionEngine

ap = argparse.ArgumentParser()
ap.add_argument("steps", nargs="?", type=int, default=1)
ap.add_argument("--route", choices=("onecall", "host", "both"), default="onecall")
ap.add_argument("--reps", type=int, default=1)
ap.add_argument("--latent-frames", type=int, default=41)
ap.add_argument("--no-decode", action="store_true")
a = ap.parse_args()
steps = a.steps
dev = "cuda"
sampler_params = dict(hunyuan_schedule=True, shift_scale=5, num_steps=50,
                      guider_config={"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": 4}})
mc = {
    "use_i2v_clip": True, "scale_factor": 1.0, "build_first_stage": True,
    "network_config": {"target": "dit_video_crossattn_sc_xc.DiffusionTransformer", "params": dict(
        time_freq_dim=256, time_embed_dim=5120, share_adaln=True, elementwise_affine=False, num_frames=81,
        time_compressed_rate=4, latent_width=300, latent_height=300, num_layers=40, patch_size=[1, 2, 2], in_channels=20,
        out_channels=16, text_dim=4096, hidden_size=5120, inner_hidden_size=13824, num_attention_heads=40,
        transformer_args=dict(model_parallel_size=1, is_decoder=True),
        modules={"pos_embed_config": {"params": {"hidden_size_head": 128, "interleaved_rope": True}},
                 "adaln_layer_config": {"params": {"qk_ln": True, "hidden_size_head": 5120}}})},
    "first_stage_config": {"target": "sgm.models.wan_vae.WanVAE", "params": {"vae_pth": None, "dtype": "torch.bfloat16"}},
    "sampler_config": {"target": "sgm.modules.diffusionmodules.sampling.RFSamplerLong", "params": sampler_params},
}


class HostLoop(S.RFSamplerLong):
    """the Python loop of RFSamplerLong.sample_hip: a step callback keeps a request off the one-call route"""

    def sample_hip(self, *args, **kw):
        return super().sample_hip(*args, step_callback=lambda i, x: None, **kw)


eng = SATVideoDiffusionEngine(mc, device=dev)
samplers = {"onecall": eng.sampler, "host": HostLoop(**sampler_params)}
T, H, W, Tt = a.latent_frames, 64, 112, 21
tiles = plan_tiles(T, Tt, 10)
g = torch.Generator().manual_seed(0)
r = lambda *s: torch.randn(*s, generator=g)
ctx = r(1, 512, 4096); ctx[:, 64:] = 0
uctx = torch.zeros(1, 512, 4096); uctx[:, :1] = r(1, 1, 4096)
shared = dict(concat_images=torch.zeros(1, device=dev), ref_concat=r(1, 1, 16, H, W).to(dev).to(torch.bfloat16),
              smpl_tiled=r(1, len(tiles), Tt, 16, H // 2, W // 2).to(dev).to(torch.bfloat16),
              image_clip_features=r(1, 257, 1280).to(dev).to(torch.bfloat16))
c = dict(crossattn=ctx.to(dev), **shared)
uc = dict(crossattn=uctx.to(dev), **shared)
case = f"long video: {T}-frame latent, {len(tiles)} tiles of {Tt} (starts {[t[0] for t in tiles]}), {steps} step(s)"


def sample(route):
    eng.sampler = samplers[route]
    torch.cuda.reset_peak_memory_stats()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    z = eng.sample(c, uc=uc, batch_size=1, shape=(T, 16, H, W), num_steps=steps, tile_indices=tiles, generator=torch.Generator().manual_seed(1))
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    return z, dt, torch.cuda.max_memory_allocated() / 1e9


routes = ["onecall", "host"] if a.route == "both" else [a.route]
sample(routes[0])                                  # warm-up: conditioning cache, tables, workspaces
per_step = {k: [] for k in routes}
peak = {k: 0.0 for k in routes}
last = {}
for rep in range(a.reps):
    for route in routes:
        z, dt, mem = sample(route)
        per_step[route].append(dt / steps)
        peak[route] = max(peak[route], mem)
        last[route] = z
        print(json.dumps(dict(case=case, rep=rep, route=route, sample_s=dt, s_per_step=dt / steps, peak_mem_GB=mem)), flush=True)
summary = dict(case=case, latent=list(z.shape), finite=bool(torch.isfinite(z.float()).all()))
for route in routes:
    v = per_step[route]
    summary[route] = dict(s_per_step_min=min(v), s_per_step_median=sorted(v)[len(v) // 2], s_per_step_max=max(v),
                          spread_s=max(v) - min(v), peak_mem_GB=peak[route])
if len(routes) == 2:
    summary["routes_equal"] = bool(torch.equal(last["onecall"], last["host"]))
    summary["onecall_minus_host_median_s"] = summary["onecall"]["s_per_step_median"] - summary["host"]["s_per_step_median"]
if not a.no_decode:
    torch.cuda.reset_peak_memory_stats()
    torch.cuda.synchronize(); t1 = time.perf_counter()
    x = eng.decode_first_stage(z.permute(0, 2, 1, 3, 4).contiguous().float())
    torch.cuda.synchronize(); t2 = time.perf_counter()
    summary.update(video=list(x.shape), finite=summary["finite"] and bool(torch.isfinite(x).all()), decode_s=t2 - t1,
                   decode_peak_mem_GB=torch.cuda.max_memory_allocated() / 1e9)
print(json.dumps(summary))
