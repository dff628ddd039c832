"""Sampling engine: the ``sample`` / first-stage surface of SATVideoDiffusionEngine
(reference diffusion_video.py:41-174, :298-331, :456-587) on top of the HIP network.

Only the inference members the CLI uses are reproduced: ``sample(cond, uc, batch_size, shape, ...)``,
``encode_first_stage`` / ``decode_first_stage``, ``.model`` (OpenAIWrapper), ``.denoiser``, ``.sampler``, and -- opt-in --
``.conditioner`` (scail_amd/conditioner.py) and ``.i2v_clip``.
Training (``shared_step``, loss, EMA) is out of scope."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple, Union

import torch
from torch import nn

from . import sampler as S
from .config import instantiate_from_config
from .dit import DiffusionTransformer


class SATVideoDiffusionEngine(nn.Module):
    def __init__(self, model_config: Dict, device="cuda", seed_offset: int = 0, sp=None):
        super().__init__()
        net_cfg = dict(model_config["network_config"])
        params = dict(net_cfg.get("params", {}))
        params["dtype"] = "bf16"                                           # diffusion_video.py:92-105
        params["use_i2v_clip"] = model_config.get("use_i2v_clip", False)
        params["device"] = device
        net = instantiate_from_config({"target": net_cfg["target"], "params": params})
        self.model = S.OpenAIWrapper(net, dtype=torch.bfloat16)
        self.denoiser = instantiate_from_config(model_config["denoiser_config"]) if "denoiser_config" in model_config else S.Denoiser()
        scfg = dict(model_config["sampler_config"])
        sp_params = dict(scfg.get("params", {}))
        sp_params["device"] = device
        self.sampler = instantiate_from_config({"target": scfg["target"], "params": sp_params})
        self.scale_factor = model_config.get("scale_factor", 1.0)
        self.latent_input = model_config.get("latent_input", False)
        self.device = torch.device(device)
        self.dtype = torch.bfloat16
        self.first_stage_model = None
        self.sp = sp
        net.sp = sp
        fs = model_config.get("first_stage_config")
        if fs is not None and model_config.get("build_first_stage", False):
            self.first_stage_model = instantiate_from_config(fs)
        # request-time encoders (diffusion_video.py:113-127: conditioner + i2v_clip).  The reference always builds them; here
        # they are opt-in because their checkpoints / tokenizer files do not exist offline and they cost 13 GB of HBM.
        self.use_i2v_clip = model_config.get("use_i2v_clip", False)
        self.conditioner = self.i2v_clip = None
        if model_config.get("build_conditioner", False) and "conditioner_config" in model_config:
            self.conditioner = instantiate_from_config(model_config["conditioner_config"])
        if model_config.get("build_i2v_clip", False) and "i2v_clip_config" in model_config:
            self.i2v_clip = instantiate_from_config(model_config["i2v_clip_config"])

    @property
    def network(self) -> DiffusionTransformer:
        return self.model.diffusion_model

    def load_lora(self, path, strength: float = 1.0):
        """Merge a LoRA adapter into the network's weights (an extension, opt-in): DiffusionTransformer.merge_lora"""
        return self.network.merge_lora(path, strength)

    @torch.no_grad()
    def sample(self, cond: Dict, uc: Optional[Dict] = None, batch_size: int = 1, shape: Union[None, Tuple, List] = None,
               prefix=None, concat_images=None, ofs=None, fps=None, tile_indices=None,
               generator: Optional[torch.Generator] = None, num_steps: Optional[int] = None, fused: bool = True, step_cache=None, guidance=None,
               solver=None, **kwargs):
        """diffusion_video.py:456-587.  shape = (T, C, H, W).  Noise is drawn in fp32 on the host RNG
        stream of ``generator`` like ``torch.randn(batch, *shape)`` (:470), broadcast inside the
        sequence-parallel group (:486-493) and H/W-chunked (:495-552); result gathered to SP rank 0 (:571-585).
        ``step_cache``: None, or the step-cache option of RFSampler.sample_hip (an extension, opt-in; fused HIP network, one rank).  With
        ``tile_indices`` it reaches RFSamplerLong.sample_hip: one plan for every tile and one block residual per tile, for the requests
        that take the one-call tiled loop; the sampler refuses the others (a callback, several characters, tiles above 64 frames).
        ``guidance``: None, or the guidance option of RFSampler.sample_hip (an extension, opt-in; fused HIP network, one rank, no temporal
        tiles): which steps run the CFG pair, the cond branch with the stored delta, or the cond branch alone.
        ``solver``: None, or the solver option of RFSampler.sample_hip / RFSamplerLong.sample_hip (an extension, opt-in; fused HIP network,
        one rank, with or without ``tile_indices``): "dpmpp2m" or "dpm1" in place of the Euler update.  Not with ``step_cache`` / ``guidance``."""
        if solver is not None:
            S.check_solver_name(solver, "solver")
            if not (fused and isinstance(self.network, DiffusionTransformer)):
                raise NotImplementedError("solver needs the fused path of the HIP network (RFSampler.sample_hip)")
            if self.sp is not None and self.sp.size > 1:
                raise NotImplementedError("solver runs on a single rank only: the sequence-parallel calls have no solver form")
            if step_cache is not None or guidance is not None:
                raise NotImplementedError("solver together with step_cache or guidance is out of scope: the solver's pass takes the pair "
                                          "[v_u; v_c] of a full step (composition is the natural follow-up)")
        if guidance is not None:
            if not (fused and isinstance(self.network, DiffusionTransformer)):
                raise NotImplementedError("guidance needs the fused path of the HIP network (RFSampler.sample_hip)")
            if self.sp is not None and self.sp.size > 1:
                raise NotImplementedError("guidance runs on a single rank only: the sequence-parallel calls have no guided form")
            if tile_indices is not None:
                raise NotImplementedError("guidance with temporal tiles (tile_indices, RFSamplerLong) is out of scope: the tiled loops keep no delta per tile")
        if step_cache is not None:
            if not (fused and isinstance(self.network, DiffusionTransformer)):
                raise NotImplementedError("step_cache needs the fused path of the HIP network (RFSampler.sample_hip)")
            if self.sp is not None and self.sp.size > 1:
                raise NotImplementedError("step_cache runs on a single rank only: the sequence-parallel calls have no cached form")
        randn = torch.randn(batch_size, *shape, generator=generator).to(torch.float32).to(self.device)
        if prefix is not None:
            randn = torch.cat([prefix, randn[:, prefix.shape[1]:]], dim=1)
        chunk_dim = None
        sp = self.sp if (self.sp is not None and self.sp.size > 1) else None
        uc = cond if uc is None else uc
        if sp is not None:
            sp.broadcast(randn)
            h, w = shape[-2:]
            chunk_dim = 3 if h < w else 4
            randn = sp.chunk(randn, chunk_dim)
            cond, uc = dict(cond), dict(uc)
            for k in ("concat_images", "ref_concat", "concat_pose", "concat_smpl_render"):
                if k in cond and cond[k].dim() > chunk_dim:                # a placeholder concat_images (never read) has no such axis
                    cond[k] = sp.chunk(cond[k], chunk_dim)
                    uc[k] = sp.chunk(uc[k], chunk_dim)
            if "smpl_tiled" in cond:                                       # one more leading (tile) axis, :518-524
                cond["smpl_tiled"] = sp.chunk(cond["smpl_tiled"], chunk_dim + 1)
                uc["smpl_tiled"] = sp.chunk(uc["smpl_tiled"], chunk_dim + 1)
        extra = {} if tile_indices is None else {"tile_indices": tile_indices}     # RFSamplerLong, :564-569
        if tile_indices is not None and not isinstance(self.sampler, S.RFSamplerLong):
            raise TypeError("tile_indices needs sampler_config.target = RFSamplerLong")
        if step_cache is not None:
            extra["step_cache"] = step_cache
        if guidance is not None:
            extra["guidance"] = guidance
        if solver is not None:
            extra["solver"] = solver
        if fused and isinstance(self.network, DiffusionTransformer):
            samples = self.sampler.sample_hip(self.network, randn, cond, uc, num_steps=num_steps, chunk_dim=chunk_dim, **extra)
        else:
            denoiser = lambda inp, sigma, c, **kw: self.denoiser(self.model, inp, sigma, c, concat_images=concat_images,
                                                                  chunk_dim=chunk_dim, **kw)
            samples = self.sampler(denoiser, randn, dict(cond), uc=dict(uc), num_steps=num_steps, **extra)
        samples = samples.to(self.dtype)
        if sp is not None:
            samples = sp.gather_to_rank0(samples, chunk_dim)
        return samples

    @torch.no_grad()
    def calibrate_fp8(self, cond: Dict, uc: Optional[Dict], shape, max_rel_err: float, num_steps: Optional[int] = None, seed: int = 0):
        """Per-layer fp8 selection for one request (an extension; scail_amd.dit.DiffusionTransformer.fp8_probe / choose_fp8_layers): the
        sampler's first network evaluation -- first sigma, the CFG batch [uncond; cond], ``cond`` / ``uc`` as for ``sample`` -- runs once
        through the executor's probe, and every (layer, GEMM) whose fp8 result is further than ``max_rel_err`` (relative, Frobenius) from
        its bf16 twin stays in bf16 from then on.  shape = (T, C, H, W); the noise comes from a generator of its own (``seed``), so the
        request's random stream is not consumed.  With ``smpl_tiled`` in ``cond`` (temporal tiles) the first window is probed.
        Returns dict(rel_err (layers, 6), worst (layers, 6), masks [layers], enabled = the quantised mask, scaling = the network's fp8_scaling, which the probe measured); columns in lib.FP8_GEMMS order;
        precision = "fp8" | "fp6", the quantised form the probe measured (the call works under either)."""
        from .dit import choose_fp8_layers
        net = self.network
        if self.sp is not None and self.sp.size > 1:
            raise NotImplementedError("calibrate_fp8: the fp8 GEMMs run on a single rank only")
        if not getattr(net, "fp8_mask", 0):
            raise ValueError("calibrate_fp8 needs a network built with gemm_precision='fp8'")
        uc = cond if uc is None else uc
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(1, *shape, generator=g).to(torch.float32).to(self.device)
        shared = {k: v for k, v in cond.items() if k not in ("crossattn", "smpl_tiled")}
        if "smpl_tiled" in cond:                                           # RFSamplerLong: the first temporal window and its pose tile
            shared["concat_smpl_render"] = cond["smpl_tiled"][:, 0]
            x = x[:, :cond["smpl_tiled"].shape[2]].contiguous()
        t = (self.sampler.sigmas(num_steps)[0] * 1000.0).repeat(2).to(self.device)        # c_noise = 1000 sigma (RFScaling)
        ctx = torch.cat((uc["crossattn"], cond["crossattn"]), 0)
        rel, worst = net.fp8_probe(torch.cat([x, x], 0), t, ctx, None, cond_key=("sample_hip", id(cond)), cfg_pair=True, **shared)
        masks = choose_fp8_layers(rel, max_rel_err, net.fp8_mask)
        net.select_fp8_layers(masks)
        return dict(rel_err=rel, worst=worst, masks=masks, enabled=net.fp8_mask, scaling=getattr(net, "fp8_scaling", "row"),
                    precision=getattr(net, "gemm_precision", "fp8"))

    @torch.no_grad()
    def decode_first_stage(self, z, chunk_frames=None):
        """diffusion_video.py:298-309.  ``chunk_frames`` (an extension): the VAE's streamed decode, WanVAE_.decode."""
        if self.first_stage_model is None:
            raise RuntimeError("first stage (VAE) not built; pass build_first_stage: true in the model config")
        if chunk_frames is None:
            return self.first_stage_model.decode(1.0 / self.scale_factor * z)
        return self.first_stage_model.decode(1.0 / self.scale_factor * z, chunk_frames=chunk_frames)

    @torch.no_grad()
    def decode_first_stage_u8(self, z, chunk_frames=None):
        """``decode_first_stage`` ending in the writers' pixels (an extension): uint8 (B, T, H, W, 3) on the device, WanVAE_.decode_u8."""
        if self.first_stage_model is None:
            raise RuntimeError("first stage (VAE) not built; pass build_first_stage: true in the model config")
        return self.first_stage_model.decode_u8(1.0 / self.scale_factor * z, chunk_frames=chunk_frames)

    @torch.no_grad()
    def encode_first_stage(self, x, batch=None, force_encode=False):
        """diffusion_video.py:311-331."""
        if not force_encode and self.latent_input:
            return x * self.scale_factor
        if self.first_stage_model is None:
            raise RuntimeError("first stage (VAE) not built; pass build_first_stage: true in the model config")
        z = self.scale_factor * self.first_stage_model.encode(x)
        if self.sp is not None and self.sp.size > 1:
            self.sp.broadcast(z)
        return z
