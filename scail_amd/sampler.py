"""sgm sampler stack for the SCAIL hot path, mirrored class-for-class so the reference's yaml
``target:`` strings can be pointed here (seam between L5 engine and L3 DiT).

  RFSampler          sgm/modules/diffusionmodules/sampling.py:920-982 (+ make_flow_timesteps :888-903)
  RFSamplerLong      sampling.py:986-1085 (temporal tiling for videos longer than the trained window)
  Denoiser/RFScaling sgm/modules/diffusionmodules/denoiser.py:9-43, denoiser_scaling.py:71-78
  VanillaCFG         sgm/modules/diffusionmodules/guiders.py:23-57 (+ sampling_utils.py:7-10)
  OpenAIWrapper      sgm/modules/diffusionmodules/wrappers.py:24-45

The generic path keeps the reference call protocol (``sampler(denoiser, x, cond, uc)``,
``denoiser(network, input, sigma, cond, **kw)``, ``network(x, t, c, **kw)``) and works with any
network.  When the network is a ``scail_amd.dit.DiffusionTransformer`` the sampler step uses the
fused HIP kernel for CFG-combine + Euler update (``scail_cfg_euler``) on the fp32 state instead of
four elementwise torch ops; the arithmetic is the same fp32 expression.
"""
from __future__ import annotations

import math
from typing import Dict

import numpy as np
import torch
from torch import nn

from . import ops


def append_dims(x: torch.Tensor, target_dims: int) -> torch.Tensor:
    """sgm/util.py:292 -- append trailing singleton dims."""
    return x[(...,) + (None,) * (target_dims - x.ndim)]


def make_flow_timesteps(t_start, num_flow_steps, verbose=False, shift_scale=7, mode="normal"):
    """sampling.py:888-903: linspace in float64, hunyuan shift, float32, 1 - s for mode 'normal'."""
    s = np.linspace(t_start, 1.0, num_flow_steps + 1, endpoint=True)
    s = s / (shift_scale + s - shift_scale * s)
    s = torch.tensor(s, dtype=torch.float32)
    if mode == "normal":
        s = 1 - s
    elif mode != "meta":
        raise ValueError(f"Unknown mode {mode}.")
    if verbose:
        print(f"Selected timesteps for flow sampler: {s}")
    return s


class RFScaling:
    """denoiser_scaling.py:71-78."""

    def __call__(self, sigma, **additional_model_inputs):
        return torch.zeros_like(sigma), torch.ones_like(sigma), torch.ones_like(sigma), sigma.clone() * 1000


class EpsWeighting:
    """denoiser_weighting.py (training only; kept so denoiser_config instantiates)."""

    def __call__(self, sigma):
        return sigma ** -2.0


class Denoiser(nn.Module):
    """denoiser.py:9-43 with scaling_config resolved to RFScaling by default."""

    def __init__(self, weighting_config=None, scaling_config=None):
        super().__init__()
        from .config import instantiate_from_config
        self.weighting = instantiate_from_config(weighting_config) if weighting_config else EpsWeighting()
        self.scaling = instantiate_from_config(scaling_config) if scaling_config else RFScaling()

    def forward(self, network, input, sigma, cond: Dict, **additional_model_inputs):
        sigma_shape = sigma.shape
        sigma = append_dims(sigma, input.ndim)
        c_skip, c_out, c_in, c_noise = self.scaling(sigma, **additional_model_inputs)
        c_noise = c_noise.reshape(sigma_shape)
        model_output = network(input * c_in, c_noise, cond, **additional_model_inputs)
        return model_output * c_out + input * c_skip


class NoDynamicThresholding:
    """sampling_utils.py:7-10."""

    def __call__(self, uncond, cond, scale):
        scale = append_dims(scale, cond.ndim) if isinstance(scale, torch.Tensor) else scale
        return uncond + scale * (cond - uncond)


class VanillaCFG:
    """guiders.py:23-57: batch-2 (uncond, cond) assembly and u + s (c - u)."""

    def __init__(self, scale, dyn_thresh_config=None):
        self.scale = scale
        self.dyn_thresh = NoDynamicThresholding()

    def __call__(self, x, sigma, scale=None):
        x_u, x_c = x.chunk(2)
        return self.dyn_thresh(x_u, x_c, self.scale if scale is None else scale)

    def prepare_inputs(self, x, s, c, uc):
        c_out = dict()
        for k in c:
            if k in ["vector", "crossattn", "concat"]:
                if uc[k].shape[1] != c[k].shape[1]:
                    uc[k] = torch.cat([uc[k], uc[k][:, -1:].repeat(1, abs(c[k].shape[1] - uc[k].shape[1]), 1)], dim=1)
                c_out[k] = torch.cat((uc[k], c[k]), 0)
            else:
                c_out[k] = c[k]
        # the batch below is ONE latent and ONE sigma twice: scail_amd's network evaluates layer 0 up to its first cross attention once
        # (include/scail_dit.h SCAIL_DIT_CFG_PAIR; result-preserving).  A plain bool: other networks ignore the key.
        c_out["cfg_pair"] = True
        return torch.cat([x] * 2), torch.cat([s] * 2), c_out


class OpenAIWrapper(nn.Module):
    """wrappers.py:24-45 (IdentityWrapper + OpenAIWrapper)."""

    def __init__(self, diffusion_model, compile_model: bool = False, dtype=torch.float32, **kwargs):
        super().__init__()
        self.diffusion_model = diffusion_model
        self.dtype = dtype

    def forward(self, x, t, c: dict, **kwargs):
        for key in c:
            if torch.is_tensor(c[key]):
                c[key] = c[key].to(self.dtype)
        kwargs.update(c)
        if "concat" in c:
            x = torch.cat((x, c["concat"]), dim=2 if x.dim() == 5 else 1)
        return self.diffusion_model(x, timesteps=t, context=c.get("crossattn", None), y=c.get("vector", None), **kwargs)


class RFDiscretization:
    """discretizer.py:131-180 is bypassed by hunyuan_schedule=True in the shipped config
    (sampling.py:941-942); kept as a named target so sampler_config instantiates."""

    def __init__(self, reverse=False, **kw):
        self.reverse = reverse


def _executor_takes_loop(network) -> bool:
    """Whether the network runs a whole sampler loop in one executor call (DiffusionTransformer.executor_ok); a network without that
    method takes the generic loop"""
    return getattr(network, "executor_ok", lambda **kw: False)(whole_loop=True)


def plan_step_cache(dist, threshold, coefficients=(1.0, 0.0), keep_first=1, keep_last=1):
    """The step cache's plan (include/scail_dit.h "step cache"): one 0 (compute) / 1 (reuse the block residual of the last computed step)
    per sampler step, from the table ``dist`` of DiffusionTransformer.time_distances -- n rows (sum |v_i - v_{i-1}|, sum |v_{i-1}|).
    Pure host fp64; needs no device.

      d_i = dist[i][0] / dist[i][1]                       (a zero denominator: step i computes)
      acc += polynomial(d_i)                              (``coefficients`` highest degree first, Horner; (1, 0) is the identity)
      step i computes and resets acc when i < keep_first, i >= n - keep_last, or acc >= threshold; otherwise it reuses.

    Step 0 always computes (keep_first >= 1): it has nothing to reuse.  threshold 0 gives all zeros.  Example: d_i = 0.125 for
    i = 1..5, threshold 0.3, n = 6 -> [0, 1, 1, 0, 1, 0]."""
    rows = [(float(r[0]), float(r[1])) for r in dist]
    n = len(rows)
    threshold = float(threshold)
    coefficients = [float(c) for c in coefficients]
    if not threshold >= 0.0:
        raise ValueError(f"plan_step_cache: threshold must be >= 0, got {threshold}")
    if not coefficients or not all(np.isfinite(c) for c in coefficients):
        raise ValueError(f"plan_step_cache: coefficients must be a non-empty list of finite numbers, got {coefficients}")
    if int(keep_first) != keep_first or keep_first < 1:
        raise ValueError(f"plan_step_cache: keep_first must be an integer >= 1 (step 0 has nothing to reuse), got {keep_first}")
    if int(keep_last) != keep_last or keep_last < 0:
        raise ValueError(f"plan_step_cache: keep_last must be an integer >= 0, got {keep_last}")
    if any(not (np.isfinite(a) and np.isfinite(b)) or a < 0 or b < 0 for a, b in rows):
        raise ValueError("plan_step_cache: dist must hold finite, non-negative sums")
    mask, acc = [], 0.0
    for i, (num, den) in enumerate(rows):
        if i < keep_first or i >= n - keep_last or den == 0.0:
            mask.append(0)
            acc = 0.0
            continue
        p = 0.0
        for c in coefficients:
            p = p * (num / den) + c
        acc += p
        if acc < threshold:
            mask.append(1)
        else:
            mask.append(0)
            acc = 0.0
    return mask


GUIDE_PAIR, GUIDE_DELTA, GUIDE_COND = 0, 1, 2          # include/scail_dit.h SCAIL_DIT_GUIDE_*
GUIDANCE_KEYS = ("interval", "every", "modes")


def check_guidance_plan(guide, reuse=None, what="guidance plan"):
    """The rules scail_dit_sample_guided checks a plan by (include/scail_dit.h "guidance plan"), on the host: entries 0 / 1 / 2; a DELTA entry
    has a PAIR entry before it; with a step-cache mask ``reuse`` (0 / 1 entries, reuse[0] == 0) a reusing step evaluates the same elements
    as the last computing step (PAIR with PAIR, DELTA or COND with DELTA or COND).  Raises ValueError naming the index; returns the plan
    as a list of ints."""
    guide = [int(v) for v in guide]
    seen_pair = False
    for i, g in enumerate(guide):
        if g not in (GUIDE_PAIR, GUIDE_DELTA, GUIDE_COND):
            raise ValueError(f"{what}: entry {i} is {g} (an entry is 0 = pair, 1 = delta or 2 = cond)")
        if g == GUIDE_DELTA and not seen_pair:
            raise ValueError(f"{what}: entry {i} is 1 (delta) with no pair step before it: there is no stored delta to use")
        seen_pair = seen_pair or g == GUIDE_PAIR
    if reuse is not None:
        reuse = [int(v) for v in reuse]
        if len(reuse) != len(guide):
            raise ValueError(f"{what}: the reuse mask needs one entry per step ({len(guide)}), got {len(reuse)}")
        if any(v not in (0, 1) for v in reuse) or (reuse and reuse[0] != 0):
            raise ValueError(f"{what}: the reuse mask holds 0 / 1 entries and starts with 0 (the first step has nothing to reuse), got {reuse}")
        j = 0
        for i, r in enumerate(reuse):
            if not r:
                j = i
            elif (guide[i] == GUIDE_PAIR) != (guide[j] == GUIDE_PAIR):
                raise ValueError(f"{what}: step {i} reuses (entry {guide[i]}) what step {j}, the last computing step, left (entry {guide[j]}): "
                                 "they do not evaluate the same elements")
    return guide


def plan_guidance(sigmas, interval=None, every=1, modes=None):
    """The guidance plan (include/scail_dit.h "guidance plan"): one entry per sampler step -- 0 = the batch-2 pair (guided; stores
    v_c - v_u), 1 = the cond branch alone with the stored delta, 2 = the cond branch alone, no guidance.  Pure host; needs no device.

    ``sigmas``: the STARTING sigma of every step, one value per step (``RFSampler.sigmas()[:-1]``).  ``interval`` = (lo, hi): step i is
    inside when lo <= sigmas[i] <= hi (None: every step is inside).  Steps outside get 2.  Inside each maximal run of inside steps,
    position p gets 0 when p % every == 0, else 1.  Example: 10 steps, the interval covering steps 2..7, every = 3 ->
    [2, 2, 0, 1, 1, 0, 1, 1, 2, 2].  Explicit ``modes`` stand alone (no interval, every left at 1) and are checked as the library checks them
    (check_guidance_plan).  No default interval or ``every`` is recommended: nothing has been measured on real weights."""
    sig = [float(v) for v in sigmas]
    n = len(sig)
    if modes is not None:
        if interval is not None or every != 1:
            raise ValueError("plan_guidance: explicit 'modes' stand alone (interval and every make a plan from the schedule)")
        modes = check_guidance_plan(modes, what="plan_guidance: modes")
        if len(modes) != n:
            raise ValueError(f"plan_guidance: 'modes' needs one entry per step ({n}), got {len(modes)}")
        return modes
    if isinstance(every, bool) or int(every) != every or every < 1:
        raise ValueError(f"plan_guidance: every must be an integer >= 1, got {every!r}")
    every = int(every)
    lo, hi = -np.inf, np.inf
    if interval is not None:
        if len(interval) != 2:
            raise ValueError(f"plan_guidance: interval is (lo, hi), got {interval!r}")
        lo, hi = float(interval[0]), float(interval[1])
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError(f"plan_guidance: the interval's bounds must be finite, got ({lo}, {hi})")
        if lo > hi:
            raise ValueError(f"plan_guidance: the interval needs lo <= hi, got ({lo}, {hi})")
    plan, p = [], 0
    for v in sig:
        if lo <= v <= hi:
            plan.append(GUIDE_PAIR if p % every == 0 else GUIDE_DELTA)
            p += 1
        else:
            plan.append(GUIDE_COND)
            p = 0
    return plan


def merge_guidance_with_step_cache(guide, reuse):
    """A guidance plan made to agree with a step-cache plan ``reuse`` (plan_step_cache): a reusing step takes the entry of the last computing
    step, since it must find the residual slots that step filled.  A computing DELTA step whose PAIR steps were all replaced that way
    becomes a PAIR step: it has no stored delta to use.  The result always passes check_guidance_plan(result, reuse).  Both inputs are
    checked first (the guide on its own, the mask for 0 / 1 entries starting with 0)."""
    guide = check_guidance_plan(guide, what="merge_guidance_with_step_cache: guide")
    reuse = [int(v) for v in reuse]
    if len(reuse) != len(guide):
        raise ValueError(f"merge_guidance_with_step_cache: the reuse mask needs one entry per step ({len(guide)}), got {len(reuse)}")
    if any(v not in (0, 1) for v in reuse) or (reuse and reuse[0] != 0):
        raise ValueError(f"merge_guidance_with_step_cache: the reuse mask holds 0 / 1 entries and starts with 0, got {reuse}")
    out, j, seen_pair = [], 0, False
    for i, r in enumerate(reuse):
        if r:
            g = out[j]
        else:
            j, g = i, guide[i]
            if g == GUIDE_DELTA and not seen_pair:
                g = GUIDE_PAIR
        seen_pair = seen_pair or g == GUIDE_PAIR
        out.append(g)
    return out


SOLVERS = ("dpmpp2m", "dpm1")


def check_solver_name(solver, what="plan_solver"):
    if solver not in SOLVERS:
        raise ValueError(f"{what}: unknown solver {solver!r} (one of {SOLVERS}; None is the Euler loop)")
    return solver


def plan_solver(sigmas, solver):
    """The solver plan (include/scail_dit.h "solver plan"): one (a, b, c) per sampler step, x_{i+1} = a x_i + b D_i + c D_{i-1} with the
    data prediction D_i = x_i - sigma_i d_i.  Pure host, fp64 (Python floats) from the host fp32 schedule; needs no device.

    ``sigmas``: the whole schedule, n_steps + 1 values from the first step's starting sigma to the last step's end (``RFSampler.sigmas()``).
    ``solver``: "dpmpp2m" = DPM-Solver++(2M), or "dpm1" = its first-order rows everywhere (for tests and A/B).  With rho =
    sigma_{i+1} / sigma_i a first-order row is (rho, 1 - rho, 0) -- Euler mathematically, not in bits -- and a second-order row
    (rho, (1 - rho)(1 + 1 / (2 r_i)), -(1 - rho) / (2 r_i)), r_i = h_{i-1} / h_i, h_i = lambda_{i+1} - lambda_i, lambda = log((1 - sigma) /
    sigma).  A step is second order only where i >= 1 and lambda_{i-1}, lambda_i, lambda_{i+1} are finite, so a schedule from 1 to 0 has
    steps 0, 1 and the last one first order, and its last row is (0, 1, 0).  a + b + c = 1.
    Refused by name: an unknown solver, fewer than 2 sigmas, a sigma outside [0, 1], a sigma of 0 anywhere but last, a schedule that is
    not strictly decreasing."""
    check_solver_name(solver)
    sig = [float(v) for v in (sigmas.tolist() if torch.is_tensor(sigmas) else sigmas)]
    if len(sig) < 2:
        raise ValueError(f"plan_solver: a schedule has at least 2 sigmas (one step), got {len(sig)}")
    for i, v in enumerate(sig):
        if not 0.0 <= v <= 1.0:
            raise ValueError(f"plan_solver: sigma[{i}] = {v} lies outside [0, 1]")
    for i, v in enumerate(sig[:-1]):
        if v == 0.0:
            raise ValueError(f"plan_solver: sigma[{i}] = 0 is not the last value: a step cannot start at sigma = 0")
    for i in range(len(sig) - 1):
        if not sig[i + 1] < sig[i]:
            raise ValueError(f"plan_solver: the schedule must be strictly decreasing, got sigma[{i}] = {sig[i]} then sigma[{i + 1}] = {sig[i + 1]}")
    lam = [math.log((1.0 - v) / v) if 0.0 < v < 1.0 else (-math.inf if v == 1.0 else math.inf) for v in sig]
    rows = []
    for i in range(len(sig) - 1):
        rho = sig[i + 1] / sig[i]
        if solver == "dpmpp2m" and i >= 1 and all(math.isfinite(lam[j]) for j in (i - 1, i, i + 1)):
            r = (lam[i] - lam[i - 1]) / (lam[i + 1] - lam[i])
            c = -(1.0 - rho) / (2.0 * r)
            rows.append((rho, (1.0 - rho) - c, c))
        else:
            rows.append((rho, 1.0 - rho, 0.0))
    return rows


def solver_uses_prev(row) -> bool:
    """Whether a row of a solver plan reads the history, as the library decides it: its c, rounded to fp32, is not zero"""
    return float(np.float32(row[2])) != 0.0


def _solver_alone(solver, step_cache, guidance, chunk_dim):
    """The refusals of a ``solver`` option that RFSampler.sample_hip and RFSamplerLong.sample_hip share, before the network is touched"""
    check_solver_name(solver, "solver")
    if step_cache is not None:
        raise NotImplementedError("solver together with step_cache is out of scope: the solver's pass takes the pair [v_u; v_c] of a full step "
                                  "(composition is the natural follow-up); drop one of the two")
    if guidance is not None:
        raise NotImplementedError("solver together with guidance is out of scope: the solver's pass takes the pair [v_u; v_c], a cond-only step has "
                                  "v_c and a stored delta (composition is the natural follow-up); drop one of the two")
    if chunk_dim is not None:
        raise NotImplementedError("solver runs on a single rank only: not on sequence-parallel ranks (chunk_dim)")


STEP_CACHE_KEYS = ("threshold", "coefficients", "keep_first", "keep_last", "signal", "mask")


class RFSampler:
    """sampling.py:920-982.  Only the shipped branch (hunyuan_schedule) is implemented.

    One deliberate difference: a ``num_steps`` ARGUMENT (``__call__`` / ``sample_hip`` / ``engine.sample``) overrides the configured
    step count here.  In the reference the argument only reaches the discretization, whose result the hunyuan schedule then
    replaces with ``make_flow_timesteps(0, self.num_steps, ...)`` (:936-942) -- i.e. it is silently ignored; the reference's own
    engine never passes it (diffusion_video.py:565-569).  Leave it ``None`` for the reference's behaviour."""

    def __init__(self, schedule_shift=False, hunyuan_schedule=False, shift_scale=7, mode="normal", distill=False,
                 discretization_config=None, num_steps=None, guider_config=None, verbose=False, device="cuda"):
        from .config import instantiate_from_config
        if schedule_shift or not hunyuan_schedule or distill:
            raise NotImplementedError("only schedule_shift=False, hunyuan_schedule=True, distill=False (shipped config)")
        self.num_steps, self.shift_scale, self.mode, self.verbose, self.device = num_steps, shift_scale, mode, verbose, device
        self.guider = instantiate_from_config(guider_config) if guider_config else VanillaCFG(1.0)

    def sigmas(self, num_steps=None) -> torch.Tensor:
        return make_flow_timesteps(0, self.num_steps if num_steps is None else num_steps, verbose=False,
                                   shift_scale=self.shift_scale, mode=self.mode)

    def denoise(self, x, denoiser, sigma, cond, uc, scale=None, fps=None):
        """sampling.py:950-958."""
        extra = {"cfg_scale": scale if scale is not None else self.guider.scale}
        denoised = denoiser(*self.guider.prepare_inputs(x, sigma, cond, uc), **extra).to(torch.float32)
        return self.guider(denoised, sigma)

    def sampler_step(self, sigma, next_sigma, denoiser, x, cond, uc=None, scale=None, fps=None):
        """sampling.py:960-963."""
        output = self.denoise(x, denoiser, sigma, cond, uc, scale=scale, fps=fps).to(torch.float32)
        return x + append_dims(next_sigma - sigma, x.ndim) * output

    def __call__(self, denoiser, x, cond, uc=None, num_steps=None, scale=None, ofs=None, fps=None):
        sigmas = self.sigmas(num_steps).to(x.device)
        uc = cond if uc is None else uc
        s_in = x.new_ones([x.shape[0]])
        for i in range(len(sigmas) - 1):
            x = self.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], denoiser, x, cond, uc, scale=scale, fps=fps)
        return x

    # ---- fused path for the HIP network (same arithmetic, fewer passes / no host syncs) ----
    def step_cache_plan(self, network, sig, step_cache) -> list:
        """The 0 / 1 plan of a ``step_cache`` option (sample_hip) for the host schedule ``sig``: its explicit ``mask``, or
        plan_step_cache on the network's time distances (signal "time" | "modulation"; one small device run and one synchronisation,
        before the loop).  The plan depends on the schedule and the weights alone, never on the latent."""
        if not isinstance(step_cache, dict) or not step_cache or any(k not in STEP_CACHE_KEYS for k in step_cache):
            raise ValueError(f"step_cache must be None or a dict with keys out of {STEP_CACHE_KEYS}, got {step_cache!r}")
        n = len(sig) - 1
        if step_cache.get("mask") is not None:
            if len(step_cache) != 1:
                raise ValueError("step_cache: an explicit 'mask' stands alone (the other keys make a plan from a threshold)")
            mask = [int(v) for v in step_cache["mask"]]
            if len(mask) != n or any(v not in (0, 1) for v in mask) or (n > 0 and mask[0] != 0):
                raise ValueError(f"step_cache: 'mask' needs {n} entries of 0 / 1 and mask[0] == 0 (the first step has nothing to reuse), got {mask}")
            return mask
        if "threshold" not in step_cache:
            raise ValueError("step_cache needs a 'threshold' (or an explicit 'mask'); no default is recommended: nothing has been measured on real weights")
        dist = network.time_distances((sig[:-1] * 1000.0), step_cache.get("signal", "time"))
        return plan_step_cache(dist, step_cache["threshold"], step_cache.get("coefficients", (1.0, 0.0)), step_cache.get("keep_first", 1),
                               step_cache.get("keep_last", 1))

    def guidance_plan(self, sig, guidance, reuse=None) -> list:
        """The plan of a ``guidance`` option (sample_hip) for the host schedule ``sig`` (n_steps + 1 values): plan_guidance on the steps'
        starting sigmas, merged with the step cache's plan ``reuse`` when there is one (explicit ``modes`` are not rewritten: they must
        agree with it as they stand)."""
        if not isinstance(guidance, dict) or not guidance or any(k not in GUIDANCE_KEYS for k in guidance):
            raise ValueError(f"guidance must be None or a dict with keys out of {GUIDANCE_KEYS}, got {guidance!r}")
        plan = plan_guidance([float(v) for v in sig[:-1]], guidance.get("interval"), guidance.get("every", 1), guidance.get("modes"))
        if reuse is None:
            return plan
        if guidance.get("modes") is not None:
            return check_guidance_plan(plan, reuse, what="guidance: modes")
        return merge_guidance_with_step_cache(plan, reuse)

    def sample_hip(self, network, x, cond: Dict, uc: Dict, num_steps=None, scale=None, chunk_dim=None,
                   step_callback=None, step_cache=None, guidance=None, solver=None):
        """x (1,T,16,H,W) fp32 on the GPU; cond/uc as the CLI builds them (sample_video.py:455-470).
        One step = one batch-2 DiT forward (uncond, cond) + scail_cfg_euler.
        ``step_cache`` (opt-in, an extension; None = this method as it was): a dict with ``threshold`` and optionally ``coefficients``,
        ``keep_first``, ``keep_last``, ``signal`` (plan_step_cache / step_cache_plan), or an explicit ``mask`` of one 0 / 1 per step.  A step
        planned 1 skips the blocks and adds the block residual of the last computed step to its own embedded tokens
        (include/scail_dit.h "step cache").  Both routes below take the plan and give the same bits.  ``self.last_step_cache_plan`` keeps it.
        ``guidance`` (opt-in, an extension; None = this method as it was): a dict with ``interval`` = (lo, hi) and / or ``every``, or explicit
        ``modes`` (plan_guidance): which steps run the batch-2 pair, which the cond branch alone with the stored v_c - v_u, which the cond
        branch alone without guidance (include/scail_dit.h "guidance plan").  Combines with ``step_cache`` (merge_guidance_with_step_cache).
        Both routes take the plan and give the same bits, provided the conditioning GEMMs compute a row of the cond prompt alone as they
        compute it in the batch of two (they do wherever both sizes take one kernel: scail_gemm_kernel_name_for).
        ``self.last_guidance_plan`` keeps it.
        ``solver`` (opt-in, an extension; None = this method as it was): "dpmpp2m" or "dpm1" (plan_solver): the Euler update is replaced by
        x <- a x + b D + c D_prev in the data prediction D (include/scail_dit.h "solver plan"), with one fp32 latent of history and no
        further network evaluation.  The one call (scail_dit_sample_solver) and the host loop below -- the instrumented route:
        ``step_callback``, SCAIL_C_STEP=0 -- take the same table and give the same bits.  Not together with ``step_cache`` or ``guidance``, not
        on sequence-parallel ranks.  ``self.last_solver_plan`` keeps the table."""
        if solver is not None:
            _solver_alone(solver, step_cache, guidance, chunk_dim)
        sig = self.sigmas(num_steps)                     # host fp32, like the reference
        cfg = float(self.guider.scale if scale is None else scale)
        ctx = torch.cat((uc["crossattn"], cond["crossattn"]), 0)
        shared = {k: v for k, v in cond.items() if k != "crossattn"}
        plan = None
        if step_cache is not None:
            if chunk_dim is not None or not _executor_takes_loop(network):
                raise NotImplementedError("step_cache runs in the C executor on a single rank only: not on sequence-parallel ranks (chunk_dim), not "
                                          "with SCAIL_C_STEP=0, _tap or kernel_timer")
            plan = self.last_step_cache_plan = self.step_cache_plan(network, sig, step_cache)
        gplan = None
        if guidance is not None:
            if chunk_dim is not None or not _executor_takes_loop(network):
                raise NotImplementedError("guidance runs in the C executor on a single rank only: not on sequence-parallel ranks (chunk_dim), not "
                                          "with SCAIL_C_STEP=0, _tap or kernel_timer")
            if x.shape[0] != 1 or shared["ref_concat"].shape[0] != 1 or shared["concat_smpl_render"].shape[0] != 1:
                raise NotImplementedError("guidance takes one latent with one shared ref / pose (the cond branch is a batch-1 evaluation)")
            gplan = self.last_guidance_plan = self.guidance_plan(sig, guidance, plan)
        splan = None
        if solver is not None:
            if x.shape[0] != 1:
                raise NotImplementedError(f"solver takes one latent (the update pass reads one CFG pair), got a batch of {x.shape[0]}")
            splan = self.last_solver_plan = plan_solver(sig, solver)
        if (_executor_takes_loop(network) and step_callback is None and chunk_dim is None
                and shared["ref_concat"].shape[0] == 1 and shared["concat_smpl_render"].shape[0] == 1):
            # the whole loop enqueued by ONE call into the library (scail_dit_sample_chars; any number of reference frames / pose
            # streams); same kernels, same order
            if splan is not None:
                return network.sample_c(x, sig, cfg, ctx, shared["ref_concat"], shared["concat_smpl_render"],
                                        shared["image_clip_features"], cond_key=("sample_hip", id(cond)), solver=(sig[:-1], splan))
            if gplan is not None:
                return network.sample_c(x, sig, cfg, ctx, shared["ref_concat"], shared["concat_smpl_render"],
                                        shared["image_clip_features"], cond_key=("sample_hip", id(cond)), reuse=plan, guide=gplan)
            if plan is not None:
                return network.sample_c(x, sig, cfg, ctx, shared["ref_concat"], shared["concat_smpl_render"],
                                        shared["image_clip_features"], cond_key=("sample_hip", id(cond)), reuse=plan)
            return network.sample_c(x, sig, cfg, ctx, shared["ref_concat"], shared["concat_smpl_render"],
                                    shared["image_clip_features"], cond_key=("sample_hip", id(cond)))
        x = x.float().contiguous().clone()
        delta = torch.empty_like(x) if gplan is not None and any(g != GUIDE_COND for g in gplan) else None
        hist = torch.empty_like(x) if splan is not None else None
        for i in range(len(sig) - 1):
            t = (sig[i] * 1000.0).repeat(2).to(x.device)                 # c_noise = 1000 sigma (RFScaling)
            if plan is not None:
                shared["step_cache"] = "reuse" if plan[i] else "fill"
            if gplan is not None and gplan[i] != GUIDE_PAIR:
                # the cond branch alone: a batch-1 evaluation under the cond prompt (the network keeps ONE conditioning: a change between
                # pair and branch steps computes it again -- this is the instrumented route)
                v = network.forward_f32(x, t[:1], ctx[1:2], None, cond_key=("sample_hip", id(cond), "cond"), chunk_dim=chunk_dim, **shared)
                ops.cfg_euler_delta_(x, v, delta if gplan[i] == GUIDE_DELTA else None, cfg, float(sig[i + 1] - sig[i]))
                if step_callback is not None:
                    step_callback(i, x)
                continue
            xin = torch.cat([x, x], 0)
            v = network.forward_f32(xin, t, ctx, None, cond_key=("sample_hip", id(cond)), chunk_dim=chunk_dim, **shared)
            if gplan is not None:
                ops.cfg_delta_store(v, out=delta)
            if splan is not None:
                ops.cfg_multistep_(x, v, hist, cfg, float(sig[i]), *splan[i], use_prev=solver_uses_prev(splan[i]))
                if step_callback is not None:
                    step_callback(i, x)
                continue
            ops.cfg_euler_(x, v, cfg, float(sig[i + 1] - sig[i]))
            if step_callback is not None:
                step_callback(i, x)
        return x


class RFSamplerLong(RFSampler):
    """sampling.py:986-1085: every step denoises overlapping temporal tiles of the latent (``tile_indices``: lists of
    frame indices, equal length) against the matching pose tile ``cond['smpl_tiled'][:, k]`` and blends the
    CFG-combined predictions with triangular weights before one Euler update of the whole latent.

    The reference walks the pairs (k, k+1) and therefore denoises every interior tile twice with identical inputs;
    here each tile is evaluated once and enters the weighted sums with the same multiplicity (x2 is exact in
    floating point), which halves the network evaluations for long videos.  Needs >= 2 tiles like the reference
    (a single tile leaves its weight_sum at zero)."""

    @staticmethod
    def tile_weight(n: int, device=None) -> torch.Tensor:
        w = (torch.arange(n, device=device, dtype=torch.float32) + 0.5) * 2.0 / n
        return torch.minimum(w, 2.0 - w)

    @staticmethod
    def _mult(k: int, n: int) -> int:
        return 1 if (k == 0 or k == n - 1) else 2

    @staticmethod
    def _check(tile_indices):
        if tile_indices is None or len(tile_indices) < 2:
            raise ValueError("RFSamplerLong needs tile_indices with at least two temporal tiles")
        n0 = len(tile_indices[0])
        if any(len(t) != n0 for t in tile_indices):
            raise ValueError("all temporal tiles must have the same length")

    ONE_CALL_MAX_TILE = 64        # include/scail_dit.h scail_dit_sample_tiled: a tile's indices and weights travel in kernel arguments

    @classmethod
    def _one_call_ok(cls, network, x, ref_concat, smpl_tiled, tile_indices, step_callback, chunk_dim) -> bool:
        """Whether a request takes scail_dit_sample_tiled: RFSampler's conditions for its one-call route (C step on, no callback, no
        chunk_dim, no timer / tap, one rank, batch 1) AND what that entry point covers -- one character, tiles of at most 64 latent
        frames, one pose tile of Tt frames per tile.  Every other request keeps the Python loop below (several characters with
        tiles, longer tiles, sequence-parallel ranks, instrumented runs)."""
        Tt = len(tile_indices[0])
        return bool(_executor_takes_loop(network) and step_callback is None and chunk_dim is None
                    and x.shape[0] == 1 and ref_concat.shape[0] == 1 and ref_concat.shape[1] == 1
                    and smpl_tiled.dim() == 6 and smpl_tiled.shape[0] == 1 and smpl_tiled.shape[1] == len(tile_indices)
                    and smpl_tiled.shape[2] == Tt and Tt <= cls.ONE_CALL_MAX_TILE and Tt <= x.shape[1] < (1 << 15))

    def sampler_step(self, sigma, next_sigma, denoiser, x, cond, uc=None, scale=None, fps=None, tile_indices=None,
                     smpl_tiled=None):
        """sampling.py:1036-1068 (generic protocol: any denoiser / network)."""
        self._check(tile_indices)
        n = len(tile_indices)
        denoised = torch.zeros_like(x)
        weight_sum = torch.zeros((x.shape[1],), device=x.device)
        weight = self.tile_weight(len(tile_indices[0]), x.device)
        for k in range(n):
            idx = list(tile_indices[k])
            c_k, uc_k = dict(cond), dict(uc)
            c_k["concat_smpl_render"] = smpl_tiled[:, k]
            uc_k["concat_smpl_render"] = smpl_tiled[:, k]
            d = self.denoise(x[:, idx], denoiser, sigma, c_k, uc_k, scale=scale, fps=fps).to(torch.float32)
            m = self._mult(k, n)
            denoised[:, idx] += m * d * weight[:, None, None, None]
            weight_sum[idx] += m * weight
        denoised.div_(weight_sum[:, None, None, None])
        return x + append_dims(next_sigma - sigma, x.ndim) * denoised

    def __call__(self, denoiser, x, cond, uc=None, num_steps=None, scale=None, ofs=None, fps=None, tile_indices=None):
        sigmas = self.sigmas(num_steps).to(x.device)
        uc = cond if uc is None else uc
        s_in = x.new_ones([x.shape[0]])
        smpl_tiled = cond["smpl_tiled"]
        for i in range(len(sigmas) - 1):
            x = self.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], denoiser, x, cond, uc, scale=scale, fps=fps,
                                  tile_indices=tile_indices, smpl_tiled=smpl_tiled)
        return x

    def _tile_table(self, tile_indices, T, dev):
        """(frame index tensors, tile_w (n_tiles, Tt) = m_k * tile_weight, inv_wsum (T) = 1 / the per-frame sums of tile_w) for both
        routes of sample_hip, formed on the latent's device: torch divides by a host scalar differently on the two devices, and the
        one-call route has to hand the library the bits the loop below multiplies by."""
        n = len(tile_indices)
        weight = self.tile_weight(len(tile_indices[0]), dev)
        idxs = [torch.as_tensor(list(t), device=dev, dtype=torch.long) for t in tile_indices]
        tile_w = torch.stack([self._mult(k, n) * weight for k in range(n)])
        wsum = torch.zeros(T, device=dev)
        for k in range(n):
            wsum[idxs[k]] += tile_w[k]
        return idxs, tile_w, 1.0 / wsum

    def sample_hip(self, network, x, cond: Dict, uc: Dict, num_steps=None, scale=None, chunk_dim=None,
                   step_callback=None, tile_indices=None, step_cache=None, guidance=None, solver=None):
        """Fused path for the HIP network: per step and tile one batch-2 DiT forward (fp32 out); the text / CLIP
        conditioning (step- AND tile-invariant) is computed once per request.
        ``step_cache`` (opt-in; None = this method as it was): RFSampler.sample_hip's option.  One plan for every tile -- it depends on the
        schedule and the weights alone -- and one block residual per tile (scail_dit_sample_tiled_cached).  Only requests that take the
        one-call route below have a cached form (``_one_call_ok``); every other one is refused before the network is touched: there is no
        cached host loop.  ``self.last_step_cache_plan`` keeps the plan.
        ``solver`` (opt-in; None = this method as it was): RFSampler.sample_hip's option.  The update happens once per step on the whole
        latent, after the blend, so one history serves every tile (scail_dit_sample_tiled_solver; the host loop below takes the same table
        through ops.tile_finish_multistep_ and gives the same bits).  ``self.last_solver_plan`` keeps the table."""
        self._check(tile_indices)
        if solver is not None:
            _solver_alone(solver, step_cache, guidance, chunk_dim)
        if guidance is not None:
            raise NotImplementedError("guidance with temporal tiles (RFSamplerLong) is out of scope: the tiled loops (scail_dit_sample_tiled*) keep "
                                      "no delta per tile; sample the clip in one window or drop the option")
        smpl_tiled = cond.get("smpl_tiled")
        if step_cache is not None:
            ref = cond.get("ref_concat")
            if not (torch.is_tensor(smpl_tiled) and torch.is_tensor(ref)
                    and self._one_call_ok(network, x, ref, smpl_tiled, tile_indices, step_callback, chunk_dim)):
                raise NotImplementedError("step_cache with temporal tiles (RFSamplerLong) runs in the one-call tiled loop of the C executor only "
                                          "(scail_dit_sample_tiled_cached): one rank, no chunk_dim, no step_callback, not with SCAIL_C_STEP=0, _tap or "
                                          "kernel_timer, one character, tiles of at most 64 latent frames and smpl_tiled of shape "
                                          "(1, n_tiles, Tt, 16, H/2, W/2); the host loop has no cached form")
        n = len(tile_indices)
        sig = self.sigmas(num_steps)
        cfg = float(self.guider.scale if scale is None else scale)
        ctx = torch.cat((uc["crossattn"], cond["crossattn"]), 0)
        shared = {k: v for k, v in cond.items() if k not in ("crossattn", "smpl_tiled", "concat_smpl_render")}
        smpl_tiled = cond["smpl_tiled"]
        plan = None
        if step_cache is not None:
            plan = self.last_step_cache_plan = self.step_cache_plan(network, sig, step_cache)
        splan = None
        if solver is not None:
            if x.shape[0] != 1:
                raise NotImplementedError(f"solver takes one latent, got a batch of {x.shape[0]}")
            splan = self.last_solver_plan = plan_solver(sig, solver)
        idxs, tile_w, inv_wsum = self._tile_table(tile_indices, x.shape[1], x.device)
        if self._one_call_ok(network, x, shared["ref_concat"], smpl_tiled, tile_indices, step_callback, chunk_dim):
            # the whole loop enqueued by ONE call into the library (scail_dit_sample_tiled): same network kernels, the gather / blend /
            # Euler arithmetic below as HIP row kernels that round every operation on its own -- the same bits.  The weights are handed
            # over as host values once per request.
            if splan is not None:
                return network.sample_tiled_c(x, sig, cfg, ctx, shared["ref_concat"], smpl_tiled, shared["image_clip_features"],
                                              [list(map(int, t)) for t in tile_indices], tile_w.cpu(), inv_wsum.cpu(),
                                              cond_key=("sample_hip", id(cond)), solver=(sig[:-1], splan))
            if plan is not None:
                return network.sample_tiled_c(x, sig, cfg, ctx, shared["ref_concat"], smpl_tiled, shared["image_clip_features"],
                                              [list(map(int, t)) for t in tile_indices], tile_w.cpu(), inv_wsum.cpu(),
                                              cond_key=("sample_hip", id(cond)), reuse=plan)
            return network.sample_tiled_c(x, sig, cfg, ctx, shared["ref_concat"], smpl_tiled, shared["image_clip_features"],
                                          [list(map(int, t)) for t in tile_indices], tile_w.cpu(), inv_wsum.cpu(),
                                          cond_key=("sample_hip", id(cond)))
        x = x.float().contiguous().clone()
        dev = x.device
        hist, inv_host = (torch.empty_like(x), inv_wsum.cpu()) if splan is not None else (None, None)
        tile_w, inv = tile_w[:, :, None, None, None], inv_wsum[:, None, None, None]
        for i in range(len(sig) - 1):
            t = (sig[i] * 1000.0).repeat(2).to(dev)
            den = torch.zeros_like(x)
            for k in range(n):
                xt = x[:, idxs[k]]
                v = network.forward_f32(torch.cat([xt, xt], 0), t, ctx, None, cond_key=("sample_hip", id(cond)),
                                        chunk_dim=chunk_dim, concat_smpl_render=smpl_tiled[:, k], **shared)
                d = v[0:1] + cfg * (v[1:2] - v[0:1])                     # VanillaCFG, guiders.py:41-45
                den[:, idxs[k]] += tile_w[k] * d
            if splan is not None:
                ops.tile_finish_multistep_(x, den, inv_host, hist, float(sig[i]), *splan[i], use_prev=solver_uses_prev(splan[i]))
                if step_callback is not None:
                    step_callback(i, x)
                continue
            x = x + float(sig[i + 1] - sig[i]) * (den * inv)
            if step_callback is not None:
                step_callback(i, x)
        return x
