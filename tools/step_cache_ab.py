"""A/B of the opt-in step cache (include/scail_dit.h "step cache") against the plain routes, alternating in one process with device events
after a warm-up, on the random-init 14B network at config-2 size (512x896x81f: latent 21 x 64 x 112, B = 2, CFG pair):
  * step leg: the plain step (scail_dit_step_chars) against a FILL evaluation -- the two outputs must be bit-equal at this size -- and one
    REUSE evaluation;
  * row leg: scail_resid_store and scail_resid_apply on the evaluation's own [2, Lnoise, D] rows, bytes moved / time as a fraction of the
    8.0 TB/s HBM peak, next to an existing row pass (scail_ln_modulate) on the same rows in the same rounds;
  * sample leg: the --sample-steps Euler loop, scail_dit_sample against scail_dit_sample_cached under the all-zero plan and the plans of
    --ratios x the median relative distance of the schedule's time embeddings (thresholds chosen to spread the plans, NOT recommendations:
    on random-init weights they say nothing about quality), and the cosine of each final latent against the uncached one;
  * tiny leg: the same plans' cosine against the fp32 reference trajectory tests/golden/sampler_tiny_50.npz on BASELINE config 1's
    network (recorded, not gated);
  * tiled leg (--tiled: this leg alone): a latent of --tiled-frames frames in the windows of cli.plan_tiles(frames, 21, 10) -- 41 frames
    in three 21-frame windows, the shape of profiles/longclip_onecall.log --, --tiled-steps steps: scail_dit_sample_tiled against
    scail_dit_sample_tiled_cached under the all-zero plan (the same evaluations: the two should differ by no more than the spread of the
    repetitions) and under two explicit plans in which about 60 % and 40 % of the steps compute, evenly spread, first and last step
    computing (plans chosen to spread the cost, NOT recommendations).  --reps may be 2 here: one round is minutes.
Usage: python tools/step_cache_ab.py [--reps 3] [--layers 40] [--sample-steps 50] [--ratios 1.5,3] [--signal time] [--no-step] [--no-rows]
       [--no-sample] [--no-tiny]
       python tools/step_cache_ab.py --tiled [--reps 2] [--layers 40] [--tiled-frames 41] [--tiled-steps 5]
Prints one line per measurement (median and [min, max] of the repetitions) and a JSON summary line last."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scail_amd import lib as L, ops  # noqa: E402
from scail_amd.sampler import RFSampler, make_flow_timesteps, plan_step_cache  # noqa: E402

P14B = dict(hidden_size=5120, num_attention_heads=40, inner_hidden_size=13824, text_dim=4096, time_freq_dim=256, time_embed_dim=5120)
HBM_PEAK_TBS = 8.0
T, H, W, LT, LC = 21, 64, 112, 512, 257


def _time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _summ(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": len(ts)}


def _fmt(s):
    return f"{s['median_ms']:.3f} ms [{s['min_ms']:.3f}, {s['max_ms']:.3f}]"


def ab(arms, reps, warmup=1):
    """arms: {name: fn}; `warmup` rounds, then `reps` rounds alternating the arms; {name: summary}"""
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in arms}
    for i in range(reps):
        for k, fn in arms.items():
            out[k].append(_time(fn))
        if sum(v[-1] for v in out.values()) > 10e3:          # long rounds: say that the run is alive
            print(f"  (round {i + 1} of {reps}: " + ", ".join(f"{k} {v[-1]:.0f} ms" for k, v in out.items()) + ")", flush=True)
    return {k: _summ(v) for k, v in out.items()}


def _cos(a, b):
    a, b = a.flatten().double(), b.flatten().double()
    return float((a @ b) / (a.norm() * b.norm()))


def _plans(dist, ratios):
    """{label: (threshold, plan)}: the all-zero plan and one plan per ratio x the median relative distance"""
    d = [float(r[0] / r[1]) for r in dist[1:] if float(r[1]) > 0]
    med = statistics.median(d) if d else 0.0
    plans = {"all-zero": (0.0, plan_step_cache(dist, 0.0))}
    for r in ratios:
        plans[f"{r:g} x median"] = (r * med, plan_step_cache(dist, r * med))
    return med, plans


def _net14b(layers, dev):
    from scail_amd.dit import DiffusionTransformer
    net = DiffusionTransformer(transformer_args=dict(model_parallel_size=1), num_frames=81, latent_width=300, latent_height=300,
                               share_adaln=True, use_i2v_clip=True, device=dev, init_seed=1234, num_layers=layers, **P14B)
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(1, T, 16, H, W, generator=g).to(dev)
    ref = torch.randn(1, 1, 16, H, W, generator=g).to(dev).to(torch.bfloat16)
    pose = torch.randn(1, T, 16, H // 2, W // 2, generator=g).to(dev).to(torch.bfloat16)
    ctx = torch.randn(2, LT, P14B["text_dim"], generator=g).to(dev).to(torch.bfloat16)
    clip = torch.randn(1, LC, 1280, generator=g).to(dev).to(torch.bfloat16)
    return net, x, ref, pose, ctx, clip


def step_leg(net, inputs, reps, dev):
    x, ref, pose, ctx, clip = inputs
    sig = make_flow_timesteps(0, 50, shift_scale=5, mode="normal")
    kw = dict(concat_images=torch.zeros(1, device=dev), ref_concat=ref, concat_smpl_render=pose, image_clip_features=clip, cfg_pair=True)
    xin = torch.cat([x, x], 0)
    t10, t11 = ((sig[i] * 1000.0).repeat(2).to(dev) for i in (10, 11))
    plain = net.forward_f32(xin, t10, ctx, None, **kw).clone()
    fill = net.forward_f32(xin, t10, ctx, None, step_cache="fill", **kw)
    assert torch.equal(plain, fill), f"FILL differs from the plain step in {int((plain != fill).sum())} values at full size"
    del fill
    full11 = net.forward_f32(xin, t11, ctx, None, **kw).clone()
    reuse11 = net.forward_f32(xin, t11, ctx, None, step_cache="reuse", **kw)
    cos = _cos(full11, reuse11)
    del plain, full11, reuse11
    r = ab({"plain": lambda: net.forward_f32(xin, t10, ctx, None, **kw),
            "fill": lambda: net.forward_f32(xin, t10, ctx, None, step_cache="fill", **kw),
            "reuse": lambda: net.forward_f32(xin, t11, ctx, None, step_cache="reuse", **kw)}, reps)
    r["fill_bit_equal_to_plain"] = True
    r["cosine_reuse_vs_full_next_step"] = cos
    print(f"config-2 evaluation ({net.num_layers} layers): plain {_fmt(r['plain'])}, FILL {_fmt(r['fill'])} (out bit-equal to plain), "
          f"REUSE {_fmt(r['reuse'])}; velocity of step 11 from step 10's residual against its full evaluation: cosine {cos:.6f}", flush=True)
    return r


def rows_leg(reps, dev):
    D, Ln = P14B["hidden_size"], T * (H // 2) * (W // 2)
    g = torch.Generator(device=dev).manual_seed(1)
    a = torch.randn(2, Ln, D, device=dev, generator=g).to(torch.bfloat16)
    b = torch.randn(2, Ln, D, device=dev, generator=g).to(torch.bfloat16)
    r = torch.empty_like(a)
    y = torch.empty_like(a)
    sh = torch.randn(2, D, device=dev, generator=g)
    one = 2 * Ln * D * 2                             # bytes of one [2, Lnoise, D] bf16 operand
    arms = {"resid_store": (lambda: ops.resid_store(a, b, out=r), 3 * one),
            "resid_store in_bs 0": (lambda: ops.resid_store(a, b[:1].expand(2, Ln, D), out=r), 2 * one + one // 2),
            "resid_apply": (lambda: ops.resid_apply(b, r, out=y), 3 * one),
            "resid_apply in place, in_bs 0": (lambda: ops.resid_apply(y[:1].expand(2, Ln, D), r, out=y), 2 * one + one // 2),
            "ln_modulate": (lambda: ops.ln_modulate(a, sh, sh, out=y), 2 * one)}
    ts = ab({k: v[0] for k, v in arms.items()}, max(reps, 10), warmup=2)
    out = {}
    for k, (_, nbytes) in arms.items():
        s = ts[k]
        tbs = [nbytes / s[m] / 1e9 for m in ("median_ms", "max_ms", "min_ms")]
        out[k] = dict(s, bytes=nbytes, tb_per_s=tbs[0], frac_hbm_peak=tbs[0] / HBM_PEAK_TBS)
        print(f"row pass {k:32s} [2, {Ln}, {D}]: {_fmt(s)}, {nbytes / 1e6:.0f} MB moved, {tbs[0]:.2f} TB/s [{tbs[1]:.2f}, {tbs[2]:.2f}] = "
              f"{tbs[0] / HBM_PEAK_TBS:.2f} of the {HBM_PEAK_TBS:g} TB/s HBM peak", flush=True)
    return out


def sample_leg(net, inputs, reps, steps, ratios, signal, dev):
    x, ref, pose, ctx, clip = inputs
    sig = make_flow_timesteps(0, steps, shift_scale=5, mode="normal")
    dist = net.time_distances(sig[:-1] * 1000.0, signal)
    med, plans = _plans(dist, ratios)
    run = lambda plan: net.sample_c(x, sig, 4.0, ctx, ref, pose, clip, reuse=plan)
    base = net.sample_c(x, sig, 4.0, ctx, ref, pose, clip).clone()
    res = {"steps": steps, "signal": signal, "median_relative_distance": med, "plans": {}}
    arms = {"uncached": lambda: net.sample_c(x, sig, 4.0, ctx, ref, pose, clip)}
    for label, (thr, plan) in plans.items():
        out = run(plan)
        res["plans"][label] = {"threshold": thr, "plan": plan, "computed": plan.count(0), "cosine_vs_uncached": _cos(out, base),
                               "bit_equal_to_uncached": bool(torch.equal(out, base))}
        arms[label] = (lambda plan=plan: run(plan))
        del out
        print(f"  (plan {label}: {plan.count(0)} of {steps} steps compute: {plan})", flush=True)
    ts = ab(arms, reps, warmup=0)
    res["uncached"] = ts["uncached"]
    print(f"{steps}-step sampler ({net.num_layers} layers, signal {signal}, median relative distance {med:.4g}): uncached {_fmt(ts['uncached'])}", flush=True)
    for label, p in res["plans"].items():
        p.update(ts[label])
        p["time_over_uncached"] = {"median": p["median_ms"] / ts["uncached"]["median_ms"],
                                   "range": [p["min_ms"] / ts["uncached"]["max_ms"], p["max_ms"] / ts["uncached"]["min_ms"]]}
        v = p["time_over_uncached"]
        print(f"  plan {label:14s} threshold {p['threshold']:.4g}: {p['computed']} of {steps} steps compute; {_fmt(p)}; time / uncached "
              f"{v['median']:.3f} [{v['range'][0]:.3f}, {v['range'][1]:.3f}]; final latent cosine vs uncached {p['cosine_vs_uncached']:.6f}"
              f"{' (bit-equal)' if p['bit_equal_to_uncached'] else ''}", flush=True)
    return res


def tiny_leg(ratios, signal, dev):
    """BASELINE config 1's network on the golden request: cosine of the final latent against the fp32 reference trajectory, per plan"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_dit_gpu as TD
    from oracle import scail_oracle as O
    g = TD._load(os.path.join(ROOT, "tests", "golden"), "sampler_tiny_50.npz")
    _, _, net = TD._net(O.CONFIG1, int(g["seed"]))
    smp = RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=50,
                    guider_config={"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": 4}})
    shared = dict(concat_images=torch.zeros(1, *g["x0"].shape[1:], device=dev), ref_concat=g["ref"].to(dev),
                  concat_smpl_render=g["pose"].to(dev), image_clip_features=g["clip"].to(dev))
    c, uc = dict(crossattn=g["c_ctx"].to(dev), **shared), dict(crossattn=g["uc_ctx"].to(dev), **shared)
    base = smp.sample_hip(net, g["x0"].to(dev), c, uc).cpu()
    dist = net.time_distances(smp.sigmas()[:-1] * 1000.0, signal)
    med, plans = _plans(dist, ratios)
    res = {"uncached_cosine_vs_reference": _cos(base, g["xT"]), "median_relative_distance": med, "plans": {}}
    print(f"tiny golden (config 1, 50 steps): uncached cosine vs the fp32 reference {res['uncached_cosine_vs_reference']:.6f}", flush=True)
    for label, (thr, plan) in plans.items():
        out = smp.sample_hip(net, g["x0"].to(dev), c, uc, step_cache=dict(mask=plan)).cpu()
        res["plans"][label] = p = {"threshold": thr, "computed": plan.count(0), "cosine_vs_reference": _cos(out, g["xT"]),
                                   "cosine_vs_uncached": _cos(out, base)}
        print(f"  plan {label:14s} threshold {thr:.4g}: {p['computed']} of 50 steps compute; cosine vs the fp32 reference "
              f"{p['cosine_vs_reference']:.6f}, vs the uncached run {p['cosine_vs_uncached']:.6f} (random-init weights: recorded, not a quality figure)", flush=True)
    return res


def spread_plan(steps, fraction):
    """a plan in which round(fraction * steps) steps compute (at least the first; the last too from two on), evenly spread"""
    k = min(steps, max(1, round(fraction * steps)))
    computed = {0} if k == 1 else {round(j * (steps - 1) / (k - 1)) for j in range(k)}
    return [0 if i in computed else 1 for i in range(steps)]


def tiled_leg(net, reps, steps, frames, dev):
    from scail_amd.cli import plan_tiles
    from scail_amd.sampler import RFSamplerLong
    Tt = T
    tiles = plan_tiles(frames, Tt, 10)
    if tiles is None:
        raise SystemExit(f"--tiled-frames must exceed one window of {Tt} latent frames, got {frames}")
    g = torch.Generator().manual_seed(4321)
    x = torch.randn(1, frames, 16, H, W, generator=g).to(dev)
    ref = torch.randn(1, 1, 16, H, W, generator=g).to(dev).to(torch.bfloat16)
    pose = torch.randn(1, len(tiles), Tt, 16, H // 2, W // 2, generator=g).to(dev).to(torch.bfloat16)
    ctx = torch.randn(2, LT, P14B["text_dim"], generator=g).to(dev).to(torch.bfloat16)
    clip = torch.randn(1, LC, 1280, generator=g).to(dev).to(torch.bfloat16)
    sig = make_flow_timesteps(0, steps, shift_scale=5, mode="normal")
    _, tile_w, inv_wsum = RFSamplerLong(hunyuan_schedule=True)._tile_table(tiles, frames, dev)
    tile_w, inv_wsum = tile_w.cpu(), inv_wsum.cpu()
    run = lambda s, **kw: net.sample_tiled_c(x, s, 4.0, ctx, ref, pose, clip, tiles, tile_w, inv_wsum, **kw)
    plans = {"all-zero": [0] * steps, "60 %": spread_plan(steps, 0.6), "40 %": spread_plan(steps, 0.4)}
    # warm-up: one uncached step, then one computed and one reused step (every kernel, table and buffer of both modes)
    run(sig[:2])
    run(sig[:3], reuse=[0, 1])
    torch.cuda.synchronize()
    ex = net._executor()
    res = {"frames": frames, "tiles": [t[0] for t in tiles], "tile_frames": Tt, "steps": steps,
           "cache_bytes": ex.sample_tiled_cache_bytes(len(tiles), Tt, H, W), "stacked_step_caches_bytes": len(tiles) * ex.step_cache_bytes(2, Tt, H, W),
           "plans": {}}
    print(f"tiled: {frames}-frame latent {H}x{W}, {len(tiles)} windows of {Tt} (starts {res['tiles']}), {steps} steps, {net.num_layers} layers; cache "
          f"{res['cache_bytes'] / 1e9:.3f} GB (stacked step caches would be {res['stacked_step_caches_bytes'] / 1e9:.3f} GB)", flush=True)
    arms = {"uncached": lambda: run(sig)}
    for label, plan in plans.items():
        arms[label] = (lambda plan=plan: run(sig, reuse=plan))
        print(f"  (plan {label}: {plan.count(0)} of {steps} steps compute: {plan})", flush=True)
    outs = {}
    ts = {k: [] for k in arms}
    for i in range(reps):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            o = fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
            if i == 0:
                outs[k] = o.clone()
            print(f"  (round {i + 1} of {reps}: {k} {ts[k][-1]:.0f} ms)", flush=True)
    ts = {k: _summ(v) for k, v in ts.items()}
    res["uncached"] = ts["uncached"]
    print(f"{steps}-step tiled sampler: uncached (scail_dit_sample_tiled) {_fmt(ts['uncached'])}", flush=True)
    for label, plan in plans.items():
        p = res["plans"][label] = dict(ts[label], plan=plan, computed=plan.count(0), cosine_vs_uncached=_cos(outs[label], outs["uncached"]),
                                       bit_equal_to_uncached=bool(torch.equal(outs[label], outs["uncached"])))
        p["time_over_uncached"] = v = {"median": p["median_ms"] / ts["uncached"]["median_ms"],
                                       "range": [p["min_ms"] / ts["uncached"]["max_ms"], p["max_ms"] / ts["uncached"]["min_ms"]]}
        print(f"  plan {label:8s}: {p['computed']} of {steps} steps compute; {_fmt(p)}; time / uncached {v['median']:.3f} "
              f"[{v['range'][0]:.3f}, {v['range'][1]:.3f}]; final latent cosine vs uncached {p['cosine_vs_uncached']:.6f}"
              f"{' (bit-equal)' if p['bit_equal_to_uncached'] else ''}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--sample-steps", type=int, default=50)
    ap.add_argument("--ratios", default="1.5,3", help="thresholds of the measured plans, as multiples of the median relative distance")
    ap.add_argument("--signal", choices=tuple(L.CACHE_SIGNALS), default="time")
    for leg in ("step", "rows", "sample", "tiny"):
        ap.add_argument(f"--no-{leg}", action="store_true")
    ap.add_argument("--tiled", action="store_true", help="run the tiled leg alone (scail_dit_sample_tiled against scail_dit_sample_tiled_cached)")
    ap.add_argument("--tiled-frames", type=int, default=41, help="latent frames of the tiled leg's clip (windows of 21, overlap 10)")
    ap.add_argument("--tiled-steps", type=int, default=5)
    a = ap.parse_args()
    if a.reps < (2 if a.tiled else 3):
        ap.error("--reps must be at least 3 (2 with --tiled): ranges are reported")
    if a.tiled:
        if a.tiled_steps < 3:
            ap.error("--tiled-steps must be at least 3 (the plans need a step to skip)")
        L.load()
        net = _net14b(a.layers, "cuda")[0]
        out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "tiled": tiled_leg(net, a.reps, a.tiled_steps, a.tiled_frames, "cuda")}
        print(json.dumps(out))
        return
    ratios = [float(v) for v in a.ratios.split(",")]
    dev = "cuda"
    L.load()
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    if not a.no_rows:
        out["rows"] = rows_leg(a.reps, dev)
    if not (a.no_step and a.no_sample):
        net, *inputs = _net14b(a.layers, dev)
        if not a.no_step:
            out["step"] = step_leg(net, inputs, a.reps, dev)
        if not a.no_sample:
            out["sample"] = sample_leg(net, inputs, a.reps, a.sample_steps, ratios, a.signal, dev)
        net._cstep.close()
        del net, inputs
        torch.cuda.empty_cache()
    if not a.no_tiny:
        out["tiny"] = tiny_leg(ratios, a.signal, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
