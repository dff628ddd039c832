"""A/B of the fp8 (e4m3) per-token GEMM path against bf16, in one process, alternating the two arms with device events after warm-up
(include/scail_hip.h scail_gemm_fp8 / scail_quant_fp8_rows, include/scail_dit.h scail_dit_enable_fp8):
  * the four distinct 14B GEMM shapes at M = 97 664 (N x K = 15360 x 5120, 5120 x 5120, 13824 x 5120, 5120 x 13824): TFLOP/s of
    scail_gemm_bf16 (gemm4) and scail_gemm_fp8, the fraction of the 5 PF dense MX-fp8 peak, the ratio fp8 / gemm4;
  * the quantization pass in GB/s (bf16 read + e4m3 write + scales);
  * the config-2 step (14B, 512x896x81f, B = 2, CFG pair, scail_dit_step): bf16 against fp8 with every per-token GEMM in fp8, or the
    --mask of SCAIL_DIT_FP8_* bits;
  * --probe: the executor's GEMM error probe (scail_dit_fp8_probe) on the same config-2 evaluation: the (layers, 6) table of relative
    errors of every fp8 GEMM against its bf16 twin on clean bf16 activations, the worst token row per GEMM, and what the probed
    evaluation costs next to a plain one.
--scaling row | mx | both chooses the fp8 arm(s): per-row fp32 scales (scail_quant_fp8_rows + scail_gemm_fp8, the default), MX block scales
(scail_quant_mxfp8_rows + scail_gemm_mxfp8, E8M0 per 32 along K), or both, alternating with bf16 in the same rounds; every leg follows it,
and with both the MX figures are also given relative to the per-row arm of the same process (ratio of medians, and its min - max range
from max / min and min / max of the two arms).
--fp6 adds the 6-bit arm (scail_quant_mxfp6_rows + scail_gemm_mxfp6, scail_dit_enable_fp6: packed OCP e2m3 with E8M0 block scales) to every
leg, alternating with the others in the same rounds; its times are also given relative to the per-row and the MX fp8 arms of the run.
Usage: python tools/fp8_ab.py [--reps 10] [--layers 40] [--no-step] [--no-gemm] [--mask 63] [--probe] [--scaling row|mx|both] [--fp6]
Prints one line per measurement and a JSON summary line last."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scail_amd import lib as L, ops  # noqa: E402

M14B = 97664
SHAPES = [(15360, 5120), (5120, 5120), (13824, 5120), (5120, 13824)]
PEAK_FP8_TF = 5000.0
P14B = dict(hidden_size=5120, num_attention_heads=40, inner_hidden_size=13824, text_dim=4096, time_freq_dim=256, time_embed_dim=5120)


def _time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _summ(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def ab(arms, reps, warmup=2):
    """arms: {name: fn}; runs warmup rounds, then `reps` rounds alternating the arms; returns {name: [ms]}"""
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            out[k].append(_time(fn))
    return out


def _vs_row(row, mx):
    """mx time / row time: the ratio of the medians and the range [min / max, max / min] the repetitions allow"""
    return {"median": mx["median_ms"] / row["median_ms"], "range": [mx["min_ms"] / row["max_ms"], mx["max_ms"] / row["min_ms"]]}


def gemm_leg(reps, dev, scalings=("row",), fp6=False):
    res = []
    g = torch.Generator(device=dev).manual_seed(0)
    for N, K in SHAPES:
        x = torch.randn(M14B, K, device=dev, generator=g).to(torch.bfloat16)
        w = (torch.randn(N, K, device=dev, generator=g) * 0.02).to(torch.bfloat16)
        b = torch.randn(N, device=dev, generator=g)
        y = torch.empty(M14B, N, device=dev, dtype=torch.bfloat16)
        arms = {"bf16": lambda: ops.gemm(x, w, b, out=y)}
        if "row" in scalings:
            xq, sx = ops.quant_fp8_rows(x)
            wq, sw = ops.quant_fp8_rows(w)
            arms["fp8"] = lambda: ops.gemm_fp8(xq, sx, wq, sw, b, out=y)
            arms["quant"] = lambda: ops.quant_fp8_rows(x, out=xq, scale=sx)
        if "mx" in scalings:
            xm, ex = ops.quant_mxfp8_rows(x)
            wm, ew = ops.quant_mxfp8_rows(w)
            arms["mx"] = lambda: ops.gemm_mxfp8(xm, ex, wm, ew, b, out=y)
            arms["quant_mx"] = lambda: ops.quant_mxfp8_rows(x, out=xm, scale=ex)
        if fp6:
            x6, e6 = ops.quant_mxfp6_rows(x)
            w6, f6 = ops.quant_mxfp6_rows(w)
            arms["fp6"] = lambda: ops.gemm_mxfp6(x6, e6, w6, f6, b, out=y)
            arms["quant_fp6"] = lambda: ops.quant_mxfp6_rows(x, out=x6, scale=e6)
        ts = ab(arms, reps)
        flop = 2.0 * M14B * N * K
        r = {"N": N, "K": K, "M": M14B, "kernel_bf16": L.load().scail_gemm_kernel_for(K, N, 0, M14B, N, K, 0)}
        for k in ("bf16", "fp8", "mx", "fp6"):
            if k in ts:
                s = _summ(ts[k])
                r[k] = dict(s, tflops=flop / s["median_ms"] / 1e9, tflops_range=[flop / s["max_ms"] / 1e9, flop / s["min_ms"] / 1e9])
        line = f"GEMM {N:5d} x {K:5d} (M {M14B}): bf16 {r['bf16']['tflops']:7.1f} TF ({r['bf16']['median_ms']:.3f} ms)"
        # bytes of a quantization pass: bf16 read + e4m3 write + the scales (4 per row, or 1 per 32 columns); fp6 writes 3/4 byte per code
        for k, qk, sbytes in (("fp8", "quant", M14B * 4), ("mx", "quant_mx", M14B * K // 32), ("fp6", "quant_fp6", M14B * K // 32 - M14B * K // 4)):
            if k not in ts:
                continue
            r[k]["frac_mxfp8_peak"] = r[k]["tflops"] / PEAK_FP8_TF
            r[k + "_over_gemm4"] = r["bf16"]["median_ms"] / r[k]["median_ms"]
            qs = _summ(ts[qk])
            r[qk] = dict(qs, gbps=(M14B * K * 3 + sbytes) / qs["median_ms"] / 1e6)
            line += (f", {k} {r[k]['tflops']:7.1f} TF ({r[k]['median_ms']:.3f} ms, {100 * r[k]['frac_mxfp8_peak']:.1f} % of 5 PF), "
                     f"{k} / gemm4 {r[k + '_over_gemm4']:.3f}x;  {qk} of x {r[qk]['gbps']:.0f} GB/s ({qs['median_ms']:.3f} ms)")
        if "fp8" in ts and "mx" in ts:
            r["mx_time_over_row"] = {"gemm": _vs_row(r["fp8"], r["mx"]), "quant": _vs_row(r["quant"], r["quant_mx"])}
            v = r["mx_time_over_row"]
            line += (f";  mx / row time: GEMM {v['gemm']['median']:.3f} [{v['gemm']['range'][0]:.3f}, {v['gemm']['range'][1]:.3f}], "
                     f"quant {v['quant']['median']:.3f} [{v['quant']['range'][0]:.3f}, {v['quant']['range'][1]:.3f}]")
        if "fp6" in ts:
            r["fp6_time_over"] = {o: {"gemm": _vs_row(r[o], r["fp6"]), "quant": _vs_row(r[q], r["quant_fp6"])}
                                  for o, q in (("fp8", "quant"), ("mx", "quant_mx")) if o in ts}
            for o, v in r["fp6_time_over"].items():
                line += (f";  fp6 / {o} time: GEMM {v['gemm']['median']:.3f} [{v['gemm']['range'][0]:.3f}, {v['gemm']['range'][1]:.3f}], "
                         f"quant {v['quant']['median']:.3f} [{v['quant']['range'][0]:.3f}, {v['quant']['range'][1]:.3f}]")
        print(line, flush=True)
        res.append(r)
        del x, w, y, arms
        xq = wq = xm = wm = x6 = w6 = None
        torch.cuda.empty_cache()
    return res


def step_leg(reps, layers, mask, dev, scalings=("row",), fp6=False):
    from scail_amd.cstep import CStep
    from scail_amd.dit import DiffusionTransformer
    from scail_amd.sampler import make_flow_timesteps
    T, H, W, Lt, Lc = 21, 64, 112, 512, 257
    net = DiffusionTransformer(transformer_args=dict(model_parallel_size=1), num_frames=81, latent_width=300, latent_height=300,
                               share_adaln=True, use_i2v_clip=True, device=dev, init_seed=1234, num_layers=layers, **P14B)
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(1, T, 16, H, W, generator=g).to(dev)
    ref = torch.randn(1, 1, 16, H, W, generator=g).to(dev).to(torch.bfloat16)
    pose = torch.randn(1, T, 16, H // 2, W // 2, generator=g).to(dev).to(torch.bfloat16)
    ctx = torch.randn(2, Lt, P14B["text_dim"], generator=g).to(dev).to(torch.bfloat16)
    clip = torch.randn(1, Lc, 1280, generator=g).to(dev).to(torch.bfloat16)
    sig = make_flow_timesteps(0, 50, shift_scale=5, mode="normal")
    t = (sig[10] * 1000.0).repeat(2).to(dev)
    xin = torch.cat([x, x], 0)
    dummy = torch.zeros(1, device=dev)
    net._cstep = CStep(net, net.prepare())
    state = {}

    def run(mode):
        if state.get("mode") != mode:
            if mode == "fp6":
                net._cstep.enable_fp6(mask, dev)
            else:
                net._cstep.enable_fp8(0 if mode == "bf16" else mask, dev, scaling="mx" if mode == "mx" else "row")
            torch.cuda.synchronize()
            state["mode"] = mode
        return net.forward_f32(xin, t, ctx, None, concat_images=dummy, ref_concat=ref, concat_smpl_render=pose, image_clip_features=clip,
                               cfg_pair=True)

    modes = ["bf16"] + [{"row": "fp8", "mx": "mx"}[s] for s in scalings] + (["fp6"] if fp6 else [])
    ref16 = run("bf16").float().flatten().double()
    cos = {m: float(torch.nn.functional.cosine_similarity(ref16, run(m).float().flatten().double(), dim=0)) for m in modes[1:]}
    del ref16
    ts = ab({m: (lambda m=m: run(m)) for m in modes}, reps, warmup=1)
    r = {"layers": layers, "mask": mask, "L": (1 + T) * (H // 2) * (W // 2) + T * (H // 4) * (W // 4)}
    for k in modes:
        r[k] = _summ(ts[k])
    # per-category kernel time of one step of each arm (the executor's own event pairs)
    for mode in modes:
        run(mode)
        torch.cuda.synchronize()
        net._cstep.profile(True)
        run(mode)
        torch.cuda.synchronize()
        r[mode]["gemm_ms"] = net._cstep.profile_read(CStep.PROF_GEMM)[0]
        net._cstep.profile(False)
    line = (f"config-2 step ({layers} layers, mask {mask}): bf16 {r['bf16']['median_ms']:.1f} ms [{r['bf16']['min_ms']:.1f}, "
            f"{r['bf16']['max_ms']:.1f}] (GEMMs {r['bf16']['gemm_ms']:.1f})")
    for k in modes[1:]:
        r["cosine_" + k + "_vs_bf16"] = cos[k]
        r["speedup" if k == "fp8" else "speedup_" + k] = sp = r["bf16"]["median_ms"] / r[k]["median_ms"]
        line += (f", {k} {r[k]['median_ms']:.1f} ms [{r[k]['min_ms']:.1f}, {r[k]['max_ms']:.1f}] (GEMMs + quant {r[k]['gemm_ms']:.1f}); "
                 f"speedup {sp:.3f}x; output cosine {k} vs bf16 {cos[k]:.6f}")
    if "fp8" in r and "mx" in r:
        r["mx_time_over_row"] = v = _vs_row(r["fp8"], r["mx"])
        line += f";  mx / row step time {v['median']:.3f} [{v['range'][0]:.3f}, {v['range'][1]:.3f}]"
    if "fp6" in r:
        r["fp6_time_over"] = {o: _vs_row(r[o], r["fp6"]) for o in ("fp8", "mx") if o in r}
        for o, v in r["fp6_time_over"].items():
            line += f";  fp6 / {o} step time {v['median']:.3f} [{v['range'][0]:.3f}, {v['range'][1]:.3f}]"
    print(line, flush=True)
    net._cstep.close()
    return r


def probe_leg(layers, mask, dev, scaling="row"):
    """scaling: "row" | "mx" (fp8) or "fp6" (the 6-bit form)"""
    precision = "fp6" if scaling == "fp6" else "fp8"
    from scail_amd import cli
    from scail_amd.dit import DiffusionTransformer
    from scail_amd.sampler import make_flow_timesteps
    T, H, W, Lt, Lc = 21, 64, 112, 512, 257
    net = DiffusionTransformer(transformer_args=dict(model_parallel_size=1), num_frames=81, latent_width=300, latent_height=300,
                               share_adaln=True, use_i2v_clip=True, device=dev, init_seed=1234, num_layers=layers, gemm_precision=precision,
                               fp8_gemms=mask, fp8_scaling="row" if precision == "fp6" else scaling, **P14B)
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(1, T, 16, H, W, generator=g).to(dev)
    ref = torch.randn(1, 1, 16, H, W, generator=g).to(dev).to(torch.bfloat16)
    pose = torch.randn(1, T, 16, H // 2, W // 2, generator=g).to(dev).to(torch.bfloat16)
    ctx = torch.randn(2, Lt, P14B["text_dim"], generator=g).to(dev).to(torch.bfloat16)
    clip = torch.randn(1, Lc, 1280, generator=g).to(dev).to(torch.bfloat16)
    t = (make_flow_timesteps(0, 50, shift_scale=5, mode="normal")[0] * 1000.0).repeat(2).to(dev)     # the sampler's first evaluation
    xin = torch.cat([x, x], 0)
    kw = dict(concat_images=torch.zeros(1, device=dev), ref_concat=ref, concat_smpl_render=pose, image_clip_features=clip, cfg_pair=True)
    net.forward_f32(xin, t, ctx, None, **kw)                      # warm-up: conditioning, tile tables, workspace
    torch.cuda.synchronize()
    plain_ms = _time(lambda: net.forward_f32(xin, t, ctx, None, **kw))
    res = {}
    probe_ms = _time(lambda: res.update(zip(("rel_err", "worst"), net.fp8_probe(xin, t, ctx, None, **kw))))
    rel, worst = res["rel_err"], res["worst"]
    print(cli.format_fp8_table(dict(rel_err=rel, masks=[mask] * layers, enabled=mask, scaling=scaling, precision=precision), float("inf")))
    print("worst token row of each GEMM (same layout):")
    for i in range(layers):
        print(f"{i:5d} " + " ".join(f"{float(worst[i, k]):8.2e}" for k in range(6)))
    on = [k for k in range(6) if (mask >> k) & 1]
    r = {"layers": layers, "mask": mask, "scaling": scaling, "plain_fp8_step_ms": plain_ms, "probed_step_ms": probe_ms,
         "rel_err_min": float(rel[:, on].min()), "rel_err_max": float(rel[:, on].max()), "worst_row_max": float(worst[:, on].max()),
         "rows_per_gemm": net.fp8_probe_table[:, :, 3].tolist()}
    print(f"probe at config-2 size ({layers} layers, mask {mask}, {scaling} scaling, random-init weights): relative error {r['rel_err_min']:.4f} .. {r['rel_err_max']:.4f}, "
          f"worst token row {r['worst_row_max']:.4f}; probed evaluation {probe_ms:.1f} ms (with the host read of the table) against "
          f"{plain_ms:.1f} ms for a plain {precision} step", flush=True)
    net._cstep.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step-reps", type=int, default=4)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--mask", type=int, default=L.FP8_ALL)
    ap.add_argument("--no-gemm", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--probe", action="store_true", help="also print the GEMM error probe's table at config-2 size")
    ap.add_argument("--scaling", choices=("row", "mx", "both"), default="row",
                    help="fp8 arm(s): per-row fp32 scales, MX block scales (E8M0 per 32 along K), or both alternating with bf16")
    ap.add_argument("--fp6", action="store_true", help="add the 6-bit (MXFP6 e2m3) arm to every leg")
    a = ap.parse_args()
    scalings = ("row", "mx") if a.scaling == "both" else (a.scaling,)
    dev = "cuda"
    L.load()
    out = {"device": torch.cuda.get_device_name(0)}
    if not a.no_gemm:
        out["gemm"] = gemm_leg(a.reps, dev, scalings, a.fp6)
    if not a.no_step:
        out["step"] = step_leg(a.step_reps, a.layers, a.mask, dev, scalings, a.fp6)
    if a.probe:
        legs = scalings + (("fp6",) if a.fp6 else ())
        out["probe"] = {s: probe_leg(a.layers, a.mask, dev, s) for s in legs} if len(legs) > 1 else probe_leg(a.layers, a.mask, dev, legs[0])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
