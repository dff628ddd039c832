"""A/B of the opt-in guidance plan (include/scail_dit.h "guidance plan") against the plain routes, on the random-init 14B network at config-2
size (512x896x81f: latent 21 x 64 x 112, CFG scale 4).  Two stages, each a child process of its own under its own time limit; inside a stage
the arms alternate in one process, timed with device events after a warm-up.  The tool stops at the first stage that fails.
  * eval stage: one pair evaluation (B = 2, SCAIL_DIT_CFG_PAIR, what a step runs today) against one branch evaluation
    (scail_dit_step_branch, elem 1 of 2); the measured ratio is printed next to the ratio of executed FLOPs, by bench.py's accounting
    (step_flops minus the last-layer row pruning and, for the pair, the shared layer 0).  No gate: the B = 1 launches fill whole-device
    rounds differently.
  * loops stage: the --steps Euler loop (default 10): scail_dit_sample_chars, scail_dit_sample_guided under the all-PAIR plan (the same
    evaluations plus one pass per step that reads 2 n and writes n floats: its median should lie within the plain arm's own repetition
    range, and the tool says so or says by how much it does not), the plan [0, 1] x steps / 2, an interval plan with half the steps COND,
    and that interval plan merged with a step-cache plan in which 6 of 10 steps compute.  Each is reported as a multiple of the plain
    loop next to the count of pair, branch and reused evaluations in its plan.
The plans are chosen to spread the cost, NOT recommendations: on random-init weights nothing can be said about quality, and nothing is.
Usage: python tools/guidance_ab.py [--reps 3] [--layers 40] [--steps 10] [--log profiles/guidance_ab.log] [--stage-seconds 1100]
Prints one line per measurement (median and [min, max] of the repetitions) and a JSON summary line per stage; everything also goes to --log."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scail_amd import lib as L  # noqa: E402
from scail_amd.sampler import make_flow_timesteps, merge_guidance_with_step_cache, plan_guidance  # noqa: E402

P14B = dict(hidden_size=5120, num_attention_heads=40, inner_hidden_size=13824, text_dim=4096, time_freq_dim=256, time_embed_dim=5120)
T, H, W, LT, LC = 21, 64, 112, 512, 257
CFG = 4.0
STAGES = ("eval", "loops")


def _summ(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": len(ts)}


def _fmt(s):
    return f"{s['median_ms']:.1f} ms [{s['min_ms']:.1f}, {s['max_ms']:.1f}]"


def ab(arms, reps, first=None):
    """arms: {name: fn}; `reps` rounds alternating the arms, each call between two device events; {name: summary}.  ``first``: a dict that
    receives a copy of what each arm returned in the first round"""
    out = {k: [] for k in arms}
    for i in range(reps):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            o = fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1))
            if i == 0 and first is not None:
                first[k] = o.clone()
        print(f"  (round {i + 1} of {reps}: " + ", ".join(f"{k} {v[-1]:.0f} ms" for k, v in out.items()) + ")", flush=True)
    return {k: _summ(v) for k, v in out.items()}


def executed_flops(layers):
    """(pair, branch) executed FLOPs of one evaluation, by bench.py's accounting: step_flops(B) minus the last layer's pruned ref / pose
    rows per element, minus (pair only) layer 0's shared self-attention part"""
    import bench
    p = dict(P14B, num_layers=layers)
    D, FF = p["hidden_size"], p["inner_hidden_size"]
    hp, wp = H // 2, W // 2
    Lnoise = T * hp * wp
    L = hp * wp + Lnoise + T * (H // 4) * (W // 4)
    prune = (L - Lnoise) * (4 * L * D + 4 * (LT + LC) * D + 2 * D * (3 * D + 2 * FF))
    pair = bench.step_flops(p, L, LT, LC, B=2) - 2 * prune - (4.0 * L * L * D + 2.0 * L * D * 4 * D)
    branch = bench.step_flops(p, L, LT, LC, B=1) - prune
    return pair, branch


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


def eval_stage(a):
    dev = "cuda"
    net, x, ref, pose, ctx, clip = _net14b(a.layers, dev)
    sig = make_flow_timesteps(0, 50, shift_scale=5, mode="normal")
    t2 = (sig[10] * 1000.0).repeat(2).to(dev)
    t1 = t2[:1].contiguous()
    xin = torch.cat([x, x], 0)
    kw = dict(concat_images=torch.zeros(1, device=dev), ref_concat=ref, concat_smpl_render=pose, image_clip_features=clip)
    ex = net._executor()
    cond = net._conditioning(ctx, clip)
    cos, sin = net._rope(T, H // 2, W // 2, 0, 0, torch.device(dev), 1)
    pair = lambda: net.forward_f32(xin, t2, ctx, None, cfg_pair=True, **kw)
    branch = lambda: ex.step_branch(x, t1, cond, 1, ref, pose, cos, sin)
    vp, vb = pair().clone(), branch().clone()          # (also the warm-up)
    same = bool(torch.equal(vp[1:2], vb))
    del vp, vb
    r = ab({"pair": pair, "branch": branch}, a.reps)
    fp, fb = executed_flops(a.layers)
    r["time_branch_over_pair"] = {"median": r["branch"]["median_ms"] / r["pair"]["median_ms"],
                                  "range": [r["branch"]["min_ms"] / r["pair"]["max_ms"], r["branch"]["max_ms"] / r["pair"]["min_ms"]]}
    r["executed_tflop"] = {"pair": fp / 1e12, "branch": fb / 1e12, "branch_over_pair": fb / fp}
    r["branch_bit_equal_to_the_pairs_cond_half"] = same
    v = r["time_branch_over_pair"]
    print(f"config-2 evaluation ({a.layers} layers): pair {_fmt(r['pair'])}, branch {_fmt(r['branch'])}; branch / pair measured {v['median']:.3f} "
          f"[{v['range'][0]:.3f}, {v['range'][1]:.3f}], by executed FLOPs {fb / fp:.3f} ({fb / 1e12:.1f} / {fp / 1e12:.1f} TFLOP); the branch's "
          f"velocity {'equals' if same else 'DIFFERS from'} the cond half of the pair's bit for bit (recorded, not required: B = 1 and B = 2 "
          "may take different GEMM kernels)", flush=True)
    return {"device": torch.cuda.get_device_name(0), "layers": a.layers, "eval": r}


def _spread(steps, k):
    """a step-cache plan in which k steps compute, evenly spread, first and last among them"""
    computed = {round(j * (steps - 1) / (k - 1)) for j in range(k)} if k > 1 else {0}
    return [0 if i in computed else 1 for i in range(steps)]


def loops_stage(a):
    dev = "cuda"
    net, x, ref, pose, ctx, clip = _net14b(a.layers, dev)
    n = a.steps
    sig = make_flow_timesteps(0, n, shift_scale=5, mode="normal")
    start = [float(v) for v in sig[:-1]]
    lo = n // 4
    interval = plan_guidance(start, interval=(start[lo + n // 2 - 1], start[lo]))          # the middle half guided, half the steps COND
    mask = _spread(n, max(2, round(0.6 * n)))
    plans = {"all-PAIR": (plan_guidance(start), None),
             "[0,1] alternating": (plan_guidance(start, every=2), None),
             "interval, half COND": (interval, None),
             "interval + step cache": (merge_guidance_with_step_cache(interval, mask), mask)}
    run = lambda guide=None, reuse=None, s=sig: net.sample_c(x, s, CFG, ctx, ref, pose, clip, guide=guide, reuse=reuse)
    # warm-up: every kernel, table and buffer of every mode, in three short loops
    run(s=sig[:3])
    run([0, 1, 2], None, sig[:4])
    run([0, 0, 2, 2], [0, 1, 0, 1], sig[:5])
    torch.cuda.synchronize()
    res = {"steps": n, "plans": {}}
    arms = {"plain": lambda: run()}
    for label, (guide, reuse) in plans.items():
        computing = [g for i, g in enumerate(guide) if not (reuse and reuse[i])]
        res["plans"][label] = {"guide": guide, "reuse": reuse, "pair_evaluations": computing.count(0), "branch_evaluations": len(computing) - computing.count(0),
                               "reused_evaluations": n - len(computing)}
        arms[label] = (lambda guide=guide, reuse=reuse: run(guide, reuse))
        print(f"  (plan {label}: guide {guide}" + (f", reuse {reuse}" if reuse else "") + ")", flush=True)
    outs = {}
    ts = ab(arms, a.reps, first=outs)
    for label, p in res["plans"].items():
        p["bit_equal_to_plain"] = bool(torch.equal(outs[label], outs["plain"]))
        p["finite"] = bool(torch.isfinite(outs[label]).all())
    res["plain"] = pl = ts["plain"]
    print(f"{n}-step sampler ({a.layers} layers): plain (scail_dit_sample_chars) {_fmt(pl)}", flush=True)
    for label, p in res["plans"].items():
        p.update(ts[label])
        p["time_over_plain"] = v = {"median": p["median_ms"] / pl["median_ms"], "range": [p["min_ms"] / pl["max_ms"], p["max_ms"] / pl["min_ms"]]}
        print(f"  plan {label:22s}: {p['pair_evaluations']} pair, {p['branch_evaluations']} branch, {p['reused_evaluations']} reused evaluations; {_fmt(p)}; "
              f"time / plain {v['median']:.3f} [{v['range'][0]:.3f}, {v['range'][1]:.3f}]"
              f"{' (final latent bit-equal to plain)' if p['bit_equal_to_plain'] else ''}", flush=True)
    ap_ = res["plans"]["all-PAIR"]
    inside = pl["min_ms"] <= ap_["median_ms"] <= pl["max_ms"]
    res["all_pair_median_within_plain_range"] = inside
    nbytes = 3 * T * 16 * H * W * 4
    if inside:
        print(f"all-PAIR: median {ap_['median_ms']:.1f} ms lies within the plain arm's own range [{pl['min_ms']:.1f}, {pl['max_ms']:.1f}] ms", flush=True)
    elif ap_["median_ms"] < pl["min_ms"]:
        print(f"all-PAIR: median {ap_['median_ms']:.1f} ms lies BELOW the plain arm's own range [{pl['min_ms']:.1f}, {pl['max_ms']:.1f}] ms: the plan "
              "cost no measurable time (the arms alternate; the difference is drift between them)", flush=True)
    else:
        per = (ap_["median_ms"] - pl["median_ms"]) / n
        print(f"all-PAIR: median {ap_['median_ms']:.1f} ms lies OUTSIDE the plain arm's own range [{pl['min_ms']:.1f}, {pl['max_ms']:.1f}] ms: "
              f"{per:+.3f} ms per step against the plain median; the only extra work of a step is scail_cfg_delta_store, one pass over "
              f"{nbytes / 1e6:.1f} MB (read 2 n, write n floats: {nbytes / 8e12 * 1e3:.4f} ms at the 8 TB/s HBM peak) and its launch, so whatever "
              "exceeds that is run-to-run drift between the alternating arms, not work of the plan", flush=True)
    return {"device": torch.cuda.get_device_name(0), "layers": a.layers, "loops": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "guidance_ab.log"))
    ap.add_argument("--stage-seconds", type=int, default=1100, help="time limit of each stage's process")
    ap.add_argument("--stage", choices=STAGES, default=None, help="run this stage in this process (what the tool starts for each stage)")
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("--reps must be at least 3: ranges are reported")
    if a.steps < 4 or a.steps % 2:
        ap.error("--steps must be even and at least 4 (the plans need steps to skip)")
    if a.stage is not None:
        L.load()
        print(json.dumps({"eval": eval_stage, "loops": loops_stage}[a.stage](a)), flush=True)
        return
    with open(a.log, "w") as log:
        for stage in STAGES:
            cmd = [sys.executable, os.path.abspath(__file__), "--stage", stage, "--reps", str(a.reps), "--layers", str(a.layers), "--steps", str(a.steps)]
            head = f"== stage {stage}: {' '.join(cmd[1:])} (limit {a.stage_seconds} s)"
            print(head, flush=True)
            log.write(head + "\n")
            log.flush()
            proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
            try:
                # the stage's lines as they come; the limit covers the whole stage
                import threading
                timer = threading.Timer(a.stage_seconds, proc.kill)
                timer.start()
                for line in proc.stdout:
                    sys.stdout.write(line)
                    sys.stdout.flush()
                    log.write(line)
                    log.flush()
                rc = proc.wait()
            finally:
                timer.cancel()
            if rc != 0:
                tail = f"== stage {stage} failed (status {rc}{': killed at its time limit' if rc == -9 else ''}); stopping"
                print(tail, flush=True)
                log.write(tail + "\n")
                sys.exit(1)


if __name__ == "__main__":
    main()
