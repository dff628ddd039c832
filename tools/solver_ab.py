"""A/B of the opt-in solver plan (include/scail_dit.h "solver plan") against the plain Euler loop, on the random-init 14B network at config-2
size (512x896x81f: latent 21 x 64 x 112, CFG scale 4).  Two stages, each a child process of its own under its own time limit; inside a stage
the arms alternate in one process, timed with device events after a warm-up.  The tool stops at the first stage that fails.
  * pass stage: the update pass alone on config-2-sized buffers: scail_cfg_euler (what a step runs today) next to scail_cfg_multistep with
    and without the history term, on the same x and v.  Reported as times; the pass moves 5 to 6 floats per latent element and is not what
    a step's time is made of.
  * loops stage: the --steps loop (default 10): scail_dit_sample_chars, scail_dit_sample_solver under the "dpm1" table (first-order rows
    everywhere) and under the "dpmpp2m" table.  The three run the same evaluations; the expectation is that their medians lie within the
    plain arm's own repetition range, and the tool says so or says by how much they do not.
No step count is recommended and nothing is said about quality: on random-init weights nothing can be.
Usage: python tools/solver_ab.py [--reps 3] [--layers 40] [--steps 10] [--log profiles/solver_ab.log] [--stage-seconds 1100]
Prints one line per measurement (median and [min, max] of the repetitions) and a JSON summary line per stage; everything also goes to --log."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import threading

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from guidance_ab import CFG, H, T, W, _fmt, _net14b, _summ, ab  # noqa: E402
from scail_amd import lib as L  # noqa: E402
from scail_amd.sampler import make_flow_timesteps, plan_solver, solver_uses_prev  # noqa: E402

STAGES = ("pass", "loops")


def pass_stage(a):
    from scail_amd import ops
    dev = "cuda"
    n = T * 16 * H * W
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(1, T, 16, H, W, generator=g).to(dev)
    v = torch.randn(2, T, 16, H, W, generator=g).to(dev)
    hist = torch.randn(1, T, 16, H, W, generator=g).to(dev)
    row = plan_solver(make_flow_timesteps(0, 10, shift_scale=5), "dpmpp2m")[4]
    assert solver_uses_prev(row)
    arms = {"cfg_euler": lambda: ops.cfg_euler_(x, v, CFG, -0.05),
            "cfg_multistep, first order": lambda: ops.cfg_multistep_(x, v, hist, CFG, 0.7, row[0], 1.0 - row[0], 0.0, use_prev=False),
            "cfg_multistep, second order": lambda: ops.cfg_multistep_(x, v, hist, CFG, 0.7, *row, use_prev=True)}
    for fn in arms.values():                                   # warm-up
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in arms}
    for _ in range(max(a.reps, 20)):                           # a pass takes microseconds: more repetitions than a loop gets
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1))
    res = {k: _summ(ts) for k, ts in out.items()}
    floats = {"cfg_euler": 4, "cfg_multistep, first order": 5, "cfg_multistep, second order": 6}
    print(f"the update pass alone, n = {n} fp32 elements ({n * 4 / 1e6:.1f} MB per latent):", flush=True)
    for k, s in res.items():
        s["floats_moved_per_element"] = floats[k]
        print(f"  {k:28s}: {s['median_ms']:.4f} ms [{s['min_ms']:.4f}, {s['max_ms']:.4f}] ({floats[k]} floats per element, {floats[k] * n * 4 / 1e6:.1f} MB)",
              flush=True)
    return {"device": torch.cuda.get_device_name(0), "elements": n, "pass": res}


def loops_stage(a):
    dev = "cuda"
    net, x, ref, pose, ctx, clip = _net14b(a.layers, dev)
    n = a.steps
    sig = make_flow_timesteps(0, n, shift_scale=5, mode="normal")
    tables = {name: plan_solver(sig, name) for name in ("dpm1", "dpmpp2m")}
    run = lambda table=None, s=sig: net.sample_c(x, s, CFG, ctx, ref, pose, clip, **({} if table is None else {"solver": (s[:-1], table)}))
    # warm-up: every kernel, table and buffer of both routes, in two short loops (5 values: steps 2 and 3 are second order)
    run(s=sig[:3])
    run(plan_solver(sig[:5], "dpmpp2m"), sig[:5])
    torch.cuda.synchronize()
    res = {"steps": n, "arms": {}}
    arms = {"plain": lambda: run()}
    for name, table in tables.items():
        second = [i for i, r in enumerate(table) if solver_uses_prev(r)]
        res["arms"][name] = {"second_order_steps": second}
        arms[name] = (lambda table=table: run(table))
        print(f"  (table {name}: {len(second)} of {n} steps second order {second})", flush=True)
    outs = {}
    ts = ab(arms, a.reps, first=outs)
    res["plain"] = pl = ts["plain"]
    print(f"{n}-step sampler ({a.layers} layers): plain (scail_dit_sample_chars) {_fmt(pl)}", flush=True)
    for name, p in res["arms"].items():
        p.update(ts[name])
        p["finite"] = bool(torch.isfinite(outs[name]).all())
        p["bit_equal_to_plain"] = bool(torch.equal(outs[name], outs["plain"]))
        p["time_over_plain"] = v = {"median": p["median_ms"] / pl["median_ms"], "range": [p["min_ms"] / pl["max_ms"], p["max_ms"] / pl["min_ms"]]}
        p["median_within_plain_range"] = inside = pl["min_ms"] <= p["median_ms"] <= pl["max_ms"]
        where = ("within" if inside else "BELOW" if p["median_ms"] < pl["min_ms"] else "ABOVE")
        print(f"  {name:8s} (scail_dit_sample_solver): {_fmt(p)}; time / plain {v['median']:.4f} [{v['range'][0]:.4f}, {v['range'][1]:.4f}]; median "
              f"{where} the plain arm's own range [{pl['min_ms']:.1f}, {pl['max_ms']:.1f}] ms"
              + ("" if inside else f" ({(p['median_ms'] - pl['median_ms']) / n:+.3f} ms per step against the plain median)"), flush=True)
    return {"device": torch.cuda.get_device_name(0), "layers": a.layers, "loops": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "solver_ab.log"))
    ap.add_argument("--stage-seconds", type=int, default=1100, help="time limit of each stage's process")
    ap.add_argument("--stage", choices=STAGES, default=None, help="run this stage in this process (what the tool starts for each stage)")
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("--reps must be at least 3: ranges are reported")
    if a.steps < 4:
        ap.error("--steps must be at least 4 (fewer hold no second-order step)")
    if a.stage is not None:
        L.load()
        print(json.dumps({"pass": pass_stage, "loops": loops_stage}[a.stage](a)), flush=True)
        return
    with open(a.log, "w") as log:
        for stage in STAGES:
            cmd = [sys.executable, os.path.abspath(__file__), "--stage", stage, "--reps", str(a.reps), "--layers", str(a.layers), "--steps", str(a.steps)]
            head = f"== stage {stage}: {os.path.relpath(cmd[1], ROOT)} {' '.join(cmd[2:])} (limit {a.stage_seconds} s)"
            print(head, flush=True)
            log.write(head + "\n")
            log.flush()
            proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
            timer = threading.Timer(a.stage_seconds, proc.kill)
            try:
                timer.start()
                for line in proc.stdout:                   # the stage's lines as they come; the limit covers the whole stage
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
