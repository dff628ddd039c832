"""A/B of the whole-sequence and the streamed VAE decode (include/scail_vae.h scail_vae_decode_stream) on one GPU, in one process,
alternating: time and peak device memory of a 41-frame latent at 64 x 112 (161 frames of 512 x 896) for the chunks asked for, then --
``--long`` -- one clip the whole-sequence decode cannot hold, streamed only.

    python tools/vae_stream_ab.py [--chunks 2 4 8] [--reps 5] [--long 101]

Each figure is the median of ``--reps`` timed decodes after one warm-up of that variant; the variants alternate inside every repetition so
that clock and thermal drift hit all of them alike.  Peak memory is torch.cuda.max_memory_allocated over one decode of that variant with the
other variants' workspaces released first (latent, output video and workspace; the output video alone is 3 x T x 512 x 896 fp32)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, nargs="*", default=[2, 4, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=41, help="latent frames of the A/B clip")
    ap.add_argument("--long", type=int, default=0, help="latent frames of a clip to decode streamed only (0: skip)")
    ap.add_argument("--long-chunk", type=int, default=4)
    ap.add_argument("--hl", type=int, default=64)
    ap.add_argument("--wl", type=int, default=112)
    a = ap.parse_args(argv)
    from scail_amd.wan_vae import WanVAE_
    m = WanVAE_(dim=96, z_dim=16, device="cuda")
    c = m._c()
    g = torch.Generator().manual_seed(5)
    z = torch.randn(1, 16, a.frames, a.hl, a.wl, generator=g).cuda()
    variants = [None] + list(a.chunks)

    def decode(chunk, lat=z):
        c._ws = None                         # every variant allocates its own workspace: the peak is that variant's
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.decode(lat, chunk_frames=chunk)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return out, dt, torch.cuda.max_memory_allocated(), (c._ws.numel() if c._ws is not None else 0)

    def timed(chunk):                        # the decode alone, workspace already allocated
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.decode(z, chunk_frames=chunk)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    peak, ws, same = {}, {}, {}
    ref = None
    for v in variants:                       # warm-up + memory + equality
        out, _, peak[v], ws[v] = decode(v)
        if v is None:
            ref = out.cpu()
        else:
            same[v] = bool(torch.equal(out.cpu(), ref))
        del out
    times = {v: [] for v in variants}
    for _ in range(a.reps):
        for v in variants:
            c._ws = None
            timed(v)                          # (re)allocates this variant's workspace outside the timed call
            times[v].append(timed(v))
    base = statistics.median(times[None])
    for v in variants:
        t = statistics.median(times[v])
        print(json.dumps({"decode": "whole" if v is None else f"stream chunk {v}", "latent_frames": a.frames, "frames": 1 + 4 * (a.frames - 1),
                          "seconds_median": round(t, 4), "seconds_min": round(min(times[v]), 4), "vs_whole": round(t / base, 3),
                          "peak_allocated_GB": round(peak[v] / 1e9, 2), "workspace_GB": round(ws[v] / 1e9, 2),
                          "equals_whole": None if v is None else same[v], "reps": a.reps}))
    if a.long:
        del ref
        zl = torch.randn(1, 16, a.long, a.hl, a.wl, generator=g).cuda()
        out, dt, pk, w = decode(a.long_chunk, zl)
        print(json.dumps({"decode": f"stream chunk {a.long_chunk}", "latent_frames": a.long, "frames": 1 + 4 * (a.long - 1),
                          "seconds_first_call": round(dt, 4), "peak_allocated_GB": round(pk / 1e9, 2), "workspace_GB": round(w / 1e9, 2),
                          "output_video_GB": round(out.numel() * 4 / 1e9, 2), "finite": bool(torch.isfinite(out).all())}))


if __name__ == "__main__":
    main()
