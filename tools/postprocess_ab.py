"""A/B of the two request-output routes on one GPU box, in one process, alternating: a random latent -> the uint8 frames on the host that the
file writers take (``video_io._write_frames``), by the default route (``--postprocess torch``: fp32 decode, clamp and scaling as torch ops,
permuted copy, ``.cpu()``, the writer's stack and per-frame quantisation) and by the opt-in one (``--postprocess hip``: the decoder's last
kernel writes uint8 (T, H, W, 3), one ``.cpu()``).  Both decode streamed (``chunk_frames``), so the VAE workspace is the same for both.

    python tools/postprocess_ab.py [--latent-frames 41 101] [--reps 2] [--chunk-frames 4]

Per clip length and route: wall time from the latent to the host frames (host clock, median and minimum over ``--reps`` after one warm-up of
both routes on a 3-frame latent), the peak of ``torch.cuda.max_memory_allocated`` above what is allocated before the call (weights, latent and
the streamed workspace, which both routes keep between calls: the figure is the memory ABOVE the workspace), and the peak host RSS during the
call above the RSS before it (tools/preprocess_ab.py ``PeakRSS``; free heap is returned to the system before every call, so that a call's
buffers show in the RSS instead of reusing what the call before left).  The frames of the two routes are asserted equal.  The routes
alternate inside every repetition.  The yardstick is the torch route in the same process on the same box: no ratio is fixed in advance.
There is no fallback: without a GPU the tool fails."""
import argparse
import ctypes
import gc
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--latent-frames", type=int, nargs="*", default=[41, 101])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--chunk-frames", type=int, default=4)
    ap.add_argument("--latent-size", type=int, nargs=2, default=[64, 112], help="latent H W (the frames are 8 x as large)")
    ap.add_argument("--dim", type=int, default=96)
    a = ap.parse_args(argv)
    from scail_amd import lib
    from scail_amd.wan_vae import WanVAE
    from tools.preprocess_ab import PeakRSS
    lib.load()
    if not torch.cuda.is_available():
        raise lib.ScailHipError("tools/postprocess_ab.py measures on a GPU; none is available")
    torch.manual_seed(0)
    vae = WanVAE(dim=a.dim, device="cuda")
    hl, wl = a.latent_size

    def route_torch(z):                                      # cli._finish, cli.main and video_io.save_multi_video_grid, statement by statement
        x = vae.decode(z, chunk_frames=a.chunk_frames)       # (1, 3, T, H, W) fp32 in [-1, 1]
        video = torch.clamp((x + 1.0) / 2.0, 0.0, 1.0)
        torch.cuda.synchronize()
        samples = video.permute(0, 2, 1, 3, 4).contiguous().cpu()
        multi = torch.stack([v.float().cpu() for v in [samples]], dim=2)
        frames = []
        for fr in multi[0]:
            n, c, h, w = fr.shape
            grid = fr.permute(2, 0, 3, 1).reshape(h, n * w, c)
            frames.append((255.0 * grid).numpy().astype(np.uint8))
        return frames

    def route_hip(z):                                        # the same three places with postprocess="hip"
        video = vae.decode_u8(z, chunk_frames=a.chunk_frames)        # (1, T, H, W, 3) uint8
        torch.cuda.synchronize()
        return list(video.cpu().contiguous().numpy()[0])

    routes = {"hip": route_hip, "torch": route_torch}

    def measure(fn, z):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        gc.collect()
        libc.malloc_trim(0)
        with PeakRSS() as rss:
            t0 = time.perf_counter()
            out = fn(z)
            dt = time.perf_counter() - t0
        return out, dt, rss.peak - rss.base, torch.cuda.max_memory_allocated() - base

    libc = ctypes.CDLL("libc.so.6")
    g = torch.Generator().manual_seed(7)
    warm = [torch.randn(16, 3, hl, wl, generator=g).to("cuda")]
    for fn in routes.values():                               # warm-up: code objects, the streamed workspace, allocator
        fn(warm)
    ws = vae.model._c()._ws.numel()
    for Tl in a.latent_frames:
        z = [torch.randn(16, Tl, hl, wl, generator=g).to("cuda")]
        T = 1 + 4 * (Tl - 1)
        times = {r: [] for r in routes}
        rss, dev, last = {r: 0 for r in routes}, {r: 0 for r in routes}, {}
        for _ in range(a.reps):
            for r, fn in routes.items():
                last[r] = None                               # (the frames of the repetition before are not part of this one's RSS)
                out, dt, host, mem = measure(fn, z)
                times[r].append(dt)
                rss[r], dev[r] = max(rss[r], host), max(dev[r], mem)
                last[r] = out
                del out
        assert vae.model._c()._ws.numel() == ws             # one workspace served every call
        assert len(last["hip"]) == len(last["torch"]) == T
        differing = sum(int((p != q).sum()) for p, q in zip(last["hip"], last["torch"]))
        for r in routes:
            print(json.dumps({"route": r, "latent_frames": Tl, "frames": T, "frame_size": [8 * hl, 8 * wl], "chunk_frames": a.chunk_frames, "dim": a.dim,
                              "seconds_median": round(statistics.median(times[r]), 3), "seconds_min": round(min(times[r]), 3), "reps": a.reps,
                              "peak_device_above_workspace_GB": round(dev[r] / 1e9, 3), "workspace_GB": round(ws / 1e9, 3),
                              "peak_host_rss_above_start_GB": round(rss[r] / 1e9, 3), "frames_uint8_GB": round(T * 8 * hl * 8 * wl * 3 / 1e9, 3),
                              "fp32_clip_GB": round(T * 8 * hl * 8 * wl * 12 / 1e9, 3), "bytes_that_differ_between_routes": differing}), flush=True)
        assert differing == 0, f"{differing} bytes differ between the routes"
        del z, last


if __name__ == "__main__":
    main()
