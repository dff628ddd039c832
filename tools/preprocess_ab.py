"""A/B of the two request-preprocessing routes (scail_amd/preprocess.py: ``prepare_pose_video`` on the host with torch, and
``prepare_pose_video_hip`` on the library's kernels) on one GPU box, in one process, alternating: a synthetic 1080 x 1920 uint8 driving
clip -> the half-resolution pose of a 512 x 896 request, as ``cli.request_from_files`` builds it (the result on the device, (3, T, 256, 448)).

    python tools/preprocess_ab.py [--frames 161 401] [--reps 2] [--chunk-frames 16]

Per clip length and route: wall time (host clock around the call, ended by a device synchronise; median and minimum over ``--reps`` after
one warm-up of the HIP route on a short clip), the peak host RSS DURING the call above the RSS before it (a sampling thread reads
/proc/self/statm every 2 ms; the clip itself is resident before and not counted), ``torch.cuda.max_memory_allocated`` over the call, and
the largest absolute difference of the two half-resolution results.  The routes alternate inside every repetition so that clock drift and
the other jobs on the host hit both alike.  The yardstick is the torch route in the same process on the same box: no ratio is fixed in
advance.  There is no fallback: without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _rss() -> int:
    with open("/proc/self/statm") as f:
        return int(f.read().split()[1]) * os.sysconf("SC_PAGE_SIZE")


class PeakRSS:
    """Peak resident set of this process while the block runs, sampled every 2 ms."""

    def __enter__(self):
        self.base = self.peak = _rss()
        self._stop = threading.Event()
        self._t = threading.Thread(target=self._run, daemon=True)
        self._t.start()
        return self

    def _run(self):
        while not self._stop.wait(0.002):
            self.peak = max(self.peak, _rss())

    def __exit__(self, *exc):
        self._stop.set()
        self._t.join()
        self.peak = max(self.peak, _rss())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="*", default=[161, 401])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--chunk-frames", type=int, default=16)
    ap.add_argument("--source", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--size", type=int, nargs=2, default=[512, 896])
    a = ap.parse_args(argv)
    from scail_amd import lib, preprocess
    lib.load()
    if not torch.cuda.is_available():
        raise lib.ScailHipError("tools/preprocess_ab.py measures on a GPU; none is available")
    size = tuple(a.size)

    def route_torch(clip):                                   # what request_from_files does with preprocess="torch"
        smpl = preprocess.prepare_pose_video(clip.permute(0, 3, 1, 2), size, downsample=True)[1]
        return smpl.permute(1, 0, 2, 3).contiguous().to("cuda")

    def route_hip(clip):
        return preprocess.prepare_pose_video_hip(clip, size, chunk_frames=a.chunk_frames)[1]

    routes = {"hip": route_hip, "torch": route_torch}

    def measure(fn, clip):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        with PeakRSS() as rss:
            t0 = time.perf_counter()
            out = fn(clip)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        return out, dt, rss.peak - rss.base, torch.cuda.max_memory_allocated()

    g = torch.Generator().manual_seed(7)
    route_hip(torch.randint(0, 256, (4, a.source[0], a.source[1], 3), dtype=torch.uint8, generator=g))      # warm-up: code objects, allocator
    torch.cuda.synchronize()
    for T in a.frames:
        clip = torch.randint(0, 256, (T, a.source[0], a.source[1], 3), dtype=torch.uint8, generator=g)
        times = {r: [] for r in routes}
        rss, dev, last = {r: 0 for r in routes}, {r: 0 for r in routes}, {}
        for _ in range(a.reps):
            for r, fn in routes.items():
                out, dt, host, mem = measure(fn, clip)
                times[r].append(dt)
                rss[r], dev[r] = max(rss[r], host), max(dev[r], mem)
                last[r] = out.cpu()
                del out
        diff = float((last["hip"] - last["torch"]).abs().max())
        differing = float(((last["hip"] - last["torch"]).abs() > 2.0 ** -22).float().mean())
        for r in routes:
            print(json.dumps({"route": r, "frames": T, "source": list(a.source), "target": list(size), "chunk_frames": a.chunk_frames if r == "hip" else None,
                              "seconds_median": round(statistics.median(times[r]), 3), "seconds_min": round(min(times[r]), 3), "reps": a.reps,
                              "peak_host_rss_above_start_GB": round(rss[r] / 1e9, 3), "clip_uint8_GB": round(clip.numel() / 1e9, 3),
                              "cuda_max_memory_allocated_GB": round(dev[r] / 1e9, 3), "half_shape": list(last[r].shape),
                              "half_max_abs_diff_between_routes": diff, "half_share_of_values_that_differ": differing}), flush=True)
        del clip, last


if __name__ == "__main__":
    main()
