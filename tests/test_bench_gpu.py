"""bench.py contract on the GPU box: one JSON line at N=1, and the N=2 launch line the driver uses
(python -m torch.distributed.run ...) -- here with both ranks on GPU 0 and the exchanges staged through
the host (SCAIL_DIST_BACKEND=gloo; RCCL refuses two ranks on one device), so that the multi-rank code
path of the script itself (sharding, both exchange modes, barrier/max timing, rank-0 print) is executed."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _run(cmd, env_extra=None, timeout=600, base_env=None):
    env = dict(os.environ if base_env is None else base_env)
    env.update(env_extra or {})
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_full_tiny():
    """--full: the headline line plus what takes runs of its own after the timed region (here cpu_baseline)."""
    o = _run([sys.executable, "bench.py", "--config", "tiny", "--steps", "2", "--warmup", "1", "--full"])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in o, k
    assert o["n_gpus"] == 1 and o["config"]["finite"] and o["value"] > 0
    assert o["roofline"]["achieved"] > 0 and o["cpu_baseline"]["value"] > 0
    assert o["config"]["path"].startswith("scail_dit_step") and o["roofline"]["timed_by"].startswith("scail_dit_profile")
    assert o["roofline"]["launches_timed"] == 2 * 2                      # 2 layers x 2 timed steps, from the executor's own event pairs
    assert o["cpu_baseline"]["kind"] == "port, extrapolated" and o["cpu_baseline"]["cores"] >= 1 and o["cpu_baseline"]["threads"] >= 1


def test_bench_plain_run_prints_the_headline_only():
    """Without --full the run ends after the timed steps: the headline line and the timed region's own kernel times, nothing that takes
    runs of its own after it."""
    o = _run([sys.executable, "bench.py", "--config", "tiny", "--steps", "2", "--warmup", "1"])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "config", "roofline"):
        assert k in o, k
    assert o["config"]["finite"] and o["value"] > 0 and o["roofline"]["launches_timed"] == 2 * 2
    assert "cpu_baseline" not in o and "traffic_in_run" not in o["roofline"]
    assert not {"vae", "sp_compute_side", "multichar"} & set(o["config"])


def test_bench_dump_outputs_tiny(tmp_path):
    """--dump-outputs DIR: after the --steps timed steps, the last step's network output and updated latent as float32 .npy files; the
    latent is the one the line's fingerprint (config.x_abs_mean) was taken from."""
    import numpy as np
    o = _run([sys.executable, "bench.py", "--config", "tiny", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-vae",
              "--dump-outputs", str(tmp_path / "out")])
    assert o["steps"] == 3 and o["ms_per_step"] > 0
    assert o["roofline"]["launches_timed"] == 2 * 3                      # 2 layers x 3 timed steps
    lat, vel = np.load(tmp_path / "out" / "latent.npy"), np.load(tmp_path / "out" / "velocity.npy")
    assert lat.dtype == vel.dtype == np.float32
    assert list(lat.shape) == o["dumped_outputs"]["latent"]["shape"] and lat.shape[0] == 1
    assert list(vel.shape) == o["dumped_outputs"]["velocity"]["shape"] and vel.shape == (2,) + lat.shape[1:]
    assert np.isfinite(lat).all() and np.isfinite(vel).all() and float(np.abs(vel).mean()) > 0
    assert abs(float(np.abs(lat).mean()) - o["config"]["x_abs_mean"]) <= 1e-5 * o["config"]["x_abs_mean"]


@pytest.mark.parametrize("mode", ["allgather", "ulysses"])
def test_bench_two_ranks_one_gpu(mode):
    one = _run([sys.executable, "bench.py", "--config", "tiny", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"])
    if mode == "allgather":          # the driver's launch line
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
               "--master-addr", "127.0.0.1", "--master-port", "29641", "bench.py", "--gpus", "2"]
    else:                            # a bare `python bench.py --gpus 2`: the script re-executes itself under torch.distributed.run
        cmd = [sys.executable, "bench.py", "--gpus", "2"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    two = _run(cmd + ["--config", "tiny", "--steps", "2", "--warmup", "1"], {"SCAIL_DIST_BACKEND": "gloo", "SCAIL_SP_MODE": mode}, base_env=env)
    assert two["n_gpus"] == 2 and two["config"]["finite"]
    assert two["config"]["parallelism"] == f"sp2-{mode}"
    assert "cpu_baseline" not in two
    # same seeds, same steps: the sharded run reproduces the single-rank latent (bf16 re-association only)
    assert abs(two["config"]["x_abs_mean"] - one["config"]["x_abs_mean"]) < 2e-3 * one["config"]["x_abs_mean"]


def test_bench_eight_process_ranks_full_width_two_layers():
    """The driver's 8-rank launch line, `python -m torch.distributed.run --nproc-per-node 8 ... bench.py --gpus 8`, at FULL WIDTH AND LENGTH (14B
    layer shapes, 512x896x81f: 8 ulysses ranks of 5 heads x 6 104 token rows) with 2 of the 40 layers, on the gloo vehicle (the exchange staged
    through the host): eight PROCESSES drive scail_dit_step_sp with SCAIL_DIT_CFG_PAIR, the last-layer pruning and the planned
    attention launch shape through a real process group, and the gathered result must reproduce the single-rank run of the same 2 layers.
    The ranks go one per GPU (bench.py maps a gloo rank to LOCAL_RANK % device count): eight processes on one device oversubscribe it,
    so the test needs an 8-GPU box."""
    import torch
    if torch.cuda.device_count() < 8:
        pytest.skip(f"needs 8 GPUs (one rank process per GPU), found {torch.cuda.device_count()}")
    common = ["--config", "14b", "--layers", "2", "--steps", "1", "--warmup", "1", "--no-vae", "--no-cpu-baseline", "--no-extra-legs"]
    one = _run([sys.executable, "bench.py"] + common, timeout=900)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1", "--master-port", "29643",
           "bench.py", "--gpus", "8"]
    eight = _run(cmd + common, {"SCAIL_DIST_BACKEND": "gloo"}, base_env=env, timeout=1500)
    cfg = eight["config"]
    assert eight["n_gpus"] == 8 and cfg["finite"] and cfg["parallelism"] == "sp8-ulysses" and cfg["path"].startswith("scail_dit_step_sp")
    from conftest import attention_plan_rows
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cfg["sp_check"]["ranks"] == 8 and cfg["attn_query_tile_rows"] == attention_plan_rows(cus, 5, 48832)      # 448 on the 256-CU part
    assert cfg["exchange_collectives_per_layer"] == 4 and cfg["exchange_exposed"]["waits_per_step"] == 2 * (2 * 2 - 1)   # fwd + back waits per element-layer
    assert cfg["result_preserving_prunings"] == {"last_layer_noise_rows_only": True, "cfg_pair_layer0_once": True}
    assert eight["roofline"]["launches_timed"] == 2 * 2 - 1                       # per CFG element and layer, layer 0 once (cfg pair)
    assert abs(cfg["x_abs_mean"] - one["config"]["x_abs_mean"]) < 2e-3 * one["config"]["x_abs_mean"]


def test_bench_config5_line_reduced_layers():
    """BASELINE config 5 (2 reference frames + 2 pose streams in one token sequence, L = 60 032: the long-sequence self-attention stress) through
    `bench.py --config 14b-2char` at full width and full length with 2 of the 40 layers, so that GPUTEST exercises the code path behind the
    builder's config-5 number.  The line must say what it is: an EXTENSION (the reference has one reference frame and one pose stream,
    dit...:1559) whose parity is unpinned by construction, and a debug layer count."""
    o = _run([sys.executable, "bench.py", "--config", "14b-2char", "--layers", "2", "--steps", "1", "--warmup", "1", "--no-vae", "--no-cpu-baseline"],
             timeout=900)
    cfg = o["config"]
    assert "EXTENSION_not_in_reference" in cfg and "unpinned by construction" in cfg["EXTENSION_not_in_reference"]
    assert cfg["INVALID_debug_layers"] == 2 and cfg["finite"] and "L=60032" in cfg["workload"]
    assert cfg["path"].startswith("scail_dit_block per layer (C executor)")
    assert o["roofline"]["launches_timed"] == 2 and o["roofline"]["achieved"] > 500.0        # the 4-wave kernel at L = 60 032 (measured 1 646 TFLOP/s)


def test_fullsize_request_two_steps():
    """BASELINE config-2 SIZES end to end through the driver (SCAIL-14B shapes, 512x896x81f, random-init weights, 2 of the 50
    sampler steps): VAE encode of the reference frame and the pose clip, the C-level sampler loop, VAE decode.  Guards the
    full-size-only failure modes (workspace sizing, 32-bit offsets, tile counts) that the toy configurations cannot reach."""
    r = subprocess.run([sys.executable, "tools/e2e_fullsize.py", "2"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    o = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert o["latent"] == [1, 16, 21, 64, 112] and o["video"] == [1, 3, 81, 512, 896]
    assert o["finite"] and 0.0 <= o["vmin"] and o["vmax"] <= 1.0


def test_cli_two_ranks_one_gpu(tmp_path):
    """The CLI under the multi-rank launch line (sequence parallel over the token axis; both ranks on GPU 0 with host-staged
    exchanges): rank 0 writes the same video as the single-process run, up to bf16 re-association."""
    import numpy as np
    from PIL import Image
    from scail_amd import video_io
    d = tmp_path / "001"
    d.mkdir()
    g = np.random.default_rng(1)
    Image.fromarray(g.integers(0, 255, (72, 96, 3), dtype=np.uint8)).save(d / "ref.png")
    np.save(d / "rendered.npy", g.integers(0, 255, (9, 72, 96, 3), dtype=np.uint8))
    args = ["--tiny", "--steps", "2", "--request", f"a girl is dancing@@{d}", "--format", ".png"]

    def go(cmd, out, env_extra=None):
        env = dict(os.environ)
        env.update(env_extra or {})
        r = subprocess.run(cmd + args + ["--output-dir", str(out)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return video_io.load_video_for_pose_sample(str(out / "001" / "001_output_000000.png")).float()

    one = go([sys.executable, "-m", "scail_amd.cli"], tmp_path / "one")
    two = go([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
              "--master-port", "29643", "-m", "scail_amd.cli"], tmp_path / "two", {"SCAIL_DIST_BACKEND": "gloo"})
    assert one.shape == two.shape == (9, 64, 64, 3)
    assert float((one - two).abs().mean()) < 2.0 and float((one - two).abs().max()) <= 40.0      # 8-bit levels
