"""The solver plan (include/scail_dit.h "solver plan") where it needs no device: the host planner against the lambda-form of
DPM-Solver++(2M) restated here in fp64, what the table is for on a problem with a closed form, every refusal by its message, and the
C entries' refusals that come before a device is touched."""
import ctypes as C
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_HIP = ["scail_cfg_multistep", "scail_tile_finish_multistep"]
NEW_DIT = ["scail_dit_solver_bytes", "scail_dit_sample_solver", "scail_dit_sample_tiled_solver"]
SIG6 = [1.0, 0.9, 0.75, 0.6, 0.4, 0.2, 0.0]


def shipped(n, shift=7):
    """the shipped schedule (host fp32) as Python floats"""
    from scail_amd.sampler import make_flow_timesteps
    return [float(v) for v in make_flow_timesteps(0, n, shift_scale=shift)]


SCHEDULES = [("shipped4", lambda: shipped(4)), ("shipped6", lambda: shipped(6)), ("shipped10", lambda: shipped(10)),
             ("shipped50", lambda: shipped(50)), ("SIG6", lambda: list(SIG6))]


# ---- the planner against the lambda-form ---------------------------------------------------------------------------------------------------
def lam(s):
    return -math.inf if s == 1.0 else math.inf if s == 0.0 else math.log((1.0 - s) / s)


def lambda_form(sig, second_order=True):
    """DPM-Solver++(2M) as published, in lambda: x' = (sigma' / sigma) x - alpha' expm1(-h) [D + (1 / (2 r)) (D - D_prev)], as rows
    (a, b, c) of x' = a x + b D + c D_prev.  A step that starts at sigma = 1 or ends at sigma = 0 has h = inf: expm1(-h) = -1."""
    rows = []
    for i in range(len(sig) - 1):
        s0, s1 = sig[i], sig[i + 1]
        h = lam(s1) - lam(s0)
        k = -(1.0 - s1) * math.expm1(-h)           # the factor of the bracket
        if second_order and i >= 1 and all(math.isfinite(lam(sig[j])) for j in (i - 1, i, i + 1)):
            r = (lam(s0) - lam(sig[i - 1])) / h
            rows.append((s1 / s0, k * (1.0 + 1.0 / (2.0 * r)), -k / (2.0 * r)))
        else:
            rows.append((s1 / s0, k, 0.0))
    return rows


@pytest.mark.parametrize("name, make", SCHEDULES)
def test_plan_matches_the_lambda_form(name, make):
    from scail_amd.sampler import plan_solver
    sig = make()
    for solver, second in (("dpmpp2m", True), ("dpm1", False)):
        plan, want = plan_solver(sig, solver), lambda_form(sig, second)
        assert len(plan) == len(sig) - 1 == len(want)
        worst = max(abs(p - w) for rp, rw in zip(plan, want) for p, w in zip(rp, rw))
        print(f"{name} {solver}: max |plan - lambda form| = {worst:.3e}")
        assert worst <= 1e-12
        for row in plan:
            assert abs(sum(row) - 1.0) <= 1e-15, row
        assert plan[-1] == (0.0, 1.0, 0.0)


@pytest.mark.parametrize("make, second", [
    (lambda: shipped(4), [2]), (lambda: shipped(6), [2, 3, 4]), (lambda: shipped(10), list(range(2, 9))),
    (lambda: shipped(50), list(range(2, 49))), (lambda: list(SIG6), [2, 3, 4])])
def test_which_steps_are_second_order(make, second):
    from scail_amd.sampler import plan_solver, solver_uses_prev
    plan = plan_solver(make(), "dpmpp2m")
    assert [i for i, row in enumerate(plan) if row[2] != 0.0] == second
    assert [i for i, row in enumerate(plan) if solver_uses_prev(row)] == second
    assert len(second) in (1, 3, 7, 47)
    assert all(row[2] == 0.0 for row in plan_solver(make(), "dpm1"))


def test_plan_takes_the_host_tensor():
    from scail_amd.sampler import RFSampler, plan_solver
    sig = RFSampler(hunyuan_schedule=True, shift_scale=7, num_steps=10).sigmas()
    assert plan_solver(sig, "dpmpp2m") == plan_solver([float(v) for v in sig], "dpmpp2m")
    assert len(plan_solver([0.5, 0.25], "dpmpp2m")) == 1 and plan_solver([0.5, 0.25], "dpmpp2m")[0] == (0.5, 0.5, 0.0)


# ---- what the solver is for: a problem with a closed form ---------------------------------------------------------------------------------
def velocity(x, s, sd):
    """data N(0, sd^2) under x_sigma = (1 - sigma) x0 + sigma eps: the exact v = E[eps - x0 | x]"""
    al = 1.0 - s
    return x * (s - al * sd * sd) / (al * al * sd * sd + s * s)


def integrate(sig, plan, sd):
    x, prev = 1.0, 0.0
    for i, (a, b, c) in enumerate(plan):
        D = x - sig[i] * velocity(x, sig[i], sd)
        x, prev = a * x + b * D + c * prev, D
    return x


def euler(sig, sd):
    x = 1.0
    for i in range(len(sig) - 1):
        x = x + (sig[i + 1] - sig[i]) * velocity(x, sig[i], sd)
    return x


@pytest.mark.parametrize("sd", [0.5, 1.0, 2.0])
def test_second_order_beats_first_order_on_a_gaussian(sd):
    from scail_amd.sampler import plan_solver
    for n in (10, 20, 40, 80):
        sig = shipped(n)
        e2 = abs(integrate(sig, plan_solver(sig, "dpmpp2m"), sd) - sd)       # the exact solution from x(1) = 1 is x(0) = sd
        x1 = integrate(sig, plan_solver(sig, "dpm1"), sd)
        e1 = abs(x1 - sd)
        print(f"sd {sd} N {n}: |err| dpmpp2m {e2:.3e}  dpm1 {e1:.3e}  ratio {e2 / e1 if e1 else float('nan'):.3f}")
        assert e2 < e1
        if n in (40, 80):
            assert e2 <= 0.5 * e1
        assert abs(x1 - euler(sig, sd)) <= 1e-12


# ---- the planner's refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sig, solver, needle", [
    (SIG6, "unipc", r"plan_solver: unknown solver 'unipc'"),
    (SIG6, None, r"plan_solver: unknown solver None"),
    ([1.0], "dpmpp2m", r"at least 2 sigmas \(one step\), got 1"),
    ([], "dpm1", r"at least 2 sigmas \(one step\), got 0"),
    ([1.0, 0.5, 0.5, 0.0], "dpmpp2m", r"strictly decreasing, got sigma\[1\] = 0.5 then sigma\[2\] = 0.5"),
    ([0.2, 0.6, 0.0], "dpmpp2m", r"strictly decreasing, got sigma\[0\] = 0.2 then sigma\[1\] = 0.6"),
    ([1.5, 0.5, 0.0], "dpmpp2m", r"sigma\[0\] = 1.5 lies outside \[0, 1\]"),
    ([1.0, 0.5, -0.25], "dpmpp2m", r"sigma\[2\] = -0.25 lies outside \[0, 1\]"),
    ([1.0, float("nan"), 0.0], "dpmpp2m", r"sigma\[1\] = nan lies outside \[0, 1\]"),
    ([1.0, 0.0, 0.0], "dpmpp2m", r"sigma\[1\] = 0 is not the last value"),
    ([0.0, 0.5], "dpm1", r"sigma\[0\] = 0 is not the last value"),
])
def test_plan_refusals(sig, solver, needle):
    from scail_amd.sampler import plan_solver
    with pytest.raises(ValueError, match=needle):
        plan_solver(sig, solver)


# ---- the library ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from scail_amd import build
    from scail_amd import lib as L
    build.build(verbose=False)
    return L.load()


def _decls(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(scail_[a-z0-9_]+)\s*\(", src))


def test_symbols_declared_exported_bound(lib):
    from scail_amd import lib as L
    assert set(NEW_HIP) <= _decls("scail_hip.h") and set(NEW_DIT) <= _decls("scail_dit.h")
    for name in NEW_HIP + NEW_DIT:
        assert name in L.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.argtypes == L.SIGNATURES[name]
        assert fn.restype is (C.c_int64 if name.endswith("_bytes") else C.c_int), name
    assert lib.scail_abi_version() == 8 == L.ABI_VERSION, "only entry points were added"


def test_solver_bytes(lib):
    assert lib.scail_dit_solver_bytes(3, 8, 20) == 3 * 16 * 8 * 20 * 4
    assert lib.scail_dit_solver_bytes(1, 4, 4) == 1024
    assert lib.scail_dit_solver_bytes(1, 4, 12) == 3072
    # the FULL latent of a tiled clip: no single evaluation's token limit applies
    assert lib.scail_dit_solver_bytes(501, 64, 112) == 501 * 16 * 64 * 112 * 4
    for bad in ((0, 8, 20), (3, 0, 20), (3, 8, 0), (3, 6, 20), (3, 8, 18), (-1, 8, 20), (1 << 15, 8, 20), (3, 1 << 15, 20)):
        assert lib.scail_dit_solver_bytes(*bad) == -1, bad


A = 0x10000        # a fake, 256-byte aligned device address: every refusal below comes before it could be dereferenced


def test_row_kernels_refuse_on_the_host(lib):
    from scail_amd import lib as L
    co = (4.0, 0.5, 0.5, 0.75, -0.25, 1, None)
    cases = [
        (r"scail_cfg_multistep: n must be .* got -1", "scail_cfg_multistep", (A, A, A, -1) + co),
        (r"scail_cfg_multistep: n must be .* got 549755813888", "scail_cfg_multistep", (A, A, A, 1 << 39) + co),
        (r"scail_cfg_multistep: null pointer: x \(n = 7\)", "scail_cfg_multistep", (None, A, A, 7) + co),
        (r"scail_cfg_multistep: null pointer: v \(n = 7\)", "scail_cfg_multistep", (A, None, A, 7) + co),
        (r"scail_cfg_multistep: null pointer: hist \(n = 7\)", "scail_cfg_multistep", (A, A, None, 7) + co),
        (r"scail_cfg_multistep: null pointer: hist \(n = 7\)", "scail_cfg_multistep", (A, A, None, 7, 4.0, 0.5, 0.5, 0.5, 0.0, 0, None)),
        (r"scail_tile_finish_multistep: bad frame size F = -1", "scail_tile_finish_multistep", (A, A, A, A, 3, -1) + co[1:]),
        (r"scail_tile_finish_multistep.*bad frame count", "scail_tile_finish_multistep", (A, A, A, A, -1, 16) + co[1:]),
        (r"scail_tile_finish_multistep.*null pointer", "scail_tile_finish_multistep", (A, A, A, None, 3, 16) + co[1:]),
        (r"scail_tile_finish_multistep.*null pointer", "scail_tile_finish_multistep", (A, A, None, A, 3, 16) + co[1:]),
    ]
    for needle, name, args in cases:
        with pytest.raises(L.ScailHipError, match=needle):
            L.call(name, *args)
    # n == 0 launches nothing and needs no device, whatever the pointers
    L.call("scail_cfg_multistep", None, None, None, 0, *co)
    L.call("scail_tile_finish_multistep", A, A, (C.c_float * 3)(1.0, 1.0, 1.0), A, 3, 0, *co[1:])


def _f32(vals):
    vals = list(vals)
    return (C.c_float * max(len(vals), 1))(*vals)


GOOD_SIGMA = [1.0, 0.9, 0.75]
GOOD_COEF = [0.9, 0.1, 0.0, 0.8, 0.2, 0.0, 0.8, 0.3, -0.1]
NEED = 3 * 16 * 8 * 20 * 4


def _solver(sigma=GOOD_SIGMA, coef=GOOD_COEF, n_steps=None, hist=A, hist_bytes=NEED):
    n_steps = len(sigma) if n_steps is None else n_steps
    return ("scail_dit_sample_solver", None, A, A, A, n_steps, 4.0, A, A, A, 1, 3, A, A, 3, 8, 20, A, 1 << 20,
            None if sigma is None else _f32(sigma), None if coef is None else _f32(coef), hist, hist_bytes, None)


def _tiled(sigma=GOOD_SIGMA, coef=GOOD_COEF, n_steps=None, hist=A, hist_bytes=5 * 16 * 8 * 20 * 4, n_tiles=2, frames=(0, 1, 2, 2, 3, 4),
           ws_bytes=1 << 30):
    n_steps = len(sigma) if n_steps is None else n_steps
    fr = (C.c_int32 * len(frames))(*frames)
    tw, iw = _f32([1.0] * len(frames)), _f32([1.0, 1.0, 0.5, 1.0, 1.0])
    return ("scail_dit_sample_tiled_solver", None, A, A, A, n_steps, 4.0, A, A, A, fr, tw, iw, n_tiles, 5, 3, A, A, 8, 20, A, ws_bytes,
            None if sigma is None else _f32(sigma), None if coef is None else _f32(coef), hist, hist_bytes, None)


@pytest.mark.parametrize("make, who", [(_solver, "scail_dit_sample_solver"), (_tiled, "scail_dit_sample_tiled_solver")])
def test_sample_solver_refuses_a_bad_plan_or_history(lib, make, who):
    from scail_amd import lib as L
    need = NEED if make is _solver else 5 * 16 * 8 * 20 * 4
    inf, nan = float("inf"), float("nan")
    with pytest.raises(L.ScailHipError, match=rf"{who}: sigma\[1\] = nan is not finite"):
        L.call(*make(sigma=[1.0, nan, 0.75]))
    with pytest.raises(L.ScailHipError, match=rf"{who}: sigma\[2\] = -?inf is not finite"):
        L.call(*make(sigma=[1.0, 0.9, inf]))
    bad = list(GOOD_COEF)
    bad[4] = inf
    with pytest.raises(L.ScailHipError, match=rf"{who}: coef\[1\]\[1\] = inf is not finite"):
        L.call(*make(coef=bad))
    bad = list(GOOD_COEF)
    bad[8] = nan
    with pytest.raises(L.ScailHipError, match=rf"{who}: coef\[2\]\[2\] = nan is not finite"):
        L.call(*make(coef=bad))
    bad = list(GOOD_COEF)
    bad[2] = -0.125
    with pytest.raises(L.ScailHipError, match=rf"{who}: coef\[0\]\[2\] = -0.125000 must be 0: step 0 has no history"):
        L.call(*make(coef=bad))
    with pytest.raises(L.ScailHipError, match=rf"{who}: n_steps must be >= 0, got -2"):
        L.call(*make(n_steps=-2))
    with pytest.raises(L.ScailHipError, match=rf"{who}: null solver sigma with n_steps = 3"):
        L.call(*make(sigma=None, n_steps=3))
    with pytest.raises(L.ScailHipError, match=rf"{who}: null solver coefficients with n_steps = 3"):
        L.call(*make(coef=None))
    with pytest.raises(L.ScailHipError, match=rf"{who}: null history buffer \(hist_bytes 4096; scail_dit_solver_bytes\)"):
        L.call(*make(hist=None, hist_bytes=4096))
    with pytest.raises(L.ScailHipError, match=r"the history buffer must be 256-byte aligned.*is 64 past"):
        L.call(*make(hist=A + 64))
    with pytest.raises(L.ScailHipError, match=rf"history buffer too small: {need - 1} bytes, needs {need} \(scail_dit_solver_bytes\)"):
        L.call(*make(hist_bytes=need - 1))


def test_sample_solver_then_refuses_what_its_twin_refuses(lib):
    from scail_amd import lib as L
    # a well-formed plan and buffer get as far as the handle, in scail_dit_sample_chars' wording
    with pytest.raises(L.ScailHipError, match="null argument"):
        L.call(*_solver())
    args = list(_solver())
    args[10] = 0                                          # n_char
    with pytest.raises(L.ScailHipError, match=r"n_char must be 1..64, got 0"):
        L.call(*args)


def test_sample_tiled_solver_then_refuses_what_its_twin_refuses(lib):
    from scail_amd import lib as L
    who = "scail_dit_sample_tiled_solver"
    with pytest.raises(L.ScailHipError, match=rf"{who}: needs at least 2 tiles .* got n_tiles = 1"):
        L.call(*_tiled(n_tiles=1))
    with pytest.raises(L.ScailHipError, match=rf"{who}: tile 1: frame index 7 .* is outside \[0, T = 5\)"):
        L.call(*_tiled(frames=(0, 1, 2, 2, 3, 7)))
    with pytest.raises(L.ScailHipError, match=rf"{who}: frame 4 of \[0, T = 5\) is covered by no tile"):
        L.call(*_tiled(frames=(0, 1, 2, 1, 2, 3)))
    with pytest.raises(L.ScailHipError, match=rf"{who}: workspace too small: 4096 bytes cannot hold"):
        L.call(*_tiled(ws_bytes=4096))
    with pytest.raises(L.ScailHipError, match=rf"{who}: null pointer: handle"):
        L.call(*_tiled())


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------------
def test_cli_parses_the_flag():
    from scail_amd import cli
    a = cli.build_parser().parse_args([])
    assert a.solver == "euler" and cli.solver_args(a.solver) is None and cli.solver_args(None) is None
    a = cli.build_parser().parse_args(["--solver", "dpmpp2m"])
    assert cli.solver_args(a.solver) == "dpmpp2m"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--solver", "unipc"])
    with pytest.raises(ValueError, match="--solver must be one of"):
        cli.solver_args("unipc")
    with pytest.raises(ValueError, match="--solver dpmpp2m does not go with --step-cache-threshold"):
        cli.solver_args("dpmpp2m", step_cache={"threshold": 0.1})
    with pytest.raises(ValueError, match="--solver dpmpp2m does not go with --cfg-interval"):
        cli.solver_args("dpmpp2m", guidance={"every": 2})


def test_cli_prints_the_plan():
    from scail_amd import cli
    from scail_amd.sampler import plan_solver
    text = cli.format_solver_plan(plan_solver(SIG6, "dpmpp2m"))
    assert text.startswith("solver plan (dpmpp2m): 3 of 6 steps are second order (2, 3, 4); the others are first order")
    assert "47 of 50 steps are second order" in cli.format_solver_plan(plan_solver(shipped(50), "dpmpp2m"))


def test_cli_argument_errors_come_before_any_model(capsys):
    from scail_amd import cli
    with pytest.raises(SystemExit):
        cli.main(["--tiny", "--solver", "dpmpp2m", "--step-cache-threshold", "0.1"])
    assert "does not go with --step-cache-threshold" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["--tiny", "--solver", "dpmpp2m", "--cfg-delta-every", "2"])
    assert "does not go with --cfg-interval" in capsys.readouterr().err


# ---- the samplers' routing, on a stand-in network -----------------------------------------------------------------------------------------
class _Net:
    """records what the samplers hand the network's one-call loops"""

    def __init__(self, ok=True):
        self.ok, self.calls = ok, []

    def executor_ok(self, whole_loop=False):
        return self.ok

    def sample_c(self, x, sig, cfg, ctx, ref, pose, clip, cond_key=None, **kw):
        self.calls.append(kw)
        return x

    def sample_tiled_c(self, x, sig, cfg, ctx, ref, pose_tiles, clip, tiles, tile_w, inv_wsum, cond_key=None, **kw):
        self.calls.append(kw)
        return x


def _request():
    import torch
    shared = dict(concat_images=torch.zeros(1), ref_concat=torch.zeros(1, 1, 16, 8, 20), concat_smpl_render=torch.zeros(1, 3, 16, 4, 10),
                  image_clip_features=torch.zeros(1, 5, 1280))
    return torch.zeros(1, 3, 16, 8, 20), dict(crossattn=torch.zeros(1, 12, 64), **shared), dict(crossattn=torch.ones(1, 12, 64), **shared)


def _tiled_request():
    import torch
    x, c, uc = _request()
    return x, dict(c, smpl_tiled=torch.zeros(1, 2, 2, 16, 4, 10)), uc, [[0, 1], [1, 2]]


def test_sample_hip_without_the_option_takes_todays_route():
    from scail_amd.sampler import RFSampler, RFSamplerLong
    x, c, uc = _request()
    net, s = _Net(), RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=6)
    s.sample_hip(net, x, c, uc, scale=4.0)
    s.sample_hip(net, x, c, uc, scale=4.0, solver=None)
    assert net.calls == [{}, {}] and not hasattr(s, "last_solver_plan")
    x, c, uc, tiles = _tiled_request()
    long = RFSamplerLong(hunyuan_schedule=True, shift_scale=5, num_steps=2)
    long.sample_hip(net, x, c, uc, tile_indices=tiles, solver=None)
    assert net.calls[-1] == {} and not hasattr(long, "last_solver_plan")


def test_sample_hip_plans_and_takes_the_solver_route():
    import torch
    from scail_amd.sampler import RFSampler, RFSamplerLong, plan_solver
    x, c, uc = _request()
    net, s = _Net(), RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=6)
    for name in ("dpmpp2m", "dpm1"):
        s.sample_hip(net, x, c, uc, scale=4.0, solver=name)
        assert s.last_solver_plan == plan_solver(s.sigmas(), name)
        (sigma, coef), = [net.calls[-1]["solver"]]
        assert list(net.calls[-1]) == ["solver"] and torch.equal(sigma, s.sigmas()[:-1]) and coef == s.last_solver_plan
    x, c, uc, tiles = _tiled_request()
    long = RFSamplerLong(hunyuan_schedule=True, shift_scale=5, num_steps=4)
    long.sample_hip(net, x, c, uc, tile_indices=tiles, solver="dpmpp2m")
    assert long.last_solver_plan == plan_solver(long.sigmas(), "dpmpp2m") and net.calls[-1]["solver"][1] == long.last_solver_plan


def test_python_layers_refuse_what_the_plan_does_not_cover():
    from scail_amd.sampler import RFSampler, RFSamplerLong
    x, c, uc = _request()
    net, s = _Net(), RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=6)
    with pytest.raises(ValueError, match=r"solver: unknown solver 'unipc'"):
        s.sample_hip(net, x, c, uc, scale=4.0, solver="unipc")
    with pytest.raises(NotImplementedError, match="solver together with step_cache is out of scope"):
        s.sample_hip(net, x, c, uc, scale=4.0, solver="dpmpp2m", step_cache=dict(mask=[0, 1, 0, 1, 0, 1]))
    with pytest.raises(NotImplementedError, match="solver together with guidance is out of scope"):
        s.sample_hip(net, x, c, uc, scale=4.0, solver="dpmpp2m", guidance=dict(every=2))
    with pytest.raises(NotImplementedError, match=r"solver runs on a single rank only: not on sequence-parallel ranks \(chunk_dim\)"):
        s.sample_hip(net, x, c, uc, scale=4.0, solver="dpmpp2m", chunk_dim=3)
    x, c, uc, tiles = _tiled_request()
    long = RFSamplerLong(hunyuan_schedule=True, shift_scale=5, num_steps=2)
    with pytest.raises(ValueError, match=r"solver: unknown solver 'euler'"):
        long.sample_hip(net, x, c, uc, tile_indices=tiles, solver="euler")
    with pytest.raises(NotImplementedError, match="solver together with step_cache is out of scope"):
        long.sample_hip(net, x, c, uc, tile_indices=tiles, solver="dpm1", step_cache=dict(mask=[0, 1]))
    with pytest.raises(NotImplementedError, match="solver together with guidance is out of scope"):
        long.sample_hip(net, x, c, uc, tile_indices=tiles, solver="dpm1", guidance=dict(every=2))
    with pytest.raises(NotImplementedError, match=r"solver runs on a single rank only: not on sequence-parallel ranks \(chunk_dim\)"):
        long.sample_hip(net, x, c, uc, tile_indices=tiles, solver="dpm1", chunk_dim=4)
    assert net.calls == []


def test_network_and_executor_layers_refuse_a_combination():
    from scail_amd.cstep import CStep
    from scail_amd.dit import DiffusionTransformer
    from scail_amd import lib as L
    with pytest.raises(L.ScailHipError, match=r"solver: needs one starting sigma and one \(a, b, c\) per step \(3\), got 2 sigmas and 3 rows"):
        CStep.solver_tables(([1.0, 0.5], [(0.5, 0.5, 0.0)] * 3), 3)
    with pytest.raises(L.ScailHipError, match=r"got 3 sigmas and 3 rows"):
        CStep.solver_tables(([1.0, 0.5, 0.2], [(0.5, 0.5, 0.0), (0.5, 0.5), (0.5, 0.5, 0.0)]), 3)
    sg, co = CStep.solver_tables(([1.0, 0.5], [(0.5, 0.5, 0.0), (0.25, 1.0, -0.25)]), 2)
    assert list(sg) == [1.0, 0.5] and list(co) == [0.5, 0.5, 0.0, 0.25, 1.0, -0.25]
    import inspect
    assert "solver" in inspect.signature(DiffusionTransformer.sample_c).parameters
    assert "solver" in inspect.signature(DiffusionTransformer.sample_tiled_c).parameters
