"""The step cache without a device: the host plan (sampler.plan_step_cache), the new symbols of the library and their binding, every
refusal that needs neither a handle nor a GPU, the CLI flags, and that ``step_cache=None`` leaves RFSampler.sample_hip on today's route."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_HIP = ("scail_resid_store", "scail_resid_apply", "scail_abs_diff_sums")
NEW_DIT = ("scail_dit_step_cache_bytes", "scail_dit_step_cached", "scail_dit_sample_cached", "scail_dit_time_distances",
           "scail_dit_time_distances_bytes")


# ---- plan_step_cache: hand-computed masks ------------------------------------------------------------------------------------------------
def _dist(ds):
    """a distance table whose ratios are ``ds`` (row 0 is the executor's {0, 0})"""
    return [(0.0, 0.0)] + [(d * 4.0, 4.0) for d in ds]


def test_plan_worked_example():
    from scail_amd.sampler import plan_step_cache
    # acc: .125 .25 | .375 >= .3 -> compute | .125 | last step is kept
    assert plan_step_cache(_dist([0.125] * 5), 0.3) == [0, 1, 1, 0, 1, 0]


def test_plan_threshold_zero_and_huge():
    from scail_amd.sampler import plan_step_cache
    d = _dist([0.125] * 7)
    assert plan_step_cache(d, 0.0) == [0] * 8
    assert plan_step_cache(d, 1e30) == [0, 1, 1, 1, 1, 1, 1, 0]
    assert plan_step_cache(d, 1e30, keep_last=0) == [0, 1, 1, 1, 1, 1, 1, 1]
    assert plan_step_cache([], 0.5) == [] and plan_step_cache(_dist([]), 0.5) == [0]


def test_plan_keep_edges():
    from scail_amd.sampler import plan_step_cache
    d = _dist([0.125] * 7)
    assert plan_step_cache(d, 1e30, keep_first=3, keep_last=2) == [0, 0, 0, 1, 1, 1, 0, 0]
    assert plan_step_cache(d, 1e30, keep_first=8, keep_last=0) == [0] * 8
    assert plan_step_cache(d, 1e30, keep_first=5, keep_last=5) == [0] * 8                  # the two ranges overlap
    # a kept step resets the accumulator: .125 (reuse), .25 (reuse), kept step 3, then .125, .25 again -- never .375
    assert plan_step_cache(d, 0.3, keep_first=1, keep_last=0) == [0, 1, 1, 0, 1, 1, 0, 1]
    assert plan_step_cache(d, 0.3, keep_first=4, keep_last=0) == [0, 0, 0, 0, 1, 1, 0, 1]


def test_plan_zero_denominator_computes():
    from scail_amd.sampler import plan_step_cache
    d = [(0.0, 0.0), (0.5, 4.0), (0.5, 0.0), (0.5, 4.0), (0.5, 4.0), (0.5, 4.0)]
    # step 2 has no denominator: it computes and resets, so step 3 starts from .125 again
    assert plan_step_cache(d, 0.2, keep_last=0) == [0, 1, 0, 1, 0, 1]


def test_plan_coefficients_horner():
    from scail_amd.sampler import plan_step_cache
    d = _dist([0.5] * 5)
    # p(d) = 2 d^2 + 0.25 = 0.75 per step: .75 | 1.5 >= 1 -> compute | .75 | 1.5 -> compute | last
    assert plan_step_cache(d, 1.0, coefficients=(2.0, 0.0, 0.25)) == [0, 1, 0, 1, 0, 0]
    # a constant polynomial ignores the distances: 0.4 per step, threshold 1 -> two reuses, then compute
    assert plan_step_cache(_dist([7.0] * 6), 1.0, coefficients=(0.4,), keep_last=0) == [0, 1, 1, 0, 1, 1, 0]
    # the identity, spelled out, is the default
    assert plan_step_cache(d, 0.6, coefficients=(0.0, 1.0, 0.0)) == plan_step_cache(d, 0.6) == [0, 1, 0, 1, 0, 0]


def test_plan_takes_tensors_and_is_fp64():
    from scail_amd.sampler import plan_step_cache
    t = torch.tensor(_dist([0.1] * 4), dtype=torch.float64)
    # 0.1 + 0.1 + 0.1 in fp64 is 0.30000000000000004 >= 0.3
    assert plan_step_cache(t, 0.3, keep_last=0) == [0, 1, 1, 0, 1]


@pytest.mark.parametrize("kw,needle", [
    (dict(threshold=-0.1), "threshold"), (dict(threshold=float("nan")), "threshold"),
    (dict(threshold=0.1, keep_first=0), "keep_first"), (dict(threshold=0.1, keep_first=1.5), "keep_first"),
    (dict(threshold=0.1, keep_last=-1), "keep_last"), (dict(threshold=0.1, coefficients=()), "coefficients"),
    (dict(threshold=0.1, coefficients=(float("inf"), 0.0)), "coefficients")])
def test_plan_bad_arguments(kw, needle):
    from scail_amd.sampler import plan_step_cache
    with pytest.raises(ValueError, match=needle):
        plan_step_cache(_dist([0.1] * 3), **kw)


def test_plan_bad_table():
    from scail_amd.sampler import plan_step_cache
    with pytest.raises(ValueError, match="dist"):
        plan_step_cache([(0.0, 0.0), (float("nan"), 1.0)], 0.1)
    with pytest.raises(ValueError, match="dist"):
        plan_step_cache([(0.0, 0.0), (-1.0, 1.0)], 0.1)


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
    assert lib.scail_abi_version() == 8 == L.ABI_VERSION
    assert L.CACHE_MODES == {"fill": 1, "reuse": 2} and L.CACHE_SIGNALS == {"time": 0, "modulation": 1}
    hdr = open(os.path.join(ROOT, "include", "scail_dit.h")).read()
    assert "#define SCAIL_DIT_CACHE_FILL 1" in hdr and "#define SCAIL_DIT_CACHE_REUSE 2" in hdr


def test_queries_refuse_a_null_handle(lib):
    assert lib.scail_dit_step_cache_bytes(None, 2, 3, 8, 20) == -1
    assert lib.scail_dit_time_distances_bytes(None, 0) == -1 and lib.scail_dit_time_distances_bytes(None, 1) == -1


A = 0x10000        # a fake, 256-byte aligned device address: every refusal below comes before it could be dereferenced


def _step_cached(mode, cache, cache_bytes=1 << 20):
    return ("scail_dit_step_cached", None, A, A, None, A, 1, A, 1, 1, 3, A, A, A, 2, 3, 8, 20, 0, A, 1 << 20, mode, cache, cache_bytes, None)


def _sample_cached(reuse, n_steps, cache=A):
    mask = None if reuse is None else (C.c_uint8 * len(reuse))(*reuse)
    return ("scail_dit_sample_cached", None, A, A, A, n_steps, 4.0, A, A, A, 1, 3, A, A, 3, 8, 20, A, 1 << 20, mask, cache, 1 << 20, None)


@pytest.mark.parametrize("mode", [0, 3, -1, 7])
def test_step_cached_refuses_an_unknown_mode(lib, mode):
    from scail_amd import lib as L
    with pytest.raises(L.ScailHipError, match=rf"unknown cache mode {mode} "):
        L.call(*_step_cached(mode, A))


def test_step_cached_refuses_a_null_or_misaligned_cache(lib):
    from scail_amd import lib as L
    for mode in (1, 2):
        with pytest.raises(L.ScailHipError, match=r"scail_dit_step_cached: null cache \(cache_bytes 4096"):
            L.call(*_step_cached(mode, None, 4096))
        with pytest.raises(L.ScailHipError, match=r"256-byte aligned.*is 128 past"):
            L.call(*_step_cached(mode, A + 128))
        with pytest.raises(L.ScailHipError, match=r"256-byte aligned.*is 16 past"):
            L.call(*_step_cached(mode, A + 16))
        # a well-formed mode and cache get as far as the handle
        with pytest.raises(L.ScailHipError, match="null handle"):
            L.call(*_step_cached(mode, A))


def test_sample_cached_refuses_bad_masks(lib):
    from scail_amd import lib as L
    with pytest.raises(L.ScailHipError, match=r"reuse\[0\] = 1: the first step has nothing to reuse"):
        L.call(*_sample_cached([1, 0, 0], 3))
    with pytest.raises(L.ScailHipError, match=r"reuse\[2\] = 2 \(an entry is 0 = compute or 1 = reuse\)"):
        L.call(*_sample_cached([0, 1, 2, 0], 4))
    with pytest.raises(L.ScailHipError, match=r"reuse\[1\] = 255"):
        L.call(*_sample_cached([0, 255], 2))
    with pytest.raises(L.ScailHipError, match=r"null reuse mask with n_steps = 5"):
        L.call(*_sample_cached(None, 5))
    with pytest.raises(L.ScailHipError, match=r"scail_dit_sample_cached: null cache"):
        L.call(*_sample_cached([0, 1], 2, cache=None))
    with pytest.raises(L.ScailHipError, match=r"256-byte aligned.*is 64 past"):
        L.call(*_sample_cached([0, 1], 2, cache=A + 64))
    with pytest.raises(L.ScailHipError, match="null handle"):
        L.call(*_sample_cached([0, 1], 2))


def test_time_distances_refusals(lib):
    from scail_amd import lib as L
    with pytest.raises(L.ScailHipError, match=r"unknown signal 2 "):
        L.call("scail_dit_time_distances", None, A, 4, 2, A, A, 1 << 20, None)
    with pytest.raises(L.ScailHipError, match=r"n_steps must be .* got -1"):
        L.call("scail_dit_time_distances", None, A, -1, 0, A, A, 1 << 20, None)
    with pytest.raises(L.ScailHipError, match="null handle"):
        L.call("scail_dit_time_distances", None, A, 4, 1, A, A, 1 << 20, None)


def test_row_kernels_refuse_on_the_host(lib):
    from scail_amd import lib as L
    cases = [
        (r"D must be a multiple of 8 .* got 132", "scail_resid_store", (A, 132 * 4, A, 0, A, 2, 4, 132, None)),
        (r"in_bs must be a non-negative multiple of 8 elements, got 12", "scail_resid_store", (A, 1024, A, 12, A, 2, 4, 128, None)),
        (r"out_bs must be .* got -8", "scail_resid_store", (A, -8, A, 0, A, 2, 4, 128, None)),
        (r"16-byte aligned", "scail_resid_store", (A + 2, 1024, A, 0, A, 2, 4, 128, None)),
        (r"n_batch must be 0..64, got 65", "scail_resid_apply", (A, 0, A, A, 1024, 65, 4, 128, None)),
        (r"h_bs = 256 is smaller than one element's rows \* D = 512", "scail_resid_apply", (A, 0, A + 0x8000, A + 0x10000, 256, 2, 4, 128, None)),
        (r"h overlaps h_in without being h_in \(h - h_in = 128 elements", "scail_resid_apply", (A, 512, A + 0x8000, A + 256, 512, 2, 4, 128, None)),
        (r"h overlaps h_in without being h_in", "scail_resid_apply", (A, 1024, A + 0x8000, A, 512, 2, 4, 128, None)),
        (r"null pointer", "scail_resid_apply", (A, 0, None, A, 512, 2, 4, 128, None)),
        (r"n must be 0 .. 2\^31 - 1, got -3", "scail_abs_diff_sums", (A, A, -3, A, None)),
        (r"8-byte aligned", "scail_abs_diff_sums", (A, A, 8, A + 4, None)),
        (r"4-byte aligned", "scail_abs_diff_sums", (A + 2, A, 8, A, None)),
    ]
    for needle, fn, args in cases:
        with pytest.raises(L.ScailHipError, match=needle):
            L.call(fn, *args)
    # empty problems are accepted and launch nothing
    L.call("scail_resid_store", None, 0, None, 0, None, 0, 4, 128, None)
    L.call("scail_resid_apply", None, 0, None, None, 0, 2, 0, 128, None)


# ---- CLI -----------------------------------------------------------------------------------------------------------------------------------
def test_cli_parses_the_flags():
    from scail_amd import cli
    a = cli.build_parser().parse_args([])
    assert (a.step_cache_threshold, a.step_cache_coefficients, a.step_cache_keep, a.step_cache_signal) == (None, None, None, None)
    assert cli.step_cache_args(None) is None
    a = cli.build_parser().parse_args(["--step-cache-threshold", "0.25", "--step-cache-coefficients", "2,-1.5,0.25", "--step-cache-keep", "3,2",
                                       "--step-cache-signal", "modulation"])
    opt = cli.step_cache_args(a.step_cache_threshold, a.step_cache_coefficients, a.step_cache_keep, a.step_cache_signal)
    assert opt == {"threshold": 0.25, "coefficients": [2.0, -1.5, 0.25], "keep_first": 3, "keep_last": 2, "signal": "modulation"}
    assert cli.step_cache_args(0.5) == {"threshold": 0.5, "signal": "time"}
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--step-cache-signal", "latent"])
    for bad, needle in [((-1.0,), "threshold"), ((0.1, "a,b"), "coefficients"), ((0.1, None, "3"), "keep"), ((0.1, None, "0,1"), "keep"),
                        ((None, "1,0"), "need --step-cache-threshold"), ((None, None, None, "time"), "need --step-cache-threshold")]:
        with pytest.raises(ValueError, match=needle):
            cli.step_cache_args(*bad)


def test_cli_prints_the_plan():
    from scail_amd import cli
    assert cli.format_step_cache_plan([0, 1, 1, 0, 1, 0]).startswith("step cache: 3 of 6 steps compute the blocks (0, 3, 5)")


def test_cli_argument_errors_come_before_any_model(capsys):
    from scail_amd import cli
    with pytest.raises(SystemExit):
        cli.main(["--tiny", "--step-cache-keep", "1,1"])
    assert "need --step-cache-threshold" in capsys.readouterr().err


# ---- the sampler's routes, on a fake network ---------------------------------------------------------------------------------------------
class _FakeNet:
    """stands in for DiffusionTransformer: records which entry of the binding a request would reach"""

    def __init__(self, takes_loop=True):
        self.calls, self.takes_loop = [], takes_loop

    def executor_ok(self, whole_loop=False):
        return self.takes_loop

    def sample_c(self, x, sig, cfg, ctx, ref, pose, clip, cond_key=None, **kw):
        # what DiffusionTransformer.sample_c does with its ``reuse`` argument: CStep.sample without one, CStep.sample_cached with one
        self.calls.append(("CStep.sample_cached", list(kw["reuse"])) if kw.get("reuse") is not None else ("CStep.sample", sorted(kw)))
        return x

    def time_distances(self, timesteps, signal="time"):
        self.calls.append(("time_distances", signal, int(timesteps.numel())))
        return [(0.0, 0.0)] + [(0.5, 4.0)] * (int(timesteps.numel()) - 1)

    def forward_f32(self, xin, t, ctx, y, **kw):
        self.calls.append(("forward_f32", kw.get("step_cache", "absent")))
        return torch.zeros_like(xin)


def _request():
    c = dict(crossattn=torch.zeros(1, 4, 8), ref_concat=torch.zeros(1, 1, 16, 8, 8), concat_smpl_render=torch.zeros(1, 2, 16, 4, 4),
             image_clip_features=torch.zeros(1, 3, 8))
    return torch.zeros(1, 2, 16, 8, 8), c, dict(c)


def _sampler():
    from scail_amd.sampler import RFSampler
    return RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=6)


def test_sample_hip_without_the_option_takes_todays_route():
    net, (x, c, uc) = _FakeNet(), _request()
    _sampler().sample_hip(net, x, c, uc)
    assert net.calls == [("CStep.sample", [])], "step_cache=None must reach sample_c exactly as before: no reuse argument, no distance run"
    _sampler().sample_hip(net, x, c, uc, step_cache=None)
    assert net.calls == [("CStep.sample", [])] * 2


def test_sample_hip_with_the_option_plans_and_takes_the_cached_route():
    net, (x, c, uc) = _FakeNet(), _request()
    s = _sampler()
    s.sample_hip(net, x, c, uc, step_cache=dict(threshold=0.3, signal="modulation"))
    assert net.calls == [("time_distances", "modulation", 6), ("CStep.sample_cached", [0, 1, 1, 0, 1, 0])] and s.last_step_cache_plan == [0, 1, 1, 0, 1, 0]
    net.calls.clear()
    s.sample_hip(net, x, c, uc, step_cache=dict(mask=[0, 1, 0, 1, 1, 0]))
    assert net.calls == [("CStep.sample_cached", [0, 1, 0, 1, 1, 0])]
    # with a step callback the host loop runs: one forward per step, told "fill" or "reuse"
    net.calls.clear()
    import scail_amd.sampler as S
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(S.ops, "cfg_euler_", lambda x, v, cfg, ds: x)
        s.sample_hip(net, x, c, uc, step_cache=dict(mask=[0, 1, 0, 1, 1, 0]), step_callback=lambda i, x: None)
        assert net.calls == [("forward_f32", m) for m in ("fill", "reuse", "fill", "reuse", "reuse", "fill")]
        net.calls.clear()
        s.sample_hip(net, x, c, uc, step_callback=lambda i, x: None)
        assert net.calls == [("forward_f32", "absent")] * 6, "without the option the host loop passes no step_cache key"


def test_sample_hip_refuses_what_the_cache_does_not_cover():
    from scail_amd.sampler import RFSamplerLong
    net, (x, c, uc) = _FakeNet(), _request()
    s = _sampler()
    for bad in ({}, dict(threshold=0.1, foo=1), dict(mask=[0, 1], threshold=0.1), dict(mask=[1, 0, 0, 0, 0, 0]), dict(mask=[0, 1]), dict(signal="time"),
                dict(mask=[0, 2, 0, 0, 0, 0])):
        with pytest.raises(ValueError, match="step_cache"):
            s.sample_hip(net, x, c, uc, step_cache=bad)
    with pytest.raises(NotImplementedError, match="step_cache"):          # sequence-parallel ranks
        s.sample_hip(net, x, c, uc, chunk_dim=3, step_cache=dict(threshold=0.1))
    with pytest.raises(NotImplementedError, match="step_cache"):          # SCAIL_C_STEP=0, _tap, kernel_timer: the network does not take the loop
        s.sample_hip(_FakeNet(takes_loop=False), x, c, uc, step_cache=dict(threshold=0.1))
    long = RFSamplerLong(hunyuan_schedule=True, shift_scale=5, num_steps=6)
    with pytest.raises(NotImplementedError, match="step_cache"):
        long.sample_hip(net, x, c, uc, tile_indices=[[0, 1], [1, 2]], step_cache=dict(threshold=0.1))
    assert net.calls == []


def test_network_refuses_instrumented_and_per_op_runs():
    """DiffusionTransformer's own refusals need no device: they come before any tensor is touched"""
    from scail_amd.dit import DiffusionTransformer
    net = DiffusionTransformer(transformer_args=dict(model_parallel_size=1), hidden_size=128, num_layers=1, num_attention_heads=1, text_dim=64,
                               time_embed_dim=128, time_freq_dim=256, inner_hidden_size=256, share_adaln=True, use_i2v_clip=True, device="cpu")
    for setup in (lambda: setattr(net, "use_c_step", False), lambda: setattr(net, "_tap", lambda i, h: None), lambda: setattr(net, "kernel_timer", {}),
                  lambda: setattr(net, "_c_blocks", True)):
        net.use_c_step, net._tap, net.kernel_timer, net._c_blocks = True, None, None, False
        setup()
        with pytest.raises(NotImplementedError, match="step_cache"):
            net._step_cache_ok()
        with pytest.raises(NotImplementedError, match="step_cache"):
            net.time_distances(torch.zeros(3))
    net.use_c_step, net._tap, net.kernel_timer, net._c_blocks = True, None, None, False
    net._step_cache_ok()
