"""The guidance plan without a GPU (include/scail_dit.h "guidance plan"): the host planner and its merge with the step cache's plan, the
refusals the library makes before anything is enqueued (they need neither a handle nor a device), the CLI flags, and the new names in the
headers, the library and the ctypes table."""
import ctypes as C
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_HIP = ["scail_cfg_delta_store", "scail_cfg_euler_delta"]
NEW_DIT = ["scail_dit_step_branch", "scail_dit_guidance_bytes", "scail_dit_sample_guided"]


# ---- plan_guidance --------------------------------------------------------------------------------------------------------------------------
SIG10 = [1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1]          # the starting sigma of each of 10 steps


def test_plan_worked_example():
    from scail_amd.sampler import plan_guidance
    # steps 2..7 start at sigma 0.8 .. 0.3
    assert plan_guidance(SIG10, interval=(0.25, 0.85), every=3) == [2, 2, 0, 1, 1, 0, 1, 1, 2, 2]


def test_plan_edges():
    from scail_amd.sampler import plan_guidance
    assert plan_guidance(SIG10) == [0] * 10, "no interval, every 1: today's sampler, every step the pair"
    assert plan_guidance(SIG10, every=2) == [0, 1] * 5
    assert plan_guidance(SIG10, every=100) == [0] + [1] * 9
    assert plan_guidance(SIG10, interval=(0.5, 0.5)) == [2] * 5 + [0] + [2] * 4, "both bounds are inside"
    assert plan_guidance(SIG10, interval=(0.3, 0.8)) == [2, 2] + [0] * 6 + [2, 2]
    assert plan_guidance(SIG10, interval=(2.0, 3.0)) == [2] * 10
    assert plan_guidance([], every=3) == []
    # two maximal runs of inside steps (a schedule that is not monotonic): the position restarts in each
    assert plan_guidance([0.5, 0.5, 0.5, 0.9, 0.5, 0.5], interval=(0.4, 0.6), every=2) == [0, 1, 0, 2, 0, 1]


def test_plan_takes_tensors():
    import torch
    from scail_amd.sampler import RFSampler, plan_guidance
    sig = RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=6).sigmas()
    assert sig.numel() == 7
    plan = plan_guidance(sig[:-1], interval=(float(sig[4]), float(sig[1])), every=2)
    assert plan == [2, 0, 1, 0, 1, 2] and all(type(v) is int for v in plan)
    assert plan_guidance(torch.tensor(SIG10), interval=(0.25, 0.85), every=3) == [2, 2, 0, 1, 1, 0, 1, 1, 2, 2]


@pytest.mark.parametrize("kw, needle", [
    (dict(every=0), "every must be an integer >= 1"),
    (dict(every=-2), "every must be an integer >= 1"),
    (dict(every=1.5), "every must be an integer >= 1"),
    (dict(interval=(0.6, 0.4)), "lo <= hi"),
    (dict(interval=(float("nan"), 0.4)), "finite"),
    (dict(interval=(0.1, float("inf"))), "finite"),
    (dict(interval=(0.1, 0.2, 0.3)), r"interval is \(lo, hi\)"),
])
def test_plan_bad_arguments(kw, needle):
    from scail_amd.sampler import plan_guidance
    with pytest.raises(ValueError, match=needle):
        plan_guidance(SIG10, **kw)


def test_plan_modes_stand_alone_and_are_validated():
    from scail_amd.sampler import plan_guidance
    assert plan_guidance(SIG10[:6], modes=[0, 1, 2, 0, 1, 1]) == [0, 1, 2, 0, 1, 1]
    assert plan_guidance(SIG10[:3], modes=(2, 2, 2)) == [2, 2, 2]
    with pytest.raises(ValueError, match="stand alone"):
        plan_guidance(SIG10[:2], interval=(0.0, 1.0), modes=[0, 1])
    with pytest.raises(ValueError, match="stand alone"):
        plan_guidance(SIG10[:2], every=2, modes=[0, 1])
    with pytest.raises(ValueError, match="one entry per step"):
        plan_guidance(SIG10[:3], modes=[0, 1])
    with pytest.raises(ValueError, match=r"entry 1 is 3 "):
        plan_guidance(SIG10[:2], modes=[0, 3])
    with pytest.raises(ValueError, match=r"entry 0 is -1 "):
        plan_guidance(SIG10[:1], modes=[-1])
    with pytest.raises(ValueError, match=r"entry 1 is 1 \(delta\) with no pair step before it"):
        plan_guidance(SIG10[:3], modes=[2, 1, 0])


# ---- merge_guidance_with_step_cache -----------------------------------------------------------------------------------------------------------
def c_rules(guide, reuse):
    """the library's rules restated (scail_dit_sample_guided): the text of the first refusal, or None"""
    seen_pair = False
    for i, g in enumerate(guide):
        if g > 2:
            return f"entry {i} above 2"
        if g == 1 and not seen_pair:
            return f"delta at {i} with no pair before it"
        seen_pair = seen_pair or g == 0
    if reuse is not None:
        if any(r > 1 for r in reuse):
            return "mask entry above 1"
        if reuse and reuse[0] != 0:
            return "first step reuses"
        j = 0
        for i, r in enumerate(reuse):
            if r == 0:
                j = i
            elif (guide[i] == 0) != (guide[j] == 0):
                return f"step {i} reuses step {j} of the other kind"
    return None


def test_merge_examples():
    from scail_amd.sampler import merge_guidance_with_step_cache as merge
    assert merge([0, 0, 1, 1, 2, 2], [0, 0, 0, 0, 0, 0]) == [0, 0, 1, 1, 2, 2], "nothing reuses: the guide as it was"
    assert merge([0, 0, 1, 1, 2, 2], [0, 1, 0, 1, 0, 1]) == [0, 0, 1, 1, 2, 2]
    assert merge([0, 1, 0, 1, 2, 2], [0, 1, 1, 0, 1, 0]) == [0, 0, 0, 1, 1, 2], "a reusing step takes the last computing step's entry"
    assert merge([2, 0, 1, 1], [0, 1, 0, 0]) == [2, 2, 0, 1], "the pair step was reused away: the first computing delta step becomes the pair"
    assert merge([2, 2, 0], [0, 1, 1]) == [2, 2, 2]
    assert merge([], []) == []


def test_merge_refuses_bad_inputs():
    from scail_amd.sampler import merge_guidance_with_step_cache as merge
    with pytest.raises(ValueError, match="one entry per step"):
        merge([0, 1], [0])
    with pytest.raises(ValueError, match="starts with 0"):
        merge([0, 1], [1, 0])
    with pytest.raises(ValueError, match="0 / 1 entries"):
        merge([0, 1], [0, 2])
    with pytest.raises(ValueError, match="no pair step before it"):
        merge([1, 0], [0, 0])
    with pytest.raises(ValueError, match="entry 0 is 5"):
        merge([5], [0])


def test_merge_always_satisfies_the_c_rules_exhaustively():
    """every guide that passes the rules on its own, with every mask that passes them on its own, up to length 5"""
    from scail_amd.sampler import check_guidance_plan, merge_guidance_with_step_cache as merge
    pairs = changed = 0
    for n in range(0, 6):
        for guide in itertools.product((0, 1, 2), repeat=n):
            if c_rules(guide, None) is not None:
                with pytest.raises(ValueError):
                    merge(list(guide), [0] * n)
                continue
            for reuse in itertools.product((0, 1), repeat=n):
                if n and reuse[0] != 0:
                    continue
                out = merge(list(guide), list(reuse))
                pairs += 1
                changed += out != list(guide)
                assert len(out) == n and c_rules(out, reuse) is None, (guide, reuse, out, c_rules(out, reuse))
                assert check_guidance_plan(out, reuse) == out
                for i in range(n):
                    if not reuse[i]:
                        assert out[i] == guide[i] or (guide[i], out[i]) == (1, 0), "a computing step keeps its entry (or is promoted to the pair)"
                j = 0
                for i in range(n):
                    j = j if reuse[i] else i
                    assert out[i] == out[j], "a reusing step takes the entry of the last computing step"
                if c_rules(guide, reuse) is not None:
                    with pytest.raises(ValueError):
                        check_guidance_plan(guide, reuse)
    assert pairs > 2000 and changed > 500, (pairs, changed)


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
    assert (L.GUIDE_PAIR, L.GUIDE_DELTA, L.GUIDE_COND) == (0, 1, 2)
    hdr = open(os.path.join(ROOT, "include", "scail_dit.h")).read()
    for line in ("#define SCAIL_DIT_GUIDE_PAIR 0", "#define SCAIL_DIT_GUIDE_DELTA 1", "#define SCAIL_DIT_GUIDE_COND 2"):
        assert line in hdr, line


def test_guidance_bytes(lib):
    assert lib.scail_dit_guidance_bytes(3, 8, 20) == 3 * 16 * 8 * 20 * 4
    assert lib.scail_dit_guidance_bytes(1, 4, 4) == 1024
    assert lib.scail_dit_guidance_bytes(1, 4, 12) == 3072 and lib.scail_dit_guidance_bytes(3, 4, 4) == 3072
    assert lib.scail_dit_guidance_bytes(21, 64, 112) == 21 * 16 * 64 * 112 * 4
    for bad in ((0, 8, 20), (3, 0, 20), (3, 8, 0), (3, 6, 20), (3, 8, 18), (-1, 8, 20), (1 << 15, 8, 20)):
        assert lib.scail_dit_guidance_bytes(*bad) == -1, bad


A = 0x10000        # a fake, 256-byte aligned device address: every refusal below comes before it could be dereferenced


def test_row_kernels_refuse_on_the_host(lib):
    from scail_amd import lib as L
    cases = [
        (r"scail_cfg_delta_store: n must be .* got -1", "scail_cfg_delta_store", (A, A, -1, None)),
        (r"scail_cfg_delta_store: n must be .* got 549755813888", "scail_cfg_delta_store", (A, A, 1 << 39, None)),
        (r"scail_cfg_delta_store: null pointer: v \(n = 7\)", "scail_cfg_delta_store", (None, A, 7, None)),
        (r"scail_cfg_delta_store: null pointer: delta \(n = 7\)", "scail_cfg_delta_store", (A, None, 7, None)),
        (r"scail_cfg_euler_delta: n must be .* got -3", "scail_cfg_euler_delta", (A, A, A, -3, 4.0, 0.1, None)),
        (r"scail_cfg_euler_delta: null pointer: x \(n = 5\)", "scail_cfg_euler_delta", (None, A, A, 5, 4.0, 0.1, None)),
        (r"scail_cfg_euler_delta: null pointer: v_c \(n = 5\)", "scail_cfg_euler_delta", (A, None, None, 5, 4.0, 0.1, None)),
    ]
    for needle, name, args in cases:
        with pytest.raises(L.ScailHipError, match=needle):
            L.call(name, *args)
    # n == 0 launches nothing and needs no device
    L.call("scail_cfg_delta_store", A, A, 0, None)
    L.call("scail_cfg_euler_delta", A, A, None, 0, 4.0, 0.1, None)


def _branch(cond_batch=2, elem=1, mode=0, cache=None, cache_bytes=0):
    return ("scail_dit_step_branch", None, A, A, A, cond_batch, elem, A, A, 1, 3, A, A, A, 3, 8, 20, A, 1 << 20, mode, cache, cache_bytes, None)


def test_step_branch_refusals(lib):
    from scail_amd import lib as L
    for cb in (0, 9, -1):
        with pytest.raises(L.ScailHipError, match=rf"scail_dit_step_branch: cond_batch must be 1..8, got {cb}"):
            L.call(*_branch(cond_batch=cb))
    for cb, elem in ((2, 2), (2, -1), (1, 1), (8, 8)):
        with pytest.raises(L.ScailHipError, match=rf"elem must lie in \[0, cond_batch = {cb}\), got {elem}"):
            L.call(*_branch(cond_batch=cb, elem=elem))
    for mode in (3, -1, 7):
        with pytest.raises(L.ScailHipError, match=rf"scail_dit_step_branch: unknown mode {mode} "):
            L.call(*_branch(mode=mode))
    for mode in (1, 2):
        with pytest.raises(L.ScailHipError, match=r"scail_dit_step_branch: null cache \(cache_bytes 4096"):
            L.call(*_branch(mode=mode, cache=None, cache_bytes=4096))
        with pytest.raises(L.ScailHipError, match=r"256-byte aligned.*is 128 past"):
            L.call(*_branch(mode=mode, cache=A + 128, cache_bytes=1 << 20))
        with pytest.raises(L.ScailHipError, match=r"a cache mode takes elem 0 or 1 .* got 2"):
            L.call(*_branch(cond_batch=3, elem=2, mode=mode, cache=A, cache_bytes=1 << 20))
        with pytest.raises(L.ScailHipError, match="null handle"):
            L.call(*_branch(mode=mode, cache=A, cache_bytes=1 << 20))
    with pytest.raises(L.ScailHipError, match="null handle"):
        L.call(*_branch())


def _guided(guide, n_steps=None, delta=A, delta_bytes=1 << 20, reuse=None, cache=A, cache_bytes=1 << 20):
    n_steps = len(guide) if n_steps is None else n_steps
    g = None if guide is None else (C.c_uint8 * max(len(guide), 1))(*guide)
    r = None if reuse is None else (C.c_uint8 * max(len(reuse), 1))(*reuse)
    return ("scail_dit_sample_guided", None, A, A, A, n_steps, 4.0, A, A, A, 1, 3, A, A, 3, 8, 20, A, 1 << 20, g, delta, delta_bytes, r, cache,
            cache_bytes, None)


def test_sample_guided_refuses_bad_plans(lib):
    from scail_amd import lib as L
    who = "scail_dit_sample_guided"
    with pytest.raises(L.ScailHipError, match=rf"{who}: guide\[2\] = 3 \(an entry is 0 = pair, 1 = delta or 2 = cond\)"):
        L.call(*_guided([0, 1, 3, 0]))
    with pytest.raises(L.ScailHipError, match=r"guide\[0\] = 255"):
        L.call(*_guided([255]))
    with pytest.raises(L.ScailHipError, match=r"guide\[1\] = 1 \(delta\) has no pair step before it"):
        L.call(*_guided([2, 1, 0]))
    with pytest.raises(L.ScailHipError, match=r"guide\[0\] = 1 \(delta\) has no pair step before it"):
        L.call(*_guided([1]))
    with pytest.raises(L.ScailHipError, match=r"null guide plan with n_steps = 4"):
        L.call(*_guided(None, n_steps=4))
    with pytest.raises(L.ScailHipError, match=r"n_steps must be >= 0, got -2"):
        L.call(*_guided([0], n_steps=-2))


def test_sample_guided_refuses_a_bad_delta_buffer(lib):
    from scail_amd import lib as L
    need = 3 * 16 * 8 * 20 * 4
    for plan in ([0, 0], [0, 1], [2, 0]):
        with pytest.raises(L.ScailHipError, match=r"scail_dit_sample_guided: null delta buffer \(delta_bytes 4096"):
            L.call(*_guided(plan, delta=None, delta_bytes=4096))
        with pytest.raises(L.ScailHipError, match=r"the delta buffer must be 256-byte aligned.*is 64 past"):
            L.call(*_guided(plan, delta=A + 64))
        with pytest.raises(L.ScailHipError, match=rf"delta buffer too small: {need - 1} bytes, needs {need} \(scail_dit_guidance_bytes\)"):
            L.call(*_guided(plan, delta_bytes=need - 1))
        with pytest.raises(L.ScailHipError, match="null argument"):           # a well-formed plan and buffer get as far as the handle
            L.call(*_guided(plan, delta_bytes=need))
    # a plan of COND entries alone takes no delta buffer: it gets as far as the handle without one
    with pytest.raises(L.ScailHipError, match="null argument"):
        L.call(*_guided([2, 2, 2], delta=None, delta_bytes=0))


def test_sample_guided_with_a_mask_refuses_what_sample_cached_refuses(lib):
    from scail_amd import lib as L
    with pytest.raises(L.ScailHipError, match=r"scail_dit_sample_guided: reuse\[0\] = 1: the first step has nothing to reuse"):
        L.call(*_guided([0, 0, 0], reuse=[1, 0, 0]))
    with pytest.raises(L.ScailHipError, match=r"reuse\[2\] = 2 \(an entry is 0 = compute or 1 = reuse\)"):
        L.call(*_guided([0, 0, 0, 0], reuse=[0, 1, 2, 0]))
    with pytest.raises(L.ScailHipError, match=r"scail_dit_sample_guided: null cache"):
        L.call(*_guided([0, 0], reuse=[0, 1], cache=None))
    with pytest.raises(L.ScailHipError, match=r"256-byte aligned.*is 64 past"):
        L.call(*_guided([0, 0], reuse=[0, 1], cache=A + 64))
    with pytest.raises(L.ScailHipError, match="null handle"):
        L.call(*_guided([0, 0], reuse=[0, 1]))


@pytest.mark.parametrize("guide, reuse, i, j", [
    ([0, 1], [0, 1], 1, 0),
    ([0, 2], [0, 1], 1, 0),
    ([2, 0], [0, 1], 1, 0),
    ([0, 1, 0], [0, 0, 1], 2, 1),
    ([0, 0, 2, 2, 0], [0, 1, 0, 1, 1], 4, 2),
])
def test_sample_guided_refuses_a_reuse_of_the_other_kind(lib, guide, reuse, i, j):
    from scail_amd import lib as L
    assert c_rules(guide, reuse) == f"step {i} reuses step {j} of the other kind"
    with pytest.raises(L.ScailHipError, match=rf"step {i} reuses \(guide {guide[i]}\) what step {j}, the last computing step, left \(guide {guide[j]}\)"):
        L.call(*_guided(guide, reuse=reuse))
    # the kinds that go together get as far as the handle
    with pytest.raises(L.ScailHipError, match="null handle"):
        L.call(*_guided([0, 0, 1, 2, 2, 1], reuse=[0, 1, 0, 1, 0, 1]))


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------------
def test_cli_parses_the_flags():
    from scail_amd import cli
    a = cli.build_parser().parse_args([])
    assert a.cfg_interval is None and a.cfg_delta_every is None and a.cfg_plan is None
    assert cli.guidance_args() is None
    a = cli.build_parser().parse_args(["--cfg-interval", "0.2", "0.9", "--cfg-delta-every", "3"])
    assert cli.guidance_args(a.cfg_interval, a.cfg_delta_every, a.cfg_plan, a.tile_frames) == {"interval": (0.2, 0.9), "every": 3}
    assert cli.guidance_args(every=2) == {"every": 2}
    a = cli.build_parser().parse_args(["--cfg-plan", "0,2,1,1"])
    assert cli.guidance_args(a.cfg_interval, a.cfg_delta_every, a.cfg_plan) == {"modes": [0, 2, 1, 1]}
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--cfg-interval", "0.2"])
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--cfg-delta-every", "two"])


@pytest.mark.parametrize("kw, needle", [
    (dict(interval=(0.9, 0.2)), "finite LO <= HI"),
    (dict(interval=(float("nan"), 0.2)), "finite LO <= HI"),
    (dict(every=0), "integer >= 1"),
    (dict(plan="0,1", every=2), "--cfg-plan stands alone"),
    (dict(plan="0,1", interval=(0.0, 1.0)), "--cfg-plan stands alone"),
    (dict(plan="0,x"), "separated by commas"),
    (dict(plan="0,3"), "--cfg-plan: entry 1 is 3"),
    (dict(plan="1,0"), "--cfg-plan: entry 0 is 1 .* no pair step before it"),
    (dict(every=2, tile_frames=81), "do not go with --tile-frames"),
    (dict(plan="0,0", tile_frames=41), "do not go with --tile-frames"),
])
def test_cli_argument_refusals(kw, needle):
    from scail_amd import cli
    with pytest.raises(ValueError, match=needle):
        cli.guidance_args(**kw)


def test_cli_prints_the_plan():
    from scail_amd import cli
    text = cli.format_guidance_plan([2, 2, 0, 1, 1, 0, 1, 1, 2, 2])
    assert text.startswith("guidance plan: 2 of 10 steps run the uncond / cond pair (2, 5); 4 run the cond branch with the last stored delta, 4 the cond")


def test_cli_argument_errors_come_before_any_model(capsys):
    from scail_amd import cli
    with pytest.raises(SystemExit):
        cli.main(["--tiny", "--cfg-delta-every", "2", "--tile-frames", "41"])
    assert "do not go with --tile-frames" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["--tiny", "--cfg-plan", "1,0"])
    assert "no pair step before it" in capsys.readouterr().err


# ---- the sampler's routing, on a stand-in network -----------------------------------------------------------------------------------------
class _Net:
    """records what RFSampler.sample_hip hands the network's one-call loop"""

    def __init__(self, ok=True):
        self.ok, self.calls = ok, []

    def executor_ok(self, whole_loop=False):
        return self.ok

    def sample_c(self, x, sig, cfg, ctx, ref, pose, clip, cond_key=None, **kw):
        self.calls.append(kw)
        return x


def _request():
    import torch
    shared = dict(concat_images=torch.zeros(1), ref_concat=torch.zeros(1, 1, 16, 8, 20), concat_smpl_render=torch.zeros(1, 3, 16, 4, 10),
                  image_clip_features=torch.zeros(1, 5, 1280))
    return torch.zeros(1, 3, 16, 8, 20), dict(crossattn=torch.zeros(1, 12, 64), **shared), dict(crossattn=torch.ones(1, 12, 64), **shared)


def test_sample_hip_without_the_option_takes_todays_route():
    from scail_amd.sampler import RFSampler
    x, c, uc = _request()
    net, s = _Net(), RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=6)
    s.sample_hip(net, x, c, uc, scale=4.0)
    assert net.calls == [{}] and not hasattr(s, "last_guidance_plan")


def test_sample_hip_plans_and_takes_the_guided_route():
    from scail_amd.sampler import RFSampler
    x, c, uc = _request()
    net, s = _Net(), RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=6)
    sig = s.sigmas()
    s.sample_hip(net, x, c, uc, scale=4.0, guidance=dict(interval=(float(sig[4]), float(sig[1])), every=2))
    assert s.last_guidance_plan == [2, 0, 1, 0, 1, 2] and net.calls[-1] == dict(reuse=None, guide=[2, 0, 1, 0, 1, 2])
    s.sample_hip(net, x, c, uc, scale=4.0, guidance=dict(modes=[0, 1, 2, 0, 1, 1]))
    assert net.calls[-1] == dict(reuse=None, guide=[0, 1, 2, 0, 1, 1])
    # with the step cache: the merge
    s.sample_hip(net, x, c, uc, scale=4.0, guidance=dict(every=2), step_cache=dict(mask=[0, 1, 1, 0, 1, 0]))
    assert s.last_step_cache_plan == [0, 1, 1, 0, 1, 0] and s.last_guidance_plan == [0, 0, 0, 1, 1, 1]
    assert net.calls[-1] == dict(reuse=[0, 1, 1, 0, 1, 0], guide=[0, 0, 0, 1, 1, 1])
    # explicit modes are not rewritten: they must agree with the mask as they stand
    with pytest.raises(ValueError, match="step 1 reuses"):
        s.sample_hip(net, x, c, uc, scale=4.0, guidance=dict(modes=[0, 1, 0, 1, 0, 1]), step_cache=dict(mask=[0, 1, 0, 1, 0, 1]))
    for bad in ({}, dict(scale=2.0), [0, 1], dict(every=0), dict(modes=[0, 1])):
        with pytest.raises(ValueError):
            s.sample_hip(net, x, c, uc, scale=4.0, guidance=bad)


def test_sample_hip_refuses_what_the_plan_does_not_cover():
    from scail_amd.sampler import RFSampler, RFSamplerLong
    x, c, uc = _request()
    s = RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=6)
    net = _Net()
    with pytest.raises(NotImplementedError, match=r"guidance .* sequence-parallel ranks \(chunk_dim\)"):
        s.sample_hip(net, x, c, uc, scale=4.0, chunk_dim=3, guidance=dict(every=2))
    with pytest.raises(NotImplementedError, match="guidance .* SCAIL_C_STEP=0, _tap or kernel_timer"):
        s.sample_hip(_Net(ok=False), x, c, uc, scale=4.0, guidance=dict(every=2))
    long = RFSamplerLong(hunyuan_schedule=True, shift_scale=5, num_steps=2)
    with pytest.raises(NotImplementedError, match="guidance with temporal tiles"):
        long.sample_hip(net, x, dict(c, smpl_tiled=c["concat_smpl_render"][:, None]), uc, tile_indices=[[0, 1], [1, 2]], guidance=dict(every=2))
    assert net.calls == []
