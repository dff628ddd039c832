"""The solver plan on the GPU (include/scail_dit.h "solver plan"): the two fp32 kernels against the torch expression on the CPU, one tensor
operation per arithmetic operation, and the solver loops against compositions the test makes itself.

No tolerance anywhere: every check is on bits (a NaN is compared as NaN-ness).  Values, networks and shapes are the guidance and step-cache
tests' own: the 36 chosen bit patterns, toy networks of 3 layers, latents of Ltok 190 and 882, SIG6; the tiled case is the long-clip
tests' golden request (6 latent frames, three 4-frame tiles) over 4 steps, the fewest that hold a second-order step."""
import ctypes as C

import numpy as np
import pytest
import torch

import ws_contract as W
from test_guidance_gpu import CFG, CHOSEN, _chosen, _f, _request, _rope, _same_f32, _sampler_request
from test_step_cache_gpu import LARGE, SIG6, SMALL, _net

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = torch.float32


# ---- the CPU expression ---------------------------------------------------------------------------------------------------------------------
def cpu_update(x, d, hist, sigma, a, b, c, use_prev):
    """D = x - sigma d; y = a x + b D (+ c hist); -> (y, D): each operation a separate fp32 op"""
    D = x - _f(sigma) * d
    y = _f(a) * x + _f(b) * D
    if use_prev:
        y = y + _f(c) * hist
    return y, D


def cpu_multistep(x, vu, vc, hist, cfg, sigma, a, b, c, use_prev):
    return cpu_update(x, vu + _f(cfg) * (vc - vu), hist, sigma, a, b, c, use_prev)


def cpu_tile_finish(x, den, inv, hist, sigma, a, b, c, use_prev):
    """x, den, hist (1, T, F); inv (T)"""
    return cpu_update(x, den * inv[None, :, None], hist, sigma, a, b, c, use_prev)


# (cfg_scale, sigma, a, b, c, use_prev): a second-order row, a first-order row over a history that is never read, a last step with history
SETS = [(4.0, 0.75, 0.8, 0.35, -0.15, 1), (1.0, 0.9, 0.6, 0.4, 0.0, 0), (7.5, 1.0, 0.0, 1.0, 0.25, 1)]
K = len(CHOSEN)
INV = [0.5, 1.0, 1.0 / 3.0, 0.7, 2.0, 0.2857142857142857]


@pytest.fixture(scope="module")
def crossed():
    """(x, v_c or den, hist) crossed 36^3, v_u a rotation of the list along x; the CPU results of both kernels for every set, once"""
    c = _chosen()
    x, v3, h3 = c.repeat(K * K), c.repeat_interleave(K).repeat(K), c.repeat_interleave(K * K)
    vu = c.roll(7).repeat(K * K)
    inv = torch.tensor([INV[f % len(INV)] for f in range(K)], dtype=f32)
    out = dict(x=x, v3=v3, h3=h3, vu=vu, inv=inv)
    for s in SETS:
        out[("cfg",) + s] = cpu_multistep(x, vu, v3, h3, *s)
        out[("tile",) + s] = cpu_tile_finish(x.view(1, K, K * K), v3.view(1, K, K * K), inv, h3.view(1, K, K * K), *s[1:])
    return out


@pytest.mark.parametrize("s", SETS, ids=["second", "first_nan_hist", "last"])
def test_cfg_multistep_every_chosen_triple(crossed, s):
    from scail_amd import ops
    e = crossed
    want_x, want_D = e[("cfg",) + s]
    assert torch.isnan(want_x).any() and torch.isinf(want_x).any() and torch.isfinite(want_x).any()
    v = torch.stack([e["vu"], e["v3"]]).to(DEV)
    snap = W.snapshot(dict(v=v))
    x, xcheck = W.guarded_like(torch.empty(e["x"].numel(), dtype=f32, device=DEV), W.FILLS["big"])
    hist, hcheck = W.guarded_like(torch.empty(e["x"].numel(), dtype=f32, device=DEV), W.FILLS["nan"])
    x.copy_(e["x"])
    if s[-1]:
        hist.copy_(e["h3"])                                  # (use_prev == 0: hist stays NaN-filled; the kernel must not read it)
    ops.cfg_multistep_(x, v, hist, s[0], s[1], s[2], s[3], s[4], use_prev=bool(s[-1]))
    xcheck("cfg_multistep x"); hcheck("cfg_multistep hist")
    _same_f32(x, want_x, f"cfg_multistep x {s}")
    _same_f32(hist, want_D, f"cfg_multistep: hist after the call is D {s}")
    W.assert_unchanged(snap)


@pytest.mark.parametrize("s", SETS, ids=["second", "first_nan_hist", "last"])
def test_tile_finish_multistep_every_chosen_triple(crossed, s):
    from scail_amd import ops
    e = crossed
    want_x, want_D = e[("tile",) + s]
    assert torch.isnan(want_x).any() and torch.isfinite(want_x).any()
    shape = (1, K, K * K)                                    # 36 frames of 1296 floats
    x, xcheck = W.guarded_like(torch.empty(shape, dtype=f32, device=DEV), W.FILLS["big"])
    den, dcheck = W.guarded_like(torch.empty(shape, dtype=f32, device=DEV), W.FILLS["big"])
    hist, hcheck = W.guarded_like(torch.empty(shape, dtype=f32, device=DEV), W.FILLS["nan"])
    x.copy_(e["x"].view(shape)); den.copy_(e["v3"].view(shape))
    if s[-1]:
        hist.copy_(e["h3"].view(shape))
    ops.tile_finish_multistep_(x, den, e["inv"], hist, s[1], s[2], s[3], s[4], use_prev=bool(s[-1]))
    xcheck("tile_finish_multistep x"); dcheck("tile_finish_multistep den"); hcheck("tile_finish_multistep hist")
    _same_f32(x, want_x, f"tile_finish_multistep x {s}")
    _same_f32(hist, want_D, f"tile_finish_multistep: hist after the call is D {s}")
    assert int(den.count_nonzero()) == 0 and not bool(torch.isnan(den).any()), "den is left zeroed"


def _strewn(n, seed, scales):
    """random data with the chosen values strewn in"""
    g = torch.Generator().manual_seed(seed)
    c = _chosen()
    out = [torch.randn(n, generator=g) * s for s in scales]
    for k, t in enumerate(out):
        idx = torch.randperm(n, generator=g)[:min(n, 72)]
        t[idx] = c[(torch.arange(idx.numel()) * (k + 5)) % c.numel()]
    return out


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1025, 7680])
def test_cfg_multistep_sizes(n):
    """nothing, one element (the tail alone), sizes around one workgroup of 256 threads and of 1024 elements, sizes that are no multiple of
    4 (v_c is then not 16-byte aligned) and 30 workgroups; outputs between 0xA5 bands, v unchanged"""
    from scail_amd import ops
    x, vu, vc, h = _strewn(n, n + 1, (3.0, 0.5, 1.0, 40.0))
    gv = torch.stack([vu, vc]).to(DEV)
    snap = W.snapshot(dict(v=gv)) if n else None
    for s in SETS:
        gx, xcheck = W.guarded_like(torch.empty(n, dtype=f32, device=DEV), W.FILLS["nan"])
        gh, hcheck = W.guarded_like(torch.empty(n, dtype=f32, device=DEV), W.FILLS["nan"])
        gx.copy_(x)
        if s[-1]:
            gh.copy_(h)
        ops.cfg_multistep_(gx, gv, gh, s[0], s[1], s[2], s[3], s[4], use_prev=bool(s[-1]))
        xcheck("cfg_multistep x"); hcheck("cfg_multistep hist")
        want_x, want_D = cpu_multistep(x, vu, vc, h, *s)
        _same_f32(gx, want_x, f"cfg_multistep n {n} {s}")
        _same_f32(gh, want_D, f"cfg_multistep hist n {n} {s}")
    if n:
        W.assert_unchanged(snap)


@pytest.mark.parametrize("which", ["x", "v", "hist"])
def test_cfg_multistep_takes_pointers_that_are_not_16_byte_aligned(which):
    """a view one float into its buffer: the scalar form of the kernel, the same bits"""
    from scail_amd import ops
    n, s = 1025, SETS[0]
    x, vu, vc, h = _strewn(n, 3, (3.0, 0.5, 1.0, 40.0))
    off = {k: int(k == which) for k in ("x", "v", "hist")}
    bx = torch.zeros(n + 1, device=DEV); bh = torch.zeros(n + 1, device=DEV); bv = torch.zeros(2 * n + 1, device=DEV)
    gx, gh, gv = bx[off["x"]:off["x"] + n], bh[off["hist"]:off["hist"] + n], bv[off["v"]:off["v"] + 2 * n].view(2, n)
    assert {"x": gx, "v": gv, "hist": gh}[which].data_ptr() % 16 == 4
    gx.copy_(x); gh.copy_(h); gv.copy_(torch.stack([vu, vc]))
    ops.cfg_multistep_(gx, gv, gh, s[0], s[1], s[2], s[3], s[4], use_prev=True)
    want_x, want_D = cpu_multistep(x, vu, vc, h, *s)
    _same_f32(gx, want_x, "x"); _same_f32(gh, want_D, "hist")
    for buf, o in ((bx, off["x"]), (bh, off["hist"]), (bv, off["v"])):
        assert float(buf[0 if o else -1]) == 0.0, "the float beside the view was written"


@pytest.mark.parametrize("T, shape", [(9, (16, 5, 7)), (9, (3, 5)), (70, (3, 5)), (70, (4, 4)), (1, (1,))],
                         ids=["F560", "F15_scalar", "T70_scalar", "T70_vec", "one"])
def test_tile_finish_multistep_sizes(T, shape):
    """F a multiple of 4 (16-byte accesses) and not (the scalar form), neither F nor T F a multiple of the block, more than 64 frames (two
    launches of 64 frames' factors)"""
    from scail_amd import ops
    F = int(np.prod(shape))
    x, den, h = (t.view(1, T, *shape) for t in _strewn(T * F, T + F, (3.0, 1.0, 40.0)))
    inv = torch.rand(T, generator=torch.Generator().manual_seed(T)) + 0.3
    for s in SETS:
        gx, xcheck = W.guarded_like(torch.empty(1, T, *shape, dtype=f32, device=DEV), W.FILLS["nan"])
        gd, dcheck = W.guarded_like(torch.empty(1, T, *shape, dtype=f32, device=DEV), W.FILLS["nan"])
        gh, hcheck = W.guarded_like(torch.empty(1, T, *shape, dtype=f32, device=DEV), W.FILLS["nan"])
        gx.copy_(x); gd.copy_(den)
        if s[-1]:
            gh.copy_(h)
        ops.tile_finish_multistep_(gx, gd, inv, gh, s[1], s[2], s[3], s[4], use_prev=bool(s[-1]))
        xcheck("x"); dcheck("den"); hcheck("hist")
        want_x, want_D = cpu_tile_finish(x.view(1, T, F), den.view(1, T, F), inv, h.view(1, T, F), *s[1:])
        _same_f32(gx, want_x, f"tile_finish_multistep x T {T} F {F} {s}")
        _same_f32(gh, want_D, f"tile_finish_multistep hist T {T} F {F} {s}")
        assert int(gd.count_nonzero()) == 0 and not bool(torch.isnan(gd).any())


# ---- no contraction: one case per multiply-add of the sequence -----------------------------------------------------------------------------
ULP = 2.0 ** -23
ONE_ULP = 1.0 + ULP                # 3 * (1 + 2^-23) = 3 + 1.5 ulp(3) rounds to 3 + 4 * 2^-23; fused with -3 it is 3 * 2^-23
# name -> (x, v_u, v_c, hist, cfg, sigma, a, b, c): the multiply-add named is the only place where fusing changes the result
CONTRACTIONS = {
    "v_u + cfg * (v_c - v_u)": (0.0, -3.0, -2.0 + ULP, 0.0, 3.0, 1.0, 0.0, 1.0, 0.0),          # d; then D = 0 - d, y = 0 + D
    "x - sigma * d": (3.0, ONE_ULP, ONE_ULP, 0.0, 1.0, 3.0, 0.0, 1.0, 0.0),                     # D; then y = 0 + D
    "a * x + (b * D)": (ONE_ULP, -2.0 + ULP, -2.0 + ULP, 0.0, 1.0, 1.0, 3.0, -1.0, 0.0),        # D = 3 exactly, b D = -3, a x = 3 (1 + ulp)
    "(a * x) + b * D": (-0.75, -1.75 - ULP, -1.75 - ULP, 0.0, 1.0, 1.0, 4.0, 3.0, 0.0),         # D = 1 + ulp exactly, a x = -3
    "y + c * hist": (-3.0, 0.0, 0.0, ONE_ULP, 1.0, 0.5, 1.0, 0.0, 3.0),                         # y = -3 + 0, c hist = 3 (1 + ulp)
}


def _fma(a, b, c):
    """round32(a * b + c): the product of two fp32 values is exact in fp64"""
    return (a.double() * b.double() + c.double()).float()


def _contracted(name, x, vu, vc, hist, cfg, sigma, a, b, c):
    """the sequence with the named multiply-add fused, every other operation as the kernel does it"""
    x, vu, vc, hist, cfg, sigma, a, b, c = (_f(v) for v in (x, vu, vc, hist, cfg, sigma, a, b, c))
    d = _fma(cfg, vc - vu, vu) if name.startswith("v_u") else vu + cfg * (vc - vu)
    D = _fma(-sigma, d, x) if name.startswith("x -") else x - sigma * d
    if name == "a * x + (b * D)":
        y = _fma(a, x, b * D)
    elif name == "(a * x) + b * D":
        y = _fma(b, D, a * x)
    else:
        y = a * x + b * D
    return _fma(c, hist, y) if name.startswith("y +") else y + c * hist


@pytest.mark.parametrize("name", list(CONTRACTIONS))
def test_kernels_do_not_contract(name):
    from scail_amd import ops
    case = CONTRACTIONS[name]
    x, vu, vc, hist, cfg, sigma, a, b, c = case
    one = lambda v: torch.tensor([float(np.float32(v))], dtype=f32)
    want, want_D = cpu_multistep(one(x), one(vu), one(vc), one(hist), cfg, sigma, a, b, c, True)
    fused = _contracted(name, *case)
    assert abs(float(want)) == 4 * ULP and abs(float(fused)) == 3 * ULP, f"the test cannot see a contraction of {name}: {float(want)} {float(fused)}"
    for n in (1, 5):                                     # the scalar tail alone; a 16-byte body and a tail
        gx, gh = one(x).repeat(n).to(DEV), one(hist).repeat(n).to(DEV)
        gv = torch.stack([one(vu).repeat(n), one(vc).repeat(n)]).to(DEV)
        ops.cfg_multistep_(gx, gv, gh, cfg, sigma, a, b, c, use_prev=True)
        _same_f32(gx, want.repeat(n), f"cfg_multistep: {name} (n {n})")
        _same_f32(gh, want_D.repeat(n), f"cfg_multistep hist: {name} (n {n})")
    if name.startswith("v_u"):
        return                                           # the finishing pass has no CFG combination: its d is den * inv
    assert vu == vc and cfg == 1.0                       # d = v_u: the same case with den = d, inv = 1
    for F in (1, 4):                                     # the scalar form; 16-byte accesses
        gx, gd, gh = (one(v).repeat(F).view(1, 1, F).to(DEV) for v in (x, vu, hist))
        ops.tile_finish_multistep_(gx, gd, [1.0], gh, sigma, a, b, c, use_prev=True)
        _same_f32(gx, want.repeat(F), f"tile_finish_multistep: {name} (F {F})")
        _same_f32(gh, want_D.repeat(F), f"tile_finish_multistep hist: {name} (F {F})")


# ---- the loop against a composition the test makes itself ----------------------------------------------------------------------------------
def _plan(sig, solver):
    from scail_amd.sampler import plan_solver
    return plan_solver(sig, solver)


def _compose(net, x0, sig, cfg, inputs, plan):
    """the solver loop as the header states it: the executor's own step for the evaluation, the CPU expression for the update.
    -> (x, the last step's D)"""
    from scail_amd.sampler import solver_uses_prev
    _, _, ctx, ref, pose, clip = inputs
    kw = dict(concat_images=torch.zeros(1, device=DEV), image_clip_features=clip, ref_concat=ref, concat_smpl_render=pose)
    x, hist = x0.float().contiguous().clone(), None
    for i, (a, b, c) in enumerate(plan):
        t = (sig[i] * 1000.0).repeat(2).to(DEV)
        v = net.forward_f32(torch.cat([x, x], 0), t, ctx, None, cfg_pair=True, **kw).cpu()
        y, hist = cpu_multistep(x.cpu(), v[0:1], v[1:2], hist, cfg, float(sig[i]), a, b, c, solver_uses_prev((a, b, c)))
        x = y.to(DEV)
    return x, hist


def _sample(net, x0, inputs, sig=SIG6, **kw):
    _, _, ctx, ref, pose, clip = inputs
    return net.sample_c(x0, sig, CFG, ctx, ref, pose, clip, **kw).clone()


@pytest.mark.parametrize("shape", [SMALL, LARGE], ids=["small", "large"])
@pytest.mark.parametrize("n_char", [1, 2])
def test_loop_is_the_composition(shape, n_char):
    net = _net("toy" if n_char == 1 else "tiny2")
    x0, inputs = _request(n_char, shape)
    got = {}
    for solver in ("dpmpp2m", "dpm1"):
        plan = _plan(SIG6, solver)
        want, want_D = _compose(net, x0, SIG6, CFG, inputs, plan)
        net._executor()._hist = None
        got[solver] = _sample(net, x0, inputs, solver=(SIG6[:-1], plan))
        assert bool(torch.isfinite(got[solver]).all())
        assert torch.equal(got[solver], want), f"{solver}: differs from the composition in {int((got[solver] != want).sum())} values"
        _same_f32(net._executor().solver_history(*shape), want_D, f"{solver}: hist after the call is the last step's D")
    assert [i for i, r in enumerate(_plan(SIG6, "dpmpp2m")) if r[2] != 0.0] == [2, 3, 4]
    assert not torch.equal(got["dpmpp2m"], got["dpm1"]), "the second-order rows changed nothing"
    net._executor()._hist = None


def test_solver_none_gives_todays_bits():
    from scail_amd.sampler import RFSampler
    net = _net()
    x0, inputs = _request()
    c, uc = _sampler_request(inputs)
    s = RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=6)
    net._executor()._hist = None
    plain = s.sample_hip(net, x0, c, uc, scale=CFG).clone()
    assert torch.equal(s.sample_hip(net, x0, c, uc, scale=CFG, solver=None), plain)
    assert torch.equal(_sample(net, x0, inputs, sig=s.sigmas(), solver=None), plain) and not hasattr(s, "last_solver_plan")
    assert net._executor()._hist is None, "no history buffer without a solver"


@pytest.mark.parametrize("solver", ["dpmpp2m", "dpm1"])
def test_sample_hip_routes_agree(solver):
    """RFSampler.sample_hip: the one-call route and the host loop (a step callback forces it) take the same table and give the same bits"""
    from scail_amd.sampler import RFSampler, plan_solver
    net = _net()
    x0, inputs = _request()
    c, uc = _sampler_request(inputs)
    s = RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=6)
    one = s.sample_hip(net, x0, c, uc, scale=CFG, solver=solver).clone()
    plan = list(s.last_solver_plan)
    assert plan == plan_solver(s.sigmas(), solver)
    want, _ = _compose(net, x0, s.sigmas(), CFG, inputs, plan)
    assert torch.equal(one, want)
    seen = []
    loop = s.sample_hip(net, x0, c, uc, scale=CFG, step_callback=lambda i, xx: seen.append(i), solver=solver)
    assert seen == list(range(6)) and s.last_solver_plan == plan
    assert torch.equal(one, loop), f"the two routes differ in {int((one != loop).sum())} values"
    assert not torch.equal(one, s.sample_hip(net, x0, c, uc, scale=CFG))
    net._executor()._hist = None


# ---- tiled ------------------------------------------------------------------------------------------------------------------------------------
def test_tiled_one_call_equals_the_host_loop(golden_dir, monkeypatch):
    from test_longclip_gpu import _Calls, _golden_request, _sampler
    from scail_amd.sampler import plan_solver
    calls = _Calls(monkeypatch, "sample_tiled", "sample", "step")
    g, net, tiles, c, uc = _golden_request(golden_dir)
    steps, x0 = 4, g["x0"].to(DEV)
    smp = _sampler(steps)
    got = {}
    for solver in ("dpmpp2m", "dpm1"):
        before = dict(calls.n)
        with W.poisoned(W.FILLS["nan"]) as s:
            one = smp.sample_hip(net, x0, c, uc, tile_indices=tiles, solver=solver).clone()
            s.check()
            sizes = {what.split(" ")[0]: ws.numel() for what, ws in s.workspaces}
        assert sizes["scail_dit_solver_bytes"] == net._cstep.solver_bytes(6, 8, 8) == 6 * 16 * 8 * 8 * 4, "one history of the FULL latent"
        assert sizes["scail_dit_sample_tiled_workspace_bytes"] == net._cstep.sample_tiled_workspace_bytes(6, 4, 8, 8)
        assert calls.n["sample_tiled"] == before["sample_tiled"] + 1 and calls.n["step"] == before["step"], "the one-call route was not taken"
        assert smp.last_solver_plan == plan_solver(smp.sigmas(), solver)
        seen = []
        loop = smp.sample_hip(net, x0, c, uc, tile_indices=tiles, solver=solver, step_callback=lambda i, xx: seen.append(i))
        assert seen == list(range(steps)) and calls.n["step"] == before["step"] + steps * len(tiles)
        assert bool(torch.isfinite(one).all()) and not torch.equal(one, x0)
        assert torch.equal(one, loop), f"{solver}: the two routes differ in {int((one != loop).sum())} values"
        got[solver] = one
        net._cstep._hist = None
    assert [i for i, r in enumerate(plan_solver(smp.sigmas(), "dpmpp2m")) if r[2] != 0.0] == [2]
    assert not torch.equal(got["dpmpp2m"], got["dpm1"])
    plain = smp.sample_hip(net, x0, c, uc, tile_indices=tiles)
    assert torch.equal(smp.sample_hip(net, x0, c, uc, tile_indices=tiles, solver=None), plain) and not torch.equal(plain, got["dpm1"])
    assert net._cstep._hist is None


# ---- the raw entry: capture, the workspace contract, refusals -------------------------------------------------------------------------------
def _raw(net, x, inputs, sig, plan, hist, hist_bytes=None, n_char=1, ws=None, sigma=None, said_n_char=None):
    """scail_dit_sample_solver with caller-owned buffers (the binding owns them otherwise); -> the call as a closure, for a capture.
    ``said_n_char``: the character count the call states, when it is to differ from the request's"""
    from scail_amd import lib as L
    from scail_amd.cstep import CStep, _cond_struct
    _, _, ctx, ref, pose, clip = inputs
    ex = net._executor()
    T, H, Wd = x.shape[1], x.shape[3], x.shape[4]
    cond = net._conditioning(ctx, clip)
    cc = _cond_struct(cond)
    cos, sin = _rope(net, (T, H, Wd), n_char)
    ts, dsa, n = ex._schedule(sig, x.device)
    if ws is None:
        ws = torch.empty(L.load().scail_dit_sample_chars_workspace_bytes(ex._h, T, H, Wd, n_char), device=DEV, dtype=torch.uint8)
    sg, co = CStep.solver_tables((sig[:-1] if sigma is None else sigma, plan), n)
    keep = (cond, cc, cos, sin, ts, dsa, ws, sg, co)

    def run():
        assert keep
        L.call("scail_dit_sample_solver", ex._h, x.data_ptr(), ts.data_ptr(), C.cast(dsa, C.c_void_p), n, CFG, C.byref(cc), ref.data_ptr(),
               pose.data_ptr(), n_char if said_n_char is None else said_n_char, pose.shape[1], cos.data_ptr(), sin.data_ptr(), T, H, Wd,
               ws.data_ptr(), ws.numel(), sg, co, None if hist is None else hist.data_ptr(), (0 if hist is None else hist.numel()) if hist_bytes is None else hist_bytes,
               torch.cuda.current_stream().cuda_stream)
    return run


def test_graph_replay_of_a_solver_loop():
    """SIG6's first five values: steps 0, 1 first order, steps 2, 3 second order; the default queue count"""
    net = _net()
    x0, inputs = _request()
    sig = SIG6[:5].clone()
    plan = _plan(sig, "dpmpp2m")
    assert [r[2] != 0.0 for r in plan] == [False, False, True, True]
    ex = net._executor()
    hist = torch.empty(ex.solver_bytes(*SMALL), device=DEV, dtype=torch.uint8)
    eager = x0.clone()
    _raw(net, eager, inputs, sig, plan, hist)()
    want, _ = _compose(net, x0, sig, CFG, inputs, plan)
    assert torch.equal(eager, want)
    xg = x0.clone()
    run = _raw(net, xg, inputs, sig, plan, hist)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                  # warm-up on the capture stream
    torch.cuda.synchronize()
    assert torch.equal(xg, eager)
    xg.copy_(x0)
    hist.fill_(0xFF)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        run()
    for n in (1, 2):
        xg.copy_(x0)
        hist.fill_(0xFF)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(xg, eager), f"graph replay {n}: {int((xg != eager).sum())} values differ"


def test_new_entries_on_poisoned_guarded_buffers(golden_dir):
    """scail_dit_sample_solver and scail_dit_sample_tiled_solver with the workspace and the history handed out at exactly the queried size
    between guard bands, once per fill pattern: the same bits as on ordinary buffers, bands intact, inputs unchanged"""
    from test_longclip_gpu import _golden_request, _sampler
    net = _net()
    x0, inputs = _request()
    ex = net._executor()
    plan = _plan(SIG6, "dpmpp2m")
    g, gnet, tiles, c, uc = _golden_request(golden_dir)
    gx0, smp = g["x0"].to(DEV), _sampler(4)

    def run():
        ex._hist = gnet._executor()._hist = None
        a = _sample(net, x0, inputs, solver=(SIG6[:-1], plan))
        b = smp.sample_hip(gnet, gx0, c, uc, tile_indices=tiles, solver="dpmpp2m").clone()
        ex._hist = gnet._executor()._hist = None
        return a, b

    plain = run()
    snap = W.snapshot(dict(net=net, prepared=net._prepared, inputs=inputs, x0=x0, gnet=gnet, c=c, uc=uc, gx0=gx0))
    for name, fill in W.FILLS.items():
        with W.poisoned(fill) as s:
            got = run()
            s.check()
            whats = [what for what, _ in s.workspaces]
            for q in ("scail_dit_solver_bytes", "scail_dit_sample_chars_workspace_bytes", "scail_dit_sample_tiled_workspace_bytes"):
                assert any(q in w for w in whats), (q, whats)
            sizes = sorted(ws.numel() for what, ws in s.workspaces if "scail_dit_solver_bytes" in what)
            assert sizes == sorted([ex.solver_bytes(*SMALL), ex.solver_bytes(6, 8, 8)]), "the history buffers, at exactly the queried size"
        for gt, p in zip(got, plain):
            assert bool(torch.isfinite(gt).all()), f"fill {name}: non-finite output"
            assert torch.equal(gt, p), f"fill {name}: differs from the plain run in {int((gt != p).sum())} values"
    W.assert_unchanged(snap)


@pytest.mark.parametrize("how", W.TAMPERINGS)
def test_tampered_workspace_is_refused(how):
    from scail_amd import lib as L
    net = _net()
    x0, inputs = _request()
    ex = net._executor()
    _, _, ctx, ref, pose, clip = inputs
    ex._hist = None
    snap = W.snapshot(dict(inputs=inputs, x0=x0))
    with W.poisoned(W.FILLS["big"], out_fill=W.FILLS["nan"]) as s, W.tampered(s, how) as hit:
        with pytest.raises(L.ScailHipError, match="workspace"):
            net.sample_c(x0, SIG6, CFG, ctx, ref, pose, clip, solver=(SIG6[:-1], _plan(SIG6, "dpmpp2m")))
        torch.cuda.synchronize()
        assert hit == ["scail_dit_sample_solver"], hit
        for what, ws in s.workspaces:
            assert W.holds_fill(ws, W.FILLS["big"]), f"{hit[0]} wrote to {what} before it refused"
        s.check()
    ex._hist = None
    W.assert_unchanged(snap)


def test_refusals_leave_x_and_hist_untouched():
    from scail_amd import lib as L
    net = _net()
    x0, inputs = _request()
    ex = net._executor()
    need = ex.solver_bytes(*SMALL)
    hist, hcheck = W.guarded(need, W.FILLS["big"], DEV)
    x = x0.clone()
    plan = _plan(SIG6, "dpmpp2m")

    def with_row(i, row):
        return [row if j == i else r for j, r in enumerate(plan)]

    sig_nan = SIG6[:-1].clone()
    sig_nan[3] = float("nan")
    cases = [
        (r"scail_dit_sample_solver: coef\[4\]\[1\] = inf is not finite", dict(plan=with_row(4, (0.5, float("inf"), 0.0)))),
        (r"scail_dit_sample_solver: coef\[1\]\[0\] = nan is not finite", dict(plan=with_row(1, (float("nan"), 0.5, 0.0)))),
        (r"scail_dit_sample_solver: sigma\[3\] = nan is not finite", dict(sigma=sig_nan)),
        (r"scail_dit_sample_solver: coef\[0\]\[2\] = 0.250000 must be 0: step 0 has no history", dict(plan=with_row(0, (0.5, 0.25, 0.25)))),
        (r"null history buffer", dict(hist=None)),
        (r"history buffer must be 256-byte aligned.*is 128 past", dict(hist=hist[128:])),
        (rf"history buffer too small: {need - 1} bytes, needs {need}", dict(hist_bytes=need - 1)),
        (r"workspace too small", dict(ws=torch.empty(4096, device=DEV, dtype=torch.uint8))),
        (r"n_char must be 1..64, got 0", dict(said_n_char=0)),
    ]
    for needle, kw in cases:
        kw = dict(dict(hist=hist, plan=plan), **kw)
        with pytest.raises(L.ScailHipError, match=needle):
            _raw(net, x, inputs, SIG6, kw.pop("plan"), kw.pop("hist"), **kw)()
    torch.cuda.synchronize()
    hcheck("hist")
    assert torch.equal(x, x0), "a refused call changed x"
    assert W.holds_fill(hist, W.FILLS["big"]), "a refused call wrote into hist"
    # the Python layers
    _, _, ctx, ref, pose, clip = inputs
    ex._hist = None
    with pytest.raises(L.ScailHipError, match=r"one \(a, b, c\) per step \(6\), got 5 sigmas and 2 rows"):
        net.sample_c(x0, SIG6, CFG, ctx, ref, pose, clip, solver=(SIG6[:-2], plan[:2]))
    with pytest.raises(NotImplementedError, match="solver plan together with the step cache or the guidance plan"):
        net.sample_c(x0, SIG6, CFG, ctx, ref, pose, clip, solver=(SIG6[:-1], plan), reuse=[0] * 6)
    with pytest.raises(NotImplementedError, match="solver plan together with the step cache or the guidance plan"):
        net.sample_c(x0, SIG6, CFG, ctx, ref, pose, clip, solver=(SIG6[:-1], plan), guide=[0] * 6)
    assert ex._hist is None, "a refused request allocated a buffer"
