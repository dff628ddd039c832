"""The guidance plan on the GPU (include/scail_dit.h "guidance plan"): the two fp32 kernels against the torch expressions on the CPU, one
branch of the CFG pair as an evaluation against the batch-1 network, and the guided sampler loop against compositions the test makes itself.

No tolerance anywhere: every check is on bits (a NaN is compared as NaN-ness).  Networks and shapes are the step-cache tests' own: toy
networks of 3 layers (D 512 / 256), latents of Ltok 190 and 882, Lt 12, Lc 5, 6 steps."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import ws_contract as W
from test_step_cache_gpu import LARGE, SIG6, SMALL, _fwd, _inputs, _net

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = torch.float32
CFG = 4.0


def _bits32(t):
    return t.detach().contiguous().view(-1).view(torch.int32).cpu()


def _same_f32(got, want, what):
    """bit equality of two fp32 tensors, a NaN compared as NaN-ness"""
    got, want = got.detach().cpu().reshape(-1), want.detach().cpu().reshape(-1)
    assert got.shape == want.shape and got.dtype == want.dtype == f32, what
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f"{what}: NaN in {int((gn != wn).sum())} different places"
    bad = (_bits32(got) != _bits32(want)) & ~wn
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} values differ, first at flat index {int(bad.nonzero()[0])}"


# ---- 1. scail_cfg_delta_store / scail_cfg_euler_delta ---------------------------------------------------------------------------------------
# zeros, subnormals (smallest, largest), the edges of the normal range, infinities, NaNs (quiet, signalling, negative), neighbours of one
# (odd and even last bits), values whose products and sums land on rounding ties (1 + 2^-23 times 3 is 3 + 1.5 ulp), 2^24 and its odd
# neighbour, and ordinary values
CHOSEN = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000, 0x00800001, 0x7f7fffff, 0xff7fffff,
          0x7f7ffffe, 0x7f000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x7f800001, 0x3f800000, 0xbf800000, 0x3f800001, 0xbf800001,
          0x3f7fffff, 0x3f000000, 0x40400000, 0xc0400000, 0x40400001, 0x4b800000, 0x4b800001, 0xcb800001, 0x3eaaaaab, 0x3dcccccd, 0xc0490fdb,
          0x12345678, 0x9abcdef0, 0x5d5e0b6b]
assert len(CHOSEN) == 36 and len(set(CHOSEN)) == 36
SCALARS = [(4.0, -0.15), (1.0, 0.1), (7.5, -1.0)]       # (cfg_scale, dsigma): cfg 1 makes g = 0 (0 * inf = NaN)


def _chosen():
    return torch.tensor(np.array(CHOSEN, dtype=np.uint32).view(np.int32)).view(f32)


def _f(v):
    """a 0-dim fp32 tensor: every torch operation below is one fp32 operation on fp32 operands"""
    return torch.tensor(float(np.float32(v)), dtype=f32)


def cpu_delta(vu, vc):
    return vc - vu


def cpu_euler_delta(x, vc, delta, cfg, ds):
    """x + dsigma * (v_c + g * delta), each operation a separate fp32 op; g = cfg - 1 formed in fp32"""
    g = _f(cfg) - _f(1.0)
    d = vc if delta is None else vc + g * delta
    return x + _f(ds) * d


@pytest.fixture(scope="module")
def crossed():
    """every chosen value against every chosen value (delta: 36^2 pairs) and against every pair (euler: 36^3 triples); the CPU results, once"""
    c = _chosen()
    k = c.numel()
    vu, vc = c.repeat(k), c.repeat_interleave(k)
    x, v3, d3 = c.repeat(k * k), c.repeat_interleave(k).repeat(k), c.repeat_interleave(k * k)
    out = dict(vu=vu, vc=vc, delta=cpu_delta(vu, vc), x=x, v3=v3, d3=d3)
    for cfg, ds in SCALARS:
        out[("euler", cfg, ds)] = cpu_euler_delta(x, v3, d3, cfg, ds)
        out[("plain", cfg, ds)] = cpu_euler_delta(x, v3, None, cfg, ds)
    return out


def test_delta_store_every_chosen_pair(crossed):
    from scail_amd import ops
    e = crossed
    assert torch.isnan(e["delta"]).any() and torch.isinf(e["delta"]).any() and (e["delta"] == 0).any()
    v = torch.stack([e["vu"], e["vc"]]).to(DEV)
    before = _bits32(v)
    out, check = W.guarded_like(torch.empty(e["vu"].numel(), dtype=f32, device=DEV), W.FILLS["big"])
    ops.cfg_delta_store(v, out=out)
    check("cfg_delta_store delta")
    _same_f32(out, e["delta"], "cfg_delta_store")
    assert torch.equal(_bits32(v), before), "v was changed"


@pytest.mark.parametrize("cfg, ds", SCALARS)
def test_euler_delta_every_chosen_triple(crossed, cfg, ds):
    from scail_amd import ops
    e = crossed
    want = e[("euler", cfg, ds)]
    assert torch.isnan(want).any() and torch.isinf(want).any() and torch.isfinite(want).any()
    vc, dl = e["v3"].to(DEV), e["d3"].to(DEV)
    vb, db = _bits32(vc), _bits32(dl)
    for key, delta in (("euler", dl), ("plain", None)):
        x, check = W.guarded_like(torch.empty(e["x"].numel(), dtype=f32, device=DEV), W.FILLS["big"])
        x.copy_(e["x"])
        ops.cfg_euler_delta_(x, vc, delta, cfg, ds)
        check(f"cfg_euler_delta x ({key})")
        _same_f32(x, e[(key, cfg, ds)], f"cfg_euler_delta ({key}, cfg {cfg}, dsigma {ds})")
    assert torch.equal(_bits32(vc), vb) and torch.equal(_bits32(dl), db), "an input was changed"


@pytest.mark.parametrize("n", [1, 255, 257, 7680])
def test_kernels_sizes(n):
    """sizes below, around and above one workgroup of 256 and 30 of them: random data with the chosen values strewn in, outputs between 0xA5
    bands, inputs unchanged, the delta == NULL form"""
    from scail_amd import ops
    g = torch.Generator().manual_seed(n)
    c = _chosen()
    ops_ = [torch.randn(n, generator=g) * s for s in (3.0, 0.5, 1.0, 40.0)]
    for k, t in enumerate(ops_):
        idx = torch.randperm(n, generator=g)[:min(n, 72)]
        t[idx] = c[(torch.arange(idx.numel()) * (k + 5)) % c.numel()]
    x, vu, vc, dl = ops_
    gv, gc, gd = torch.stack([vu, vc]).to(DEV), vc.to(DEV), dl.to(DEV)
    snap = W.snapshot(dict(v=gv, vc=gc, delta=gd))
    out, check = W.guarded_like(torch.empty(n, dtype=f32, device=DEV), W.FILLS["nan"])
    ops.cfg_delta_store(gv, out=out)
    check("cfg_delta_store delta")
    _same_f32(out, cpu_delta(vu, vc), f"cfg_delta_store n {n}")
    for delta_cpu, delta_gpu in ((dl, gd), (None, None)):
        gx, check = W.guarded_like(torch.empty(n, dtype=f32, device=DEV), W.FILLS["nan"])
        gx.copy_(x)
        ops.cfg_euler_delta_(gx, gc, delta_gpu, CFG, -0.15)
        check("cfg_euler_delta x")
        _same_f32(gx, cpu_euler_delta(x, vc, delta_cpu, CFG, -0.15), f"cfg_euler_delta n {n}, delta {'given' if delta_cpu is not None else 'NULL'}")
    W.assert_unchanged(snap)


def test_kernels_do_not_contract():
    """operands for which a fused multiply-add gives other bits than two roundings: 3 * (1 + 2^-23) = 3 + 1.5 ulp rounds to 3 + 2 ulp, so
    -3 + that is 4 * 2^-23 unfused and 3 * 2^-23 fused.  Once in the inner multiply-add (g * delta + v_c), once in the outer (dsigma * d + x)."""
    from scail_amd import ops
    one_ulp = torch.tensor([0x3f800001], dtype=torch.int32).view(f32)           # 1 + 2^-23
    minus3, zero = torch.tensor([-3.0]), torch.tensor([0.0])

    def fused(a, b, c):                                                        # round32(a * b + c): the product is exact in fp64
        return (a.double() * b.double() + c.double()).float()

    # inner: x = 0, dsigma = 1, v_c = -3, g = 3 (cfg 4), delta = 1 + 2^-23
    want = cpu_euler_delta(zero, minus3, one_ulp, 4.0, 1.0)
    contracted = zero + _f(1.0) * fused(_f(3.0), one_ulp, minus3)
    assert float(want) == 4 * 2.0 ** -23 and float(contracted) == 3 * 2.0 ** -23, "the test cannot see a contraction"
    x = zero.to(DEV)
    ops.cfg_euler_delta_(x, minus3.to(DEV), one_ulp.to(DEV), 4.0, 1.0)
    _same_f32(x, want, "inner multiply-add")
    # outer: x = -3, dsigma = 3, v_c = 1 + 2^-23, delta NULL and delta = 0 (g * 0 = 0, v_c + 0 = v_c)
    want = cpu_euler_delta(minus3, one_ulp, None, 4.0, 3.0)
    contracted = fused(_f(3.0), one_ulp, minus3)
    assert float(want) == 4 * 2.0 ** -23 and float(contracted) == 3 * 2.0 ** -23, "the test cannot see a contraction"
    for delta in (None, zero.to(DEV)):
        x = minus3.to(DEV)
        ops.cfg_euler_delta_(x, one_ulp.to(DEV), delta, 4.0, 3.0)
        _same_f32(x, want, "outer multiply-add")


# ---- 2. scail_dit_step_branch -----------------------------------------------------------------------------------------------------------------
def _one(inputs, elem):
    """the batch-1 request under element ``elem`` of the context"""
    x, t, ctx, ref, pose, clip = inputs
    return x[:1].contiguous(), t[:1].contiguous(), ctx[elem:elem + 1].contiguous(), ref, pose, clip


def _rope(net, shape, n_char):
    return net._rope(shape[0], shape[1] // 2, shape[2] // 2, 0, 0, torch.device(DEV), n_char)


def _gemm_name(M, N, K, epi):
    from scail_amd import lib as L
    buf = C.create_string_buffer(128)
    L.call("scail_gemm_kernel_name_for", K, N, 0, M, N, K, epi, 0, buf, 128)
    return buf.value


def _same_conditioning_kernels(net, Lt, batch=2):
    """the text conditioning of one prompt alone (M = Lt) runs the kernels it runs in the batch (M = batch * Lt): a row of it has the same
    bits either way"""
    from scail_amd import lib as L
    D = net.hidden_size
    for N, K, epi in ((D, net.text_dim, L.EPI_GELU_TANH), (D, D, L.EPI_BIAS), (2 * D, D, L.EPI_BIAS)):
        assert _gemm_name(Lt, N, K, epi) == _gemm_name(batch * Lt, N, K, epi), (N, K, epi)


def _branch_case(net, shape, n_char, elem):
    inputs = _inputs(shape, n_char=n_char, pair=True)
    x, t, ctx, ref, pose, clip = inputs
    _same_conditioning_kernels(net, ctx.shape[1])
    cond2 = net._conditioning(ctx, clip)
    one = _one(inputs, elem)
    want = _fwd(net, one).clone()
    cond1 = net._conditioning(one[2], clip)
    for k in ("k_text", "vt_text"):
        assert torch.equal(cond1[k].view(torch.int16), cond2[k][:, elem:elem + 1].view(torch.int16)), f"{k}: the slice of the batch-2 conditioning"
    cos, sin = _rope(net, shape, n_char)
    got = net._executor().step_branch(one[0], one[1], cond2, elem, ref, pose, cos, sin, n_char=n_char)
    assert got.shape == want.shape == (1, shape[0], 16, shape[1], shape[2]) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want), f"branch({elem}) differs from the batch-1 evaluation in {int((got != want).sum())} values"
    return got


@pytest.mark.parametrize("shape", [SMALL, LARGE], ids=["small", "large"])
@pytest.mark.parametrize("n_char", [1, 2])
def test_branch_is_the_batch_one_evaluation(shape, n_char):
    net = _net("toy" if n_char == 1 else "tiny2")
    b0, b1 = (_branch_case(net, shape, n_char, elem) for elem in (0, 1))
    assert not torch.equal(b0, b1), "the two branches carry different conditionings"


def test_branch_fp8():
    net = _net(gemm_precision="fp8", fp8_scaling="row")
    b0, b1 = (_branch_case(net, SMALL, 1, elem) for elem in (0, 1))
    assert net._cstep._fp8_buf is not None and not torch.equal(b0, b1)
    assert not torch.equal(b1, _branch_case(_net(), SMALL, 1, 1)), "the fp8 network is not the bf16 network"


def test_branch_of_a_wider_conditioning():
    """cond_batch 3, elem 2: the conditioning is addressed by (cond_batch, elem), not by the pair's two"""
    net = _net()
    x, t, ctx, ref, pose, clip = _inputs(SMALL, pair=True)
    ctx3 = torch.cat([ctx, ctx[1:2].flip(1)]).contiguous()
    _same_conditioning_kernels(net, ctx.shape[1], batch=3)
    cond3 = {k: v.clone() for k, v in net._conditioning(ctx3, clip).items() if torch.is_tensor(v)}
    want = _fwd(net, (x[:1].contiguous(), t[:1].contiguous(), ctx3[2:3].contiguous(), ref, pose, clip)).clone()
    cos, sin = _rope(net, SMALL, 1)
    got = net._executor().step_branch(x[:1].contiguous(), t[:1].contiguous(), cond3, 2, ref, pose, cos, sin)
    assert torch.equal(got, want)


@pytest.mark.parametrize("elem", [0, 1])
def test_branch_fill_and_reuse_use_one_slot(elem):
    """FILL leaves in slot ``elem`` of the pair's cache what scail_dit_step_cached with B = 1 leaves at offset 0 of its own, REUSE gives that
    evaluation's bits and only reads; the other slot keeps a planted pattern throughout"""
    net = _net()
    ex, D = net._executor(), net.hidden_size
    first, second = _inputs(SMALL, pair=True, seed=11, t=700.0), _inputs(SMALL, pair=True, seed=12, t=350.0)
    ctx, clip = first[2], first[5]
    cond2 = {k: v.clone() for k, v in net._conditioning(ctx, clip).items() if torch.is_tensor(v)}
    cos, sin = _rope(net, SMALL, 1)
    slot = 120 * D * 2                                         # Lnoise * D bf16
    need2, need1 = ex.step_cache_bytes(2, *SMALL), ex.step_cache_bytes(1, *SMALL)
    assert need2 == 2 * need1 == 4 * slot
    cache2, check2 = W.guarded(need2, W.FILLS["big"], DEV)
    cache1, check1 = W.guarded(need1, W.FILLS["big"], DEV)
    f1, s1 = _one(first, elem), _one(second, elem)
    # FILL
    want = ex.step_cached(f1[0], f1[1], net._conditioning(f1[2], clip), f1[3], f1[4], cos, sin, "fill", cache=cache1).clone()
    got = ex.step_branch(f1[0], f1[1], cond2, elem, f1[3], f1[4], cos, sin, mode="fill", cache=cache2).clone()
    check1("B = 1 cache"); check2("pair cache")
    assert torch.equal(got, want) and torch.equal(got, _fwd(net, f1)), "FILL changed the result"
    r = cache2[:2 * slot].view(2, slot)
    assert torch.equal(r[elem], cache1[:slot]), "slot elem of r is not the B = 1 residual"
    assert not W.holds_fill(r[elem], W.FILLS["big"]) and W.holds_fill(r[1 - elem], W.FILLS["big"]), "the other slot of r was written"
    # REUSE on another latent and timestep
    kept = cache2.clone()
    want = ex.step_cached(s1[0], s1[1], None, s1[3], s1[4], cos, sin, "reuse", cache=cache1).clone()
    got = ex.step_branch(s1[0], s1[1], cond2, elem, s1[3], s1[4], cos, sin, mode="reuse", cache=cache2).clone()
    check2("pair cache")
    assert torch.equal(got, want) and not torch.equal(got, _fwd(net, s1)), "REUSE is the B = 1 REUSE, not a full evaluation"
    assert torch.equal(cache2, kept), "REUSE wrote into the cache"


# ---- 3. scail_dit_sample_guided -------------------------------------------------------------------------------------------------------------
def _compose(net, x0, sig, cfg, inputs, guide, reuse=None):
    """the guided loop as the header states it, from forward_f32, the pair's own Euler kernel, and the CPU expressions of the two new
    kernels.  -> (x, delta as the last PAIR step left it or None)"""
    from scail_amd import ops
    _, _, ctx, ref, pose, clip = inputs
    kw = dict(concat_images=torch.zeros(1, device=DEV), image_clip_features=clip, ref_concat=ref, concat_smpl_render=pose)
    x, delta = x0.float().contiguous().clone(), None
    net._executor()._cache = None
    for i, g in enumerate(guide):
        t = (sig[i] * 1000.0).repeat(2).to(DEV)
        ds = float(sig[i + 1] - sig[i])
        sc = {} if reuse is None else dict(step_cache="reuse" if reuse[i] else "fill")
        if g == 0:
            v = net.forward_f32(torch.cat([x, x], 0), t, ctx, None, cfg_pair=True, **kw, **sc)
            delta = cpu_delta(v[0:1].cpu(), v[1:2].cpu())
            ops.cfg_euler_(x, v, cfg, ds)
        else:
            v = net.forward_f32(x, t[:1], ctx[1:2].contiguous(), None, **kw, **sc)
            x = cpu_euler_delta(x.cpu(), v.cpu(), delta if g == 1 else None, cfg, ds).to(DEV)
    net._executor()._cache = None
    return x, delta


def _request(n_char=1, shape=SMALL):
    inputs = _inputs(shape, n_char=n_char)
    return inputs[0][:1].contiguous(), inputs


def _sample(net, x0, inputs, **kw):
    _, _, ctx, ref, pose, clip = inputs
    net._executor()._cache = None
    out = net.sample_c(x0, SIG6, CFG, ctx, ref, pose, clip, **kw).clone()
    net._executor()._cache = None
    return out


@pytest.mark.parametrize("n_char", [1, 2])
def test_all_pair_is_the_plain_sampler_and_keeps_the_last_delta(n_char):
    net = _net("toy" if n_char == 1 else "tiny2")
    x0, inputs = _request(n_char)
    plain = _sample(net, x0, inputs)
    got = _sample(net, x0, inputs, guide=[0] * 6)
    assert torch.equal(got, plain) and bool(torch.isfinite(got).all())
    delta = net._executor().guidance_delta(*SMALL).clone()
    want_x, want_delta = _compose(net, x0, SIG6, CFG, inputs, [0] * 6)
    assert torch.equal(want_x, plain)
    _same_f32(delta, want_delta, "delta after the last PAIR step")
    assert bool((delta != 0).any())


@pytest.mark.parametrize("n_char", [1, 2])
def test_plan_is_the_composition(n_char):
    net = _net("toy" if n_char == 1 else "tiny2")
    x0, inputs = _request(n_char)
    plan = [0, 1, 2, 0, 1, 1]
    want, want_delta = _compose(net, x0, SIG6, CFG, inputs, plan)
    net._executor()._delta = None
    with W.poisoned(W.FILLS["nan"]) as s:
        got = _sample(net, x0, inputs, guide=plan)
        delta = net._executor().guidance_delta(*SMALL).clone()
        s.check()
        assert any("scail_dit_guidance_bytes" in what for what, _ in s.workspaces)
    net._executor()._delta = None
    assert torch.equal(got, want), f"differs from the composition in {int((got != want).sum())} values"
    _same_f32(delta, want_delta, "delta of step 3, the last PAIR step")
    assert bool(torch.isfinite(got).all()) and not torch.equal(got, _sample(net, x0, inputs)), "the plan skipped nothing"


def test_plan_large_shape():
    net = _net()
    x0, inputs = _request(shape=LARGE)
    plan = [2, 0, 1, 0, 2, 1]
    want, _ = _compose(net, x0, SIG6, CFG, inputs, plan)
    assert torch.equal(_sample(net, x0, inputs, guide=plan), want)


def _sampler_request(inputs):
    _, _, ctx, ref, pose, clip = inputs
    shared = dict(concat_images=torch.zeros(1, device=DEV), ref_concat=ref, concat_smpl_render=pose, image_clip_features=clip)
    return dict(crossattn=ctx[1:2], **shared), dict(crossattn=ctx[0:1], **shared)


@pytest.mark.parametrize("option", [dict(guidance=dict(modes=[0, 1, 2, 0, 1, 1])), dict(guidance=dict(every=3)),
                                    dict(guidance=dict(every=2), step_cache=dict(mask=[0, 1, 1, 0, 1, 0]))], ids=["modes", "every", "with_cache"])
def test_sample_hip_routes_agree(option):
    """RFSampler.sample_hip: the one-call route and the host loop (a step callback forces it) take the same plan and give the same bits"""
    from scail_amd.sampler import RFSampler
    net = _net()
    x0, inputs = _request()
    _same_conditioning_kernels(net, inputs[2].shape[1])
    c, uc = _sampler_request(inputs)
    s = RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=6)
    net._executor()._cache = None
    one = s.sample_hip(net, x0, c, uc, scale=CFG, **option).clone()
    plan = list(s.last_guidance_plan)
    assert plan == {"modes": [0, 1, 2, 0, 1, 1], "every": [0, 1, 1, 0, 1, 1], "with_cache": [0, 0, 0, 1, 1, 1]}[
        "with_cache" if "step_cache" in option else next(iter(option["guidance"]))]
    seen = []
    net._executor()._cache = None
    loop = s.sample_hip(net, x0, c, uc, scale=CFG, step_callback=lambda i, xx: seen.append(i), **option)
    net._executor()._cache = None
    assert seen == list(range(6)) and s.last_guidance_plan == plan
    assert torch.equal(one, loop), f"the two routes differ in {int((one != loop).sum())} values"
    assert not torch.equal(one, s.sample_hip(net, x0, c, uc, scale=CFG))


def _raw(net, x, inputs, guide, delta, delta_bytes=None, reuse=None, cache=None, n_char=1, sig=SIG6, ws=None):
    """scail_dit_sample_guided with caller-owned buffers (the binding owns them otherwise); -> the call as a closure, for a capture"""
    from scail_amd import lib as L
    from scail_amd.cstep import _cond_struct
    _, _, ctx, ref, pose, clip = inputs
    ex = net._executor()
    T, H, Wd = x.shape[1], x.shape[3], x.shape[4]
    cond = net._conditioning(ctx, clip)
    cc = _cond_struct(cond)
    cos, sin = _rope(net, (T, H, Wd), n_char)
    ts, dsa, n = ex._schedule(sig, x.device)
    if ws is None:
        ws = torch.empty(L.load().scail_dit_sample_chars_workspace_bytes(ex._h, T, H, Wd, n_char), device=DEV, dtype=torch.uint8)
    g = (C.c_uint8 * max(len(guide), 1))(*guide)
    r = None if reuse is None else (C.c_uint8 * max(len(reuse), 1))(*reuse)
    keep = (cond, cc, cos, sin, ts, dsa, ws, g, r)

    def run():
        assert keep
        L.call("scail_dit_sample_guided", ex._h, x.data_ptr(), ts.data_ptr(), C.cast(dsa, C.c_void_p), len(guide), CFG, C.byref(cc), ref.data_ptr(),
               pose.data_ptr(), n_char, pose.shape[1], cos.data_ptr(), sin.data_ptr(), T, H, Wd, ws.data_ptr(), ws.numel(), g,
               None if delta is None else delta.data_ptr(), (0 if delta is None else delta.numel()) if delta_bytes is None else delta_bytes,
               r, None if cache is None else cache.data_ptr(), 0 if cache is None else cache.numel(), torch.cuda.current_stream().cuda_stream)
    return run


def test_all_cond_neither_reads_nor_writes_delta():
    net = _net()
    x0, inputs = _request()
    want, _ = _compose(net, x0, SIG6, CFG, inputs, [2] * 6)
    assert not torch.equal(want, _sample(net, x0, inputs))
    net._executor()._delta = None
    assert torch.equal(_sample(net, x0, inputs, guide=[2] * 6), want)
    assert net._executor()._delta is None, "a plan of COND entries alone takes no delta buffer"
    need = net._executor().guidance_bytes(*SMALL)
    for name, fill in W.FILLS.items():
        delta, check = W.guarded(need, fill, DEV)
        x = x0.clone()
        _raw(net, x, inputs, [2] * 6, delta)()
        check(f"delta ({name})")
        assert torch.equal(x, want), f"delta filled with {name}: the result depends on it"
        assert W.holds_fill(delta, fill), f"delta filled with {name}: it was written"
    x = x0.clone()
    _raw(net, x, inputs, [2] * 6, None)()
    assert torch.equal(x, want), "delta == NULL"


def test_with_the_step_cache():
    net = _net()
    x0, inputs = _request()
    guide, reuse = [0, 0, 1, 1, 2, 2], [0, 1, 0, 1, 0, 1]
    want, _ = _compose(net, x0, SIG6, CFG, inputs, guide, reuse)
    got = _sample(net, x0, inputs, guide=guide, reuse=reuse)
    assert torch.equal(got, want), f"differs from the composition in {int((got != want).sum())} values"
    assert bool(torch.isfinite(got).all()) and not torch.equal(got, _sample(net, x0, inputs, guide=guide))
    mask = [0, 1, 0, 1, 1, 0]
    assert torch.equal(_sample(net, x0, inputs, guide=[0] * 6, reuse=mask), _sample(net, x0, inputs, reuse=mask)), "all-PAIR with a mask"
    assert torch.equal(_sample(net, x0, inputs, guide=[0] * 6, reuse=[0] * 6), _sample(net, x0, inputs))


def test_graph_replay_of_a_guided_loop():
    net = _net()
    x0, inputs = _request()
    sig3, plan = SIG6[:4].clone(), [0, 1, 2]
    ex = net._executor()
    delta = torch.empty(ex.guidance_bytes(*SMALL), device=DEV, dtype=torch.uint8)
    eager = x0.clone()
    _raw(net, eager, inputs, plan, delta, sig=sig3)()
    want, _ = _compose(net, x0, sig3, CFG, inputs, plan)
    assert torch.equal(eager, want)
    xg = x0.clone()
    run = _raw(net, xg, inputs, plan, delta, sig=sig3)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                  # warm-up on the capture stream
    torch.cuda.synchronize()
    assert torch.equal(xg, eager)
    xg.copy_(x0)
    delta.fill_(0xFF)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        run()
    xg.copy_(x0)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(xg, eager), f"graph replay: {int((xg != eager).sum())} values differ"


# ---- 4. the workspace contract --------------------------------------------------------------------------------------------------------------
def test_new_entries_on_poisoned_guarded_buffers():
    """sample_guided (with and without the step cache) and step_branch with every buffer handed out at exactly the queried size between
    guard bands, once per fill pattern: the same bits as on ordinary buffers, bands intact, inputs unchanged"""
    net = _net()
    x0, inputs = _request()
    ex = net._executor()
    x, t, ctx, ref, pose, clip = inputs
    cond2 = {k: v.clone() for k, v in net._conditioning(ctx, clip).items() if torch.is_tensor(v)}
    cos, sin = _rope(net, SMALL, 1)
    x1, t1 = x[:1].contiguous(), t[:1].contiguous()

    def run():
        ex._delta = None
        a = _sample(net, x0, inputs, guide=[0, 1, 2, 0, 1, 1])
        b = _sample(net, x0, inputs, guide=[0, 0, 1, 1, 2, 2], reuse=[0, 1, 0, 1, 0, 1])
        c = ex.step_branch(x1, t1, cond2, 1, ref, pose, cos, sin).clone()
        d = ex.step_branch(x1, t1, cond2, 1, ref, pose, cos, sin, mode="fill").clone()
        e = ex.step_branch(x1, t1, cond2, 1, ref, pose, cos, sin, mode="reuse").clone()
        ex._cache = ex._delta = None
        return a, b, c, d, e

    plain = run()
    snap = W.snapshot(dict(net=net, prepared=net._prepared, inputs=inputs, x0=x0, cond=cond2))
    for name, fill in W.FILLS.items():
        with W.poisoned(fill) as s:
            got = run()
            s.check()
            whats = [what for what, _ in s.workspaces]
            for q in ("scail_dit_guidance_bytes", "scail_dit_step_cache_bytes", "scail_dit_sample_chars_workspace_bytes", "scail_dit_chars_workspace_bytes"):
                assert any(q in w for w in whats), (q, whats)
            for what, ws in s.workspaces:
                if "scail_dit_guidance_bytes" in what:
                    assert ws.numel() == ex.guidance_bytes(*SMALL), "the delta buffer, at exactly the queried size"
        for g, p in zip(got, plain):
            assert bool(torch.isfinite(g).all()), f"fill {name}: non-finite output"
            assert torch.equal(g, p), f"fill {name}: differs from the plain run in {int((g != p).sum())} values"
    W.assert_unchanged(snap)


@pytest.mark.parametrize("how", W.TAMPERINGS)
@pytest.mark.parametrize("entry", ["sample_guided", "step_branch"])
def test_tampered_workspace_is_refused(entry, how):
    from scail_amd import lib as L
    net = _net()
    x0, inputs = _request()
    ex = net._executor()
    x, t, ctx, ref, pose, clip = inputs
    cond2 = {k: v.clone() for k, v in net._conditioning(ctx, clip).items() if torch.is_tensor(v)}
    cos, sin = _rope(net, SMALL, 1)
    ex._cache = ex._delta = None
    snap = W.snapshot(dict(inputs=inputs, x0=x0, cond=cond2))
    with W.poisoned(W.FILLS["big"], out_fill=W.FILLS["nan"]) as s, W.tampered(s, how) as hit:
        with pytest.raises(L.ScailHipError, match="workspace"):
            if entry == "sample_guided":
                net.sample_c(x0, SIG6, CFG, ctx, ref, pose, clip, guide=[0, 1, 2, 0, 1, 1], reuse=[0, 0, 0, 0, 0, 0])
            else:
                ex.step_branch(x[:1].contiguous(), t[:1].contiguous(), cond2, 1, ref, pose, cos, sin, mode="fill")
        torch.cuda.synchronize()
        assert hit == ["scail_dit_" + entry], hit
        for what, ws in s.workspaces:
            assert W.holds_fill(ws, W.FILLS["big"]), f"{hit[0]} wrote to {what} before it refused"
        for o in s.outs:
            assert W.holds_fill(o, W.FILLS["nan"]), f"{hit[0]} wrote to its output before it refused"
        s.check()
    ex._cache = ex._delta = None
    W.assert_unchanged(snap)


# ---- 5. refusals that need a handle ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_x_delta_and_cache_untouched():
    from scail_amd import lib as L
    net = _net()
    x0, inputs = _request()
    ex = net._executor()
    need, cneed = ex.guidance_bytes(*SMALL), ex.step_cache_bytes(2, *SMALL)
    delta, dcheck = W.guarded(need, W.FILLS["big"], DEV)
    cache, ccheck = W.guarded(cneed, W.FILLS["big"], DEV)
    x = x0.clone()
    cases = [
        (r"guide\[3\] = 3 ", dict(guide=[0, 1, 2, 3, 0, 0])),
        (r"guide\[1\] = 1 \(delta\) has no pair step before it", dict(guide=[2, 1, 0, 0, 0, 0])),
        (r"null delta buffer", dict(guide=[0] * 6, delta=None)),
        (r"null delta buffer", dict(guide=[2, 2, 0, 1, 2, 2], delta=None)),
        (r"delta buffer must be 256-byte aligned.*is 128 past", dict(guide=[0] * 6, delta=delta[128:])),
        (rf"delta buffer too small: {need - 1} bytes, needs {need}", dict(guide=[0] * 6, delta_bytes=need - 1)),
        (r"reuse\[0\] = 1", dict(guide=[0] * 6, reuse=[1, 0, 0, 0, 0, 0], cache=cache)),
        (r"reuse\[4\] = 2 ", dict(guide=[0] * 6, reuse=[0, 0, 0, 0, 2, 0], cache=cache)),
        (r"null cache", dict(guide=[0] * 6, reuse=[0, 1, 0, 1, 0, 1], cache=None)),
        (rf"cache too small: {cneed - 1} bytes, needs {cneed}", dict(guide=[0] * 6, reuse=[0, 1, 0, 1, 0, 1], cache=cache[:cneed - 1])),
        (r"cache must be 256-byte aligned", dict(guide=[0] * 6, reuse=[0, 1, 0, 1, 0, 1], cache=cache[64:])),
        (r"step 1 reuses \(guide 1\) what step 0, the last computing step, left \(guide 0\)", dict(guide=[0, 1, 0, 0, 0, 0], reuse=[0, 1, 0, 0, 0, 0], cache=cache)),
        (r"step 5 reuses \(guide 0\) what step 4, the last computing step, left \(guide 2\)", dict(guide=[0, 0, 1, 1, 2, 0], reuse=[0, 1, 0, 1, 0, 1], cache=cache)),
        (r"workspace too small", dict(guide=[0] * 6, ws=torch.empty(4096, device=DEV, dtype=torch.uint8))),
    ]
    for needle, kw in cases:
        kw = dict(dict(delta=delta), **kw)
        with pytest.raises(L.ScailHipError, match=needle):
            _raw(net, x, inputs, kw.pop("guide"), kw.pop("delta"), **kw)()
    torch.cuda.synchronize()
    dcheck("delta"); ccheck("cache")
    assert torch.equal(x, x0), "a refused call changed x"
    assert W.holds_fill(delta, W.FILLS["big"]) and W.holds_fill(cache, W.FILLS["big"]), "a refused call wrote into delta / the cache"
    # the branch
    xx, t, ctx, ref, pose, clip = inputs
    cond2 = net._conditioning(ctx, clip)
    cos, sin = _rope(net, SMALL, 1)
    x1, t1 = xx[:1].contiguous(), t[:1].contiguous()
    with pytest.raises(L.ScailHipError, match=r"elem must lie in \[0, cond_batch = 2\), got 2"):
        ex.step_branch(x1, t1, cond2, 2, ref, pose, cos, sin)
    with pytest.raises(L.ScailHipError, match=r"elem must lie in \[0, cond_batch = 2\), got -1"):
        ex.step_branch(x1, t1, cond2, -1, ref, pose, cos, sin)
    with pytest.raises(L.ScailHipError, match="mode must be None or one of"):
        ex.step_branch(x1, t1, cond2, 1, ref, pose, cos, sin, mode="refill")
    with pytest.raises(L.ScailHipError, match="ONE latent and ONE timestep"):
        ex.step_branch(xx, t, cond2, 1, ref, pose, cos, sin)
    with pytest.raises(L.ScailHipError, match=rf"scail_dit_step_branch: cache too small: {cneed - 1} bytes, needs {cneed}"):
        ex.step_branch(x1, t1, cond2, 1, ref, pose, cos, sin, mode="fill", cache=cache[:cneed - 1])
    ex._cache = None
    with pytest.raises(L.ScailHipError, match="needs a 'fill' evaluation"):
        ex.step_branch(x1, t1, cond2, 1, ref, pose, cos, sin, mode="reuse")
    torch.cuda.synchronize()
    assert W.holds_fill(cache, W.FILLS["big"])


def test_python_refusals():
    from scail_amd import lib as L
    from scail_amd.sampler import RFSampler, RFSamplerLong
    net = _net()
    x0, inputs = _request()
    _, _, ctx, ref, pose, clip = inputs
    ex = net._executor()
    ex._cache = ex._delta = None
    with pytest.raises(L.ScailHipError, match="one entry per step"):
        net.sample_c(x0, SIG6, CFG, ctx, ref, pose, clip, guide=[0, 1])
    with pytest.raises(L.ScailHipError, match="one entry per step"):
        net.sample_c(x0, SIG6, CFG, ctx, ref, pose, clip, guide=[0] * 6, reuse=[0, 1])
    ex._cache = ex._delta = None
    c, uc = _sampler_request(inputs)
    long = RFSamplerLong(hunyuan_schedule=True, shift_scale=5, num_steps=2)
    with pytest.raises(NotImplementedError, match="guidance with temporal tiles"):
        long.sample_hip(net, x0, dict(c, smpl_tiled=pose[:, None]), uc, tile_indices=[[0, 1], [1, 2]], guidance=dict(every=2))
    s = RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=2)
    settings = [("sp", types.SimpleNamespace(size=2, rank=0)), ("use_c_step", False), ("_tap", lambda i, h: None), ("kernel_timer", {}), ("_c_blocks", True)]
    for attr, value in settings:
        old = getattr(net, attr)
        setattr(net, attr, value)
        try:
            with pytest.raises(NotImplementedError, match="guidance"):
                net.sample_c(x0, SIG6, CFG, ctx, ref, pose, clip, guide=[0, 1, 2, 0, 1, 1])
            if attr != "_c_blocks":
                with pytest.raises(NotImplementedError, match="guidance"):
                    s.sample_hip(net, x0, c, uc, scale=CFG, guidance=dict(modes=[0, 1]))
        finally:
            setattr(net, attr, old)
    with pytest.raises(NotImplementedError, match="guidance"):
        s.sample_hip(net, x0, c, uc, scale=CFG, chunk_dim=3, guidance=dict(every=2))
    assert ex._cache is None and ex._delta is None, "a refused request allocated a buffer"
