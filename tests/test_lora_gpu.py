"""LoRA adapters on the GPU (include/scail_hip.h scail_lora_merge_bf16 / scail_add_scaled_bf16; scail_amd/lora.py): the two kernels
against the torch expression on the CPU (tests/lora_ref.py: one tensor operation per arithmetic operation), and merged networks against
fresh networks loaded from the CPU-merged state dict.

No tolerance anywhere: every check is on bits (a NaN is compared as NaN-ness).  The networks are the step-cache tests' 3-layer toy
network (D 512), built fresh here: a merge changes weights in place, so the shared cached instances of test_step_cache_gpu._net are
not touched."""
import numpy as np
import pytest
import torch

import lora_ref as R
import ws_contract as W
from test_guidance_gpu import _same_f32
from test_step_cache_gpu import SIG6, SMALL, TOY, _fwd, _inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32, bf16 = torch.float32, torch.bfloat16
ULP = 2.0 ** -23
SCALE = R.scale_of(0.37, 1, 1)

# (N, K, r): tile edges in both axes (the merge kernel's tile is 64 x 128), a K that is no multiple of 8, more than one workgroup in both
# axes, and ranks around the LDS chunk of the r loop -- LORA_RC = 32 in scail_amd/csrc/lora.hip: 33 is one chunk and a tail of one, 64
# two whole chunks, 97 three and a tail of one, 300 nine and a tail of twelve
SIZES = [(1, 1, 1), (3, 5, 2), (64, 256, 4), (65, 257, 7), (130, 520, 33), (256, 1024, 64), (8, 8, 300), (70, 136, 97)]


def _window_case(N, K, r, ldw=None, ld_up=None, ld_down=None, off=0, seed=0, diff=False):
    """(guarded device buffer that holds the window, its check, device window, CPU copy of the buffer before, CPU window of that copy,
    CPU factors, device factors)"""
    g = torch.Generator().manual_seed(seed + 1000 * N + 10 * K + r)
    ldw = K if ldw is None else ldw
    ld_up = max(r, 1) if ld_up is None else ld_up
    ld_down = K if ld_down is None else ld_down
    n = off + max(N - 1, 0) * ldw + K + 5
    buf, check = W.guarded_like(torch.empty(n, dtype=bf16, device=DEV), W.FILLS["big"])
    host = torch.randn(n, generator=g).to(bf16)                     # what lies around the window is data too: it must keep its bits
    buf.copy_(host)
    win = torch.as_strided(buf, (N, K), (ldw, 1), buf.storage_offset() + off)     # (as_strided counts from the storage's start)
    hwin = torch.as_strided(host, (N, K), (ldw, 1), off)
    if diff:
        d = torch.randn(N, ld_down, generator=g)
        return buf, check, win, host, hwin, (d[:, :K],), (d.to(DEV)[:, :K],)
    up, down = torch.randn(N, ld_up, generator=g), torch.randn(r, ld_down, generator=g)
    return buf, check, win, host, hwin, (up[:, :r], down[:, :K]), (up.to(DEV)[:, :r], down.to(DEV)[:, :K])


def _run_case(N, K, r, diff=False, **kw):
    from scail_amd import ops
    buf, check, win, host, hwin, cpu, dev = _window_case(N, K, r, diff=diff, **kw)
    want = host.clone()
    wwin = torch.as_strided(want, hwin.shape, hwin.stride(), hwin.storage_offset())
    if diff:
        wwin.copy_(R.cpu_add_scaled(hwin.contiguous(), cpu[0].contiguous(), SCALE))
        ops.add_scaled_(win, dev[0], SCALE)
    else:
        wwin.copy_(R.cpu_merge(hwin.contiguous(), cpu[0].contiguous(), cpu[1].contiguous(), SCALE))
        ops.lora_merge_(win, dev[0], dev[1], SCALE)
    check(f"{'add_scaled' if diff else 'lora_merge'} {(N, K, r)} {kw}")
    R.same_bf16(buf, want, f"{'add_scaled' if diff else 'lora_merge'} {(N, K, r)} {kw}")
    assert not torch.equal(R.bits16(want), R.bits16(host)) or N * K * (1 if diff else r) == 0


# ---- 1. the kernels against the expression ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, K, r", SIZES)
def test_merge_is_the_expression(N, K, r):
    _run_case(N, K, r)


@pytest.mark.parametrize("N, K, r", [(3, 5, 2), (65, 257, 7), (64, 256, 33)])
def test_merge_strides_and_guards(N, K, r):
    _run_case(N, K, r, ldw=K + 3, ld_up=r + 2, ld_down=K + 1)        # nothing 16-byte aligned past row 0
    _run_case(N, K, r, ldw=(K + 15) // 8 * 8, ld_up=r + 3, ld_down=K + 4)   # a padded, 16-byte aligned leading dimension: vector rows with a tail


@pytest.mark.parametrize("off", [1, 2, 3])
def test_merge_unaligned_base(off):
    _run_case(65, 264, 7, off=off)
    _run_case(65, 264, 7, off=off, ldw=272)


@pytest.mark.parametrize("N, K, r", [(4, 16, 0), (0, 16, 3), (4, 0, 3)])
def test_empty_problems_leave_w_alone(N, K, r):
    from scail_amd import ops
    w = torch.tensor([-0.0, float("nan"), float("inf"), 1.0] * 16, dtype=bf16).view(4, 16).to(DEV)
    before = R.bits16(w)
    win = w[:N, :K]
    ops.lora_merge_(win, torch.ones(N, r, device=DEV), torch.ones(r, K, device=DEV), 2.0)
    if r:
        ops.add_scaled_(win, torch.ones(N, K, device=DEV), 2.0)
    torch.cuda.synchronize()
    assert torch.equal(R.bits16(w), before)


# values of scale * acc (merge: r = 1, up = the value, down = 1, scale = 1): zeros, half-ulp ties of several binades (2^-8 is half a bf16
# ulp of [1, 2), 2^-4 of [16, 32), 2^12 of [2^20, 2^21), 3 * 2^-9 sits between), a value lost against most weights, values whose sum with
# a large weight overflows bf16, infinities and a NaN
SWEEP = [0.0, -0.0, 2.0 ** -8, -2.0 ** -8, 2.0 ** -4, 2.0 ** 12, 3 * 2.0 ** -9, 1.2345678, -2.0 ** -60, 3.0e38, -3.3e38, float("inf"), float("-inf"),
         float("nan")]


@pytest.fixture(scope="module")
def sweep():
    """all 65 536 bf16 values as w, crossed with SWEEP: (w (V, 65536) bf16, values (V,) fp32, {scale: expected of add_scaled, "merge": expected of the r = 1 merge})"""
    allw = torch.tensor(np.arange(65536, dtype=np.uint16).view(np.int16)).view(bf16)
    v = torch.tensor(SWEEP, dtype=f32)
    w = allw.unsqueeze(0).repeat(len(SWEEP), 1).contiguous()
    d = v.unsqueeze(1).repeat(1, 65536).contiguous()
    want = {s: R.cpu_add_scaled(w, d, s) for s in (1.0, -0.75)}
    want["merge"] = R.cpu_merge(w, v.view(-1, 1), torch.ones(1, 65536), 1.0)      # acc = 0 + v * 1: v itself, but +0 for v = -0
    return w, v, want


def test_sweep_sees_what_it_should(sweep):
    w, v, want = sweep
    e = want[1.0]
    assert torch.isnan(e).any() and torch.isinf(e).any() and (e == 0).any()
    assert bool((torch.isinf(e) & torch.isfinite(w) & torch.isfinite(v).unsqueeze(1)).any()), "no sum overflows bf16"
    exact = w.double() + v.double().unsqueeze(1)
    ok = torch.isfinite(e) & (e != 0)
    ties = ok & ((exact - e.double()).abs() == 0.5 * R.bf16_ulp(torch.where(ok, e.double(), torch.ones_like(exact))))
    assert int(ties.sum()) > 1000 and len({int(torch.floor(torch.log2(x.abs()))) for x in e[ties][::97].double()}) >= 3


def test_merge_every_bf16_value(sweep):
    from scail_amd import ops
    w, v, want = sweep
    gw, check = W.guarded_like(torch.empty(w.shape, dtype=bf16, device=DEV), W.FILLS["big"])
    gw.copy_(w)
    ops.lora_merge_(gw, v.view(-1, 1).to(DEV), torch.ones(1, 65536, device=DEV), 1.0)
    check("lora_merge sweep")
    R.same_bf16(gw, want["merge"], "lora_merge over every bf16 value")


@pytest.mark.parametrize("scale", [1.0, -0.75])
def test_add_scaled_every_bf16_value(sweep, scale):
    from scail_amd import ops
    w, v, want = sweep
    gw, check = W.guarded_like(torch.empty(w.shape, dtype=bf16, device=DEV), W.FILLS["big"])
    gw.copy_(w)
    ops.add_scaled_(gw, v.unsqueeze(1).repeat(1, 65536).contiguous().to(DEV), scale)
    check("add_scaled sweep")
    R.same_bf16(gw, want[scale], f"add_scaled over every bf16 value (scale {scale})")


# ---- no contraction, and the order of the sum ----------------------------------------------------------------------------------------------
ONE_ULP = 1.0 + ULP                # 3 * (1 + 2^-23) = 3 + 1.5 ulp(3) rounds to 3 + 4 * 2^-23; fused with -3 it is 3 * 2^-23
# name -> (w, up [r], down [r], scale): the multiply-add named is the only place where fusing changes the result
CONTRACTIONS = {
    "acc + up * down": (0.0, [-3.0, 3.0], [1.0, ONE_ULP], 1.0),          # acc = -3 after j = 0
    "w + scale * acc": (-3.0, [ONE_ULP], [1.0], 3.0),
}


def _fma(a, b, c):
    """round32(a * b + c): the product of two fp32 values is exact in fp64"""
    return (a.double() * b.double() + c.double()).float()


def _contracted(name, w, up, down, scale):
    one = lambda x: torch.tensor([float(np.float32(x))], dtype=f32)
    acc = torch.zeros(1, dtype=f32)
    for j in range(len(up)):
        acc = _fma(one(up[j]), one(down[j]), acc) if name.startswith("acc") and j == len(up) - 1 else acc + one(up[j]) * one(down[j])
    s = _fma(one(scale), acc, one(w)) if name.startswith("w +") else one(w) + one(scale) * acc
    return s.to(bf16)


@pytest.mark.parametrize("name", list(CONTRACTIONS))
def test_kernels_do_not_contract(name):
    from scail_amd import ops
    w, up, down, scale = CONTRACTIONS[name]
    r = len(up)
    u1, d1 = torch.tensor([up], dtype=f32), torch.tensor(down, dtype=f32).view(r, 1)
    want = R.cpu_merge(torch.tensor([[w]], dtype=bf16), u1, d1, scale)
    fused = _contracted(name, w, up, down, scale)
    assert float(want) == 4 * ULP and float(fused) == 3 * ULP, f"the test cannot see a contraction of {name}: {float(want)} {float(fused)}"
    for N, K, off in ((1, 1, 0), (3, 5, 1), (1, 8, 0), (4, 24, 0)):          # the scalar path (a tail; an unaligned base), 16-byte rows
        buf = torch.full((off + N * K,), w, dtype=bf16, device=DEV)
        win = torch.as_strided(buf, (N, K), (K, 1), off)
        ops.lora_merge_(win, u1.repeat(N, 1).to(DEV), d1.repeat(1, K).to(DEV), scale)
        R.same_bf16(win, want.repeat(N, K), f"lora_merge: {name} {(N, K, off)}")
    if name.startswith("w +"):
        acc = R.cpu_acc(u1, d1)
        for N, K, off in ((1, 1, 0), (3, 5, 1), (1, 8, 0), (4, 24, 0)):
            buf = torch.full((off + N * K,), w, dtype=bf16, device=DEV)
            win = torch.as_strided(buf, (N, K), (K, 1), off)
            ops.add_scaled_(win, acc.repeat(N, K).to(DEV), scale)
            R.same_bf16(win, want.repeat(N, K), f"add_scaled: {name} {(N, K, off)}")


def test_sum_runs_over_ascending_j():
    from scail_amd import ops
    up, down = torch.tensor([[1.0e8, -1.0e8, 1.0]], dtype=f32), torch.ones(3, 1, dtype=f32)
    want = R.cpu_acc(up, down)
    assert float(want) == 1.0 and float(R.cpu_acc(up, down, order=[2, 1, 0])) == 0.0           # descending loses the 1
    assert float(up[0, 0] * 1 + (up[0, 1] * 1 + up[0, 2] * 1)) == 0.0                          # and so does a pairwise tree from the right
    for N, K in ((1, 1), (5, 24)):
        w = torch.zeros(N, K, dtype=bf16, device=DEV)
        ops.lora_merge_(w, up.repeat(N, 1).to(DEV), down.repeat(1, K).to(DEV), 1.0)
        R.same_bf16(w, torch.ones(N, K, dtype=bf16), f"order {(N, K)}")


# ---- add_scaled: the same sizes and alignments ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, K, r", SIZES)
def test_add_scaled_is_the_expression(N, K, r):
    _run_case(N, K, r, diff=True)
    _run_case(N, K, r, diff=True, ldw=K + 3, ld_down=K + 1)
    _run_case(N, K, r, diff=True, ldw=(K + 15) // 8 * 8, ld_down=(K + 7) // 4 * 4)


@pytest.mark.parametrize("off", [1, 2, 3])
def test_add_scaled_unaligned_base(off):
    _run_case(65, 264, 1, diff=True, off=off)
    _run_case(1, 1531, 1, diff=True, off=off)                # one long row, as a bias or a modulation table is


# ---- row windows of a fused matrix -----------------------------------------------------------------------------------------------------------
def test_slices_of_a_fused_matrix():
    from scail_amd import ops
    D = 128
    g = torch.Generator().manual_seed(5)
    host = torch.randn(3 * D, D, generator=g).to(bf16)
    pairs = [(torch.randn(D, r, generator=g), torch.randn(r, D, generator=g)) for r in (2, 5, 1)]
    w = host.to(DEV)
    for j, (up, down) in enumerate(pairs):
        ops.lora_merge_(w[j * D:(j + 1) * D], up.to(DEV), down.to(DEV), SCALE)
    want = torch.cat([R.cpu_merge(host[j * D:(j + 1) * D], up, down, SCALE) for j, (up, down) in enumerate(pairs)])
    R.same_bf16(w, want, "q, k, v windows")
    w = host.to(DEV)
    ops.lora_merge_(w[D:2 * D], pairs[1][0].to(DEV), pairs[1][1].to(DEV), SCALE)
    R.same_bf16(w, torch.cat([host[:D], want[D:2 * D], host[2 * D:]]), "k alone")


# ---- networks ------------------------------------------------------------------------------------------------------------------------------------
def _mk(**kw):
    import test_parallel_gpu as P
    return P._mk(dict(TOY, **kw), 3, seed=77)


def _adapter(net, seed, scale=0.05):
    """every aliased module of ``net``: a pair (ranks 1, 2, 5; fp32, fp16, bf16; every third with an alpha != rank) on the matrices and a
    difference on everything else, with the bias difference of every fourth linear"""
    from scail_amd import lora
    g = torch.Generator().manual_seed(seed)
    spec, t = net.param_spec(), {}
    for i, (name, tgt) in enumerate(lora.wan_aliases(net).items()):
        shape = spec[tgt.weight]
        rows = shape[0] if tgt.rows is None else tgt.rows
        dt = (f32, torch.float16, bf16)[i % 3]
        if len(shape) == 2:
            r = (1, 2, 5)[i % 3]
            a, b = (".lora_A.weight", ".lora_B.weight") if i % 2 else (".lora_down.weight", ".lora_up.weight")
            t[name + a] = (torch.randn(r, shape[1], generator=g) * scale).to(dt)
            t[name + b] = (torch.randn(rows, r, generator=g) * scale).to(dt)
            if i % 3 == 0:
                t[name + ".alpha"] = torch.tensor(1.5)
            if i % 4 == 0 and tgt.bias is not None:
                t[name + ".diff_b"] = (torch.randn(rows, generator=g) * 0.02).to(dt)
        else:
            t[("diffusion_model." if i % 2 else "") + name + ".diff"] = (torch.randn(shape, generator=g) * 0.02).to(dt)
            if tgt.bias is not None:
                t[name + ".diff_b"] = (torch.randn(spec[tgt.bias], generator=g) * 0.02).to(dt)
    return t


def _steps(net, tensors, strength):
    from scail_amd import lora
    plan = lora.plan_adapter(net, tensors, strength)
    for e in plan:
        assert e.scale == (R.scale_of(strength, e.alpha, e.rank) if e.kind == "lora" else R.scale_of(strength, 1, 1))
    return [(e.param, e.row_offset, e.rows, e.kind, e.up, e.down, e.scale) for e in plan]


def _cpu_sd(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def _twin(sd, **kw):
    twin = _mk(**kw)
    twin.load_state_dict({k: v.to(DEV) for k, v in sd.items()})
    return twin


def test_merged_parameters_are_the_cpu_merge():
    net = _mk()
    base = _cpu_sd(net)
    t = _adapter(net, 1)
    rows = net.merge_lora(t, 0.8)
    want = R.cpu_apply(base, _steps(net, t, 0.8))
    touched = {r[0] for r in rows}
    assert len(rows) > 60 and net.loras == [("<dict>", 0.8, len(rows))]
    for k, v in net.state_dict().items():
        R.same_bf16(v, want[k], k)
        assert (k in touched) != torch.equal(R.bits16(v), R.bits16(base[k])), k
    assert len(touched) < len(base)                                          # the patch embeddings have no alias: they keep their bits


@pytest.mark.parametrize("kw", [{}, dict(gemm_precision="fp8"), dict(gemm_precision="fp8", fp8_scaling="mx"), dict(gemm_precision="fp6")],
                         ids=["bf16", "fp8", "mx", "fp6"])
def test_merged_network_is_a_fresh_network_of_the_merged_weights(kw):
    """with a forward pass BEFORE the merge under the same cond_key: a stale conditioning cache, executor binding, prepared vector or
    quantised weight buffer shows"""
    net = _mk(**kw)
    inputs = _inputs(SMALL)
    before = _fwd(net, inputs, cond_key="request").clone()
    t = _adapter(net, 2)
    want = R.cpu_apply(_cpu_sd(net), _steps(net, t, 1.0))
    net.merge_lora(t)
    got = _fwd(net, inputs, cond_key="request").clone()
    ref = _fwd(_twin(want, **kw), inputs, cond_key="request")
    assert bool(torch.isfinite(got).all()) and not torch.equal(got, before)
    _same_f32(got, ref, f"forward_f32 after merge_lora ({kw})")


def test_two_adapters_and_the_sampler(tmp_path):
    from safetensors.torch import save_file
    net = _mk()
    x, _, ctx, ref, pose, clip = inputs = _inputs(SMALL)
    first = net.sample_c(x[:1], SIG6, 4.0, ctx, ref, pose, clip, cond_key="request").clone()
    t1, t2 = _adapter(net, 3), _adapter(net, 4)
    path = str(tmp_path / "second.safetensors")
    save_file({k: v.contiguous() for k, v in t2.items()}, path)
    want = R.cpu_apply(R.cpu_apply(_cpu_sd(net), _steps(net, t1, 0.6)), _steps(net, t2, -0.4))
    net.merge_lora(t1, 0.6)
    net.merge_lora(path, -0.4)
    assert [l[:2] for l in net.loras] == [("<dict>", 0.6), (path, -0.4)]
    for k, v in net.state_dict().items():
        R.same_bf16(v, want[k], k)
    twin = _twin(want)
    _same_f32(_fwd(net, inputs, cond_key="request"), _fwd(twin, inputs, cond_key="request"), "forward_f32 after two adapters")
    got = net.sample_c(x[:1], SIG6, 4.0, ctx, ref, pose, clip, cond_key="request")
    _same_f32(got, twin.sample_c(x[:1], SIG6, 4.0, ctx, ref, pose, clip, cond_key="request"), "sample_c after two adapters")
    assert not torch.equal(got, first)


def test_a_bad_last_key_leaves_every_parameter_alone():
    net = _mk()
    base = _cpu_sd(net)
    t = _adapter(net, 5)
    t["blocks.2.ffn.2.diff"] = torch.zeros(3, 3)                              # the last key: a difference of the wrong shape
    with pytest.raises(ValueError, match=r"blocks\.2\.ffn\.2\.diff: a difference of shape \(3, 3\)"):
        net.merge_lora(t)
    assert net.loras == []
    for k, v in net.state_dict().items():
        assert torch.equal(R.bits16(v), R.bits16(base[k])), k


def test_cli_lora(tmp_path, capsys):
    from scail_amd import cli
    engine = cli.build_engine(cli.TINY)
    t = _adapter(engine.network, 6, scale=0.1)
    path = str(tmp_path / "adapter.pt")
    torch.save(t, path)
    out = [str(tmp_path / f"out{i}.pt") for i in range(2)]
    capsys.readouterr()
    cli.main(["--tiny", "--steps", "2", "--out", out[0]])
    assert "lora " not in capsys.readouterr().out
    cli.main(["--tiny", "--steps", "2", "--lora", f"{path}:0.5", "--out", out[1]])
    text = capsys.readouterr().out
    n = len(_steps(engine.network, t, 0.5))
    assert f"lora {path}: {n} entries" in text and "rank 1..5, alpha 1.5..5, strength 0.5" in text
    plain, merged = (torch.load(o)["latent"] for o in out)
    assert bool(torch.isfinite(merged).all()) and not torch.equal(plain, merged)
    rows = engine.load_lora(path, 0.5)
    assert len(rows) == n and engine.network.loras == [(path, 0.5, n)]
    _, z, _ = cli.run(cli.TINY, steps=2, engine=engine)
    assert torch.equal(z.cpu(), merged)
    with pytest.raises(ValueError, match="merge them into a passed engine once"):
        cli.run(cli.TINY, steps=2, engine=engine, loras=[(path, 0.5)])
