"""scail_flash_attn_vrows_bf16 (self-attention on v as the QKV projection wrote it: scail_attn4_m16f_vr / scail_attn4_m16f_q3_vr) on the GPU: every
case asserts its kernels through the name query and is torch.equal to scail_transpose_v + scail_flash_attn_bf16 on the same inputs -- the same keys
sit in the same MFMA k-slots in the same order, so there is no tolerance.  v lies inside a NaN-filled allocation: the rows behind key Lk - 1 and the
columns beside it are NaN, and a kernel that touched them (0 x NaN is NaN) would not come out finite and equal.  tests/test_attn_vrows_cpu.py has
the emulator, the refusals and the generator."""
import pytest
import torch

import attn_exact as X

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
VR = {256: "scail_attn4_m16f_vr", 192: "scail_attn4_m16f_q3_vr"}


@pytest.fixture(scope="module")
def ops():
    from scail_amd import lib, ops as _ops
    lib.load()
    assert torch.cuda.is_available()
    return _ops


def nan_buf(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=BF16)


def vr_name(q, k, v, o, plan=True):
    import ctypes as C
    from scail_amd import lib as L
    B, Lq, D = q.shape
    buf, pl = C.create_string_buffer(128), (C.c_int64 * 9)()
    L.call("scail_flash_attn_vrows_kernel_name_for", q.stride(1), k.stride(1), v.stride(1), o.stride(1), B, D // X.HD, Lq, k.shape[1], buf, len(buf),
           C.cast(pl, C.c_void_p) if plan else None)
    launches = [dict(zip(("rows", "item0", "n_items", "xcd_mode"), pl[1 + 4 * i:5 + 4 * i])) for i in range(pl[0])]
    return buf.value.decode(), launches


def place(x, cols=1, col=0, pad_rows=0):
    """x (B, L, D) on the device as columns [col D, (col + 1) D) of rows [0, L) of a NaN-filled (B, L + pad_rows, cols D) buffer"""
    B, L, D = x.shape
    buf = nan_buf(B, L + pad_rows, cols * D)
    view = buf[:, :L, col * D:(col + 1) * D]
    view.copy_(x.to(BF16).to(DEV))
    return view


def both_routes(ops, q, k, v, H, raw=False, want=None, opts=None):
    """the V-rows entry and today's two calls on the same device tensors under the same options: (o_vrows, o_vt) on the CPU; asserts the query's
    answer, the kernel names (want: the expected name, or None = any V-rows plan) and that the V^T route runs the V^T kernels of the same plan"""
    from scail_amd import lib as L
    B, Lq, D = q.shape
    Lk = k.shape[1]
    kw = dict(scale=X.raw_scale()) if raw else dict(q_prescaled=True)

    def run():
        o1, o0 = nan_buf(B, Lq, D), nan_buf(B, Lq, D)
        assert L.load().scail_flash_attn_vrows_for(q.stride(1), k.stride(1), v.stride(1), o1.stride(1), B, H, Lq, Lk) == 1
        name, launches = vr_name(q, k, v, o1)
        assert name == " + ".join(VR[l["rows"]] for l in launches) and (want is None or name == want), (name, want)
        name0, plan0 = X.kernel_name(q.stride(1), k.stride(1), o0.stride(1), B, H, Lq, Lk, False, not raw, plan=True)
        assert name0 == name.replace("_vr", "") and plan0["launches"] == launches, (name0, plan0, launches)
        ops.flash_attn_vrows(q, k, v, out=o1, **kw)
        ops.flash_attn(q, k, ops.transpose_v(v, H), out=o0, **kw)
        torch.cuda.synchronize()
        return o1.cpu(), o0.cpu(), launches

    o1, o0, launches = X.conv_exact.with_options(opts, run, dict(X.OPTION_DEFAULTS, attn_vrows=1)) if opts else run()
    assert bool(torch.isfinite(o1.float()).all()), "non-finite output: the kernel met a NaN of the allocation around v"
    assert torch.equal(o1, o0), f"V-rows kernels against scail_transpose_v + scail_flash_attn_bf16: {int((o1 != o0).sum())} elements differ"
    return o1, launches


def randn(B, L, D, seed):
    return torch.randn(B, L, D, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("rows", X.HEIGHTS)
@pytest.mark.parametrize("Lk", [512, 513, 575, 1088])
def test_every_tail_at_both_heights(ops, Lk, rows):
    """8 tiles exactly, 1 and 63 keys in a ninth, 17 tiles; q, k, v the three column thirds of one NaN-padded buffer (v_rs = 3 x 128 heads), 64 NaN
    rows behind key Lk - 1; raw scale at the ragged counts"""
    B, H, Lq = 2, 2, 300
    D = H * X.HD
    raw = Lk in (513, 575)
    q = place(randn(B, Lq, D, Lk) * (1.0 if raw else 0.1275), 3, 0, 20)
    k, v = place(randn(B, Lk, D, Lk + 1), 3, 1, 64), place(randn(B, Lk, D, Lk + 2), 3, 2, 64)
    both_routes(ops, q, k, v, H, raw=raw, want=VR[rows], opts={"attn4_rows": rows})


@pytest.mark.parametrize("cols,raw", [(1, False), (2, True), (3, False)], ids=["v_rs-1x", "v_rs-2x-raw", "v_rs-3x"])
def test_v_row_and_batch_strides(ops, cols, raw):
    """v_rs = 128 heads, 2 x and 3 x that (v the LAST column block of its buffer), a batch stride of (Lk + 7) rows; k and q with strides of their own"""
    B, H, Lq, Lk = 2, 4, 257, 520
    D = H * X.HD
    q = place(randn(B, Lq, D, 5) * (1.0 if raw else 0.1275))
    k, v = place(randn(B, Lk, D, 6), 2, 0, 3), place(randn(B, Lk, D, 7), cols, cols - 1, 7)
    assert v.stride(1) == cols * D and v.stride(0) == (Lk + 7) * cols * D
    both_routes(ops, q, k, v, H, raw=raw)


@pytest.mark.parametrize("B,H", [(3, 3), (2, 4), (1, 3)], ids=["nine-pairs", "eight-pairs", "three-pairs"])
def test_workgroup_id_decodes(ops, B, H):
    """nine pairs: 8 runs of the item list (mode 2, padded grid); eight pairs: pairs dealt to the XCDs (mode 1); three: the plain decode"""
    Lq, Lk, D = 400, 576, H * X.HD
    q, k, v = place(randn(B, Lq, D, 11) * 0.1275), place(randn(B, Lk, D, 12)), place(randn(B, Lk, D, 13), 1, 0, 1)
    _, launches = both_routes(ops, q, k, v, H, opts={"attn4_rows": 256})
    assert [l["xcd_mode"] for l in launches] == [X.expected_xcd_mode(B * H, {})]


def test_planned_two_launch_shape_with_the_split_inside_a_pair(ops):
    """option "attn4_cus" makes the plan count on a few CUs; the smallest Lq <= 1024 for which one pair gets whole rounds of 256-row workgroups + 192-row
    workgroups from a 768-row boundary on: both launches run their V-rows kernel, every row once"""
    from scail_amd import lib as L
    lib = L.load()
    found = None
    try:
        for Lq in range(832, 1025, 64):
            for cus in range(1, 17):
                L.set_option("attn4_cus", cus)
                if found is None and lib.scail_flash_attn_rows_for(1, 1, Lq) == 448:
                    found = (cus, Lq)
    finally:
        L.set_option("attn4_cus", 0)
    assert found is not None, "no planned two-launch shape up to 1024 rows"
    cus, Lq = found
    q, k, v = place(randn(1, Lq, X.HD, 21) * 0.1275), place(randn(1, 600, X.HD, 22)), place(randn(1, 600, X.HD, 23), 1, 0, 2)
    _, launches = both_routes(ops, q, k, v, 1, want=VR[256] + " + " + VR[192], opts={"attn4_cus": cus})
    first, second = launches
    n4, n3 = -(-Lq // 256), -(-Lq // 192)
    assert first["item0"] == 0 and 0 < first["n_items"] < n4 and first["n_items"] % 3 == 0
    assert second["item0"] == first["n_items"] // 3 * 4 and second["item0"] + second["n_items"] == n3


RESTART_CASES = [c for c in X.G4_CASES if c["form"] == "restart"]


@pytest.mark.parametrize("rows", X.HEIGHTS)
@pytest.mark.parametrize("case", RESTART_CASES, ids=lambda c: c["id"])
def test_restarts_on_exact_operands(ops, case, rows):
    """the restart cases of tests/test_attn_exact_gpu.py (the c = 64 key overflows the optimistic pass of the target rows, one in each of the four
    waves; thresholds 8, 0 and 2 for the lazy-maximum loop that runs again): the V-rows kernels restart the same workgroups, the exact operands
    pass the checker, and the result equals the V^T route bit for bit"""
    from scail_amd import lib as L
    d = X.self_case(case)
    B, H, Lq = case["B"], case["H"], case["Lq"]
    q, k, v = (place(d[n], 1, 0, 5) for n in ("q", "k", "v"))
    ctr = torch.zeros(1, device=DEV, dtype=torch.int32)
    L.call("scail_flash_attn_count_restarts", ctr.data_ptr())
    try:
        o, _ = both_routes(ops, q, k, v, H, want=VR[rows], opts=dict(case["opts"], attn4_rows=rows))
    finally:
        L.call("scail_flash_attn_count_restarts", None)
    want = len({t // rows for t in X.TARGETS if t < Lq}) * B * H
    assert int(ctr.item()) == 2 * want, (int(ctr.item()), want)          # both routes restart them
    X.check_interval_bf16(o, d["r"]["ref"], d["r"]["lo"], d["r"]["hi"], f"{case['id']} {VR[rows]}")


# ---- the executor -------------------------------------------------------------------------------------------------------------------------------
TOY = dict(hidden_size=512, num_attention_heads=4, inner_hidden_size=1024, text_dim=64, time_freq_dim=256, time_embed_dim=512)
T, HL, WL = 2, 32, 32                       # 3 x 256 + 2 x 64 = 896 tokens: 14 key tiles


def _option(value, fn):
    return X.conv_exact.with_options({"attn_vrows": value}, fn, {"attn_vrows": 1})


def test_executor_one_step_equals_the_transpose_route(ops):
    import test_parallel_gpu as P
    from scail_amd import lib as L
    x, t, ctx, ref, pose, clip = P._inputs(T, HL, WL, 1, 64, 12, 5, seed=11)
    net = P._mk(TOY, 3, seed=77)
    run = lambda: net.forward_f32(x, t, ctx, None, concat_images=torch.zeros(1, device=DEV), image_clip_features=clip, ref_concat=ref, concat_smpl_render=pose)
    Ltok, D = 896, 512
    assert L.load().scail_flash_attn_vrows_for(3 * D, 3 * D, 3 * D, D, 2, 4, Ltok, Ltok) == 1
    on, off = _option(1, run), _option(0, run)
    torch.cuda.synchronize()
    assert net._cstep is not None, "the C executor must have run"
    assert bool(torch.isfinite(on).all()) and torch.equal(on, off)


@pytest.mark.parametrize("world,mode,chunk_dim", [(2, "allgather", 3), (4, "ulysses", 4)])
def test_executor_virtual_ranks_equal_the_transpose_route(ops, world, mode, chunk_dim):
    """the gathered V of the all-gather branch (row stride 2 D) and of the ulysses branch (3 D / ranks): option 1 against option 0"""
    import test_parallel_gpu as P
    from scail_amd import lib as L
    inputs = P._inputs(T, HL, WL, 1, 64, 12, 5, seed=11)
    mk = lambda: P._mk(TOY, 3, seed=77)
    D, Lf = 512, 896
    Dn, Hn = (D // world, 4 // world) if mode == "ulysses" else (D, 4)
    rs = (3 * Dn, 3 * Dn, 3 * Dn, Dn) if mode == "ulysses" else (3 * D, 2 * D, 2 * D, D)
    assert L.load().scail_flash_attn_vrows_for(*rs, 1, Hn, Lf if mode == "ulysses" else Lf // world, Lf) == 1
    on = _option(1, lambda: P._run_ranks(world, mode, mk, inputs, chunk_dim, use_c=True))
    off = _option(0, lambda: P._run_ranks(world, mode, mk, inputs, chunk_dim, use_c=True))
    assert bool(torch.isfinite(on).all()) and torch.equal(on, off)
