"""GPU tests of the MX block scaling of the fp8 per-token GEMMs (include/scail_hip.h scail_quant_mxfp8_rows / scail_gemm_mxfp8,
include/scail_dit.h scail_dit_enable_fp8_scaled): the quantizer bit for bit against the tests' reference (tests/test_mxfp8_cpu.py), the
GEMM's scale map one (row, block) at a time, the GEMM bit for bit on exact operands with random block exponents (every epilogue), a
planted outlier that costs its own block where per-row scaling loses the row, the 14B shapes on random data, the executor under
fp8_scaling="mx" (CFG pair, determinism, enable / disable, block-wise path, sequence-parallel refusal, workspace), accuracy against the
goldens next to per-row scaling, the probe under MX and the command line.  Executor network: hidden 256, 2 heads, FF 512, 3 layers,
2 x 224 token rows (that of tests/test_fp8_probe_gpu.py)."""
import copy
import ctypes
import math

import pytest
import torch

from oracle import scail_oracle as O
from test_fp8_cpu import e4m3_value
from test_fp8_gpu import P14B, _cos, _fwd, _golden_kw, _inputs, _load, _mk, _net_golden
from test_fp8_probe_gpu import CFGD, CSTAR, D, FF, LAYERS, LTOK, W2, _planted
from test_mxfp8_cpu import BLOCK, dequant_mxfp8, quant_mxfp8_rows_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ONE = 0x38                    # e4m3 code of 1.0


# ---- scail_quant_mxfp8_rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,ld", [(257, 5120, 5120), (64, 13824, 13888), (7, 128, 160), (1, 32, 32)])
def test_quant_matches_reference_bit_exactly(rows, cols, ld):
    from scail_amd import ops
    g = torch.Generator().manual_seed(3 + rows)
    x = torch.randn(rows, cols, generator=g) * torch.logspace(-20, 20, rows)[:, None]
    if rows >= 7:
        x[0] = 0.0                                          # zero row
        x[1] = 0.0
        x[1, cols // 2] = -3.0e30                           # one huge element: its block keeps it, the others are zero blocks
        x[2] = torch.randn(cols, generator=g) * 1e-30       # tiny row
        x[3] = -0.0
        x[4] = 448.0                                        # the saturation value itself
        blk = torch.arange(cols) // BLOCK                   # blocks alternate between magnitude 1 and 2^20
        x[5] = torch.randn(cols, generator=g) * torch.where(blk % 2 == 0, 1.0, 2.0 ** 20)
    xb = x.to(torch.bfloat16)
    buf = torch.zeros(rows, ld, dtype=torch.bfloat16)
    buf[:, :cols] = xb
    src = buf.to(DEV)[:, :cols]
    q, e = ops.quant_mxfp8_rows(src)
    # the same into a code matrix and a scale matrix with row strides of their own (the padding must stay untouched)
    q2 = torch.full((rows, cols + 8), 0xAA, dtype=torch.uint8, device=DEV)
    e2 = torch.full((rows, cols // BLOCK + 3), 0xAA, dtype=torch.uint8, device=DEV)
    ops.quant_mxfp8_rows(src, out=q2[:, :cols], scale=e2[:, :cols // BLOCK])
    torch.cuda.synchronize()
    qr, er = quant_mxfp8_rows_ref(xb)
    assert e.dtype == torch.uint8 and tuple(e.shape) == (rows, cols // BLOCK)
    assert int((e.cpu() != er).sum()) == 0, f"{int((e.cpu() != er).sum())} scale bytes differ at {(rows, cols)}"
    assert int((q.cpu() != qr).sum()) == 0, f"{int((q.cpu() != qr).sum())} codes differ at {(rows, cols)}"
    assert torch.equal(q2[:, :cols], q) and torch.equal(e2[:, :cols // BLOCK], e)
    assert bool((q2[:, cols:] == 0xAA).all()) and bool((e2[:, cols // BLOCK:] == 0xAA).all())
    assert not bool((e == 255).any()) and not bool(((q & 0x7F) == 0x7F).any())
    if rows >= 7:
        assert bool((e[0] == 127).all()) and not bool(q[0].any()) and bool((e[3] == 127).all()) and not bool(q[3].any())
        assert bool((e[4] == 127).all()) and bool((q[4] == 0x7E).all())
        assert int((e[1] != 127).sum()) == 1 and int((q[1] != 0).sum()) == 1


# ---- scail_gemm_mxfp8: which scale byte reaches which products -------------------------------------------------------------------
def test_gemm_scale_map_one_row_and_block_at_a_time():
    """K = 256 (two k-tiles of two MFMA steps of two blocks), M = N = 128, every code 1.0 and every scale byte 127: y = 256 everywhere.
    Raising one scale byte by 3 must raise exactly that row (x) or column (w) of y by 32 (2^3 - 1) = 224: the byte at (row, block) scales
    the 32 products of that row and block and nothing else.  Rows 0, 31, 32, 127 x the 8 blocks cover the step ks, the lane half g, the
    k-tile parity and the fragment index, on both operands."""
    from scail_amd import ops
    M = N = 128
    K = 256
    xq = torch.full((M, K), ONE, dtype=torch.uint8, device=DEV)
    wq = torch.full((N, K), ONE, dtype=torch.uint8, device=DEV)
    ex = torch.full((M, K // BLOCK), 127, dtype=torch.uint8, device=DEV)
    ew = torch.full((N, K // BLOCK), 127, dtype=torch.uint8, device=DEV)
    base = ops.gemm_mxfp8(xq, ex, wq, ew).float().cpu()
    assert bool((base == 256.0).all())
    for r in (0, 31, 32, 127):
        for b in range(K // BLOCK):
            want = torch.full((M, N), 256.0)
            want[r, :] += 32.0 * (2 ** 3 - 1)
            ex[r, b] = 130
            got = ops.gemm_mxfp8(xq, ex, wq, ew).float().cpu()
            ex[r, b] = 127
            assert torch.equal(got, want), f"x scale (row {r}, block {b}): rows changed {sorted(set((got != 256).nonzero()[:, 0].tolist()))}, " \
                                           f"values {sorted(set(got[got != 256].tolist()))}"
            ew[r, b] = 130
            got = ops.gemm_mxfp8(xq, ex, wq, ew).float().cpu()
            ew[r, b] = 127
            assert torch.equal(got, want.T), f"w scale (row {r}, block {b}): columns changed {sorted(set((got != 256).nonzero()[:, 1].tolist()))}, " \
                                             f"values {sorted(set(got[got != 256].tolist()))}"


def test_gemm_scale_byte_reaches_exactly_its_own_32_columns():
    """The test above cannot see WHICH 32 products of the row a scale byte reaches (every code is 1).  Here the other operand is the
    identity, w[j, k] = (k == j), so y[i, j] = x[i, j] 2^(the scale applied to column j of x): with ex[i, b] = 127 + b, y[i, j] must be
    2^(j / 32) -- the byte of block b scales columns 32 b .. 32 b + 31 of the row-major operand and no others.  (The hardware applies a
    lane's scale to one 16-byte half of both lanes of a row, not to the lane's own 32 bytes: the kernel deals its bytes to match.)  Then
    the same with the roles of x and w swapped.  K = 256: both k-tiles."""
    from scail_amd import ops
    M = N = K = 256
    ones = torch.full((M, K), ONE, dtype=torch.uint8, device=DEV)
    eye = torch.zeros(N, K, dtype=torch.uint8, device=DEV)
    eye[torch.arange(N), torch.arange(K)] = ONE
    unit = torch.full((M, K // BLOCK), 127, dtype=torch.uint8, device=DEV)
    ramp = (127 + torch.arange(K // BLOCK, dtype=torch.uint8, device=DEV)).repeat(M, 1).contiguous()
    want = torch.pow(2.0, (torch.arange(K) // BLOCK).float()).repeat(M, 1)
    got = ops.gemm_mxfp8(ones, ramp, eye, unit).float().cpu()
    assert torch.equal(got, want), f"x: block applied to each column of row 0: {got[0].log2().tolist()}"
    got = ops.gemm_mxfp8(eye, unit, ones, ramp).float().cpu()
    assert torch.equal(got, want.T), f"w: block applied to each column of row 0: {got[:, 0].log2().tolist()}"


# ---- scail_gemm_mxfp8: exact operands, every epilogue ----------------------------------------------------------------------------
def _mx_int_operands(M, N, K, lda, ldex, g, vmax=3):
    """e4m3 codes of small integers (exact), an ASYMMETRIC W, block exponents drawn per (row, block) from {-2, -1, 0, 1} for both operands"""
    xi = torch.randint(-vmax, vmax + 1, (M, K), generator=g).float()
    wi = torch.randint(-vmax, vmax + 1, (N, K), generator=g).float()
    wi[0, :] = torch.arange(K).remainder(7).float() - 3          # a structured, non-symmetric row
    px = torch.randint(-2, 2, (M, K // BLOCK), generator=g)
    pw = torch.randint(-2, 2, (N, K // BLOCK), generator=g)
    xq = torch.zeros(M, lda, dtype=torch.uint8)
    xq[:, :K] = xi.to(torch.float8_e4m3fn).view(torch.uint8)
    ex = torch.full((M, ldex), 255, dtype=torch.uint8)            # the padding holds the NaN byte: it must never be read as a scale
    ex[:, :K // BLOCK] = (px + 127).to(torch.uint8)
    wq = wi.to(torch.float8_e4m3fn).view(torch.uint8).contiguous()
    ew = (pw + 127).to(torch.uint8).contiguous()
    return xi, wi, px, pw, xq, ex, wq, ew


@pytest.mark.parametrize("M,N,K", [(1, 128, 128), (97, 384, 256), (300, 256, 640), (513, 512, 1152), (260, 256, 13824)])
def test_gemm_mxfp8_exact_every_epilogue(M, N, K):
    from scail_amd import lib as L, ops
    g = torch.Generator().manual_seed(M * 7 + N + K)
    lda, ldex = K + 16, K // BLOCK + 4
    xi, wi, px, pw, xq, ex, wq, ew = _mx_int_operands(M, N, K, lda, ldex, g)
    # every partial sum is an integer multiple of 2^-4 below 9 K 2^2 (|code| <= 3, both block scales <= 2): it fits 24 bits, so the fp32
    # accumulation is exact in any order
    assert 9 * K * 2 ** 2 * 2 ** 4 < 2 ** 24
    xdq = xi.double() * torch.pow(2.0, px.double()).repeat_interleave(BLOCK, 1)
    wdq = wi.double() * torch.pow(2.0, pw.double()).repeat_interleave(BLOCK, 1)
    v = xdq @ wdq.T                                               # exact in fp64
    assert float(v.abs().max()) * 16 < 2 ** 24 and torch.equal(v.float().double(), v)
    bias = torch.randint(-8, 9, (N,), generator=g).float()
    xq_d, ex_d = xq.to(DEV)[:, :K], ex.to(DEV)[:, :K // BLOCK]
    wq_d, ew_d, b_d = wq.to(DEV), ew.to(DEV), bias.to(DEV)
    assert xq_d.stride(0) == lda and ex_d.stride(0) == ldex
    # the bf16 GEMM on the dequantized operands (exact in bf16: small integers times powers of two)
    xd = xdq.to(torch.bfloat16).to(DEV)
    wd = wdq.to(torch.bfloat16).to(DEV).contiguous()
    assert torch.equal(xd.double().cpu(), xdq) and torch.equal(wd.double().cpu(), wdq)

    # BIAS: bit-exact against the fp64 product (+ integer bias, exact) rounded once to bf16
    y = ops.gemm_mxfp8(xq_d, ex_d, wq_d, ew_d, b_d)
    want = (v + bias.double()).to(torch.bfloat16)
    assert torch.equal(y.cpu(), want), f"max |d| {float((y.double().cpu() - want.double()).abs().max())}"
    assert torch.equal(y, ops.gemm(xd, wd, b_d))
    # no bias
    assert torch.equal(ops.gemm_mxfp8(xq_d, ex_d, wq_d, ew_d).cpu(), v.to(torch.bfloat16))
    # GELU-tanh: the same epilogue code as the bf16 kernel on the same fp32 values
    yg = ops.gemm_mxfp8(xq_d, ex_d, wq_d, ew_d, b_d, epilogue=L.EPI_GELU_TANH)
    assert torch.equal(yg, ops.gemm(xd, wd, b_d, epilogue=L.EPI_GELU_TANH))
    ref = torch.nn.functional.gelu(v + bias.double(), approximate="tanh")
    torch.testing.assert_close(yg.double().cpu(), ref, rtol=8e-3, atol=1e-3)
    # RESID ungated, resid aliasing y, output with a row stride > N
    r0 = torch.randint(-64, 65, (M, N), generator=g).float().to(torch.bfloat16)
    out = torch.zeros(M, N + 128, dtype=torch.bfloat16, device=DEV)[:, :N]
    out.copy_(r0.to(DEV))
    ops.gemm_mxfp8(xq_d, ex_d, wq_d, ew_d, b_d, out=out, epilogue=L.EPI_RESID, resid=out)
    ob = torch.zeros(M, N + 128, dtype=torch.bfloat16, device=DEV)[:, :N]
    ob.copy_(r0.to(DEV))
    ops.gemm(xd, wd, b_d, out=ob, epilogue=L.EPI_RESID, resid=ob)
    assert torch.equal(out, ob)
    assert torch.equal(out.cpu(), (r0.double() + v + bias.double()).to(torch.bfloat16))
    # RESID gated, rows_per_batch: gate[(m / rpb), n]; both kernels share the epilogue -> same bits as the bf16 kernel
    rpb = max(1, (M + 1) // 2)
    nb = (M + rpb - 1) // rpb
    gate = torch.randn(nb, 2 * N, generator=g).to(DEV)[:, :N]
    o8 = r0.to(DEV).clone()
    o16 = r0.to(DEV).clone()
    ops.gemm_mxfp8(xq_d, ex_d, wq_d, ew_d, b_d, out=o8, epilogue=L.EPI_RESID, resid=o8, gate=gate, rows_per_batch=rpb)
    ops.gemm(xd, wd, b_d, out=o16, epilogue=L.EPI_RESID, resid=o16, gate=gate, rows_per_batch=rpb)
    assert torch.equal(o8, o16)
    gm = gate.cpu().repeat_interleave(rpb, 0)[:M]
    torch.testing.assert_close(o8.double().cpu(), r0.double() + gm.double() * (v + bias.double()), rtol=8e-3, atol=1e-2)


# ---- planted outlier: what the feature buys --------------------------------------------------------------------------------------
def test_gemm_planted_outlier_costs_one_block_where_row_scaling_loses_the_row():
    """K = 256, x in {1, 2, 3} except column 137 = 2^24 in every row; W integers with column 137 zero.  Under MX the outlier's block
    (columns 128 .. 159) keeps the outlier and flushes its 31 neighbours; the other 7 blocks are exact: the result is, bit for bit, the
    product of x with columns 128 .. 159 zeroed.  Per-row scaling flushes every entry but the outlier (448 * 3 / 2^24 < 2^-10): all zeros."""
    from scail_amd import ops
    M, N, K, c = 97, 128, 256, 137
    g = torch.Generator().manual_seed(17)
    x = torch.randint(1, 4, (M, K), generator=g).float()
    x[:, c] = 2.0 ** 24
    w = torch.randint(-3, 4, (N, K), generator=g).float()
    w[:, c] = 0.0
    xb, wb = x.to(torch.bfloat16).to(DEV), w.to(torch.bfloat16).to(DEV)
    assert torch.equal(xb.float().cpu(), x) and torch.equal(wb.float().cpu(), w)
    x0 = x.clone().double()
    x0[:, 128:160] = 0.0
    want = (x0 @ w.double().T).to(torch.bfloat16)                 # |sum| <= 9 * 224: exact in fp32, rounded once
    assert float(want.float().abs().max()) > 0.0
    xq, ex = ops.quant_mxfp8_rows(xb)
    wq, ew = ops.quant_mxfp8_rows(wb)
    y_mx = ops.gemm_mxfp8(xq, ex, wq, ew)
    assert torch.equal(y_mx.cpu(), want), f"max |d| {float((y_mx.float().cpu() - want.float()).abs().max())}"
    xr, sx = ops.quant_fp8_rows(xb)
    wr, sw = ops.quant_fp8_rows(wb)
    y_row = ops.gemm_fp8(xr, sx, wr, sw)
    assert bool((y_row == 0).all()), "per-row scaling was expected to lose every row to the outlier"


# ---- scail_gemm_mxfp8: random data at the 14B shapes -----------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(15360, 5120), (5120, 5120), (13824, 5120), (5120, 13824)])
def test_gemm_mxfp8_random_matches_dequantized_product(N, K):
    from scail_amd import ops
    M = 4099
    g = torch.Generator(device=DEV).manual_seed(N + K)
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV, generator=g) * 0.02).to(torch.bfloat16)
    b = torch.randn(N, device=DEV, generator=g)
    xq, ex = ops.quant_mxfp8_rows(x)
    wq, ew = ops.quant_mxfp8_rows(w)
    y = ops.gemm_mxfp8(xq, ex, wq, ew, b)
    rows = torch.tensor([0, 1, 255, 256, 2047, 4000, M - 1])
    xd = dequant_mxfp8(xq[rows].cpu(), ex[rows].cpu())
    wd = dequant_mxfp8(wq.cpu(), ew.cpu())
    ref = xd @ wd.T + b.cpu().double()
    mag = xd.abs() @ wd.abs().T
    err = (y[rows].double().cpu() - ref).abs()
    # bf16 output rounding (2^-9 relative, with margin) + fp32 accumulation over K (measured up to ~2e-6 of sum |a b|); the reference is
    # the dequantized product, so the bound is that of the per-row test
    assert bool((err <= 2.0 ** -8 * ref.abs() + 1e-5 * mag + 1e-6).all()), float((err - 2.0 ** -8 * ref.abs() - 1e-5 * mag).max())


# ---- executor ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs():
    return _inputs(2, 16, 16, 64, 12, 5)


@pytest.fixture(scope="module")
def plain(inputs):
    """(bf16, per-row fp8, MX fp8) step outputs of the seed-1234 network: computed once, read by several tests, never written"""
    o16 = _fwd(_mk(CFGD, LAYERS), inputs)
    o8 = _fwd(_mk(CFGD, LAYERS, gemm_precision="fp8"), inputs)
    omx = _fwd(_mk(CFGD, LAYERS, gemm_precision="fp8", fp8_scaling="mx"), inputs)
    assert torch.isfinite(omx).all() and not torch.equal(o16, o8) and not torch.equal(o16, omx) and not torch.equal(o8, omx)
    return o16, o8, omx


def test_mx_cfg_pair_determinism_and_blockwise(inputs, plain):
    _, _, omx = plain
    net = _mk(CFGD, LAYERS, gemm_precision="fp8", fp8_scaling="mx")
    assert torch.equal(_fwd(net, inputs), omx) and torch.equal(_fwd(net, inputs), omx), "two MX runs differ"
    assert net._cstep is not None and net._cstep._fp8_buf is not None and net._cstep.fp8_scaling == "mx"
    # the CFG pair (equal latents, two contexts): with and without SCAIL_DIT_CFG_PAIR the same bits -- a block lies inside a row
    x, t, ctx, ref, pose, clip = inputs
    pair = (torch.cat([x[:1], x[:1]]).contiguous(), t, ctx, ref, pose, clip)
    outs = [_fwd(net, pair, cfg_pair=p) for p in (False, True)]
    assert not torch.equal(outs[0][0], outs[0][1])
    assert torch.equal(outs[0], outs[1]), f"cfg_pair changed the MX result: max |d| {float((outs[0] - outs[1]).abs().max())}"
    # the same network driven block by block through scail_dit_block (the last layer then runs all rows: the step's row pruning is exact)
    net._c_blocks = True
    o_blocks = _fwd(net, inputs)
    net._c_blocks = False
    assert torch.equal(o_blocks, omx), f"max |d| {float((o_blocks - omx).abs().max())}"


def test_mx_enable_row_disable_restores_the_bits(inputs, plain):
    from scail_amd import lib as L
    o16, o8, omx = plain
    net = _mk(CFGD, LAYERS, gemm_precision="fp8", fp8_scaling="mx")
    assert torch.equal(_fwd(net, inputs), omx)
    ex = net._executor()
    ex.enable_fp8(L.FP8_ALL, DEV, scaling="row")
    assert torch.equal(_fwd(net, inputs), o8), "enable(mx) -> enable(row) is not the per-row result"
    ex.enable_fp8(L.FP8_ALL, DEV, scaling="mx")
    assert torch.equal(_fwd(net, inputs), omx)
    ex.enable_fp8(0, DEV)
    assert torch.equal(_fwd(net, inputs), o16), "disable is not the bf16 result"
    # the ROW form of the C call on the same handle is the old function: per-row bits
    nbytes = L.load().scail_dit_fp8_weight_bytes(ex._h, L.FP8_ALL)
    assert nbytes == L.load().scail_dit_fp8_weight_bytes_scaled(ex._h, L.FP8_ALL, L.FP8_SCALINGS["row"]) > 0
    buf = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    L.call("scail_dit_enable_fp8", ex._h, L.FP8_ALL, buf.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(_fwd(net, inputs), o8)
    # an unknown scaling is refused with a message that names it, and changes nothing
    with pytest.raises(L.ScailHipError, match="unknown scaling 2"):
        L.call("scail_dit_enable_fp8_scaled", ex._h, L.FP8_ALL, 2, buf.data_ptr(), nbytes, None)
    assert L.load().scail_dit_fp8_weight_bytes_scaled(ex._h, L.FP8_ALL, 2) == -1
    assert torch.equal(_fwd(net, inputs), o8)
    ex.enable_fp8(0, DEV)


def test_mx_refuses_sequence_parallel_and_sizes_the_workspace(inputs):
    from scail_amd import lib as L
    lib = L.load()
    net = _mk(CFGD, LAYERS, gemm_precision="fp8", fp8_scaling="mx")
    assert torch.isfinite(_fwd(net, inputs)).all()
    ex = net._executor()
    a = ctypes.c_void_p(1 << 20)
    with pytest.raises(L.ScailHipError, match="fp8 GEMMs are enabled"):
        L.call("scail_dit_block_sp", ex._h, 0, a, a, a, a, a, 2, 16, a, a, 1 << 30, None)
    with pytest.raises(L.ScailHipError, match="fp8 GEMMs are enabled"):
        L.call("scail_dit_step_sp", ex._h, a, a, a, a, 1, a, 1, a, a, a, 2, 2, 16, 16, a, 0, a, 1 << 30, None)
    # workspace: the scale region is rows x Kmax / 32 bytes under MX where it is rows x 4 per row; 448 x 16 and 448 x 4 are both
    # multiples of the 256-byte carving unit, so the queries differ by exactly rows (Kmax / 32 - 4)
    rows, kmax = 2 * LTOK, FF
    assert (rows * (kmax // 32)) % 256 == 0 and (rows * 4) % 256 == 0
    q = lambda: (lib.scail_dit_block_workspace_bytes(ex._h, 2, LTOK), lib.scail_dit_workspace_bytes(ex._h, 2, 2, 16, 16),
                 lib.scail_dit_sample_workspace_bytes(ex._h, 2, 16, 16))
    mx = q()
    ex.enable_fp8(L.FP8_ALL, DEV, scaling="row")
    row = q()
    ex.enable_fp8(0, DEV)
    off = q()
    assert [m - r for m, r in zip(mx, row)] == [rows * (kmax // 32 - 4)] * 3, (mx, row)
    assert [r - o for r, o in zip(row, off)] == [rows * kmax + rows * 4] * 3, (row, off)
    # only the attention projections in fp8: the widest fp8 K is then D
    ex.enable_fp8(L.FP8_GEMMS["qkv"] | L.FP8_GEMMS["o"], DEV, scaling="mx")
    assert lib.scail_dit_block_workspace_bytes(ex._h, 2, LTOK) - off[0] == rows * D + rows * (D // 32)


# ---- accuracy against the goldens, next to per-row scaling ---------------------------------------------------------------------------
def test_mx_one_step_accuracy_vs_row_on_the_golden(golden_dir, capsys):
    """dit_tiny, one step: 1 - cosine against the reference golden under both scalings.  MX is held to 1.25 x the per-row figure (on
    Gaussian data without outliers block scaling has at most 1.043 x the per-row squared GEMM error; the rest is margin for seeds and
    layers) and to the absolute bound tests/test_fp8_gpu.py sets for per-row scaling (cosine >= 0.995 against the golden and bf16)."""
    g = _load(golden_dir, "dit_tiny.npz")
    seed = int(g["seed"])
    x, t, ctx = g["x"].to(DEV), g["t"].to(DEV), g["ctx"].to(DEV)
    kw = _golden_kw(g)
    o16 = _net_golden(O.TINY, seed).forward_f32(x, t, ctx, None, **kw).cpu()
    o = {s: _net_golden(O.TINY, seed, gemm_precision="fp8", fp8_scaling=s).forward_f32(x, t, ctx, None, **kw).cpu() for s in ("row", "mx")}
    d = {s: 1.0 - _cos(o[s], g["out"]) for s in o}
    with capsys.disabled():
        print(f"\none step (dit_tiny), 1 - cosine vs the reference golden: row {d['row']:.3e}, mx {d['mx']:.3e} (ratio {d['mx'] / d['row']:.3f}), "
              f"bf16 {1.0 - _cos(o16, g['out']):.3e}; vs bf16: row {1.0 - _cos(o['row'], o16):.3e}, mx {1.0 - _cos(o['mx'], o16):.3e}")
    assert not torch.equal(o["row"], o["mx"])
    assert _cos(o["mx"], g["out"]) >= 0.995 and _cos(o["mx"], o16) >= 0.995
    assert d["mx"] <= 1.25 * d["row"], (d["mx"], d["row"])


def test_mx_sampler_fifty_steps_vs_row_on_the_golden(golden_dir, capsys):
    """sampler_tiny_50 (config 1, 50 steps, CFG 4): 1 - cosine of the final latent against the reference golden under both scalings; MX
    <= 1.25 x per-row, and the per-row test's absolute bound (cosine >= 0.98)."""
    from scail_amd import sampler as S
    g = _load(golden_dir, "sampler_tiny_50.npz")
    shared = dict(concat_images=torch.zeros(1, *g["x0"].shape[1:], device=DEV), ref_concat=g["ref"].to(DEV),
                  concat_smpl_render=g["pose"].to(DEV), image_clip_features=g["clip"].to(DEV))
    d = {}
    for s in ("row", "mx"):
        net = _net_golden(O.CONFIG1, int(g["seed"]), gemm_precision="fp8", fp8_scaling=s)
        smp = S.RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=50,
                          guider_config={"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": 4}})
        xT = smp.sample_hip(net, g["x0"].to(DEV), dict(crossattn=g["c_ctx"].to(DEV), **shared), dict(crossattn=g["uc_ctx"].to(DEV), **shared))
        assert net._cstep is not None and net._cstep._fp8_buf is not None and net._cstep.fp8_scaling == s
        d[s] = 1.0 - _cos(xT.cpu(), g["xT"])
    with capsys.disabled():
        print(f"\n50-step sampler (config 1), 1 - cosine of the final latent vs the reference golden: row {d['row']:.3e}, mx {d['mx']:.3e} "
              f"(ratio {d['mx'] / d['row']:.3f})")
    assert 1.0 - d["mx"] >= 0.98
    assert d["mx"] <= 1.25 * d["row"], (d["mx"], d["row"])


# ---- the probe under MX -----------------------------------------------------------------------------------------------------------
def test_probe_under_mx_on_the_planted_network(inputs):
    """The planted network of tests/test_fp8_probe_gpu.py section 4 (layer 1: one MLP channel c* made huge, W2's column c* zero).  Per
    row, entry (1, W2) is exactly 1: the outlier takes every row's scale.  Under MX it costs block c* / 32 alone, so the entry is
    strictly below 1, and it equals an fp64 restatement -- the reference block quantizer on the very activation, the library's MX GEMM,
    sums in fp64 -- within section 3's bound (a row of cols = D squares summed in fp32: cols * 2^-24 relative)."""
    from scail_amd import lib as L, ops
    kw = dict(concat_images=torch.zeros(1, device=DEV), image_clip_features=inputs[5], ref_concat=inputs[3], concat_smpl_render=inputs[4])
    # max |ff| of the control's layer 1 and the planted bias, as section 4 derives them (the per-op path runs the executor's kernels in
    # the executor's order: its MLP buffer holds layer 1's activation when the tap fires)
    ctl16 = _planted()
    seen = []
    ctl16._tap = lambda i, h: seen.append(float(next(iter(ctl16._ws.values()))["ff"].abs().max())) if i == 1 else None
    _fwd(ctl16, inputs)
    ctl16._tap = None
    o16 = _fwd(ctl16, inputs)
    big = 2.0 ** 20 * 2.0 ** math.ceil(math.log2(seen[0]))
    pl16 = _planted(big)
    ff = []
    pl16._tap = lambda i, h: ff.append(next(iter(pl16._ws.values()))["ff"].clone()) if i == 1 else None
    assert torch.equal(_fwd(pl16, inputs), o16), "the bf16 network must not see the planted channel"
    pl16._tap = None
    ff = ff[0].reshape(-1, FF)
    assert ff.shape[0] == 2 * LTOK and bool((ff[:, CSTAR].float() >= big).all())
    tables = {}
    for s in ("row", "mx"):
        net = _planted(big, gemm_precision="fp8", fp8_scaling=s)
        o_fp8 = _fwd(net, inputs)
        ex = net._executor()
        table = ex.fp8_probe_on(2, LTOK, DEV)
        assert torch.equal(_fwd(net, inputs), o16), f"with the probe on ({s}) the network output is not the bf16 bits"
        ex.fp8_probe_off()
        assert torch.equal(_fwd(net, inputs), o_fp8)
        tables[s] = table.cpu()
        if s == "mx":
            w2 = net.prepare()["layers"][1]
    tr, tm = tables["row"][1, W2], tables["mx"][1, W2]
    assert float(tr[0]) == float(tr[1]) > 0.0 and float(tr[2]) == 1.0, "per-row scaling: Y8 == 0, the relative error is exactly 1"
    rel_mx = math.sqrt(float(tm[0]) / float(tm[1]))
    print(f"\nplanted (1, w2): row {math.sqrt(float(tr[0]) / float(tr[1])):.4f}, mx {rel_mx:.4f}, worst row mx {math.sqrt(float(tm[2])):.4f}")
    assert 0.0 < rel_mx < 1.0 and float(tm[1]) == float(tr[1]) and float(tm[3]) == 2 * LTOK
    # the fp64 restatement
    y16 = ops.gemm(ff, w2["w2"], w2["b2"])
    xq, xe = quant_mxfp8_rows_ref(ff.cpu())
    wq, we = quant_mxfp8_rows_ref(w2["w2"].cpu())
    y8 = ops.gemm_mxfp8(xq.to(DEV), xe.to(DEV), wq.to(DEV), we.to(DEV), w2["b2"])
    a, b = y16.double().cpu(), y8.double().cpu()
    err_r, pow_r = ((b - a) ** 2).sum(1), (a ** 2).sum(1)
    num, den, worst = float(err_r.sum()), float(pow_r.sum()), float((err_r / pow_r).max())
    tol = D * 2.0 ** -24
    got = tm.tolist()
    assert abs(got[0] - num) <= tol * num and abs(got[1] - den) <= tol * den
    assert abs(got[2] - worst) <= (2 * tol + 2.0 ** -23) * worst               # two row sums and one fp32 division
    # the other entries of the MX table are ordinary e4m3 errors
    rel = (tables["mx"][..., 0] / tables["mx"][..., 1]).sqrt()
    assert bool((rel > 0).all()) and float(rel.max()) == pytest.approx(rel_mx) and float(rel[rel < rel_mx].max()) < 0.25


# ---- command line ---------------------------------------------------------------------------------------------------------------------
def test_cli_fp8_scaling_mx_prints_the_table_and_runs(capsys):
    from scail_amd import cli
    cli.main(["--tiny", "--gemm-precision", "fp8", "--fp8-scaling", "mx", "--fp8-max-error", "inf", "--steps", "2"])
    out = capsys.readouterr().out
    assert "fp8 probe (mx scaling): relative error of each fp8 GEMM" in out and "left in bf16: none" in out and out.count("e-0") >= 12
    # the yaml key, through cli.run: the engine's network carries the scaling and the executor runs it
    cfg = copy.deepcopy(cli.TINY)
    cfg["model"]["network_config"]["params"].update(gemm_precision="fp8", fp8_scaling="mx")
    eng = cli.build_engine(cfg)
    v, z, _ = cli.run(cfg, engine=eng, steps=2)
    assert eng.network.fp8_scaling == "mx" and eng.network._cstep.fp8_scaling == "mx" and torch.isfinite(z).all()
    cfg_row = copy.deepcopy(cli.TINY)
    cfg_row["model"]["network_config"]["params"].update(gemm_precision="fp8")
    _, z_row, _ = cli.run(cfg_row, steps=2)
    assert not torch.equal(z, z_row)
