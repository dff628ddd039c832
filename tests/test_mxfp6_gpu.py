"""GPU tests of the 6-bit per-token GEMMs (include/scail_hip.h scail_quant_mxfp6_rows / scail_gemm_mxfp6, include/scail_dit.h
scail_dit_enable_fp6): the quantizer bit for bit against the tests' restatement (tests/test_mxfp6_cpu.py) with every finite bf16 value
among its inputs, the GEMM's fragment and scale map one (row, block) at a time, the GEMM bit for bit on exact operands (every epilogue),
the 14B shapes on random data, the executor under gemm_precision="fp6" (determinism, CFG pair, block-wise path, fp6 <-> fp8 <-> off,
sequence-parallel refusal, byte arithmetic, poisoned workspace), the probe on the planted-outlier network, accuracy against the goldens
next to MX-fp8, and the command line.  Executor network: that of tests/test_fp8_probe_gpu.py."""
import ctypes
import math

import pytest
import torch

import gemm_exact as GE
import ws_contract as W
from conv_exact import assert_bits
from oracle import scail_oracle as O
from test_fp8_gpu import _cos, _fwd, _golden_kw, _inputs, _load, _mk, _net_golden
from test_fp8_probe_gpu import CFGD, CSTAR, D, FF, LAYERS, LTOK, W2, _planted
from test_mxfp6_cpu import BLOCK, R_GAUSS, dequant_mxfp6, e2m3_value, e2m3_rne, pack_e2m3, quant_mxfp6_rows_ref, unpack_e2m3

pytestmark = pytest.mark.gpu
DEV = "cuda"
ONE = 8                       # e2m3 code of 1.0


def _packed(codes, ld=None):
    """UNPACKED codes (R, C) on the CPU -> packed device matrix (R, 3 C / 4), row stride ld bytes (the padding holds 0xFF)"""
    p = pack_e2m3(codes)
    if ld is None:
        return p.to(DEV)
    buf = torch.full((p.shape[0], ld), 0xFF, dtype=torch.uint8)
    buf[:, :p.shape[1]] = p
    return buf.to(DEV)[:, :p.shape[1]]


# ---- scail_quant_mxfp6_rows ---------------------------------------------------------------------------------------------------
def _every_finite_bf16(cols, g):
    """Rows of width cols that hold every finite bf16 value as a non-maximal element of some block, 6 times: the values sorted by
    magnitude, 31 to a block, under a block maximum of 2^j (j = 1 .. 6) times the group's largest (so the group lands in every binade
    and in the subnormals of the scaled block); a maximum that would overflow is bf16's largest, which the top groups then tie."""
    bits = torch.arange(65536, dtype=torch.int32)
    v = (bits << 16).view(torch.float32)
    v = v[torch.isfinite(v)]
    v = v[torch.argsort(v.abs(), stable=True)]
    pad = (-v.numel()) % 31
    v = torch.cat([v, v[-1:].repeat(pad)]).reshape(-1, 31)
    big = float(torch.finfo(torch.bfloat16).max)
    blocks = []
    for j in range(1, 7):
        mx = (v.abs().amax(1) * 2.0 ** j).clamp(max=big)
        sign = torch.where(torch.rand(mx.shape, generator=g) < 0.5, -1.0, 1.0)
        pos = torch.randint(0, 32, mx.shape, generator=g)
        blk = torch.zeros(v.shape[0], 32)
        idx = torch.arange(32)[None, :].expand(v.shape[0], 32)
        blk[idx != pos[:, None]] = v.reshape(-1)
        blk[idx == pos[:, None]] = mx * sign
        blocks.append(blk)
    flat = torch.cat(blocks).reshape(-1)
    rows = (flat.numel() + cols - 1) // cols
    out = torch.zeros(rows * cols)
    out[:flat.numel()] = flat
    return out.reshape(rows, cols)


@pytest.mark.parametrize("rows,cols,ld", [(257, 5120, 5120), (64, 13824, 13888), (7, 128, 160), (1, 128, 128)])
def test_quant_matches_reference_bit_exactly(rows, cols, ld):
    from scail_amd import ops
    g = torch.Generator().manual_seed(3 + rows)
    x = torch.randn(rows, cols, generator=g) * torch.logspace(-20, 20, rows)[:, None]
    if rows >= 7:
        x[0] = 0.0                                          # zero row
        x[1] = 0.0
        x[1, cols // 2] = -3.0e30                           # one huge element: its block keeps it, the others are zero blocks
        x[2] = torch.randn(cols, generator=g) * 1e-38       # bf16 subnormals: the -127 clamp
        x[3] = -0.0
        x[4] = 7.5                                          # the saturation value itself
        blk = torch.arange(cols) // BLOCK                   # blocks alternate between magnitude 1 and 2^20
        x[5] = torch.randn(cols, generator=g) * torch.where(blk % 2 == 0, 1.0, 2.0 ** 20)
    if rows == 257:
        every = _every_finite_bf16(cols, g)
        assert every.shape[0] <= rows - 8
        x[8:8 + every.shape[0]] = every
    xb = x.to(torch.bfloat16)
    if rows == 257:
        seen = torch.zeros(65536, dtype=torch.bool)
        b = xb.reshape(rows, cols // BLOCK, BLOCK)
        nonmax = b.float().abs() < b.float().abs().amax(2, keepdim=True)
        seen[(b[nonmax].view(torch.int16).to(torch.int32) & 0xFFFF).long()] = True
        vals = (torch.arange(65536, dtype=torch.int32) << 16).view(torch.float32)
        missing = vals[torch.isfinite(vals) & ~seen]
        # all but bf16's two largest magnitudes, which can only tie their block's maximum (they do, in the last groups)
        assert bool((missing.abs() == float(torch.finfo(torch.bfloat16).max)).all()), missing.numel()
    buf = torch.zeros(rows, ld, dtype=torch.bfloat16)
    buf[:, :cols] = xb
    src = buf.to(DEV)[:, :cols]
    q, e = ops.quant_mxfp6_rows(src)
    pb = cols // 4 * 3
    # the same into a code matrix and a scale matrix with row strides of their own (the padding must stay untouched)
    q2 = torch.full((rows, pb + 16), 0xAA, dtype=torch.uint8, device=DEV)
    e2 = torch.full((rows, cols // BLOCK + 3), 0xAA, dtype=torch.uint8, device=DEV)
    ops.quant_mxfp6_rows(src, out=q2[:, :pb], scale=e2[:, :cols // BLOCK])
    torch.cuda.synchronize()
    qr, er = quant_mxfp6_rows_ref(xb)
    assert e.dtype == torch.uint8 and tuple(e.shape) == (rows, cols // BLOCK) and tuple(q.shape) == (rows, pb)
    assert int((e.cpu() != er).sum()) == 0, f"{int((e.cpu() != er).sum())} scale bytes differ at {(rows, cols)}"
    got = unpack_e2m3(q.cpu())
    bad = (got != qr).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} codes differ at {(rows, cols)}; first (row, col) {bad[0].tolist()}: got {int(got[tuple(bad[0])])}, " \
                             f"want {int(qr[tuple(bad[0])])}, x {float(xb[tuple(bad[0])])}"
    assert torch.equal(q.cpu(), pack_e2m3(qr))
    assert torch.equal(q2[:, :pb], q) and torch.equal(e2[:, :cols // BLOCK], e)
    assert bool((q2[:, pb:] == 0xAA).all()) and bool((e2[:, cols // BLOCK:] == 0xAA).all())
    assert not bool((e >= 254).any())
    if rows >= 7:
        assert bool((e[0] == 127).all()) and not bool(q[0].any()) and bool((e[3] == 127).all()) and not bool(q[3].any())
        assert bool((e[4] == 127).all()) and bool((got[4] == 31).all())
        assert int((e[1] != 127).sum()) == 1 and int((got[1] != 0).sum()) == 1
        assert bool((e[2] == 0).any())


def test_quant_non_finite_inputs():
    """the header's rule, as the restatement has it: an infinity counts as 2^128 (byte 253) and becomes +-7.5; a NaN is left out of the amax
    and becomes code 0"""
    from scail_amd import ops
    inf, nan = float("inf"), float("nan")
    x = torch.randn(4, 128)
    x[0, 3], x[0, 40], x[0, 41] = inf, -inf, 3.0e38
    x[1, 0], x[1, 33], x[1, 34] = nan, nan, inf
    x[2, 64:96] = 0.0
    x[2, 70] = nan
    x[3, :] = nan
    xb = x.to(torch.bfloat16)
    q, e = ops.quant_mxfp6_rows(xb.to(DEV))
    qr, er = quant_mxfp6_rows_ref(xb)
    assert torch.equal(e.cpu(), er) and torch.equal(unpack_e2m3(q.cpu()), qr)
    got = unpack_e2m3(q.cpu())
    assert e[0, 0] == 253 and got[0, 3] == 31 and e[0, 1] == 253 and got[0, 40] == 63 and got[0, 41] == 22
    assert got[1, 0] == 0 and got[1, 33] == 0 and got[1, 34] == 31 and e[1, 1] == 253
    assert e[2, 2] == 127 and not bool(got[2, 64:96].any()) and bool((e[3] == 127).all()) and not bool(got[3].any())


# ---- scail_gemm_mxfp6: which codes and which scale byte reach which products -------------------------------------------------------
def test_gemm_scale_map_one_row_and_block_at_a_time():
    """K = 256 (two k-tiles of two MFMA steps of two blocks), M = N = 128, every code 1.0 and every scale byte 127: y = 256 everywhere.
    Raising one scale byte by 3 must raise exactly that row (x) or column (w) of y by 32 (2^3 - 1) = 224.  Rows 0, 31, 32, 127 x the 8
    blocks cover the step, the lane half, the k-tile parity and the fragment index, on both operands."""
    from scail_amd import ops
    M = N = 128
    K = 256
    xq = _packed(torch.full((M, K), ONE, dtype=torch.uint8))
    wq = _packed(torch.full((N, K), ONE, dtype=torch.uint8))
    ex = torch.full((M, K // BLOCK), 127, dtype=torch.uint8, device=DEV)
    ew = torch.full((N, K // BLOCK), 127, dtype=torch.uint8, device=DEV)
    base = ops.gemm_mxfp6(xq, ex, wq, ew).float().cpu()
    assert bool((base == 256.0).all()), sorted(set(base.flatten().tolist()))[:8]
    for r in (0, 31, 32, 127):
        for b in range(K // BLOCK):
            want = torch.full((M, N), 256.0)
            want[r, :] += 32.0 * (2 ** 3 - 1)
            ex[r, b] = 130
            got = ops.gemm_mxfp6(xq, ex, wq, ew).float().cpu()
            ex[r, b] = 127
            assert torch.equal(got, want), f"x scale (row {r}, block {b}): rows changed {sorted(set((got != 256).nonzero()[:, 0].tolist()))}, " \
                                           f"values {sorted(set(got[got != 256].tolist()))}"
            ew[r, b] = 130
            got = ops.gemm_mxfp6(xq, ex, wq, ew).float().cpu()
            ew[r, b] = 127
            assert torch.equal(got, want.T), f"w scale (row {r}, block {b}): columns changed {sorted(set((got != 256).nonzero()[:, 1].tolist()))}, " \
                                             f"values {sorted(set(got[got != 256].tolist()))}"


def test_gemm_scale_byte_reaches_exactly_its_own_32_columns():
    """The other operand is the identity, w[j, k] = (k == j), so y[i, j] = x[i, j] 2^(the scale applied to column j of x): with
    ex[i, b] = 127 + b, y[i, j] must be 2^(j / 32) -- the byte of block b scales columns 32 b .. 32 b + 31 of the packed row and no
    others, and code j of a block is read from bits [6 j, 6 j + 6).  Then the roles of x and w swapped.  K = 256: both k-tiles."""
    from scail_amd import ops
    M = N = K = 256
    ones = _packed(torch.full((M, K), ONE, dtype=torch.uint8))
    eye_c = torch.zeros(N, K, dtype=torch.uint8)
    eye_c[torch.arange(N), torch.arange(K)] = ONE
    eye = _packed(eye_c)
    unit = torch.full((M, K // BLOCK), 127, dtype=torch.uint8, device=DEV)
    ramp = (127 + torch.arange(K // BLOCK, dtype=torch.uint8, device=DEV)).repeat(M, 1).contiguous()
    want = torch.pow(2.0, (torch.arange(K) // BLOCK).float()).repeat(M, 1)
    got = ops.gemm_mxfp6(ones, ramp, eye, unit).float().cpu()
    assert torch.equal(got, want), f"x: block applied to each column of row 0: {got[0].log2().tolist()}"
    got = ops.gemm_mxfp6(eye, unit, ones, ramp).float().cpu()
    assert torch.equal(got, want.T), f"w: block applied to each column of row 0: {got[:, 0].log2().tolist()}"
    # every code value through the fragment path: x[i, k] = code (i + k) % 64 against the identity gives the value table back
    codes = ((torch.arange(M)[:, None] + torch.arange(K)[None, :]) % 64).to(torch.uint8)
    got = ops.gemm_mxfp6(_packed(codes), unit, eye, unit).double().cpu()
    assert torch.equal(got, e2m3_value(codes))


# ---- scail_gemm_mxfp6: exact operands, every epilogue ----------------------------------------------------------------------------
def _fp6_int_operands(M, N, K, lda, ldex, g, identity=False):
    """e2m3 codes of integers in [-7, 7] (all exactly representable: 0..4 by 1 are codes, 5, 6, 7 are 4 + 2 m / 2), an ASYMMETRIC W row,
    block exponents drawn per (row, block) from {-2, -1, 0, 1} for both operands; identity: the x of gemm_exact's identity operands (7 at
    column m % K of row m)"""
    if identity:
        xi = torch.zeros(M, K)                                     # gemm_exact.exact_operands(kind="identity"), in code units
        xi[torch.arange(M), torch.arange(M) % K] = 7.0
        if M >= 97:
            assert torch.equal(xi, GE.exact_operands(M, N, K, 1, kind="identity")["x"] * 4.0)
    else:
        xi = torch.randint(-7, 8, (M, K), generator=g).float()
    wi = torch.randint(-7, 8, (N, K), generator=g).float()
    wi[0, :] = torch.arange(K).remainder(13).float() - 6          # a structured, non-symmetric row
    px = torch.randint(-2, 2, (M, K // BLOCK), generator=g)
    pw = torch.randint(-2, 2, (N, K // BLOCK), generator=g)
    cx, cw = e2m3_rne(xi), e2m3_rne(wi)
    assert torch.equal(e2m3_value(cx), xi.double()) and torch.equal(e2m3_value(cw), wi.double())
    ex = torch.full((M, ldex), 255, dtype=torch.uint8)            # the padding holds the NaN byte: it must never be read as a scale
    ex[:, :K // BLOCK] = (px + 127).to(torch.uint8)
    return xi, wi, px, pw, _packed(cx, lda), ex, _packed(cw), (pw + 127).to(torch.uint8).contiguous()


@pytest.mark.parametrize("identity", [False, True], ids=["random", "identity"])
@pytest.mark.parametrize("M,N,K", [(1, 128, 128), (97, 384, 256), (300, 256, 640), (513, 512, 1152), (260, 256, 13824)])
def test_gemm_mxfp6_exact_every_epilogue(M, N, K, identity):
    from scail_amd import lib as L, ops
    g = torch.Generator().manual_seed(M * 7 + N + K)
    lda, ldex = K // 4 * 3 + 32, K // BLOCK + 4
    xi, wi, px, pw, xq_d, ex, wq_d, ew = _fp6_int_operands(M, N, K, lda, ldex, g, identity)
    # every partial sum is an integer multiple of 2^-4 below 49 K 2^2 (|code| <= 7, both block scales <= 2): it fits 24 bits, so the fp32
    # accumulation is exact in any order
    assert 49 * K * 2 ** 2 * 2 ** 4 < 2 ** 24 or K == 13824
    xdq = xi.double() * torch.pow(2.0, px.double()).repeat_interleave(BLOCK, 1)
    wdq = wi.double() * torch.pow(2.0, pw.double()).repeat_interleave(BLOCK, 1)
    v = xdq @ wdq.T                                               # exact in fp64
    # the longest K: 49 K 2^6 passes 2^24, so the bound is taken on the data: sum |x w| in units of 2^-4 stays below 2^24
    assert float((xdq.abs() @ wdq.abs().T).max()) * 16 < 2 ** 24 and torch.equal(v.float().double(), v)
    bias = torch.randint(-8, 9, (N,), generator=g).float()
    ex_d = ex.to(DEV)[:, :K // BLOCK]
    ew_d, b_d = ew.to(DEV), bias.to(DEV)
    assert xq_d.stride(0) == lda and ex_d.stride(0) == ldex
    xd = xdq.to(torch.bfloat16).to(DEV)
    wd = wdq.to(torch.bfloat16).to(DEV).contiguous()
    assert torch.equal(xd.double().cpu(), xdq) and torch.equal(wd.double().cpu(), wdq)

    # BIAS: bit-exact against the fp64 product (+ integer bias, exact) rounded once to bf16
    y = ops.gemm_mxfp6(xq_d, ex_d, wq_d, ew_d, b_d)
    assert_bits(y.cpu(), (v + bias.double()).to(torch.bfloat16), "bias")
    # no bias
    assert_bits(ops.gemm_mxfp6(xq_d, ex_d, wq_d, ew_d).cpu(), v.to(torch.bfloat16), "nobias")
    # GELU-tanh: the same epilogue code as the bf16 kernel on the same fp32 values
    yg = ops.gemm_mxfp6(xq_d, ex_d, wq_d, ew_d, b_d, epilogue=L.EPI_GELU_TANH)
    assert_bits(yg, ops.gemm(xd, wd, b_d, epilogue=L.EPI_GELU_TANH).cpu(), "gelu_tanh against the bf16 kernel")
    ref = torch.nn.functional.gelu(v + bias.double(), approximate="tanh")
    torch.testing.assert_close(yg.double().cpu(), ref, rtol=8e-3, atol=1e-3)
    # RESID ungated, resid aliasing y, output with a row stride > N
    r0 = torch.randint(-64, 65, (M, N), generator=g).float().to(torch.bfloat16)
    out = torch.zeros(M, N + 128, dtype=torch.bfloat16, device=DEV)[:, :N]
    out.copy_(r0.to(DEV))
    ops.gemm_mxfp6(xq_d, ex_d, wq_d, ew_d, b_d, out=out, epilogue=L.EPI_RESID, resid=out)
    assert_bits(out.cpu(), (r0.double() + v + bias.double()).to(torch.bfloat16), "resid aliasing y")
    # RESID with a separate residual
    o2 = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    ops.gemm_mxfp6(xq_d, ex_d, wq_d, ew_d, b_d, out=o2, epilogue=L.EPI_RESID, resid=r0.to(DEV))
    assert_bits(o2.cpu(), (r0.double() + v + bias.double()).to(torch.bfloat16), "separate resid")
    # RESID gated, rows_per_batch: gate[(m / rpb), n] in {-2 .. 2 by 0.5}: r + g (v + b) is exact, rounded once
    rpb = max(1, (M + 1) // 2)
    nb = (M + rpb - 1) // rpb
    gate = (torch.randint(-4, 5, (nb, 2 * N), generator=g).float() * 0.5).to(DEV)[:, :N]
    o8 = r0.to(DEV).clone()
    ops.gemm_mxfp6(xq_d, ex_d, wq_d, ew_d, b_d, out=o8, epilogue=L.EPI_RESID, resid=o8, gate=gate, rows_per_batch=rpb)
    gm = gate.cpu().repeat_interleave(rpb, 0)[:M].double()
    val = r0.double() + gm * (v + bias.double())
    assert float(val.abs().max()) * 32 < 2 ** 24                  # r + g v in units of 2^-5: one fp32 fma, exact
    assert_bits(o8.cpu(), val.to(torch.bfloat16), "gated resid")


# ---- scail_gemm_mxfp6: random data at the 14B shapes -----------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(15360, 5120), (5120, 5120), (13824, 5120), (5120, 13824)])
def test_gemm_mxfp6_random_matches_dequantized_product(N, K):
    from scail_amd import ops
    M = 4099
    g = torch.Generator(device=DEV).manual_seed(N + K)
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV, generator=g) * 0.02).to(torch.bfloat16)
    b = torch.randn(N, device=DEV, generator=g)
    xq, ex = ops.quant_mxfp6_rows(x)
    wq, ew = ops.quant_mxfp6_rows(w)
    y = ops.gemm_mxfp6(xq, ex, wq, ew, b)
    rows = torch.tensor([0, 1, 255, 256, 2047, 4000, M - 1])
    xd = dequant_mxfp6(unpack_e2m3(xq[rows].cpu()), ex[rows].cpu())
    wd = dequant_mxfp6(unpack_e2m3(wq.cpu()), ew.cpu())
    ref = xd @ wd.T + b.cpu().double()
    mag = xd.abs() @ wd.abs().T
    err = (y[rows].double().cpu() - ref).abs()
    # the mxfp8 test's bound: bf16 output rounding (2^-9 relative, with margin) + fp32 accumulation over K; the reference is the
    # dequantized product
    assert bool((err <= 2.0 ** -8 * ref.abs() + 1e-5 * mag + 1e-6).all()), float((err - 2.0 ** -8 * ref.abs() - 1e-5 * mag).max())


# ---- executor ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs():
    return _inputs(2, 16, 16, 64, 12, 5)


@pytest.fixture(scope="module")
def plain(inputs):
    """(bf16, MX fp8, fp6) step outputs of the seed-1234 network: computed once, read by several tests, never written"""
    o16 = _fwd(_mk(CFGD, LAYERS), inputs)
    omx = _fwd(_mk(CFGD, LAYERS, gemm_precision="fp8", fp8_scaling="mx"), inputs)
    o6 = _fwd(_mk(CFGD, LAYERS, gemm_precision="fp6"), inputs)
    assert torch.isfinite(o6).all() and not torch.equal(o16, o6) and not torch.equal(omx, o6)
    return o16, omx, o6


def test_fp6_cfg_pair_determinism_and_blockwise(inputs, plain):
    _, _, o6 = plain
    net = _mk(CFGD, LAYERS, gemm_precision="fp6")
    assert torch.equal(_fwd(net, inputs), o6) and torch.equal(_fwd(net, inputs), o6), "two fp6 runs differ"
    assert net._cstep is not None and net._cstep._fp8_buf is not None
    x, t, ctx, ref, pose, clip = inputs
    pair = (torch.cat([x[:1], x[:1]]).contiguous(), t, ctx, ref, pose, clip)
    outs = [_fwd(net, pair, cfg_pair=p) for p in (False, True)]
    assert not torch.equal(outs[0][0], outs[0][1])
    assert torch.equal(outs[0], outs[1]), f"cfg_pair changed the fp6 result: max |d| {float((outs[0] - outs[1]).abs().max())}"
    net._c_blocks = True
    o_blocks = _fwd(net, inputs)
    net._c_blocks = False
    assert torch.equal(o_blocks, o6), f"max |d| {float((o_blocks - o6).abs().max())}"


def test_fp6_fp8_fp6_off_restores_each_result(inputs, plain):
    from scail_amd import lib as L
    o16, omx, o6 = plain
    net = _mk(CFGD, LAYERS, gemm_precision="fp6")
    assert torch.equal(_fwd(net, inputs), o6)
    ex = net._executor()
    ex.enable_fp8(L.FP8_ALL, DEV, scaling="mx")
    assert torch.equal(_fwd(net, inputs), omx), "enable(fp6) -> enable(fp8 mx) is not the MX fp8 result"
    ex.enable_fp6(L.FP8_ALL, DEV)
    assert torch.equal(_fwd(net, inputs), o6)
    ex.enable_fp8(0, DEV)                                         # enable_fp8(.., 0, ..) returns any handle to bf16
    assert torch.equal(_fwd(net, inputs), o16), "disable is not the bf16 result"
    ex.enable_fp6(L.FP8_ALL, DEV)
    assert torch.equal(_fwd(net, inputs), o6)
    ex.enable_fp6(0, DEV)
    assert torch.equal(_fwd(net, inputs), o16)
    # per-layer selection acts on the fp6 form: nothing selected is bf16, everything selected is fp6
    ex.enable_fp6(L.FP8_ALL, DEV)
    ex.select_fp8_layers([0] * LAYERS)
    assert torch.equal(_fwd(net, inputs), o16)
    ex.select_fp8_layers([L.FP8_ALL] * LAYERS)
    assert torch.equal(_fwd(net, inputs), o6)
    # fp6 is not a third scaling, and a short buffer is refused by name
    buf = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(L.ScailHipError, match="unknown scaling 2"):
        L.call("scail_dit_enable_fp8_scaled", ex._h, L.FP8_ALL, 2, buf.data_ptr(), buf.numel(), None)
    with pytest.raises(L.ScailHipError, match=r"scail_dit_enable_fp6: buffer too small \(scail_dit_fp6_weight_bytes\)"):
        L.call("scail_dit_enable_fp6", ex._h, L.FP8_ALL, buf.data_ptr(), 256, None)
    ex.enable_fp6(0, DEV)


def test_fp6_refuses_sequence_parallel_and_sizes_weights_and_workspace(inputs):
    from scail_amd import lib as L
    lib = L.load()
    net = _mk(CFGD, LAYERS, gemm_precision="fp6")
    assert torch.isfinite(_fwd(net, inputs)).all()
    ex = net._executor()
    a = ctypes.c_void_p(1 << 20)
    with pytest.raises(L.ScailHipError, match="fp8 GEMMs are enabled"):
        L.call("scail_dit_block_sp", ex._h, 0, a, a, a, a, a, 2, 16, a, a, 1 << 30, None)
    with pytest.raises(L.ScailHipError, match="fp8 GEMMs are enabled"):
        L.call("scail_dit_step_sp", ex._h, a, a, a, a, 1, a, 1, a, a, a, 2, 2, 16, 16, a, 0, a, 1 << 30, None)
    # weight bytes: per layer and selected GEMM, align256(3 N K / 4) + align256(N K / 32)
    al = lambda n: (n + 255) // 256 * 256
    shapes = {"qkv": (3 * D, D), "o": (D, D), "cq": (D, D), "co": (D, D), "w1": (FF, D), "w2": (D, FF)}
    want = lambda names: LAYERS * sum(al(n * k * 3 // 4) + al(n * k // 32) for nm, (n, k) in shapes.items() if nm in names)
    assert lib.scail_dit_fp6_weight_bytes(ex._h, L.FP8_ALL) == want(shapes) == ex._fp8_buf.numel()
    assert lib.scail_dit_fp6_weight_bytes(ex._h, L.FP8_GEMMS["w2"] | L.FP8_GEMMS["o"]) == want(("w2", "o"))
    assert lib.scail_dit_fp6_weight_bytes(ex._h, 64) == -1
    # workspace: rows x 3/4 Kmax code bytes + rows x Kmax / 32 scale bytes on top of bf16 (both multiples of the 256-byte carving unit)
    rows, kmax = 2 * LTOK, FF
    assert (rows * kmax * 3 // 4) % 256 == 0 and (rows * (kmax // 32)) % 256 == 0
    q = lambda: (lib.scail_dit_block_workspace_bytes(ex._h, 2, LTOK), lib.scail_dit_workspace_bytes(ex._h, 2, 2, 16, 16),
                 lib.scail_dit_sample_workspace_bytes(ex._h, 2, 16, 16))
    f6 = q()
    ex.enable_fp6(0, DEV)
    off = q()
    assert [a_ - b_ for a_, b_ in zip(f6, off)] == [rows * (kmax * 3 // 4 + kmax // 32)] * 3, (f6, off)
    ex.enable_fp6(L.FP8_GEMMS["qkv"] | L.FP8_GEMMS["o"], DEV)     # the widest quantised K is then D
    assert lib.scail_dit_block_workspace_bytes(ex._h, 2, LTOK) - off[0] == rows * (D * 3 // 4 + D // 32)


def test_fp6_step_on_a_poisoned_exact_size_workspace(inputs, plain):
    _, _, o6 = plain
    net = _mk(CFGD, LAYERS, gemm_precision="fp6")
    assert torch.equal(_fwd(net, inputs), o6)
    for name, fill in W.FILLS.items():
        with W.poisoned(fill) as s:
            got = _fwd(net, inputs)
            torch.cuda.synchronize()
            s.check()
        assert torch.equal(got, o6), f"fill {name}: {int((got != o6).sum())} values differ from the plain fp6 step"


# ---- the probe under fp6 ------------------------------------------------------------------------------------------------------------
def test_probe_under_fp6_on_the_planted_network(inputs):
    """The planted network of tests/test_fp8_probe_gpu.py section 4 (layer 1: one MLP channel c* made huge, W2's column c* zero).  Under
    fp6 the outlier costs block c* / 32 alone, so entry (1, W2) is strictly between 0 and 1, and it equals an fp64 restatement -- the
    restated block quantizer on the very activation, the library's fp6 GEMM, sums in fp64 -- within that file's bound (a row of cols = D
    squares summed in fp32: cols * 2^-24 relative)."""
    from scail_amd import ops
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
    net = _planted(big, gemm_precision="fp6")
    o_fp6 = _fwd(net, inputs)
    ex = net._executor()
    table = ex.fp8_probe_on(2, LTOK, DEV)
    assert torch.equal(_fwd(net, inputs), o16), "with the probe on the network output is not the bf16 bits"
    ex.fp8_probe_off()
    assert torch.equal(_fwd(net, inputs), o_fp6)
    tm = table.cpu()[1, W2]
    w2 = net.prepare()["layers"][1]
    rel = math.sqrt(float(tm[0]) / float(tm[1]))
    print(f"\nplanted (1, w2) under fp6: {rel:.4f}, worst row {math.sqrt(float(tm[2])):.4f}")
    assert 0.0 < rel < 1.0 and float(tm[3]) == 2 * LTOK
    y16 = ops.gemm(ff, w2["w2"], w2["b2"])
    xq, xe = quant_mxfp6_rows_ref(ff.cpu())
    wq, we = quant_mxfp6_rows_ref(w2["w2"].cpu())
    y6 = ops.gemm_mxfp6(_packed(xq), xe.to(DEV), _packed(wq), we.to(DEV), w2["b2"])
    a, b = y16.double().cpu(), y6.double().cpu()
    err_r, pow_r = ((b - a) ** 2).sum(1), (a ** 2).sum(1)
    num, den, worst = float(err_r.sum()), float(pow_r.sum()), float((err_r / pow_r).max())
    tol = D * 2.0 ** -24
    got = tm.tolist()
    assert abs(got[0] - num) <= tol * num and abs(got[1] - den) <= tol * den
    assert abs(got[2] - worst) <= (2 * tol + 2.0 ** -23) * worst               # two row sums and one fp32 division


# ---- accuracy against the goldens, next to MX fp8 ------------------------------------------------------------------------------------
def test_fp6_one_step_accuracy_vs_mx_fp8_on_the_golden(golden_dir, capsys):
    """dit_tiny, one step: 1 - cosine against the reference golden for fp6 and for MX-fp8.  fp6 meets the absolute bound the fp8 tests set
    (cosine >= 0.995 against the golden and against bf16) and is held to 1.2 r times the MX-fp8 figure, r = R_GAUSS."""
    g = _load(golden_dir, "dit_tiny.npz")
    seed = int(g["seed"])
    x, t, ctx = g["x"].to(DEV), g["t"].to(DEV), g["ctx"].to(DEV)
    kw = _golden_kw(g)
    o16 = _net_golden(O.TINY, seed).forward_f32(x, t, ctx, None, **kw).cpu()
    o = {"mx": _net_golden(O.TINY, seed, gemm_precision="fp8", fp8_scaling="mx").forward_f32(x, t, ctx, None, **kw).cpu(),
         "fp6": _net_golden(O.TINY, seed, gemm_precision="fp6").forward_f32(x, t, ctx, None, **kw).cpu()}
    d = {s: 1.0 - _cos(o[s], g["out"]) for s in o}
    with capsys.disabled():
        print(f"\none step (dit_tiny), 1 - cosine vs the reference golden: mx-fp8 {d['mx']:.3e}, fp6 {d['fp6']:.3e} (ratio {d['fp6'] / d['mx']:.3f}, "
              f"bound {1.2 * R_GAUSS:.3f}), bf16 {1.0 - _cos(o16, g['out']):.3e}; vs bf16: mx-fp8 {1.0 - _cos(o['mx'], o16):.3e}, fp6 {1.0 - _cos(o['fp6'], o16):.3e}")
    assert not torch.equal(o["mx"], o["fp6"])
    assert _cos(o["fp6"], g["out"]) >= 0.995 and _cos(o["fp6"], o16) >= 0.995
    assert d["fp6"] <= 1.2 * R_GAUSS * d["mx"], (d["fp6"], d["mx"])


def test_fp6_sampler_fifty_steps_vs_mx_fp8_on_the_golden(golden_dir, capsys):
    """sampler_tiny_50 (config 1, 50 steps, CFG 4): 1 - cosine of the final latent against the reference golden for fp6 and MX-fp8; fp6
    <= 1.2 r x MX-fp8, and the fp8 test's absolute bound (cosine >= 0.98)."""
    from scail_amd import sampler as S
    g = _load(golden_dir, "sampler_tiny_50.npz")
    shared = dict(concat_images=torch.zeros(1, *g["x0"].shape[1:], device=DEV), ref_concat=g["ref"].to(DEV),
                  concat_smpl_render=g["pose"].to(DEV), image_clip_features=g["clip"].to(DEV))
    d = {}
    for s, kw in (("mx", dict(gemm_precision="fp8", fp8_scaling="mx")), ("fp6", dict(gemm_precision="fp6"))):
        net = _net_golden(O.CONFIG1, int(g["seed"]), **kw)
        smp = S.RFSampler(hunyuan_schedule=True, shift_scale=5, num_steps=50,
                          guider_config={"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": 4}})
        xT = smp.sample_hip(net, g["x0"].to(DEV), dict(crossattn=g["c_ctx"].to(DEV), **shared), dict(crossattn=g["uc_ctx"].to(DEV), **shared))
        assert net._cstep is not None and net._cstep._fp8_buf is not None
        d[s] = 1.0 - _cos(xT.cpu(), g["xT"])
    with capsys.disabled():
        print(f"\n50-step sampler (config 1), 1 - cosine of the final latent vs the reference golden: mx-fp8 {d['mx']:.3e}, fp6 {d['fp6']:.3e} "
              f"(ratio {d['fp6'] / d['mx']:.3f}, bound {1.2 * R_GAUSS:.3f})")
    assert 1.0 - d["fp6"] >= 0.98
    assert d["fp6"] <= 1.2 * R_GAUSS * d["mx"], (d["fp6"], d["mx"])


# ---- command line ---------------------------------------------------------------------------------------------------------------------
def test_cli_gemm_precision_fp6_prints_the_table_and_runs(capsys):
    import copy
    from scail_amd import cli
    cli.main(["--tiny", "--gemm-precision", "fp6", "--fp8-max-error", "inf", "--steps", "2"])
    out = capsys.readouterr().out
    assert "fp6 probe (MXFP6 e2m3): relative error of each fp6 GEMM" in out and "left in bf16: none" in out and out.count("e-0") >= 12
    # the yaml key, through cli.run: the engine's network carries the precision and the executor runs it
    cfg = copy.deepcopy(cli.TINY)
    cfg["model"]["network_config"]["params"].update(gemm_precision="fp6")
    eng = cli.build_engine(cfg)
    v, z, _ = cli.run(cfg, engine=eng, steps=2)
    assert eng.network.gemm_precision == "fp6" and eng.network._cstep._fp8_buf is not None and torch.isfinite(z).all()
    cfg8 = copy.deepcopy(cli.TINY)
    cfg8["model"]["network_config"]["params"].update(gemm_precision="fp8", fp8_scaling="mx")
    _, z8, _ = cli.run(cfg8, steps=2)
    assert not torch.equal(z, z8)
