"""CPU checks of the 6-bit per-token GEMMs (include/scail_hip.h scail_quant_mxfp6_rows / scail_gemm_mxfp6, include/scail_dit.h
scail_dit_enable_fp6 / scail_dit_fp6_weight_bytes): the tests' restatement of the numerics (quantise, pack, unpack, dequantise to fp64;
the only statement beside the header) on hand-worked blocks, host-side refusals of the new entry points before any launch, the
gemm_precision="fp6" option of DiffusionTransformer, the yaml and the command line, and the new symbols.  (The weight-byte and workspace
arithmetic needs an executor handle, which loads the generated kernels: tests/test_mxfp6_gpu.py holds it.)"""
import copy
import os

import pytest
import torch

from test_fp8_cpu import _tiny

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 32
E2M3_MAX = 7.5
# the Gaussian squared-error ratio MX-e2m3 / MX-e4m3 printed by tools/mxfp6_error_cpu.py (profiles/fp6_error_cpu.log): the figure r that
# tests/test_mxfp6_gpu.py holds the network-level accuracy to
R_GAUSS = 1.128
# magnitude of code & 31: exp 0 subnormal man / 8; else (1 + man / 8) 2^(exp - 1)
E2M3_MAG = torch.tensor([m / 8.0 for m in range(8)] + [(1.0 + m / 8.0) * 2.0 ** (e - 1) for e in (1, 2, 3) for m in range(8)], dtype=torch.float64)


def e2m3_value(code: torch.Tensor) -> torch.Tensor:
    """6-bit codes (uint8, sign << 5 | exp << 3 | man) -> fp64 values"""
    c = code.to(torch.int64)
    assert bool((c < 64).all())
    return E2M3_MAG[c & 31] * torch.where((c & 32) != 0, -1.0, 1.0).double()


def e2m3_rne(v: torch.Tensor) -> torch.Tensor:
    """fp32 / fp64 values in [-7.5, 7.5] -> nearest e2m3 code, ties to the even code; the sign bit of v is kept (-0 too)"""
    a = v.double().abs()
    lo = (torch.searchsorted(E2M3_MAG, a.contiguous(), right=True) - 1).clamp(0, 31)
    hi = (lo + 1).clamp(max=31)
    dl, dh = a - E2M3_MAG[lo], E2M3_MAG[hi] - a
    up = (dh < dl) | ((dh == dl) & (hi % 2 == 0) & (hi != lo))
    mag = torch.where(up, hi, lo)
    return (mag | (torch.signbit(v).to(torch.int64) << 5)).to(torch.uint8)


def quant_mxfp6_rows_ref(x: torch.Tensor):
    """The numerics scail_quant_mxfp6_rows promises, per aligned block of 32 columns: amax = max |x| over the non-NaN elements; amax == 0
    -> byte 127, codes 0; otherwise amax = m 2^E with 1 <= m < 2 (frexp gives m / 2 and E + 1; an infinity counts as 2^128), s = E - 2 if
    m <= 1.875 else E - 1, clamped to >= -127, byte = s + 127, q = e2m3_rne(clamp(x * 2^-s, -7.5, 7.5)), NaN -> code 0.  Returns (codes
    uint8 (R, C), one code per byte, UNPACKED; E8M0 bytes uint8 (R, C / 32))."""
    xf = x.float().cpu()
    R, C = xf.shape
    assert C % BLOCK == 0
    b = xf.reshape(R, C // BLOCK, BLOCK)
    nan = torch.isnan(b)
    amax = torch.where(nan, torch.zeros_like(b), b.abs()).amax(dim=2)
    zero = amax == 0
    inf = torch.isinf(amax)
    m, e = torch.frexp(torch.where(zero | inf, torch.ones_like(amax), amax))      # amax = m 2^e, 0.5 <= m < 1
    s = (e.to(torch.int32) - 1) - 2 + (m > 0.9375).to(torch.int32)
    s = torch.where(inf, torch.full_like(s, 126), s).clamp(min=-127)
    s[zero] = 0
    # x 2^-s in fp64 is exact (and equals the fp32 product: a power of two, no overflow past the clamp)
    v = (b.double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), -s.double())[:, :, None]).clamp(-E2M3_MAX, E2M3_MAX)
    v = torch.where(nan, torch.zeros_like(v), v)
    q = e2m3_rne(v)
    q[zero] = 0
    return q.reshape(R, C).contiguous(), (s + 127).to(torch.uint8)


def pack_e2m3(q: torch.Tensor) -> torch.Tensor:
    """codes (R, C), one per byte -> packed (R, 3 C / 4): code j of a block in bits [6 j, 6 j + 6) of the block's little-endian 192-bit
    string.  4 codes are 24 bits = 3 whole bytes, so the string is built 4 codes at a time."""
    R, C = q.shape
    c = q.to(torch.int64).reshape(R, C // 4, 4)
    w = c[..., 0] | c[..., 1] << 6 | c[..., 2] << 12 | c[..., 3] << 18
    return torch.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255], dim=-1).to(torch.uint8).reshape(R, C // 4 * 3).contiguous()


def unpack_e2m3(p: torch.Tensor) -> torch.Tensor:
    """packed (R, 3 C / 4) -> codes (R, C), one per byte"""
    R, Bn = p.shape
    b = p.to(torch.int64).reshape(R, Bn // 3, 3)
    w = b[..., 0] | b[..., 1] << 8 | b[..., 2] << 16
    return torch.stack([(w >> (6 * j)) & 63 for j in range(4)], dim=-1).to(torch.uint8).reshape(R, Bn // 3 * 4).contiguous()


def dequant_mxfp6(q: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """UNPACKED codes (R, C) and E8M0 bytes (R, C / 32) -> fp64 values (exact: a 4-bit significand times a power of two)"""
    R, C = q.shape
    v = e2m3_value(q.cpu()).reshape(R, C // BLOCK, BLOCK)
    return (v * torch.pow(torch.tensor(2.0, dtype=torch.float64), e.cpu().double() - 127.0)[:, :, None]).reshape(R, C)


def _block(*head, fill=0.0):
    return list(head) + [fill] * (BLOCK - len(head))


def test_all_64_codes_round_trip_and_the_value_table():
    codes = torch.arange(64, dtype=torch.uint8)
    v = e2m3_value(codes)
    assert v[:8].tolist() == [0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875]                 # subnormals
    assert v[8:16].tolist() == [1.0 + m / 8 for m in range(8)] and v[16:24].tolist() == [2.0 + m / 4 for m in range(8)]
    assert v[24:32].tolist() == [4.0 + m / 2 for m in range(8)] and float(v[31]) == 7.5
    assert torch.equal(v[32:], -v[:32]) and bool(torch.signbit(v[32]))
    assert torch.equal(e2m3_rne(v), codes)                                                       # every code is its own nearest
    # packing: 64 codes = 2 blocks = 48 bytes; the hand-packed first bytes; unpack inverts pack
    p = pack_e2m3(codes[None])
    assert p.shape == (1, 48) and p[0, :3].tolist() == [0 | (1 << 6) & 255, (1 >> 2) | (2 << 4) & 255, (2 >> 4) | (3 << 2)]
    assert torch.equal(unpack_e2m3(p), codes[None])
    # element j of a block sits in bits [6 j, 6 j + 6) of the 192-bit little-endian string
    blk = int.from_bytes(bytes(p[0, 24:48].tolist()), "little")
    assert [(blk >> (6 * j)) & 63 for j in range(32)] == list(range(32, 64))


def test_rne_ties_in_every_binade_and_in_the_subnormals():
    # midpoints go to the even code: subnormals (step 1/8), [1, 2) (1/8), [2, 4) (1/4), [4, 7.5] (1/2), and across the binade borders
    ties = [(0.0625, 0), (0.1875, 2), (0.3125, 2), (0.9375, 8), (1.0625, 8), (1.1875, 10), (1.9375, 16), (2.125, 16), (2.375, 18),
            (3.875, 24), (4.25, 24), (4.75, 26), (7.25, 30)]
    for v, code in ties:
        assert e2m3_rne(torch.tensor([v, -v])).tolist() == [code, code | 32], v
    # just off the midpoint goes to the nearer side
    assert e2m3_rne(torch.tensor([0.0626, 0.0624, 4.2501, 4.2499, 7.4, 7.5])).tolist() == [1, 0, 25, 24, 31, 31]
    assert e2m3_rne(torch.tensor([-0.0, 0.0, -0.01])).tolist() == [32, 0, 32]                    # the sign bit is kept


def test_reference_block_quantizer_hand_worked_values():
    x = torch.tensor([
        # block 0: amax 7.5 = 1.875 * 2^2 -> s = 0, byte 127: codes are the values' own
        _block(7.5, 1.0, -2.0, 0.125, 0.0625, 0.1875)
        # block 1: amax 7.75 = 1.9375 * 2^2, m > 1.875 -> s = 1, byte 128: 3.875 is a tie between 3.75 (23) and 4.0 (24) -> 24
        + _block(7.75, -7.75, 1.0)
        # block 2: amax 7.53125 (just above 1.875 * 4) -> s = 1: 3.765625 -> 3.75 (23); amax just below is block 0's case
        + _block(7.53125)
        # block 3: amax 2^24 -> s = 22, byte 149: 2^24 -> 4.0 (24), 3 * 2^-22 rounds to 0
        + _block(2.0 ** 24, 3.0)
        # block 4: zeros; block 5: negative zeros -> byte 127, codes 0
        + _block() + _block(fill=-0.0)
        # block 6: -0 inside a non-zero block keeps its sign bit; amax 3 = 1.5 * 2^1 -> s = -1, 3 * 2 = 6.0 (28)
        + _block(-0.0, 3.0)
        # block 7: bf16 subnormals: amax 2^-130 asks for s = -132, clamped to -127 -> byte 0; 2^-130 * 2^127 = 0.125 (1), 2^-133 * 2^127 =
        # 2^-6 rounds to 0
        + _block(2.0 ** -130, 2.0 ** -133)
        # block 8: amax 1.0 -> s = -2, byte 125: 1 -> 4.0 (24); 0.3 * 4 = 1.2 -> 1.25 (10); 0.29 * 4 = 1.16 -> 1.125 (9)
        + _block(1.0, 0.3, 0.29)], dtype=torch.float32)
    q, e = quant_mxfp6_rows_ref(x)
    assert e.dtype == torch.uint8 and e.shape == (1, 9) and q.shape == (1, 288)
    assert e[0].tolist() == [127, 128, 128, 149, 127, 127, 126, 0, 125]
    qb = q.reshape(9, BLOCK)
    assert qb[0, :6].tolist() == [31, 8, 48, 1, 0, 2] and not bool(qb[0, 6:].any())            # 0.0625 and 0.1875: ties to even (0, 0.25)
    assert qb[1, :3].tolist() == [24, 56, 4]
    assert qb[2, 0] == 23
    assert qb[3, :2].tolist() == [24, 0]
    assert not bool(qb[4].any()) and not bool(qb[5].any())
    assert qb[6, :2].tolist() == [32, 28] and not bool(qb[6, 2:].any())
    assert qb[7, :2].tolist() == [1, 0]
    assert qb[8, :3].tolist() == [24, 10, 9]
    # pack -> unpack -> dequantise: the values above
    d = dequant_mxfp6(unpack_e2m3(pack_e2m3(q)), e).reshape(9, BLOCK)
    assert d[1, :3].tolist() == [8.0, -8.0, 1.0] and float(d[3, 0]) == 2.0 ** 24 and float(d[7, 0]) == 2.0 ** -130


def test_reference_non_finite_inputs():
    """the header's rule: an infinity counts as 2^128 (byte 253) and becomes +-7.5; a NaN is left out of the amax and becomes code 0"""
    inf, nan = float("inf"), float("nan")
    x = torch.tensor([_block(inf, -inf, 3.0e38, 1.0) + _block(nan, 3.0, -1.0) + _block(nan, 0.0) + _block(nan, inf)], dtype=torch.float32)
    q, e = quant_mxfp6_rows_ref(x)
    qb = q.reshape(4, BLOCK)
    assert e[0].tolist() == [253, 126, 127, 253]
    assert qb[0, :4].tolist() == [31, 63, 22, 0]                        # 3e38 * 2^-126 = 3.526.. -> 3.5 (22); 2^-126 -> 0
    assert qb[1, :3].tolist() == [0, 28, 48] and not bool(qb[2].any()) and qb[3, :2].tolist() == [0, 31]


def test_reference_error_bound_and_scale_choice():
    g = torch.Generator().manual_seed(0)
    xr = (torch.randn(64, 512, generator=g) * torch.logspace(-30, 30, 64)[:, None]).to(torch.bfloat16)
    q, e = quant_mxfp6_rows_ref(xr)
    R, C = xr.shape
    assert bool((q < 64).all()) and not bool((e == 255).any())
    # the smallest exponent that does not clip: every block's largest scaled magnitude lands in (3.75, 7.5]
    top = xr.double().abs().reshape(R, C // BLOCK, BLOCK).amax(2) * torch.pow(torch.tensor(2.0, dtype=torch.float64), 127.0 - e.double())
    assert bool((top <= 7.5).all()) and bool((top > 3.75).all())
    # an element is off by at most half a step: 2^-4 of itself when normal (3 mantissa bits), 2^-4 2^s <= 2^-4 amax / 3.75 when subnormal
    err = (dequant_mxfp6(q, e) - xr.double()).abs().reshape(R, C // BLOCK, BLOCK).amax(2)
    amax = xr.double().abs().reshape(R, C // BLOCK, BLOCK).amax(2)
    assert bool((err <= 2.0 ** -4 * amax).all()), float((err / amax).max())


def test_mxfp6_entry_points_refuse_bad_arguments_without_gpu():
    from scail_amd import lib as L
    lib = L.load()
    a = 1 << 20
    # scail_gemm_mxfp6(x, lda, ex, ldex, w, ew, bias, y, ldc, M, N, K, epilogue, resid, ldr, gate, gate_stride, rows_per_batch, stream)
    args = lambda M, N, K, lda=None, ldex=None: (a, K // 4 * 3 if lda is None else lda, a, K // 32 if ldex is None else ldex, a, a, None, a, N,
                                                 M, N, K, L.EPI_BIAS, None, 0, None, 0, 0, None)
    with pytest.raises(L.ScailHipError, match="K must be a positive multiple of 128"):
        L.call("scail_gemm_mxfp6", *args(16, 128, 64))
    with pytest.raises(L.ScailHipError, match="N must be a positive multiple of 128"):
        L.call("scail_gemm_mxfp6", *args(16, 136, 128))
    with pytest.raises(L.ScailHipError, match="M must be >= 1"):
        L.call("scail_gemm_mxfp6", *args(0, 128, 128))
    with pytest.raises(L.ScailHipError, match=r"lda \(bytes\) must be >= 3 \* K / 4 and a multiple of 16"):
        L.call("scail_gemm_mxfp6", *args(16, 128, 128, lda=80))                 # 96 bytes are needed
    with pytest.raises(L.ScailHipError, match=r"lda \(bytes\) must be >= 3 \* K / 4 and a multiple of 16"):
        L.call("scail_gemm_mxfp6", *args(16, 128, 128, lda=104))
    with pytest.raises(L.ScailHipError, match="ldex must be >= K / 32 and a multiple of 4"):
        L.call("scail_gemm_mxfp6", *args(16, 128, 256, ldex=4))
    for k in (0, 2, 4, 5, 7):                                                   # x, ex, w, ew, y
        bad = list(args(16, 128, 128))
        bad[k] = None
        with pytest.raises(L.ScailHipError, match="null pointer"):
            L.call("scail_gemm_mxfp6", *bad)
    for k, off in ((0, 8), (2, 2), (4, 8), (5, 2), (6, a + 4), (7, 4)):         # x, ex, w, ew, bias, y
        bad = list(args(16, 128, 128))
        bad[k] = (bad[k] or 0) + off
        with pytest.raises(L.ScailHipError, match="pointer alignment"):
            L.call("scail_gemm_mxfp6", *bad)
    with pytest.raises(L.ScailHipError, match="scail_gemm_mxfp6: epilogue must be"):
        L.call("scail_gemm_mxfp6", *args(16, 128, 128)[:12], L.EPI_GELU_ERF, None, 0, None, 0, 0, None)
    with pytest.raises(L.ScailHipError, match="RESID epilogue needs resid"):
        L.call("scail_gemm_mxfp6", *args(16, 128, 128)[:12], L.EPI_RESID, None, 0, None, 0, 0, None)
    with pytest.raises(L.ScailHipError, match="gate needs rows_per_batch > 0"):
        L.call("scail_gemm_mxfp6", *args(16, 128, 128)[:12], L.EPI_RESID, a, 128, a, 128, 0, None)
    # scail_quant_mxfp6_rows(x, ldx, q, ldq_bytes, e, lde, rows, cols, stream)
    for k in (0, 2, 4):
        bad = [a, 64, a, 48, a, 2, 4, 64, None]
        bad[k] = None
        with pytest.raises(L.ScailHipError, match="null pointer"):
            L.call("scail_quant_mxfp6_rows", *bad)
    with pytest.raises(L.ScailHipError, match="multiple of 32"):
        L.call("scail_quant_mxfp6_rows", a, 64, a, 48, a, 2, 4, 40, None)
    with pytest.raises(L.ScailHipError, match="multiple of 32"):
        L.call("scail_quant_mxfp6_rows", a, 64, a, 48, a, 2, 4, 0, None)
    with pytest.raises(L.ScailHipError, match="ldx must be >= cols"):
        L.call("scail_quant_mxfp6_rows", a, 32, a, 48, a, 2, 4, 64, None)
    with pytest.raises(L.ScailHipError, match=r"ldq \(bytes\) must be >= 3 \* cols / 4"):
        L.call("scail_quant_mxfp6_rows", a, 64, a, 44, a, 2, 4, 64, None)       # 48 bytes are needed
    with pytest.raises(L.ScailHipError, match=r"ldq \(bytes\) must be >= 3 \* cols / 4 and a multiple of 4"):
        L.call("scail_quant_mxfp6_rows", a, 64, a, 50, a, 2, 4, 64, None)
    with pytest.raises(L.ScailHipError, match="lde must be >= cols / 32"):
        L.call("scail_quant_mxfp6_rows", a, 64, a, 48, a, 1, 4, 64, None)
    with pytest.raises(L.ScailHipError, match="pointer alignment"):
        L.call("scail_quant_mxfp6_rows", a + 8, 64, a, 48, a, 2, 4, 64, None)
    with pytest.raises(L.ScailHipError, match="pointer alignment"):
        L.call("scail_quant_mxfp6_rows", a, 64, a + 2, 48, a, 2, 4, 64, None)
    L.call("scail_quant_mxfp6_rows", a, 64, a, 48, a + 1, 2, 0, 64, None)       # no rows: accepted, launches nothing
    # executor: a null handle and an unknown mask bit are refused; fp6 is not a third scaling of the fp8 entry
    with pytest.raises(L.ScailHipError, match="scail_dit_enable_fp6: null handle"):
        L.call("scail_dit_enable_fp6", None, L.FP8_ALL, a, 1 << 30, None)
    assert lib.scail_dit_fp6_weight_bytes(None, 1) == -1
    with pytest.raises(L.ScailHipError, match="unknown scaling 2"):
        L.call("scail_dit_enable_fp8_scaled", None, L.FP8_ALL, 2, a, 1 << 30, None)
    assert L.FP8_SCALINGS == {"row": 0, "mx": 1} and L.GEMM_PRECISIONS == ("fp8", "fp6")


def test_gemm_precision_fp6_option_of_the_network_yaml_and_cli():
    from scail_amd import cli, lib as L
    net = _tiny(gemm_precision="fp6", fp8_gemms=["w1", "w2"])
    assert net.gemm_precision == "fp6" and net.fp8_mask == 48
    assert _tiny(gemm_precision="fp6", fp8_gemms="qkv o").fp8_mask == 3
    assert _tiny(gemm_precision="fp6", fp8_layers=[63]).fp8_layer_masks == [63]
    with pytest.raises(ValueError, match="needs gemm_precision='fp8'"):       # fp8_scaling stays an fp8-only option
        _tiny(gemm_precision="fp6", fp8_scaling="mx")
    with pytest.raises(ValueError, match="gemm_precision must be 'bf16', 'fp8' or 'fp6'"):
        _tiny(gemm_precision="fp4")
    with pytest.raises(ValueError, match="fp8_gemms needs gemm_precision='fp8'"):      # the bf16 messages stay word for word
        _tiny(fp8_gemms=["w1"])
    with pytest.raises(NotImplementedError, match="fp6 GEMM w1"):
        from scail_amd.dit import DiffusionTransformer
        DiffusionTransformer(transformer_args=dict(model_parallel_size=1), hidden_size=128, num_layers=1, num_attention_heads=1, text_dim=64,
                             time_embed_dim=128, time_freq_dim=256, inner_hidden_size=192, share_adaln=True, use_i2v_clip=True, device="cpu",
                             gemm_precision="fp6")
    from scail_amd.config import instantiate_from_config
    net = instantiate_from_config({"target": "dit_video_crossattn_sc_xc.DiffusionTransformer", "params": dict(
        transformer_args=dict(model_parallel_size=1), hidden_size=128, num_layers=1, num_attention_heads=1, text_dim=64,
        time_embed_dim=128, time_freq_dim=256, inner_hidden_size=256, share_adaln=True, use_i2v_clip=True, device="cpu",
        gemm_precision="fp6")})
    assert net.gemm_precision == "fp6" and net.fp8_mask == 63
    # command line
    assert "fp6" in cli.build_parser().format_help()
    assert cli.build_parser().parse_args(["--tiny", "--gemm-precision", "fp6"]).gemm_precision == "fp6"
    assert cli.fp8_max_error_arg(0.5, "fp6") == 0.5 and cli.fp8_max_error_arg(float("inf"), "fp6") == float("inf")
    with pytest.raises(ValueError, match="needs --gemm-precision fp8"):
        cli.fp8_max_error_arg(0.5, "bf16")
    with pytest.raises(ValueError, match="needs --gemm-precision fp8"):
        cli.fp8_scaling_arg("mx", "fp6")
    with pytest.raises(SystemExit) as e:
        cli.main(["--tiny", "--gemm-precision", "fp6", "--fp8-scaling", "mx"])
    assert e.value.code == 2
    cal = dict(rel_err=torch.zeros(1, 6), masks=[3], enabled=3)
    head = cli.format_fp8_table(dict(cal, precision="fp6"), 0.5).splitlines()[0]
    assert head.startswith("fp6 probe (MXFP6 e2m3): relative error of each fp6 GEMM")
    assert cli.format_fp8_table(cal, 0.5).splitlines()[0].startswith("fp8 probe (row scaling): relative error of each fp8 GEMM")
    assert copy.deepcopy(cli.TINY)["model"]["network_config"]["params"].get("gemm_precision") is None


def test_the_committed_tool_prints_r():
    """R_GAUSS is the tool's figure, not the kernel's"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("mxfp6_error_cpu", os.path.join(ROOT, "tools", "mxfp6_error_cpu.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert abs(m.gaussian_squared_ratio(3) - R_GAUSS) < 0.01
    assert f"r = {R_GAUSS:.3f}" in open(os.path.join(ROOT, "profiles", "fp6_error_cpu.log")).read()


def test_new_symbols_are_declared_exported_and_bound():
    from scail_amd import cstep, lib as L, ops
    lib = L.load()
    assert lib.scail_abi_version() == L.ABI_VERSION == 8
    hip = open(os.path.join(ROOT, "include", "scail_hip.h")).read()
    dit = open(os.path.join(ROOT, "include", "scail_dit.h")).read()
    for name, header in (("scail_quant_mxfp6_rows", hip), ("scail_gemm_mxfp6", hip), ("scail_dit_fp6_weight_bytes", dit),
                         ("scail_dit_enable_fp6", dit)):
        assert name in L.SIGNATURES and getattr(lib, name).argtypes == L.SIGNATURES[name]
        assert f" {name}(" in header, f"{name} is not declared"
    assert lib.scail_dit_fp6_weight_bytes.restype is L._i64
    assert L.SIGNATURES["scail_gemm_mxfp6"] == L.SIGNATURES["scail_gemm_mxfp8"]
    assert callable(ops.quant_mxfp6_rows) and callable(ops.gemm_mxfp6) and callable(cstep.CStep.enable_fp6)
