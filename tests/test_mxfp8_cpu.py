"""CPU checks of the MX block scaling of the fp8 per-token GEMMs (include/scail_hip.h scail_quant_mxfp8_rows / scail_gemm_mxfp8,
include/scail_dit.h scail_dit_enable_fp8_scaled): the tests' own reference block quantizer on hand-worked values and its error
property, host-side refusals of the new entry points before any launch, the fp8_scaling option of DiffusionTransformer and of the
command line, and the new symbols."""
import copy
import os

import pytest
import torch

from test_fp8_cpu import _tiny, e4m3_value

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E4M3_MAX = 448.0
BLOCK = 32


def quant_mxfp8_rows_ref(x: torch.Tensor):
    """The numerics scail_quant_mxfp8_rows promises, in torch fp32, per aligned block of 32 columns: amax = max |x|; amax == 0 -> byte
    127, codes 0; otherwise amax = m 2^E with 1 <= m < 2 (frexp gives m / 2 and E + 1), s = E - 8 if m <= 1.75 else E - 7, clamped to
    [-127, 127], byte = s + 127, q = e4m3fn_rne(clamp(x * 2^-s, -448, 448)); 2^-s is built from its fp32 bits (exponent field 127 - s).
    Returns (codes uint8 (R, C), E8M0 bytes uint8 (R, C / 32))."""
    xf = x.float().cpu()
    R, C = xf.shape
    assert C % BLOCK == 0
    b = xf.reshape(R, C // BLOCK, BLOCK)
    amax = b.abs().amax(dim=2)
    zero = amax == 0
    m, e = torch.frexp(torch.where(zero, torch.ones_like(amax), amax))        # amax = m 2^e, 0.5 <= m < 1
    s = (e.to(torch.int32) - 1) - 8 + (m > 0.875).to(torch.int32)
    s = s.clamp(-127, 127)
    s[zero] = 0
    inv = ((127 - s) << 23).to(torch.int32).view(torch.float32)               # 2^-s, exact
    q = (b * inv[:, :, None]).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)
    q[zero] = 0
    return q.reshape(R, C).contiguous(), (s + 127).to(torch.uint8)


def dequant_mxfp8(q: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """codes (R, C) and E8M0 bytes (R, C / 32) -> fp64 values (exact: a 4-bit significand times a power of two)"""
    R, C = q.shape
    v = e4m3_value(q.cpu()).double().reshape(R, C // BLOCK, BLOCK)
    return (v * torch.pow(torch.tensor(2.0, dtype=torch.float64), e.cpu().double() - 127.0)[:, :, None]).reshape(R, C)


def _block(*head, fill=0.0):
    """one block of 32: the given leading values, the rest `fill`"""
    return list(head) + [fill] * (BLOCK - len(head))


def test_reference_block_quantizer_hand_worked_values():
    x = torch.tensor([
        # block 0: amax 448 = 1.75 * 2^8 -> s = 0, byte 127: the row kernel's own hand-worked codes
        _block(448.0, 1.0, -2.0, 0.0625)
        # block 1: amax 480 = 1.875 * 2^8, m > 1.75 -> s = 1, byte 128: 480 / 2 = 240 = 1.875 * 2^7 = 0x77 (the exponent
        # floor(log2 amax) - 8 = 0 would have clipped it to 448)
        + _block(480.0, -480.0, 1.0)
        # block 2: amax 2^24 -> s = 16, byte 143: 2^24 -> 256 = 0x78, and 3 * 2^-16 is below half of e4m3's smallest subnormal: code 0
        + _block(2.0 ** 24, 3.0)
        # block 3: zeros -> byte 127, codes 0;  block 4: negative zeros -> the same
        + _block() + _block(fill=-0.0)
        # block 5: a -0 inside a non-zero block keeps its sign bit
        + _block(-0.0, 3.0)
        # block 6: bf16 subnormals: amax 2^-130 asks for s = -138, clamped to -127 -> byte 0; x * 2^127: 2^-3 = 0x20, 2^-6 = 0x08
        # (bf16's smallest subnormal 2^-133)
        + _block(2.0 ** -130, 2.0 ** -133)
        # block 7: amax 449 (rounds to 448 in bf16, but this reference takes fp32): just above 1.75 * 2^8 -> s = 1
        + _block(449.0)], dtype=torch.float32)
    q, e = quant_mxfp8_rows_ref(x)
    assert e.dtype == torch.uint8 and e.shape == (1, 8) and q.shape == (1, 256)
    assert e[0].tolist() == [127, 128, 143, 127, 127, 120, 0, 128]            # block 5: amax 3 = 1.5 * 2^1 -> s = -7
    qb = q.reshape(8, BLOCK)
    assert qb[0, :4].tolist() == [0x7E, 0x38, 0xC0, 0x18] and not bool(qb[0, 4:].any())
    assert qb[1, :3].tolist() == [0x77, 0xF7, 0x30] and float(e4m3_value(qb[1, :1])) == 240.0      # 1 / 2 = 0.5 = 0x30
    assert qb[2, :2].tolist() == [0x78, 0x00] and float(e4m3_value(qb[2, :1])) == 256.0
    assert not bool(qb[3].any()) and not bool(qb[4].any())
    assert qb[5, 0] == 0x80 and float(e4m3_value(qb[5, 1:2])) == 384.0        # 3 * 2^7 <= 448 < 3 * 2^8
    assert qb[6, :2].tolist() == [0x20, 0x08]
    assert float(e4m3_value(qb[7, :1])) == 224.0                              # 449 / 2 = 224.5 -> 224 (ties to even; e4m3 steps of 16 there)


def test_reference_block_quantizer_never_emits_nan_codes_and_keeps_the_error_bound():
    g = torch.Generator().manual_seed(0)
    xr = torch.randn(64, 512, generator=g) * torch.logspace(-30, 30, 64)[:, None]
    q, e = quant_mxfp8_rows_ref(xr)
    assert not bool(((q & 0x7F) == 0x7F).any()), "a NaN code (0x7f / 0xff)"
    assert not bool((e == 255).any()), "the E8M0 NaN byte"
    # every block's largest scaled magnitude lands in (224, 448]: the smallest exponent that does not clip
    R, C = xr.shape
    top = (xr.reshape(R, C // BLOCK, BLOCK).abs().amax(2).double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), 127.0 - e.double()))
    assert bool((top <= 448.0).all()) and bool((top > 224.0).all())
    # dequantized error per block <= 2^-4 of the block's amax: an e4m3 normal is off by at most 2^-4 of itself (3 mantissa bits), a
    # subnormal by at most 2^-10 2^s < 2^-17 amax.  (Holds wherever the clamp of s to -127 does not bind: |x| > 2^-126 here.)
    err = (dequant_mxfp8(q, e) - xr.double()).abs().reshape(R, C // BLOCK, BLOCK).amax(2)
    amax = xr.double().abs().reshape(R, C // BLOCK, BLOCK).amax(2)
    assert bool((err <= 2.0 ** -4 * amax).all()), float((err / amax).max())
    # and the same on bf16 input, which is what the kernel reads
    xb = xr.to(torch.bfloat16)
    qb, eb = quant_mxfp8_rows_ref(xb)
    errb = (dequant_mxfp8(qb, eb) - xb.double()).abs().reshape(R, C // BLOCK, BLOCK).amax(2)
    assert bool((errb <= 2.0 ** -4 * xb.double().abs().reshape(R, C // BLOCK, BLOCK).amax(2)).all())


def test_planted_outlier_costs_its_own_block_only():
    """what the GPU test of the same name relies on: K = 256, entries in {1, 2, 3}, column 137 = 2^24 -> block 4 (columns 128 .. 159)
    keeps the outlier as 256 * 2^16 and flushes its 31 neighbours; every other block is exact"""
    g = torch.Generator().manual_seed(5)
    x = torch.randint(1, 4, (16, 256), generator=g).float()
    x[:, 137] = 2.0 ** 24
    q, e = quant_mxfp8_rows_ref(x.to(torch.bfloat16))
    want = x.clone().double()
    want[:, 128:160] = 0.0
    want[:, 137] = 2.0 ** 24
    assert torch.equal(dequant_mxfp8(q, e), want)
    assert e[:, 4].eq(143).all() and e[:, :4].eq(120).all()                   # amax 3 = 1.5 * 2^1 -> s = -7


def test_mxfp8_entry_points_refuse_bad_arguments_without_gpu():
    from scail_amd import lib as L
    lib = L.load()
    a = 1 << 20                 # a 256-byte aligned non-null address: the checks fire before anything is dereferenced
    # scail_gemm_mxfp8(x, lda, ex, ldex, w, ew, bias, y, ldc, M, N, K, epilogue, resid, ldr, gate, gate_stride, rows_per_batch, stream)
    args = lambda M, N, K, lda, ldex=None: (a, lda, a, K // 32 if ldex is None else ldex, a, a, None, a, N, M, N, K, L.EPI_BIAS,
                                            None, 0, None, 0, 0, None)
    with pytest.raises(L.ScailHipError, match="K must be a positive multiple of 128"):
        L.call("scail_gemm_mxfp8", *args(16, 128, 72, 80))
    with pytest.raises(L.ScailHipError, match="N must be a positive multiple of 128"):
        L.call("scail_gemm_mxfp8", *args(16, 136, 128, 128))
    with pytest.raises(L.ScailHipError, match="M must be >= 1"):
        L.call("scail_gemm_mxfp8", *args(0, 128, 128, 128))
    with pytest.raises(L.ScailHipError, match="lda must be >= K and a multiple of 16"):
        L.call("scail_gemm_mxfp8", *args(16, 128, 128, 136))
    with pytest.raises(L.ScailHipError, match="ldex must be >= K / 32 and a multiple of 4"):
        L.call("scail_gemm_mxfp8", *args(16, 128, 256, 256, ldex=4))
    with pytest.raises(L.ScailHipError, match="ldex must be >= K / 32 and a multiple of 4"):
        L.call("scail_gemm_mxfp8", *args(16, 128, 128, 128, ldex=6))
    for k in (0, 2, 4, 5, 7):                                                 # x, ex, w, ew, y
        bad = list(args(16, 128, 128, 128))
        bad[k] = None
        with pytest.raises(L.ScailHipError, match="null pointer"):
            L.call("scail_gemm_mxfp8", *bad)
    for k, off in ((0, 8), (2, 2), (4, 8), (5, 2), (6, a + 4), (7, 4)):       # x, ex, w, ew, bias, y
        bad = list(args(16, 128, 128, 128))
        bad[k] = (bad[k] or 0) + off
        with pytest.raises(L.ScailHipError, match="pointer alignment"):
            L.call("scail_gemm_mxfp8", *bad)
    with pytest.raises(L.ScailHipError, match="epilogue must be"):
        L.call("scail_gemm_mxfp8", *args(16, 128, 128, 128)[:12], L.EPI_GELU_ERF, None, 0, None, 0, 0, None)
    with pytest.raises(L.ScailHipError, match="RESID epilogue needs resid"):
        L.call("scail_gemm_mxfp8", *args(16, 128, 128, 128)[:12], L.EPI_RESID, None, 0, None, 0, 0, None)
    with pytest.raises(L.ScailHipError, match="gate needs rows_per_batch > 0"):
        L.call("scail_gemm_mxfp8", *args(16, 128, 128, 128)[:12], L.EPI_RESID, a, 128, a, 128, 0, None)
    # scail_quant_mxfp8_rows(x, ldx, q, ldq, e, lde, rows, cols, stream)
    for k in (0, 2, 4):
        bad = [a, 64, a, 64, a, 2, 4, 64, None]
        bad[k] = None
        with pytest.raises(L.ScailHipError, match="null pointer"):
            L.call("scail_quant_mxfp8_rows", *bad)
    with pytest.raises(L.ScailHipError, match="multiple of 32"):
        L.call("scail_quant_mxfp8_rows", a, 64, a, 64, a, 2, 4, 40, None)     # a multiple of 8 is not enough here
    with pytest.raises(L.ScailHipError, match="multiple of 32"):
        L.call("scail_quant_mxfp8_rows", a, 64, a, 64, a, 2, 4, 0, None)
    with pytest.raises(L.ScailHipError, match="ldx / ldq must be"):
        L.call("scail_quant_mxfp8_rows", a, 32, a, 64, a, 2, 4, 64, None)
    with pytest.raises(L.ScailHipError, match="ldx / ldq must be"):
        L.call("scail_quant_mxfp8_rows", a, 64, a, 68, a, 2, 4, 64, None)
    with pytest.raises(L.ScailHipError, match="lde must be >= cols / 32"):
        L.call("scail_quant_mxfp8_rows", a, 64, a, 64, a, 1, 4, 64, None)
    with pytest.raises(L.ScailHipError, match="pointer alignment"):
        L.call("scail_quant_mxfp8_rows", a + 8, 64, a, 64, a, 2, 4, 64, None)
    with pytest.raises(L.ScailHipError, match="pointer alignment"):
        L.call("scail_quant_mxfp8_rows", a, 64, a + 4, 64, a, 2, 4, 64, None)
    L.call("scail_quant_mxfp8_rows", a, 64, a, 64, a + 1, 2, 0, 64, None)     # no rows: accepted, launches nothing; e needs no alignment
    # executor: an unknown scaling is named, a null handle and an unknown mask bit are refused; the ROW forms are the old functions
    with pytest.raises(L.ScailHipError, match="unknown scaling 7"):
        L.call("scail_dit_enable_fp8_scaled", None, L.FP8_ALL, 7, a, 1 << 30, None)
    with pytest.raises(L.ScailHipError, match="null handle"):
        L.call("scail_dit_enable_fp8_scaled", None, L.FP8_ALL, L.FP8_SCALINGS["mx"], a, 1 << 30, None)
    assert lib.scail_dit_fp8_weight_bytes_scaled(None, 1, 1) == -1
    assert L.FP8_SCALINGS == {"row": 0, "mx": 1}


def test_fp8_scaling_option_of_the_network():
    net = _tiny()
    assert (net.gemm_precision, net.fp8_scaling) == ("bf16", "row")
    assert _tiny(gemm_precision="fp8").fp8_scaling == "row"
    assert _tiny(gemm_precision="fp8", fp8_scaling="mx").fp8_scaling == "mx"
    assert _tiny(fp8_scaling="row").fp8_scaling == "row"                      # the default, spelled out
    with pytest.raises(ValueError, match="needs gemm_precision='fp8'"):
        _tiny(fp8_scaling="mx")
    for bad in ("block", "MX", None, 1):
        with pytest.raises(ValueError, match="fp8_scaling must be one of"):
            _tiny(gemm_precision="fp8", fp8_scaling=bad)
    # the yaml route: network_config.params reach the constructor unchanged
    from scail_amd.config import instantiate_from_config
    net = instantiate_from_config({"target": "dit_video_crossattn_sc_xc.DiffusionTransformer", "params": dict(
        transformer_args=dict(model_parallel_size=1), hidden_size=128, num_layers=1, num_attention_heads=1, text_dim=64,
        time_embed_dim=128, time_freq_dim=256, inner_hidden_size=256, share_adaln=True, use_i2v_clip=True, device="cpu",
        gemm_precision="fp8", fp8_scaling="mx")})
    assert net.fp8_scaling == "mx" and net.fp8_mask == 63


def test_cli_fp8_scaling_option():
    from scail_amd import cli
    assert "--fp8-scaling" in cli.build_parser().format_help()
    for argv in (["--tiny", "--fp8-scaling", "mx"],                           # mx without fp8 GEMMs
                 ["--tiny", "--gemm-precision", "bf16", "--fp8-scaling", "mx"],
                 ["--tiny", "--gemm-precision", "fp8", "--fp8-scaling", "block"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv
    assert cli.fp8_scaling_arg(None, "bf16") is None and cli.fp8_scaling_arg("row", "bf16") == "row"
    assert cli.fp8_scaling_arg("mx", "fp8") == "mx"
    with pytest.raises(ValueError, match="needs --gemm-precision fp8"):
        cli.fp8_scaling_arg("mx", "bf16")
    with pytest.raises(ValueError, match="must be one of"):
        cli.fp8_scaling_arg("block", "fp8")
    # the table's heading names the scaling that was probed; a result without the key is the per-row one
    cal = dict(rel_err=torch.zeros(1, 6), masks=[3], enabled=3)
    assert cli.format_fp8_table(cal, 0.5).splitlines()[0].startswith("fp8 probe (row scaling)")
    assert cli.format_fp8_table(dict(cal, scaling="mx"), 0.5).splitlines()[0].startswith("fp8 probe (mx scaling)")
    assert copy.deepcopy(cli.TINY)["model"]["network_config"]["params"].get("fp8_scaling") is None      # the default config is untouched


def test_new_symbols_are_declared_exported_and_bound():
    from scail_amd import lib as L, ops
    lib = L.load()
    assert lib.scail_abi_version() == L.ABI_VERSION == 8
    hip = open(os.path.join(ROOT, "include", "scail_hip.h")).read()
    dit = open(os.path.join(ROOT, "include", "scail_dit.h")).read()
    for name, header in (("scail_quant_mxfp8_rows", hip), ("scail_gemm_mxfp8", hip), ("scail_dit_fp8_weight_bytes_scaled", dit),
                         ("scail_dit_enable_fp8_scaled", dit)):
        assert name in L.SIGNATURES and getattr(lib, name).argtypes == L.SIGNATURES[name]
        assert f" {name}(" in header, f"{name} is not declared"
    assert lib.scail_dit_fp8_weight_bytes_scaled.restype is L._i64
    assert "#define SCAIL_DIT_FP8_SCALE_ROW 0" in dit and "#define SCAIL_DIT_FP8_SCALE_MX 1" in dit
    assert callable(ops.quant_mxfp8_rows) and callable(ops.gemm_mxfp8)
