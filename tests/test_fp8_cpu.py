"""CPU checks of the fp8 (e4m3) per-token GEMM path (include/scail_hip.h "fp8 per-token GEMMs", include/scail_dit.h
scail_dit_enable_fp8): host-side refusals of the new entry points before any launch, the tests' own reference quantizer on
hand-worked values, and the gemm_precision options of DiffusionTransformer."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E4M3_MAX = 448.0


def quant_fp8_rows_ref(x: torch.Tensor):
    """The numerics scail_quant_fp8_rows promises, in torch fp32: per row amax = max |x|; amax == 0 -> s = 1, q = 0; otherwise
    s = amax / 448, q = e4m3fn_rne(clamp(x * (448 / amax), -448, 448)).  Returns (codes uint8 (R, C), scales fp32 (R,))."""
    xf = x.float().cpu()
    amax = xf.abs().amax(dim=1)
    zero = amax == 0
    safe = torch.where(zero, torch.ones_like(amax), amax)
    r = torch.where(zero, torch.zeros_like(amax), torch.full_like(amax, E4M3_MAX) / safe)
    s = torch.where(zero, torch.ones_like(amax), safe / torch.full_like(amax, E4M3_MAX))
    q = (xf * r[:, None]).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)
    q[zero] = 0
    return q, s


def e4m3_value(codes: torch.Tensor) -> torch.Tensor:
    return codes.view(torch.float8_e4m3fn).float()


def test_reference_quantizer_hand_worked_values():
    # row 0: amax 448 -> r = 1 exactly: 448 stays the largest code (0x7e), 1.0 = 0x38, -2.0 = 0xc0, 0.0625 = 2^-4 = 0x18
    # row 1: amax 2 -> r = 224: 2 -> 448 (saturates at the top code, never NaN), 1/224 * ... the smallest subnormal 2^-9 of e4m3
    #        comes from x = 2^-9 / 224; half of it rounds to zero (ties to even), 3/4 of it rounds up to the subnormal
    # row 2: all zero -> s = 1, q = 0;  row 3: negative zero and zero -> also the zero row
    sub = 2.0 ** -9 / 224.0
    x = torch.tensor([[448.0, 1.0, -2.0, 0.0625],
                      [2.0, sub, 0.5 * sub, 0.75 * sub],
                      [0.0, 0.0, 0.0, 0.0],
                      [-0.0, 0.0, -0.0, 0.0]], dtype=torch.float32)
    q, s = quant_fp8_rows_ref(x)
    assert q[0].tolist() == [0x7E, 0x38, 0xC0, 0x18]
    assert float(s[0]) == 1.0
    assert q[1, 0] == 0x7E and float(e4m3_value(q[1, :1])) == 448.0
    assert q[1, 1] == 0x01 and float(e4m3_value(q[1, 1:2])) == 2.0 ** -9       # smallest subnormal
    assert q[1, 2] == 0x00                                                       # a tie at half of it rounds to even (zero)
    assert q[1, 3] == 0x01
    assert float(s[1]) == float(torch.tensor(2.0 / 448.0, dtype=torch.float32))
    assert q[2].tolist() == [0, 0, 0, 0] and float(s[2]) == 1.0
    assert q[3].tolist() == [0, 0, 0, 0] and float(s[3]) == 1.0
    # negative zero in a non-zero row keeps its sign bit (x * r = -0)
    q2, _ = quant_fp8_rows_ref(torch.tensor([[-0.0, 3.0]]))
    assert q2[0, 0] == 0x80
    # no NaN code (0x7f / 0xff) for any finite input; an input far past amax cannot occur (amax is the row maximum)
    g = torch.Generator().manual_seed(0)
    xr = torch.randn(64, 512, generator=g) * torch.logspace(-30, 30, 64)[:, None]
    qr, sr = quant_fp8_rows_ref(xr)
    assert not bool(((qr & 0x7F) == 0x7F).any())
    deq = e4m3_value(qr) * sr[:, None]
    assert float(((deq - xr).abs() / xr.abs().amax(dim=1, keepdim=True)).max()) <= 2.0 ** -4 + 1e-6   # e4m3: 3 mantissa bits


def test_fp8_entry_points_refuse_bad_arguments_without_gpu():
    from scail_amd import lib as L
    L.load()
    a = 1 << 20                 # a 256-byte aligned non-null address: the checks fire before anything is dereferenced
    args = lambda M, N, K, lda: (a, lda, a, a, a, None, a, N, M, N, K, L.EPI_BIAS, None, 0, None, 0, 0, None)
    with pytest.raises(L.ScailHipError, match="K must be a positive multiple of 128"):
        L.call("scail_gemm_fp8", *args(16, 128, 72, 80))
    with pytest.raises(L.ScailHipError, match="N must be a positive multiple of 128"):
        L.call("scail_gemm_fp8", *args(16, 136, 128, 128))
    with pytest.raises(L.ScailHipError, match="M must be >= 1"):
        L.call("scail_gemm_fp8", *args(0, 128, 128, 128))
    with pytest.raises(L.ScailHipError, match="null pointer"):
        L.call("scail_gemm_fp8", None, 128, a, a, a, None, a, 128, 16, 128, 128, L.EPI_BIAS, None, 0, None, 0, 0, None)
    with pytest.raises(L.ScailHipError, match="null pointer"):
        L.call("scail_gemm_fp8", a, 128, None, a, a, None, a, 128, 16, 128, 128, L.EPI_BIAS, None, 0, None, 0, 0, None)
    with pytest.raises(L.ScailHipError, match="epilogue must be"):
        L.call("scail_gemm_fp8", *args(16, 128, 128, 128)[:11], L.EPI_GELU_ERF, None, 0, None, 0, 0, None)
    with pytest.raises(L.ScailHipError, match="RESID epilogue needs resid"):
        L.call("scail_gemm_fp8", *args(16, 128, 128, 128)[:11], L.EPI_RESID, None, 0, None, 0, 0, None)
    with pytest.raises(L.ScailHipError, match="null pointer"):
        L.call("scail_quant_fp8_rows", None, 64, a, 64, a, 4, 64, None)
    with pytest.raises(L.ScailHipError, match="multiple of 8"):
        L.call("scail_quant_fp8_rows", a, 64, a, 64, a, 4, 60, None)
    # executor: null handle, unknown mask bit
    with pytest.raises(L.ScailHipError, match="null handle"):
        L.call("scail_dit_enable_fp8", None, L.FP8_ALL, a, 1 << 30, None)
    lib = L.load()
    assert lib.scail_dit_fp8_weight_bytes(None, 1) == -1
    assert L.FP8_ALL == sum(L.FP8_GEMMS.values()) == 63


def _tiny(**kw):
    from scail_amd.dit import DiffusionTransformer
    return DiffusionTransformer(transformer_args=dict(model_parallel_size=1), hidden_size=128, num_layers=1, num_attention_heads=1,
                                text_dim=64, time_embed_dim=128, time_freq_dim=256, inner_hidden_size=256, share_adaln=True,
                                use_i2v_clip=True, device="cpu", **kw)


def test_gemm_precision_options_of_the_network():
    from scail_amd import lib as L
    assert (_tiny().gemm_precision, _tiny().fp8_mask) == ("bf16", 0)
    net = _tiny(gemm_precision="fp8")
    assert net.gemm_precision == "fp8" and net.fp8_mask == L.FP8_ALL
    assert _tiny(gemm_precision="fp8", fp8_gemms=["w1", "w2"]).fp8_mask == 48
    assert _tiny(gemm_precision="fp8", fp8_gemms="qkv,o").fp8_mask == 3
    assert _tiny(gemm_precision="fp8", fp8_gemms=5).fp8_mask == 5
    with pytest.raises(ValueError, match="gemm_precision"):
        _tiny(gemm_precision="fp16")
    with pytest.raises(ValueError, match="unknown GEMM"):
        _tiny(gemm_precision="fp8", fp8_gemms=["mlp"])
    with pytest.raises(ValueError, match="needs gemm_precision='fp8'"):
        _tiny(fp8_gemms=["w1"])
    with pytest.raises(ValueError, match="at least one"):
        _tiny(gemm_precision="fp8", fp8_gemms=[])
    with pytest.raises(NotImplementedError, match="multiples of 128"):
        from scail_amd.dit import DiffusionTransformer
        DiffusionTransformer(transformer_args=dict(model_parallel_size=1), hidden_size=128, num_layers=1, num_attention_heads=1,
                             text_dim=64, time_embed_dim=128, time_freq_dim=256, inner_hidden_size=192, share_adaln=True,
                             use_i2v_clip=True, device="cpu", gemm_precision="fp8")
    # the yaml route: network_config.params reach the constructor unchanged
    from scail_amd.config import instantiate_from_config
    net = instantiate_from_config({"target": "dit_video_crossattn_sc_xc.DiffusionTransformer", "params": dict(
        transformer_args=dict(model_parallel_size=1), hidden_size=128, num_layers=1, num_attention_heads=1, text_dim=64,
        time_embed_dim=128, time_freq_dim=256, inner_hidden_size=256, share_adaln=True, use_i2v_clip=True, device="cpu",
        gemm_precision="fp8", fp8_gemms=["qkv"])})
    assert net.fp8_mask == 1


def test_cli_has_gemm_precision():
    out = subprocess.run([sys.executable, "-m", "scail_amd.cli", "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0 and "--gemm-precision" in out.stdout and "fp8" in out.stdout
