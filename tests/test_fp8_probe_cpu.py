"""CPU checks of the per-layer fp8 selection and the GEMM error probe: the pure selection function, the constructor option, the CLI's
argument error, and the host-side validation of the new entry points (all before any launch, so no GPU is needed)."""
import copy
import math

import pytest
import torch

INF, NAN = float("inf"), float("nan")


def _tiny(**kw):
    from scail_amd.dit import DiffusionTransformer
    return DiffusionTransformer(transformer_args=dict(model_parallel_size=1), hidden_size=128, num_layers=2, num_attention_heads=1,
                                text_dim=64, time_embed_dim=128, time_freq_dim=256, inner_hidden_size=256, share_adaln=True,
                                use_i2v_clip=True, device="cpu", **kw)


def test_choose_fp8_layers_on_hand_made_tables():
    from scail_amd import lib as L
    from scail_amd.dit import choose_fp8_layers, fp8_rel_err
    #        qkv   o            cq    co   w1           w2
    rel = [[0.5, math.nextafter(0.5, 1.0), NAN, INF, 0.0, 0.49999],
           [0.0, 0.0, 0.0, 0.0, 0.0, 1.0],
           [-INF, 1e-300, 0.5, 0.5, 0.5, 0.5]]
    # the edge itself is kept, the next float above it is not; NaN and +-inf never are
    assert choose_fp8_layers(rel, 0.5, L.FP8_ALL) == [1 | 16 | 32, 31, 2 | 4 | 8 | 16 | 32]
    assert choose_fp8_layers(torch.tensor(rel, dtype=torch.float64), 0.5, L.FP8_ALL) == [49, 31, 62]
    # a bit that is not enabled is never selected, however small its value
    assert choose_fp8_layers(rel, 0.5, L.FP8_GEMMS["qkv"] | L.FP8_GEMMS["w2"]) == [33, 1, 32]
    assert choose_fp8_layers(rel, 0.5, 0) == [0, 0, 0]
    # threshold 0 keeps exact zeros only; inf keeps every finite value and still no inf / NaN
    assert choose_fp8_layers(rel, 0.0, L.FP8_ALL) == [16, 31, 0]
    assert choose_fp8_layers(rel, INF, L.FP8_ALL) == [1 | 2 | 16 | 32, 63, 62]
    for bad in (NAN, -1.0):
        with pytest.raises(ValueError, match="max_rel_err"):
            choose_fp8_layers(rel, bad, L.FP8_ALL)
    with pytest.raises(ValueError, match="enabled_mask"):
        choose_fp8_layers(rel, 0.5, 64)
    with pytest.raises(ValueError, match=r"\(layers, 6\)"):
        choose_fp8_layers([[0.0] * 5], 0.5, 63)
    # the raw table: sqrt(num / den); den == 0 counts as 0 with num == 0 and as +inf otherwise
    table = torch.zeros(1, 6, 4, dtype=torch.float64)
    table[0, 0] = torch.tensor([1.0, 4.0, 0.25, 7.0])        # 0.5
    table[0, 1] = torch.tensor([0.0, 0.0, 0.0, 7.0])         # 0 / 0 -> 0
    table[0, 2] = torch.tensor([1.0, 0.0, INF, 7.0])         # x / 0 -> inf
    table[0, 3] = torch.tensor([NAN, 1.0, NAN, 7.0])
    table[0, 4] = torch.tensor([9.0, 1.0, 16.0, 7.0])        # 3
    rel_t, worst = fp8_rel_err(table)
    assert rel_t[0].tolist()[:3] == [0.5, 0.0, INF] and math.isnan(rel_t[0, 3]) and rel_t[0, 4] == 3.0 and rel_t[0, 5] == 0.0
    assert worst[0, 0] == 0.5 and worst[0, 4] == 4.0 and worst[0, 2] == INF
    assert choose_fp8_layers(table, 0.5, L.FP8_ALL) == [1 | 2 | 32]
    assert choose_fp8_layers(table, 3.0, L.FP8_ALL) == [1 | 2 | 16 | 32]


def test_fp8_layers_option_validation():
    from scail_amd import lib as L
    assert _tiny().fp8_layer_masks is None and _tiny(gemm_precision="fp8").fp8_layer_masks is None
    net = _tiny(gemm_precision="fp8", fp8_layers=[63, 0])
    assert net.fp8_mask == L.FP8_ALL and net.fp8_layer_masks == [63, 0]
    assert _tiny(gemm_precision="fp8", fp8_layers=[["qkv", "w2"], "o, cq"]).fp8_layer_masks == [33, 6]
    assert _tiny(gemm_precision="fp8", fp8_gemms=["w1", "w2"], fp8_layers=[[], 48]).fp8_layer_masks == [0, 48]
    with pytest.raises(ValueError, match="needs gemm_precision='fp8'"):
        _tiny(fp8_layers=[0, 0])
    with pytest.raises(ValueError, match=r"one entry per layer \(2\), got 3"):
        _tiny(gemm_precision="fp8", fp8_layers=[1, 1, 1])
    with pytest.raises(ValueError, match="one entry per layer"):
        _tiny(gemm_precision="fp8", fp8_layers="qkv")
    with pytest.raises(ValueError, match=r"fp8_layers\[1\]: unknown GEMM"):
        _tiny(gemm_precision="fp8", fp8_layers=[["qkv"], ["mlp"]])
    with pytest.raises(ValueError, match=r"fp8_layers\[0\]: mask must be 0\.\.63"):
        _tiny(gemm_precision="fp8", fp8_layers=[64, 0])
    with pytest.raises(ValueError, match=r"fp8_layers\[1\] selects \['w2'\]"):
        _tiny(gemm_precision="fp8", fp8_gemms=["qkv", "w1"], fp8_layers=[17, 33])
    with pytest.raises(ValueError, match=r"fp8_layers\[0\]: expected a mask or GEMM names"):
        _tiny(gemm_precision="fp8", fp8_layers=[True, 0])
    # the same validation after construction; None drops the selection
    net.select_fp8_layers([1, 2])
    assert net.fp8_layer_masks == [1, 2]
    with pytest.raises(ValueError, match="one entry per layer"):
        net.select_fp8_layers([1])
    net.select_fp8_layers(None)
    assert net.fp8_layer_masks is None
    with pytest.raises(ValueError, match="gemm_precision='fp8'"):
        _tiny().fp8_probe(torch.zeros(2, 1, 16, 4, 4))


def test_cli_fp8_max_error_needs_fp8(capsys):
    from scail_amd import cli
    # an argument error (exit status 2) before any model is built: no GPU is touched on the way
    with pytest.raises(SystemExit) as e:
        cli.main(["--tiny", "--fp8-max-error", "0.1"])
    assert e.value.code == 2 and "--fp8-max-error needs --gemm-precision fp8" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        cli.main(["--tiny", "--gemm-precision", "bf16", "--fp8-max-error", "0.1"])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        cli.main(["--tiny", "--gemm-precision", "fp8", "--fp8-max-error", "-0.5"])
    assert e.value.code == 2 and "must be a number >= 0" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        cli.main(["--tiny", "--gemm-precision", "fp8", "--fp8-max-error", "nan"])
    assert e.value.code == 2
    # the function behind it, and cli.run's own check (also before the engine is built)
    assert cli.fp8_max_error_arg(None, "bf16") is None and cli.fp8_max_error_arg(0.25, "fp8") == 0.25
    assert cli.fp8_max_error_arg(INF, "fp8") == INF
    with pytest.raises(ValueError, match="needs --gemm-precision fp8"):
        cli.run(copy.deepcopy(cli.TINY), fp8_max_error=0.1)
    assert "--fp8-max-error" in cli.build_parser().format_help()
    # the printed table: one row per layer, the pairs left in bf16 by (layer, name)
    text = cli.format_fp8_table(dict(rel_err=torch.tensor([[0.01] * 6, [0.01, 0.02, 0.03, 0.04, 0.05, 1.0]]), masks=[63, 31], enabled=63), 0.5)
    assert "left in bf16: (1, w2)" in text and text.count("\n") == 4 and "1.00e+00" in text
    assert "left in bf16: none" in cli.format_fp8_table(dict(rel_err=torch.zeros(1, 6), masks=[3], enabled=3), 0.5)


def test_new_entry_points_validate_without_gpu():
    from scail_amd import lib as L
    lib = L.load()
    a = 1 << 20                 # a 256-byte aligned non-null address: the checks fire before anything is dereferenced
    # scail_rel_err_rows(a, lda, b, ldb, acc, rows, cols, stream)
    for args in ((None, 64, a, 64, a, 4, 64, None), (a, 64, None, 64, a, 4, 64, None), (a, 64, a, 64, None, 4, 64, None)):
        with pytest.raises(L.ScailHipError, match="null pointer"):
            L.call("scail_rel_err_rows", *args)
    with pytest.raises(L.ScailHipError, match="multiple of 8"):
        L.call("scail_rel_err_rows", a, 64, a, 64, a, 4, 60, None)
    with pytest.raises(L.ScailHipError, match="multiple of 8"):
        L.call("scail_rel_err_rows", a, 64, a, 64, a, 4, 0, None)
    with pytest.raises(L.ScailHipError, match="lda / ldb"):
        L.call("scail_rel_err_rows", a, 56, a, 64, a, 4, 64, None)
    with pytest.raises(L.ScailHipError, match="lda / ldb"):
        L.call("scail_rel_err_rows", a, 64, a, 68, a, 4, 64, None)
    with pytest.raises(L.ScailHipError, match="pointer alignment"):
        L.call("scail_rel_err_rows", a + 8, 64, a, 64, a, 4, 64, None)
    with pytest.raises(L.ScailHipError, match="pointer alignment"):
        L.call("scail_rel_err_rows", a, 64, a, 64, a + 4, 4, 64, None)
    with pytest.raises(L.ScailHipError, match="too many rows"):
        L.call("scail_rel_err_rows", a, 64, a, 64, a, 1 << 31, 64, None)
    with pytest.raises(L.ScailHipError, match="multiple of 8"):
        L.call("scail_rel_err_rows", a, 64, a, 64, a, -1, 64, None)
    L.call("scail_rel_err_rows", a, 64, a, 64, a, 0, 64, None)          # an empty problem is accepted and launches nothing
    # executor: null handles
    with pytest.raises(L.ScailHipError, match="null handle"):
        L.call("scail_dit_fp8_select_layers", None, None)
    with pytest.raises(L.ScailHipError, match="null handle"):
        L.call("scail_dit_fp8_probe", None, a, a, 1 << 20)
    with pytest.raises(L.ScailHipError, match="null handle"):
        L.call("scail_dit_fp8_probe", None, None, None, 0)
    assert lib.scail_dit_fp8_probe_bytes(None, 2, 64) == -1
