"""CPU emulation (tools/asm_emu.py) of the generated GEMM kernels (scail_amd/asmgen/gemm4.py): the four shipped kernels
(scail_gemm4_e0/1/3/4, csrc/gemm4.s) and the timing ablations of the measurement build: the generator produces hazard-free code, and the
shipped kernels' results equal the fp64 product of the bf16-rounded operands, under the emulator's lazy (latest-allowed) completion of LDS / memory
operations -- the mode that exposes a missing or too-weak s_waitcnt."""
import math

import numpy as np
import pytest

from scail_amd.asmgen import gemm4
from tools import gemm4_emu_run as R


def _case(cfg, M, N, K, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / math.sqrt(K)).astype(np.float32)
    kw = dict(bias=rng.standard_normal(N).astype(np.float32))
    if cfg.epi in (3, 4):
        kw["resid"] = rng.standard_normal((M, N)).astype(np.float32)
    if cfg.epi == 3:
        kw.update(gate=rng.standard_normal((2, N)).astype(np.float32), rows_per_batch=(M + 1) // 2)
    return x, w, kw


def _variant(name):
    return [c for c in gemm4.DEFAULTS + gemm4.variant_cfgs() if c.name == name][0]


@pytest.mark.parametrize("name,shape", [("scail_gemm4_e0", (300, 256, 192)),              # SHIPPED: LDS-DMA two tiles deep, 16x16x32 MFMAs; ragged last m-tile
                                        ("scail_gemm4_e1", (256, 256, 128)),              # + GELU-tanh
                                        ("scail_gemm4_e3", (264, 256, 320)),              # gate * (acc + bias) + residual, odd tile count
                                        ("scail_gemm4_e4", (520, 512, 128))])             # residual, two m-tiles and n-tiles + ragged third
def test_gemm4_emulated(name, shape):
    cfg = _variant(name)
    assert R.check_static(cfg) == [], "hazard distances of the generated loop / prologue"
    x, w, kw = _case(cfg, *shape)
    y, _ = R.run(cfg, x, w, lazy=True, **kw)
    ref = R.reference(cfg, x, w, **kw)
    err = np.abs(y - ref)
    assert err.max() <= 2.0 ** -7 * max(1.0, np.abs(ref).max()), float(err.max())     # one bf16 rounding of the output


@pytest.mark.parametrize("cfg", gemm4.variant_cfgs(), ids=lambda c: c.name)
def test_gemm4_timing_ablations_are_hazard_free(cfg):
    """the measurement build's timing ablations (an instruction class of the k-loop removed: wrong results on purpose, so nothing to
    compare) still keep every issue distance"""
    assert cfg.abl and R.check_static(cfg) == []
