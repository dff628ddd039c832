"""Generate tests/golden/partition_rules.npz: the REAL reference's tensor-parallel split of a weight
(sat/mpu/layers.py ColumnParallelLinear.partition :286-340, RowParallelLinear.partition :438-460) on seeded
weights, for the strides the DiT uses.  tests/test_checkpoint_cpu.py checks scail_amd/checkpoint.py against it.

Build-container only (needs the reference tree, oracle/ref_shims.py).  Usage:  python oracle/gen_golden_partition.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from oracle import ref_shims  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")
COLUMN_STRIDES = (1, 2, 3)
COLUMN_RANKS = (2, 4)
ROW_RANKS = 4


def main():
    ref_shims.load_reference()
    from sat import mpu
    if not mpu.model_parallel_is_initialized():
        mpu.initialize_model_parallel(1)
    from sat.mpu.layers import ColumnParallelLinear, RowParallelLinear
    res = {}
    for stride in COLUMN_STRIDES:
        g = torch.Generator().manual_seed(1)
        out_f, in_f = 24 * stride, 16
        lin = ColumnParallelLinear(in_f, out_f, stride=stride, gather_output=False, bias=True)
        w = torch.randn(out_f, in_f, generator=g)
        res[f"col_s{stride}_w"] = w.numpy()
        for n in COLUMN_RANKS:
            for r, part in enumerate(lin.partition(new_model_parallel_size=n, full_weight=w)):
                res[f"col_s{stride}_n{n}_r{r}"] = part.numpy()
    lin = RowParallelLinear(32, 8, input_is_parallel=True, bias=True)
    w = torch.randn(8, 32, generator=torch.Generator().manual_seed(2))
    res["row_w"] = w.numpy()
    for r, part in enumerate(lin.partition(new_model_parallel_size=ROW_RANKS, full_weight=w)):
        res[f"row_n{ROW_RANKS}_r{r}"] = part.numpy()
    np.savez_compressed(os.path.join(OUT, "partition_rules.npz"), **res)
    print("wrote", os.path.join(OUT, "partition_rules.npz"), len(res), "arrays")


if __name__ == "__main__":
    main()
