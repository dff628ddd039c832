"""Record the attention dispatch of a checkout as a table: tests/golden/attn_dispatch_parent.json (names and integers only).

Run ONCE, in a checkout of the commit BEFORE csrc/attn.hip got its choice functions (bfdbb18), where the kernel choice was still stated by
scail_flash_attn_kernel_for, by the launch and by cross4_eligible separately:

    python tools/attn_dispatch_table.py tests/golden/attn_dispatch_parent.json

For every row of the two grids below it records that commit's scail_flash_attn_kernel_for (4 / 8) and scail_cross_attn2_kernel_for (4 / 2)
answer under the row's options.  tests/test_attn_dispatch_cpu.py holds the library of every later commit against the table.
scail_flash_attn_rows_for is left out: it needs a device, and tests/conftest.py attention_plan_rows states it independently.  Needs no GPU."""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 5120                                       # 40 heads x 128
# 32-bit offsets: 69 905 x 15 360 < 2^30 <= 69 906 x 15 360; V^T limit: 128 (Lk + 63) < 2^30 up to Lk = 8 388 544
SELF_COLUMNS = ["q_rs", "k_rs", "o_rs", "Lq", "Lk", "accumulate", "prescaled", "attn4"]
SELF_STRIDES = [(128, 128, 128), (3 * D, 3 * D, D), (3 * D, 128, 128), (128, 3 * D, 128), (128, 128, 3 * D), (D, 2 * D, D + 64)]
SELF_LQ = [1, 256, 300, 48832, 69905, 69906]
SELF_LK = [1, 64, 511, 512, 513, 576, 69905, 69906, 8388544, 8388545]
CROSS_COLUMNS = ["q_rs", "k1_rs", "k2_rs", "o_rs", "Lq", "Lk1", "Lk2", "n_batch", "heads", "attn4", "cross4"]
CROSS_STRIDES = [(128, 128, 128, 128), (3 * D, D, D, D), (D, D, 2 * D, D), (3 * D, 128, 128, 128), (128, 3 * D, 3 * D, 128), (128, 128, 128, 3 * D)]
CROSS_LQ = [1, 300, 69905, 69906]
# 63 / 64 keys per set; 20 / 21 tiles together (1024 + 256 / 257, 1216 / 1217 + 64); the shipped 512 + 257; the V^T limit per set
CROSS_LK = [(63, 64), (64, 63), (64, 64), (512, 257), (1024, 256), (1024, 257), (1216, 64), (1217, 64), (69905, 64), (69906, 64), (64, 69906),
            (8388544, 64), (8388545, 64), (64, 8388545)]
CROSS_BH = [(1, 1), (2, 40), (1, 32767), (1, 32768), (32768, 1), (3, 3)]


def self_grid():
    """rows of SELF_COLUMNS"""
    return [list(s) + [Lq, Lk, acc, pre, a4] for a4 in (1, 0) for s in SELF_STRIDES for Lq in SELF_LQ for Lk in SELF_LK for acc in (0, 1) for pre in (0, 1)]


def cross_grid():
    """rows of CROSS_COLUMNS"""
    return [list(s) + [Lq, k1, k2, b, h, a4, c4] for a4, c4 in itertools.product((1, 0), (2, 1, 0)) for s in CROSS_STRIDES for Lq in CROSS_LQ
            for k1, k2 in CROSS_LK for b, h in CROSS_BH]


def answers(L):
    """-> (one digit per self_grid() row, one digit per cross_grid() row) of the loaded library, under each row's options"""
    lib = L.load()
    opts = None
    out = [[], []]
    try:
        for r in self_grid():
            if r[7] != opts:
                opts = r[7]
                L.set_option("attn4", opts)
            out[0].append(str(lib.scail_flash_attn_kernel_for(*r[:7])))
        opts = None
        for r in cross_grid():
            if (r[9], r[10]) != opts:
                opts = (r[9], r[10])
                L.set_option("attn4", r[9])
                L.set_option("cross4", r[10])
            out[1].append(str(lib.scail_cross_attn2_kernel_for(*r[:9])))
    finally:
        L.set_option("attn4", 1)
        L.set_option("cross4", 2)
    return "".join(out[0]), "".join(out[1])


def write(path, s, x):
    """the table: the answers as digit strings, 120 rows to a line, in the order of the two grids"""
    lines = lambda a: ",\n".join(json.dumps(a[i:i + 120]) for i in range(0, len(a), 120))
    with open(path, "w") as f:
        f.write('{"grids": "tools/attn_dispatch_table.py self_grid(), cross_grid()", "self_rows": %d, "cross_rows": %d,\n "self": [\n%s\n],\n "cross": [\n%s\n]}\n' %
                (len(s), len(x), lines(s), lines(x)))


def read(path):
    """-> (self answers, cross answers) as digit strings"""
    t = json.load(open(path))
    s, x = "".join(t["self"]), "".join(t["cross"])
    assert len(s) == t["self_rows"] and len(x) == t["cross_rows"]
    return s, x


if __name__ == "__main__":
    from scail_amd import build
    build.build(verbose=False)
    from scail_amd import lib as L
    s, x = answers(L)
    write(sys.argv[1], s, x)
    print(f"{len(s)} self-attention rows, {len(x)} cross-attention rows -> {sys.argv[1]}")
