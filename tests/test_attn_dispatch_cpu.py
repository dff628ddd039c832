"""The attention dispatch of csrc/attn.hip (attn_choose and cross_choose, one statement each behind the launches and the host-only queries)
against the table recorded at the commit before they existed (tests/golden/attn_dispatch_parent.json, written by tools/attn_dispatch_table.py):
for 2 880 self-attention and 12 096 cross-attention argument rows on both sides of every threshold -- key counts, accumulate, the 32-bit offset
limit of each stride, the V^T limit, 20 / 21 key tiles, K row strides, 32 767 / 32 768 heads and batch elements, options attn4 and cross4 --
scail_flash_attn_kernel_for and scail_cross_attn2_kernel_for answer what they answered, and the name queries name a kernel of that family.
scail_flash_attn_rows_for is not in the table: it needs a device (tests/conftest.py attention_plan_rows states it independently).  Needs no GPU."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_dispatch_parent.json")


def library():
    from scail_amd import build
    build.build(verbose=False)
    from scail_amd import lib as L
    L.load()
    return L


def test_every_row_answers_as_the_parent_did():
    import attn_dispatch_table as T
    L = library()
    want_self, want_cross = T.read(TABLE)
    got_self, got_cross = T.answers(L)
    assert len(want_self) == len(T.self_grid()) == 2880 and len(want_cross) == len(T.cross_grid()) == 12096
    assert set(want_self) == {"4", "8"} and set(want_cross) == {"4", "2"}
    bad = [(r, g, w) for r, g, w in zip(T.self_grid(), got_self, want_self) if g != w]
    assert not bad, f"{len(bad)} self-attention rows differ, the first: {bad[:5]}"
    bad = [(r, g, w) for r, g, w in zip(T.cross_grid(), got_cross, want_cross) if g != w]
    assert not bad, f"{len(bad)} cross-attention rows differ, the first: {bad[:5]}"


def test_the_name_queries_name_the_same_family():
    """the name queries on the rows of both grids under the default options and with the generated kernels off (kernel_name / cross_kernel_name
    assert that the number queries agree; the self-attention rows are one (batch, head) pair, which the seven-argument query answers for)"""
    import attn_dispatch_table as T
    import attn_exact as X
    library()
    want_self, want_cross = T.read(TABLE)
    for r, w in zip(T.self_grid(), want_self):
        got = X.with_options({"attn4": r[7]}, lambda: X.kernel_name(r[0], r[1], r[2], 1, 1, r[3], r[4], r[5], r[6]))
        assert got == {"4": X.GEN, "8": X.W8}[w], r
    for r, w in zip(T.cross_grid(), want_cross):
        if r[10] == 2:                                                                       # (the default; cross4 = 0 / 1 are in the first test)
            got = X.with_options({"attn4": r[9]}, lambda: X.cross_kernel_name(*r[:9]))
            assert got == {"4": X.X_GEN, "2": X.X_HIP}[w], r
