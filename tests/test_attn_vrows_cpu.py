"""The V-rows self-attention (scail_flash_attn_vrows_bf16: v as the QKV projection wrote it, no scail_transpose_v pass) without a GPU: the emulator's
ds_read_b64_tr_b16 against a numpy statement of the instruction, scail_attn4_m16f_vr / scail_attn4_m16f_q3_vr in the emulator on the exact operands
of tests/attn_exact.py -- bit-equal to the V^T kernels' emulator output, inside a v buffer that ends at key row Lk - 1 (the emulator's arena refuses
any read past it), with the dynamic hazard walk on (tests/conftest.py) --, the host queries and refusals, and the code objects."""
import os
import sys

import numpy as np
import pytest
import torch

import attn_exact as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scail_amd.asmgen import attn4, codeobj, isa, sched  # noqa: E402
from tools import asm_emu as E  # noqa: E402
from tools import attn4_emu_run as R  # noqa: E402


# ---- the instruction ------------------------------------------------------------------------------------------------------------------------
def _tr_program(offset=0):
    V = isa.V
    return [isa.ds_read_b64_tr_b16(V(2, 2), V(1), offset), isa.waitcnt(lgkmcnt=0), isa.Instr("s_endpgm", cls=isa.BRANCH)]


def _tr_emu(addr, offset=0, exec_mask=None):
    """one wave: LDS holds the 16-bit element index at every position; v1 = the lane addresses; returns v2, v3"""
    emu = E.Emu(_tr_program(offset), E.Memory(size=1 << 16), n_waves=1, lds_bytes=8192)
    emu.lds[:] = np.arange(4096, dtype=np.uint16).view(np.uint8)
    w = emu.waves[0]
    w.v[1] = np.asarray(addr, dtype=np.uint32)
    if exec_mask is not None:
        w.exec = exec_mask
    emu.launch(b"\0" * 8)
    return w.v[2].copy(), w.v[3].copy()


def test_emulator_transposed_read_is_the_numpy_statement():
    """Each 16-lane group g reads its own 4-row x 16-column block of 16-bit elements -- here four different blocks of a row-major [rows][cols] image,
    one per group, with different row strides -- and lane i of the group receives column i: row q in element q.  Lane 4 q + p addresses columns
    4 p .. 4 p + 3 of row q"""
    lane = np.arange(64)
    g, q, p = lane >> 4, (lane >> 2) & 3, lane & 3
    stride = np.array([64, 128, 256, 72])[g]                  # elements per row of the group's image (72: rows 144 bytes apart, 8-byte aligned)
    row0, col0 = np.array([0, 3, 1, 5])[g], np.array([0, 16, 32, 8])[g]
    addr = 2 * ((row0 + q) * stride + col0 + 4 * p)
    for offset in (0, 1024):
        lo, hi = _tr_emu(addr, offset)
        i = lane & 15
        want = [(row0 + r) * stride + col0 + i + offset // 2 for r in range(4)]      # the element index = what the LDS holds there
        assert np.array_equal(lo, want[0] | (want[1] << 16)) and np.array_equal(hi, want[2] | (want[3] << 16)), offset
    assert len({int(x) for x in lo[:16]}) == 16 and not np.array_equal(lo[:16], lo[16:32])


def test_emulator_transposed_read_refuses_partial_exec_and_misaligned_addresses():
    addr = 8 * np.arange(64)
    mask = np.ones(64, dtype=bool)
    mask[37] = False
    with pytest.raises(RuntimeError, match="partial EXEC"):
        _tr_emu(addr, exec_mask=mask)
    bad = addr.copy()
    bad[5] += 4
    with pytest.raises(RuntimeError, match="8-byte alignment"):
        _tr_emu(bad)
    _tr_emu(addr)
    # an LGKM operation of class DS_READ for the hazard rules and the counted waits, EXEC an implicit read
    ins = _tr_program()[0]
    assert ins.cls == isa.DS_READ and ("exec", 0) in ins.reads()
    seq = sched.insert_lgkm_waits([ins, isa.vop("v_mov_b32", isa.V(9), isa.V(3))])
    assert [i.op for i in seq] == ["ds_read_b64_tr_b16", "s_waitcnt", "v_mov_b32"] and seq[1].lgkmcnt == 0


# ---- the kernels in the emulator ----------------------------------------------------------------------------------------------------------------
PAIRS = {256: (attn4.M16F, attn4.M16F_VR), 192: (attn4.M16F_Q3, attn4.M16F_Q3_VR)}


def _both(rows, Lk, **kw):
    """the V^T kernel and its V-rows form on the same exact operands: (outputs as bf16 tensors, statistics, operands)"""
    spike = kw.pop("spike", None)
    q, k, v = X.exact_qkv("sparse_q", 1, 1, rows, Lk, 2000 + rows + Lk, False, spike, lazy_key=kw.pop("lazy_key", None))
    out = []
    for cfg in PAIRS[rows]:
        o, st = R.run(cfg, q.numpy(), [k.numpy()], [v.numpy()], 1, sl2=1.0, **kw)
        out.append((o, st))
    return out, (q, k, v)


@pytest.mark.parametrize("rows,Lk", [(256, 512), (192, 536)])
def test_emulator_vr_kernels_equal_the_vt_kernels_bit_for_bit(rows, Lk):
    """one pair, a whole number of tiles and a ragged last tile (24 valid keys: v ends at row 535, and the arena refuses a read behind it); the exact
    operands also go through the checker"""
    ((o_vt, st_vt), (o_vr, st_vr)), (q, k, v) = _both(rows, Lk)
    assert PAIRS[rows][1].vr and not PAIRS[rows][0].vr
    assert np.array_equal(o_vr.view(np.uint32), o_vt.view(np.uint32))
    assert st_vr["mfma"] == st_vt["mfma"] and st_vr["restarts"] == 0
    X.check(torch.from_numpy(o_vr).to(X.BF16), X.reference(q, k, v, 1), f"emulator {PAIRS[rows][1].name} Lk {Lk}")


def test_emulator_vr_restart_walks_v_again():
    """the c = 64 key (tile 3: inside the optimistic hot loop of a 12-tile pass) overflows the row sums: the workgroup runs again from L_restart and
    re-walks the V stream from row 0; ragged key count"""
    Lk, spike = 64 * 11 + 9, (64 * 3 + 7, X.RESTART_C)
    ((o_vt, st_vt), (o_vr, st_vr)), (q, k, v) = _both(256, Lk, spike=spike)
    assert st_vr["restarts"] == st_vt["restarts"] == 1
    assert np.array_equal(o_vr.view(np.uint32), o_vt.view(np.uint32))
    X.check(torch.from_numpy(o_vr).to(X.BF16), X.reference(q, k, v, 1, restart_key=spike[0]), "emulator scail_attn4_m16f_vr restart")


@pytest.mark.parametrize("cfg", [attn4.M16F_VR, attn4.M16F_Q3_VR], ids=lambda c: c.name)
def test_vr_static_hazards_clean(cfg):
    assert R.check_static(cfg) == []


def test_vr_tile_image_is_conflict_free_and_needs_one_address():
    """the bank rule of the transposed read: (address / 4) % 64 over each 32-lane half must be 32 x 2 different banks.  Addresses as the prologue
    computes them (2048 (g >> 1) + 128 (g & 1) + 8 (lane % 16)) + every immediate offset of a tile's 32 reads"""
    lane = np.arange(64)
    g = lane >> 4
    base = 2048 * (g >> 1) + 128 * (g & 1) + 8 * (lane & 15)
    reads = [i for i in attn4.Gen(attn4.M16F_VR).v_frag_reads16(1, 0.0, 1.0)]
    assert len(reads) == 32 and {i.src[0] for i in reads} == {attn4.VADDR16[0]} and all(i.op == "ds_read_b64_tr_b16" for i in reads)
    seen = set()
    for i in reads:
        a = base + i.offset
        assert not (a % 8).any()
        for half in (a[:32], a[32:]):
            banks = np.concatenate([(half // 4) % 64, (half // 4 + 1) % 64])
            assert len(set(banks.tolist())) == 64
        seen.update((a - 16384).tolist())
    assert seen == set(range(0, 16384, 8))               # the 32 reads of a wave cover the 16 KiB slot exactly once


def test_attn4_kept_its_kernels_and_the_vrows_code_object_is_a_build_product():
    """the V-rows kernels are a code object of their own that build.py generates (not committed); csrc/attn4.s holds the three V^T kernels as the
    generator emits them, which use neither the new instruction nor the extra SGPRs"""
    cos = {c.stem: c for c in codeobj.CODE_OBJECTS if c.gen == "attn4"}
    assert sorted(cos) == ["attn4", "attn4v"] and cos["attn4"].committed and not cos["attn4v"].committed
    assert not os.path.exists(os.path.join(codeobj.CSRC, "attn4v.s")) and os.path.dirname(cos["attn4v"].path("/some/build")) == "/some/build"
    assert [c.name for c in attn4.SHIPPED] == ["scail_attn4_m16f", "scail_attn4_m16f_q3", "scail_attn4_x2"]
    assert [c.name for c in attn4.VROWS] == ["scail_attn4_m16f_vr", "scail_attn4_m16f_q3_vr"]
    old, new = open(cos["attn4"].path()).read(), cos["attn4v"].text()
    assert old == cos["attn4"].text() and "tr_b16" not in old and "s96" not in old and "_vr" not in old
    assert new.count("ds_read_b64_tr_b16") > 0 and new.count(".amdhsa_next_free_sgpr 100") == 2 and ".amdhsa_next_free_sgpr 96" in old


# ---- the host: queries and refusals -----------------------------------------------------------------------------------------------------------
def _name(q_rs, k_rs, v_rs, o_rs, B, H, Lq, Lk, plan=False):
    import ctypes as C
    from scail_amd import lib as L
    buf, pl = C.create_string_buffer(128), (C.c_int64 * 9)()
    L.call("scail_flash_attn_vrows_kernel_name_for", q_rs, k_rs, v_rs, o_rs, B, H, Lq, Lk, buf, len(buf), C.cast(pl, C.c_void_p) if plan else None)
    return (buf.value.decode(), list(pl)) if plan else buf.value.decode()


def test_vrows_queries():
    from scail_amd import lib as L
    lib = L.load()
    D = 4 * X.HD
    assert lib.scail_flash_attn_vrows_for(3 * D, 3 * D, 3 * D, D, 2, 4, 300, 512) == 1
    assert _name(3 * D, 3 * D, 3 * D, D, 2, 4, 300, 512) == "scail_attn4_m16f_vr"
    for rows, want in ((256, "scail_attn4_m16f_vr"), (192, "scail_attn4_m16f_q3_vr")):
        got = X.with_options({"attn4_rows": rows}, lambda: _name(3 * D, 3 * D, 3 * D, D, 2, 4, 300, 512, plan=True))
        assert got == (want, [1, rows, 0, 8 * -(-300 // rows), 1, 0, 0, 0, 0]), got
    # what scail_flash_attn_bf16 runs does not change with the new input of the choice
    assert X.kernel_name(3 * D, 3 * D, D, 2, 4, 300, 512, False, True) == X.GEN
    no = [dict(Lk=511), dict(v_rs=D - 8), dict(v_rs=3 * D + 4), dict(Lk=(1 << 30) // (3 * D) + 1), dict(B=1 << 15)]
    for kw in no:
        a = dict(q_rs=3 * D, k_rs=3 * D, v_rs=3 * D, o_rs=D, B=2, H=4, Lq=300, Lk=512)
        a.update(kw)
        assert lib.scail_flash_attn_vrows_for(*a.values()) == 0, kw
        assert _name(*a.values(), plan=True) == ("none", [0] * 9), kw
    for opt in ("attn_vrows", "attn4"):
        assert X.conv_exact.with_options({opt: 0}, lambda: lib.scail_flash_attn_vrows_for(3 * D, 3 * D, 3 * D, D, 2, 4, 300, 512), {opt: 1}) == 0
    assert lib.scail_flash_attn_vrows_for(3 * D, 3 * D, 3 * D, D, 2, 4, 300, 512) == 1


def test_vrows_entry_refuses_what_the_kernel_cannot_take_and_names_the_value():
    """before anything touches a device: the entry has no other kernel to fall to"""
    from scail_amd import lib as L
    L.load()
    D = 2 * X.HD

    def call(q_rs=D, k_rs=D, v_rs=D, o_rs=D, B=1, H=2, Lq=256, Lk=512, scale=0.1, v=0):
        L.call("scail_flash_attn_vrows_bf16", None, Lq * q_rs, q_rs, None, Lk * k_rs, k_rs, v or None, Lk * v_rs, v_rs, None, Lq * o_rs, o_rs, B, H, Lq, Lk, scale, None)

    big = (1 << 30) // (3 * D) + 1
    for kw, msg in ((dict(Lk=300), r"Lk = 300 is below the 512 keys"), (dict(v_rs=D - 8), rf"v_rs = {D - 8} must be a multiple of 8 and at least heads \* 128 = {D}"),
                    (dict(v_rs=3 * D, Lk=big), rf"Lk \* v_rs = {big * 3 * D} elements is beyond the 32-bit byte offsets"),
                    (dict(k_rs=3 * D, Lk=big), rf"Lk \* k_rs = {big * 3 * D} elements"), (dict(q_rs=3 * D, Lq=big), rf"Lq \* q_rs = {big * 3 * D} elements"),
                    (dict(B=1 << 15), r"n_batch = 32768, heads = 2, Lq = 256 is beyond the kernel's workgroup-id decode"),
                    (dict(v_rs=D + 4), "alignment"), (dict(v=8), "pointer alignment"), (dict(v_rs=0), "v_rs = 0"), (dict(scale=0.0), "scale must be")):
        with pytest.raises(L.ScailHipError, match=msg):
            call(**kw)
    for opt, msg in (("attn_vrows", "option attn_vrows is 0"), ("attn4", "option attn4 is 0")):
        with pytest.raises(L.ScailHipError, match=msg):
            X.conv_exact.with_options({opt: 0}, call, {opt: 1})
    with pytest.raises(L.ScailHipError, match="unknown option"):
        L.set_option("attn_vrow", 1)
