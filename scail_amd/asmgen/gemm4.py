"""gemm4 -- hand-scheduled bf16 GEMM  y = epi(x W^T + b)  for the big per-token projections of the SCAIL DiT on gfx950
(generator of csrc/gemm4.s).  Replaces F.linear in ColumnParallelLinear / RowParallelLinear (sat/mpu/layers.py:237, 435) and the
gate / residual / GELU ops around it (dit_video_crossattn_sc_xc.py:1036, 1042, 1050; sat/transformer_defaults.py:163-176); same C
entry point as the kernels of csrc/gemm.hip (scail_gemm_bf16), which selects this kernel for M >= 2048, N % 256 == 0, K % 64 == 0.

Shape (the structure of the vendor's own MI355X GEMM: 256 x 256 x 64 macro tile, 4 waves, one per SIMD):
  * workgroup = one 256 (m) x 256 (n) tile of y, 4 waves as 2 (m) x 2 (n), wave tile 128 x 128 = 8 x 8 blocks of 16 x 16
    (v_mfma_f32_16x16x32_bf16, 128 per k-tile); the 256 fp32 accumulators per lane fill the whole accumulator file a[0:255]; the arch
    VGPRs hold only fragments and addresses
  * MFMA issued "transposed" like gemm.hip: A = W fragment (rows n), B = x fragment (columns m) -> a lane's accumulator registers
    run along n: 4 consecutive n per register quad
  * x and W k-tiles (256 rows x 64 k = 32 KB each) arrive by LDS-DMA (`buffer_load ... lds`, 16 pieces of 1 KB per wave and k-tile), two
    tiles deep inside two 64 KB slots.  LDS rows are whole 128-byte lines, XOR-swizzled on the SOURCE address (chunk ^ ((row >> 1) & 7));
    the fragments of a 32-wide k-step are read half a tile ahead of their MFMAs into two register sets; two s_barrier per k-tile (see
    Gen.body); no LDS write instruction exists in the k-loop
  * tile order = a host-built table (XCD-aware + grouped: the 32 tiles resident on an XCD share 4 + 8 operand panels in its L2),
    read with one s_load per workgroup: no integer division in the kernel
  * epilogues as separate kernels: bias (0), bias + GELU-tanh (1), residual + gate * (. + bias) (3), residual + (. + bias) (4);
    bias may be NULL.  Every epilogue goes through LDS, so that a global store / residual load moves whole cache lines (Gen.epilogue)

The measurement build adds timing ablations of this schedule (``abl``: wrong results on purpose; variant_cfgs).

Limits (the C entry keeps gemm.hip's kernels otherwise): N % 256 == 0, K % 64 == 0, K >= 128, M * ld < 2^31 elements.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import List

from . import codeobj, isa, sched
from .isa import A, S, V, I32, F32, Neg, VCC, EXEC, M0, Instr

KERNARG_SIZE = 112
KERNARG_FMT = "<7Q4q4i2i"      # x w bias y resid gate table | lda ldc ldr gs | M N K rows_per_batch | two reserved words (0)


def pack_args(x, w, bias, y, resid, gate, table, lda, ldc, ldr, gs, M, N, K, rpb) -> bytes:
    b = struct.pack(KERNARG_FMT, x, w, bias, y, resid, gate, table, lda, ldc, ldr, gs, M, N, K, rpb, 0, 0)
    assert len(b) == KERNARG_SIZE
    return b


def tile_table(M: int, N: int, group_m: int = 4):
    """Tile order (list of (m_tile << 16 | n_tile... stored as m_tile | n_tile << 16): workgroup id b runs on XCD b % 8; each XCD
    gets a contiguous range of the GROUPED order (group_m m-tiles x all n-tiles column by column), so the 32 tiles in flight on an
    XCD cover ~4 m-panels x 8 n-panels."""
    tm, tn = (M + 255) // 256, N // 256
    order = []
    for g0 in range(0, tm, group_m):
        rows = range(g0, min(g0 + group_m, tm))
        for n in range(tn):
            for m in rows:
                order.append(m | (n << 16))
    T = len(order)
    per = (T + 7) // 8
    table = []
    for b in range(per * 8):
        xcd, j = b & 7, b >> 3
        lin = xcd * per + j
        table.append(order[lin] if lin < T else 0xFFFFFFFF)
    return table


@dataclass
class Cfg:
    """Defaults = the shipped schedule (measured best of the sweep in profiles/r02_gemm4_mi16.log: 1467 TFLOP/s where q8 does 1309, the
    vendor 1495).  Gap numbers are in units of 32 matrix-pipe cycles = two MFMA gaps."""
    epi: int = 0           # 0 bias, 1 bias + GELU-tanh, 3 resid + gate * (acc + bias), 4 resid + (acc + bias)
    name: str = "scail_gemm4_e0"
    cap: int = 1           # fillers per MFMA gap
    lookahead: float = 1.0 # scheduler: how far before its target gap a filler may be placed
    b1_at: float = 5.5     # gap of the barrier that releases the slot (after the reads of the second k-step)
    b2_at: float = 31.5    # gap of the barrier that publishes tile t+1
    rd2_step: float = 0.25 # spacing of the 16 fragment reads of a k-step
    dma_step: float = 1.75 # spacing of the 16 LDS-DMA pieces of tile t+2 (x 2: one piece per 7 MFMA gaps)
    abl: str = ""          # TIMING ABLATIONS (wrong results; measurement build only): "dma" / "lds" / "bar" removed from the k-loop


# 8 x 8 blocks of 16 x 16 per wave (4 accumulators each), fragments of a k32-step = 8 + 8 quads: set 0 = v0..63, set 1 = v96..159
def ACC16(nb, mb): return A((nb * 8 + mb) * 4, 4)
def FW16(s, nb): return V((0 if s == 0 else 96) + nb * 4, 4)            # W fragments (MFMA A operand)
def FX16(s, mb): return V((0 if s == 0 else 96) + 32 + mb * 4, 4)       # x fragments (MFMA B operand)


XADDR = [[V(64 + s * 4 + ks) for ks in range(2)] for s in range(2)]      # fragment read address [slot][k-step]
WADDR = [[V(72 + s * 4 + ks) for ks in range(2)] for s in range(2)]
XDMA = [V(80 + i) for i in range(8)]         # per-piece source offsets (bytes inside the operand panel)
WDMA = [V(88 + i) for i in range(8)]
LANE = V(228)
T_ = [V(229 + i) for i in range(27)]         # v229..255 temporaries (prologue / epilogue); T_[1], T_[2] = lane geometry, kept

S_KARG = S(0, 2)
S_WG = S(2)
S_X, S_W, S_BIAS, S_Y = S(8, 2), S(10, 2), S(12, 2), S(14, 2)
S_RES, S_GATE = S(16, 2), S(18, 2)
S_TAB = S(20, 2)
S_LDA, S_LDC, S_LDR, S_GS = S(24, 2), S(26, 2), S(28, 2), S(30, 2)
S_M, S_N, S_K, S_RPB = S(32), S(33), S(34), S(35)
S_XRSRC, S_WRSRC = S(36, 4), S(40, 4)
S_KOFF, S_KMAX, S_T, S_KT = S(44), S(45), S(46), S(47)
S_WAVE, S_WM, S_WN = S(48), S(49), S(50)
S_M0T, S_N0T = S(51), S(52)                  # tile origin (rows / columns)
S_XLDS, S_WLDS = S(53), S(54)                # LDS byte offset of this wave's DMA region inside a slot
ST = [S(56 + i) for i in range(16)]          # s56..s71 temporaries
S_SAVE = S(72, 2)
S_WOFF, S_WMAX = S(74), S(75)                # set by the prologue, read by nothing (two instructions the committed code objects carry)


class Gen:
    def __init__(self, cfg: Cfg):
        self.cfg = cfg

    # ---------------------------------------------------------------------------------------------
    def mfmas16(self, s: int) -> List[Instr]:
        return [isa.mfma16(ACC16(nb, mb), FW16(s, nb), FX16(s, mb), ACC16(nb, mb), tag=f"k{s}") for nb in range(8) for mb in range(8)]

    def frag_reads16(self, slot: int, s: int, t0: float, step: float) -> List[Instr]:
        out = []
        for i in range(8):
            out.append(isa.ds_read_b128(FW16(s, i), WADDR[slot][s], 2048 * i, target_gap=t0 + step * (2 * i)))
            out.append(isa.ds_read_b128(FX16(s, i), XADDR[slot][s], 2048 * i, target_gap=t0 + step * (2 * i + 1)))
        return out

    def dma_tile(self, slot: int, t0: float, step: float) -> List[Instr]:
        """16 LDS-DMA pieces of this wave (8 x rows, 8 W rows: 64 rows of each operand tile) for the k-tile at S_KOFF."""
        out = []
        k = 0
        for lds, offs, rsrc in ((S_XLDS, XDMA, S_XRSRC), (S_WLDS, WDMA, S_WRSRC)):
            for half in range(2):
                out.append(isa.sop("s_add_u32", M0, lds, I32(slot * 65536 + half * 4096), target_gap=t0 + step * k - 0.5))
                for i in range(4):
                    out.append(isa.buffer_load_lds(offs[half * 4 + i], rsrc, S_KOFF, 1024 * i, target_gap=t0 + step * k, tag="dma"))
                    k += 1
        out.append(isa.sop("s_add_u32", S_KOFF, S_KOFF, I32(128), target_gap=t0 + step * k))
        out.append(isa.sop("s_min_u32", S_KOFF, S_KOFF, S_KMAX, target_gap=t0 + step * k + 0.1))
        return out

    # ---- LDS-DMA staging two tiles deep inside the two 64 KB slots -----------------------------------------------------------------
    #   registers hold the fragments of a whole k-tile (2 sets); they are read HALF A TILE ahead of their MFMAs:
    #     gaps  0-31  MFMA k-step 0 of tile t   ||  read fragments of k-step 1 of tile t (slot p)
    #     barrier B1 (every wave has read the last fragments of tile t: slot p is free)
    #     gaps ~11-.. the 16 LDS-DMA pieces of tile t+2 -> slot p
    #     barrier B2 (each wave: vmcnt(pieces of THIS iteration issued so far) -> its pieces of tile t+1, issued one iteration
    #                 ago, have landed; after the barrier everybody's have)
    #     gaps 32-63  MFMA k-step 1 of tile t   ||  read fragments of k-step 0 of tile t+1 (slot p^1)
    #   -> a DMA piece has 0.8-1.3 tile periods of flight, a fragment read half a tile, and no LDS write instruction exists.
    def body(self, p: int) -> List[Instr]:
        """One k-tile (128 MFMAs) on slot p."""
        c = self.cfg
        abl = c.abl.split(",")
        gs = 2.0                                  # MFMA gaps per 32 matrix-pipe cycles
        b1_at, b2_at = c.b1_at * gs, c.b2_at * gs + 0.5
        rd_a = [] if "lds" in abl else self.frag_reads16(p, 1, 0.0, c.rd2_step * gs)
        w1, b1 = isa.waitcnt(lgkmcnt=0, target_gap=b1_at - 0.2), isa.barrier(target_gap=b1_at)
        w1.after, b1.after = list(rd_a), list(rd_a) + [w1]
        dma = [] if "dma" in abl else self.dma_tile(p, b1_at + 0.5, c.dma_step * 2.0 * gs)
        for i in dma:
            i.after = [b1]
        w2, b2 = isa.waitcnt(vmcnt=0, target_gap=b2_at - 0.2), isa.barrier(target_gap=b2_at)
        b2.after = [w2, b1]
        w2.after = [b1]
        rd_b = [] if "lds" in abl else self.frag_reads16(p ^ 1, 0, b2_at + 0.5, c.rd2_step * gs)
        for i in rd_b:
            i.after = [b2]
        sync1 = [w1] + ([b1] if "bar" not in abl else [])
        sync2 = [w2] + ([b2] if "bar" not in abl else [])
        blk = rd_a + sync1 + dma + self.mfmas16(0) + sync2 + rd_b + self.mfmas16(1)
        seq = sched.schedule(blk, cap=c.cap, lookahead=c.lookahead)
        n_before = sum(1 for i in seq[:seq.index(w2)] if getattr(i, "tag", "") == "dma")
        w2.vmcnt, w2.mods = n_before, f"vmcnt({n_before})"
        return seq

    # ---------------------------------------------------------------------------------------------
    def addr64_madd(self, ptr: isa.Reg, a, b, shift: int) -> List[Instr]:
        """ptr(64) += (a * b) << shift   (a, b: 32-bit SGPRs / immediates, unsigned)."""
        lo, hi = ST[0], ST[1]
        st = S(ST[2].idx, 2)
        return [isa.sop("s_mul_i32", lo, a, b), isa.sop("s_mul_hi_u32", hi, a, b),
                isa.sop("s_mov_b32", st.sub(0), lo), isa.sop("s_mov_b32", st.sub(1), hi), isa.sop("s_lshl_b64", st, st, I32(shift)),
                isa.sop("s_add_u32", ptr.sub(0), ptr.sub(0), st.sub(0)), isa.sop("s_addc_u32", ptr.sub(1), ptr.sub(1), st.sub(1))]

    def prologue(self) -> List[Instr]:
        c = self.cfg
        o: List[Instr] = [isa.label(c.name)]
        o += [isa.s_load(8, S(8, 8), S_KARG, 0), isa.s_load(4, S(16, 4), S_KARG, 32), isa.s_load(2, S_TAB, S_KARG, 48),
              isa.s_load(8, S(24, 8), S_KARG, 56), isa.s_load(4, S(32, 4), S_KARG, 88),
              isa.vop("v_and_b32", LANE, I32(63), V(0)), isa.vop("v_lshrrev_b32", T_[0], I32(6), V(0)),
              isa.waitcnt(lgkmcnt=0), isa.vop("v_readfirstlane_b32", S_WAVE, T_[0])]
        # tile of this workgroup from the host-built order table
        ent = ST[4]
        o += [isa.sop("s_lshl_b32", ST[5], S_WG, I32(2)), isa.sop("s_add_u32", S_TAB.sub(0), S_TAB.sub(0), ST[5]),
              isa.sop("s_addc_u32", S_TAB.sub(1), S_TAB.sub(1), I32(0)), isa.s_load(1, ent, S_TAB, 0), isa.waitcnt(lgkmcnt=0),
              isa.sop("s_cmp_eq_u32", None, ent, I32(0xFFFFFFFF)), isa.branch("s_cbranch_scc1", "L_exit"),
              isa.sop("s_and_b32", ST[5], ent, I32(0xFFFF)), isa.sop("s_lshr_b32", ST[6], ent, I32(16)),
              isa.sop("s_lshl_b32", S_M0T, ST[5], I32(8)), isa.sop("s_lshl_b32", S_N0T, ST[6], I32(8)),
              isa.sop("s_lshr_b32", S_WM, S_WAVE, I32(1)), isa.sop("s_and_b32", S_WN, S_WAVE, I32(1))]
        # descriptors: x rows from m0 (base += m0 * lda * 2), W rows from n0 (base += n0 * K * 2)
        o += self.addr64_madd(S_X, S_M0T, S_LDA.sub(0), 1) + self.addr64_madd(S_W, S_N0T, S_K, 1)
        for rs, ptr in ((S_XRSRC, S_X), (S_WRSRC, S_W)):
            o += [isa.sop("s_mov_b32", rs.sub(0), ptr.sub(0)), isa.sop("s_and_b32", rs.sub(1), ptr.sub(1), I32(0xFFFF)),
                  isa.sop("s_mov_b32", rs.sub(2), I32(0xFFFFFFFF)), isa.sop("s_mov_b32", rs.sub(3), I32(0x00020000))]
        ldab, kb2 = ST[6], ST[7]
        o += [isa.sop("s_lshl_b32", ldab, S_LDA.sub(0), I32(1)), isa.sop("s_lshl_b32", kb2, S_K, I32(1)),
              isa.sop("s_lshr_b32", S_KT, S_K, I32(6)), isa.sop("s_sub_u32", ST[8], S_KT, I32(1)), isa.sop("s_lshl_b32", S_KMAX, ST[8], I32(7)),
              isa.sop("s_mov_b32", S_KOFF, I32(0)), isa.sop("s_mov_b32", S_T, I32(0)),
              isa.sop("s_mov_b32", S_WOFF, I32(0)), isa.sop("s_lshl_b32", S_WMAX, ST[8], I32(15)),
              isa.sop("s_lshl_b32", S_XLDS, S_WAVE, I32(13)), isa.sop("s_add_u32", S_WLDS, S_XLDS, I32(32768))]
        ql, g, t = T_[1], T_[2], T_
        # 16 x 16 x 32 fragments: lane -> row l % 16, 16-byte chunk 4 s + (l / 16) of the 128-byte k-row (s = k32-step)
        o += [isa.vop("v_and_b32", ql, I32(15), LANE), isa.vop("v_lshrrev_b32", g, I32(4), LANE)]
        # fragment read addresses: row r (128 B), chunk (4 s + g) ^ ((r >> 1) & 7); x rows 128 wm + 16 mb + ql, W rows 128 wn + ...
        o += [isa.vop("v_lshrrev_b32", t[3], I32(1), ql), isa.vop("v_and_b32", t[3], I32(7), t[3]), isa.vop("v_lshlrev_b32", t[4], I32(7), ql),
              isa.vop("v_lshlrev_b32", t[5], I32(14), S_WM), isa.vop("v_add_u32", t[5], t[5], t[4]),                     # x: wm * 128 rows * 128 B
              isa.vop("v_lshlrev_b32", t[6], I32(14), S_WN), isa.vop("v_add_u32", t[6], t[6], t[4]),
              isa.vop("v_add_u32", t[6], I32(32768), t[6])]
        for ks in range(2):
            o += [isa.vop("v_or_b32", t[7], I32(4 * ks), g), isa.vop("v_xor_b32", t[7], t[7], t[3]),
                  isa.vop("v_lshl_add_u32", XADDR[0][ks], t[7], I32(4), t[5]), isa.vop("v_lshl_add_u32", WADDR[0][ks], t[7], I32(4), t[6]),
                  isa.vop("v_add_u32", XADDR[1][ks], I32(65536), XADDR[0][ks]), isa.vop("v_add_u32", WADDR[1][ks], I32(65536), WADDR[0][ks])]
        # source offsets: piece i of this wave = tile rows 64 w + 8 i + (lane >> 3), 16-byte chunk lane & 7 of the 128-byte k-row.
        # LDS image: row r, chunk c lives at chunk position c ^ ((r >> 1) & 7).  LDS-DMA writes lane-linearly, so the SOURCE chunk is permuted
        mlast = ST[9]
        o += [isa.sop("s_sub_u32", mlast, S_M, S_M0T), isa.sop("s_sub_u32", mlast, mlast, I32(1)),         # last valid x row of the tile
              isa.vop("v_lshrrev_b32", t[3], I32(3), LANE), isa.vop("v_and_b32", t[4], I32(7), LANE),
              isa.vop("v_lshlrev_b32", t[5], I32(6), S_WAVE)]
        for i in range(8):
            o += [isa.vop("v_add_u32", t[6], I32(8 * i), t[3]), isa.vop("v_add_u32", t[6], t[6], t[5]),           # row in tile
                  isa.vop("v_lshrrev_b32", t[7], I32(1), t[6]), isa.vop("v_and_b32", t[7], I32(7), t[7]), isa.vop("v_xor_b32", t[7], t[4], t[7]),
                  isa.vop("v_min_u32", t[8], t[6], mlast), isa.vop("v_mul_lo_u32", t[8], t[8], ldab),
                  isa.vop("v_lshl_add_u32", t[8], t[7], I32(4), t[8]), isa.vop("v_subrev_u32", XDMA[i], I32(1024 * (i & 3)), t[8]),
                  isa.vop("v_mul_lo_u32", t[9], t[6], kb2), isa.vop("v_lshl_add_u32", t[9], t[7], I32(4), t[9]),
                  isa.vop("v_subrev_u32", WDMA[i], I32(1024 * (i & 3)), t[9])]
        # pipeline fill: tiles 0 and 1 in LDS, first fragments of tile 0; the 32 LDS-DMA pieces go out first and the 256 accumulator
        # clears run under their latency
        o += self.dma_tile(0, 0, 0) + self.dma_tile(1, 0, 0) + [isa.vop("v_accvgpr_write_b32", A(i), I32(0)) for i in range(256)]
        o += [isa.waitcnt(vmcnt=0), isa.barrier()]
        o = sched.pad_hazards(sched.insert_lgkm_waits(o))
        return o + self.first_reads()          # the reads stay in flight into the first body (see loop())

    N_CARRY = 16           # fragment reads a body leaves in flight for its successor

    def first_reads(self) -> List[Instr]:
        """The first fragment reads of tile 0 (slot 0), issued by the prologue in the SAME order in which a loop body leaves the next
        tile's first reads in flight, so that the counted LDS waits at the top of a body are right on both ways into it."""
        if "lds" in self.cfg.abl.split(","):
            return []
        tail: List[Instr] = []
        sched.insert_lgkm_waits(self.body(1), carry_in=[], carry_out=tail)
        order = [tuple(i.writes()) for i in tail[-self.N_CARRY:]]
        reads = {tuple(i.writes()): i for i in self.frag_reads16(0, 0, 0, 0)}
        assert sorted(order) == sorted(reads), "the last LDS operations of a body must be the next tile's first fragment reads"
        return [reads[k] for k in order]

    def loop(self) -> List[Instr]:
        """The k-loop, two bodies (slot 0 / slot 1).  The first fragments of tile t+1 are read at the end of body t and consumed
        at the start of body t+1: the counted LDS waits of a body start from the reads its predecessor left in flight."""
        sig = lambda q: [tuple(i.writes()) for i in q]
        first = self.first_reads()
        c0: List[Instr] = []
        c1: List[Instr] = []
        # (LDS operations retire in order: as long as the reads are the youngest operations in flight when a body ends, the
        # counts that wait for them do not depend on what older operations are still queued before them)
        b0 = sched.insert_lgkm_waits(self.body(0), carry_in=first, carry_out=c0)
        b1 = sched.insert_lgkm_waits(self.body(1), carry_in=first, carry_out=c1)
        if "lds" not in self.cfg.abl.split(","):
            n = self.N_CARRY
            assert sig(c0[-n:]) == sig(first) and sig(c1[-n:]) == sig(first), "a body must end with the next tile's first fragment reads in flight"
        o: List[Instr] = [isa.label("L_loop_w0")]
        o += b0
        o += [isa.sop("s_add_u32", S_T, S_T, I32(1)), isa.sop("s_cmp_lt_u32", None, S_T, S_KT), isa.branch("s_cbranch_scc0", "L_done")]
        o += b1
        o += [isa.sop("s_add_u32", S_T, S_T, I32(1)), isa.sop("s_cmp_lt_u32", None, S_T, S_KT), isa.branch("s_cbranch_scc1", "L_loop_w0")]
        o += [isa.label("L_done"), isa.waitcnt(vmcnt=0), isa.waitcnt(lgkmcnt=0), isa.nop(15), isa.nop(15)]
        return o

    # ---------------------------------------------------------------------------------------------
    STG_ROW = 272          # bytes per staged row: 256 + 16 (conflict-free 8-byte writes of 16 rows, 16-byte aligned chunks)
    STG_WAVE = 16 * 272    # staging: 4 x 4352 bytes behind the two k-tile slots

    def epilogue(self) -> List[Instr]:
        """Whole-line epilogue.  Accumulator layout: lane (v = l % 16, g = l / 16) owns row 16 mb + v, columns 16 nb + 4 g .. + 3 of the
        wave's 128 x 128 block; memory layout of a row block: chunk j = 64 i + l (i = 0..3) = row j / 16, 16-byte chunk j % 16 of the row's 256 bytes.
        Per row block: [residual rows: 4 whole-line loads -> LDS -> 8 pairs in accumulator layout] -> bias / GELU / gate / residual in fp32 ->
        packed pairs -> LDS -> 4 quads in memory layout -> 4 whole-line stores.  Loads of block mb + 1 are requested before block mb is waited
        for (counted vmcnt: vector-memory operations retire in issue order; the stores of block mb - 1 are never waited for)."""
        c = self.cfg
        e: List[Instr] = []
        ql, g, t = T_[1], T_[2], T_
        n_mb = 8
        BQ = lambda nb: V(nb * 4, 4)
        LQ = lambda par, i: V(32 + 16 * par + 4 * i, 4)        # residual row block in memory layout, two in flight
        RB = lambda nb: V(64 + 2 * nb, 2)                       # ... back in accumulator layout
        OUTP = lambda nb: V(80 + 2 * nb, 2)                     # packed outputs, accumulator layout
        GQ = lambda par, nb: V(96 + 32 * par + 4 * nb, 4)       # gate quads, two row blocks in flight
        RQ = lambda i: V(202 + 4 * i, 4)                        # output row block in memory layout
        ROW = [V(164), V(197)]                                  # accumulator-layout row of the lane, by block parity (gate batch index, e3)
        GOFF = [V(165), V(198)]
        TB = V(166)
        E_W = V(236)
        E_R = [V(237 + i) for i in range(4)]
        E_Y = [V(241 + i) for i in range(4)]
        E_Z = [V(245 + i) for i in range(4)]
        E_M = [V(249 + i) for i in range(4)]                    # memory-layout row of the lane's chunk (row mask), advanced per block
        nw = ST[4]            # n0 + 128 wn (first column of the wave)
        e += [isa.sop("s_lshl_b32", nw, S_WN, I32(7)), isa.sop("s_add_u32", nw, nw, S_N0T)]
        e += self.addr64_madd(S_Y, nw, I32(1), 1)
        for i in range(32):
            e.append(isa.vop("v_mov_b32", V(i), I32(0)))
        e += [isa.sop("s_cmp_eq_u64", None, S_BIAS, I32(0)), isa.branch("s_cbranch_scc1", "L_nobias")]
        e += self.addr64_madd(S_BIAS, nw, I32(1), 2)
        e += [isa.vop("v_lshlrev_b32", t[3], I32(4), g)]                       # 4 g floats = 16 g bytes
        for nb in range(8):
            e.append(isa.global_load(4, BQ(nb), t[3], nb * 64, saddr=S_BIAS))
        e += [isa.label("L_nobias")]
        mw = ST[5]
        e += [isa.sop("s_lshl_b32", mw, S_WM, I32(7)), isa.sop("s_add_u32", mw, mw, S_M0T)]
        ldcb, ldrb = ST[6], ST[7]
        e += [isa.sop("s_lshl_b32", ldcb, S_LDC.sub(0), I32(1))]
        RCP, KC0, KC1 = V(161), V(162), V(163)
        if c.epi in (3, 4):
            e += self.addr64_madd(S_RES, nw, I32(1), 1)
            e += [isa.sop("s_lshl_b32", ldrb, S_LDR.sub(0), I32(1))]
        if c.epi == 3:
            e += self.addr64_madd(S_GATE, nw, I32(1), 2)
            e += [isa.vop("v_cvt_f32_u32", RCP, S_RPB), isa.vop("v_rcp_f32", RCP, RCP),
                  isa.sop("s_cmp_eq_u32", None, S_RPB, I32(0)), isa.sop("s_cselect_b32", ST[9], I32(0), I32(0xFFFFFFFF)),
                  isa.sop("s_lshl_b32", ST[12], S_GS.sub(0), I32(2))]
        if c.epi == 1:
            K0, K1 = 0.7978845608028654, 0.044715
            sc = 2.0 * 1.4426950408889634
            e += [isa.vop("v_mov_b32", KC0, F32(K0 * sc)), isa.vop("v_mov_b32", KC1, F32(K0 * K1 * sc))]
        # staging addresses and the lane's place in the memory layout
        sb = ST[8]
        e += [isa.sop("s_mul_i32", sb, S_WAVE, I32(self.STG_WAVE)), isa.sop("s_add_u32", sb, sb, I32(131072)),
              isa.vop("v_mul_u32_u24", t[4], I32(self.STG_ROW), ql), isa.vop("v_lshl_add_u32", t[4], g, I32(3), t[4]), isa.vop("v_add_u32", E_W, sb, t[4]),
              isa.vop("v_lshlrev_b32", t[5], I32(4), ql)]                                     # chunk l % 16 -> 16 (l % 16) bytes
        for i in range(4):
            e += [isa.vop("v_add_u32", t[4], I32(4 * i), g),                                  # row of the block: 4 i + l / 16
                  isa.vop("v_add_u32", E_M[i], mw, t[4]),
                  isa.vop("v_mul_u32_u24", t[6], I32(self.STG_ROW), t[4]), isa.vop("v_add_u32", t[6], t[6], t[5]), isa.vop("v_add_u32", E_R[i], sb, t[6]),
                  isa.vop("v_mul_lo_u32", t[6], E_M[i], ldcb), isa.vop("v_add_u32", E_Y[i], t[6], t[5])]
            if c.epi in (3, 4):
                e += [isa.vop("v_mul_lo_u32", t[6], E_M[i], ldrb), isa.vop("v_add_u32", E_Z[i], t[6], t[5])]
        step_y, step_z = ST[10], ST[11]
        e += [isa.sop("s_lshl_b32", step_y, ldcb, I32(4)), isa.sop("s_lshl_b32", step_z, ldrb, I32(4))]          # 16 rows on

        def masked(i, ins_list):
            return ([isa.v_cmp("v_cmp_lt_u32", E_M[i], S_M),
                     Instr("s_and_saveexec_b64", [S_SAVE], [VCC], extra_reads=[EXEC], extra_writes=[EXEC, isa.SCC], cls=isa.SALU)] + ins_list +
                    [Instr("s_mov_b64", [EXEC], [S_SAVE], cls=isa.SALU)])

        def loads(mb):
            """residual rows (memory layout; E_M / E_Z point at block mb) and the gate quads of the lane's row (accumulator layout)."""
            o_ = []
            for i in range(4):
                o_ += masked(i, [isa.global_load(4, LQ(mb & 1, i), E_Z[i], 0, saddr=S_RES, extra_reads=[EXEC])])
            if c.epi == 3:
                row, goff = ROW[mb & 1], GOFF[mb & 1]
                o_ += [isa.vop("v_add_u32", row, mw, ql)] + ([isa.vop("v_add_u32", row, I32(16 * mb), row)] if mb else [])
                # batch index of the row: floor((m + 0.5) / rows_per_batch); rows_per_batch == 0 -> 0
                o_ += [isa.vop("v_cvt_f32_u32", TB, row), isa.vop("v_add_f32", TB, F32(0.5), TB), isa.vop("v_mul_f32", TB, TB, RCP),
                       isa.vop("v_cvt_u32_f32", TB, TB), isa.vop("v_and_b32", TB, ST[9], TB),
                       isa.vop("v_mul_lo_u32", goff, TB, ST[12]), isa.vop("v_lshl_add_u32", goff, g, I32(4), goff),
                       isa.v_cmp("v_cmp_lt_u32", row, S_M),
                       Instr("s_and_saveexec_b64", [S_SAVE], [VCC], extra_reads=[EXEC], extra_writes=[EXEC, isa.SCC], cls=isa.SALU)]
                for nb in range(8):
                    o_.append(isa.global_load(4, GQ(mb & 1, nb), goff, nb * 64, saddr=S_GATE, extra_reads=[EXEC]))
                o_ += [Instr("s_mov_b64", [EXEC], [S_SAVE], cls=isa.SALU)]
            return o_

        def advance_z():
            return [isa.vop("v_add_u32", E_Z[i], step_z, E_Z[i]) for i in range(4)]

        n_loads = {0: 0, 1: 0, 4: 4, 3: 12}[c.epi]
        # E_M / E_Y follow the block being STORED, E_Z the block being LOADED (one ahead); the load masks of block mb + 1 use E_M + 16
        if n_loads:
            e += loads(0) + advance_z()
        e.append(isa.waitcnt(vmcnt=n_loads))             # the bias quads (older than the first block's loads)
        for mb in range(n_mb):
            if n_loads:
                if mb + 1 < n_mb:
                    # block mb + 1's loads: rows 16 further (E_M is advanced after block mb's stores: mask with a temporary)
                    for i in range(4):
                        e.append(isa.vop("v_add_u32", E_M[i], I32(16), E_M[i]))
                    e += loads(mb + 1) + advance_z()
                    for i in range(4):
                        e.append(isa.vop("v_subrev_u32", E_M[i], I32(16), E_M[i]))
                # behind the loads of block mb: the stores of block mb - 1 (4) and the loads of block mb + 1
                n_after = (4 if mb >= 1 else 0) + (n_loads if mb + 1 < n_mb else 0)
                e.append(isa.waitcnt(vmcnt=n_after))
                e += [isa.ds_write(16, E_R[i], LQ(mb & 1, i)) for i in range(4)]
                e += [isa.ds_read(8, RB(nb), E_W, 32 * nb) for nb in range(8)]
            for nb in range(8):
                base = 170 + 16 * (nb % 2)         # two rotating register groups
                f = [V(base + i) for i in range(4)]
                r_, u2 = V(base + 8), [V(base + 9), V(base + 10)]
                acc = ACC16(nb, mb)
                for i in range(4):
                    e += [isa.vop("v_accvgpr_read_b32", f[i], acc.sub(i)), isa.vop("v_add_f32", f[i], f[i], BQ(nb).sub(i))]
                if c.epi == 1:
                    for i in range(4):           # gelu_tanh(v) = v - v / (exp2(2 log2e k0 (v + k1 v^3)) + 1)
                        u = u2[i & 1]
                        e += [isa.vop("v_mul_f32", u, f[i], f[i]), isa.vop("v_fma_f32", u, u, KC1, KC0),
                              isa.vop("v_mul_f32", u, u, f[i]), isa.vop("v_exp_f32", u, u), isa.vop("v_add_f32", u, F32(1.0), u),
                              isa.vop("v_rcp_f32", u, u), isa.vop("v_fma_f32", f[i], Neg(f[i]), u, f[i])]
                if c.epi in (3, 4):
                    if c.epi == 3:
                        for i in range(4):
                            e.append(isa.vop("v_mul_f32", f[i], f[i], GQ(mb & 1, nb).sub(i)))
                    for i in range(4):           # + residual (bf16 pairs: low half << 16, high half & 0xffff0000)
                        src = RB(nb).sub(i >> 1)
                        e += [isa.vop("v_lshlrev_b32", r_, I32(16), src) if (i & 1) == 0 else isa.vop("v_and_b32", r_, I32(0xFFFF0000), src),
                              isa.vop("v_add_f32", f[i], f[i], r_)]
                e += [isa.vop("v_cvt_pk_bf16_f32", OUTP(nb).sub(0), f[0], f[1]), isa.vop("v_cvt_pk_bf16_f32", OUTP(nb).sub(1), f[2], f[3])]
            e += [isa.ds_write(8, E_W, OUTP(nb), 32 * nb) for nb in range(8)]
            e += [isa.ds_read_b128(RQ(i), E_R[i]) for i in range(4)]
            for i in range(4):
                e += masked(i, [isa.global_store(4, E_Y[i], RQ(i), 0, saddr=S_Y, extra_reads=[EXEC])])
            if mb + 1 < n_mb:
                for i in range(4):
                    e += [isa.vop("v_add_u32", E_M[i], I32(16), E_M[i]), isa.vop("v_add_u32", E_Y[i], step_y, E_Y[i])]
        e += [isa.label("L_exit"), Instr("s_endpgm", cls=isa.BRANCH)]       # (stores may still be in flight: the hardware drains them)
        return sched.pad_hazards(sched.insert_lgkm_waits(e))

    def program(self) -> List[Instr]:
        prog = self.prologue() + self.loop() + self.epilogue()
        pre = f"L_{self.cfg.name}"                     # labels are per kernel (several kernels share one .s file)
        for i in prog:
            if i.label and i.label.startswith("L_"):
                i.label = pre + i.label[1:]
        return prog


HEAD = """// GENERATED by scail_amd/asmgen/gemm4.py -- do not edit; regenerate with `python -m scail_amd.asmgen.gemm4`.
// Hand-scheduled 4-wave bf16 GEMM for gfx950 (256 x 256 x 64 tile, accumulators in a[0:255]); see the generator's docstring.
"""


def kernel(c: Cfg) -> codeobj.Kernel:
    return codeobj.Kernel(c.name, f"epilogue {c.epi}, <= {c.cap} fillers per MFMA gap", isa.render(Gen(c).program()),
                          lds_bytes=131072 + 4 * Gen.STG_WAVE, kernarg_size=KERNARG_SIZE)


def assembly(cfgs) -> str:
    return codeobj.assembly(HEAD, map(kernel, cfgs))


# the shipped kernels, one per epilogue.  The epilogue through LDS measured +3.1 % qkv, +6.6 % out-projection, +3.5 / +5.2 % cross q / out,
# +0.3 % MLP up (GELU: VALU-bound), +2.8 % MLP down over partial-line stores, bit-identical (profiles/r03_gemm_staged_epilogue_ab.log)
DEFAULTS = [Cfg(epi=e, name=f"scail_gemm4_e{e}") for e in (0, 1, 3, 4)]

# timing ablations of the shipped schedule (wrong results on purpose): what each instruction class of the k-loop costs beside the MFMAs
ABLATIONS = ("dma", "lds", "bar", "dma,lds", "dma,lds,bar")


def variant_cfgs():
    """the measurement build's additions to DEFAULTS (tools/probes/microbench.py times them)"""
    return [Cfg(epi=0, abl=abl, name="scail_gemm4_e0_s_abl_" + abl.replace(",", "_")) for abl in ABLATIONS]


if __name__ == "__main__":
    codeobj.main("gemm4")
