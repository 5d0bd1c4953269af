#!/usr/bin/env python3
"""Generator of the hand-scheduled gfx950 assembly of the fp32 ConvTranspose2d(kernel 2, stride 2) forward kernel.

Emits `mgu_convt_x3_gfx950`: the forward form (MODE 0, NI = 2) of convt2x2_x3_kernel (csrc/convt_x3.hip; unet_decoder.py:25,36) with
the same data layout and the same arithmetic in the same ORDER -- operands split by truncation into 8 + 8 + 8 mantissa bits, K walked
in ascending 16-channel half steps, per half step and accumulator the six products a2 b0, a0 b2, a1 b1, a1 b0, a0 b1, a0 b0, fp32
accumulation from zero, + shift[n] once at the store -- so the results are bitwise equal to the C++ kernel's.  What is fixed by hand:

  * 240 VGPRs per wave, two workgroups of four waves per CU, no scratch: 64 accumulators | 2 x 24 weight pieces | 2 x 24 operand
    pieces (both half steps of a K = 32 step) | 2 x 16 raw fp32 operands | 24 split pieces on their way to LDS | 4 split temporaries |
    13 lane constants | 7 temporaries of the cold code;
  * a half step is 24 MFMAs; everything else rides in the gaps behind them, at most three VALU operations and two ds_read_b128 per
    gap: the operand pieces of a half step are read from LDS one half step ahead, the weight pieces are requested one half step
    ahead, the raw rows one K = 32 step ahead (vmcnt retires in order, so a row load cannot stay in flight longer than the weight
    pieces requested behind it by more than a half step), and the three-way split of a step (88 VALU, 12 ds_write_b64) is spread
    over the 36 gaps of two half steps -- rows 64..127 of step s + 1 in the first half of step s, rows 0..63 of step s + 2 in its
    second half;
  * ONE barrier per K = 32 step, in the middle of it: it publishes step s + 1 (the other LDS buffer) and frees the buffer of step
    s, whose last reads were issued a half step earlier; the MFMAs behind it find their operands already in registers;
  * every s_waitcnt is counted: vmcnt(4) in front of a step (only the four row loads of the previous half step are younger than
    the weight pieces it needs), vmcnt(0) in front of its second half;
  * the K index of every load is clamped on the scalar unit (s_min_u32), the rows ride on the buffer descriptors' range checks
    (which count the scalar offset: every descriptor ends where the last byte a workgroup may touch ends).

Applicability (the host checks, csrc/convt_x3.hip: convt_x3_asm_shape): M % 128 == 0, Cin % 32 == 0, 4 Cout % 128 == 0, Hout == 2 H,
Wout == 2 W, pitches and channel offsets % 4 == 0, a tile's rows within 2^31 bytes.  With Hout == 2 H and Wout == 2 W the output pixel
(2y, 2x) of input pixel m = (img, y, x) is 4 m - 2 x: one division per row instead of two.

Layout of this file: the register map; the instruction lists of a step (loads, reads, split, mfmas) and emit_half, which interleaves
them; the prologue; the epilogue; generate().  Stream, kernel descriptor, metadata and the division / descriptor helpers are asmkit.py.

Usage: gen_convt_x3.py OUT.s
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # asmkit is a sibling: found also when this file is loaded by its path
from asmkit import Stream, vr, divmod_magic, desc_base, desc_mask   # noqa: E402

NAME = "mgu_convt_x3_gfx950"

# ---------------------------------------------------------------------------------------------------------------------
# register map
# ---------------------------------------------------------------------------------------------------------------------
def ACC(mi, ni): return (mi * 2 + ni) * 16
def BR(buf, f): return 64 + (buf * 6 + f) * 4                 # f = ni * 3 + piece: the wave's six fragments of a half step
def PA(ss, mi, q): return 112 + ((ss * 2 + mi) * 3 + q) * 4   # operand piece q of m tile mi, half step ss of the K = 32 step
def AREG(st, j): return 160 + (st * 4 + j) * 4                # raw rows j * 32 + arow of the step in register set st
def PCS(j, q): return 192 + (j * 3 + q) * 2                   # the pair of dwords of piece q on its way to LDS
TB = 216                                                      # v216..v219: the truncated values of a split stage
VMASK, VST, VRD, VLANE16 = 220, 221, 222, 223
VAOFF = [224, 225, 226, 227]
VSH = [228, 229]
VTID, VROW, VLR4 = 230, 231, 232
VT = [233, 234, 235, 236, 237, 238, 239]
def VOFF(mi, g): return AREG(0, 0) + (mi * 4 + g) * 4         # epilogue: byte offsets of the lane's 32 output rows (the raw registers)

# SGPRs: s[0:1] kernarg pointer, s2 workgroup id, s[4:25] the argument block (csrc/convt_x3.hip: ConvtAsmArgs)
S_IN, S_WX, S_OUT, S_SHIFT = 4, 6, 8, 10
S_W, S_LDIN, S_LDOUT, S_CIN, S_COUT, S_NK, S_NTN, S_NBLOCKS, S_PERXCD, S_WOUT, S_MGNTN, S_MGW, S_MGCOUT, S_PAD = range(12, 26)
S_T = [26, 27, 28, 29, 30, 31, 32, 33]
S_NT, S_MT, S_BM0, S_X0, S_WI, S_WM, S_WN = 34, 35, 36, 37, 38, 39, 40
S_KK, S_NKK1, S_NK1 = 41, 42, 43      # half steps requested so far; 2 nk - 1; nk - 1
S_INR, S_BRD, S_OUTR, S_SHR = 44, 48, 52, 56   # descriptors
S_PERM, S_AK, S_BK, S_BK3 = 60, 61, 62, 63
S_NC = [64, 65]                       # byte offset of n tile ni's first column inside an output pixel quad
S_S, S_LDOUT4, S_LDIN4 = 66, 67, 68
S_N04 = [69, 70]                      # (first column of n tile ni) * 4

ABUF = 3 * 128 * 80                   # bytes of one LDS buffer: [3 pieces][128 rows][32 k + 8 pad] bf16
ROWTAB = 2 * ABUF                     # 128 row offsets (bytes) behind the two buffers
LDS_BYTES, VGPRS, SGPRS, THREADS, KERNARG = ROWTAB + 512, 240, 72, 256, 88
PRODUCTS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))   # (operand piece, weight piece): smallest terms first


class Kernel:
    def __init__(self, o):
        self.o, self.E, self.L, self.newlabel = o, o.E, o.L, o.newlabel
        self.end = f".Lend_{NAME}"


def emit(kn, ops):
    for x in ops:
        kn.E(x)


# ---------------------------------------------------------------------------------------------------------------------
# instruction lists of a step
# ---------------------------------------------------------------------------------------------------------------------
def b_loads(buf):
    """the wave's six weight fragments of the half step whose byte offset is in S_BK (S_BK3: + three fragments)"""
    return [f"buffer_load_dwordx4 {vr(BR(buf, f), 4)}, v{VLANE16}, s[{S_BRD}:{S_BRD + 3}], s{S_BK3 if f >= 3 else S_BK} offen offset:{(f % 3) * 1024}"
            for f in range(6)]


def b_advance():
    """S_BK = min(++kk, 2 nk - 1) * 12288: a half step past the end re-reads the last one (never used)"""
    return [f"s_add_u32 s{S_KK}, s{S_KK}, 1", f"s_min_u32 s{S_T[0]}, s{S_KK}, s{S_NKK1}", f"s_mul_i32 s{S_BK}, s{S_T[0]}, 0x3000",
            f"s_add_u32 s{S_BK3}, s{S_BK}, 0xc00"]


def a_loads(st):
    """the thread's four 16-byte row pieces of the step whose byte offset is in S_AK"""
    return [f"buffer_load_dwordx4 {vr(AREG(st, j), 4)}, v{VAOFF[j]}, s[{S_INR}:{S_INR + 3}], s{S_AK} offen" for j in range(4)]


def a_offset(ahead):
    """S_AK = min(s + ahead, nk - 1) * 128"""
    return [f"s_add_u32 s{S_T[1]}, s{S_S}, {ahead}", f"s_min_u32 s{S_T[1]}, s{S_T[1]}, s{S_NK1}", f"s_lshl_b32 s{S_AK}, s{S_T[1]}, 7"]


def pa_reads(buf, ss):
    return [f"ds_read_b128 {vr(PA(ss, mi, q), 4)}, v{VRD} offset:{buf * ABUF + (q * 128 + mi * 32) * 80 + ss * 32}"
            for mi in range(2) for q in range(3)]


def split_ops(st, j, buf):
    """split3_pack of the four values of row piece j and their way to LDS buffer buf: 22 VALU, 3 ds_write_b64"""
    a = AREG(st, j)
    r = []
    for q in range(3):
        for p in range(2):
            r.append(f"v_perm_b32 v{PCS(j, q) + p}, v{a + 2 * p + 1}, v{a + 2 * p}, s{S_PERM}")
        r.append(f"ds_write_b64 v{VST}, {vr(PCS(j, q), 2)} offset:{buf * ABUF + (q * 128 + j * 32) * 80}")
        if q < 2:
            for e in range(4):
                r.append(f"v_and_b32_e32 v{TB + e}, v{VMASK}, v{a + e}")
            for e in range(4):
                r.append(f"v_sub_f32_e32 v{a + e}, v{a + e}, v{TB + e}")
    assert len(r) == 25
    return r


def mfmas(ss):
    """the 24 MFMAs of half step ss: per accumulator the six products in the C++ kernel's order"""
    r = []
    for mi in range(2):
        for ni in range(2):
            acc = vr(ACC(mi, ni), 16)
            for (pa, pb) in PRODUCTS:
                r.append(f"v_mfma_f32_32x32x16_bf16 {acc}, {vr(PA(ss, mi, pa), 4)}, {vr(BR(ss, ni * 3 + pb), 4)}, {acc}")
    return r


SPLIT_GAPS = (3, 20)      # the split of a half step rides in these gaps: its last LDS store is three MFMAs old at the barrier


def emit_half(kn, ss, first, spread):
    """24 MFMAs; first[g]: what is issued right behind MFMA g (loads, reads, scalar bookkeeping); spread: the split, at most three
    operations per gap over SPLIT_GAPS"""
    g0, g1 = SPLIT_GAPS
    per = -(-len(spread) // (g1 - g0 + 1))
    assert per <= 3
    spread = list(spread)
    for g, m in enumerate(mfmas(ss)):
        kn.E(m)
        emit(kn, first.get(g, []))
        if g0 <= g <= g1:
            emit(kn, spread[:per])
            del spread[:per]
    assert not spread


def emit_step(kn, p):
    """K = 32 step s of parity p.  On entry: LDS buffer p holds step s, its half-0 pieces are on their way to PA(0); buffer p ^ 1
    holds rows 0..63 of step s + 1; register set p ^ 1 holds step s + 1, set p receives step s + 2 (the four youngest loads); BR(0)
    was requested before those."""
    rd = pa_reads(p, 1)
    first = {g: [x] for g, x in enumerate(b_loads(1))}
    first[0] = b_advance() + first[0]
    for g in range(3):
        first[g] = first[g] + rd[2 * g:2 * g + 2]
    kn.E("s_waitcnt vmcnt(4) lgkmcnt(0)")
    emit_half(kn, 0, first, split_ops(p ^ 1, 2, p ^ 1) + split_ops(p ^ 1, 3, p ^ 1))
    # step s + 1 is complete in buffer p ^ 1 and nobody reads buffer p any more; BR(1) has landed
    kn.E("s_waitcnt vmcnt(0) lgkmcnt(0)")
    kn.E("s_barrier")
    rd = pa_reads(p ^ 1, 0)
    first = {g: [x] for g, x in enumerate(b_loads(0))}
    first[0] = b_advance() + first[0]
    for g in range(3):
        first[g] = first[g] + rd[2 * g:2 * g + 2]
    first[5] = first[5] + a_offset(3)
    for j, x in enumerate(a_loads(p ^ 1)):
        first[6 + j] = [x]
    emit_half(kn, 1, first, split_ops(p, 0, p) + split_ops(p, 1, p))


# ---------------------------------------------------------------------------------------------------------------------
# prologue
# ---------------------------------------------------------------------------------------------------------------------
def emit_prologue(kn):
    E, t = kn.E, S_T
    E("s_load_dwordx16 s[4:19], s[0:1], 0x0")
    E("s_load_dwordx4 s[20:23], s[0:1], 0x40")
    E("s_load_dwordx2 s[24:25], s[0:1], 0x50")
    E(f"v_mov_b32_e32 v{VTID}, v0")
    E("s_waitcnt lgkmcnt(0)")
    # logical block = (wg & 7) * per_xcd + (wg >> 3): all n tiles of a pixel tile on one XCD, back to back
    E(f"s_and_b32 s{t[0]}, s2, 7")
    E(f"s_mul_i32 s{t[0]}, s{t[0]}, s{S_PERXCD}")
    E(f"s_lshr_b32 s{t[1]}, s2, 3")
    E(f"s_add_u32 s{t[0]}, s{t[0]}, s{t[1]}")
    E(f"s_cmp_ge_u32 s{t[0]}, s{S_NBLOCKS}")
    E(f"s_cbranch_scc1 {kn.end}")                      # workgroup-uniform, before any barrier
    divmod_magic(kn, t[0], S_NTN, S_MGNTN, S_MT, S_NT, t[2], t[3])
    E(f"s_lshl_b32 s{S_BM0}, s{S_MT}, 7")
    divmod_magic(kn, S_BM0, S_W, S_MGW, t[4], S_X0, t[2], t[3])       # x of the tile's first pixel
    E(f"v_lshrrev_b32_e32 v{VT[0]}, 6, v{VTID}")
    E("s_nop 3")                                       # VALU write -> v_readfirstlane of the same register
    E(f"v_readfirstlane_b32 s{S_WI}, v{VT[0]}")
    E("s_nop 3")
    E(f"s_lshr_b32 s{S_WM}, s{S_WI}, 1")
    E(f"s_and_b32 s{S_WN}, s{S_WI}, 1")
    E(f"s_mov_b32 s{S_PERM}, 0x07060302")
    E(f"s_lshl_b32 s{S_LDIN4}, s{S_LDIN}, 2")
    E(f"s_lshl_b32 s{S_LDOUT4}, s{S_LDOUT}, 2")
    E(f"s_sub_u32 s{S_NK1}, s{S_NK}, 1")
    E(f"s_lshl_b32 s{t[4]}, s{S_NK}, 1")
    E(f"s_sub_u32 s{S_NKK1}, s{t[4]}, 1")
    # input descriptor: the tile's 128 rows, (127 * ldin + Cin) * 4 bytes from row bm0
    desc_base(kn, S_INR, S_IN, S_BM0, S_LDIN4, t[2], t[3])
    E(f"s_mul_i32 s{t[2]}, s{S_LDIN}, 0x7f")
    E(f"s_add_u32 s{t[2]}, s{t[2]}, s{S_CIN}")
    E(f"s_lshl_b32 s{S_INR + 2}, s{t[2]}, 2")
    E(f"s_mov_b32 s{S_INR + 3}, 0x00020000")
    # weight descriptor: the n tile's 2 nk half steps of 12 fragments, from the wave's first fragment (wn * 6)
    E(f"s_mul_i32 s{t[4]}, s{t[4]}, 0x3000")
    desc_base(kn, S_BRD, S_WX, S_NT, t[4], t[2], t[3], mask=False)
    E(f"s_mul_i32 s{t[5]}, s{S_WN}, 0x1800")
    E(f"s_add_u32 s{S_BRD}, s{S_BRD}, s{t[5]}")
    E(f"s_addc_u32 s{S_BRD + 1}, s{S_BRD + 1}, 0")
    desc_mask(kn, S_BRD)
    E(f"s_sub_u32 s{S_BRD + 2}, s{t[4]}, s{t[5]}")
    E(f"s_mov_b32 s{S_BRD + 3}, 0x00020000")
    # lane constants
    E(f"v_and_b32_e32 v{VT[0]}, 63, v{VTID}")              # lane
    E(f"v_lshlrev_b32_e32 v{VLANE16}, 4, v{VT[0]}")
    E(f"v_and_b32_e32 v{VT[1]}, 31, v{VT[0]}")             # lr
    E(f"v_lshrrev_b32_e32 v{VT[2]}, 5, v{VT[0]}")          # lh
    E(f"v_lshlrev_b32_e32 v{VLR4}, 2, v{VT[1]}")
    E(f"s_lshl_b32 s{t[2]}, s{S_WM}, 6")
    E(f"v_add_u32_e32 v{VT[3]}, s{t[2]}, v{VT[1]}")
    E(f"v_mul_u32_u24_e32 v{VT[3]}, 0x50, v{VT[3]}")
    E(f"v_lshl_add_u32 v{VRD}, v{VT[2]}, 4, v{VT[3]}")     # (wm * 64 + lr) * 80 + lh * 16
    E(f"s_lshl_b32 s{t[2]}, s{S_WM}, 8")
    E(f"v_lshlrev_b32_e32 v{VROW}, 4, v{VT[2]}")
    E(f"v_add_u32_e32 v{VROW}, s{t[2]}, v{VROW}")          # (wm * 64 + lh * 4) * 4
    E(f"v_lshrrev_b32_e32 v{VT[3]}, 3, v{VTID}")           # arow
    E(f"v_and_b32_e32 v{VT[4]}, 7, v{VTID}")               # 16-byte piece of the row's 128 bytes
    E(f"v_mul_u32_u24_e32 v{VST}, 0x50, v{VT[3]}")
    E(f"v_lshl_add_u32 v{VST}, v{VT[4]}, 3, v{VST}")       # arow * 80 + piece * 8
    for j in range(4):
        E(f"v_add_u32_e32 v{VT[5]}, {j * 32}, v{VT[3]}")
        E(f"v_mul_lo_u32 v{VT[5]}, v{VT[5]}, s{S_LDIN4}")
        E(f"v_lshl_add_u32 v{VAOFF[j]}, v{VT[4]}, 4, v{VT[5]}")
    E(f"v_mov_b32_e32 v{VMASK}, 0xffff0000")
    # n tile ni: columns n0 .. n0 + 31 = tap q, channels co0 .. of it (Cout % 32 == 0: one tap per n tile)
    E(f"s_lshl_b32 s{t[4]}, s{S_NT}, 7")
    E(f"s_lshl_b32 s{t[5]}, s{S_WN}, 6")
    E(f"s_add_u32 s{t[4]}, s{t[4]}, s{t[5]}")
    for ni in range(2):
        if ni:
            E(f"s_add_u32 s{t[4]}, s{t[4]}, 32")
        E(f"s_lshl_b32 s{S_N04[ni]}, s{t[4]}, 2")
        divmod_magic(kn, t[4], S_COUT, S_MGCOUT, t[5], t[6], t[3], t[7])
        E(f"s_lshr_b32 s{t[3]}, s{t[5]}, 1")
        E(f"s_mul_i32 s{t[3]}, s{t[3]}, s{S_WOUT}")
        E(f"s_and_b32 s{t[5]}, s{t[5]}, 1")
        E(f"s_add_u32 s{t[3]}, s{t[3]}, s{t[5]}")
        E(f"s_mul_i32 s{t[3]}, s{t[3]}, s{S_LDOUT}")
        E(f"s_add_u32 s{t[3]}, s{t[3]}, s{t[6]}")
        E(f"s_lshl_b32 s{S_NC[ni]}, s{t[3]}, 2")
    lnul = kn.newlabel("noshift")
    E(f"v_mov_b32_e32 v{VSH[0]}, 0")
    E(f"v_mov_b32_e32 v{VSH[1]}, 0")
    E(f"s_cmp_eq_u64 s[{S_SHIFT}:{S_SHIFT + 1}], 0")
    E(f"s_cbranch_scc1 {lnul}")
    E(f"s_mov_b32 s{S_SHR}, s{S_SHIFT}")
    desc_mask(kn, S_SHR, S_SHIFT)
    E(f"s_lshl_b32 s{S_SHR + 2}, s{S_COUT}, 4")            # 4 Cout values
    E(f"s_mov_b32 s{S_SHR + 3}, 0x00020000")
    for ni in range(2):
        E(f"buffer_load_dword v{VSH[ni]}, v{VLR4}, s[{S_SHR}:{S_SHR + 3}], s{S_N04[ni]} offen")
    kn.L(lnul)
    # the first requests: weight pieces of half step 0, rows of steps 0 and 1
    E(f"s_mov_b32 s{S_KK}, 0")
    E(f"s_mov_b32 s{S_S}, 0")
    E(f"s_mov_b32 s{S_BK}, 0")
    E(f"s_mov_b32 s{S_BK3}, 0xc00")
    E(f"s_mov_b32 s{S_AK}, 0")
    emit(kn, b_loads(0))
    emit(kn, a_loads(0))
    emit(kn, a_offset(1))
    emit(kn, a_loads(1))
    # under them: the row-offset table, the output descriptor, the cleared accumulators
    # row t of the tile is pixel m = bm0 + t, x = (x0 + t) % W; its output pixel lies 4 t - 2 (x - x0) pixels behind the tile's first
    E(f"v_and_b32_e32 v{VT[0]}, 0x7f, v{VTID}")            # both halves of the workgroup write the same 128 values
    E(f"v_add_u32_e32 v{VT[1]}, s{S_X0}, v{VT[0]}")
    E(f"v_mul_hi_u32 v{VT[2]}, v{VT[1]}, s{S_MGW}")
    E(f"v_mul_lo_u32 v{VT[2]}, v{VT[2]}, s{S_W}")
    E(f"v_sub_u32_e32 v{VT[1]}, v{VT[1]}, v{VT[2]}")
    E(f"v_subrev_u32_e32 v{VT[2]}, s{S_W}, v{VT[1]}")
    E(f"v_cmp_le_u32_e32 vcc, s{S_W}, v{VT[1]}")
    E("s_nop 1")
    E(f"v_cndmask_b32_e32 v{VT[1]}, v{VT[1]}, v{VT[2]}, vcc")      # x
    E(f"v_lshlrev_b32_e32 v{VT[2]}, 2, v{VT[0]}")
    E(f"v_lshlrev_b32_e32 v{VT[1]}, 1, v{VT[1]}")
    E(f"v_sub_u32_e32 v{VT[2]}, v{VT[2]}, v{VT[1]}")
    E(f"s_lshl_b32 s{t[2]}, s{S_X0}, 1")
    E(f"v_add_u32_e32 v{VT[2]}, s{t[2]}, v{VT[2]}")
    E(f"v_mul_lo_u32 v{VT[2]}, v{VT[2]}, s{S_LDOUT4}")
    E(f"v_lshlrev_b32_e32 v{VT[0]}, 2, v{VT[0]}")
    E(f"ds_write_b32 v{VT[0]}, v{VT[2]} offset:{ROWTAB}")
    # output descriptor: from the tile's first output pixel 4 bm0 - 2 x0 (the launcher added the channel offset) to the end of the
    # last row's last tap (one output row and one pixel further, Cout channels): the range check counts the scalar offset, which
    # carries a store's tap and channel
    E(f"s_lshl_b32 s{t[4]}, s{S_BM0}, 2")
    E(f"s_sub_u32 s{t[4]}, s{t[4]}, s{t[2]}")
    desc_base(kn, S_OUTR, S_OUT, t[4], S_LDOUT4, t[5], t[6])
    E(f"s_add_u32 s{t[4]}, s{S_X0}, 0x7f")
    divmod_magic(kn, t[4], S_W, S_MGW, t[5], t[6], t[3], t[7])      # x of row 127
    E(f"s_lshl_b32 s{t[6]}, s{t[6]}, 1")
    E(f"s_sub_u32 s{t[6]}, 0x1fc, s{t[6]}")
    E(f"s_add_u32 s{t[6]}, s{t[6]}, s{t[2]}")
    E(f"s_add_u32 s{t[6]}, s{t[6]}, s{S_WOUT}")
    E(f"s_add_u32 s{t[6]}, s{t[6]}, 1")
    E(f"s_mul_i32 s{t[6]}, s{t[6]}, s{S_LDOUT4}")
    E(f"s_lshl_b32 s{t[5]}, s{S_COUT}, 2")
    E(f"s_add_u32 s{S_OUTR + 2}, s{t[6]}, s{t[5]}")
    E(f"s_mov_b32 s{S_OUTR + 3}, 0x00020000")
    for r in range(64):
        E(f"v_mov_b32_e32 v{r}, 0")
    E("s_waitcnt vmcnt(4)")                 # rows of step 0 (the shift and the weight pieces are older)
    for j in range(4):
        emit(kn, split_ops(0, j, 0))
    E("s_waitcnt vmcnt(0)")
    for j in range(2):
        emit(kn, split_ops(1, j, 1))
    emit(kn, a_offset(2))
    emit(kn, a_loads(0))
    E("s_waitcnt lgkmcnt(0)")
    E("s_barrier")
    emit(kn, pa_reads(0, 0))


# ---------------------------------------------------------------------------------------------------------------------
# epilogue: C/D layout col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); 32 lanes store the 128 contiguous bytes
# of 32 output channels of one output pixel.  The stores of one accumulator tile go out while the next tile's + shift is formed.
# ---------------------------------------------------------------------------------------------------------------------
def emit_epilogue(kn):
    E = kn.E
    E("s_waitcnt vmcnt(0) lgkmcnt(0)")       # the loads past the last step land in the registers reused below
    for mi in range(2):
        for g in range(4):
            E(f"ds_read_b128 {vr(VOFF(mi, g), 4)}, v{VROW} offset:{ROWTAB + (mi * 32 + 8 * g) * 4}")
    E("s_waitcnt lgkmcnt(0)")
    for i in range(32):
        E(f"v_add_u32_e32 v{VOFF(0, 0) + i}, v{VLR4}, v{VOFF(0, 0) + i}")
    tiles = [(0, 0), (0, 1), (1, 0), (1, 1)]
    def add(mi, ni, r): return f"v_add_f32_e32 v{ACC(mi, ni) + r}, v{ACC(mi, ni) + r}, v{VSH[ni]}"
    def store(mi, ni, r):
        return f"buffer_store_dword v{ACC(mi, ni) + r}, v{VOFF(mi, r >> 2) + (r & 3)}, s[{S_OUTR}:{S_OUTR + 3}], s{S_NC[ni]} offen"
    # (the 41 instructions above are the wait states between the last MFMA and the first read of an accumulator: 18 needed)
    for r in range(16):
        E(add(*tiles[0], r))
    for k, tl in enumerate(tiles):
        for r in range(16):
            E(store(*tl, r))
            if k + 1 < len(tiles):
                E(add(*tiles[k + 1], r))


def generate():
    """the text of the code object"""
    o = Stream()
    kn = Kernel(o)
    o.begin_kernel(NAME)
    emit_prologue(kn)
    loop, epi = kn.newlabel("step"), kn.newlabel("store")
    # two steps per trip: the LDS buffer and the register set of a step are static
    kn.L(loop)
    emit_step(kn, 0)
    kn.E(f"s_add_u32 s{S_S}, s{S_S}, 1")
    kn.E(f"s_cmp_ge_u32 s{S_S}, s{S_NK}")
    kn.E(f"s_cbranch_scc1 {epi}")
    emit_step(kn, 1)
    kn.E(f"s_add_u32 s{S_S}, s{S_S}, 1")
    kn.E(f"s_cmp_lt_u32 s{S_S}, s{S_NK}")
    kn.E(f"s_cbranch_scc1 {loop}")
    kn.L(epi)
    emit_epilogue(kn)
    kn.L(kn.end)
    kn.E("s_endpgm")
    o.end_kernel(NAME, LDS_BYTES, VGPRS, SGPRS, KERNARG, THREADS)
    return o.text()


def main():
    ap = argparse.ArgumentParser(description="gfx950 assembly of the fp32 ConvTranspose forward kernel")
    ap.add_argument("out", metavar="OUT.s")
    args = ap.parse_args()
    with open(args.out, "w") as f:
        f.write(generate())


if __name__ == "__main__":
    main()
