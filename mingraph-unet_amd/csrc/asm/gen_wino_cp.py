#!/usr/bin/env python3
"""Generator of the hand-scheduled gfx950 assembly of the component-pair Winograd kernels.

Emits `mgu_wino_cp2_gfx950` (wide: 64 output channels per workgroup) and the narrow kernels `mgu_wino_cp1r2_gfx950`,
`mgu_wino_cp1r4_gfx950` and, as a code object of its own, the head-fused `mgu_wino_cp1r2h_gfx950`: the same algorithm, data layout
and arithmetic ORDER as wino3x3_cp_kernel<2, false, false, false> / <1, false, true, *>
(csrc/wino_f32.hip; the 3x3 convolutions of ConvBlock, model/unet/unet_encoder.py:15-25) -- results are bitwise equal to the
C++ kernel -- with the register map and the instruction order of the chunk loop fixed by hand:

  * 256 VGPRs per wave, no scratch: 128 accumulators | 48 weight pieces | 2 x 12 operand pieces | 32 raw operands |
    12 halo registers | 9 lane constants | 3 temporaries;
  * the steps of a chunk run in the order (jj, mi) = (0,0), (1,0), (0,1), (1,1): the two components of a pair share one tile
    column, and the jj = 1 step takes that column's inner sum from the raw registers of the jj = 0 step before it (raw_reads,
    form_valu) -- four LDS reads and four VALU per half fewer;
  * a step issues the LDS reads of the NEXT step's raw operands first, then its twelve MFMAs with the transform and the
    three-way split of those operands spread between them (nothing waits for a read it has just issued); the weight pieces of
    the next chunk are requested right behind the last MFMA that uses the register they land in;
  * every s_waitcnt is counted (vmcnt: halo loads, weight pieces and stores retire in order; lgkmcnt: LDS only, no scalar
    loads inside the loops);
  * out-of-image halo pixels ride on the buffer descriptor's range check (offset 0x7fff0000): no mask, no select.

Applicability (the launcher checks; everything else stays on the C++ kernel): inference epilogue (no statistics), H % 8 == 0,
W % 32 == 0, N % 64 == 0, Cp % 32 == 0, channel pitches and offsets % 4 == 0, scale and shift present, x-fastest patch order.

Layout of this file: the register map; the instruction lists of a step (raw_reads, form_valu, mfmas) and emit_step, the ONE
interleaver of both kernel widths (wide_step / narrow_step hand it their gap ranges, waits and per-gap extras); the pieces of the
patch epilogue, each written once, and the two drivers that order them (emit_epilogue_wide / emit_epilogue_narrow); the prologue;
generate(head), which returns the text of one code object and keeps no state behind.  What is not Winograd -- the output stream,
kernel descriptor and metadata, descriptor and division helpers, packed-fp32 forms -- is asmkit.py.

Usage: gen_wino_cp.py OUT.s            (the three plain kernels)
       gen_wino_cp.py --head OUT.s     (mgu_wino_cp1r2h_gfx950)
"""
import argparse
import os
import sys
from types import SimpleNamespace as Regs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # asmkit is a sibling: found also when this file is loaded by its path
from asmkit import Stream, vr, divmod_magic, desc_base, desc_mask, pk2, pkfma2   # noqa: E402

# ---------------------------------------------------------------------------------------------------------------------
# register map
# ---------------------------------------------------------------------------------------------------------------------
class Kernel:
    """The kernel being emitted: name; ntb: output-channel tiles per workgroup (2 wide, 1 narrow); nc: static chunk count (narrow
    kernels); head: the finishing pass also applies the 1x1 head and sums graph patches; the stream it goes to; and the part of
    the register map that depends on these."""
    def __init__(self, name, ntb, nc=None, head=False, o=None):
        self.name, self.ntb, self.nc, self.head, self.o = name, ntb, nc, head, o
        self.end = f".Lend_{name}"
        # 0xffff0000 in a VGPR and the wave's transform sign (+-1.0) in a VGPR: with all-VGPR VOP2 forms (v_fmac / v_add / v_sub /
        # v_and) two waves of a SIMD issue the transform + split at 2.4 cycles per instruction instead of 4
        # (tools/ubench/gen_issue_cost.py: mix2 vs mix)
        self.VMASK, self.VSGN = (254, 255) if ntb == 2 else (172, 173)
        if o is not None:
            self.E, self.L, self.newlabel = o.E, o.L, o.newlabel

    def ACC(self, jj, nt, mi): return ((jj * 2 + nt) * 2 + mi) * 16 if self.ntb == 2 else (jj * 2 + mi) * 16

WIDE = Kernel("mgu_wino_cp2_gfx950", 2)       # (no stream: the configuration alone, for the instruction lists below)
# narrow kernels (ntb = 1): the layer's whole weight-piece slice of the wave stays in registers, two halo register sets
def WN(c, jj, p): return 64 + ((c * 2 + jj) * 3 + p) * 4
def HSET(setn, i): return (232 if setn == 0 else 160) + i * 4
def BX(jj, nt, p): return 128 + ((jj * 2 + nt) * 3 + p) * 4
def PC(slot, p): return 176 + (slot * 3 + p) * 4
def RAW(hf, k): return 200 + (hf * 4 + k) * 4          # k: 0 = a(x), 1 = b(x), 2 = a(y), 3 = b(y)
VA, VB = 244, 245
VHST = [246, 247, 248]
VHOFF = [249, 250, 251]
VLANE16 = 252
VTID = 253
VT0, VT1 = 230, 231   # temporaries of the cold code (halo-offset setup, epilogue addressing): the last two registers of raw half 1,
                      # free at every point those run (narrow kernels: see emit_epilogue_narrow, which keeps its own temporaries clear of them)

# SGPRs
S_IN, S_WU, S_OUT, S_SCALE, S_SHIFT, S_POOL = 4, 6, 8, 10, 12, 14
S_H, S_W, S_LDIN, S_LDOUT, S_LDPOOL, S_NC, S_RELU, S_TX, S_TY, S_TOTAL, S_PPB, S_NGROUPS = 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27
S_NITEMS, S_PERXCD, S_MGNG, S_MGTX, S_MGTXTY, S_PAD = 28, 29, 30, 31, 32, 33
S_NBLOCK, S_PBEGIN, S_NPATCH, S_LC, S_LP, S_PI, S_C, S_LC64 = 34, 35, 36, 37, 38, 39, 40, 41
S_N64X4 = 42        # (nblock * 64) * 4: byte offset of the workgroup's first channel
S_SUMOFF = 43       # (W * ldout + ldout) * 4
S_INR = 44          # s[44:47] input descriptor
S_UR = 48           # s[48:51] weight-piece descriptor
S_SGN, S_W1, S_MASK, S_PERM, S_NTSTRIDE, S_TXTY, S_IMGB, S_OOB = 52, 53, 54, 55, 56, 57, 58, 59
S_T = [60, 61, 62, 63, 64, 65, 66, 67]
S_WI, S_JP = 68, 69
S_P, S_IMG, S_REM, S_PY, S_PX, S_Y0, S_X0 = 70, 71, 72, 73, 74, 75, 88
S_M = 76            # s[76:77]
S_WO = [[78, 79], [90, 91]]   # weight soffsets [jj][nt] of the chunk being requested
S_OUTR = 80         # s[80:83]
S_POOLR = 84        # s[84:87]
S_OUTIMGB = 89
S_SCR = 92          # s[92:95] scale descriptor
S_SHR = 96          # s[96:99] shift descriptor
S_LD4, S_SW4 = 100, 101

S1F, S2F, S3F = 17 * 20, 20, 17 * 20 + 20     # LDS offsets (floats) of tile columns 1..3
BUFX = 0x20000                                # byte distance of the two raw buffers (slots 0 and 4 of the LDS map)
RAWB = 8192 * 4                               # bytes of an LDS slot
ZBIAS = 57472

LDS_BYTES, VGPRS, SGPRS, THREADS = 163840, 256, 102, 512   # of every kernel here: kernel descriptor and metadata (emit_kernel)
KERNARG = 120       # bytes of the plain kernels' argument block (csrc/wino_asm.hip: WinoAsmArgs)


def patch_coords(kn, p):
    """s_p -> S_IMG, S_Y0, S_X0 (x fastest inside an image)"""
    divmod_magic(kn, p, S_TXTY, S_MGTXTY, S_IMG, S_REM, S_T[6], S_T[7])
    divmod_magic(kn, S_REM, S_TX, S_MGTX, S_PY, S_PX, S_T[6], S_T[7])
    kn.E(f"s_lshl_b32 s{S_Y0}, s{S_PY}, 3")
    kn.E(f"s_lshl_b32 s{S_X0}, s{S_PX}, 5")


# ---------------------------------------------------------------------------------------------------------------------
# head-fused form of the 2-chunk narrow kernel (mgu_wino_cp1r2h_gfx950).  Registers the 2-chunk kernel leaves free: v112..v159 (the
# weight pieces of chunks 2, 3 of the 4-chunk kernel); SGPRs that the narrow kernels need in the prologue only (weight descriptor,
# sign / mask constants, weight offsets) or for the fused pool, which this form does not have (the launcher passes no pool).
# ---------------------------------------------------------------------------------------------------------------------
def WQ(k, e): return 112 + k * 4 + e        # head weight of class k, channel e of the lane's channel quad (lane constant)
def BL(k): return 128 + k                   # bias of class k in the lanes of channel quad 0, 0 in the others (lane constant)
def DL(k, p): return 132 + k * 4 + p        # logit of class k, pixel p of the lane's 2 x 2 tile (p = 2 * row + column)
def SS(j): return 148 + j                   # store registers of a lane's output row: [column][class]
VLG, VPS, VBP16, VBP32 = 156, 157, 158, 159   # byte offsets of the lane's logit row / patch-sum quad (out of range in the lanes that do
#                                               not store), bpermute addresses of lane ^ 16 / lane ^ 32
S_LOGP = 14         # s[14:15] logits (the pool pointer's registers)
S_LGR = 84          # s[84:87] logits descriptor of the image (the pooled descriptor's registers)
S_PSR = 48          # s[48:51] patch-sum descriptor (the weight descriptor's registers: the weight pieces are resident)
S_NCLS, S_NCLS4, S_WNCLS4, S_LOGIMGB, S_NPW, S_NPIMG, S_NODE0 = 40, 52, 53, 54, 56, 78, 79
HEAD_KERNARG = 160  # the plain kernels' 120 bytes + head weight, head bias, logits, patch sums (8 each), ncls, patch-sum bytes (4 each)

S_VHST = S_PAD      # 1: the halo-offset registers hold the patch-independent offsets of an INTERIOR patch (kernarg pad word: 0 at entry)


def setup_load(kn):
    """setup_load(p_begin + lp): input descriptor of the patch and the three halo offsets of the thread.
    The per-lane part (three times: unit -> (row, column) of the 10 x 34 halo, bounds, byte offset; 57 VALU in a loop whose VALU issue is
    the bottleneck) depends on the patch only through the bounds: for an INTERIOR patch (no halo pixel outside the image) the patch's
    position goes into the descriptor's base and the offsets are the same for every such patch, so they are formed once and kept while
    interior patches follow each other (x runs fastest: 14 of 16 patches of a 512-wide row)."""
    kn.E(f"s_add_u32 s{S_P}, s{S_PBEGIN}, s{S_LP}")
    patch_coords(kn, S_P)
    desc_base(kn, S_INR, S_IN, S_IMG, S_IMGB, S_T[6], S_T[7], mask=False)
    ledge, lvalu, ldone = kn.newlabel("edge"), kn.newlabel("hofs"), kn.newlabel("hdone")
    # edge patch?  (y0, x0 are multiples of 8 / 32, H, W too)
    kn.E(f"s_add_u32 s{S_M}, s{S_Y0}, 8")
    kn.E(f"s_cmp_eq_u32 s{S_M}, s{S_H}")
    kn.E(f"s_cselect_b32 s{S_M + 1}, 1, 0")
    kn.E(f"s_cmp_eq_u32 s{S_Y0}, 0")
    kn.E(f"s_cselect_b32 s{S_M + 1}, 1, s{S_M + 1}")
    kn.E(f"s_add_u32 s{S_M}, s{S_X0}, 32")
    kn.E(f"s_cmp_eq_u32 s{S_M}, s{S_W}")
    kn.E(f"s_cselect_b32 s{S_M + 1}, 1, s{S_M + 1}")
    kn.E(f"s_cmp_eq_u32 s{S_X0}, 0")
    kn.E(f"s_cselect_b32 s{S_M + 1}, 1, s{S_M + 1}")
    kn.E(f"s_sub_u32 s{S_T[6]}, s{S_Y0}, 1")     # y0 - 1
    kn.E(f"s_sub_u32 s{S_T[7]}, s{S_X0}, 1")     # x0 - 1
    kn.E(f"s_cmp_lg_u32 s{S_M + 1}, 0")
    kn.E(f"s_cbranch_scc1 {ledge}")
    # interior: base += ((y0 - 1) * W + (x0 - 1)) * ldin * 4  (< 2^31: the launcher's size check)
    kn.E(f"s_mul_i32 s{S_M}, s{S_T[6]}, s{S_W}")
    kn.E(f"s_add_u32 s{S_M}, s{S_M}, s{S_T[7]}")
    kn.E(f"s_mul_i32 s{S_M}, s{S_M}, s{S_LDIN}")
    kn.E(f"s_lshl_b32 s{S_M}, s{S_M}, 2")
    kn.E(f"s_add_u32 s{S_INR}, s{S_INR}, s{S_M}")
    kn.E(f"s_addc_u32 s{S_INR + 1}, s{S_INR + 1}, 0")
    desc_mask(kn, S_INR)
    kn.E(f"s_cmp_eq_u32 s{S_VHST}, 1")
    kn.E(f"s_cbranch_scc1 {ldone}")             # the registers already hold the interior offsets
    kn.E(f"s_mov_b32 s{S_T[6]}, 0")
    kn.E(f"s_mov_b32 s{S_T[7]}, 0")
    kn.E(f"s_mov_b32 s{S_VHST}, 1")
    kn.E(f"s_branch {lvalu}")
    kn.L(ledge)
    desc_mask(kn, S_INR)
    kn.E(f"s_mov_b32 s{S_VHST}, 0")
    kn.L(lvalu)
    for i in range(3):
        d = VHOFF[i]
        kn.E(f"v_lshrrev_b32_e32 v{VT0}, 2, v{VTID}")
        if i:
            kn.E(f"v_add_u32_e32 v{VT0}, {128 * i}, v{VT0}")                    # hp
        kn.E(f"v_mul_u32_u24_e32 v{VT1}, 0x788, v{VT0}")
        kn.E(f"v_lshrrev_b32_e32 v{VT1}, 16, v{VT1}")                            # r = hp / 34
        kn.E(f"v_mul_u32_u24_e32 v{d}, 34, v{VT1}")
        kn.E(f"v_sub_u32_e32 v{d}, v{VT0}, v{d}")                                # cc
        kn.E(f"v_cmp_gt_u32_e32 vcc, 0x154, v{VT0}")                             # hp < 340
        kn.E(f"v_add_u32_e32 v{VT1}, s{S_T[6]}, v{VT1}")                         # y
        kn.E(f"v_add_u32_e32 v{d}, s{S_T[7]}, v{d}")                             # x
        kn.E(f"v_cmp_gt_u32_e64 s[{S_M}:{S_M + 1}], s{S_H}, v{VT1}")
        kn.E(f"s_and_b64 vcc, vcc, s[{S_M}:{S_M + 1}]")
        kn.E(f"v_cmp_gt_u32_e64 s[{S_M}:{S_M + 1}], s{S_W}, v{d}")
        kn.E(f"s_and_b64 vcc, vcc, s[{S_M}:{S_M + 1}]")
        kn.E(f"v_mad_u32_u24 v{VT1}, v{VT1}, s{S_W}, v{d}")                      # y * W + x
        kn.E(f"v_mul_lo_u32 v{VT1}, v{VT1}, s{S_LDIN}")
        kn.E(f"v_and_b32_e32 v{VT0}, 3, v{VTID}")                                # kq
        kn.E(f"v_lshl_add_u32 v{VT1}, v{VT0}, 2, v{VT1}")
        kn.E(f"v_lshlrev_b32_e32 v{VT1}, 2, v{VT1}")                             # bytes
        kn.E(f"v_mov_b32_e32 v{d}, s{S_OOB}")
        kn.E("s_nop 1")
        kn.E(f"v_cndmask_b32_e32 v{d}, v{d}, v{VT1}, vcc")
    kn.L(ldone)


def setup_load_at_patch_start(kn):
    """setup_load when the next halo request is chunk 0 of a patch the workgroup still has"""
    lskip = kn.newlabel("nosetup")
    kn.E(f"s_cmp_lg_u32 s{S_LC}, 0")
    kn.E(f"s_cbranch_scc1 {lskip}")
    kn.E(f"s_cmp_ge_u32 s{S_LP}, s{S_NPATCH}")
    kn.E(f"s_cbranch_scc1 {lskip}")
    setup_load(kn)
    kn.L(lskip)


def halo_load_ops(setn):
    return [f"buffer_load_dwordx4 {vr(HSET(setn, i), 4)}, v{VHOFF[i]}, s[{S_INR}:{S_INR + 3}], s{S_LC64} offen" for i in range(3)]


def halo_advance_ops():
    """lc = lc + 1 == nC ? 0 : lc + 1;  lp += lc == 0"""
    return [f"s_add_u32 s{S_LC}, s{S_LC}, 1", f"s_cmp_eq_u32 s{S_LC}, s{S_NC}", f"s_cselect_b32 s{S_LC}, 0, s{S_LC}",
            f"s_cmp_eq_u32 s{S_LC}, 0", f"s_addc_u32 s{S_LP}, s{S_LP}, 0", f"s_lshl_b32 s{S_LC64}, s{S_LC}, 6"]


def halo_store_ops(setn):
    return [f"ds_write_b128 v{VHST[i]}, {vr(HSET(setn, i), 4)}" for i in range(3)]


def flip_ops(regs):
    """the LDS addresses in regs move to the other raw buffer"""
    return [f"v_xor_b32_e32 v{r}, 0x{BUFX:x}, v{r}" for r in regs]


def emit(kn, ops):
    for x in ops:
        kn.E(x)


def halo_loads(kn, setn=0):
    emit(kn, halo_load_ops(setn) + halo_advance_ops())


def step_jm(s):
    """(jj, mi) of step s of a chunk: the two steps of one mi are adjacent, jj = 0 first"""
    return s & 1, s >> 1


def raw_reads(jp, jj, mi, hf):
    """the ds_read_b128 of half hf of step (jj, mi): returns instruction strings.
    The two components of a pair share one tile column (jp 0: cy = S2F for both; jp 1: cy = S1F of jj = 0 is cx of jj = 1), and
    the jj = 0 forming leaves that column's inner sum in the c quad (form_valu).  A jj = 1 step reads only its other column, into
    the a / b quads: two reads instead of four; the jj = 0 step of the same mi must be formed right before it."""
    base = mi * 10880 + hf * 16
    if jj == 1:
        cu = S3F if jp else S1F
        return [f"ds_read_b128 {vr(RAW(hf, 0), 4)}, v{VA} offset:{base + cu * 4}",
                f"ds_read_b128 {vr(RAW(hf, 1), 4)}, v{VB} offset:{base + cu * 4}"]
    cx = S2F if jp else 0
    cy = S1F if jp else S2F
    return [f"ds_read_b128 {vr(RAW(hf, 0), 4)}, v{VA} offset:{base + cx * 4}",
            f"ds_read_b128 {vr(RAW(hf, 1), 4)}, v{VB} offset:{base + cx * 4}",
            f"ds_read_b128 {vr(RAW(hf, 2), 4)}, v{VA} offset:{base + cy * 4}",
            f"ds_read_b128 {vr(RAW(hf, 3), 4)}, v{VB} offset:{base + cy * 4}"]


def form_valu(jp, jj, slot, hf, kn=WIDE):
    """transform + three-way split of half hf of step (jj, .) into pc[slot]: 34 VALU (jj = 0) / 30 VALU (jj = 1), chains interleaved.
    kn: the kernel whose sign / mask registers the list names (it is the same list otherwise)"""
    w = "-1.0" if not (jj == 1 and jp == 0) else "1.0"
    a, b, c, d = RAW(hf, 0), RAW(hf, 1), RAW(hf, 2), RAW(hf, 3)
    r = []
    # v = fma(w, fma(sgn, rb_y, ra_y), fma(sgn, rb_x, ra_x)) bit for bit: fma(sgn, b, a) as v_fmac; fma(+-1, qy, qx) = qx +- qy rounded once
    for e in range(4):
        r.append(f"v_fmac_f32_e32 v{a + e}, v{kn.VSGN}, v{b + e}")
    if jj == 0:
        # the c quad keeps qy: the shared column's inner sum, which the jj = 1 step of the same mi reuses
        for e in range(4):
            r.append(f"v_fmac_f32_e32 v{c + e}, v{kn.VSGN}, v{d + e}")
        for e in range(4):
            r.append(f"v_{'add' if w == '1.0' else 'sub'}_f32_e32 v{a + e}, v{a + e}, v{c + e}")
    elif jp == 0:
        for e in range(4):                # a = qx (column S1F), c = qy (S2F, shared): qx + qy
            r.append(f"v_add_f32_e32 v{a + e}, v{a + e}, v{c + e}")
    else:
        for e in range(4):                # c = qx (S1F, shared), a = qy (column S3F): qx - qy, the operands in the same order
            r.append(f"v_sub_f32_e32 v{a + e}, v{c + e}, v{a + e}")
    # pairs (0,1) -> piece dword hf*2, (2,3) -> hf*2+1;  temporaries: the b registers
    for piece in range(3):
        for p in range(2):
            r.append(f"v_perm_b32 v{PC(slot, piece) + hf * 2 + p}, v{a + 2 * p + 1}, v{a + 2 * p}, s{S_PERM}")
        if piece < 2:
            for e in range(4):
                r.append(f"v_and_b32_e32 v{b + e}, v{kn.VMASK}, v{a + e}")
            for e in range(4):
                r.append(f"v_sub_f32_e32 v{a + e}, v{a + e}, v{b + e}")
    assert len(r) == (34 if jj == 0 else 30)
    return r


def mfmas(kn, jj, mi, slot, c):
    """the MFMAs of step (jj, mi) of chunk c, six per n tile.  c == 0 is the first chunk of a patch: every accumulator chain starts from
    the constant 0 (no clearing of the 128 / 64 accumulators per patch: they were 8 % of the VALU operations of a 64-channel layer).
    The wide kernel streams its weight pieces through BX (c only tells the peeled first chunk from the loop's); the narrow kernels
    keep the pieces of every chunk in WN(c, ...)."""
    r = []
    for nt in range(kn.ntb):
        acc = vr(kn.ACC(jj, nt, mi), 16)
        for i, (pa, pb) in enumerate(((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))):
            w = BX(jj, nt, pb) if kn.ntb == 2 else WN(c, jj, pb)
            r.append(f"v_mfma_f32_32x32x16_bf16 {acc}, {vr(PC(slot, pa), 4)}, {vr(w, 4)}, {'0' if c == 0 and i == 0 else acc}")
    return r


def weight_load(jj, nt, p):
    return f"buffer_load_dwordx4 {vr(BX(jj, nt, p), 4)}, v{VLANE16}, s[{S_UR}:{S_UR + 3}], s{S_WO[jj][nt]} offen offset:{p * 1024}"


def emit_step(kn, jp, s, mf, a0, a1, pre, extra):
    """Step s of a chunk, both kernel widths: the MFMAs mf, and in the gap behind each of them its share of the rest.  a0, a1: the
    (first, last) gaps of the two transform halves; pre: the waits and wait states in front of the first MFMA; extra[gap]: what the
    caller adds to a gap, issued right behind the MFMA (wide_step, narrow_step).
    The raw-operand reads are spread over the gaps (at most two ds_read_b128 per gap, none waited for in the step it was issued
    in): the raw registers are two halves of four 16-byte registers (input channels 0-3 / 4-7 of the lane's eight); half 0 of step
    s + 2 is requested in the first two gaps of a1 of step s (its registers are free once the first half of step s + 1's transform
    has run), half 1 of step s + 1 in gaps 0-1 -- four reads per half for a jj = 0 step, two for a jj = 1 step (the shared column's
    inner sum stays in the c quad from the jj = 0 forming, one step earlier).  Reads of the next chunk begin in a1 of step 2: B1
    sits in front of step 2 and the read bases flip to the other buffer inside it."""
    slot = s & 1
    n1, n2 = (s + 1) & 3, (s + 2) & 3
    if s == 2:
        kn.E("s_waitcnt lgkmcnt(0)")
        kn.E("s_barrier")                    # B1: chunk c + 1 is complete in the other buffer
    emit(kn, pre)
    v0 = form_valu(jp, step_jm(n1)[0], slot ^ 1, 0, kn)
    v1 = form_valu(jp, step_jm(n1)[0], slot ^ 1, 1, kn)
    r1 = raw_reads(jp, *step_jm(n1), 1)            # half 1 of the next step
    r2 = raw_reads(jp, *step_jm(n2), 0)            # half 0 of the step after it
    def take(lst, n):
        for _ in range(min(n, len(lst))):
            kn.E(lst.pop(0))
    per0 = -(-len(v0) // (a0[1] - a0[0] + 1))
    per1 = -(-len(v1) // (a1[1] - a1[0] + 1))
    nlds = 0                              # LDS operations issued in this step so far (all younger than half 0's reads)
    for g, m in enumerate(mf):
        kn.E(m)
        for x in extra.get(g, []):
            kn.E(x)
            nlds += x.startswith("ds_")
        if g in (0, 1):
            nlds += min(2, len(r1))
            take(r1, 2)
        if g == a0[0]:
            # half 0 (requested in the previous step) complete: everything issued in this step so far may stay in flight
            kn.E(f"s_waitcnt lgkmcnt({nlds})")
        if a0[0] <= g <= a0[1]:
            take(v0, per0)
        if g == a1[0]:
            assert not v0
            kn.E("s_waitcnt lgkmcnt(0)")
            if s == 2:
                emit(kn, flip_ops([VA, VB]))
        if g in (a1[0], a1[0] + 1):
            take(r2, 2)
        if a1[0] <= g <= a1[1]:
            take(v1, per1)
    assert not v1 and not r1 and not r2


def wide_step(kn, jp, s, c):
    """twelve MFMAs; the transform halves in gaps 2..6 and 7..10"""
    jj, mi = step_jm(s)
    pre, extra = [], {}
    if s == 0:
        # this component's weight pieces (requested in step 2 of the previous chunk).  VMEM operations retire in order: younger than
        # them are the other component's six pieces (step 3); this chunk's staging is issued BEHIND this wait.  The halo registers
        # (older) are covered.
        pre.append("s_waitcnt vmcnt(6)")
        # Parking chunk c + 1 (halo registers -> the idle buffer) and requesting chunk c + 2 ride in the gaps of step 0 instead of
        # standing in front of it: the matrix pipe starts right behind B0.  vmcnt(6) above covers the halo registers (they are
        # older than the weight pieces it waits for).
        extra = {i: [x] for i, x in enumerate(halo_store_ops(0))}
        for i, x in enumerate(halo_load_ops(0)):
            extra.setdefault(3 + i, []).append(x)
        extra[6] = halo_advance_ops()
        extra[3] += flip_ops(VHST)
    if s == 1:
        pre.append("s_waitcnt vmcnt(3)")  # pieces requested in step 3 of the previous chunk; younger: the 3 halo loads of step 0
    # two wait states between the v_perm that wrote the last dword of this step's low-order operand piece (tail of the previous
    # step: only its final MFMA lies between) and the first MFMA, which reads that piece
    pre.append("s_nop 1")
    if mi == 1:                           # steps 2 (jj = 0) and 3 (jj = 1): the last reads of this component's pieces in the chunk;
        #                                   the next chunk's are requested right behind them
        extra = {1: [weight_load(jj, 0, 2)], 4: [weight_load(jj, 0, 1)], 5: [weight_load(jj, 0, 0)],
                 7: [weight_load(jj, 1, 2)], 10: [weight_load(jj, 1, 1)], 11: [weight_load(jj, 1, 0)]}
    emit_step(kn, jp, s, mfmas(kn, jj, mi, s & 1, c), (2, 6), (7, 10), pre, extra)


# =====================================================================================================================
# Narrow kernels (32 output channels per workgroup; asm form of wino3x3_cp_kernel<1, false, true, *>): a chunk is only six MFMAs
# per wave and step, so the loop is bound by the transform's VALU issue and by latency, not by the matrix pipe.  Against the wide
# kernel: (i) the wave's weight pieces of ALL chunks stay in registers (2 or 4 chunks: 48 / 96 registers; the accumulators are only
# 64) -- no weight stream at all; (ii) the halo is requested two chunks ahead through two register sets whose parity is static
# (the chunk loop is unrolled); (iii) scale / shift are applied by the finishing pass (two of the four shares are plain copies of
# the accumulators).  Same arithmetic order as the C++ kernel: bitwise equal outputs.
# =====================================================================================================================
def narrow_step(kn, jp, s, c):
    """six MFMAs; the transform halves in gaps 1..2 and 3..5"""
    jj, mi = step_jm(s)
    pre, extra = ["s_nop 1"], {}          # the previous step ends with the v_perm that writes this step's low-order operand piece, and the
    #                                       first MFMA reads that piece: two wait states between a VALU write and an MFMA read of it
    if s == 0:
        hs = (c + 1) & 1                  # the set holding chunk c + 1; it is refilled with chunk c + 3
        pre.append("s_waitcnt vmcnt(3)")  # (only the three loads of chunk c + 2 are younger)
        extra = {i: [x] for i, x in enumerate(halo_store_ops(hs))}
        extra[3] = flip_ops(VHST)
        for i, x in enumerate(halo_load_ops(hs)):
            extra.setdefault(3 + i, []).append(x)
        extra[5] += halo_advance_ops()
    emit_step(kn, jp, s, mfmas(kn, jj, mi, s & 1, c), (1, 2), (3, 5), pre, extra)


def emit_chunk(kn, jp, c):
    """one 16-channel chunk: B0, then four steps.  Parking chunk c + 1 and requesting the chunk after the parked ones ride in step 0.
    c: wide kernel 0 = the peeled first chunk of a patch, 1 = the body of the chunk loop; narrow kernels: the (static) chunk"""
    setup_load_at_patch_start(kn)
    kn.E("s_waitcnt lgkmcnt(0)")
    kn.E("s_barrier")                        # B0
    if kn.ntb == 2:
        # weight soffsets of chunk cn = c + 1 == nC ? 0 : c + 1
        kn.E(f"s_add_u32 s{S_T[0]}, s{S_C}, 1")
        kn.E(f"s_cmp_eq_u32 s{S_T[0]}, s{S_NC}")
        kn.E(f"s_cselect_b32 s{S_T[0]}, 0, s{S_T[0]}")
        kn.E(f"s_mul_i32 s{S_WO[0][0]}, s{S_T[0]}, 0xc000")
        kn.E(f"s_add_u32 s{S_WO[0][1]}, s{S_WO[0][0]}, s{S_NTSTRIDE}")
        kn.E(f"s_add_u32 s{S_WO[1][0]}, s{S_WO[0][0]}, 0xc00")
        kn.E(f"s_add_u32 s{S_WO[1][1]}, s{S_WO[0][1]}, 0xc00")
    for s in range(4):
        (wide_step if kn.ntb == 2 else narrow_step)(kn, jp, s, c)


def emit_finish_math(kn, Z, q, SCq, SHq):
    """z_i = share(jp 0) + share(jp 1); ya = (z0 + z1) + z2; yb = (z1 - z2) - z3; y = sc * y + sh -- the scalar sequence's values, packed"""
    for i in range(4):
        for e in (0, 2):
            kn.E(pk2("add", Z(q, 0, i) + e, Z(q, 0, i) + e, Z(q, 1, i) + e))
    ya, yb = Z(q, 1, 0), Z(q, 1, 1)
    for e in (0, 2):
        kn.E(pk2("add", ya + e, Z(q, 0, 0) + e, Z(q, 0, 1) + e))
    for e in (0, 2):
        kn.E(pk2("add", ya + e, ya + e, Z(q, 0, 2) + e))
    for e in (0, 2):
        kn.E(pk2("add", yb + e, Z(q, 0, 1) + e, Z(q, 0, 2) + e, neg_b=True))
    for e in (0, 2):
        kn.E(pk2("add", yb + e, yb + e, Z(q, 0, 3) + e, neg_b=True))
    for y in (ya, yb):
        for e in (0, 2):
            kn.E(pkfma2(y + e, SCq + e, y + e, SHq + e))


# ---------------------------------------------------------------------------------------------------------------------
# The patch epilogue.  Each of its sequences is written once and takes its registers from R (the driver's choice) and its n tile as
# arguments; emit_epilogue_wide and emit_epilogue_narrow order them.
# ---------------------------------------------------------------------------------------------------------------------
def nt_off(kn, nt):
    """the instruction offset of n tile nt's 32 channels (the narrow kernels have one n tile and write no offset)"""
    return f" offset:{nt * 128}" if kn.ntb == 2 else ""


def epilogue_begin(kn):
    """position of patch p_begin + pi, output descriptor of its image"""
    kn.E("s_nop 7")
    kn.E("s_nop 7")
    kn.E("s_nop 7")
    kn.E(f"s_add_u32 s{S_P}, s{S_PBEGIN}, s{S_PI}")
    patch_coords(kn, S_P)
    desc_base(kn, S_OUTR, S_OUT, S_IMG, S_OUTIMGB, S_T[6], S_T[7])


def pool_descriptor(kn):
    # pooled image bytes = (H/2) * (W/2) * ldpool * 4
    kn.E(f"s_lshr_b32 s{S_T[4]}, s{S_H}, 1")
    kn.E(f"s_lshr_b32 s{S_T[5]}, s{S_W}, 1")
    kn.E(f"s_mul_i32 s{S_T[4]}, s{S_T[4]}, s{S_T[5]}")
    kn.E(f"s_mul_i32 s{S_T[4]}, s{S_T[4]}, s{S_LDPOOL}")
    kn.E(f"s_lshl_b32 s{S_T[4]}, s{S_T[4]}, 2")
    kn.E(f"s_mov_b32 s{S_POOLR + 2}, s{S_T[4]}")
    desc_base(kn, S_POOLR, S_POOL, S_IMG, S_T[4], S_T[6], S_T[7])


def unit_ids(kn, R):
    """finishing unit of the thread: channel quad cq, tile T"""
    kn.E(f"v_and_b32_e32 v{R.CQ}, 7, v{VTID}")
    kn.E(f"v_lshrrev_b32_e32 v{R.VT}, 3, v{VTID}")


def unit_addresses(kn, R):
    """the unit's two LDS read bases; leaves oy in e1, ox in e2, oy * W + ox in e3"""
    kn.E(f"v_and_b32_e32 v{R.e0}, 32, v{R.VT}")
    kn.E(f"v_and_b32_e32 v{R.e1}, 3, v{R.VT}")
    kn.E(f"v_bfe_u32 v{R.e2}, v{R.VT}, 3, 2")                       # (T & 31) >> 3
    kn.E(f"v_lshl_add_u32 v{R.e1}, v{R.e2}, 2, v{R.e1}")
    kn.E(f"v_lshl_add_u32 v{R.e0}, v{R.e1}, 1, v{R.e0}")
    kn.E(f"v_bfe_u32 v{R.e2}, v{R.VT}, 2, 1")
    kn.E(f"v_add_u32_e32 v{R.e0}, v{R.e0}, v{R.e2}")                  # Tslot
    kn.E(f"v_lshlrev_b32_e32 v{R.e0}, 7, v{R.e0}")
    kn.E(f"v_lshl_add_u32 v{R.VZ0}, v{R.CQ}, 4, v{R.e0}")
    kn.E(f"v_add_u32_e32 v{R.VZ1}, 0x10000, v{R.VZ0}")
    kn.E(f"v_lshrrev_b32_e32 v{R.e1}, 4, v{R.VT}")
    kn.E(f"v_lshl_add_u32 v{R.e1}, v{R.e1}, 1, s{S_Y0}")            # oy
    kn.E(f"v_and_b32_e32 v{R.e2}, 15, v{R.VT}")
    kn.E(f"v_lshl_add_u32 v{R.e2}, v{R.e2}, 1, s{S_X0}")            # ox
    kn.E(f"v_mad_u32_u24 v{R.e3}, v{R.e1}, s{S_W}, v{R.e2}")


def out_address(kn, R):
    kn.E(f"v_mul_lo_u32 v{R.e3}, v{R.e3}, s{S_LDOUT}")
    kn.E(f"v_lshl_add_u32 v{R.e3}, v{R.CQ}, 2, v{R.e3}")
    kn.E(f"v_lshlrev_b32_e32 v{R.VOUT}, 2, v{R.e3}")
    kn.E(f"v_add_u32_e32 v{R.VOUT}, s{S_N64X4}, v{R.VOUT}")


def pool_address(kn, R):
    """pooled pixel (behind out_address: oy, ox are used up)"""
    kn.E(f"v_lshrrev_b32_e32 v{R.e1}, 1, v{R.e1}")
    kn.E(f"v_lshrrev_b32_e32 v{R.e2}, 1, v{R.e2}")
    kn.E(f"v_mad_u32_u24 v{R.e3}, v{R.e1}, s{S_T[5]}, v{R.e2}")
    kn.E(f"v_mul_lo_u32 v{R.e3}, v{R.e3}, s{S_LDPOOL}")
    kn.E(f"v_lshl_add_u32 v{R.e3}, v{R.CQ}, 2, v{R.e3}")
    kn.E(f"v_lshlrev_b32_e32 v{R.VPOOL}, 2, v{R.e3}")
    kn.E(f"v_add_u32_e32 v{R.VPOOL}, s{S_N64X4}, v{R.VPOOL}")


def request_scale_shift(kn, voff, SC, SH):
    """per-channel scale / shift of the FINISHING unit's channel quad (n0 = first channel of the workgroup + nt * 32 + cq * 4; voff =
    cq * 16), SC[nt] / SH[nt] of every n tile: requested first, used last; a missing array is 1 / 0.  (Reader side: two of the four
    shares are then plain copies of the accumulators and the other two one add / subtract -- 32 instead of 96 VALU per n tile in
    the write phase, 16 fma in the finishing pass.)"""
    for (ptr, rs, regs, dflt) in ((S_SCALE, S_SCR, SC, "1.0"), (S_SHIFT, S_SHR, SH, "0")):
        ln, ldn = kn.newlabel("nul"), kn.newlabel("nud")
        kn.E(f"s_cmp_eq_u64 s[{ptr}:{ptr + 1}], 0")
        kn.E(f"s_cbranch_scc1 {ln}")
        for nt, r in enumerate(regs):
            kn.E(f"buffer_load_dwordx4 {vr(r, 4)}, v{voff}, s[{rs}:{rs + 3}], s{S_N64X4} offen{nt_off(kn, nt)}")
        kn.E(f"s_branch {ldn}")
        kn.L(ln)
        for r in regs:
            for e in range(4):
                kn.E(f"v_mov_b32_e32 v{r + e}, {dflt}")
        kn.L(ldn)


def share_bases(kn, jp):
    # add-TID bases of this wave's two shares
    #   q = 0: jp 0 -> region (0,0) = slot 0 (the consumed raw buffer, even chunk count), jp 1 -> region (0,1) = slot 1
    #   q = 1: slot 2 + jp, biased by ZBIAS
    kn.E(f"s_lshl_b32 s{S_T[0]}, s{S_WI}, 13")                  # wi * 64 * 32 * 4
    if jp:
        kn.E(f"s_add_u32 s{S_T[0]}, s{S_T[0]}, 0x{RAWB:x}")
    kn.E(f"s_lshl_b32 s{S_T[1]}, s{S_WI}, 13")
    kn.E(f"s_add_u32 s{S_T[1]}, s{S_T[1]}, 0x{(2 + jp) * RAWB - ZBIAS:x}")
    kn.E("s_waitcnt lgkmcnt(0)")
    kn.E("s_barrier")                       # every wave has finished reading the consumed raw buffer
    # (no vmcnt wait here: the write phase reads accumulators only; the scale / shift quads requested above are first needed by the
    # finishing pass of n tile 0, a whole write phase and a barrier later)


def write_shares(kn, jp, nt, TMP):
    """the wave's shares of n tile nt -> LDS; TMP: two groups of four temporaries, used in turn"""
    def share2(q, mi, r, t):         # -> the registers of the shares of accumulators r, r + 1;  jp 0: q0 = m0 + m1, q1 = m1;  jp 1: q0 = m0, q1 = -m0 - m1
        m0, m1 = kn.ACC(0, nt, mi) + r, kn.ACC(1, nt, mi) + r
        if jp == 0 and q == 0:
            kn.E(pk2("add", t, m0, m1))
            return [t, t + 1]
        if jp == 0:
            return [m1, m1 + 1]
        if q == 0:
            return [m0, m0 + 1]
        kn.E(pk2("add", t, m0, m1, neg_a=True, neg_b=True))
        return [t, t + 1]
    for q in range(2):
        kn.E(f"s_mov_b32 m0, s{S_T[q]}")
        kn.E("s_nop 0")
        g = 0
        for mi in range(2):
            for r0 in range(0, 16, 4):
                ts = TMP[(g & 1) * 4:(g & 1) * 4 + 4]
                g += 1
                src = share2(q, mi, r0, ts[0]) + share2(q, mi, r0 + 2, ts[2])
                kn.E("s_nop 0")
                for i in range(4):
                    off = (32 * mi + 2 * (r0 + i)) * 128 + (ZBIAS if q else 0)
                    kn.E(f"ds_write_addtid_b32 v{src[i]} offset:{off}")
    kn.E("s_waitcnt lgkmcnt(0)")
    kn.E("s_barrier")


def finish_unit(kn, nt, R, SC, SH):
    """finishing pass of unit (T, cq): 16 share reads into the dead accumulators of n tile nt, output transform, scale / shift, ReLU.
    Returns Z: the outputs are Z(q, 1, 0) (upper row) and Z(q, 1, 1) (lower row) of column q; Z(0, 0, 0), Z(0, 0, 1) are free quads"""
    zb = [kn.ACC(0, nt, 0), kn.ACC(0, nt, 1), kn.ACC(1, nt, 0), kn.ACC(1, nt, 1)]
    def Z(q, j, i):
        n = (q * 2 + j) * 4 + i
        return zb[n // 4] + (n % 4) * 4
    for q in range(2):
        for j in range(2):
            for i in range(4):
                kn.E(f"ds_read_b128 {vr(Z(q, j, i), 4)}, v{R.VZ1 if q else R.VZ0} offset:{j * RAWB + i * 8192}")
    # the q = 0 half of the reads first (LDS operations of a wave return in order): its arithmetic runs while the q = 1 half lands;
    # n tile 0 also waits for scale / shift
    kn.E("s_waitcnt vmcnt(0) lgkmcnt(8)" if nt == 0 else "s_waitcnt lgkmcnt(8)")
    emit_finish_math(kn, Z, 0, SC, SH)
    kn.E("s_waitcnt lgkmcnt(0)")
    emit_finish_math(kn, Z, 1, SC, SH)
    lnr = kn.newlabel("norelu")
    kn.E(f"s_cmp_eq_u32 s{S_RELU}, 0")
    kn.E(f"s_cbranch_scc1 {lnr}")
    for q in range(2):
        for y in (Z(q, 1, 0), Z(q, 1, 1)):
            for e in range(4):
                kn.E(f"v_max_f32_e32 v{y + e}, 0, v{y + e}")
    kn.L(lnr)
    return Z


def store_features(kn, nt, Z, R):
    for y, soff in ((Z(0, 1, 0), "0"), (Z(1, 1, 0), f"s{S_LD4}"), (Z(0, 1, 1), f"s{S_SW4}"), (Z(1, 1, 1), f"s{S_SUMOFF}")):
        kn.E(f"buffer_store_dwordx4 {vr(y, 4)}, v{R.VOUT}, s[{S_OUTR}:{S_OUTR + 3}], {soff} offen{nt_off(kn, nt)} nt")


def fused_pool(kn, nt, Z, R):
    """maximum of the unit's 2 x 2 outputs -> the pooled tensor, if there is one"""
    lnp = kn.newlabel("nopool")
    kn.E(f"s_cmp_eq_u64 s[{S_POOL}:{S_POOL + 1}], 0")
    kn.E(f"s_cbranch_scc1 {lnp}")
    pm, pn = Z(0, 0, 0), Z(0, 0, 1)
    for e in range(4):
        kn.E(f"v_max_f32_e32 v{pm + e}, v{Z(0, 1, 0) + e}, v{Z(0, 1, 1) + e}")
    for e in range(4):
        kn.E(f"v_max_f32_e32 v{pn + e}, v{Z(1, 1, 0) + e}, v{Z(1, 1, 1) + e}")
    for e in range(4):
        kn.E(f"v_max_f32_e32 v{pm + e}, v{pm + e}, v{pn + e}")
    kn.E(f"buffer_store_dwordx4 {vr(pm, 4)}, v{R.VPOOL}, s[{S_POOLR}:{S_POOLR + 3}], 0 offen{nt_off(kn, nt)}")
    kn.L(lnp)


def emit_epilogue_wide(kn, jp):
    # free registers: the second operand slot (v188..v199), the d quads of both raw halves (v212..v215, v228..v231) and the a / b
    # quads of raw half 1 (v216..v223).  The a / b quads of raw half 0 receive the next patch's first reads (spread schedule) and the
    # c quads hold the inner sums of its step 0 that its step 1 reuses (raw_reads): they stay untouched
    R = Regs(CQ=212, VT=213, VZ0=188, VZ1=189, VOUT=190, VPOOL=191, e0=196, e1=197, e2=198, e3=199)
    SC4, SH4 = [192, 228], [R.e0, 220]       # both n tiles; e0..e3 are dead once the addresses are formed
    epilogue_begin(kn)
    pool_descriptor(kn)
    unit_ids(kn, R)
    unit_addresses(kn, R)
    out_address(kn, R)
    pool_address(kn, R)
    kn.E(f"v_lshlrev_b32_e32 v{R.CQ}, 4, v{R.CQ}")                   # (cq is not needed any more)
    request_scale_shift(kn, R.CQ, SC4, SH4)
    share_bases(kn, jp)
    for nt in range(2):
        write_shares(kn, jp, nt, [216, 217, 218, 219] * 2)
        Z = finish_unit(kn, nt, R, SC4[nt], SH4[nt])
        store_features(kn, nt, Z, R)
        fused_pool(kn, nt, Z, R)
        # (the accumulators -- registers of the finishing pass -- are NOT cleared: the first chunk of a patch is a peeled copy of the
        # chunk loop whose accumulator chains start from the constant 0)
        kn.E("s_waitcnt lgkmcnt(0)")
        kn.E("s_barrier")                   # the regions are rewritten by the next pass / receive the next raw chunk


def emit_head_math(kn, Y, P, Q, CQ):
    """Head-fused finishing pass, behind the feature stores.  Y: the four pixels of the lane's 2 x 2 tile (p = 2 * row + column), four
    channels each, after scale / shift / ReLU; the eight lanes of a tile hold its 32 channels.  P, Q: two free register quads.
      * logits: per pixel and class a 4-term fma chain that starts from the bias in channel quad 0 and from 0 elsewhere, then an xor
        fold over the tile's eight lanes (quad_perm 1, quad_perm 2, half mirror: every lane ends with the same sum);
      * patch sums: (p0 + p1) + (p2 + p3) per channel, then an xor fold over the wave's eight tiles (row_ror 8, bpermute 16 and 32).
    The four chains of a stage are interleaved (a DPP operand written by the VALU needs two wait states), and the two bpermute round
    trips of the patch sums run under the logit arithmetic of classes 0 and 1."""
    def fold_add():
        kn.E("s_waitcnt lgkmcnt(0)")
        for e in (0, 2):
            kn.E(pk2("add", P + e, P + e, Q + e))
    def fold_issue(vb):
        for e in range(4):
            kn.E(f"ds_bpermute_b32 v{Q + e}, v{vb}, v{P + e}")
    for e in (0, 2):
        kn.E(pk2("add", P + e, Y[0] + e, Y[1] + e))
    for e in (0, 2):
        kn.E(pk2("add", Q + e, Y[2] + e, Y[3] + e))
    for e in (0, 2):
        kn.E(pk2("add", P + e, P + e, Q + e))
    kn.E("s_nop 1")
    for e in range(4):
        kn.E(f"v_add_f32_dpp v{P + e}, v{P + e}, v{P + e} row_ror:8 row_mask:0xf bank_mask:0xf")
    fold_issue(VBP16)
    lst = kn.newlabel("hstore")
    for k in range(4):
        if k:
            kn.E(f"s_cmp_lt_u32 s{S_NCLS}, {k + 1}")
            kn.E(f"s_cbranch_scc1 {lst}")
        for p in range(4):
            kn.E(f"v_fma_f32 v{DL(k, p)}, v{Y[p]}, v{WQ(k, 0)}, v{BL(k)}")
        for e in range(1, 4):
            for p in range(4):
                kn.E(f"v_fmac_f32_e32 v{DL(k, p)}, v{Y[p] + e}, v{WQ(k, e)}")
        for ctl in ("quad_perm:[1,0,3,2]", "quad_perm:[2,3,0,1]", "row_half_mirror"):
            for p in range(4):
                kn.E(f"v_add_f32_dpp v{DL(k, p)}, v{DL(k, p)}, v{DL(k, p)} {ctl} row_mask:0xf bank_mask:0xf")
        if k == 0:
            fold_add()
            fold_issue(VBP32)
    kn.L(lst)
    # the lane's output row: channel quad 0 takes pixels 0, 1, quad 1 pixels 2, 3; [column][class] is the NHWC order of the logits
    kn.E(f"v_cmp_eq_u32_e32 vcc, 1, v{CQ}")
    ldone = kn.newlabel("hdone")
    for n in range(1, 5):
        lnext = kn.newlabel("hn")
        if n < 4:
            kn.E(f"s_cmp_lg_u32 s{S_NCLS}, {n}")
            kn.E(f"s_cbranch_scc1 {lnext}")
        for pp in range(2):
            for k in range(n):
                kn.E(f"v_cndmask_b32_e32 v{SS(pp * (4 if n == 3 else n) + k)}, v{DL(k, pp)}, v{DL(k, 2 + pp)}, vcc")   # (register tuples are even-aligned)
        d = f"v{VLG}, s[{S_LGR}:{S_LGR + 3}], 0 offen"
        if n == 1:
            kn.E(f"buffer_store_dwordx2 {vr(SS(0), 2)}, {d}")
        elif n == 2:
            kn.E(f"buffer_store_dwordx4 {vr(SS(0), 4)}, {d}")
        elif n == 3:
            kn.E(f"buffer_store_dwordx3 {vr(SS(0), 3)}, {d}")
            kn.E(f"buffer_store_dwordx3 {vr(SS(4), 3)}, {d} offset:12")
        else:
            kn.E(f"buffer_store_dwordx4 {vr(SS(0), 4)}, {d}")
            kn.E(f"buffer_store_dwordx4 {vr(SS(4), 4)}, {d} offset:16")
        if n < 4:
            kn.E(f"s_branch {ldone}")
            kn.L(lnext)
    kn.L(ldone)
    fold_add()
    kn.E("s_nop 0")
    kn.E(f"buffer_store_dwordx4 {vr(P, 4)}, v{VPS}, s[{S_PSR}:{S_PSR + 3}], 0 offen")


def emit_epilogue_narrow(kn, jp):
    # free registers as in emit_epilogue_wide: the c quads of the raw halves (v208..v211, v224..v227) carry the next patch's step 0
    # inner sums into its step 1
    R = Regs(CQ=228, VT=229, VZ0=188, VZ1=189, VOUT=190, VPOOL=191, e0=192, e1=193, e2=194, e3=195)
    SC4, SH4 = 196, 212
    epilogue_begin(kn)
    if kn.head:
        kn.E("; only-head {")
        # logits descriptor of the image, first graph node of the image
        desc_base(kn, S_LGR, S_LOGP, S_IMG, S_LOGIMGB, S_T[6], S_T[7])
        kn.E(f"s_mul_i32 s{S_NODE0}, s{S_IMG}, s{S_NPIMG}")
        kn.E("; }")
    else:
        kn.E("; only-plain {")
        pool_descriptor(kn)
        kn.E("; }")
    unit_ids(kn, R)
    kn.E(f"v_lshlrev_b32_e32 v{R.e0}, 4, v{R.CQ}")
    request_scale_shift(kn, R.e0, [SC4], [SH4])
    unit_addresses(kn, R)
    if kn.head:
        kn.E("; only-head {")
        kn.E(f"v_mul_lo_u32 v{VLG}, v{R.e3}, s{S_NCLS4}")                      # the tile's first pixel in the logits of the image (bytes)
        kn.E("; }")
    out_address(kn, R)
    if kn.head:
        kn.E("; only-head {")
        # The eight lanes of a tile (channel quads 0..7) all hold its logits after the fold: quad 0 stores the upper row of the 2 x 2
        # tile, quad 1 the lower row, the others get an offset past the descriptor's range (the store is dropped, as the halo loads
        # of out-of-image pixels are)
        kn.E(f"v_mul_u32_u24_e32 v{VPS}, s{S_WNCLS4}, v{R.CQ}")
        kn.E(f"v_add_u32_e32 v{VLG}, v{VLG}, v{VPS}")
        kn.E(f"v_cmp_gt_u32_e32 vcc, 2, v{R.CQ}")
        kn.E(f"v_mov_b32_e32 v{VPS}, s{S_OOB}")
        kn.E("s_nop 1")
        kn.E(f"v_cndmask_b32_e32 v{VLG}, v{VPS}, v{VLG}, vcc")
        # A wave's eight tiles are 2 rows x 16 columns of ONE graph patch (16 x 16 pixels): its partial sum goes to row pair
        # (oy >> 1) & 7 of node (img, oy >> 4, ox >> 4) in the scratch [node][8 row pairs][32 channels], from the lanes of tile 0
        kn.E(f"v_lshrrev_b32_e32 v{R.e3}, 4, v{R.e1}")
        kn.E(f"v_lshrrev_b32_e32 v{VPS}, 4, v{R.e2}")
        kn.E(f"v_mad_u32_u24 v{R.e3}, v{R.e3}, s{S_NPW}, v{VPS}")
        kn.E(f"v_add_u32_e32 v{R.e3}, s{S_NODE0}, v{R.e3}")
        kn.E(f"v_bfe_u32 v{VPS}, v{R.e1}, 1, 3")
        kn.E(f"v_lshl_add_u32 v{R.e3}, v{R.e3}, 3, v{VPS}")
        kn.E(f"v_lshl_add_u32 v{R.e3}, v{R.e3}, 3, v{R.CQ}")
        kn.E(f"v_lshlrev_b32_e32 v{R.e3}, 4, v{R.e3}")
        kn.E(f"v_and_b32_e32 v{VPS}, 7, v{R.VT}")
        kn.E(f"v_cmp_eq_u32_e32 vcc, 0, v{VPS}")
        kn.E(f"v_mov_b32_e32 v{VPS}, s{S_OOB}")
        kn.E("s_nop 1")
        kn.E(f"v_cndmask_b32_e32 v{VPS}, v{VPS}, v{R.e3}, vcc")
        kn.E("; }")
    else:
        kn.E("; only-plain {")
        pool_address(kn, R)
        kn.E("; }")
    share_bases(kn, jp)
    write_shares(kn, jp, 0, [216 + i for i in range(8)])
    Z = finish_unit(kn, 0, R, SC4, SH4)
    store_features(kn, 0, Z, R)
    if kn.head:
        kn.E("; only-head {")
        emit_head_math(kn, [Z(0, 1, 0), Z(1, 1, 0), Z(0, 1, 1), Z(1, 1, 1)], Z(0, 0, 0), Z(0, 0, 1), R.CQ)
        kn.E("; }")
    else:
        kn.E("; only-plain {")
        fused_pool(kn, 0, Z, R)
        kn.E("; }")
    kn.E("s_waitcnt lgkmcnt(0)")            # (no clearing of the accumulators: chunk 0's chains start from the constant 0)
    kn.E("s_barrier")


def emit_patch_loop(kn, jp):
    lp = kn.newlabel("patch")
    lc = kn.newlabel("chunk") if kn.ntb == 2 else None
    kn.L(lp)
    if kn.ntb == 2:
        kn.E(f"s_mov_b32 s{S_C}, 0")
        emit_chunk(kn, jp, 0)                # chunk 0, peeled (a layer has at least two chunks: Cp % 32 == 0)
        kn.E(f"s_mov_b32 s{S_C}, 1")
        kn.L(lc)
        emit_chunk(kn, jp, 1)
        kn.E(f"s_add_u32 s{S_C}, s{S_C}, 1")
        kn.E(f"s_cmp_lt_u32 s{S_C}, s{S_NC}")
        kn.E(f"s_cbranch_scc1 {lc}")
    else:
        for c in range(kn.nc):
            emit_chunk(kn, jp, c)
    (emit_epilogue_wide if kn.ntb == 2 else emit_epilogue_narrow)(kn, jp)
    kn.E(f"s_add_u32 s{S_PI}, s{S_PI}, 1")
    kn.E(f"s_cmp_lt_u32 s{S_PI}, s{S_NPATCH}")
    kn.E(f"s_cbranch_scc1 {lp}")
    kn.E(f"s_branch {kn.end}")


def emit_prologue(kn):
    kn.E("s_load_dwordx16 s[4:19], s[0:1], 0x0")
    kn.E("s_load_dwordx8 s[20:27], s[0:1], 0x40")
    kn.E("s_load_dwordx4 s[28:31], s[0:1], 0x60")
    kn.E("s_load_dwordx2 s[32:33], s[0:1], 0x70")
    kn.E(f"v_mov_b32_e32 v{VTID}, v0")
    kn.E("s_waitcnt lgkmcnt(0)")
    # item = (wg & 7) * per_xcd + (wg >> 3)
    t = S_T
    kn.E(f"s_and_b32 s{t[0]}, s2, 7")
    kn.E(f"s_mul_i32 s{t[0]}, s{t[0]}, s{S_PERXCD}")
    kn.E(f"s_lshr_b32 s{t[1]}, s2, 3")
    kn.E(f"s_add_u32 s{t[0]}, s{t[0]}, s{t[1]}")
    kn.E(f"s_cmp_ge_u32 s{t[0]}, s{S_NITEMS}")
    kn.E(f"s_cbranch_scc1 {kn.end}")
    divmod_magic(kn, t[0], S_NGROUPS, S_MGNG, S_NBLOCK, t[1], t[2], t[3])
    kn.E(f"s_mul_i32 s{S_PBEGIN}, s{t[1]}, s{S_PPB}")
    kn.E(f"s_sub_i32 s{t[2]}, s{S_TOTAL}, s{S_PBEGIN}")
    kn.E(f"s_min_i32 s{S_NPATCH}, s{S_PPB}, s{t[2]}")
    kn.E(f"s_cmp_lt_i32 s{S_NPATCH}, 1")
    kn.E(f"s_cbranch_scc1 {kn.end}")
    # constants
    kn.E(f"s_mov_b32 s{S_MASK}, 0xffff0000")
    kn.E(f"s_mov_b32 s{S_PERM}, 0x07060302")
    kn.E(f"s_mov_b32 s{S_OOB}, 0x7fff0000")
    kn.E(f"s_mul_i32 s{S_TXTY}, s{S_TX}, s{S_TY}")
    kn.E(f"s_mul_i32 s{S_IMGB}, s{S_H}, s{S_W}")
    kn.E(f"s_mul_i32 s{S_OUTIMGB}, s{S_IMGB}, s{S_LDOUT}")
    kn.E(f"s_lshl_b32 s{S_OUTIMGB}, s{S_OUTIMGB}, 2")
    kn.E(f"s_mul_i32 s{S_IMGB}, s{S_IMGB}, s{S_LDIN}")
    kn.E(f"s_lshl_b32 s{S_IMGB}, s{S_IMGB}, 2")
    kn.E(f"s_mul_i32 s{S_NTSTRIDE}, s{S_NC}, 0xc000")
    kn.E(f"s_lshl_b32 s{S_N64X4}, s{S_NBLOCK}, {8 if kn.ntb == 2 else 7}")     # byte offset of the workgroup's first output channel
    kn.E(f"s_lshl_b32 s{S_LD4}, s{S_LDOUT}, 2")
    kn.E(f"s_mul_i32 s{S_SW4}, s{S_W}, s{S_LD4}")
    kn.E(f"s_add_u32 s{S_SUMOFF}, s{S_SW4}, s{S_LD4}")
    # descriptors: input (base per patch), output (base per patch), pooled, scale, shift, weight pieces
    kn.E(f"s_mov_b32 s{S_INR + 2}, s{S_IMGB}")
    kn.E(f"s_mov_b32 s{S_INR + 3}, 0x00020000")
    kn.E(f"s_mov_b32 s{S_OUTR + 2}, s{S_OUTIMGB}")
    kn.E(f"s_mov_b32 s{S_OUTR + 3}, 0x00020000")
    kn.E(f"s_mov_b32 s{S_POOLR + 3}, 0x00020000")
    for (r, p) in ((S_SCR, S_SCALE), (S_SHR, S_SHIFT)):
        kn.E(f"s_mov_b32 s{r}, s{p}")
        desc_mask(kn, r, p)
        kn.E(f"s_mov_b32 s{r + 2}, 0x7ffffff0")
        kn.E(f"s_mov_b32 s{r + 3}, 0x00020000")
    # wave roles
    kn.E(f"v_lshrrev_b32_e32 v0, 6, v{VTID}")
    kn.E("s_nop 3")                                    # VALU write -> v_readfirstlane of the same register: wait states (measured: without
    #                                                 them some waves read the OLD v0 = the thread id)
    kn.E("v_readfirstlane_b32 s60, v0")
    kn.E("s_nop 3")
    kn.E(f"s_and_b32 s{S_WI}, s60, 3")
    kn.E(f"s_lshr_b32 s{S_JP}, s60, 2")
    kn.E(f"s_lshl_b32 s61, s{S_WI}, 1")
    kn.E("s_lshr_b32 s62, 0x64, s61")
    kn.E("s_and_b32 s62, s62, 3")                      # ra
    kn.E("s_lshr_b32 s63, 0xda, s61")
    kn.E("s_and_b32 s63, s63, 3")                      # rb
    kn.E(f"s_cmp_eq_u32 s{S_WI}, 1")
    kn.E(f"s_cselect_b32 s{S_SGN}, 1.0, -1.0")
    # weight descriptor: base = wu + nblock * 2 * nC * 49152 + (wi * 4 + 2 jp) * 3072
    kn.E(f"s_lshl_b32 s64, s{S_NTSTRIDE}, {1 if kn.ntb == 2 else 0}")   # u_bytes of the workgroup's n tiles
    kn.E(f"s_mul_i32 s65, s{S_NBLOCK}, s64")
    kn.E(f"s_lshl_b32 s66, s{S_WI}, 2")
    kn.E(f"s_lshl_b32 s67, s{S_JP}, 1")
    kn.E("s_add_u32 s66, s66, s67")
    kn.E("s_mul_i32 s66, s66, 0xc00")
    kn.E("s_add_u32 s65, s65, s66")
    kn.E(f"s_add_u32 s{S_UR}, s{S_WU}, s65")
    kn.E(f"s_addc_u32 s{S_UR + 1}, s{S_WU + 1}, 0")
    desc_mask(kn, S_UR)
    kn.E(f"s_mov_b32 s{S_UR + 2}, s64")
    kn.E(f"s_mov_b32 s{S_UR + 3}, 0x00020000")
    # lane constants
    kn.E(f"v_and_b32_e32 v1, 63, v{VTID}")             # lane
    kn.E(f"v_lshlrev_b32_e32 v{VLANE16}, 4, v1")
    kn.E("v_and_b32_e32 v2, 31, v1")                   # lr
    kn.E("v_lshrrev_b32_e32 v3, 5, v1")                # lh
    kn.E("v_and_b32_e32 v4, 15, v2")                   # tx
    kn.E("v_lshrrev_b32_e32 v5, 4, v2")                # ty
    kn.E("v_lshlrev_b32_e32 v5, 1, v5")                # 2 ty
    kn.E("v_mul_u32_u24_e32 v4, 0x50, v4")             # tx * 80
    kn.E("v_lshl_add_u32 v4, v3, 5, v4")               # + lh * 32
    for (dst, srow) in ((VA, 62), (VB, 63)):
        kn.E(f"v_add_u32_e32 v6, s{srow}, v5")
        kn.E("v_mul_u32_u24_e32 v6, 0xaa0, v6")        # (2 ty + r) * 34 * 80
        kn.E("v_add_u32_e32 v6, v6, v4")
        kn.E(f"v_add_u32_e32 v{dst}, 0x{BUFX:x}, v6")  # chunk 0 of a patch sits in slot 4
    for i in range(3):
        kn.E(f"v_lshrrev_b32_e32 v1, 2, v{VTID}")
        if i:
            kn.E(f"v_add_u32_e32 v1, {128 * i}, v1")
        kn.E("v_mul_u32_u24_e32 v2, 0x788, v1")
        kn.E("v_lshrrev_b32_e32 v2, 16, v2")           # r
        kn.E("v_mul_u32_u24_e32 v3, 34, v2")
        kn.E("v_sub_u32_e32 v3, v1, v3")               # cc
        kn.E("v_and_b32_e32 v4, 1, v3")
        kn.E("v_lshl_add_u32 v4, v2, 1, v4")           # r * 2 + (cc & 1)
        kn.E("v_mul_u32_u24_e32 v4, 17, v4")
        kn.E("v_lshrrev_b32_e32 v3, 1, v3")
        kn.E("v_add_u32_e32 v4, v4, v3")
        kn.E("v_mul_u32_u24_e32 v4, 0x50, v4")
        kn.E(f"v_and_b32_e32 v5, 3, v{VTID}")
        kn.E(f"v_lshl_add_u32 v{VHST[i]}, v5, 4, v4")
    kn.E(f"v_mov_b32_e32 v{kn.VMASK}, s{S_MASK}")
    kn.E(f"v_mov_b32_e32 v{kn.VSGN}, s{S_SGN}")
    # pipeline lead-in
    kn.E(f"s_mov_b32 s{S_LC}, 0")
    kn.E(f"s_mov_b32 s{S_LP}, 0")
    kn.E(f"s_mov_b32 s{S_PI}, 0")
    kn.E(f"s_mov_b32 s{S_LC64}, 0")
    if kn.ntb == 1:
        # the wave's weight pieces of every chunk (resident for the life of the workgroup), then the halo of chunks 0 (-> slot 4), 1 and 2
        for c in range(kn.nc):
            for jj in range(2):
                kn.E(f"s_mov_b32 s{S_WO[0][0]}, 0x{c * 0xc000 + jj * 0xc00:x}")
                for pp in range(3):
                    kn.E(f"buffer_load_dwordx4 {vr(WN(c, jj, pp), 4)}, v{VLANE16}, s[{S_UR}:{S_UR + 3}], s{S_WO[0][0]} offen offset:{pp * 1024}")
        stage_chunk0(kn)
        for setn in (1, 0):
            setup_load_at_patch_start(kn)
            halo_loads(kn, setn)
        if kn.head:
            kn.E("; only-head {")
            emit_head_prologue(kn)
            kn.E("; }")
    else:
        stage_chunk0(kn)
        setup_load_at_patch_start(kn)
        halo_loads(kn)                                   # chunk 1 -> halo registers
        # weight pieces of chunk 0
        kn.E(f"s_mov_b32 s{S_WO[0][0]}, 0")
        kn.E(f"s_mov_b32 s{S_WO[0][1]}, s{S_NTSTRIDE}")
        kn.E(f"s_mov_b32 s{S_WO[1][0]}, 0xc00")
        kn.E(f"s_add_u32 s{S_WO[1][1]}, s{S_NTSTRIDE}, 0xc00")
        for jj in range(2):
            for nt in range(2):
                for p in range(3):
                    kn.E(weight_load(jj, nt, p))
    kn.E("s_waitcnt lgkmcnt(0)")
    kn.E("s_barrier")


def stage_chunk0(kn):
    """the first patch's chunk 0: halo -> registers -> slot 4 (the other buffer; the addresses flip there and back)"""
    setup_load(kn)
    halo_loads(kn)
    emit(kn, flip_ops(VHST))
    kn.E("s_waitcnt vmcnt(0)")
    emit(kn, halo_store_ops(0))
    emit(kn, flip_ops(VHST))


def emit_head_prologue(kn):
    """head-fused form: the arguments behind the plain kernels' block, the lane constants and the loop-invariant scalars.  Runs behind
    the last weight-piece load, so the weight descriptor's and the prologue constants' registers are free.  Nothing waits for the
    lane-constant loads here: the first finishing pass waits vmcnt(0) in front of its arithmetic."""
    t = S_T
    kn.E(f"s_load_dwordx4 s[{t[0]}:{t[3]}], s[0:1], 0x78")          # head weight (ncls, 32), head bias
    kn.E(f"s_load_dwordx2 s[{S_LOGP}:{S_LOGP + 1}], s[0:1], 0x88")
    kn.E(f"s_load_dwordx2 s[{S_PSR}:{S_PSR + 1}], s[0:1], 0x90")
    kn.E(f"s_load_dword s{S_NCLS}, s[0:1], 0x98")
    kn.E(f"s_load_dword s{S_PSR + 2}, s[0:1], 0x9c")                # bytes of the patch-sum scratch
    kn.E("s_waitcnt lgkmcnt(0)")
    kn.E(f"s_mov_b32 s{t[4]}, s{t[0]}")
    desc_mask(kn, t[4], t[0])
    kn.E(f"s_lshl_b32 s{t[6]}, s{S_NCLS}, 7")                        # a class past ncls reads zeros
    kn.E(f"s_mov_b32 s{t[7]}, 0x00020000")
    kn.E(f"v_and_b32_e32 v1, 7, v{VTID}")                            # channel quad of the finishing unit
    kn.E("v_lshlrev_b32_e32 v2, 4, v1")
    for k in range(4):
        kn.E(f"buffer_load_dwordx4 {vr(WQ(k, 0), 4)}, v2, s[{t[4]}:{t[7]}], 0 offen offset:{k * 128}")
    kn.E(f"s_mov_b32 s{t[4]}, s{t[2]}")
    desc_mask(kn, t[4], t[2])
    kn.E(f"s_lshl_b32 s{t[6]}, s{S_NCLS}, 2")
    kn.E("v_cmp_eq_u32_e32 vcc, 0, v1")
    kn.E(f"v_mov_b32_e32 v2, s{S_OOB}")
    kn.E("v_mov_b32_e32 v3, 0")
    kn.E("s_nop 1")
    kn.E("v_cndmask_b32_e32 v2, v2, v3, vcc")
    for k in range(4):
        kn.E(f"buffer_load_dword v{BL(k)}, v2, s[{t[4]}:{t[7]}], 0 offen offset:{k * 4}")
    kn.E(f"s_lshl_b32 s{S_NCLS4}, s{S_NCLS}, 2")
    kn.E(f"s_mul_i32 s{S_WNCLS4}, s{S_W}, s{S_NCLS4}")
    kn.E(f"s_mul_i32 s{S_LOGIMGB}, s{S_H}, s{S_WNCLS4}")
    kn.E(f"s_mov_b32 s{S_LGR + 2}, s{S_LOGIMGB}")
    kn.E(f"s_mov_b32 s{S_LGR + 3}, 0x00020000")
    kn.E(f"s_lshr_b32 s{S_NPW}, s{S_W}, 4")
    kn.E(f"s_lshr_b32 s{S_NPIMG}, s{S_H}, 4")
    kn.E(f"s_mul_i32 s{S_NPIMG}, s{S_NPIMG}, s{S_NPW}")
    desc_mask(kn, S_PSR)
    kn.E(f"s_mov_b32 s{S_PSR + 3}, 0x00020000")
    kn.E(f"v_and_b32_e32 v1, 63, v{VTID}")
    kn.E("v_xor_b32_e32 v2, 16, v1")
    kn.E(f"v_lshlrev_b32_e32 v{VBP16}, 2, v2")
    kn.E("v_xor_b32_e32 v2, 32, v1")
    kn.E(f"v_lshlrev_b32_e32 v{VBP32}, 2, v2")


def emit_first_form(kn, jp):
    """step 0 of the first chunk (no MFMAs to hide behind)"""
    emit(kn, raw_reads(jp, 0, 0, 0) + raw_reads(jp, 0, 0, 1))
    kn.E("s_waitcnt lgkmcnt(0)")
    for hf in range(2):
        emit(kn, form_valu(jp, 0, 0, hf, kn))
    emit(kn, raw_reads(jp, *step_jm(1), 0))


def emit_kernel(kn):
    jp1 = f".Ljp1_{kn.name}"
    kn.o.begin_kernel(kn.name)
    emit_prologue(kn)
    kn.E(f"s_cmp_lg_u32 s{S_JP}, 0")
    kn.E(f"s_cbranch_scc1 {jp1}")
    emit_first_form(kn, 0)
    emit_patch_loop(kn, 0)
    kn.L(jp1)
    emit_first_form(kn, 1)
    emit_patch_loop(kn, 1)
    kn.L(kn.end)
    kn.E("s_endpgm")
    kn.o.end_kernel(kn.name, LDS_BYTES, VGPRS, SGPRS, HEAD_KERNARG if kn.head else KERNARG, THREADS)


def generate(head):
    """the text of one code object: the head-fused kernel (a code object of its own), or the wide kernel and the two narrow kernels
    (32 output channels, the layer's 2 / 4 chunks of weight pieces resident)"""
    o = Stream()
    for name, ntb, nc in ([("mgu_wino_cp1r2h_gfx950", 1, 2)] if head else
                          [(WIDE.name, 2, None), ("mgu_wino_cp1r2_gfx950", 1, 2), ("mgu_wino_cp1r4_gfx950", 1, 4)]):
        emit_kernel(Kernel(name, ntb, nc, head, o))
    return o.text()


def main():
    ap = argparse.ArgumentParser(description="gfx950 assembly of the component-pair Winograd kernels")
    ap.add_argument("--head", action="store_true", help="the head-fused 2-chunk narrow kernel instead of the three plain kernels")
    ap.add_argument("out", metavar="OUT.s")
    args = ap.parse_args()
    with open(args.out, "w") as f:
        f.write(generate(args.head))


if __name__ == "__main__":
    main()
