"""What a generator of hand-scheduled gfx950 assembly needs besides its own register map and schedule: the output stream of one
code object (instructions, labels, kernel header, kernel descriptor, metadata), and a few instruction sequences that are the same
in every kernel.  The helpers take `o`, anything with the stream's E / L / newlabel.  gen_wino_cp.py is the first user."""


def vr(b, n=1):
    return f"v{b}" if n == 1 else f"v[{b}:{b + n - 1}]"


class Stream:
    """The text of one code object.  All state of a generation lives here: two streams never share anything."""
    def __init__(self, target="amdgcn-amd-amdhsa--gfx950"):
        self.target = target
        self.lines = [f'\t.amdgcn_target "{target}"']
        self.meta = []
        self.nlabel = 0

    def E(self, s=""):
        self.lines.append("\t" + s if s and not s.endswith(":") else s)

    def L(self, s):
        self.lines.append(s + ":")

    def newlabel(self, p="L"):
        self.nlabel += 1
        return f".{p}_{self.nlabel}"

    def begin_kernel(self, name):
        self.nlabel += 1000               # the label numbers of a kernel tell which kernel of the code object it is
        self.lines.append(f"""\t.text
\t.protected\t{name}
\t.globl\t{name}
\t.p2align\t8
\t.type\t{name},@function
{name}:""")

    def end_kernel(self, name, lds_bytes, vgprs, sgprs, kernarg_bytes, max_threads):
        """kernel descriptor and metadata entry of a kernel that takes its arguments as one by-value block, uses no scratch and
        gets the kernarg pointer in s[0:1] and the workgroup id x in s2.  sgprs: the kernel's own (next free); the metadata counts
        the six of VCC, FLAT_SCRATCH and XNACK_MASK on top"""
        fe = f".Lfunc_end_{name}"
        self.lines.append(f"""\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size {lds_bytes}
\t\t.amdhsa_private_segment_fixed_size 0
\t\t.amdhsa_kernarg_size {kernarg_bytes}
\t\t.amdhsa_user_sgpr_count 2
\t\t.amdhsa_user_sgpr_dispatch_ptr 0
\t\t.amdhsa_user_sgpr_queue_ptr 0
\t\t.amdhsa_user_sgpr_kernarg_segment_ptr 1
\t\t.amdhsa_user_sgpr_dispatch_id 0
\t\t.amdhsa_user_sgpr_kernarg_preload_length 0
\t\t.amdhsa_user_sgpr_kernarg_preload_offset 0
\t\t.amdhsa_user_sgpr_private_segment_size 0
\t\t.amdhsa_uses_dynamic_stack 0
\t\t.amdhsa_enable_private_segment 0
\t\t.amdhsa_system_sgpr_workgroup_id_x 1
\t\t.amdhsa_system_sgpr_workgroup_id_y 0
\t\t.amdhsa_system_sgpr_workgroup_id_z 0
\t\t.amdhsa_system_sgpr_workgroup_info 0
\t\t.amdhsa_system_vgpr_workitem_id 0
\t\t.amdhsa_next_free_vgpr {vgprs}
\t\t.amdhsa_next_free_sgpr {sgprs}
\t\t.amdhsa_accum_offset {vgprs}
\t\t.amdhsa_reserve_vcc 1
\t\t.amdhsa_float_round_mode_32 0
\t\t.amdhsa_float_round_mode_16_64 0
\t\t.amdhsa_float_denorm_mode_32 3
\t\t.amdhsa_float_denorm_mode_16_64 3
\t\t.amdhsa_dx10_clamp 1
\t\t.amdhsa_ieee_mode 1
\t\t.amdhsa_fp16_overflow 0
\t\t.amdhsa_tg_split 0
\t.end_amdhsa_kernel
\t.text
{fe}:
\t.size\t{name}, {fe}-{name}
""")
        self.meta.append(f"""  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           {kernarg_bytes}
        .value_kind:     by_value
    .group_segment_fixed_size: {lds_bytes}
    .kernarg_segment_align: 8
    .kernarg_segment_size: {kernarg_bytes}
    .max_flat_workgroup_size: {max_threads}
    .name:           {name}
    .private_segment_fixed_size: 0
    .sgpr_count:     {sgprs + 6}
    .sgpr_spill_count: 0
    .symbol:         {name}.kd
    .uniform_work_group_size: 1
    .uses_dynamic_stack: false
    .vgpr_count:     {vgprs}
    .vgpr_spill_count: 0
    .wavefront_size: 64""")

    def text(self):
        """the whole code object: the kernels, then the metadata of all of them"""
        tail = ["\t.amdgpu_metadata\n---\namdhsa.kernels:"] + self.meta + [f"""amdhsa.target:   {self.target}
amdhsa.version:
  - 1
  - 2
...

\t.end_amdgpu_metadata
"""]
        return "\n".join(self.lines + tail) + "\n"


def divmod_magic(o, n, d, mg, q, r, t0, t1):
    """q = n / d, r = n % d  (scalar; mg = floor(2^32 / d), n * d < 2^32)"""
    o.E(f"s_mul_hi_u32 s{q}, s{n}, s{mg}")
    o.E(f"s_mul_i32 s{t0}, s{q}, s{d}")
    o.E(f"s_sub_u32 s{r}, s{n}, s{t0}")
    o.E(f"s_add_u32 s{t0}, s{q}, 1")
    o.E(f"s_sub_u32 s{t1}, s{r}, s{d}")
    o.E(f"s_cmp_ge_u32 s{r}, s{d}")
    o.E(f"s_cselect_b32 s{q}, s{t0}, s{q}")
    o.E(f"s_cselect_b32 s{r}, s{t1}, s{r}")


def desc_mask(o, dst, src=None):
    """high word of the base in s[dst:dst+1] of a buffer descriptor: the 16 address bits of s[src:src+1] (default: its own), stride 0"""
    o.E(f"s_and_b32 s{dst + 1}, s{(dst if src is None else src) + 1}, 0xffff")


def desc_base(o, dst, base, index, nbytes, t0, t1, mask=True):
    """descriptor = base + index x bytes: s[dst:dst+1] = s[base:base+1] + s_index * s_nbytes (64-bit).  mask = False: the caller
    adds more to the base and calls desc_mask itself"""
    o.E(f"s_mul_i32 s{t0}, s{index}, s{nbytes}")
    o.E(f"s_mul_hi_u32 s{t1}, s{index}, s{nbytes}")
    o.E(f"s_add_u32 s{dst}, s{base}, s{t0}")
    o.E(f"s_addc_u32 s{dst + 1}, s{base + 1}, s{t1}")
    if mask:
        desc_mask(o, dst)


def pk2(op, d, a, b, neg_a=False, neg_b=False):
    """two fp32 operations per lane in one VOP3P instruction on even-aligned register pairs (bit-identical to the scalar forms).
    Next to an MFMA in flight the packed forms wait for the matrix pipe (tools/ubench): for code outside the MFMA loops."""
    assert d % 2 == 0 and a % 2 == 0 and b % 2 == 0
    mod = ""
    if neg_a or neg_b:
        mod = f" neg_lo:[{int(neg_a)},{int(neg_b)}] neg_hi:[{int(neg_a)},{int(neg_b)}]"
    return f"v_pk_{op}_f32 v[{d}:{d + 1}], v[{a}:{a + 1}], v[{b}:{b + 1}]{mod}"


def pkfma2(d, a, b, c):
    assert d % 2 == 0 and a % 2 == 0 and b % 2 == 0 and c % 2 == 0
    return f"v_pk_fma_f32 v[{d}:{d + 1}], v[{a}:{a + 1}], v[{b}:{b + 1}], v[{c}:{c + 1}]"
