"""The head-fused form of the 2-chunk narrow Winograd kernel (csrc/asm/gen_wino_cp.py --head) is a stream of its own: the same lint
(csrc/asm/lint_wino_asm.py) replays it, its main loop is the plain kernel's instruction for instruction, and the rules its
cross-lane folds add (two wait states in front of a DPP operand, ds_bpermute results counted in lgkmcnt) catch seeded faults.  CPU only."""
import re

from asm_gen import load, run_cli as _generate


def _lint():
    return load("lint_wino_asm")


def _kernel(text, name):
    return text[text.index(name + ":"):text.index(".Lfunc_end_" + name)]


def test_head_stream_passes_the_lint(tmp_path):
    text = _generate(tmp_path, "--head")
    errs, n = _lint().check(text)
    assert n == 1 and not errs, errs[:5]
    assert "mgu_wino_cp1r2h_gfx950:" in text
    mnemonics = {l.split()[0] for l in text.split("\n") if l.startswith("\t") and not l.startswith("\t.")}
    assert not [m for m in mnemonics if m.startswith("s_") and re.search(r"store|atomic|dcache", m)]   # no scalar memory writes
    assert ".amdhsa_next_free_vgpr 256" in text and ".amdhsa_group_segment_fixed_size 163840" in text   # no new registers, no new LDS
    used = {int(r) for r in re.findall(r"\bv(\d+)\b", text)} | {int(b) for a, b in re.findall(r"v\[(\d+):(\d+)\]", text)}
    assert max(used) <= 255


def _common_stream(text, name):
    """the kernel's instruction stream with the blocks the generator marks as belonging to one form only (`; only-head {` /
    `; only-plain {` ... `; }`) cut out, label numbers and the kernel's name normalised"""
    out, skip = [], False
    for l in _kernel(text, name).split("\n")[1:]:
        t = l.strip()
        if t.startswith("; only-"):
            assert not skip
            skip = True
        elif t == "; }":
            assert skip
            skip = False
        elif not skip and t:
            out.append(re.sub(r"\.(\w+?)_\d+\b", r".\1", t).replace(name, "KERNEL"))
    assert not skip
    return out


def test_everything_outside_the_marked_blocks_is_the_plain_kernel(tmp_path):
    """Instruction for instruction -- waits, wait states, transform VALU, stores and branches included: what the head-fused form adds
    is its prologue insert, the logit / patch-sum address arithmetic in place of the pooled-tensor one, and the block behind the
    feature stores in place of the fused pool."""
    plain_text, head_text = _generate(tmp_path), _generate(tmp_path, "--head")
    plain = _common_stream(plain_text, "mgu_wino_cp1r2_gfx950")
    head = _common_stream(head_text, "mgu_wino_cp1r2h_gfx950")
    assert len(plain) == len(head) > 3000 and plain.index("s_endpgm") == head.index("s_endpgm")
    diff = [(a, b) for a, b in zip(plain, head) if a != b]   # the kernel descriptor follows s_endpgm: only the argument block grows
    assert diff == [(".amdhsa_kernarg_size 120", ".amdhsa_kernarg_size 160")], diff[:5]
    # the marked blocks of the head form hold no MFMA, no barrier, no LDS write and none of the feature stores
    inside, skip = [], False
    for l in _kernel(head_text, "mgu_wino_cp1r2h_gfx950").split("\n"):
        t = l.strip()
        skip = True if t.startswith("; only-head") else False if t == "; }" else skip
        if skip:
            inside.append(t)
    assert inside and not [t for t in inside if re.match(r"v_mfma|s_barrier|ds_write|ds_read", t) or " nt" in t]


def test_lint_catches_seeded_faults_in_the_folds(tmp_path):
    lint, text = _lint(), _generate(tmp_path, "--head")
    # the patch-sum fold's DPP reads registers a packed add wrote two instructions earlier: without the s_nop it is one wait state short
    no_states = "\n".join(l for l in text.split("\n") if l.strip() != "s_nop 1")
    assert any("(DPP)" in e for e in lint.check(no_states)[0])
    # a bpermute result read before its wait
    i = text.index("ds_bpermute_b32")
    j = text.index("s_waitcnt lgkmcnt(0)", i)
    early = text[:j] + "s_nop 0" + text[j + len("s_waitcnt lgkmcnt(0)"):]
    assert any("ds_bpermute_b32" in e and "outstanding" in e for e in lint.check(early)[0])
