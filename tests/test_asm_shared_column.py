"""The shared tile column of the assembly Winograd kernels (csrc/asm/gen_wino_cp.py, CPU only): a chunk runs its steps in the
order (jj, mi) = (0,0), (1,0), (0,1), (1,1), the jj = 0 forming leaves the column both components of a pair share in the raw
registers, and the jj = 1 forming of the same mi reuses it.  Counts of the generated loops, and the lint rule
(csrc/asm/lint_wino_asm.py) that catches a shared sum overwritten before the jj = 1 forming reads it."""
import re

from asm_gen import generate, load as _load


def _generate(tmp_path, patch=None):
    return generate(patch=patch)            # in this process: the seeded faults hook the module


def _kernels(text):
    return _load("lint_wino_asm").kernels(text)


def test_generator_is_deterministic(tmp_path):
    text, gen = _generate(tmp_path)
    # the same module again, the other code object in between: a generation leaves nothing behind (label numbers restart)
    head = gen.generate(True)
    assert gen.generate(False) == text and gen.generate(True) == head
    assert _generate(tmp_path)[0] == text      # and a fresh module writes the same


def test_jj1_steps_read_and_form_only_their_own_column(tmp_path):
    _, gen = _generate(tmp_path)
    for jp in range(2):
        for mi in range(2):
            for hf in range(2):
                assert len(gen.raw_reads(jp, 0, mi, hf)) == 4 and len(gen.raw_reads(jp, 1, mi, hf)) == 2
                # the jj = 1 reads never land on the c quad that carries the shared inner sum
                c = gen.vr(gen.RAW(hf, 2), 4)
                assert not any(r.split()[1].rstrip(",") == c for r in gen.raw_reads(jp, 1, mi, hf))
            assert len(gen.form_valu(jp, 0, 0, 0)) == 34 and len(gen.form_valu(jp, 1, 0, 0)) == 30
    assert [gen.step_jm(s) for s in range(4)] == [(0, 0), (1, 0), (0, 1), (1, 1)]


def test_chunk_loop_counts(tmp_path):
    text, _ = _generate(tmp_path)
    lint = _load("lint_wino_asm")
    body = {}
    for name, lines in _kernels(text).items():
        for lab, b in lint.loop_bodies(lines):
            if lab.startswith(".chunk"):
                body.setdefault(name, []).append("\n".join(b))
    # the wide kernel's chunk loop (one per component pair): 48 MFMAs, 24 ds_read_b128 (2 x 8 for the jj = 0 steps, 2 x 4 for the
    # jj = 1 steps; 32 before the column was shared), 48 inner-sum v_fmac (64 before)
    assert len(body["mgu_wino_cp2_gfx950"]) == 2
    for b in body["mgu_wino_cp2_gfx950"]:
        assert len(re.findall(r"\bv_mfma_", b)) == 48
        assert len(re.findall(r"\bds_read_b128\b", b)) == 24
        assert len(re.findall(r"\bv_fmac_f32_e32\b", b)) == 48


def test_lint_catches_an_overwritten_shared_sum(tmp_path):
    lint = _load("lint_wino_asm")
    text, _ = _generate(tmp_path)
    assert lint.check(text) == ([], 3)

    def onto_c_quad(gen):
        # seeded fault: the jj = 1 step's first read lands on the c quad, on top of the shared inner sum
        orig = gen.raw_reads

        def raw_reads(jp, jj, mi, hf):
            r = orig(jp, jj, mi, hf)
            if jj == 1:
                r[0] = r[0].replace(gen.vr(gen.RAW(hf, 0), 4), gen.vr(gen.RAW(hf, 2), 4), 1)
            return r
        gen.raw_reads = raw_reads
    bad, _ = _generate(tmp_path, onto_c_quad)
    errs = lint.check(bad)[0]
    assert any("combines an inner sum" in e for e in errs), errs[:3]

    def epilogue_on_c_quad(gen):
        # seeded fault: the patch epilogue's temporaries on raw half 1's c quad (the register map before the column was shared)
        orig = gen.emit_epilogue_wide

        def emit_epilogue_wide(kn, jp):
            n0 = len(kn.o.lines)
            orig(kn, jp)
            kn.o.lines[n0:] = [re.sub(r"\bv212\b", "v224", ln) for ln in kn.o.lines[n0:]]
        gen.emit_epilogue_wide = emit_epilogue_wide
    bad, _ = _generate(tmp_path, epilogue_on_c_quad)
    errs = lint.check(bad)[0]
    assert any("combines an inner sum" in e and "v224" in e for e in errs), errs[:3]
