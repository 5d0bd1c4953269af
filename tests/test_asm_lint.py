"""The hand-scheduled Winograd assembly (csrc/asm/gen_wino_cp.py) carries no compiler-inserted waits: every s_waitcnt count and
every wait state is the generator's.  csrc/asm/lint_wino_asm.py replays the generated stream with the machine's in-order counters;
this test (CPU only: it needs neither a GPU nor the assembler) runs it on what the generator emits now and on deliberately broken
streams -- the lint must pass the first and catch the seeded faults."""
import re

from asm_gen import load as _load, run_cli as _generate


def test_generated_streams_pass_the_lint(tmp_path):
    lint = _load("lint_wino_asm")
    text = _generate(tmp_path)
    errs, n = lint.check(text)
    assert n == 3 and not errs, errs[:5]          # the wide kernel and the two narrow kernels
    # two component-pair code paths each; wide: the peeled first chunk + the chunk loop (48 MFMAs per chunk); narrow: 24 per unrolled chunk
    assert len(re.findall(r"v_mfma_f32_32x32x16_bf16", text)) == 2 * (2 * 48 + 24 * 2 + 24 * 4)
    # every accumulator chain of a patch starts from the constant 0 (no clearing pass): 8 tuples in the wide kernel, 4 in a narrow one
    assert len(re.findall(r"v_mfma_f32_32x32x16_bf16 v\[\d+:\d+\], v\[\d+:\d+\], v\[\d+:\d+\], 0\n", text)) == 2 * (8 + 4 + 4)


def test_lint_catches_seeded_faults(tmp_path):
    lint = _load("lint_wino_asm")
    text = _generate(tmp_path)
    weak_wait = text.replace("s_waitcnt vmcnt(6)", "s_waitcnt vmcnt(9)")          # the wide kernel's step-0 weight wait, as it once was
    assert weak_wait != text and lint.check(weak_wait)[0]
    no_states = "\n".join(l for l in text.split("\n") if l.strip() != "s_nop 1")   # VALU -> MFMA wait states, store-data distance
    assert lint.check(no_states)[0]
    weak_lds = text.replace("s_waitcnt lgkmcnt(0)", "s_waitcnt lgkmcnt(2)")
    assert lint.check(weak_lds)[0]
