"""The hand-scheduled ConvTranspose assembly (csrc/asm/gen_convt_x3.py) carries no compiler-inserted waits.  csrc/asm/lint_wino_asm.py
replays the generated stream with the machine's in-order counters (its Winograd shared-sum rule switched off: this stream has no
such sums); CPU only.  The lint must pass what the generator emits now and catch the seeded faults."""
import re

from asm_gen import load as _load

MFMA = r"v_mfma_f32_32x32x16_bf16"


def _stream():
    return _load("gen_convt_x3").generate()


def test_generated_stream_passes_the_lint():
    lint = _load("lint_wino_asm")
    text = _stream()
    errs, n = lint.check(text, shared_sum=False)
    assert n == 1 and not errs, errs[:5]
    # two K = 32 steps per trip of the loop, 48 MFMAs each, six per accumulator and half step in the C++ kernel's order
    assert len(re.findall(MFMA, text)) == 2 * 48
    first6 = re.findall(MFMA + r" v\[0:15\], v\[(\d+):\d+\], v\[(\d+):\d+\], v\[0:15\]", text)[:6]
    gen = _load("gen_convt_x3")
    assert [(int(a), int(b)) for a, b in first6] == [(gen.PA(0, 0, pa), gen.BR(0, pb)) for pa, pb in ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))]
    # the loop: one barrier per step, and nothing but vector memory instructions, LDS operations and scalar ALU between the MFMAs
    loop = text[text.index(".step_"):text.rindex(".store_")]
    assert loop.count("s_barrier") == 2 and "s_load" not in loop
    # at most two ds_read_b128 and three VALU operations in a gap
    for gap in re.split(MFMA + r"[^\n]*\n", loop)[1:]:
        ops = [l.split()[0] for l in gap.split("\n") if l.strip() and not l.strip().startswith((".", "s_"))]
        assert sum(o == "ds_read_b128" for o in ops) <= 2 and sum(o.startswith("v_") for o in ops) <= 3, gap


def test_lint_catches_seeded_faults():
    lint = _load("lint_wino_asm")
    text = _stream()
    dropped = text.replace("s_waitcnt vmcnt(4) lgkmcnt(0)", "s_waitcnt lgkmcnt(0)")           # the weight pieces of a step's first half
    assert dropped != text and lint.check(dropped, shared_sum=False)[0]
    weak = text.replace("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier", "s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier")   # ... of its second half
    assert weak != text and lint.check(weak, shared_sum=False)[0]
    weak_lds = text.replace("s_waitcnt vmcnt(4) lgkmcnt(0)", "s_waitcnt vmcnt(4) lgkmcnt(2)")  # the operand pieces read from LDS
    assert lint.check(weak_lds, shared_sum=False)[0]
    # an accumulator read directly behind the MFMA that wrote it: the epilogue's + shift without its wait states
    last = [m for m in re.finditer(MFMA + r"[^\n]*\n", text)][-1]
    early = text[:last.end()] + "\tv_add_f32_e32 v63, v63, v229\n" + text[last.end():]
    errs = lint.check(early, shared_sum=False)[0]
    assert any("MFMA result" in e for e in errs)
