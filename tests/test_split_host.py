"""CPU tier of the three-piece product tests: where the bars of tests/test_gpu_split_kernels.py come from, and the proof that those
bars can fail.

For every (family, shape, operand case) of the GPU module's table the product is evaluated on the CPU three ways, each measured
against float64 in units of sum |a b| (split_oracle.err_units):
  e_six    the six-product emulation (direct form; Winograd form for the Winograd families),
  e_ref32  plain fp32 on the CPU: torch's fp32 conv_transpose2d / conv2d / matmul, or the fp32 Winograd restatement,
  e_mut    the emulation with piece products removed (split_oracle.MUTANTS), for the mutants the case is designated to catch.
A designated mutant must sit at least 16 x above max(e_six, e_ref32); BAR is a quarter of the smallest designated e_mut, or
4 max(e_six, e_ref32) for a case that designates none.  No GPU result enters a bar."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import split_oracle as SO
import test_gpu_split_kernels as T

SEPARATION = 16.0


@functools.lru_cache(maxsize=None)
def reference(oracle, shape, case):
    """(float64 result, float64 scale) of the family's operation on the case's operands."""
    fam = SO.FAMILY[oracle]
    return fam.ref64(shape, *fam.make(shape, case))


def ref32(oracle, shape, a, b):
    """The operation in plain fp32 on the CPU."""
    fam = SO.FAMILY[oracle]
    if fam.winograd:
        return fam.emulate(shape, a, b, None)
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    if oracle == "convt_fwd":
        return F.conv_transpose2d(ta, tb, stride=2).numpy()
    if oracle == "convt_dgrad":           # the adjoint of conv_transpose2d(x, w, stride 2) is conv2d(dout, w, stride 2)
        return F.conv2d(ta, tb, stride=2).numpy()
    if oracle == "first_conv":
        return F.relu(F.conv2d(ta, tb, padding=1)).numpy()
    if oracle == "gat_linear":
        N, Fin, Fh, heads, concat = shape
        y = F.elu(ta[torch.from_numpy(fam.src(N))] @ tb.t())
        return (y if concat else y.view(N, heads, Fh).mean(1)).numpy()
    if oracle == "gat_attention":        # the float32 run of the oracle's per-head forward (it multiplies first, then aggregates)
        import mgunet_oracle as O
        N, Fin, Fh, heads, concat = shape
        ei, att = torch.from_numpy(np.stack(fam.edges(N))), torch.from_numpy(fam.att(shape))
        hs = [O.gat_head_forward(ta, ei, tb[h * Fh:(h + 1) * Fh], att[h:h + 1], 0.2) for h in range(heads)]
        return (torch.cat(hs, 1) if concat else torch.stack(hs).mean(0)).numpy()
    raise KeyError(oracle)


@functools.lru_cache(maxsize=None)
def evaluate(oracle, shape, case):
    """e_six, e_ref32 and every mutant's error for one (oracle family, shape, case)."""
    fam = SO.FAMILY[oracle]
    a, b = fam.make(shape, case)
    ref, scale = reference(oracle, shape, case)
    out, by_kept = {}, {}
    for name, kept in SO.MUTANTS.items():
        if kept not in by_kept:           # a2_zero / b2_zero keep the same products as drop_a2b0 / drop_a0b2
            by_kept[kept] = SO.err_units(fam.emulate(shape, a, b, kept), ref, scale)
        out[name] = by_kept[kept]
    return dict(e_six=SO.err_units(fam.emulate(shape, a, b), ref, scale), e_ref32=SO.err_units(ref32(oracle, shape, a, b), ref, scale), e_mut=out)


def floor(ev):
    return max(ev["e_six"], ev["e_ref32"])


class _Bars:
    """BAR[family, shape, case]: the only bars the GPU tests use."""

    def __getitem__(self, key):
        family, shape, case = key
        ev, want = evaluate(T.FAMILIES[family]["oracle"], shape, case), T.designated(family, case)
        return min(ev["e_mut"][m] for m in want) / 4 if want else 4 * floor(ev)


BAR = _Bars()
ALL = [pytest.param(f, s, c, id=f"{f}-{'-'.join(map(str, s))}-{c}") for f in T.FAMILIES for s in T.FAMILIES[f]["shapes"] for c in T.FAMILIES[f]["cases"]]


@pytest.mark.parametrize("family,shape,case", ALL)
def test_designated_mutants_are_separated_and_rejected(family, shape, case):
    oracle = T.FAMILIES[family]["oracle"]
    fam, ev = SO.FAMILY[oracle], evaluate(oracle, shape, case)
    want, bar = T.designated(family, case), BAR[family, shape, case]
    print(f"{family} {shape} {case}: e_six {ev['e_six']:.2e} e_ref32 {ev['e_ref32']:.2e} bar {bar:.2e} "
          + " ".join(f"{m}={ev['e_mut'][m] / floor(ev):.0f}x" for m in want))
    a, b = fam.make(shape, case)
    ref, scale = reference(oracle, shape, case)
    # what a correct kernel computes passes, with the headroom the bar promises
    assert SO.passes(fam.emulate(shape, a, b), ref, scale, bar) and 4 * floor(ev) <= bar
    if case == "integers":
        assert ev["e_ref32"] == 0 or oracle == "gat_linear"      # (ELU of a negative integer is not exact)
    for m in want:
        assert ev["e_mut"][m] >= SEPARATION * floor(ev), (m, ev["e_mut"][m], floor(ev))
        # the predicate the GPU tests call rejects the mutant's result
        assert not SO.passes(fam.emulate(shape, a, b, SO.MUTANTS[m]), ref, scale, bar), m


@pytest.mark.parametrize("family", list(T.FAMILIES))
def test_every_mutant_is_designated_in_every_family(family):
    caught = {m for case in T.FAMILIES[family]["cases"] for m in T.designated(family, case)}
    assert caught == set(SO.MUTANTS)
    if not T.FAMILIES[family].get("extra"):      # (an extra entry adds a case to a family that has the full set)
        assert {"full_mantissa", "positive_low_bits", "bf16_exact", "integers"} <= set(T.FAMILIES[family]["cases"])


def test_split_restates_device_h():
    rng = np.random.default_rng(1)
    a = np.concatenate([rng.standard_normal(4096).astype(np.float32) * np.float32(2.0) ** rng.integers(-60, 60, 4096).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, -1.0, 3.4e38, 1e-30, 1 + 2.0 ** -23, 1 - 2.0 ** -24], np.float32)])
    p = SO.split3(a)
    for q in p:                               # every piece is a bf16 value
        assert np.all(q.view(np.uint32) & np.uint32(0xffff) == 0)
    assert np.all(np.abs(p[1]) <= np.abs(p[0]) * 2.0 ** -7) and np.all(np.abs(p[2]) <= np.abs(p[0]) * 2.0 ** -14)


def test_winograd_restatements_are_the_convolutions():
    """The piece-arithmetic Winograd forms against the direct float64 sums, on integers (exact) and on normal data."""
    for case, tol in (("integers", 0.0), ("normal", 1e-6)):
        for name, shape in (("wino_fwd", (2, 6, 8, 16, 8)), ("wino_dgrad", (1, 4, 6, 8, 16)), ("wino_wgrad", (2, 4, 8, 8, 16))):
            fam = SO.FAMILY[name]
            a, b = fam.make(shape, case)
            ref, scale = fam.ref64(shape, a, b)
            for kept in (SO.SIX, None):
                assert SO.err_units(fam.emulate(shape, a, b, kept), ref, scale) <= tol, (name, case, kept)


def test_gemm_forms_are_the_framework_operations():
    """The GEMM layouts of the direct families (column order of the pixel shuffle, the tap-major k of the data gradient, the slot order
    of the first convolution) against torch in float64."""
    for name, shape in (("convt_fwd", (2, 3, 5, 16, 8)), ("convt_dgrad", (2, 3, 5, 16, 8)), ("first_conv", (1, 5, 7, 3, "nchw")),
                        ("first_conv", (1, 5, 7, 2, "nchw"))):
        fam = SO.FAMILY[name]
        a, b = fam.make(shape, "normal")
        ta, tb = torch.from_numpy(a).double(), torch.from_numpy(b).double()
        want = {"convt_fwd": lambda: F.conv_transpose2d(ta, tb, stride=2), "convt_dgrad": lambda: F.conv2d(ta, tb, stride=2),
                "first_conv": lambda: F.relu(F.conv2d(ta, tb, padding=1))}[name]().numpy()
        assert np.allclose(fam.ref64(shape, a, b)[0], want, rtol=0, atol=1e-12)


def test_identity_fold_of_the_first_block():
    """The first-convolution test folds both BatchNorms to scale 1: gamma / sqrtf(var + 1e-5f) with gamma = 1 in float32."""
    v = np.float32(T.identity_variance())
    assert np.float32(v + np.float32(1e-5)) == np.float32(1) and np.float32(1) / np.sqrt(np.float32(v + np.float32(1e-5))) == np.float32(1)


# ---- why these tests exist ----------------------------------------------------------------------------------------------------------
def test_the_suites_relative_bar_accepts_lost_products():
    """On N(0,1) x U(-0.2, 0.2) operands the 2e-5 max(1, max |ref|) bar of the convolution tests accepts a kernel without a1 b1, and
    one with two pieces per operand (four products); in units of sum |a b| both are an order of magnitude off."""
    rng = np.random.default_rng(7)
    for K in (64, 512):
        A, B = rng.standard_normal((96, K)).astype(np.float32), rng.uniform(-0.2, 0.2, (K, 64)).astype(np.float32)
        ref, scale = A.astype(np.float64) @ B.astype(np.float64), np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)
        six = SO.err_units(SO.piece_gemm(A, B), ref, scale)
        for m in ("drop_a1b1", "two_pieces"):
            got = SO.piece_gemm(A, B, SO.MUTANTS[m])
            assert np.abs(got - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max()), (m, K)
            assert SO.err_units(got, ref, scale) >= 8 * six, (m, K)


def test_old_tiny_residuals_construction_has_no_third_piece():
    """bf16(x) (1 + 2^-23): the split truncates, so the residual after the first piece is the one low bit and the SECOND piece holds
    it; the third piece is zero, and with it on both operands even the two-piece mutant computes the same bytes."""
    x = torch.randn((2, 64, 24, 40), generator=torch.Generator().manual_seed(5))
    x = (x.bfloat16().float() * (1 + 2.0 ** -23)).numpy()
    p0, p1, p2 = SO.split3(x)
    assert np.all(p2 == 0) and np.any(p1 != 0)
    A, B = x[0, :, 0, :].T.copy(), x[1, :, 0, :].copy()
    assert np.array_equal(SO.piece_gemm(A, B), SO.piece_gemm(A, B, SO.MUTANTS["two_pieces"]))
