"""The two kernels of csrc/tta.hip called directly on the MI355X, against tests/tta_oracle.py: mgu_tta_views bit for bit against
torch.flip / torch.rot90 for every flip / turn code, channel count and input layout; mgu_tta_merge bit for bit on one-hot data and
within bound(C, K) = (C + K + 4) 2^-24 of the float64 merge on random, underflowing, huge and dead-class logits, at every class-count
instantiation (<1>, <2>, <3>, <4>, and <0> at C = 5, 8 and 16), every named view table and three tables predict_tta never builds;
ties, launch-shape independence, predict_tta at 1, 3 and 5 classes, and the C-ABI refusals.

What the all-equal case found: the merge used to add the views' softmaxes sequentially in fp32, and 8 additions of fl(1/3) or fl(1/5)
end an ulp away from 8 fl(1/C) (3 fl(1/3) rounds to 1.0), so K = 8 returned 0.3333333 / 0.20000002 for all-equal logits where K = 1,
2 and 4 returned fl(1/C).  The kernel now adds the views in fp64 and rounds their mean once.

Measured on the MI355X, max |probs - merge64| over tta_oracle.LAYOUTS against bound(C, K), the worst case of each class count:
  C = 1   0        (every probability is exactly 1)
  C = 2   9.60e-08 of 4.77e-07 (K = 2, huge)        C = 5   1.29e-07 of 6.56e-07 (K = 2, huge)
  C = 3   1.32e-07 of 5.36e-07 (K = 2, huge)        C = 8   1.84e-07 of 8.34e-07 (K = 2, random)
  C = 4   1.29e-07 of 5.96e-07 (K = 2, random)      C = 16  2.07e-07 of 1.31e-06 (K = 2, random)
and per case: random 0.220, spread 0.167, huge 0.247, dead 0.208 of the bound at most; K = 8 never passed 0.079 of it (7.5e-08 of
9.54e-07 at C = 4).  These are the figures of the host emulation in tests/test_tta_oracle_host.py to the printed digits: the device's
expf costs no more than the host's exp here.  The bound is the derived one; no constant in it comes from a measurement."""
import ctypes as CT

import numpy as np
import pytest
import torch

import mgunet
import tta_oracle as TO
from mgunet import _lib
from test_gpu_tta import check_outputs, images, reference_tta, unet

pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. views ----------------------------------------------------------------------------------------------------------------------

CODES = [(f, r) for r in range(4) for f in range(4)]
# sizes of the calls each shape group's codes are cut into: every G of 1..8 occurs (the 16 codes of a square image share one shape)
G_SQUARE = {1: (1, 2, 5, 8), 3: (7, 6, 3)}
G_GROUPS = {1: ((8,), (1, 3, 4)), 3: ((2, 6), (7, 1))}


def coded_batch(B, Cc, H, W, layout, dev):
    """x[b, c, y, x] = ((b * 8 + c) * 64 + y) * 128 + x (exact in fp32), in one of three layouts; a window's surroundings hold -1"""
    b, c, y, x = torch.meshgrid(torch.arange(B), torch.arange(Cc), torch.arange(H), torch.arange(W), indexing="ij")
    val = (((b * 8 + c) * 64 + y) * 128 + x).float()
    if layout == "sliced":
        big = torch.full((B, Cc, H + 9, W + 11), -1.0)
        big[:, :, 4:4 + H, 6:6 + W] = val
        return big.to(dev)[:, :, 4:4 + H, 6:6 + W]
    val = val.to(dev)
    return val.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else val


def decode(v):
    v = int(v)
    return (v >> 16, (v >> 13) & 7, (v >> 7) & 63, v & 127) if v >= 0 else "outside the image"


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Cc", [1, 3, 4, 5])
@pytest.mark.parametrize("H,W", TO.SIZES)
def test_views_bit_for_bit(cuda, H, W, Cc, B):
    if H == W:
        calls, it = [], iter(CODES)
        for G in G_SQUARE[B]:
            calls.append([next(it) for _ in range(G)])
    else:
        calls = []
        for parity, sizes in enumerate(G_GROUPS[B]):
            it = iter([fr for fr in CODES if (fr[1] & 1) == parity])
            calls += [[next(it) for _ in range(G)] for G in sizes]
    assert sorted(fr for call in calls for fr in call) == sorted(CODES)
    for layout in ("contiguous", "channels_last", "sliced"):
        x = coded_batch(B, Cc, H, W, layout, cuda)
        strides = (CT.c_int64 * 4)(*x.stride())
        xc = x.cpu()
        for call in calls:
            G = len(call)
            Hv, Wv = (W, H) if call[0][1] & 1 else (H, W)
            out = torch.full((G * B, Cc, Hv, Wv), float("nan"), device=cuda)
            codes = (CT.c_int32 * (2 * G))(*[v for fr in call for v in fr])
            _lib.call("mgu_tta_views", cuda, x, B, Cc, H, W, strides, G, codes, out)
            got = out.cpu()
            assert not torch.isnan(got).any(), (layout, call)
            want = torch.cat([TO.view(xc, f, r) for f, r in call])
            if not torch.equal(bits(got), bits(want)):
                k = int((got != want).flatten().nonzero()[0])
                at = np.unravel_index(k, got.shape)
                pytest.fail(f"{layout} {call}: view image {at[0]} (code {call[at[0] // B]}, b = {at[0] % B}) channel {at[1]} pixel {at[2:]} "
                            f"shows source (b, c, y, x) = {decode(got.flatten()[k])}, expected {decode(want.flatten()[k])}")


# ---- 2. merge ----------------------------------------------------------------------------------------------------------------------

def run_merge(dev, groups, rows, B, C, H, W):
    """mgu_tta_merge on the per-group logits, the way mgunet.tta calls it; outputs start as NaN / -1 and must all be written.  A table
    with no view in group 0 gets a NaN-filled group-0 buffer of group 1's size: reading it shows."""
    dg = [None if g is None else g.to(dev) for g in groups]
    l0 = dg[0] if dg[0] is not None else torch.full_like(dg[1], float("nan"))
    probs = torch.full((B, H, W, C), float("nan"), device=dev)
    labels = torch.full((B, H, W), -1, device=dev, dtype=torch.int64)
    conf = torch.full((B, H, W), float("nan"), device=dev)
    tbl = (CT.c_int32 * (4 * len(rows)))(*[v for row in rows for v in row])
    _lib.call("mgu_tta_merge", dev, l0, dg[1], B, C, H, W, len(rows), tbl, probs, labels, conf)
    probs, labels, conf = probs.cpu(), labels.cpu(), conf.cpu()
    assert not torch.isnan(probs).any() and int(labels.min()) >= 0 and not torch.isnan(conf).any()    # every element written
    return probs, labels, conf


@pytest.mark.parametrize("C", TO.EXACT_CLASSES)
@pytest.mark.parametrize("name,size,B", TO.EXACT_LAYOUTS)
def test_merge_exact_on_one_hot_views(cuda, name, size, B, C):
    """logits 0 / -200: every view's fp32 softmax is exactly one-hot (expf(-200) = 0), every probability a multiple of 1 / K"""
    H, W = size
    rows, groups = TO.make("one_hot", C, name, H, W, B)
    K = len(rows)
    ref32 = TO.merge64(groups, rows, B, C, H, W).float()
    assert torch.equal(ref32 * K, torch.round(ref32 * K))
    probs, labels, conf = run_merge(cuda, groups, rows, B, C, H, W)
    assert torch.equal(bits(probs), bits(ref32))
    assert torch.equal(labels, ref32.argmax(-1))                 # the first maximal class
    assert torch.equal(bits(conf), bits(ref32.amax(-1)))


@pytest.mark.parametrize("C", TO.MERGE_CLASSES)
@pytest.mark.parametrize("case", TO.FLOAT_CASES)
@pytest.mark.parametrize("name,size,B", TO.LAYOUTS)
def test_merge_against_float64(cuda, name, size, B, case, C):
    H, W = size
    rows, groups = TO.make(case, C, name, H, W, B)
    K = len(rows)
    ref = TO.merge64(groups, rows, B, C, H, W)
    probs, labels, conf = run_merge(cuda, groups, rows, B, C, H, W)
    d = float((probs.double() - ref).abs().max())
    print(f"[tta merge C={C} K={K} {case} {name} {H}x{W} B={B}] max|d| = {d:.2e}  bound {TO.bound(C, K):.2e}  ratio {d / TO.bound(C, K):.3f}")
    assert d <= TO.bound(C, K)
    if case == "dead":
        for c in TO.dead_classes(C):
            assert bool((probs[..., c] == 0.0).all()), c
    assert torch.equal(labels, probs.argmax(-1)) and torch.equal(bits(conf), bits(probs.amax(-1)))
    keep = TO.margin(ref) > 2 * TO.bound(C, K)                   # tests/test_tta_oracle_host.py caps what this leaves out at 0.1 %
    assert torch.equal(labels[keep], ref.argmax(-1)[keep])


# ---- 3. ties -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", TO.MERGE_CLASSES)
@pytest.mark.parametrize("name,size,B", TO.LAYOUTS)
def test_equal_logits_give_exactly_one_over_c(cuda, name, size, B, C):
    H, W = size
    rows, groups = TO.make("equal", C, name, H, W, B)
    probs, labels, conf = run_merge(cuda, groups, rows, B, C, H, W)
    want = torch.full((B, H, W, C), float(np.float32(1) / np.float32(C)))
    assert torch.equal(bits(probs), bits(want)), (len(rows), sorted(set(probs.flatten().tolist())))
    assert int(labels.max()) == 0 and torch.equal(bits(conf), bits(want[..., 0]))


@pytest.mark.parametrize("C", [3, 4, 5, 8, 16])
@pytest.mark.parametrize("name,size,B", TO.LAYOUTS)
def test_a_tie_at_the_top_goes_to_the_first_class(cuda, name, size, B, C):
    H, W = size
    rows, groups = TO.make("tie_top", C, name, H, W, B)
    probs, labels, conf = run_merge(cuda, groups, rows, B, C, H, W)
    a, b = TO.tie_classes(C)
    assert torch.equal(bits(probs[..., a]), bits(probs[..., b]))
    assert bool((labels == a).all()) and torch.equal(bits(conf), bits(probs[..., a]))
    d = float((probs.double() - TO.merge64(groups, rows, B, C, H, W)).abs().max())
    assert d <= TO.bound(C, len(rows))


# ---- 4. launch shape ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 16])
@pytest.mark.parametrize("name,size", [("d4", (16, 16)), ("d4", (17, 31)), ("mixed_slots", (33, 16)), ("group1_only", (19, 1)), ("flips", (48, 64))])
def test_a_batch_is_its_images_and_a_rerun_is_identical(cuda, name, size, C):
    H, W = size
    B = 3
    rows, groups = TO.make("random", C, name, H, W, B)
    whole = run_merge(cuda, groups, rows, B, C, H, W)
    again = run_merge(cuda, groups, rows, B, C, H, W)
    assert all(torch.equal(bits(u), bits(v)) if u.is_floating_point() else torch.equal(u, v) for u, v in zip(whole, again))
    for b in range(B):
        one = [None if g is None else g.view(-1, B, *g.shape[1:])[:, b].contiguous() for g in groups]      # view-major: slot * B + b
        part = run_merge(cuda, one, rows, 1, C, H, W)
        for u, v in zip(whole, part):
            assert torch.equal(bits(u[b:b + 1]), bits(v)) if u.is_floating_point() else torch.equal(u[b:b + 1], v), b


# ---- 5. the model at other class counts --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", [(3, 1, 8, 2), (3, 3, 8, 2), (3, 5, 8, 2)])
def test_predict_tta_at_other_class_counts(cuda, cfg):
    shape = (1, 3, 33, 47)
    m = unet(cuda, cfg=cfg)
    x = images(shape, cuda, seed=cfg[1])
    probs, labels, conf = mgunet.predict_tta(m, x, "d4")
    check_outputs(probs, labels, conf, shape, cfg[1])
    d = float((probs.double() - reference_tta(m, x, "d4")).abs().max())
    print(f"[tta d4 {cfg} {shape}] max|probs - torch composition| = {d:.2e}")
    assert d <= 1e-5


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------

def test_c_abi_refusals_leave_the_context_usable(cuda):
    """Each bad call raises ValueError (MGU_ERR_INVALID) with a message before anything is launched; the same context then runs a
    good call of each entry point, whose result is checked."""
    B, Cc, H, W = 2, 3, 12, 20
    rows, groups = TO.make("random", Cc, "d4", H, W, B)
    l0, l1 = groups[0].to(cuda), groups[1].to(cuda)
    probs = torch.full((B, H, W, Cc), float("nan"), device=cuda)
    labels = torch.full((B, H, W), -1, device=cuda, dtype=torch.int64)
    conf = torch.full((B, H, W), float("nan"), device=cuda)
    x = images((B, Cc, H, W), cuda)
    st = (CT.c_int64 * 4)(*x.stride())
    vout = torch.full((8 * B, Cc, H, W), float("nan"), device=cuda)

    def table(rws):
        return (CT.c_int32 * (4 * len(rws)))(*[v for row in rws for v in row])

    def merge(rws=rows, K=None, Cn=Cc, g0=l0, g1=l1, tbl=0, p=probs, lab=labels, cf=conf):
        _lib.call("mgu_tta_merge", cuda, g0, g1, B, Cn, H, W, len(rws) if K is None else K, table(rws) if tbl == 0 else tbl, p, lab, cf)

    def views(codes=((0, 0), (1, 2)), G=None, strides=st, img=x, out=vout):
        flat = (CT.c_int32 * (2 * len(codes)))(*[v for fr in codes for v in fr])
        _lib.call("mgu_tta_views", cuda, img, B, Cc, H, W, strides, len(codes) if G is None else G, flat, out)

    def with_row(k, row):
        return rows[:k] + [row] + rows[k + 1:]

    assert rows[1] == (1, 0, 0, 1) and rows[2] == (0, 1, 0, 2)
    bad = [
        lambda: merge(Cn=0), lambda: merge(Cn=17),
        lambda: merge(K=0), lambda: merge(K=3), lambda: merge(K=5), lambda: merge(rws=rows + rows, K=16),
        lambda: merge(rws=with_row(1, (0, 1, 0, 1))), lambda: merge(rws=with_row(2, (1, 1, 0, 2))),      # group != turns & 1 at H != W
        lambda: merge(g1=None),                                                                           # group-1 views, no logits
        lambda: merge(rws=with_row(0, (0, 0, 4, 0))), lambda: merge(rws=with_row(0, (0, 0, 0, 4))),
        lambda: merge(rws=with_row(0, (0, 0, -1, 0))), lambda: merge(rws=with_row(1, (1, 0, 0, 5))),
        lambda: merge(rws=with_row(2, (0, 8, 0, 2))), lambda: merge(rws=with_row(2, (0, -1, 0, 2))), lambda: merge(rws=with_row(2, (2, 0, 0, 2))),
        lambda: merge(tbl=None), lambda: merge(p=None), lambda: merge(lab=None), lambda: merge(cf=None), lambda: merge(g0=None),
        lambda: views(G=0), lambda: views(codes=[(0, 0)] * 9),
        lambda: views(codes=((0, 0), (0, 1))), lambda: views(codes=((3, 3), (0, 2))),                     # mixed shapes at H != W
        lambda: views(codes=((4, 0),)), lambda: views(codes=((0, 4),)),
        lambda: views(strides=None), lambda: views(img=None), lambda: views(out=None),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
        assert _lib.lib().mgu_last_error(_lib.context(cuda).handle), i
    torch.cuda.synchronize()
    assert torch.isnan(probs).all() and int(labels.max()) == -1 and torch.isnan(conf).all() and torch.isnan(vout).all()   # nothing ran
    merge()
    views()
    torch.cuda.synchronize()
    ref = TO.merge64(groups, rows, B, Cc, H, W)
    assert float((probs.cpu().double() - ref).abs().max()) <= TO.bound(Cc, 8)
    assert torch.equal(labels.cpu(), probs.cpu().argmax(-1)) and torch.equal(conf.cpu(), probs.cpu().amax(-1))
    xc = x.cpu()
    assert torch.equal(vout[:2 * B].cpu(), torch.cat([TO.view(xc, 0, 0), TO.view(xc, 1, 2)])) and torch.isnan(vout[2 * B:]).all()
