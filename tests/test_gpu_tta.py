"""Test-time augmentation and object confidence on the MI355X (csrc/tta.hip, csrc/objects.hip mgu_object_scores, mgunet.tta).
predict_tta is checked against float64 torch compositions of separate forwards of each torch.flip / torch.rot90 view, for equivariance,
and in bf16; object_scores against a numpy restatement of its fixed-point sum and against the float64 mean."""
import numpy as np
import pytest
import torch

import mgunet
import mgunet_oracle as O
from mgunet import objects as mobj
from mgunet import tta

pytestmark = pytest.mark.gpu

CFG = (3, 2, 8, 2)


def unet(dev, dtype=torch.float32, cfg=CFG, seed=3):
    m = mgunet.UNet(*cfg, compute_dtype=dtype)
    m.load_state_dict(O.make_unet_params(*cfg, seed=seed))
    return m.to(dev).eval()


def images(shape, dev, seed=7):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def fW(x):
    return torch.flip(x, (3,))


def fH(x):
    return torch.flip(x, (2,))


def rot(x, r):
    return torch.rot90(x, r, (2, 3))


# (view, inverse) pairs in the documented averaging order
REF_VIEWS = {
    "hflip": [(lambda x: x, lambda p: p), (fW, fW)],
    "flips": [(lambda x: x, lambda p: p), (fW, fW), (fH, fH), (lambda x: fH(fW(x)), lambda p: fW(fH(p)))],
    "d4": [(lambda x, r=r: rot(x, r), lambda p, r=r: rot(p, -r)) for r in range(4)]
    + [(lambda x, r=r: rot(fW(x), r), lambda p, r=r: fW(rot(p, -r))) for r in range(4)],
}


def reference_tta(model, x, name):
    """float64 mean of the views' softmaxes, one existing-path forward per view (batch B, not K * B)."""
    acc = 0
    with torch.no_grad():
        for view, inv in REF_VIEWS[name]:
            lg = model(view(x).contiguous())[0]
            acc = acc + inv(torch.softmax(lg.double(), 1))
    return acc / len(REF_VIEWS[name])


def check_outputs(probs, labels, conf, shape, C):
    B, _, H, W = shape
    assert probs.shape == (B, C, H, W) and probs.dtype == torch.float32
    assert probs.permute(0, 2, 3, 1).is_contiguous()   # NCHW view of NHWC storage, like UNet.forward's logits
    assert labels.shape == (B, H, W) and labels.dtype == torch.int64
    assert conf.shape == (B, H, W) and conf.dtype == torch.float32
    assert torch.equal(labels, probs.argmax(1))
    assert torch.equal(conf, probs.amax(1))


@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (1, 3, 97, 131)])
def test_none_is_the_plain_softmax(cuda, shape):
    m = unet(cuda)
    x = images(shape, cuda)
    probs, labels, conf = mgunet.predict_tta(m, x, "none")
    check_outputs(probs, labels, conf, shape, CFG[1])
    with torch.no_grad():
        ref = torch.softmax(m(x)[0].double(), 1)
    d = float((probs.double() - ref).abs().max())
    print(f"[tta none {shape}] max|probs - softmax64| = {d:.2e}")
    assert d <= 2e-6


@pytest.mark.parametrize("name", ["hflip", "flips", "d4"])
@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (2, 3, 96, 160), (1, 3, 97, 131)])
def test_views_match_torch_composition(cuda, name, shape):
    m = unet(cuda)
    x = images(shape, cuda, seed=sum(shape))
    probs, labels, conf = mgunet.predict_tta(m, x, name)
    check_outputs(probs, labels, conf, shape, CFG[1])
    ref = reference_tta(m, x, name)
    d = float((probs.double() - ref).abs().max())
    print(f"[tta {name} {shape}] max|probs - torch composition| = {d:.2e}")
    assert d <= 1e-5


def test_strided_input(cuda):
    """A channels-last, sliced batch gives the same result as its contiguous copy."""
    m = unet(cuda)
    big = images((2, 3, 80, 96), cuda).contiguous(memory_format=torch.channels_last)
    x = big[:, :, 5:69, 7:87]
    assert not x.is_contiguous()
    for name in ("none", "d4"):
        a, b = mgunet.predict_tta(m, x, name), mgunet.predict_tta(m, x.contiguous(), name)
        assert all(torch.equal(u, v) for u, v in zip(a, b)), name


def margin_mask(probs):
    top2 = probs.topk(2, dim=1).values
    return (top2[:, 0] - top2[:, 1]) > 1e-5


def test_d4_rotation_equivariance(cuda):
    m = unet(cuda)
    x = images((2, 3, 64, 64), cuda, seed=11)
    pa, la, _ = mgunet.predict_tta(m, rot(x, 1).contiguous(), "d4")
    pb, lb, _ = mgunet.predict_tta(m, x, "d4")
    pb, lb = rot(pb, 1), torch.rot90(lb, 1, (1, 2))
    d = float((pa - pb).abs().max())
    print(f"[tta d4 equivariance] max diff {d:.2e}")
    assert d <= 1e-6
    keep = margin_mask(pb)
    assert torch.equal(la[keep], lb[keep])


def test_flips_flip_equivariance(cuda):
    m = unet(cuda)
    x = images((2, 3, 64, 64), cuda, seed=12)
    pa, la, _ = mgunet.predict_tta(m, fW(x).contiguous(), "flips")
    pb, lb, _ = mgunet.predict_tta(m, x, "flips")
    pb, lb = fW(pb), torch.flip(lb, (2,))
    d = float((pa - pb).abs().max())
    print(f"[tta flips equivariance] max diff {d:.2e}")
    assert d <= 1e-6
    keep = margin_mask(pb)
    assert torch.equal(la[keep], lb[keep])


@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (1, 3, 64, 96)])
def test_bf16_model(cuda, shape):
    """bf16 storage against the fp32 TTA, with test_gpu_bf16's logit bounds (max 2.5e-2, mean 3e-3 of max|logit|) carried through
    the softmax (|d p| <= max_c |d logit_c| / 2, and the mean over views keeps the bound), and >= 99 % label agreement."""
    x = images(shape, cuda, seed=5)
    m32, m16 = unet(cuda), unet(cuda, torch.bfloat16)
    p32, l32, _ = mgunet.predict_tta(m32, x, "d4")
    p16, l16, c16 = mgunet.predict_tta(m16, x, "d4")
    check_outputs(p16, l16, c16, shape, CFG[1])
    with torch.no_grad():
        scale = float(m32(x)[0].abs().max())
    d = (p16 - p32).abs()
    agree = float((l16 == l32).double().mean())
    print(f"[tta bf16 {shape}] max {float(d.max()):.3e} mean {float(d.mean()):.3e} (max|logit| {scale:.2f}), labels agree {agree*100:.2f} %")
    assert float(d.max()) <= 0.5 * 2.5e-2 * scale and float(d.mean()) <= 3e-3 * scale
    assert agree >= 0.99


def test_refusals(cuda):
    m = unet(cuda)
    x = images((1, 3, 32, 32), cuda)
    with pytest.raises(RuntimeError, match="eval"):
        mgunet.predict_tta(m.train(), x, "d4")
    m.eval()
    with pytest.raises(RuntimeError, match="HIP device"):
        mgunet.predict_tta(m, x.cpu(), "d4")
    with pytest.raises(ValueError):
        mgunet.predict_tta(m, x, "rot90")
    with pytest.raises(TypeError):
        mgunet.predict_tta(m, x.double(), "d4")


def scores_numpy(table, probs):
    """object_scores restated: sum of round_half_even(p * 2^32) per object in uint64, (sum * 2^-32) / area in float64, to float32.
    p is clamped to [0, 1] first, and a NaN counts as 0 (the kernel's fminf(fmaxf(p, 0), 1) returns the non-NaN operand)."""
    lab = table.labels.cpu().numpy().reshape(-1).astype(np.int64)
    B, C, H, W = probs.shape
    p = probs.permute(0, 2, 3, 1).cpu().numpy().reshape(-1, C)
    off, cls, area = table.offsets.cpu().numpy(), table.class_id.cpu().numpy(), table.area.cpu().numpy()
    b = np.arange(lab.size) // (H * W)
    fg = lab > 0
    obj = off[b[fg]] + lab[fg] - 1
    pv = p[fg, cls[obj]]
    pv = np.where(np.isnan(pv), np.float32(0), pv)
    q = np.rint(np.clip(pv, 0, 1).astype(np.float64) * 2.0 ** 32).astype(np.uint64)
    acc = np.zeros(cls.size, np.uint64)
    np.add.at(acc, obj, q)
    return ((acc.astype(np.float64) * 2.0 ** -32) / area.astype(np.float64)).astype(np.float32), obj, p[fg, cls[obj]]


@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (1, 3, 97, 131), (8, 3, 128, 128)])
def test_object_scores(cuda, shape):
    m = unet(cuda)
    probs, _, _ = mgunet.predict_tta(m, images(shape, cuda, seed=3), "d4")
    table = mgunet.connected_components(probs)
    N = table.class_id.numel()
    assert N > 1
    s1, s2 = mgunet.object_scores(table, probs), mgunet.object_scores(table, probs)
    assert s1.shape == (N,) and s1.dtype == torch.float32
    assert torch.equal(s1, s2)
    ref, obj, pv = scores_numpy(table, probs)
    got = s1.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    mean64 = np.zeros(N)
    np.add.at(mean64, obj, pv.astype(np.float64))
    mean64 /= table.area.cpu().numpy()
    err = np.abs(got.astype(np.float64) - mean64)
    print(f"[object scores {shape}] {N} objects, max rel err vs float64 mean {float((err / mean64).max()):.2e}")
    assert np.all(err <= 2.0 ** -24 * mean64 + 2.0 ** -32)
    dicts = table.to_dicts(scores=s1)
    flat = [d["confidence"] for img in dicts for d in img]
    assert flat == got.tolist()


def test_object_scores_clamp_and_nan(cuda):
    """Probabilities outside [0, 1] are clamped, NaN counts as 0, and an object of 90 000 pixels at exactly 1.0 scores exactly 1.0
    (90 000 * 2^32 fits the uint64 sum and the fp64 finish).  The table comes from a synthetic 3-class map."""
    H, W = 320, 400
    cmap = torch.zeros((1, H, W), dtype=torch.int64)
    cmap[0, 5:305, 10:310] = 1        # 300 x 300: all ones
    cmap[0, 0:40, 330:380] = 2        # below 0 and in range
    cmap[0, 60:100, 330:380] = 1      # above 1 and in range
    cmap[0, 120:160, 330:380] = 2     # NaN and in range
    cmap[0, 180:200, 330:380] = 1     # NaN only
    cmap[0, 220:240, 330:380] = 2     # above 1 only
    cmap[0, 260:280, 330:380] = 1     # below 0 only
    table = mgunet.connected_components(cmap.to(cuda))
    at = {y0: i for i, (_, y0, _, _) in enumerate(table.bbox.tolist())}       # object index by the first row of its box
    big, lo, hi, nan, nan_only, above, below = (at[y] for y in (5, 0, 60, 120, 180, 220, 260))
    assert table.area[big] == 90000 and table.class_id.tolist() == [[2, 1, 1, 2, 1, 2, 1][at[y]] for y in (0, 5, 60, 120, 180, 220, 260)]
    g = torch.Generator().manual_seed(9)
    p = torch.rand((1, H, W, 3), generator=g)
    p[0, 5:305, 10:310, 1] = 1.0
    p[0, 0:20, 330:380, 2] = -torch.rand((20, 50), generator=g) * 1e3 - 1e-9
    p[0, 0, 330, 2] = float("-inf")
    p[0, 60:80, 330:380, 1] = 1.0 + torch.rand((20, 50), generator=g) * 1e3 + 1e-6
    p[0, 60, 330, 1] = float("inf")
    p[0, 120:140, 330:380, 2] = float("nan")
    p[0, 180:200, 330:380, 1] = float("nan")
    p[0, 220:240, 330:380, 2] = 1.5
    p[0, 260:280, 330:380, 1] = -0.5
    probs = p.to(cuda).permute(0, 3, 1, 2)
    s = mgunet.object_scores(table, probs)
    ref, obj, pv = scores_numpy(table, probs)
    got = s.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert got[big] == np.float32(1.0) and got[nan_only] == 0.0 and got[above] == np.float32(1.0) and got[below] == 0.0
    # half of each of these objects is clamped to 0 or 1 per pixel, the other half contributes its mean
    m_lo, m_hi, m_nan = (float(p[0, y:y + 20, 330:380, c].double().mean()) for y, c in ((20, 2), (80, 1), (140, 2)))
    assert abs(got[lo] - m_lo / 2) <= 1e-6 and abs(got[hi] - (1 + m_hi) / 2) <= 1e-6 and abs(got[nan] - m_nan / 2) <= 1e-6


def test_confidence_order_decides_matching(cuda):
    """Two overlapping GT boxes A = [0,0,100,100), B = [20,0,120,100).  P2 (the first object in raster order, box [0,0,70,100)) fits
    only A; P1 (box [10,0,110,100)) fits A and B equally, so A wins the tie.  In list order P2 takes A and P1 takes B: 2 matches.  P1's
    higher confidence puts it first: it takes A and P2 is left with nothing: 1 match."""
    H = W = 128
    p1 = torch.full((1, H, W), 0.2)
    p1[0, :, 0:2] = 0.6        # P2: columns 0-1 over the full height ...
    p1[0, 0, 0:70] = 0.6       # ... and row 0 up to x = 69
    p1[0, 50, 10:110] = 0.9    # P1: row 50 from x = 10 ...
    p1[0, :100, 109] = 0.9     # ... and column 109 over rows 0-99
    p1[0, 100:, 0:2] = 0.2
    probs = torch.stack([1 - p1, p1], -1).to(cuda).permute(0, 3, 1, 2)
    table = mgunet.connected_components(probs)
    assert table.counts.tolist() == [2]
    assert table.bbox.tolist() == [[0, 0, 70, 100], [10, 0, 110, 100]]
    scores = mgunet.object_scores(table, probs)
    assert scores.tolist() == [np.float32(0.6), np.float32(0.9)]
    gts = [[{"bbox": [0, 0, 100, 100], "class_id": 1}, {"bbox": [20, 0, 120, 100], "class_id": 1}]]
    plain, scored = table.to_dicts(), table.to_dicts(scores=scores)
    assert mobj._match_host(gts, plain, 0.5)[1] == 2
    assert mobj._match_host(gts, scored, 0.5)[1] == 1
    r_plain = mgunet.yield_estimation_metrics([2], [2], gts, plain)
    r_scored = mgunet.yield_estimation_metrics([2], [2], gts, scored)
    assert r_plain["object_matching_rate_perc"] == (2 / (2 + 1e-6)) * 100
    assert r_scored["object_matching_rate_perc"] == (1 / (2 + 1e-6)) * 100
