"""Object shape analysis on the MI355X (csrc/shapes.hip, mgunet.object_shapes, EllipticalShapeLoss(objects=...)).  Expected values
come from the float64 numpy oracle in shapes_oracle.py (from pixel coordinates, not from moments) and from the fixture the
reference's own EllipticalShapeLoss wrote (tools/make_shape_golden.py).

Tolerances.  Against the oracle: 1 fp32 ulp, |got - want| <= ulp32(max(|want|, scale)) with want the oracle's value rounded to fp32.
The device computes in fp64 from exact integers, which can only flip the final fp32 rounding -- under a condition: the closed form
of the term loses digits as ((l1 + eps) / (l2 + eps))^2 times the fp64 epsilon, so the device keeps it up to a ratio of 256 (error
below 1e-11 relative, plus a few fp64 ulp of sqrt / atan2 library difference) and evaluates thinner objects pixel by pixel from
exact integers with a uint64 fixed-point sum (rounding below 2^-26 per pixel); the smaller eigenvalue is det / l1 with an exact
integer determinant, 0 exactly for collinear pixels.  The oracle evaluates such objects in exact rational arithmetic.  The fixture's
"thin" map (diagonal, anti-diagonal and sloped one-pixel lines, a two-pixel band) holds the device to that; the reference has no
usable value there.  scale is max(c_xx, c_yy) for the covariance entries and pi/2 for the angle -- a c_xy
or an angle that is exactly 0 for a symmetric shape would otherwise be compared against fp64 noise -- and 0 elsewhere.  The angle is
compared where the oracle's l1 / l2 >= 1.1; elsewhere the axis direction is ill-conditioned.  Against the reference: 2 x ref_dev
relative, ref_dev being the reference's own fp32 deviation from float64 as the generator measured it; the factor 2 covers the sum
of its deviation and ours."""
import numpy as np
import pytest
import torch

import mgunet
import objects_oracle as OO
import shapes_oracle as SO
from mgunet import objects as mobj

pytestmark = pytest.mark.gpu

FIELDS = ("centroid", "cov", "axes", "angle", "fill", "term")


def singles(g):
    return [(name, np.unpackbits(g[f"single_{k}_bits"]).reshape(256, 256).astype(np.int64), float(g[f"single_{k}_ref"]))
            for k, name in enumerate(g["single_names"].tolist())]


def scenes(g):
    return [(k, np.unpackbits(g[f"scene_{k}_bits"]).reshape(512, 512).astype(np.int64), g[f"scene_{k}_terms"], float(g[f"scene_{k}_loss"]))
            for k in range(4)]


def edges(g):
    return [(name, g[f"edge_{k}_map"].astype(np.int64), g[f"edge_{k}_terms"], float(g[f"edge_{k}_loss"]), float(g[f"edge_{k}_loss_c1"]))
            for k, name in enumerate(g["edge_names"].tolist())]


def thin_maps(g):
    return [(name, g[f"thin_{k}_map"].astype(np.int64)) for k, name in enumerate(g["thin_names"].tolist())]


def host(sh):
    return {f: getattr(sh, f).cpu().numpy() for f in FIELDS + ("status",)}


def close_ulp(got, want, scale=0.0):
    w32 = float(np.float32(want))
    return abs(float(got) - w32) <= SO.ulp32(max(abs(w32), scale))


def check_object(h, i, want, tag):
    """Row i of the device arrays against one oracle object; returns (analysed, angle compared)."""
    assert h["status"][i] == want["status"], (tag, h["status"][i], want["status"])
    for j in range(2):
        assert close_ulp(h["centroid"][i, j], want["centroid"][j]), (tag, "centroid", h["centroid"][i], want["centroid"])
    if want["status"] != 0:                                        # checked by its status: the other fields are defined as 0
        assert not any(np.any(h[f][i]) for f in FIELDS[1:]), tag
        return False, False
    cscale = max(want["cov"][0], want["cov"][2])
    for j in range(3):
        assert close_ulp(h["cov"][i, j], want["cov"][j], cscale), (tag, "cov", h["cov"][i], want["cov"])
    for j in range(2):
        assert close_ulp(h["axes"][i, j], want["axes"][j]), (tag, "axes", h["axes"][i], want["axes"])
    assert close_ulp(h["fill"][i], want["fill"]), (tag, "fill", h["fill"][i], want["fill"])
    assert close_ulp(h["term"][i], want["term"]), (tag, "term", h["term"][i], want["term"])
    l1, l2 = want["lam"]
    if l2 > 0 and l1 / l2 < 1.1:
        return True, False
    assert close_ulp(h["angle"][i], want["angle"], np.pi / 2), (tag, "angle", h["angle"][i], want["angle"])
    return True, True


def check_table(table, sh, maps, tag):
    """Every object of every image against the oracle on the oracle's own labelling; returns per image (analysed, angles compared)."""
    h = host(sh)
    off = table.offsets.cpu().numpy()
    assert len(h["status"]) == off[-1]
    out = []
    for b, m in enumerate(maps):
        lab = OO.label(m, 2)
        assert np.array_equal(table.labels[b].cpu().numpy(), lab), (tag, b)
        want = SO.shapes_of_labels(lab)
        assert off[b + 1] - off[b] == len(want)
        res = [check_object(h, off[b] + k, w, (tag, b, k)) for k, w in enumerate(want)]
        out.append((sum(r[0] for r in res), sum(r[1] for r in res)))
    return out


def run(cuda, m):
    t = mgunet.connected_components(torch.from_numpy(np.asarray(m, np.int64)).to(cuda))
    return t, mgunet.object_shapes(t)


def table_of_mask(cuda, m):
    """A hand-built one-object table: every set pixel of m belongs to object 1, connected or not."""
    ys, xs = np.nonzero(m)
    dev = lambda a, dt: torch.tensor(a, dtype=dt, device=cuda)  # noqa: E731
    return mgunet.ObjectTable(dev(m[None], torch.int32), dev([1], torch.int64), dev([0, 1], torch.int64), dev([1], torch.int64),
                              dev([len(ys)], torch.int64), dev([[xs.min(), ys.min(), xs.max() + 1, ys.max() + 1]], torch.int32),
                              dev([[xs.sum(), ys.sum()]], torch.int64))


def synthetic_batch(g):
    """8 x 3 x 512 x 512 fp32 logits whose arg-max maps are the four scenes and their transposes with the right half in class 2."""
    rng = np.random.default_rng(21)
    maps = []
    for _, m, _, _ in scenes(g):
        maps.append(m)
        t = m.T.copy()
        t[:, 256:] *= 2
        maps.append(t)
    cls = np.stack(maps)
    logits = rng.normal(0.0, 0.5, (8, 3, 512, 512)).astype(np.float32)
    logits += 6.0 * (np.arange(3)[None, :, None, None] == cls[:, None]).astype(np.float32)
    assert np.array_equal(logits.argmax(1), cls)
    return logits, cls


# 1 ---- against the float64 oracle -----------------------------------------------------------------------------------------------------
def test_fixture_images_against_oracle(cuda, golden):
    g = golden["shapes"]
    angles = {}
    for name, m, _ in singles(g):
        t, sh = run(cuda, m)
        (_, n_ang), = check_table(t, sh, [m], name)
        angles[name] = n_ang
    assert angles["ellipse"] >= 1 and angles["tilted_ellipse"] >= 1 and angles["line"] >= 1
    for k, m, terms, _ in scenes(g):
        t, sh = run(cuda, m)
        (n_ok, n_ang), = check_table(t, sh, [m], f"scene {k}")
        assert n_ok == len(terms) >= 25 and 2 * n_ang >= n_ok, (k, n_ok, n_ang)
    for name, m, terms, _, _ in edges(g):
        t, sh = run(cuda, m)
        (n_ok, _), = check_table(t, sh, [m], name)
        assert n_ok == len(terms)
    for name, m in thin_maps(g):
        t, sh = run(cuda, m)
        (n_ok, n_ang), = check_table(t, sh, [m], name)
        assert n_ok == n_ang == 9
        print(f"thin {name}: terms {[round(v, 6) for v in sh.term.tolist()]} loss {float(sh.loss()):.7f}")
    # the noise mask as ONE object (not connected): a hand-built table
    m = dict((n, x) for n, x, _ in singles(g))["noise"]
    ys, xs = np.nonzero(m)
    sh = mgunet.object_shapes(table_of_mask(cuda, m))
    assert check_object(host(sh), 0, SO.shape(ys, xs), "noise as one object")[0]


def test_logits_batch_against_oracle(cuda, golden):
    logits, cls = synthetic_batch(golden["shapes"])
    t = mgunet.connected_components(torch.from_numpy(logits).to(cuda))
    assert np.array_equal(t.class_id.cpu().numpy() > 0, np.ones(t.class_id.numel(), bool))
    res = check_table(t, mgunet.object_shapes(t), list(cls), "logits batch")
    for n_ok, n_ang in res:
        assert n_ok >= 25 and 2 * n_ang >= n_ok


def test_status_is_exact(cuda, golden):
    for _, m, _, _ in scenes(golden["shapes"])[:2]:
        t, sh = run(cuda, m)
        assert torch.equal(sh.status == 1, t.area < 10) and torch.equal(sh.valid, t.area >= 10)
        assert torch.equal(mgunet.object_shapes(t, min_pixels=40).status == 1, t.area < 40)


# 2 ---- against the reference ----------------------------------------------------------------------------------------------------------
def test_terms_and_losses_against_reference(cuda, golden):
    g = golden["shapes"]
    tol = 2.0 * float(g["ref_dev"])
    rel = lambda got, want: abs(float(got) - float(want)) / abs(float(want))  # noqa: E731
    for name, m, ref in singles(g):
        sh = mgunet.object_shapes(table_of_mask(cuda, m))       # one object per mask, as the reference was called
        d = rel(sh.term[0], ref)
        print(f"single {name}: term {float(sh.term[0]):.7f} reference {ref:.7f} rel {d:.2e}")
        assert int(sh.status[0]) == 0 and d <= tol, (name, d)
        assert rel(sh.loss(), ref) <= tol
    for tag, m, terms, total in [(f"scene {k}", m, t, lo) for k, m, t, lo in scenes(g)] + [(n, m, t, lo) for n, m, t, lo, _ in edges(g)]:
        t, sh = run(cuda, m)
        got = sh.term[sh.valid].cpu().numpy()
        assert len(got) == len(terms), tag
        if tag.startswith("scene"):
            assert len(got) >= 25
        d = np.abs(got.astype(np.float64) - terms) / np.abs(terms)
        dl = rel(sh.loss(), total)
        print(f"{tag}: {len(got)} analysed objects, worst term rel {d.max():.2e}, loss {float(sh.loss()):.7f} reference {total:.7f} rel {dl:.2e}")
        assert d.max() <= tol and dl <= tol, (tag, d.max(), dl)


# 3 ---- EllipticalShapeLoss ------------------------------------------------------------------------------------------------------------
def test_loss_module_objects_keyword(cuda, golden):
    g = golden["shapes"]
    tol = 2.0 * float(g["ref_dev"])
    t, sh = run(cuda, scenes(g)[0][1])
    via_module = mgunet.EllipticalShapeLoss()(None, objects=t)
    assert via_module.dim() == 0 and via_module.dtype == torch.float32
    assert torch.equal(via_module.view(1).view(torch.int32), sh.loss().view(1).view(torch.int32))
    name, m, _, _, ref_c1 = edges(g)[3]
    assert name == "three_class"
    probs = torch.softmax(4.0 * torch.nn.functional.one_hot(torch.from_numpy(m), 3).permute(2, 0, 1)[None].float(), 1).to(cuda)
    got = mgunet.EllipticalShapeLoss()(probs, objects=True)
    print(f"objects=True on the three-class map: {float(got):.7f}, reference over its class-1 objects {ref_c1:.7f}")
    assert abs(float(got) - ref_c1) / abs(ref_c1) <= tol
    t3, sh3 = run(cuda, m)
    assert float(sh3.loss(keep_class=1)) == float(got) != float(sh3.loss())
    assert float(mgunet.EllipticalShapeLoss()(torch.zeros(1, 1, 8, 8, device=cuda), objects=True)) == 0.0      # no foreground class
    assert float(mgunet.EllipticalShapeLoss()(torch.ones(1, 2, 8, 8, device=cuda), objects=True)) == 0.0       # no objects
    with pytest.raises(ValueError):
        mgunet.EllipticalShapeLoss()(None, object_masks_list=[[]], objects=t)


# 4 ---- cross-check with the dense route -----------------------------------------------------------------------------------------------
def test_dense_masks_route_agrees(cuda, golden):
    g = golden["shapes"]
    t, sh = run(cuda, scenes(g)[1][1])
    dense = float(mgunet.EllipticalShapeLoss()(None, t.masks()))
    got = float(sh.loss())
    print(f"dense masks route {dense:.7f}, object route {got:.7f}")
    assert abs(dense - got) / abs(dense) <= 2.0 * float(g["ref_dev"])


def test_thin_objects_beside_ordinary_ones(cuda, golden):
    """A scene with the thin lines pasted into its empty corner regions' place: one ill-conditioned object must not disturb the
    others or the loss; batch rows equal single-image rows bitwise, and the dense per-pixel route agrees on the loss."""
    g = golden["shapes"]
    thin = thin_maps(g)[0][1]
    m = np.zeros((2, 512, 512), np.int64)
    m[0] = scenes(g)[0][1]
    m[1, 32:480, 32:480] = thin
    t = mgunet.connected_components(torch.from_numpy(m).to(cuda))
    sh = mgunet.object_shapes(t)
    check_table(t, sh, list(m), "scene + thin batch")
    want = [s for b in range(2) for s in SO.shapes_of_labels(OO.label(m[b], 2))]
    # the device averages terms already rounded to fp32 (1/2 ulp each) and rounds once more: 2 ulp of the largest term covers it
    tol = 2.0 * SO.ulp32(max(s["term"] for s in want))
    assert abs(float(sh.loss()) - SO.loss(want)) <= tol, (float(sh.loss()), SO.loss(want))
    off = t.offsets.cpu().tolist()
    one = mgunet.object_shapes(mgunet.connected_components(torch.from_numpy(m[1]).to(cuda)))
    assert all(torch.equal(x[off[1]:off[2]], y) for x, y in zip(bits(sh), bits(one)))
    assert all(torch.equal(x, y) for x, y in zip(bits(sh), bits(mgunet.object_shapes(t))))
    dense = float(mgunet.EllipticalShapeLoss()(None, mgunet.connected_components(torch.from_numpy(m[1]).to(cuda)).masks()))
    print(f"thin lines: object route {float(one.loss()):.7f}, dense masks route {dense:.7f}")
    assert abs(dense - float(one.loss())) / abs(dense) <= 2.0 * float(g["ref_dev"])


# 5 ---- determinism --------------------------------------------------------------------------------------------------------------------
def bits(sh):
    return [getattr(sh, f).contiguous().view(torch.int32) for f in FIELDS] + [sh.status]


def test_repeatable_and_batch_equals_single_images(cuda, golden):
    logits, cls = synthetic_batch(golden["shapes"])
    t = mgunet.connected_components(torch.from_numpy(cls).to(cuda))
    a, b = mgunet.object_shapes(t), mgunet.object_shapes(t)
    assert all(torch.equal(x, y) for x, y in zip(bits(a), bits(b)))
    assert torch.equal(a.loss().view(1).view(torch.int32), b.loss().view(1).view(torch.int32))
    off = t.offsets.cpu().tolist()
    for i in range(len(cls)):
        one = mgunet.object_shapes(mgunet.connected_components(torch.from_numpy(cls[i]).to(cuda)))
        assert all(torch.equal(x[off[i]:off[i + 1]], y) for x, y in zip(bits(a), bits(one))), i


# 6 ---- worst-case capacity buffers, no synchronisation --------------------------------------------------------------------------------
def test_worst_case_capacity_buffers(cuda, golden):
    g = golden["shapes"]
    maps = np.stack([m[100:228, 60:188] for _, m, _, _ in scenes(g)[:2]])
    src = torch.from_numpy(maps).to(cuda)
    exact = mgunet.object_shapes(mgunet.connected_components(src))
    B, H, W = maps.shape
    cap = B * H * W                                                                  # every pixel its own object
    mk = lambda shape, dt: torch.full(shape, -1, device=cuda, dtype=dt)  # noqa: E731
    labels, counts, offsets = mk((B, H, W), torch.int32), mk((B,), torch.int64), mk((B + 1,), torch.int64)
    cls, area, bbox, sums = mk((cap,), torch.int64), mk((cap,), torch.int64), mk((cap, 4), torch.int32), mk((cap, 2), torch.int64)
    mobj._label(src, 0, B, H, W, 0, 2, 0, 0, 0, labels, counts, offsets)
    mobj._stats(labels, src, 0, B, H, W, 0, offsets, cap, cls, bbox, area, sums)
    mk7 = lambda shape, dt: torch.full(shape, 7, device=cuda, dtype=dt)  # noqa: E731
    bufs = (mk7((cap, 2), torch.float32), mk7((cap, 3), torch.float32), mk7((cap, 2), torch.float32), mk7((cap,), torch.float32),
            mk7((cap,), torch.float32), mk7((cap,), torch.float32), mk7((cap,), torch.uint8))
    moments = mk((cap, 12), torch.int64)
    out = mobj._shapes(labels, B, H, W, offsets, cap, area, bbox, sums, 1e-6, 10, out=bufs, moments=moments)
    assert all(o.data_ptr() == b.data_ptr() for o, b in zip(out, bufs))              # the caller's buffers, nothing allocated per call
    N = exact.status.numel()
    assert int(offsets[B]) == N > 0
    worst = mgunet.ObjectShapes(*[o[:N] for o in out], offsets, cls[:N])
    assert all(torch.equal(x, y) for x, y in zip(bits(worst), bits(exact)))
    assert torch.equal(worst.loss().view(1).view(torch.int32), exact.loss().view(1).view(torch.int32))
    assert all(bool((o[N:] == 7).all()) for o in out)                                # rows past the object count are left alone
    loss = torch.empty((), device=cuda)
    mgunet._lib.call("mgu_elliptical_shape_loss_objects", cuda, B, offsets, cap, out[5], out[6], None, 0, loss)
    assert torch.equal(loss.view(1).view(torch.int32), exact.loss().view(1).view(torch.int32))


# 7 ---- to_dicts -----------------------------------------------------------------------------------------------------------------------
def test_to_dicts_with_shapes(cuda, golden):
    name, m, _, _, _ = edges(golden["shapes"])[3]
    t, sh = run(cuda, m)
    plain = t.to_dicts()
    off, bbox, cls = t.offsets.cpu().tolist(), t.bbox.cpu().tolist(), t.class_id.cpu().tolist()
    assert plain == [[{"bbox": bbox[i], "class_id": cls[i]} for i in range(off[b], off[b + 1])] for b in range(len(off) - 1)]
    assert all(list(d) == ["bbox", "class_id"] for img in plain for d in img)
    rich = t.to_dicts(shapes=sh)
    st = sh.status.cpu().tolist()
    assert 0 in st and 1 in st
    for i, (d, p) in enumerate(zip(rich[0], plain[0])):
        assert list(d) == ["bbox", "class_id", "ellipse", "shape_term"] and d["bbox"] == p["bbox"] and d["class_id"] == p["class_id"]
        if st[i]:
            assert d["ellipse"] is None and d["shape_term"] is None
        else:
            assert list(d["ellipse"]) == ["center", "axes", "angle", "fill"]
            assert d["ellipse"]["center"] == sh.centroid[i].cpu().tolist() and d["ellipse"]["axes"] == sh.axes[i].cpu().tolist()
            assert d["ellipse"]["angle"] == float(sh.angle[i]) and d["ellipse"]["fill"] == float(sh.fill[i])
            assert d["shape_term"] == float(sh.term[i])
    scores = torch.linspace(0.1, 0.9, len(st))
    both = t.to_dicts(scores=scores, shapes=sh)
    assert all(list(d) == ["bbox", "class_id", "confidence", "ellipse", "shape_term"] for d in both[0])
    assert t.to_dicts(scores=scores) == [[dict(p, confidence=c) for p, c in zip(plain[0], scores.tolist())]]


# 8 ---- the exactness bound ------------------------------------------------------------------------------------------------------------
def test_exactness_bound(cuda):
    """A 2048 x 2048 all-foreground image is one object past area * (max(w, h) - 1)^4 < 2^64: the build marks it status 2 (it does not
    accumulate wider), so its wrapped sums are never used.  A 1024 x 1024 one, the largest inside the bound, matches the oracle."""
    t = mgunet.connected_components(torch.ones((1, 2048, 2048), dtype=torch.int64, device=cuda))
    sh = mgunet.object_shapes(t)
    assert t.counts.tolist() == [1] and sh.status.tolist() == [2] and sh.valid.tolist() == [False]
    assert sh.centroid.tolist() == [[1023.5, 1023.5]]
    assert not any(bool(getattr(sh, f).any()) for f in FIELDS[1:])
    assert float(sh.loss()) == 0.0 and t.to_dicts(shapes=sh)[0][0]["ellipse"] is None
    m = np.ones((1024, 1024), np.int64)
    t, sh = run(cuda, m)
    ys, xs = np.nonzero(m)
    assert check_object(host(sh), 0, SO.shape(ys, xs), "1024 x 1024 object") == (True, False)
