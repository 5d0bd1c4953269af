"""CPU tier of object shape analysis: the float64 oracle of the GPU tests (shapes_oracle.py) reproduces every per-object value the
reference's EllipticalShapeLoss wrote into the fixture (tools/make_shape_golden.py) within the fixture's own measured deviation, that
deviation stays under the ceiling the project grants the reference's fp32 accumulation, the oracle agrees with the repository's
restatement of the reference on the scenes, and the new C-ABI entries and Python names are declared, bound and exported (no GPU
needed)."""
import os
import re

import numpy as np
import torch

import mgunet
import mgunet_oracle as O
import objects_oracle as OO
import shapes_oracle as SO
from mgunet import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mgu_object_moments", "mgu_object_shapes", "mgu_elliptical_shape_loss_objects")
REF_DEV_CEILING = 2e-5      # what test_gpu_losses_pipeline.py grants the reference class for its fp32 accumulation


def singles(g):
    for k, name in enumerate(g["single_names"].tolist()):
        yield name, np.unpackbits(g[f"single_{k}_bits"]).reshape(256, 256).astype(bool), float(g[f"single_{k}_ref"])


def scenes(g):
    for k in range(4):
        yield k, np.unpackbits(g[f"scene_{k}_bits"]).reshape(512, 512).astype(np.int64), g[f"scene_{k}_terms"], float(g[f"scene_{k}_loss"])


def edges(g):
    for k, name in enumerate(g["edge_names"].tolist()):
        yield name, g[f"edge_{k}_map"].astype(np.int64), g[f"edge_{k}_terms"], float(g[f"edge_{k}_loss"]), float(g[f"edge_{k}_loss_c1"])


def rel(got, want):
    return abs(got - want) / abs(want)


def dev(ref, oracle):
    """Deviation of a stored reference value from the oracle's, as the generator measures ref_dev: relative to the oracle."""
    return abs(ref - oracle) / abs(oracle)


def test_ref_dev_is_under_the_ceiling(golden):
    assert 0.0 < float(golden["shapes"]["ref_dev"]) <= REF_DEV_CEILING


def test_oracle_reproduces_every_reference_term(golden):
    g = golden["shapes"]
    ref_dev = float(g["ref_dev"])
    worst = 0.0
    for name, m, ref in singles(g):
        ys, xs = np.nonzero(m)
        s = SO.shape(ys, xs)
        assert s["status"] == 0, name
        worst = max(worst, dev(ref, s["term"]))
    for _, m, terms, total in list(scenes(g)) + [(n, m, t, lo) for n, m, t, lo, _ in edges(g)]:
        shapes = [s for s in SO.shapes_of_labels(OO.label(m, 2)) if s["status"] == 0]
        assert len(shapes) == len(terms)
        worst = max([worst] + [dev(float(t), s["term"]) for s, t in zip(shapes, terms)])
        assert dev(total, SO.loss(shapes)) <= 2 * ref_dev       # the reference's own fp32 running sum on top of its terms
    print(f"largest deviation of the oracle from the stored reference terms: {worst:.3e} (ref_dev {ref_dev:.3e})")
    assert worst <= ref_dev                                     # measured with this oracle, by the same expression


def test_fixture_covers_the_cases(golden):
    g = golden["shapes"]
    assert g["single_names"].tolist() == ["ellipse", "tilted_ellipse", "square", "two_discs", "L", "line", "noise"]
    for k, m, terms, _ in scenes(g):
        lab = OO.label(m, 2)
        area = np.bincount(lab.reshape(-1))[1:]
        assert len(terms) == int((area >= 10).sum()) >= 25, k
        assert lab.max() >= 400 and area.max() <= 6000, k
        border = np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))
        assert (border > 0).sum() >= 4, k
    e = {name: m for name, m, *_ in edges(g)}
    assert sorted(np.bincount(OO.label(e["nine_and_ten"], 2).reshape(-1))[1:].tolist()) == [9, 10]
    assert e["row_run"].any(1).sum() == 1 and e["full_image"].all() and e["full_image"].shape == (64, 64)
    assert set(np.unique(e["three_class"]).tolist()) == {0, 1, 2}


def test_oracle_agrees_with_the_repository_oracle_on_the_scenes(golden):
    for k, m, _, _ in scenes(golden["shapes"]):
        lab = OO.label(m, 2)
        masks = [torch.from_numpy(lab == j) for j in range(1, lab.max() + 1)]
        want = float(O.elliptical_shape_loss(None, [masks], 1e-6))                  # fp32, the reference's own route
        assert rel(SO.loss(SO.shapes_of_labels(lab)), want) <= REF_DEV_CEILING, k


def test_oracle_statuses_and_the_exactness_bound():
    assert SO.shape(np.zeros(9), np.arange(9))["status"] == 1 and SO.shape(np.zeros(10), np.arange(10))["status"] == 0
    assert not SO.too_large(1024 * 1024, 1024, 1024) and SO.too_large(2048 * 2048, 2048, 2048)
    s = SO.shape(np.zeros(48), np.arange(48))                                        # a one-pixel-high run
    assert s["axes"][1] == 0.0 and s["fill"] == 0.0 and s["angle"] == 0.0 and s["cov"][2] == 0.0


def test_oracle_on_collinear_pixels_matches_the_one_dimensional_form():
    """n collinear pixels a distance s apart have a singular covariance; along the line m_j = t_j^2 s^2 / (s^2 var(t) + eps), a
    well-conditioned one-dimensional expression, and across it every centred coordinate is 0.  The oracle's exact route must give
    that for rows, diagonals and anti-diagonals alike (a float64 inverse with entries 1 / eps would not)."""
    eps = float(np.float32(1e-6))
    for n in (10, 12, 30, 100, 400):
        t = np.arange(n, dtype=np.float64)
        c = t - t.mean()
        for ys, xs, s2 in ((np.zeros(n), t, 1.0), (t, t, 2.0), (t, n - t, 2.0), (2 * t, t, 5.0)):
            want = float(np.mean((c * c * s2 / (s2 * c.var(ddof=1) + eps) - 1.0) ** 2))
            got = SO.shape(ys, xs)
            assert got["status"] == 0 and got["axes"][1] == 0.0 and got["fill"] == 0.0, (n, s2)
            assert rel(got["term"], want) <= 1e-12, (n, s2, got["term"], want)


def test_fixture_thin_objects(golden):
    g = golden["shapes"]
    assert g["thin_names"].tolist() == ["lines"]
    shapes = SO.shapes_of_labels(OO.label(g["thin_0_map"].astype(np.int64), 2))
    assert len(shapes) == 9 and all(s["status"] == 0 and 0.5 < s["term"] < 3.0 for s in shapes)
    assert sum(s["axes"][1] == 0.0 for s in shapes) == 6                       # the six exact diagonals: singular covariance
    assert all(s["lam"][0] > SO.THIN_RATIO * (s["lam"][1] + 1e-6) for s in shapes)


def test_python_names_are_exported():
    assert callable(mgunet.object_shapes) and "object_shapes" in mgunet.__all__ and "ObjectShapes" in mgunet.__all__
    fields = set(mgunet.ObjectShapes.__dataclass_fields__)
    assert {"centroid", "cov", "axes", "angle", "fill", "term", "status"} <= fields
    assert isinstance(mgunet.ObjectShapes.valid, property) and callable(mgunet.ObjectShapes.loss)


def test_new_symbols_declared_bound_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mgunet.h")).read(), flags=re.S)
    L = _lib.lib()
    for s in NEW:
        assert re.search(rf"\b{s}\s*\(", txt), s
        assert s in _lib._PROTOS and _lib._PROTOS[s][2], s          # declared, and takes the stream last
        assert hasattr(L, s), s


def test_entries_reject_a_null_context():
    L = _lib.lib()
    assert L.mgu_object_moments(None, None, 1, 1, 1, None, 0, None, None, None) == _lib.MGU_ERR_INVALID
    assert L.mgu_object_shapes(None, None, 1, 1, 1, None, 0, None, None, None, None, 1e-6, 10, None, None, None, None, None, None, None,
                               None) == _lib.MGU_ERR_INVALID
    assert L.mgu_elliptical_shape_loss_objects(None, 1, None, 0, None, None, None, 0, None, None) == _lib.MGU_ERR_INVALID
