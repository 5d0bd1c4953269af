"""CPU tier of object splitting: the numpy oracle of the GPU tests (split_objects_oracle.py) against scipy's exact Euclidean distance
transform and against the properties the definitions promise (two discs cut along their radical axis, filled ellipses left whole,
order-free ties, raster numbering, the min_area filter, the all-foreground sentinel), the yield dictionary of a scene of touching
pairs with and without the split, and the two C-ABI entries declared, bound and exported (no GPU needed)."""
import os
import re

import numpy as np
import pytest

import mgunet
import objects_oracle as OO
import split_objects_oracle as S
from mgunet import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (96, 128)


def _scenes():
    rng = np.random.default_rng(3)
    blobs = np.kron(rng.integers(0, 3, (6, 8)), np.ones((5, 5), np.int64))
    blobs[rng.random(blobs.shape) < 0.05] = 0
    edge = np.zeros((20, 30), np.int64)
    edge[2:18, 3:15], edge[2:18, 15:27] = 1, 2
    checker = (np.indices((9, 11)).sum(0) % 2) + 1
    return {"two_discs": S.two_discs(32)[0].astype(np.int64), "ellipse": S.ellipse(SHAPE, 48, 64, 30, 18, 0.3).astype(np.int64),
            "blobs": blobs, "edge": edge, "checker": checker, "negative": np.where(edge == 2, -7, edge)}


def test_oracle_d2_equals_scipy():
    from scipy import ndimage
    for name, lab in _scenes().items():
        d = S.d2(lab)
        assert d.dtype == np.int32 and not d[lab == 0].any(), name
        for k in np.unique(lab):
            if k != 0:
                ref = np.rint(ndimage.distance_transform_edt(lab == k) ** 2).astype(np.int64)
                assert np.array_equal(d[lab == k], ref[lab == k]), (name, k)


@pytest.mark.parametrize("sep", [24, 28, 32, 36, 39])
def test_two_discs_split_along_the_radical_axis(sep):
    mask, ((cy, c0), (_, c1)) = S.two_discs(sep)
    ys, xs = np.nonzero(mask)
    for r in (3, 5, 8):
        res = S.split(mask.astype(np.int64), r, 9)
        assert res["count"] == 2, (sep, r)
        lab = res["labels"]
        # equal radii: the radical axis is the perpendicular bisector x = (c0 + c1) / 2
        left, right = 2 * xs < c0 + c1, 2 * xs > c0 + c1
        assert left.any() and right.any()
        assert (lab[ys[left], xs[left]] == lab[cy, c0]).all() and (lab[ys[right], xs[right]] == lab[cy, c1]).all(), (sep, r)
        assert lab[cy, c0] != lab[cy, c1]


@pytest.mark.parametrize("axes", [(30, 18), (30, 24), (40, 16), (25, 12)])
def test_filled_ellipses_stay_whole(axes):
    for angle in (0, 0.3, 0.7, 1.2):
        mask = S.ellipse(SHAPE, 48, 64, axes[0], axes[1], angle)
        res = S.split(mask.astype(np.int64), 8, 9)
        assert res["count"] == 1 and np.array_equal(res["labels"] != 0, mask), (axes, angle)


def test_thin_component_is_returned_unchanged():
    lab = np.zeros((20, 40), np.int64)
    lab[5:9, 2:38] = 1        # 4 pixels thick: D2 <= 4 < 9
    lab[12, 3:30] = 2         # a one-pixel line
    res = S.split(lab, 5, 9)
    assert not res["seeds"].any() and res["count"] == 2
    assert np.array_equal(res["labels"], lab)


def test_result_does_not_depend_on_the_seed_order():
    rng = np.random.default_rng(11)
    bar = np.zeros((40, 90), np.int64)
    bar[10:31, 5:85] = 1      # a constant-width bar: a whole line of equal seeds, ties everywhere
    for lab in (bar, S.two_discs(28)[0].astype(np.int64)):
        ref = S.split(lab, 3, 9)
        assert ref["seeds"].sum() > 1
        for _ in range(3):
            got = S.split(lab, 3, 9, seed_order=lambda m: rng.permutation(m))
            assert np.array_equal(got["labels"], ref["labels"])


def test_numbering_is_raster_order_and_min_area_filters_after_the_split():
    lab = np.zeros((64, 160), np.int64)
    lab[S.disc(lab.shape, 40, 30, 12) | S.disc(lab.shape, 40, 48, 12)] = 1    # a pair, lower in the image
    lab[S.disc(lab.shape, 14, 120, 10)] = 2                                    # a single disc, higher: it comes first
    lab[50:53, 100:103] = 3                                                    # 9 pixels, no seed
    res = S.split(lab, 5, 9)
    out = res["labels"]
    assert res["count"] == 4
    firsts = [np.flatnonzero(out.reshape(-1) == k)[0] for k in range(1, 5)]
    assert firsts == sorted(firsts)
    assert out[14, 120] == 1 and out[40, 30] == 2 and out[40, 48] == 3 and out[51, 101] == 4
    cut = S.split(lab, 5, 9, min_area=30)
    assert cut["count"] == 3 and not cut["labels"][50:53, 100:103].any()
    assert np.array_equal(cut["labels"], np.where(out == 4, 0, out))
    big = S.split(lab, 5, 9, min_area=int((lab == 1).sum()) - 5)   # the pair passes as a whole, neither half does
    assert big["count"] == 0 or not big["labels"][lab == 1].any()


def test_one_label_full_image_hits_the_sentinel():
    res = S.split(np.full((9, 13), 4, np.int64), 3, 9)
    assert (res["d2"] == S.D2_NONE).all() and S.D2_NONE == 2 ** 30
    assert res["count"] == 1 and (res["labels"] == 1).all()


def test_three_discs_in_a_ring_give_a_fourth_cell():
    m = S.disc(SHAPE, 36, 50, 18) | S.disc(SHAPE, 36, 78, 18) | S.disc(SHAPE, 60, 64, 18)
    assert S.split(m.astype(np.int64), 5, 9)["count"] == 4   # documented: the enclosed centre peak is a cell of its own


def _object_lists(labels, values):
    cls, _, bbox, _ = OO.stats(labels, values)
    return [{"bbox": b, "class_id": c} for b, c in zip(bbox.tolist(), cls.tolist())]


def test_yield_metrics_of_touching_pairs():
    n = 3
    cmap, boxes = S.touching_pairs(n)
    gt = [[{"bbox": b, "class_id": 1} for b in boxes]]
    whole = OO.label(cmap, 2)
    off = mgunet.yield_estimation_metrics([2 * n], [int(whole.max())], gt, [_object_lists(whole, cmap)])
    assert off["total_pred_count_sum"] == n and off["object_matching_rate_perc"] == 0.0
    cut = S.split(whole, 5, 9)
    on = mgunet.yield_estimation_metrics([2 * n], [cut["count"]], gt, [_object_lists(cut["labels"], cmap)])
    assert on["total_pred_count_sum"] == 2 * n and on["total_gt_count_sum"] == 2 * n
    assert on["object_matching_rate_perc"] == (2 * n / (2 * n + 1e-6)) * 100 and round(on["object_matching_rate_perc"], 3) == 100.0
    assert on["count_accuracy_perc"] == 100.0 and on["yield_estimation_error_perc"] == 0.0
    assert on == S.touching_pairs_expected(n)


def test_new_symbols_declared_bound_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mgunet.h")).read(), flags=re.S)
    L = _lib.lib()
    for s in ("mgu_distance_transform", "mgu_split_objects"):
        assert re.search(rf"\b{s}\s*\(", txt), s
        assert s in _lib._PROTOS and _lib._PROTOS[s][2], s
        assert hasattr(L, s), s
    assert re.search(r"#define\s+MGU_D2_NONE\s+\(1 << 30\)", txt)
    assert callable(mgunet.split_objects) and callable(mgunet.distance_transform)


def test_entries_reject_a_null_context_and_python_rejects_bad_arguments():
    L = _lib.lib()
    assert L.mgu_distance_transform(None, None, 1, 1, 1, None, None) == _lib.MGU_ERR_INVALID
    assert L.mgu_split_objects(None, None, 1, 1, 1, 5, 9, 0, None, None, None, None, None, None) == _lib.MGU_ERR_INVALID
    from mgunet import objects
    assert objects._split_params(5, 3, 0) == (5, 9, 0) and objects._split_params(1, 2.5, 7) == (1, 7, 7)
    for bad in ((0, 3, 0), (17, 3, 0), (2.5, 3, 0), (5, 0, 0), (5, 3, -1)):
        with pytest.raises(ValueError):
            objects._split_params(*bad)
