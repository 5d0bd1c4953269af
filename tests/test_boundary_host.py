"""Boundary evaluation without a GPU: the scipy oracle (boundary_oracle.py) against brute force, the boundary as the pixels whose
squared distance transform is 1, the two-squares scene by hand, and mgunet.boundary_metrics on hand-made tables (quantile rank, overflow
rule, missing classes), plus the argument checks of the Python layer that need no device."""
import math

import numpy as np
import pytest
import torch
from scipy import ndimage

import boundary_oracle as K
import mgunet

NAN = float("nan")


def wrap(t, max_d2, band_r2):
    return mgunet.BoundaryTables(*t, max_d2, band_r2)


def same(a, b):
    """== with nan equal to nan"""
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_oracle_equals_brute_force_on_tiny_maps(seed):
    _, p, g = K.blob_pair((2, 9, 13), 3, seed)
    for max_d2, band_r2 in ((4, 1), (64, 5)):
        ref = K.brute_tables(p, g, 3, max_d2, band_r2)
        out = K.tables(p, g, 3, max_d2, band_r2)
        for a, b in zip(out, ref):
            assert np.array_equal(a, b)
    assert K.tables(p, g, 3, 4, 1)[1][:, :, :, 0].sum() > 0   # there were boundaries to measure


def test_oracle_equals_brute_force_on_lines_and_single_pixels():
    p, g = np.zeros((3, 1, 11), np.int64), np.zeros((3, 1, 11), np.int64)
    p[0, 0, 2:5], g[0, 0, 8] = 1, 1
    p[1, 0, :] = 2                                       # the whole image: no boundary, no band
    g[1, 0, 3] = 2
    p[2, 0, 0], g[2, 0, 10] = 1, 2                       # each class on one side only
    out, ref = K.tables(p, g, 3, 16, 2), K.brute_tables(p, g, 3, 16, 2)
    for a, b in zip(out, ref):
        assert np.array_equal(a, b)
    assert out[1][1, 1, 0].tolist() == [0, 0, 0, 0] and out[1][1, 1, 1].tolist() == [1, 1, 0, 0] and out[2][1, 1].tolist() == [0, 0, 1]


@pytest.mark.parametrize("seed", [4, 5])
def test_boundary_is_where_the_squared_distance_transform_is_one(seed):
    _, p, _ = K.blob_pair((2, 37, 65), 4, seed)
    for m in p:
        m = K.normalise(m, 4)
        for c in (1, 2, 3):
            d2 = np.rint(ndimage.distance_transform_edt(m == c) ** 2).astype(np.int64)
            assert np.array_equal(K.boundary(m, c), (d2 == 1) & ~(m == c).all())
            assert np.array_equal(d2[m == c], K.mask_d2(m == c)[m == c])


def test_two_squares_by_hand():
    p, g = K.two_squares()
    hist, stats, band = K.tables(p, g, 2, 16, 4)
    for d in (0, 1):
        assert stats[0, 0, d].tolist() == [28, 0, 9, 42 * 65536] and 42 * 65536 == 2752512
        assert {k: int(v) for k, v in enumerate(hist[0, 0, d]) if v} == {0: 10, 1: 4, 4: 4, 9: 10}
    assert band[0, 0].tolist() == [20, 48, 48]
    m = mgunet.boundary_metrics(wrap((hist, stats, band), 16, 4), tolerance=1.0)
    assert m["hausdorff"] == [3.0] and m["assd"] == [1.5] and m["boundary_iou"] == [20 / 76]
    assert m["bf_precision"] == [14 / 28] and m["bf_recall"] == [14 / 28] and m["bf_score"] == [0.5]
    assert m["hd95"] == [3.0] and m["images"] == [1] and m["missing"] == [0] and m["hd95_saturated"] == [0]
    assert m["mean_hausdorff"] == 3.0 and m["mean_boundary_iou"] == 20 / 76


def test_full_image_class_has_no_boundary_and_nan_metrics():
    full = np.ones((2, 7, 9), np.int64)
    hist, stats, band = K.tables(full, full, 2, 16, 4)
    assert not hist.any() and not stats.any() and not band.any()
    m = mgunet.boundary_metrics(wrap((hist, stats, band), 16, 4))
    for k in ("bf_precision", "bf_recall", "bf_score", "boundary_iou", "hausdorff", "hd95", "assd"):
        assert same(m[k], [NAN]) and math.isnan(m["mean_" + k])
    assert m["images"] == [0] and m["missing"] == [0]


def hand_tables(rows, max_d2=4, band=(0, 0, 0)):
    """one class, one image per row: rows of (dir-0 {d2: count}, dir-1 {d2: count}); a key of None is an unmatched pixel"""
    B = len(rows)
    hist, stats = np.zeros((B, 1, 2, max_d2 + 2), np.int64), np.zeros((B, 1, 2, 4), np.int64)
    for b, row in enumerate(rows):
        for d, cnt in enumerate(row):
            for k, v in cnt.items():
                hist[b, 0, d, max_d2 + 1 if k is None else min(k, max_d2 + 1)] += v
                stats[b, 0, d, 0] += v
                if k is None:
                    stats[b, 0, d, 1] += v
                else:
                    stats[b, 0, d, 2] = max(stats[b, 0, d, 2], k)
                    stats[b, 0, d, 3] += v * math.isqrt(k << 32)
    return wrap((hist, stats, np.tile(np.array(band, np.int64), (B, 1, 1))), max_d2, 1)


def test_quantile_rank_is_computed_in_integers():
    # n = 20: rank ceil(0.95 * 20) = 19 -> the 19th smallest; n = 21: rank 20
    t = hand_tables([({0: 18, 1: 1, 4: 1}, {0: 20}), ({0: 19, 1: 1, 4: 1}, {0: 21})])
    m = mgunet.boundary_metrics(t, tolerance=0)
    assert m["hd95"] == [1.0] and m["hausdorff"] == [2.0] and m["hd95_saturated"] == [0]
    assert mgunet.boundary_metrics(hand_tables([({0: 18, 4: 2}, {0: 20})]))["hd95"] == [2.0]
    assert mgunet.boundary_metrics(hand_tables([({0: 1, 4: 1}, {0: 1})]), quantile=0.5)["hd95"] == [0.0]
    assert mgunet.boundary_metrics(hand_tables([({0: 1, 4: 1}, {0: 1})]), quantile=1.0)["hd95"] == [2.0]
    assert m["bf_precision"] == [37 / 41] and m["bf_recall"] == [1.0]


def test_rank_in_the_overflow_bin_takes_the_exact_maximum():
    t = hand_tables([({0: 10, 100: 10}, {0: 20}), ({0: 20}, {1: 20})])
    m = mgunet.boundary_metrics(t)
    assert m["hd95_saturated"] == [1] and m["images"] == [2]
    assert m["hd95"] == [(10.0 + 1.0) / 2] and m["hausdorff"] == [(10.0 + 1.0) / 2]
    assert m["assd"] == [((10 * 10) / 40 + 20 / 40) / 2]


def test_missing_images_count_in_the_pooled_ratios_only():
    t = hand_tables([({0: 4}, {0: 4}), ({None: 6}, {}), ({}, {None: 2}), ({}, {})], band=(1, 2, 3))
    m = mgunet.boundary_metrics(t)
    assert m["images"] == [1] and m["missing"] == [2]
    assert m["hausdorff"] == [0.0] and m["hd95"] == [0.0] and m["assd"] == [0.0]
    assert m["bf_precision"] == [4 / 10] and m["bf_recall"] == [4 / 6] and m["bf_score"] == [2 * 0.4 * (4 / 6) / (0.4 + 4 / 6)]
    assert m["boundary_iou"] == [4 / (8 + 12 - 4)]
    none = mgunet.boundary_metrics(hand_tables([({None: 3}, {})]))
    assert none["bf_precision"] == [0.0] and same(none["bf_recall"], [NAN]) and same(none["bf_score"], [NAN]) and same(none["hausdorff"], [NAN])
    zero = mgunet.boundary_metrics(hand_tables([({100: 3}, {100: 3})]))
    assert zero["bf_score"] == [0.0] and zero["hausdorff"] == [10.0]
    empty = mgunet.boundary_metrics(hand_tables([]))
    assert same(empty["bf_score"], [NAN]) and empty["images"] == [0]


def test_metrics_arguments():
    t = hand_tables([({0: 4}, {0: 4})], max_d2=4)
    mgunet.boundary_metrics(t, tolerance=2.0)
    with pytest.raises(ValueError):
        mgunet.boundary_metrics(t, tolerance=2.3)        # 5 > max_d2
    with pytest.raises(ValueError):
        mgunet.boundary_metrics(t, tolerance=-1)
    for q in (0, 1.5, -0.1):
        with pytest.raises(ValueError):
            mgunet.boundary_metrics(t, quantile=q)
    with pytest.raises(ValueError):
        mgunet.boundary_metrics(mgunet.BoundaryTables(t.hist, t.stats, t.band, 5, 1))   # the histogram has max_d2 + 2 = 6 bins
    as_torch = mgunet.BoundaryTables(torch.from_numpy(t.hist), torch.from_numpy(t.stats), torch.from_numpy(t.band), 4, 1)
    assert mgunet.boundary_metrics(as_torch) == mgunet.boundary_metrics(t)


def test_python_layer_checks_its_arguments_without_a_device():
    m = torch.zeros((1, 8, 8), dtype=torch.int64)
    with pytest.raises(ValueError):
        mgunet.boundary_tables(m, m, 2, max_distance=0.5)
    with pytest.raises(ValueError):
        mgunet.boundary_tables(m, m, 2, max_distance=64.1)   # 4108 > 4096
    with pytest.raises(ValueError):
        mgunet.boundary_tables(m, m, 2, band_radius=0)
    with pytest.raises(RuntimeError):
        mgunet.boundary_tables(m, m, 2)                  # CPU tensors: there is no CPU fallback
    for kw in ({"num_classes": 1}, {"num_classes": 33}, {"max_distance": 65}, {"tolerance": 9, "max_distance": 8}, {"quantile": 0},
               {"band_radius": -1}):
        with pytest.raises(ValueError):
            mgunet.BoundaryEvaluator(**{"num_classes": 3, "device": "cuda:0", **kw})
    with pytest.raises(RuntimeError):
        mgunet.BoundaryEvaluator(3, "cpu")
    assert K.radius_sq(math.sqrt(13)) == 13 and K.default_band_r2(512, 512) == 209 and K.default_band_r2(8, 8) == 1
