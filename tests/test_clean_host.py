"""CPU tier of mask cleanup: the scipy oracle of the GPU tests (clean_oracle.py) against the exact Euclidean distance transform and
against the properties the definition promises (closing touches background only, opening is anti-extensive and idempotent, the quoted
scenes and counts, the pin-hole table of split_objects), and the C-ABI entry declared, bound and exported (no GPU needed)."""
import numpy as np
import pytest
from scipy import ndimage

import clean_oracle as K
import objects_oracle as OO
import split_objects_oracle as S
from mgunet import _lib

R2S = (1, 2, 4, 5, 8, 9, 64)


def blobs(seed, shape=(48, 70), classes=3):
    """a random class map of smooth blobs: the argmax of smoothed noise planes, sprinkled with single-pixel defects"""
    rng = np.random.default_rng(seed)
    planes = np.stack([ndimage.gaussian_filter(rng.standard_normal(shape), 3.0) for _ in range(classes)])
    planes[0] += 0.02
    m = planes.argmax(0).astype(np.int64)
    flip = rng.random(shape) < 0.03
    m[flip] = rng.integers(0, classes, shape)[flip]
    return m


def edt2(mask):
    """exact squared distance of every True pixel to the nearest False pixel of the image (a huge value when there is none)"""
    if mask.all():
        return np.full(mask.shape, 1 << 30, np.int64)
    return np.rint(ndimage.distance_transform_edt(mask) ** 2).astype(np.int64)


def test_disc_is_the_set_of_offsets_within_the_squared_radius():
    assert K.disc(1).sum() == 5 and K.disc(2).sum() == 9 and K.disc(4).sum() == 13 and K.disc(5).sum() == 21
    assert K.disc(64).shape == (17, 17) and K.disc(8).shape == (5, 5) and K.disc(9).shape == (7, 7)
    assert [K.radius_sq(r) for r in (0, 1, 1.5, 2, 2.3, 3, 8)] == [0, 1, 2, 4, 5, 9, 64]


@pytest.mark.parametrize("r2", R2S)
def test_open_equals_the_distance_transform_identities(r2):
    """erosion: p survives iff its squared distance to the nearest image pixel of another value exceeds r2 (outside does not count);
    dilation: p is kept iff an eroded pixel lies within r2"""
    for seed in (0, 1):
        m = blobs(seed)
        out = K.open_(m, 3, r2)
        for c in (1, 2):
            a = m == c
            e = a & (edt2(a) > r2)
            keep = a & (edt2(~e) <= r2) if e.any() else np.zeros_like(a)
            assert np.array_equal(out == c, keep), (seed, c)


@pytest.mark.parametrize("r2", R2S)
def test_close_equals_the_distance_transform_identities(r2):
    """on the padded plane: Dil = {distance to A <= r2}, Clo = {distance to the complement of Dil > r2}"""
    r = K.disc(r2).shape[0] // 2
    for seed in (0, 1):
        m = blobs(seed)
        out = K.close(m, 3, r2)
        expect = m.copy()
        for c in (2, 1):
            a = np.pad(m == c, 2 * r + 1)
            if not a.any():
                continue
            dil = edt2(~a) <= r2
            clo = (edt2(dil) > r2)[2 * r + 1:-2 * r - 1, 2 * r + 1:-2 * r - 1]
            expect[clo & (m == 0)] = c
        assert np.array_equal(out, expect), seed
        assert np.array_equal(out[m != 0], m[m != 0])          # closing touches background only


@pytest.mark.parametrize("r2", R2S)
def test_opening_is_anti_extensive_and_idempotent(r2):
    m = blobs(2)
    o = K.open_(m, 3, r2)
    assert np.array_equal(o[o != 0], m[o != 0]) and not o[m == 0].any()
    assert np.array_equal(K.open_(o, 3, r2), o)


def test_fill_is_idempotent_and_matches_binary_fill_holes_for_one_class():
    for seed in (0, 1, 2):
        m = (blobs(seed, classes=2) > 0).astype(np.int64)
        f = K.fill(m, 2)
        assert np.array_equal(f > 0, ndimage.binary_fill_holes(m > 0)), seed
        assert np.array_equal(K.fill(f, 2), f)
        f3 = K.fill(blobs(seed), 3)
        assert np.array_equal(K.fill(f3, 3), f3)


def test_values_out_of_range_are_background():
    m = np.array([[1, -100, 7, 2, 3, 0]])
    assert K.normalise(m, 3).tolist() == [[1, 0, 0, 2, 0, 0]]
    assert K.clean(m[None], 3, fill_holes=False)[0].tolist() == [[[1, 0, 0, 2, 0, 0]]]


def components(m):
    return int(OO.label(m, 2).max())


def test_bar_between_two_discs_opens_into_two():
    m = K.bar_scene()
    assert m.shape == (40, 72) and components(m) == 1
    assert components(K.open_(m, 2, 1)) == 2


def test_crack_through_a_disc_closes_into_one():
    m = K.crack_scene()
    assert components(m) == 2
    out, counts = K.clean(m[None], 2, close_r2=1, fill_holes=False)
    assert components(out[0]) == 1 and counts[0, 0] == (out[0] != m).sum() > 0 and counts[0, 1] == counts[0, 2] == 0


def test_diagonal_chain_is_three_components_and_the_one_on_the_ring_stays_open():
    m = K.chain_scene()
    out, counts = K.clean(m[None], 2)
    assert out[0, 1, 1] == 0 and out[0, 2, 2] == 1 and out[0, 3, 3] == 1
    assert counts[0].tolist() == [0, 2, 0]


def test_fill_rules_pocket_island_border_and_area():
    m = np.zeros((12, 20), np.int64)
    m[1:8, 1:8] = 1
    m[3:6, 3:6] = 0          # a hole of 9 pixels ...
    m[4, 4] = 2              # ... with an island of another class in it: the ring of 8 has neighbours of classes 1 and 2
    m[1:8, 10:14], m[1:8, 14:18] = 1, 2
    m[3:5, 13:15] = 0        # a pocket between classes 1 and 2
    m[9:12, 3:6] = 1
    m[10:12, 4] = 0          # a notch that touches the bottom border
    f = K.fill(m, 3)
    assert np.array_equal(f, m)
    m[4, 4] = 1              # the island is the ring's own class: the ring is a hole of 8 pixels, the island is untouched
    assert (K.fill(m, 3) != m).sum() == 8
    m[4, 4] = 0              # a plain hole of 9
    assert (K.fill(m, 3, 9) != m).sum() == 9 and (K.fill(m, 3, 8) != m).sum() == 0


def test_pin_holes_split_a_disc_and_hole_filling_restores_it():
    for holes, expected in K.PIN_HOLES:
        m = K.pin_hole_scene(holes)
        assert S.split(OO.label(m, 2))["count"] == expected, holes
        filled = K.clean(m[None], 2)[0][0]
        assert S.split(OO.label(filled, 2))["count"] == 1, holes


def test_clean_masks_is_declared_bound_and_exported():
    protos = _lib.parse_header()
    assert "mgu_clean_masks" in protos
    res, args, takes_stream = protos["mgu_clean_masks"]
    assert takes_stream and len(args) == 15
    assert hasattr(_lib.lib(), "mgu_clean_masks")
