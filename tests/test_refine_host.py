"""The host side of the edge-aware refinement (mgunet.refine, csrc/refine.hip): the numpy oracle of tests/refine_oracle.py against a
per-pixel loop, mgunet.bilateral_tables, and two scenarios whose outcome is known in advance -- saturation and an outline that snaps onto
a colour edge.  No GPU."""
import math

import numpy as np
import pytest

import mgunet
import refine_oracle as R


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("r", [1, 3, 7])
def test_oracle_matches_the_brute_force(r, C, G):
    space, rng, shift = R.tables(r, 1.5 + r / 3.0, 25.0)
    for H, W in ((1, 1), (1, 7), (7, 1), (5, 9)):
        rs = np.random.RandomState(H * 100 + W * 10 + C + G + r)
        x = rs.uniform(-0.2, 1.2, (2, H, W, C)).astype(np.float32)
        guide = rs.randint(0, 256, (2, H, W, G)).astype(np.uint8)
        for T in (1, 2):
            fast = R.refine(x, guide, space, rng, shift, T)
            slow = R.refine(x, guide, space, rng, shift, T, step=R.iterate_brute)
            for a, b in zip(fast, slow):
                assert a.dtype == b.dtype and np.array_equal(a, b), (H, W, T)


def test_quantisation_clamps_rounds_to_even_and_maps_nan_to_zero():
    x = np.array([np.nan, -1.0, -0.0, 0.0, 1.0, 2.0, np.inf, -np.inf, 0.5, 1.5 / 65535, 2.5 / 65535, 7.62951e-06], np.float32)
    want = [0, 0, 0, 0, 65535, 65535, 65535, 0, int(np.rint(np.float32(0.5) * np.float32(65535)))]
    got = R.quantise(x)
    assert got[:9].tolist() == want and got.dtype == np.int64
    assert got[8] == 32768                                   # 32767.5 rounds to the even neighbour
    assert int(got.min()) >= 0 and int(got.max()) <= 65535


def test_bilateral_tables_values_symmetry_and_shift():
    space, rng, shift = mgunet.bilateral_tables(5, 3.0, 12.0)
    assert space.dtype == np.int32 and rng.dtype == np.int32 and space.shape == (6, 6) and rng.shape == (1024,)
    assert space[0, 0] == 256 and rng[0] == 256
    assert space[0, 1] == int(np.rint(256.0 * math.exp(-1.0 / 18.0))) == 242
    assert space[3, 4] == int(np.rint(256.0 * math.exp(-25.0 / 18.0))) == 64
    assert space[5, 5] == int(np.rint(256.0 * math.exp(-50.0 / 18.0))) == 16
    assert np.array_equal(space, space.T)
    assert shift == 1                                        # ceil(12.5 * 144) = 1800: 1800 >> 1 = 900 <= 1023
    assert rng[1] == int(np.rint(256.0 * math.exp(-2.0 / 288.0))) == 254
    assert rng[900] == int(np.rint(256.0 * math.exp(-1800.0 / 288.0))) == 0
    assert (np.diff(rng) <= 0).all() and (np.diff(space, axis=0) <= 0).all()
    for r, ss, sc in ((1, 0.5, 1.0), (3, 2.0, 12.0), (7, 4.0, 40.0), (7, 1e6, 1e6)):
        got, want = mgunet.bilateral_tables(r, ss, sc), R.tables(r, ss, sc)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
        assert 0 <= int(got[0].min()) and int(got[0].max()) <= 256 and 0 <= int(got[1].min()) and int(got[1].max()) <= 256
    shifts = {sc: mgunet.bilateral_tables(3, 2.0, sc)[2] for sc in (1.0, 12.0, 40.0, 1e6)}
    assert shifts == {1.0: 0, 12.0: 1, 40.0: 5, 1e6: 8}      # 13; 1800 >> 1; 20000 >> 5 = 625; no shift up to 8 is enough
    assert isinstance(shifts[1.0], int)


def test_bilateral_tables_refuse_bad_parameters():
    for r in (0, 8, -1, 2.5, True):
        with pytest.raises(ValueError):
            mgunet.bilateral_tables(r, 3.0, 12.0)
    for ss, sc in ((0.0, 12.0), (-1.0, 12.0), (3.0, 0.0), (3.0, -2.0), (math.nan, 12.0), (3.0, math.inf), (math.inf, 12.0), (3.0, math.nan)):
        with pytest.raises(ValueError):
            mgunet.bilateral_tables(5, ss, sc)
    for T in (0, 17):
        with pytest.raises(ValueError):
            mgunet.EdgeRefiner(5, 3.0, 12.0, T)
    assert mgunet.EdgeRefiner(7, 2.0, 9.0, 16).tables[0].shape == (8, 8)


def saturation_case():
    """a flat guide, all probabilities 1.0, r = 7, both sigmas 1e6: every weight is 256"""
    space, rng, shift = mgunet.bilateral_tables(7, 1e6, 1e6)
    assert (space == 256).all() and (rng == 256).all()
    x = np.ones((1, 20, 37, 3), np.float32)
    guide = np.full((1, 20, 37, 3), 77, np.uint8)
    return x, guide, space, rng, shift


def test_saturation_reaches_the_numerator_bound_and_stays_exact():
    x, guide, space, rng, shift = saturation_case()
    assert 225 * 256 * 65535 == 3774816000 < 2 ** 32
    for T in (1, 3):
        probs, labels, conf, changed, q = R.refine(x, guide, space, rng, shift, T)       # iterate() asserts num < 2^32 itself
        assert (q == 65535).all() and (probs == 1.0).all() and (conf == 1.0).all() and not labels.any() and changed.tolist() == [0]


@pytest.mark.parametrize("one_hot", [False, True])
def test_the_outline_snaps_onto_the_colour_edge(one_hot):
    x, guide = R.snap_scene(one_hot)
    before = R.outline_columns(R.first_max(R.quantise(x)))
    assert set(before) == ({27} if one_hot else {28})        # the ramp is exactly 0.5 at column 27: that tie goes to class 0
    space, rng, shift = mgunet.bilateral_tables(5, 3.0, 12.0)
    four = R.refine(x, guide, space, rng, shift, 4)
    assert R.outline_columns(four[1][0]) == [24] * 48
    assert four[3].tolist() == [48 * (before[0] - 24)]
    two = R.outline_columns(R.refine(x, guide, space, rng, shift, 2)[1][0])
    assert set(two) == ({24, 25} if one_hot else {25, 26})
