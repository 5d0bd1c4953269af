"""The border weight map without a GPU: the two oracles of tests/border_cases.py against each other and against the kernels' own
method run in numpy, the cases against the wrong readings of the definition they are there to catch, the header's declarations and
the argument checks that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import border_cases as BC
import mgunet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(BC.cases())


@pytest.mark.parametrize("name", NAMES)
def test_the_two_oracles_and_the_kernels_method_agree(name):
    c, want = BC.cases()[name], BC.expected(name)
    assert c["labels"].dtype == np.int32 and c["labels"].ndim == 3 and c["labels"].shape[0] <= 3
    assert c["labels"].shape[1] <= 64 and c["labels"].shape[2] <= 700
    for what, got in (("edt", BC.by_edt(c["labels"])), ("method", BC.method(c["labels"]))):
        for key, g in zip(("d1sq", "d2sq", "nearest"), got):
            assert g.dtype == np.int32 and np.array_equal(g, want[key]), (name, what, key)
    lab = c["labels"]
    assert np.array_equal(want["d1sq"] == 0, lab != 0) and np.array_equal(want["nearest"][lab != 0], lab[lab != 0])
    assert bool((want["d2sq"] >= want["d1sq"]).all())
    for b in range(lab.shape[0]):                               # the sentinels follow the image's own object count
        n = len(np.unique(lab[b][lab[b] != 0]))
        assert bool((want["d1sq"][b] == BC.NONE).all()) == (n == 0) and bool((want["d2sq"][b] == BC.NONE).all()) == (n < 2)
        assert bool((want["nearest"][b] == 0).all()) == (n == 0)


def test_what_the_named_cases_are_there_for():
    e = BC.expected
    assert (e("tie_row")["d1sq"][0, 0, 2], e("tie_row")["d2sq"][0, 0, 2], e("tie_row")["nearest"][0, 0, 2]) == (4, 4, 3)
    late = e("tie_late_smaller_label")
    assert (late["d1sq"][0, 2, 2], late["d2sq"][0, 2, 2], late["nearest"][0, 2, 2]) == (4, 4, 1)
    assert e("abaa_alone")["d2sq"][0, 6, 0] == 25 and e("abaa_alone")["nearest"][0, 6, 0] == 6      # B is five rows up, behind two runs of A
    far = e("far_corner")
    assert far["d1sq"][0, 0, 0] == 63 * 63 + 699 * 699 and bool((far["d2sq"] == BC.NONE).all())
    assert set(np.unique(far["weight"]).tolist()) == {0.5, 1.25}                                    # class terms alone: no exponential term
    ids = BC.cases()["negative_sparse_ids"]["labels"]
    assert ids.min() == -2 ** 31 and ids.max() == 2 ** 31 - 1
    mixed = e("mixed_batch")
    assert bool((mixed["nearest"][1] == 7).all()) and bool((mixed["d2sq"][1] == BC.NONE).all()) and bool((mixed["d2sq"][2] < BC.NONE).all())
    t = BC.cases()["touching"]
    tgt = e("touching")["target"]
    assert (tgt != t["classes"]).sum() == 2 * 5 + 2 * 6 and tgt[1, 7, 9] == t["classes"][1, 7, 9] != 0
    assert bool((e("touching_background_2")["target"][tgt != t["classes"]] == 2).all())
    ign = e("class_ignore")
    cl = BC.cases()["class_ignore"]["classes"]
    assert bool((ign["weight"][cl == -100] <= 10.0).all()) and float(ign["weight"][1, 5, 5]) <= 10.0
    gap = e("two")["weight"]                                   # the weight peaks between the two objects, not far away from them
    assert gap[0, 4, 7] > gap[0, 0, 0] and gap.max() <= 2.0 + 10.0


def _outputs(name, variant):
    c = BC.cases()[name]
    if variant in ("second_pixel", "cityblock"):
        d = BC.brute(c["labels"], variant)
    elif variant == "sum_of_squares":
        d = BC.brute(c["labels"])
    else:
        d = BC.method(c["labels"], variant)
    w = BC.weights(d[0], d[1], c["classes"], c["class_weight"], c["w0"], c["sigma"], variant)
    return d + (w.astype(np.float32),)


@pytest.mark.parametrize("variant", BC.VARIANTS)
def test_the_cases_tell_the_wrong_variants_apart(variant):
    """second-nearest pixel for second-nearest label; one candidate per column; city-block distance; a column scan that forgets
    the older run on A, B, A; d1^2 + d2^2 for (d1 + d2)^2; ties to the larger label: each differs from the oracle on some case"""
    small = [n for n in NAMES if n != "far_corner"] if variant == "second_pixel" else NAMES
    caught = []
    for name in small:
        want = BC.expected(name)
        ref = (want["d1sq"], want["d2sq"], want["nearest"], want["weight"].astype(np.float32))
        if not all(np.array_equal(g, r) for g, r in zip(_outputs(name, variant), ref)):
            caught.append(name)
    assert caught, variant
    print(f"border variant {variant}: caught by {len(caught)} of {len(small)} cases ({', '.join(caught[:4])} ...)")
    if variant == "forget_older_run":
        assert "abaa_alone" in caught
    if variant == "tie_larger":
        assert "tie_row" in caught and "tie_late_smaller_label" in caught


def test_names_are_exported_and_declared():
    for name in ("border_distances", "border_weights"):
        assert name in mgunet.__all__ and callable(getattr(mgunet, name)), name
    header = open(os.path.join(ROOT, "include", "mgunet.h")).read()
    for name in ("mgu_border_weights", "mgu_pixel_ce_map", "mgu_pixel_ce_map_backward"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    protos = mgunet._lib.parse_header()
    assert all(protos[n][2] for n in ("mgu_border_weights", "mgu_pixel_ce_map", "mgu_pixel_ce_map_backward"))
    assert len(protos["mgu_border_weights"][1]) == 17                        # context and stream included
    assert protos["mgu_border_weights"][1][8] is ctypes.c_double and protos["mgu_border_weights"][1][9] is ctypes.c_double
    # the map entries take the old entries' arguments plus the map, after the class weights
    for old, new in (("mgu_pixel_ce", "mgu_pixel_ce_map"), ("mgu_pixel_ce_backward", "mgu_pixel_ce_map_backward")):
        a, b = protos[old][1], protos[new][1]
        assert len(b) == len(a) + 1 and b[:10] == a[:10] and b[10] is ctypes.c_void_p and b[11:] == a[10:]
    assert BC.NONE == 1 << int(re.search(r"#define\s+MGU_D2_NONE\s+\(1 << (\d+)\)", header).group(1))
    mk = open(os.path.join(ROOT, "mingraph-unet_amd", "csrc", "Makefile")).read()
    assert "border.hip" in mk and os.path.exists(os.path.join(ROOT, "mingraph-unet_amd", "csrc", "border.hip"))
    section = header[header.index("border weight map"):header.index("int mgu_border_weights")]
    assert "Scratch: 16 bytes per pixel" in " ".join(section.replace("*", " ").split())              # the header states the scratch


def test_argument_checks_that_need_no_device():
    from mgunet.border import border_options
    lab = torch.zeros(1, 4, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device"):
        mgunet.border_distances(lab)
    with pytest.raises(RuntimeError, match="HIP device"):
        mgunet.border_weights(lab)
    with pytest.raises(TypeError, match="integer"):
        mgunet.border_weights(torch.zeros(1, 4, 4))
    with pytest.raises(TypeError, match="integer"):
        mgunet.border_distances(torch.zeros(4, dtype=torch.int32))
    for kw, match in (({"sigma": 0.0}, "sigma"), ({"sigma": -1.0}, "sigma"), ({"sigma": float("nan")}, "sigma"), ({"w0": -0.5}, "w0"),
                      ({"w0": float("nan")}, "w0"), ({"class_weight": torch.ones(9)}, "class_weight"),
                      ({"class_weight": [1.0, 2.0]}, "class_weight"), ({"class_weight": torch.ones(3), "num_classes": 2}, "class_weight")):
        args = {"w0": 10.0, "sigma": 5.0}
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            border_options(**args)
    assert border_options(10, 5) == (10.0, 5.0) and border_options(0.0, 2.5, 3, torch.ones(3)) == (0.0, 2.5)
    with pytest.raises(ValueError, match="pixel_weight"):
        mgunet.losses.pixel_weight_map(torch.ones(2, 4, 4), torch.zeros(1, 2, 4, 4))
    assert mgunet.losses.pixel_weight_map(None, torch.zeros(1, 2, 4, 4)) is None


class NoModel:
    def named_parameters(self):
        raise AssertionError("the border options are checked before the model is touched")


@pytest.mark.parametrize("kw, match", [({"border_w0": -1.0}, "w0"), ({"border_sigma": 0.0}, "sigma"), ({"border_connectivity": 3}, "border_connectivity"),
                                       ({"border_w0": 10.0, "ce_weight": torch.ones(9)}, "class_weight")])
def test_trainer_refuses_bad_border_options_before_touching_the_model(kw, match):
    with pytest.raises(ValueError, match=match):
        mgunet.Trainer(NoModel(), **kw)
