"""The border weight map kernels (csrc/border.hip) on the GPU against the oracles of tests/border_cases.py: the distances, the nearest
label and the separated target bit for bit, the weight within one fp32 ulp of the float64 oracle rounded to fp32 (the device's fp64
exp may differ from libm's in the last fp64 bit; more than that is a bug), on every case; a row wide enough for the LDS opt-in;
against connected_components and distance_transform; every output alone; repeatability; the launch count; the refused arguments.
NOTES.md ("Border weight map") carries the lines these tests print under -s."""
import numpy as np
import pytest
import torch

import border_cases as BC
import mgunet
from mgunet import _lib

pytestmark = pytest.mark.gpu

NAMES = list(BC.cases())
OUTPUTS = ("d1sq", "d2sq", "nearest", "weight", "target")
DTYPE = {"d1sq": torch.int32, "d2sq": torch.int32, "nearest": torch.int32, "weight": torch.float32, "target": torch.int64}


def raw(cuda, c, outputs=OUTPUTS, fill=None):
    """mgu_border_weights on a case's inputs, writing only `outputs`: name -> device tensor"""
    lab = torch.from_numpy(c["labels"]).to(cuda)
    B, H, W = lab.shape
    cl = None if c["classes"] is None else torch.from_numpy(c["classes"]).to(cuda)
    cw = None if c["class_weight"] is None else torch.tensor(c["class_weight"], dtype=torch.float32, device=cuda)
    out = {k: (torch.empty((B, H, W), device=cuda, dtype=DTYPE[k]) if fill is None else torch.full((B, H, W), fill, device=cuda, dtype=DTYPE[k]))
           for k in outputs if not (k == "target" and cl is None)}
    _lib.call("mgu_border_weights", cuda, lab, B, H, W, cl, cw, 0 if cw is None else cw.numel(), float(c["w0"]), float(c["sigma"]),
              int(c["background"]), *(out.get(k) for k in OUTPUTS))
    return out


def ulps(got32, want64):
    """distance in fp32 ulps between got and the float64 oracle rounded to fp32 (all values are positive and finite)"""
    want32 = np.asarray(want64, np.float64).astype(np.float32)
    return np.abs(got32.view(np.int32).astype(np.int64) - want32.view(np.int32).astype(np.int64))


def check_against(name, c, got, want):
    for k in ("d1sq", "d2sq", "nearest"):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), (name, k)
    if "target" in got:
        assert np.array_equal(got["target"].cpu().numpy(), want["target"]), (name, "target")
    w = got["weight"].cpu().numpy()
    u = ulps(w, want["weight"])
    print(f"| border {name} {tuple(c['labels'].shape)} | weight ulps max {int(u.max())} | differing {int((u > 0).sum())} of {u.size} |")
    assert int(u.max()) <= 1, (name, int(u.max()))
    none = want["d2sq"] == BC.NONE                              # no second object: the class term alone, exactly
    cls_term = BC.weights(want["d1sq"], want["d2sq"], c["classes"], c["class_weight"], 0.0, c["sigma"]).astype(np.float32)
    assert np.array_equal(w[none], cls_term[none]), name


@pytest.mark.parametrize("name", NAMES)
def test_every_case_against_the_oracle(cuda, name):
    c = BC.cases()[name]
    check_against(name, c, raw(cuda, c), BC.expected(name))


def test_a_row_past_the_default_lds_budget(cuda):
    """16 bytes of LDS per pixel: a row of more than 4096 pixels needs the opt-in above 64 KiB"""
    lab = np.zeros((1, 2, 5000), np.int32)
    lab[0, 0, 7], lab[0, 1, 2600], lab[0, 0, 4999], lab[0, 1, 4100] = 3, 9, 3, -4
    c = {"labels": lab, "classes": None, "class_weight": None, "w0": 10.0, "sigma": 40.0, "background": 0}
    d1, d2, near = BC.brute(lab)
    want = {"d1sq": d1, "d2sq": d2, "nearest": near, "weight": BC.weights(d1, d2, None, None, 10.0, 40.0)}
    check_against("wide_row", c, raw(cuda, c), want)


def test_python_interface_is_the_raw_call(cuda):
    for name in ("touching_background_2", "class_ignore", "no_classes"):
        c = BC.cases()[name]
        got = raw(cuda, c)
        lab = torch.from_numpy(c["labels"]).to(cuda)
        d = mgunet.border_distances(lab)
        assert all(torch.equal(a, got[k]) for a, k in zip(d, ("d1sq", "d2sq", "nearest"))), name
        cl = None if c["classes"] is None else torch.from_numpy(c["classes"]).to(cuda)
        cw = None if c["class_weight"] is None else torch.tensor(c["class_weight"])
        kw = dict(classes=cl, class_weight=cw, w0=c["w0"], sigma=c["sigma"], background_class=c["background"])
        assert torch.equal(mgunet.border_weights(lab, **kw), got["weight"]), name
        if cl is not None:
            w, t = mgunet.border_weights(lab.to(torch.int64), separate=True, **kw)      # a wider integer map is read as int32
            assert torch.equal(w, got["weight"]) and torch.equal(t, got["target"]), name
    one = mgunet.border_distances(torch.from_numpy(BC.cases()["two"]["labels"][0]).to(cuda))    # (H, W): a batch of one
    assert tuple(one[0].shape) == (1, 7, 11)
    with pytest.raises(ValueError, match="separate"):
        mgunet.border_weights(torch.zeros(1, 4, 4, dtype=torch.int32, device=cuda), separate=True)


def test_on_connected_components_labels_and_against_distance_transform(cuda):
    c = BC.cases()["random_dense"]
    table = mgunet.connected_components(torch.from_numpy(c["classes"]).to(cuda))
    d1, d2, near = mgunet.border_distances(table)
    on = table.labels != 0
    assert bool(on.any()) and float(d1[on].abs().max()) == 0.0 and torch.equal(near[on], table.labels[on])
    assert bool((d1[~on] > 0).all()) and bool((d2 >= d1).all())
    for name in ("one", "far_corner"):                          # background and one label: d1sq is the distance transform of the inverted map
        lab = torch.from_numpy(BC.cases()[name]["labels"]).to(cuda)
        d1 = mgunet.border_distances(lab)[0]
        inv = (lab == 0).to(torch.int32)
        assert torch.equal(d1, mgunet.distance_transform(inv)), name


def test_each_output_alone_and_two_runs_are_bitwise_equal(cuda):
    for name in ("touching", "random_dense", "w257", "class_ignore"):
        c = BC.cases()[name]
        full, again = raw(cuda, c), raw(cuda, c)
        assert all(torch.equal(full[k], again[k]) for k in full), name
        for k in full:
            alone = raw(cuda, c, outputs=(k,))
            assert list(alone) == [k] and torch.equal(alone[k], full[k]), (name, k)


def count_launches(cuda, c, outputs):
    ctx = _lib.context(cuda)
    _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        raw(cuda, c, outputs)
        torch.cuda.synchronize(cuda)
        stats = _lib.read_kernel_stats(ctx)
    finally:
        _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 0), ctx.handle)
    assert all(k["name"].startswith("border_weights") for k in stats), stats
    return sum(k["launches"] for k in stats)


def test_exactly_two_launches(cuda):
    got = {}
    for name in ("two", "mixed_batch", "none", "checkerboard"):                 # B = 1, 3, 2, 1; 2, 0..3, 0 and 59 objects
        for outputs in (("d1sq", "d2sq", "nearest"), OUTPUTS, ("weight",)):
            got[(name, outputs)] = count_launches(cuda, BC.cases()[name], outputs)
    assert set(got.values()) == {2}, got


def test_invalid_arguments_return_invalid_and_launch_nothing(cuda):
    lab = torch.ones(1, 4, 4, dtype=torch.int32, device=cuda)
    cl = torch.zeros(1, 4, 4, dtype=torch.int64, device=cuda)
    cw = torch.ones(9, device=cuda)
    outs = [torch.full((16,), -5, dtype=DTYPE[k], device=cuda) for k in OUTPUTS]
    ok = dict(B=1, H=4, W=4, classes=cl, cw=None, ncls=0, w0=10.0, sigma=5.0)
    bad = [({"sigma": 0.0}, "sigma"), ({"sigma": -2.0}, "sigma"), ({"sigma": float("nan")}, "sigma"), ({"w0": -1.0}, "w0"),
           ({"B": 0}, "without pixels"), ({"H": 0}, "without pixels"), ({"W": 0}, "without pixels"), ({"classes": None}, "needs classes_dev"),
           ({"cw": cw, "ncls": 9}, "num_classes"), ({"cw": cw, "ncls": 0}, "num_classes"), ({"H": 16385}, "at most 16384"),
           ({"W": 16385}, "at most 16384"), ({"B": 65536}, "65535"), ({"B": 40000, "H": 300, "W": 300}, "2\\^31")]
    ctx = _lib.context(cuda)
    _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        for change, match in bad:
            a = dict(ok, **change)
            with pytest.raises(ValueError, match=match):
                _lib.call("mgu_border_weights", cuda, lab, a["B"], a["H"], a["W"], a["classes"], a["cw"], a["ncls"], a["w0"], a["sigma"], 0, *outs)
        with pytest.raises(ValueError, match="labels_dev"):
            _lib.call("mgu_border_weights", cuda, None, 1, 4, 4, cl, None, 0, 10.0, 5.0, 0, *outs)
        with pytest.raises(ValueError, match="LDS"):          # 256 KiB of row: more than a workgroup of this device can take
            _lib.call("mgu_border_weights", cuda, lab, 1, 1, 16384, cl, None, 0, 10.0, 5.0, 0, *outs)
        torch.cuda.synchronize(cuda)
        assert _lib.read_kernel_stats(ctx) == []
    finally:
        _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 0), ctx.handle)
    assert all(bool((o == -5).all()) for o in outs)
