"""CPU tier of the segmentation evaluation: mgunet.metrics reproduces the reference's segmentation_metrics
(experiments/metrics.py:6-69) BITWISE on the fixture the reference itself wrote (tools/make_seg_metrics_golden.py), and the two
C-ABI entries reject bad arguments before any device work (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mgunet
from mgunet import _lib

KEYS = ("iou", "precision", "recall", "f1")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _cases(golden):
    g = golden["seg_metrics"]
    return g, int(g["ncases"])


def _check(res, g, k):
    assert res["confusion_matrix"].dtype == np.int64
    assert np.array_equal(res["confusion_matrix"], g[f"{k}_cm"])
    for key in KEYS:
        vals = res[f"{key}_per_class"]
        assert isinstance(vals, list) and all(isinstance(v, np.float64) for v in vals)
        assert np.array_equal(_bits(vals), _bits(g[f"{k}_{key}"])), (k, key)
    means = [res["mean_iou"], res["mean_precision"], res["mean_recall"], res["mean_f1"]]
    assert np.array_equal(_bits(means), _bits(g[f"{k}_means"])), k


def test_fixture_covers_the_cases(golden):
    g, n = _cases(golden)
    Cs = {int(g[f"{k}_C"]) for k in range(n)}
    smooths = {float(g[f"{k}_smooth"]) for k in range(n)}
    assert {1, 2, 3, 5, 16} <= Cs and {1e-6, 0.0, 1.0} <= smooths
    assert any((g[f"{k}_true"] == -100).any() for k in range(n))
    assert any(np.isnan(g[f"{k}_iou"]).any() for k in range(n))   # smooth = 0 with absent classes


def test_metrics_from_confusion_bitwise(golden):
    g, n = _cases(golden)
    for k in range(n):
        _check(mgunet.metrics_from_confusion(g[f"{k}_cm"], float(g[f"{k}_smooth"])), g, k)


@pytest.mark.parametrize("as_tensor", [False, True])
def test_host_segmentation_metrics_bitwise(golden, as_tensor):
    g, n = _cases(golden)
    for k in range(n):
        t, p = g[f"{k}_true"], g[f"{k}_pred"]
        if as_tensor:
            t, p = torch.from_numpy(t), torch.from_numpy(p)
        _check(mgunet.segmentation_metrics(t, p, int(g[f"{k}_C"]), smooth=float(g[f"{k}_smooth"])), g, k)


def test_host_segmentation_metrics_sklearn_errors():
    with pytest.raises(ValueError, match="At least one label"):
        mgunet.segmentation_metrics(np.array([-100, 5]), np.array([0, 1]), 2)
    with pytest.raises(ValueError):
        mgunet.segmentation_metrics(np.array([0, 1, 1]), np.array([0, 1]), 2)
    r = mgunet.segmentation_metrics(np.array([], np.int64), np.array([], np.int64), 3)
    assert r["confusion_matrix"].shape == (3, 3) and not r["confusion_matrix"].any()


def test_abi_rejects_null_ctx_and_bad_args():
    L = _lib.lib()
    buf = (C.c_int64 * 64)()
    dacc = (C.c_double * 2)()
    p = C.cast(buf, C.c_void_p)
    INV = _lib.MGU_ERR_INVALID
    # null ctx: rejected before anything else (no device is touched: this tier has none)
    assert L.mgu_segmentation_eval(None, p, p, 1, 4, 2, p, None, 0, 1.0, None, None) == INV
    assert L.mgu_confusion_matrix(None, p, p, 4, 2, p, None) == INV
    assert L.mgu_segmentation_eval(None, p, p, 1, 4, 2, p, None, 1, 1.0, C.cast(dacc, C.c_void_p), None) == INV


def test_abi_argument_checks_precede_device_work():
    """With a (non-null) context the argument checks still come first: a bad call fails with MGU_ERR_INVALID and a message,
    whether or not a device exists.  Without a GPU no context can be created, so this runs where one can."""
    if not torch.cuda.is_available():
        pytest.skip("mgu_create needs a HIP device; the null-ctx checks above cover this tier")
    L = _lib.lib()
    ctx = _lib.Context(0)
    buf = torch.zeros(64, dtype=torch.int64)
    p = buf.data_ptr()
    acc = torch.zeros(2, dtype=torch.float64).data_ptr()
    INV = _lib.MGU_ERR_INVALID
    bad = [
        (None, p, 1, 4, 2, p, None, 0, 1.0, None),       # null logits
        (p, None, 1, 4, 2, p, None, 0, 1.0, None),       # null labels
        (p, p, 1, 4, 2, None, None, 0, 1.0, None),       # null confusion
        (p, p, -1, 4, 2, p, None, 0, 1.0, None),         # negative B
        (p, p, 1, -4, 2, p, None, 0, 1.0, None),         # negative HW
        (p, p, 1, 4, 0, p, None, 0, 1.0, None),          # num_classes < 1
        (p, p, 1, 4, 2, p, None, 3, 1.0, acc),           # bad loss_kind
        (p, p, 1, 4, 2, p, None, -1, 1.0, None),
        (p, p, 1, 4, 2, p, None, 1, 1.0, None),          # loss without accumulator
        (p, p, 1, 4, 2, p, None, 0, 1.0, acc),           # accumulator without loss
        (p, p, 1, 4, 9, p, None, 2, 1.0, acc),           # dice with > 8 classes
    ]
    for args in bad:
        assert L.mgu_segmentation_eval(ctx.handle, *args, None) == INV, args
        assert L.mgu_last_error(ctx.handle)
    for args in [(None, p, 4, 2, p), (p, None, 4, 2, p), (p, p, 4, 2, None), (p, p, -1, 2, p), (p, p, 4, 0, p)]:
        assert L.mgu_confusion_matrix(ctx.handle, *args, None) == INV, args
