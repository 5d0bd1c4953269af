"""CPU tier of object counting: mgunet.yield_estimation_metrics reproduces the reference's yield_estimation_metrics
(experiments/metrics.py:160-253) BITWISE on the fixture the reference itself wrote (tools/make_yield_golden.py), the numpy labelling
oracle of the GPU tests equals scipy.ndimage.label on the fixture's masks, and the three C-ABI entries are declared, bound and
exported (no GPU needed)."""
import os
import re

import numpy as np

import mgunet
import objects_oracle as OO
from mgunet import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mgu_connected_components", "mgu_object_stats", "mgu_match_objects")
KEYS = ("count_accuracy_perc", "yield_estimation_error_perc", "object_matching_rate_perc", "occlusion_robustness_perc",
        "total_gt_count_sum", "total_pred_count_sum")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _case(g, k):
    gt, pred = g[f"{k}_gt"].tolist(), g[f"{k}_pred"].tolist()
    if not int(g[f"{k}_lists"]):
        return gt, pred, None, None, 0.5
    n = int(g[f"{k}_nimg"])
    gl, pl = [[] for _ in range(n)], [[] for _ in range(n)]
    for r in g[f"{k}_gto"].tolist():
        d = {"bbox": r[1:5], "class_id": r[5]}
        if r[6] >= 0:
            d["occluded"] = bool(r[6])
        gl[r[0]].append(d)
    for r, c in zip(g[f"{k}_pro"].tolist(), g[f"{k}_prc"].tolist()):
        d = {"bbox": r[1:5], "class_id": r[5]}
        if not np.isnan(c):
            d["confidence"] = c
        pl[r[0]].append(d)
    return gt, pred, gl, pl, float(g[f"{k}_thresh"])


def test_fixture_covers_the_cases(golden):
    g = golden["objects"]
    n = int(g["ncases"])
    assert n >= 20
    assert any(int(g[f"{k}_nimg"]) > 0 and not g[f"{k}_gt"].any() for k in range(n))      # all-zero GT counts
    assert any(np.isinf(g[f"{k}_out"][1]) for k in range(n))                                # MAPE inf
    assert any(int(g[f"{k}_lists"]) and len(g[f"{k}_gto"]) == 0 for k in range(n))         # empty object lists
    assert any(g[f"{k}_out"][3] >= 0 for k in range(n))                                     # occluded GT objects
    assert any(0 < g[f"{k}_out"][2] for k in range(n))                                      # some matches


def test_yield_metrics_bitwise(golden):
    g = golden["objects"]
    for k in range(int(g["ncases"])):
        gt, pred, gl, pl, thresh = _case(g, k)
        res = mgunet.yield_estimation_metrics(gt, pred, gl, pl, matching_iou_thresh=thresh)
        assert list(res) == list(KEYS)
        assert np.array_equal(_bits([res[key] for key in KEYS]), _bits(g[f"{k}_out"])), k


def test_host_iou_exact_half():
    gl = [[{"bbox": [0, 0, 4, 4], "class_id": 1}]]
    pl = [[{"bbox": [0, 0, 4, 2], "class_id": 1}]]
    assert mgunet.yield_estimation_metrics([1], [1], gl, pl, 0.5)["object_matching_rate_perc"] > 99.99
    assert mgunet.yield_estimation_metrics([1], [1], gl, pl, 0.5000001)["object_matching_rate_perc"] == 0.0


def test_numpy_oracle_equals_scipy_golden(golden):
    g = golden["objects"]
    for j in range(int(g["nlab"])):
        m = g[f"lab_{j}_mask"]
        for c in (1, 2):
            assert np.array_equal(OO.label(m, c), g[f"lab_{j}_c{c}"]), (j, c)


def test_new_symbols_declared_bound_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mgunet.h")).read(), flags=re.S)
    L = _lib.lib()
    for s in NEW:
        assert re.search(rf"\b{s}\s*\(", txt), s
        assert s in _lib._PROTOS, s
        assert hasattr(L, s), s


def test_entries_reject_a_null_context():
    L = _lib.lib()
    assert L.mgu_connected_components(None, None, 0, 1, 1, 1, 0, 2, 0, 0, 0, None, None, None, None) == _lib.MGU_ERR_INVALID
    assert L.mgu_object_stats(None, None, None, 0, 1, 1, 1, 0, None, 0, None, None, None, None, None) == _lib.MGU_ERR_INVALID
    assert L.mgu_match_objects(None, 1, None, None, None, 0, None, None, None, 0, 0.5, None, None) == _lib.MGU_ERR_INVALID
