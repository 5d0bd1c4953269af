"""mgu_match_objects on the MI355X, driven through the C-ABI with the hand-built object tables of tests/objects_cases.py: no images
are involved.  Every designed case is built so that one wrong decision of match_kernel -- the tie-break across lanes and strides,
"strictly larger beats earlier", the used flags across strides, >= at the threshold, the class filter, a best below the threshold
-- changes totals[2]; tests/test_objects_cases_host.py shows that on restated wrong matchers.  The reference is the plain greedy
loop objects_cases.match_reference; totals are integers and compared exactly."""
import numpy as np
import pytest
import torch

import objects_cases as OC
from mgunet import _lib

pytestmark = pytest.mark.gpu


def device_tables(cuda, images):
    return [torch.from_numpy(a).to(cuda) for a in OC.tables(images)]


def match(cuda, gt, pred, thresh, totals=None, gt_capacity=None, pred_capacity=None):
    """totals after mgu_match_objects on the per-image object lists gt and pred (added to `totals` when given)"""
    (goff, gcls, gbox), (poff, pcls, pbox) = device_tables(cuda, gt), device_tables(cuda, pred)
    if totals is None:
        totals = torch.zeros(3, device=cuda, dtype=torch.int64)
    gcap = gcls.numel() if gt_capacity is None else gt_capacity
    pcap = pcls.numel() if pred_capacity is None else pred_capacity
    _lib.call("mgu_match_objects", cuda, len(gt), goff, gcls, gbox, gcap, poff, pcls, pbox, pcap, float(thresh), totals)
    return totals


@pytest.mark.parametrize("name", list(OC.MATCH_CASES))
def test_designed_case(cuda, name):
    c = OC.MATCH_CASES[name]
    want = OC.match_reference(c["gt"], c["pred"], c["thresh"])
    assert want[2] == c["matched"]
    assert match(cuda, [c["gt"]], [c["pred"]], c["thresh"]).tolist() == want


def test_designed_cases_as_one_batch(cuda):
    """the cases that share a threshold as the images of one call: every workgroup keeps its own used flags and count"""
    for thresh in (0.25, 0.5):
        cases = [c for c in OC.MATCH_CASES.values() if c["thresh"] == thresh]
        assert len(cases) >= 3
        want = np.sum([OC.match_reference(c["gt"], c["pred"], thresh) for c in cases], axis=0)
        assert match(cuda, [c["gt"] for c in cases], [c["pred"] for c in cases], thresh).tolist() == want.tolist()


@pytest.mark.parametrize("NP", OC.PRED_SIZES)
@pytest.mark.parametrize("G", OC.GT_SIZES)
def test_sizes(cuda, G, NP):
    gt, pred = OC.lattice_case(G, NP)
    for thresh in (0.5, 0.2):
        assert match(cuda, [gt], [pred], thresh).tolist() == OC.match_reference(gt, pred, thresh), thresh


def batch_of_five():
    images = [OC.lattice_case(G, NP) for G, NP in OC.MATCH_BATCH]
    return [g for g, _ in images], [p for _, p in images]


def test_batch_equals_the_sum_of_its_images_and_calls_accumulate(cuda):
    gt, pred = batch_of_five()
    thresh = 0.3
    per_image = [OC.match_reference(g, p, thresh) for g, p in zip(gt, pred)]
    assert all(0 < m[2] < m[0] for m in per_image if m[0] > 1 and m[1] > 1)
    for g, p, want in zip(gt, pred, per_image):                                    # B = 1 calls on the sliced tables
        assert match(cuda, [g], [p], thresh).tolist() == want
    whole = np.sum(per_image, axis=0).tolist()
    totals = match(cuda, gt, pred, thresh)
    assert totals.tolist() == whole
    assert match(cuda, gt, pred, thresh, totals=totals).tolist() == [2 * v for v in whole]   # a second call adds to the first


@pytest.mark.parametrize("side", ["gt", "pred"])
def test_capacity_one_below_the_last_image_skips_it(cuda, side):
    gt, pred = batch_of_five()
    thresh = 0.3
    assert len(gt[-1]) >= 1 and len(pred[-1]) >= 1
    n = sum(len(objs) for objs in (gt if side == "gt" else pred))
    got = match(cuda, gt, pred, thresh, **{side + "_capacity": n - 1})
    want = np.sum([OC.match_reference(g, p, thresh) for g, p in zip(gt[:-1], pred[:-1])], axis=0)   # the last image adds nothing
    assert got.tolist() == want.tolist()
    assert match(cuda, gt, pred, thresh, **{side + "_capacity": n}).tolist() == (want + OC.match_reference(gt[-1], pred[-1], thresh)).tolist()
