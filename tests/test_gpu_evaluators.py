"""What every evaluator's update() does before its kernels: the checks of the batch (mgunet._args.logits_and_masks through
metrics._Evaluator._batch), their order and their messages, the same for all four evaluators, and the NHWC storage read in place.  One
batch, B = 1, C = 2, 8 x 8, all-zero logits and masks; the dictionaries are the ones the evaluators gave before they shared the base."""
import math

import numpy as np
import pytest
import torch

import mgunet

pytestmark = pytest.mark.gpu

EVALUATORS = ["SegmentationEvaluator", "YieldEvaluator", "InstanceEvaluator", "BoundaryEvaluator"]
NAN = "nan"
# canon(compute()) after one update with the batch below, recorded at commit fe52fa2 (floats as repr, nan as "nan")
EXPECTED = {
    "SegmentationEvaluator": {
        "confusion_matrix": [[64, 0], [0, 0]], "f1_per_class": ["1.0", "1.0"], "iou_per_class": ["1.0", "1.0"], "mean_f1": "1.0",
        "mean_iou": "1.0", "mean_precision": "1.0", "mean_recall": "1.0", "precision_per_class": ["1.0", "1.0"],
        "recall_per_class": ["1.0", "1.0"]},
    "YieldEvaluator": {
        "count_accuracy_perc": "100.0", "object_matching_rate_perc": "0.0", "occlusion_robustness_perc": "-1.0",
        "total_gt_count_sum": 0, "total_pred_count_sum": 0, "yield_estimation_error_perc": 0},
    "InstanceEvaluator": {
        "AP50": "0.0", "AP75": "0.0", "AP_per_threshold": ["0.0"] * 10, "PQ": "0.0", "PQ_per_class": [NAN, NAN], "RQ": "0.0", "SQ": "0.0",
        "mAP": "0.0", "mask_matching_rate_perc": "0.0", "total_gt_count_sum": 0, "total_pred_count_sum": 0},
    "BoundaryEvaluator": {
        "assd": [NAN], "bf_precision": [NAN], "bf_recall": [NAN], "bf_score": [NAN], "boundary_iou": [NAN], "hausdorff": [NAN],
        "hd95": [NAN], "hd95_saturated": [0], "images": [0], "mean_assd": NAN, "mean_bf_precision": NAN, "mean_bf_recall": NAN,
        "mean_bf_score": NAN, "mean_boundary_iou": NAN, "mean_hausdorff": NAN, "mean_hd95": NAN, "missing": [0]},
}


def canon(v):
    """a dictionary of numpy / Python numbers as plain lists, ints and strings: floats by repr, so that == is bitwise and nan == nan"""
    if isinstance(v, dict):
        return {k: canon(x) for k, x in v.items()}
    if isinstance(v, np.ndarray):
        return canon(v.tolist())
    if isinstance(v, (list, tuple)):
        return [canon(x) for x in v]
    if isinstance(v, np.generic):
        v = v.item()
    if isinstance(v, float):
        return NAN if math.isnan(v) else repr(v)
    return v


@pytest.fixture(scope="module")
def batch(cuda):
    logits = torch.zeros(1, 8, 8, 2).permute(0, 3, 1, 2).to(cuda)        # the view UNet.forward returns: NHWC storage
    assert logits.permute(0, 2, 3, 1).is_contiguous()
    return logits, torch.zeros((1, 8, 8), dtype=torch.int64, device=cuda)


@pytest.mark.parametrize("name", EVALUATORS)
def test_update_checks_its_batch_in_one_order_with_one_set_of_messages(cuda, batch, name):
    """every case is wrong in its own respect and in all the later ones, so the exception names the check that comes first"""
    ev = getattr(mgunet, name)(2, cuda)
    logits, masks = batch
    short = masks[:, :, :7]
    cases = [(torch.zeros((1, 8, 8), dtype=torch.float16), RuntimeError, "logits must live on cuda:0"),
             (torch.zeros((1, 3, 8, 8), dtype=torch.float16, device=cuda), TypeError, "expected (B, C, H, W) float32 logits"),
             (torch.zeros((3, 8, 8), device=cuda), TypeError, "expected (B, C, H, W) float32 logits"),
             (torch.zeros((1, 3, 8, 8), device=cuda), ValueError, "logits have 3 classes, the evaluator 2"),
             (logits, ValueError, "masks shape (1, 8, 7) does not match logits (1, 8, 8)")]
    for bad, exc, msg in cases:
        with pytest.raises(exc) as e:
            ev.update(bad, short)
        assert type(e.value) is exc and str(e.value) == msg
    assert canon(ev.compute()) == canon(getattr(mgunet, name)(2, cuda).compute())   # a refused batch leaves nothing behind


@pytest.mark.parametrize("name", EVALUATORS)
def test_update_reads_the_storage_in_place_and_gives_the_recorded_dictionary(cuda, batch, name):
    ev = getattr(mgunet, name)(2, cuda)
    logits, masks = batch
    ptr = logits.data_ptr()
    nhwc, m, *shape = ev._batch(logits, masks)
    assert nhwc.data_ptr() == ptr and m.data_ptr() == masks.data_ptr() and shape == [1, 8, 8, 2]
    ev.update(logits, masks)
    got = ev.compute()
    assert logits.data_ptr() == ptr and not logits.any() and not masks.any()
    assert canon(got) == EXPECTED[name]
