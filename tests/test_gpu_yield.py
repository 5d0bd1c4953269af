"""Yield estimation on the MI355X: the device matching (mgu_match_objects) and YieldEvaluator against the host
yield_estimation_metrics on to_dicts() of the same objects, evaluate_yield on a small UNet, and EllipticalShapeLoss on the object
masks of a table."""
import numpy as np
import pytest
import torch

import mgunet
import mgunet_oracle as O

pytestmark = pytest.mark.gpu
KEYS = ("count_accuracy_perc", "yield_estimation_error_perc", "object_matching_rate_perc", "occlusion_robustness_perc",
        "total_gt_count_sum", "total_pred_count_sum")


def onehot_logits(cmap, C, dev, seed=0):
    """(B, C, H, W) view of NHWC logits whose first maximal class is cmap (ties broken towards the smaller class, as argmax)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 1, tuple(cmap.shape) + (C,), generator=g).float()
    x.scatter_(-1, cmap.unsqueeze(-1), 1.0)
    return x.to(dev).permute(0, 3, 1, 2)


def host_metrics(batches, C, connectivity=2, min_area=0, thresh=0.5, smooth=1e-6):
    gt_c, pr_c, gt_l, pr_l = [], [], [], []
    for logits, masks in batches:
        clean = torch.where((masks >= 0) & (masks < C), masks, torch.zeros_like(masks))
        tg = mgunet.connected_components(clean, connectivity=connectivity)
        tp = mgunet.connected_components(logits, connectivity=connectivity, min_area=min_area)
        gt_c += tg.counts.tolist()
        pr_c += tp.counts.tolist()
        gt_l += tg.to_dicts()
        pr_l += tp.to_dicts()
    return mgunet.yield_estimation_metrics(gt_c, pr_c, gt_l, pr_l, matching_iou_thresh=thresh, smooth=smooth)


def assert_same(a, b):
    assert list(a) == list(KEYS) and list(b) == list(KEYS)
    for k in KEYS:
        assert np.array_equal(np.float64(a[k]).view(np.uint64), np.float64(b[k]).view(np.uint64)), (k, a[k], b[k])


def designed_batch():
    """Image 0: IoU exactly 1/2 (GT [0,0,4,4], prediction [0,0,4,2]); image 1: a prediction at the same IoU (1/4) with two GT
    objects, the first must win; class 2 objects that overlap class 1 objects; image 2: no objects at all."""
    H, W = 40, 48
    gt = torch.zeros((3, H, W), dtype=torch.int64)
    pr = torch.zeros((3, H, W), dtype=torch.int64)
    gt[0, 0:4, 0:4] = 1
    pr[0, 0:2, 0:4] = 1
    gt[0, 20:30, 20:30] = 2
    pr[0, 22:30, 20:30] = 1                                                 # right place, wrong class
    pr[0, 31:35, 20:30] = 2
    gt[1, 10:14, 0:4] = 1
    gt[1, 10:14, 6:10] = 1
    pr[1, 10:14, 2:8] = 1
    gt[1, 30:34, 30:34] = 2
    pr[1, 30:34, 30:36] = 2
    return gt, pr


@pytest.mark.parametrize("thresh", [0.5, 0.25, 0.5000001, 0.0])
def test_device_matching_equals_host(cuda, thresh):
    gt, pr = designed_batch()
    logits = onehot_logits(pr, 3, cuda)
    ev = mgunet.YieldEvaluator(3, cuda, iou_thresh=thresh)
    ev.update(logits, gt.to(cuda))
    assert_same(ev.compute(), host_metrics([(logits, gt.to(cuda))], 3, thresh=thresh))


def test_no_objects(cuda):
    z = torch.zeros((2, 16, 16), dtype=torch.int64)
    logits = onehot_logits(z, 2, cuda)
    ev = mgunet.YieldEvaluator(2, cuda)
    ev.update(logits, z.to(cuda))
    res = ev.compute()
    assert_same(res, host_metrics([(logits, z.to(cuda))], 2))
    assert res["object_matching_rate_perc"] == 0.0 and res["total_gt_count_sum"] == 0
    assert_same(mgunet.YieldEvaluator(2, cuda).compute(), mgunet.yield_estimation_metrics([], []))


def random_batch(B, C, H, W, seed, dev):
    g = torch.Generator().manual_seed(seed)
    blocks = torch.randint(0, C, (B, H // 8 + 1, W // 8 + 1), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W]
    noise = torch.randint(0, C, (B, H, W), generator=g)
    flip = torch.rand((B, H, W), generator=g) < 0.05
    gt = torch.where(flip, noise, blocks)
    shift = torch.roll(blocks, shifts=(1, 2), dims=(1, 2))
    pr = torch.where(torch.rand((B, H, W), generator=g) < 0.03, noise, shift)
    gt[torch.rand((B, H, W), generator=g) < 0.02] = -100
    return onehot_logits(pr, C, dev, seed), gt.to(dev)


@pytest.mark.parametrize("C,connectivity,min_area", [(2, 2, 0), (3, 1, 0), (4, 2, 3)])
def test_evaluator_over_batches_equals_host(cuda, C, connectivity, min_area):
    batches = [random_batch(B, C, H, W, seed, cuda) for seed, (B, H, W) in enumerate([(2, 64, 80), (1, 130, 70), (3, 33, 200)])]
    ev = mgunet.YieldEvaluator(C, cuda, connectivity=connectivity, min_area=min_area)
    for lg, m in batches:
        ev.update(lg, m)
    res = ev.compute()
    assert res["total_gt_count_sum"] > 10 and 0 < res["object_matching_rate_perc"] < 100
    assert_same(res, host_metrics(batches, C, connectivity, min_area))
    ev.reset()
    ev.update(*batches[0])
    assert_same(ev.compute(), host_metrics(batches[:1], C, connectivity, min_area))


def test_evaluate_yield_small_unet(cuda):
    cfg = (3, 2, 8, 2)
    model = mgunet.UNet(*cfg)
    model.load_state_dict(O.make_unet_params(*cfg, seed=9))
    model = model.to(cuda)
    g = torch.Generator().manual_seed(5)
    loader = [(torch.randn((b, 3, 32, 48), generator=g), torch.randint(0, 2, (b, 32, 48), generator=g)) for b in (2, 1)]
    model.train()
    res = mgunet.evaluate_yield(model, loader)
    assert model.training
    model.eval()
    with torch.no_grad():
        batches = [(model(x.to(cuda))[0], y.to(cuda)) for x, y in loader]
    assert_same(res, host_metrics(batches, 2))
    model.eval()
    mgunet.evaluate_yield(model, loader)
    assert not model.training


def test_shape_loss_on_table_masks(cuda):
    g = torch.Generator().manual_seed(13)
    B, H, W = 2, 48, 64
    cmap = torch.zeros((B, H, W), dtype=torch.int64)
    cmap[0, 5:20, 5:30] = 1
    cmap[0, 25:45, 40:50] = 1
    cmap[1, 10:40, 10:20] = 1
    cmap[1, 2:8, 50:60] = 1
    t = mgunet.connected_components(cmap.to(cuda))
    assert t.counts.tolist() == [2, 2]
    by_hand = [[t.labels[b] == k for k in range(1, int(t.counts[b]) + 1)] for b in range(B)]
    probs = torch.softmax(torch.randn((B, 2, H, W), generator=g), 1).to(cuda)
    loss = mgunet.EllipticalShapeLoss()
    assert torch.equal(loss(probs, t.masks()), loss(probs, by_hand))
    assert float(loss(probs, t.masks())) != 0.0
