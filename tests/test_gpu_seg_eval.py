"""Device-side segmentation evaluation (csrc/seg_eval.hip, mgunet.metrics) on the MI355X.  Expected values come from numpy
(np.bincount) and torch on the host -- never from sklearn or the reference."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mgunet
import mgunet_oracle as O

pytestmark = pytest.mark.gpu


def host_cm(y, pred, C):
    y, pred = y.reshape(-1).numpy(), pred.reshape(-1).numpy()
    keep = (y >= 0) & (y < C) & (pred >= 0) & (pred < C)
    return np.bincount(y[keep] * C + pred[keep], minlength=C * C).reshape(C, C)


def tie_logits(B, C, H, W, seed):
    """Integer-valued logits in [-2, 2]: many exact ties between classes."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, (B, H, W, C), generator=g).float()


def noisy_labels(B, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, C, (B, H, W), generator=g)
    r = torch.rand((B, H, W), generator=g)
    y[r < 0.08] = -100
    y[(r >= 0.08) & (r < 0.12)] = C + 3
    y[(r >= 0.12) & (r < 0.14)] = -7
    return y


def nchw_view(nhwc_host, dev, offset=0):
    """(B,C,H,W) view of NHWC device storage (what UNet.forward returns); offset > 0 shifts the storage by that many floats."""
    B, H, W, C = nhwc_host.shape
    buf = torch.empty(nhwc_host.numel() + offset, device=dev)
    v = buf[offset:].view(B, H, W, C)
    v.copy_(nhwc_host.to(dev))
    return v.permute(0, 3, 1, 2)


@pytest.mark.parametrize("C", [1, 2, 3, 4, 7, 16, 80])
@pytest.mark.parametrize("shape", [(3, 17, 23), (2, 64, 64), (1, 1, 1), (3, 129, 131)])
def test_counts_and_predictions_exact(cuda, C, shape):
    B, H, W = shape
    lg = tie_logits(B, C, H, W, seed=C * 100 + H)
    y = noisy_labels(B, H, W, C, seed=C + W)
    logits = nchw_view(lg, cuda)
    ev = mgunet.SegmentationEvaluator(C, cuda)
    pred = ev.update(logits, y.to(cuda), return_pred=True)
    ref_pred = torch.argmax(lg.permute(0, 3, 1, 2), 1)                     # first maximal index, ties included
    assert torch.equal(pred.cpu(), ref_pred)
    assert torch.equal(pred, mgunet.argmax_classes(logits))                # bit-identical to mgu_argmax_classes
    res = ev.compute()
    assert np.array_equal(res["confusion_matrix"], host_cm(y, ref_pred, C))
    ev.update(logits, y.to(cuda))                                          # without the prediction map: same counts, added
    assert np.array_equal(ev.compute()["confusion_matrix"], 2 * host_cm(y, ref_pred, C))


@pytest.mark.parametrize("C", [2, 3])
def test_unaligned_storage_takes_the_generic_path(cuda, C):
    B, H, W = 2, 31, 37
    lg = tie_logits(B, C, H, W, seed=7)
    y = noisy_labels(B, H, W, C, seed=8)
    ev = mgunet.SegmentationEvaluator(C, cuda)
    pred = ev.update(nchw_view(lg, cuda, offset=1), y.to(cuda), return_pred=True)
    ref_pred = torch.argmax(lg.permute(0, 3, 1, 2), 1)
    assert torch.equal(pred.cpu(), ref_pred)
    assert np.array_equal(ev.compute()["confusion_matrix"], host_cm(y, ref_pred, C))


def test_flagship_shape_c2(cuda):
    B, H, W, C = 8, 512, 512, 2
    g = torch.Generator().manual_seed(3)
    lg = torch.randn((B, H, W, C), generator=g)
    y = torch.randint(0, 2, (B, H, W), generator=g)
    ev = mgunet.SegmentationEvaluator(C, cuda)
    pred = ev.update(nchw_view(lg, cuda), y.to(cuda), return_pred=True)
    ref_pred = torch.argmax(lg.permute(0, 3, 1, 2), 1)
    assert torch.equal(pred.cpu(), ref_pred)
    assert np.array_equal(ev.compute()["confusion_matrix"], host_cm(y, ref_pred, C))


@pytest.mark.parametrize("C", [2, 5, 16])
def test_accumulation_over_batches_equals_one_batch(cuda, C):
    parts = [(tie_logits(b, C, 19, 21, seed=40 + b), noisy_labels(b, 19, 21, C, seed=50 + b)) for b in (1, 2, 3)]
    ev = mgunet.SegmentationEvaluator(C, cuda)
    for lg, y in parts:                                                    # no host synchronisation in between
        ev.update(nchw_view(lg, cuda), y.to(cuda))
    many = ev.compute()
    one = mgunet.SegmentationEvaluator(C, cuda)
    one.update(nchw_view(torch.cat([p[0] for p in parts]), cuda), torch.cat([p[1] for p in parts]).to(cuda))
    assert np.array_equal(many["confusion_matrix"], one.compute()["confusion_matrix"])
    ev.reset()
    assert not ev.compute()["confusion_matrix"].any()


def ref_dice(logits64, y, smooth):
    """dice_loss of scripts/train_segmentation.py:29-40, restated in float64."""
    pr = torch.softmax(logits64, dim=1)
    oh = F.one_hot(y, num_classes=pr.shape[1]).permute(0, 3, 1, 2).double()
    inter = (pr * oh).sum(dim=(2, 3))
    union = pr.sum(dim=(2, 3)) + oh.sum(dim=(2, 3))
    return 1.0 - ((2.0 * inter + smooth) / (union + smooth)).mean()


@pytest.mark.parametrize("loss", ["ce", "ce+dice"])
@pytest.mark.parametrize("C", [2, 3, 5, 12])
def test_loss_matches_float64_and_is_reproducible(cuda, loss, C):
    if loss == "ce+dice" and C > 8:
        pytest.skip("the dice loss takes num_classes <= 8 (as mgu_dice_loss)")
    g = torch.Generator().manual_seed(C)
    batches = []
    for b, (H, W) in zip((2, 3, 1), ((33, 35), (16, 16), (65, 63))):
        lg = torch.randn((b, H, W, C), generator=g) * 3
        y = torch.randint(0, C, (b, H, W), generator=g)
        if loss == "ce":
            y[torch.rand((b, H, W), generator=g) < 0.1] = -100          # ignore_index: left out of the mean
        batches.append((lg, y))
    expect = []
    for lg, y in batches:
        l64 = lg.permute(0, 3, 1, 2).double()
        v = F.cross_entropy(l64, y, ignore_index=-100)
        if loss == "ce+dice":
            v = v + ref_dice(l64, y, 1.0)
        expect.append(float(v))
    accs = []
    for _ in range(2):
        ev = mgunet.SegmentationEvaluator(C, cuda, loss=loss)
        for lg, y in batches:
            ev.update(nchw_view(lg, cuda), y.to(cuda))
        res = ev.compute()
        accs.append(ev.loss_acc.cpu().numpy().copy())
        assert res["loss"] == pytest.approx(np.mean(expect), rel=1e-6)
    assert accs[0][1] == len(batches)
    assert np.array_equal(accs[0].view(np.uint64), accs[1].view(np.uint64))   # bitwise, run to run


@pytest.mark.parametrize("loss,label", [("ce", 2), ("ce", -5), ("ce+dice", -100), ("ce+dice", 9)])
def test_invalid_labels_raise_at_compute(cuda, loss, label):
    lg = tie_logits(2, 2, 8, 8, seed=1)
    y = torch.randint(0, 2, (2, 8, 8))
    y[1, 3, 4] = label
    ev = mgunet.SegmentationEvaluator(2, cuda, loss=loss)
    ev.update(nchw_view(lg, cuda), y.to(cuda))                             # does not raise: the host is not synchronised
    with pytest.raises(ValueError, match="label"):
        ev.compute()
    ev2 = mgunet.SegmentationEvaluator(2, cuda)                             # counts only: such pixels are simply not counted
    ev2.update(nchw_view(lg, cuda), y.to(cuda))
    assert ev2.compute()["confusion_matrix"].sum() == 2 * 64 - (label not in (0, 1))


def test_device_segmentation_metrics_equals_host(cuda):
    y = noisy_labels(2, 40, 50, 3, seed=11).reshape(-1)
    p = torch.randint(-1, 4, y.shape, generator=torch.Generator().manual_seed(12))
    dv = mgunet.segmentation_metrics(y.to(cuda), p.to(cuda), 3)
    hs = mgunet.segmentation_metrics(y, p, 3)
    assert np.array_equal(dv["confusion_matrix"], hs["confusion_matrix"])
    for k in ("iou_per_class", "precision_per_class", "recall_per_class", "f1_per_class"):
        assert np.array_equal(np.array(dv[k]), np.array(hs[k]))


def _unet(cfg, seed, dev, dtype=torch.float32):
    m = mgunet.UNet(*cfg, compute_dtype=dtype)
    m.load_state_dict(O.make_unet_params(*cfg, seed=seed))
    return m.to(dev)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_evaluate_segmentation_small_unet(cuda, dtype):
    cfg = (3, 2, 8, 2)
    model = _unet(cfg, 9, cuda, dtype)
    g = torch.Generator().manual_seed(5)
    loader = [(torch.randn((b, 3, 32, 48), generator=g), torch.randint(0, 2, (b, 32, 48), generator=g)) for b in (2, 1, 3)]
    model.train()
    if dtype == torch.bfloat16:
        model.eval()                                                       # bf16 storage is inference only
    was = model.training
    res = mgunet.evaluate_segmentation(model, loader)
    assert model.training == was
    preds, trues = [], []
    model.eval()
    with torch.no_grad():
        for x, y in loader:
            lg = model(x.to(cuda))[0]
            preds.append(torch.argmax(lg.cpu(), 1).reshape(-1))
            trues.append(y.reshape(-1))
    ref = mgunet.segmentation_metrics(torch.cat(trues), torch.cat(preds), 2)
    assert np.array_equal(res["confusion_matrix"], ref["confusion_matrix"])
    for k in ("iou_per_class", "precision_per_class", "recall_per_class", "f1_per_class"):
        assert np.array_equal(np.array(res[k]), np.array(ref[k]))
    withloss = mgunet.evaluate_segmentation(model, loader, loss="ce+dice")
    assert np.array_equal(withloss["confusion_matrix"], ref["confusion_matrix"]) and np.isfinite(withloss["loss"])


def test_evaluation_between_train_steps_changes_nothing(cuda):
    cfg = (3, 2, 8, 2)
    g = torch.Generator().manual_seed(17)
    x = torch.randn((2, 3, 32, 32), generator=g).to(cuda)
    y = torch.randint(0, 2, (2, 32, 32), generator=g).to(cuda)
    loader = [(torch.randn((2, 3, 32, 32), generator=g), torch.randint(0, 2, (2, 32, 32), generator=g))]
    runs = []
    for evaluate in (False, True):
        model = _unet(cfg, 21, cuda)
        tr = mgunet.Trainer(model, lr=1e-3, weight_decay=1e-4)
        tr.train_step(x, y)
        if evaluate:
            mgunet.evaluate_segmentation(model, loader, loss="ce")
            assert model.training
        tr.train_step(x, y)
        torch.cuda.synchronize()
        runs.append((tr.flat.cpu().numpy().copy(), {k: v.cpu().clone() for k, v in model.state_dict().items()}))
    assert np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32))
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
