"""Graph-branch inputs on the device (mgunet.patch_node_features / patch_labels / E2ETrainer.step_images).  The byte columns of the node
features against the per-image composition they replace (EdgeDetector / HistogramEqualizer -> patch_features_u8), bit for bit; the
pixel-mean block against the float64 mean, to one final rounding; the copied and zero columns bit for bit; the label vote against
the numpy oracle of tests/patch_inputs_oracle.py, exactly; step_images against step on the explicitly computed tensors, bit for bit.
Shapes are the smallest that reach every path: padded patches on both sides, a single patch (every halo pixel reflected), more pixels
than threads (p = 32), patches narrower than a wave (p = 8, p = 4: the one-wave-per-patch kernels), a one-pixel-wide patch row."""
import functools

import numpy as np
import pytest
import torch

import mgunet
import mgunet_oracle as O
import patch_inputs_oracle as PO
from mgunet import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def special_pair(H=24, W=40):
    """image 0: black except a bright top row and right column (its only edges lie on the image border); image 1: left half 255,
    right half 0"""
    a = np.zeros((2, H, W, 3), np.uint8)
    a[0, 0, :, :] = 255
    a[0, :, W - 1, :] = (250, 40, 130)
    a[1, :, :W // 2, :] = 255
    return a


@functools.lru_cache(maxsize=None)
def u8_case(name):
    """-> (B, H, W, 3) uint8 batch on the device, patch size"""
    B, H, W, p = {"ragged": (3, 40, 56, 16), "single": (2, 16, 16, 16), "p32": (2, 33, 65, 32), "p8": (2, 24, 24, 8), "p4": (1, 9, 7, 4),
                  "const1": (3, 32, 32, 16), "special": (2, 24, 40, 16)}[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    a = rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    if name == "ragged":
        a[1] = (a[1] // 3 + 60).astype(np.uint8)     # a narrow luminance range: a steep equalisation table, unlike its neighbours'
    if name == "const1":
        a[1] = 77                                    # grey: survives the YUV round trip exactly
    if name == "special":
        a = special_pair(H, W)
    return torch.from_numpy(a).to(DEV), p


@functools.lru_cache(maxsize=None)
def composed(name, per_channel):
    """the composition the fused call replaces, image by image: (B*Np, 1 + (3 | 1))"""
    batch, p = u8_case(name)
    rows = []
    for img in batch:
        sob = mgunet.patch_features_u8(mgunet.EdgeDetector().sobel_edges(img), p)
        eq = mgunet.patch_features_u8(mgunet.HistogramEqualizer().equalize_histogram_rgb(img), p, per_channel)
        rows.append(torch.cat([sob, eq], 1))
    return torch.cat(rows, 0)


@pytest.mark.parametrize("per_channel", [True, False])
@pytest.mark.parametrize("name", ["ragged", "single", "p32", "p8", "p4", "const1", "special"])
def test_byte_columns_equal_the_per_image_composition(cuda, name, per_channel):
    batch, p = u8_case(name)
    ref = composed(name, per_channel)
    got = mgunet.patch_node_features(batch, p, per_channel=per_channel, pad_to=1)
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert torch.equal(got, ref), (name, int((got != ref).sum()))
    assert torch.equal(mgunet.patch_node_features(batch, p, per_channel=per_channel, pad_to=1), got)       # deterministic
    if name == "const1":   # image 1 is constant: no gradient, and its table maps it to itself; its neighbours' statistics stay theirs
        Np = ref.shape[0] // 3
        mid = got[Np:2 * Np]
        assert torch.equal(mid[:, 0], torch.zeros(Np, device=cuda))
        assert torch.equal(mid[:, 1:], mgunet.patch_features_u8(batch[1], p, per_channel))
        assert float(got[:Np, 0].min()) > 0 and float(got[2 * Np:, 0].min()) > 0
    if name == "special":
        assert float(got[:, 0].max()) > 0


def test_numpy_input_and_single_image(cuda):
    batch, p = u8_case("ragged")
    got = mgunet.patch_node_features(batch[0].cpu().numpy(), p, pad_to=1)
    assert got.is_cuda and torch.equal(got, composed("ragged", True)[:got.shape[0]])


def float_batch(B, H, W, seed):
    return torch.from_numpy(O.formula_normal("patch_inputs/x", (B, 3, H, W), seed=seed))


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("name", ["ragged", "p4", "p32"])
def test_pixel_mean_block_is_the_float64_mean_rounded_once(cuda, name, layout):
    batch, p = u8_case(name)
    B, H, W, _ = batch.shape
    x = float_batch(B, H, W, 7)
    xd = x.to(cuda) if layout == "nchw" else x.to(cuda).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert xd.shape == x.shape and xd.is_contiguous() == (layout == "nchw")
    got = mgunet.patch_node_features(batch, p, images=xd, repeat=16)
    assert got.shape[1] == 20
    m = np.concatenate([PO.patch_pixel_mean(x[b].numpy(), p) for b in range(B)])
    g = got[:, :16].cpu().numpy()
    assert np.array_equal(g, np.repeat(g[:, :1], 16, axis=1))                                   # all R copies bitwise equal
    err = np.abs(g[:, 0].astype(np.float64) - m)
    print("pixel mean: max err / bound", float((err / (2.0 ** -24 * np.abs(m) + 2.0 ** -149)).max()))
    assert np.all(err <= 2.0 ** -24 * np.abs(m) + 2.0 ** -149)
    assert torch.equal(got[:, 16:], composed(name, True))
    # R = 0: the block is skipped, the rest is unchanged
    got0 = mgunet.patch_node_features(batch, p, images=xd, repeat=0)
    assert got0.shape[1] == 4 and torch.equal(got0, composed(name, True))


@pytest.mark.parametrize("cu,pad_to,width", [(32, 4, 52), (5, 4, 28), (5, 8, 32)])
def test_copied_block_and_zero_padding(cuda, cu, pad_to, width):
    batch, p = u8_case("ragged")
    B, H, W, _ = batch.shape
    x = float_batch(B, H, W, 9).to(cuda)
    rows = composed("ragged", True).shape[0]
    feats = torch.from_numpy(O.formula_normal("patch_inputs/unet", (rows, cu), seed=10)).to(cuda)
    out = torch.full((rows, width), float("nan"), device=cuda)
    got = mgunet.patch_node_features(batch, p, images=x, unet_patch_feats=feats, pad_to=pad_to, out=out)
    assert got is out and got.shape[1] == width and width % pad_to == 0
    assert torch.equal(got[:, 16:16 + cu], feats)
    assert torch.equal(got[:, 16 + cu:16 + cu + 4], composed("ragged", True))
    assert torch.equal(got[:, 16 + cu + 4:], torch.zeros((rows, width - 20 - cu), device=cuda))
    assert torch.equal(got[:, :16], mgunet.patch_node_features(batch, p, images=x)[:, :16])
    # without the float batch the copied block comes first
    g2 = mgunet.patch_node_features(batch, p, unet_patch_feats=feats, pad_to=1)
    assert g2.shape[1] == cu + 4 and torch.equal(g2[:, :cu], feats) and torch.equal(g2[:, cu:], composed("ragged", True))


def test_node_feature_refusals(cuda):
    batch, p = u8_case("p4")
    with pytest.raises(ValueError):
        mgunet.patch_node_features(batch, 65)
    with pytest.raises(ValueError):
        mgunet.patch_node_features(batch, 0)
    with pytest.raises(ValueError):
        mgunet.patch_node_features(batch, p, images=torch.zeros((1, 3, 8, 8), device=cuda))
    with pytest.raises(ValueError):   # ld_out below the used columns
        _lib.call("mgu_patch_node_features_u8", cuda, batch, 1, 9, 7, 4, None, 0, 0, 0, 0, 0, None, 0, 1, torch.zeros(6, 4, device=cuda), 3)


# ---- patch labels ---------------------------------------------------------------------------------------------------------------------------
def check_vote(maps, p, C):
    """labels, counts and purity of every patch of every image against the numpy oracle, exactly"""
    lab, cnt, pur = mgunet.patch_labels(maps, p, C, return_counts=True, return_purity=True)
    B = maps.shape[0]
    assert lab.dtype == torch.int64 and cnt.dtype == torch.int32 and pur.dtype == torch.float32
    host = maps.cpu().numpy()
    for b in range(B):
        rl, rc, rp = PO.patch_label_vote(host[b], p, C)
        assert np.array_equal(lab[b].cpu().numpy(), rl), b
        assert np.array_equal(cnt[b].cpu().numpy(), rc), b
        assert np.array_equal(pur[b].cpu().numpy(), rp), b
    assert torch.equal(mgunet.patch_labels(maps, p, C), lab)                       # labels alone: no tuple, no optional outputs
    return lab, cnt, pur


@pytest.mark.parametrize("shape", [(40, 56, 16), (9, 7, 4), (33, 65, 32)])
@pytest.mark.parametrize("C", [2, 3, 5])
def test_label_vote_equals_the_oracle(cuda, C, shape):
    H, W, p = shape
    rng = np.random.RandomState(100 * C + H)
    m = rng.randint(0, C, (2, H, W))
    m[1, :H // 2] = np.minimum(m[1, :H // 2], 1)                                    # skewed counts in half of image 1
    check_vote(torch.from_numpy(m).to(cuda), p, C)


def test_constructed_ties_resolve_to_the_lowest_class(cuda):
    m = np.zeros((1, 6, 12), np.int64)
    m[0, :, :6] = np.array([2, 3] * 18).reshape(6, 6)                               # 18 / 18 between classes 2 and 3
    m[0, :, 6:] = np.array([3, 1, 2] * 12).reshape(6, 6)                            # 12 / 12 / 12 between 1, 2 and 3
    lab, cnt, pur = check_vote(torch.from_numpy(m).to(cuda), 6, 4)
    assert lab.tolist() == [[2, 1]] and cnt.tolist() == [[[0, 0, 18, 18], [0, 12, 12, 12]]]
    assert pur.tolist() == [[0.5, float(np.float32(np.float64(12) / np.float64(36)))]]
    lab4, _, _ = check_vote(torch.from_numpy(np.tile(np.array([[1, 0], [0, 1]]), (8, 8))[None]).to(cuda), 16, 2)   # the 4-wave kernel
    assert lab4.tolist() == [[0]]


def test_out_of_range_values_are_counted_nowhere(cuda):
    rng = np.random.RandomState(5)
    m = rng.randint(0, 3, (2, 40, 56))
    m[0][rng.rand(40, 56) < 0.3] = -100
    m[1][rng.rand(40, 56) < 0.3] = 3
    m[1, 16:32, 32:48] = -100                                                        # patch (1, 2) of image 1: nothing to count
    m[0, 32:, 48:] = 7                                                               # the padded corner patch of image 0 too
    lab, cnt, pur = check_vote(torch.from_numpy(m).to(cuda), 16, 3)
    assert int(lab[1, 4 + 2]) == 0 and float(pur[1, 4 + 2]) == 0.0 and int(cnt[1, 4 + 2].sum()) == 0
    assert int(lab[0, 11]) == 0 and float(pur[0, 11]) == 0.0
    small = np.full((1, 9, 7), -1, np.int64)                                         # the one-wave kernel: every patch empty but one
    small[0, 4:8, 4:7] = 1
    lab, cnt, pur = check_vote(torch.from_numpy(small).to(cuda), 4, 2)
    assert lab.tolist() == [[0, 0, 0, 1, 0, 0]] and pur.tolist() == [[0, 0, 0, 1.0, 0, 0]]
    assert torch.equal(mgunet.patch_labels(torch.from_numpy(small[0]).to(cuda), 4, 2), lab)   # (H, W) is one image


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("C,shape", [(1, (9, 7, 4)), (3, (40, 56, 16)), (5, (33, 65, 32)), (2, (9, 7, 4))])
def test_logits_vote_equals_the_vote_over_argmax_classes(cuda, C, shape, layout):
    H, W, p = shape
    rng = np.random.RandomState(C + H)
    lg = rng.randn(2, C, H, W).astype(np.float32)
    lg[1] = rng.randint(0, 3, (C, H, W)).astype(np.float32)                          # exact per-pixel ties between channels
    t = torch.from_numpy(lg).to(cuda)
    if layout == "nhwc":                                                             # the view the U-Net returns
        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    cls = mgunet.argmax_classes(t)
    if C > 1:
        assert int((cls[1] == 0).sum()) > 0 and int((cls[1] > 0).sum()) > 0
    got = mgunet.patch_labels(t, p, return_counts=True, return_purity=True)
    ref = mgunet.patch_labels(cls, p, C, return_counts=True, return_purity=True)
    for g, r in zip(got, ref):
        assert g.shape == r.shape and torch.equal(g, r)
    assert got[1].shape == (2, PO.patch_grid(H, W, p)[0] * PO.patch_grid(H, W, p)[1], C)
    check_vote(cls, p, C)


def test_label_refusals(cuda):
    m = torch.zeros((1, 8, 8), dtype=torch.int64, device=cuda)
    assert mgunet.patch_labels(m, 4, 32).shape == (1, 4)
    with pytest.raises(ValueError):
        mgunet.patch_labels(m, 4, 33)
    lab = torch.zeros(4, dtype=torch.int64, device=cuda)
    with pytest.raises(ValueError):   # the library's own invalid-argument status
        _lib.call("mgu_patch_labels", cuda, m, 0, 1, 8, 8, 33, 4, None, lab, None)
    with pytest.raises(ValueError):
        _lib.call("mgu_patch_labels", cuda, m, 2, 1, 8, 8, 2, 4, None, lab, None)
    assert int(mgunet.patch_labels(m + 4, 4).max()) == 4                              # num_classes = None: max + 1


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def e2e_trainer(cuda, din, dp=32, K=2):
    unet = mgunet.UNet(3, 2, 8, 2)
    unet.load_state_dict(O.make_unet_params(3, 2, 8, 2, seed=9))
    gat = mgunet.GATNetwork(din, 16, dp, 2, num_gat_layers=1, dropout_rate=0.0)
    gat.load_state_dict(O.make_gat_params(din, 16, dp, 2, 1, seed=61))
    gat = gat.to(cuda).train()
    pred = mgunet.PatchSegmentPredictor(dp, K, hidden_dim=16, use_gnn=True, num_gnn_layers=1, num_heads=2)
    pred.load_state_dict(O.make_segment_predictor_params(dp, K, 16, True, 2, seed=62), strict=True)
    pred = pred.to(cuda).eval()   # eval: the GNN predictor's dropout is torch-RNG noise in train mode
    tr = mgunet.E2ETrainer(mgunet.Trainer(unet.to(cuda), lr=1e-3, weight_decay=1e-4), gat, pred, mgunet.MinCutRefinement(),
                           mgunet.FeatureConsistencyLoss(margin=1.0), num_segments=K)
    return tr, gat, pred


def test_step_images_is_step_on_the_derived_inputs(cuda):
    B, H, p, dp = 2, 32, 16, 32
    rng = np.random.RandomState(3)
    u8 = torch.from_numpy(rng.randint(0, 256, (B, H, H, 3)).astype(np.uint8)).to(cuda)
    mean, std = torch.tensor([0.485, 0.456, 0.406], device=cuda), torch.tensor([0.229, 0.224, 0.225], device=cuda)
    images = ((u8.float() / 255 - mean) / std).permute(0, 3, 1, 2).contiguous()
    masks = torch.from_numpy(rng.randint(0, 2, (B, H, H)).astype(np.int64)).to(cuda)
    funet = (torch.from_numpy(O.formula_normal("patch_inputs/funet", (B, 4, dp), seed=73)) * 0.4).to(cuda)
    a, gat_a, pred_a = e2e_trainer(cuda, 20)
    b, gat_b, pred_b = e2e_trainer(cuda, 20)
    out_a = a.step_images(images, masks, u8, funet)
    X = mgunet.patch_node_features(u8, p, images=images)
    Y = mgunet.patch_labels(masks, p)
    assert X.shape == (B * 4, 20) and Y.shape == (B, 4)
    ei = mgunet.PatchGraphConstructor(p).edge_index(H, H, cuda)
    out_b = b.step(images, masks, X.view(B, 4, 20), funet, Y, ei)
    assert set(out_a) == set(out_b) == {"total", "l_unet_seg", "l_shape", "l_feature", "l_partition", "l_smooth"}
    for k in out_a:
        assert bool(torch.isfinite(out_a[k])) and torch.equal(out_a[k], out_b[k]), (k, float(out_a[k]), float(out_b[k]))
    assert torch.equal(a.unet.flat, b.unet.flat)
    for ma, mb in ((gat_a, gat_b), (pred_a, pred_b)):
        for (k, v), (_, w) in zip(ma.state_dict().items(), mb.state_dict().items()):
            assert torch.equal(v, w), k
    out_e = a.step_images(images, masks, u8, funet, edge_index=ei, patch_size=p)                 # an explicit graph, a second step
    assert bool(torch.isfinite(out_e["total"])) and float(out_e["total"]) != float(out_a["total"])


def test_step_images_names_both_widths_on_a_mismatch(cuda):
    tr, _, _ = e2e_trainer(cuda, 32)
    z = torch.zeros((2, 3, 32, 32), device=cuda)
    with pytest.raises(ValueError, match=r"32.*20"):
        tr.step_images(z, torch.zeros((2, 32, 32), dtype=torch.int64, device=cuda), torch.zeros((2, 32, 32, 3), dtype=torch.uint8, device=cuda),
                       torch.zeros((2, 4, 32), device=cuda))
