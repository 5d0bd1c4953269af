"""The host view table of test-time augmentation (mgunet.tta): the transform lists, the shape groups and the index maps both kernels of
csrc/tta.hip use, checked against torch.flip / torch.rot90 on the CPU."""
import pytest
import torch

import mgunet
from mgunet import tta
from tta_oracle import unview as torch_unview, view as torch_view   # the views as the issue defines them, through torch.flip / torch.rot90

SHAPES = [(8, 8), (6, 10), (10, 6), (7, 13), (1, 5), (1, 1)]


def test_transform_lists():
    assert tta.TRANSFORMS["none"] == ((0, 0),)
    assert tta.TRANSFORMS["hflip"] == ((0, 0), (1, 0))
    assert tta.TRANSFORMS["flips"] == ((0, 0), (1, 0), (2, 0), (3, 0))
    assert tta.TRANSFORMS["d4"] == tuple((f, r) for f in (0, 1) for r in range(4))
    x = torch.arange(12.0).view(1, 1, 3, 4)
    fW, fH = (lambda t: torch.flip(t, (3,))), (lambda t: torch.flip(t, (2,)))
    want = {"hflip": [x, fW(x)], "flips": [x, fW(x), fH(x), fH(fW(x))],
            "d4": [torch.rot90(x, r, (2, 3)) for r in range(4)] + [torch.rot90(fW(x), r, (2, 3)) for r in range(4)]}
    for name, views in want.items():
        got = [torch_view(x, f, r) for f, r in tta.TRANSFORMS[name]]
        assert len(got) == len(views)
        for a, b in zip(got, views):
            assert torch.equal(a, b), name


@pytest.mark.parametrize("name", sorted(tta.TRANSFORMS))
@pytest.mark.parametrize("H,W", SHAPES)
def test_view_table_groups(name, H, W):
    views, groups = tta.view_table(name, H, W)
    assert [(f, r) for _, _, f, r in views] == list(tta.TRANSFORMS[name])
    assert len(views) in (1, 2, 4, 8)
    for g, slot, f, r in views:
        Hv, Wv, gv = groups[g]
        assert gv[slot] == (f, r)
        assert (Hv, Wv) == ((W, H) if r & 1 else (H, W))
    if H == W or name != "d4":
        assert len(groups) == 1 and groups[0][:2] == (H, W)
    else:
        assert [grp[:2] for grp in groups] == [(H, W), (W, H)]
        assert [len(grp[2]) for grp in groups] == [4, 4]
    assert sum(len(grp[2]) for grp in groups) == len(views)


@pytest.mark.parametrize("name", sorted(tta.TRANSFORMS))
@pytest.mark.parametrize("H,W", SHAPES)
def test_forward_then_inverse_is_identity(name, H, W):
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(H * 100 + W))
    for _, _, f, r in tta.view_table(name, H, W)[0]:
        fwd, inv = tta.view_source_index(f, r, H, W), tta.view_inverse_index(f, r, H, W)
        v = x.flatten(-2)[..., fwd.flatten()].view(2, 3, *fwd.shape)
        back = v.flatten(-2)[..., inv.flatten()].view(2, 3, H, W)
        assert torch.equal(back, x), (name, f, r)


@pytest.mark.parametrize("H,W", SHAPES)
def test_index_maps_match_torch(H, W):
    idx = torch.arange(H * W).view(H, W)
    for f in range(4):
        for r in range(4):
            fwd = tta.view_source_index(f, r, H, W)
            assert torch.equal(fwd, torch_view(idx, f, r)), (f, r)
            Hv, Wv = fwd.shape
            vidx = torch.arange(Hv * Wv).view(Hv, Wv)
            assert torch.equal(tta.view_inverse_index(f, r, H, W), torch_unview(vidx, f, r)), (f, r)


def test_unknown_transform_raises():
    with pytest.raises(ValueError):
        tta.view_table("rot90", 4, 4)
    with pytest.raises(ValueError):
        tta.view_table("D4", 4, 4)


def test_public_api():
    assert mgunet.predict_tta is tta.predict_tta and mgunet.object_scores is tta.object_scores
    assert "predict_tta" in mgunet.__all__ and "object_scores" in mgunet.__all__


def test_predict_tta_refusals_before_any_launch():
    m = mgunet.UNet(3, 2, 8, 2).eval()
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="HIP device"):   # CPU input
        mgunet.predict_tta(m, x, "d4")
    with pytest.raises(RuntimeError, match="eval"):
        mgunet.predict_tta(m.train(), x, "d4")
    with pytest.raises(TypeError):
        mgunet.predict_tta(torch.nn.Identity(), x, "d4")


def test_to_dicts_confidence():
    t = mgunet.ObjectTable(labels=torch.zeros(2, 4, 4, dtype=torch.int32), counts=torch.tensor([2, 1]), offsets=torch.tensor([0, 2, 3]),
                           class_id=torch.tensor([1, 1, 2]), area=torch.tensor([3, 1, 2]),
                           bbox=torch.tensor([[0, 0, 1, 1], [2, 2, 3, 3], [0, 1, 2, 2]], dtype=torch.int32), sums=torch.zeros(3, 2))
    plain = t.to_dicts()
    assert plain == [[{"bbox": [0, 0, 1, 1], "class_id": 1}, {"bbox": [2, 2, 3, 3], "class_id": 1}], [{"bbox": [0, 1, 2, 2], "class_id": 2}]]
    scored = t.to_dicts(scores=torch.tensor([0.5, 0.75, 0.25]))
    assert [[d["confidence"] for d in img] for img in scored] == [[0.5, 0.75], [0.25]]
    assert [[{k: v for k, v in d.items() if k != "confidence"} for d in img] for img in scored] == plain
    with pytest.raises(ValueError):
        t.to_dicts(scores=[0.5])
