"""Connected components and per-object statistics on the MI355X (csrc/objects.hip, mgunet.connected_components).  Expected values
come from the scipy fixture (tools/make_yield_golden.py) and from the numpy oracle in objects_oracle.py -- never from scipy itself."""
import numpy as np
import pytest
import torch

import mgunet
import objects_oracle as OO
from mgunet import objects as mobj

pytestmark = pytest.mark.gpu


def check_table(t, maps, connectivity, values=None, min_area=0, num_classes=None):
    """labels, counts, offsets and every statistic of table t equal the oracle, image by image."""
    labels = t.labels.cpu().numpy()
    counts, offsets = t.counts.cpu().numpy(), t.offsets.cpu().numpy()
    cls, area, bbox, sums = t.class_id.cpu().numpy(), t.area.cpu().numpy(), t.bbox.cpu().numpy(), t.sums.cpu().numpy()
    assert offsets[0] == 0 and np.array_equal(np.diff(offsets), counts)
    for b, m in enumerate(maps):
        ref = OO.label(m, connectivity, num_classes=num_classes, min_area=min_area)
        assert np.array_equal(labels[b], ref), b
        assert counts[b] == ref.max(initial=0)
        rc, ra, rb, rs = OO.stats(ref, m if values is None else values[b])
        s = slice(offsets[b], offsets[b + 1])
        assert np.array_equal(cls[s], rc) and np.array_equal(area[s], ra), b
        assert np.array_equal(bbox[s], rb) and np.array_equal(sums[s], rs), b


@pytest.mark.parametrize("connectivity", [1, 2])
def test_scipy_golden(cuda, golden, connectivity):
    g = golden["objects"]
    for j in range(int(g["nlab"])):
        m = g[f"lab_{j}_mask"]
        t = mgunet.connected_components(torch.from_numpy(m).to(cuda), connectivity=connectivity)
        assert np.array_equal(t.labels[0].cpu().numpy(), g[f"lab_{j}_c{connectivity}"]), j


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 700), (1, 700, 1), (1, 129, 131), (1, 511, 513), (8, 512, 512), (2, 1024, 1024)])
@pytest.mark.parametrize("density", [0.3, 0.5, 0.6])
def test_random_masks_against_oracle(cuda, shape, density):
    rng = np.random.default_rng(int(density * 10) + shape[1] + 7 * shape[2])
    maps = (rng.random(shape) < density).astype(np.int64)
    for connectivity in (1, 2):
        t = mgunet.connected_components(torch.from_numpy(maps).to(cuda), connectivity=connectivity)
        check_table(t, maps, connectivity)


def test_uniform_maps_and_checkerboards(cuda):
    H, W = 200, 333
    ones, zeros = np.ones((2, H, W), np.int64), np.zeros((1, H, W), np.int64)
    t = mgunet.connected_components(torch.from_numpy(ones).to(cuda))
    assert t.counts.tolist() == [1, 1]                                      # no join across the images of a batch
    check_table(t, ones, 2)
    assert t.area.tolist() == [H * W, H * W] and t.bbox.tolist() == [[0, 0, W, H]] * 2
    t = mgunet.connected_components(torch.from_numpy(zeros).to(cuda))
    assert t.counts.tolist() == [0] and not t.labels.any() and t.area.numel() == 0
    cb = ((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2).astype(np.int64)[None]
    t4 = mgunet.connected_components(torch.from_numpy(cb).to(cuda), connectivity=1)
    assert t4.counts.tolist() == [int(cb.sum())]                            # every foreground pixel its own object
    check_table(t4, cb, 1)
    t8 = mgunet.connected_components(torch.from_numpy(cb).to(cuda), connectivity=2)
    assert t8.counts.tolist() == [1]
    two = (cb[0] + 1)[None]                                                 # two classes in a checkerboard
    t = mgunet.connected_components(torch.from_numpy(two).to(cuda), connectivity=1)
    assert t.counts.tolist() == [H * W]                                     # 4-neighbours: every pixel its own object
    check_table(t, two, 1)
    t = mgunet.connected_components(torch.from_numpy(two).to(cuda), connectivity=2)
    assert t.counts.tolist() == [2]                                         # 8-neighbours: one object per class
    check_table(t, two, 2)


def test_no_join_across_images(cuda):
    rng = np.random.default_rng(3)
    maps = (rng.random((5, 64, 96)) < 0.6).astype(np.int64)
    maps[:, -1, :] = 1                                                      # last row of image b touches the first row of b + 1
    maps[:, 0, :] = 1
    t = mgunet.connected_components(torch.from_numpy(maps).to(cuda))
    check_table(t, maps, 2)
    t2 = mgunet.connected_components(torch.from_numpy(maps[2]).to(cuda))   # an (H, W) map
    assert torch.equal(t2.labels[0], t.labels[2])


def test_multiclass_and_background_value(cuda):
    rng = np.random.default_rng(5)
    maps = rng.integers(0, 4, (3, 97, 131)).repeat(1, 0)
    maps[0, :40, :50] = 2
    t = mgunet.connected_components(torch.from_numpy(maps).to(cuda))
    check_table(t, maps, 2)
    t = mgunet.connected_components(torch.from_numpy(maps).to(cuda), background=2, connectivity=1)
    for b in range(3):
        assert np.array_equal(t.labels[b].cpu().numpy(), OO.label(maps[b], 1, background=2))


def tie_logits(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1, 2, (B, H, W, C), generator=g).float()          # many exact ties between classes


@pytest.mark.parametrize("C", [2, 3, 5])
def test_fused_logits_equal_class_map(cuda, C):
    B, H, W = 3, 131, 150
    lg = tie_logits(B, C, H, W, seed=C)
    dev = lg.to(cuda)
    nchw = dev.permute(0, 3, 1, 2)                                          # the view UNet.forward returns
    cmap = mgunet.argmax_classes(nchw)
    assert torch.equal(cmap.cpu(), torch.argmax(lg.permute(0, 3, 1, 2), 1))
    for connectivity in (1, 2):
        a = mgunet.connected_components(nchw, connectivity=connectivity)
        b = mgunet.connected_components(cmap, connectivity=connectivity)
        for f in ("labels", "counts", "offsets", "class_id", "area", "bbox", "sums"):
            assert torch.equal(getattr(a, f), getattr(b, f)), f
        check_table(a, cmap.cpu().numpy(), connectivity)


def test_ignore_and_out_of_range_labels_are_background(cuda):
    rng = np.random.default_rng(9)
    B, H, W, C = 2, 150, 170, 3
    m = rng.integers(0, C, (B, H, W))
    r = rng.random((B, H, W))
    m[r < 0.15] = -100
    m[(r >= 0.15) & (r < 0.2)] = C + 4
    m[(r >= 0.2) & (r < 0.22)] = -3
    md = torch.from_numpy(m).to(cuda)
    labels = torch.empty((B, H, W), device=cuda, dtype=torch.int32)
    counts = torch.empty(B, device=cuda, dtype=torch.int64)
    offsets = torch.empty(B + 1, device=cuda, dtype=torch.int64)
    mobj._label(md, 0, B, H, W, 0, 2, 0, C, 0, labels, counts, offsets)    # the evaluator's GT path: class range [0, C)
    clean = np.where((m >= 0) & (m < C), m, 0)
    for b in range(B):
        assert np.array_equal(labels[b].cpu().numpy(), OO.label(clean[b], 2))
        assert np.array_equal(labels[b].cpu().numpy(), OO.label(m[b], 2, num_classes=C))
    t = mgunet.connected_components(md)                                     # no range: every value but 0 is foreground
    check_table(t, m, 2)


@pytest.mark.parametrize("min_area", [1, 2, 5, 40])
def test_min_area_renumbering(cuda, min_area):
    rng = np.random.default_rng(min_area)
    maps = (rng.random((3, 140, 190)) < 0.45).astype(np.int64) * rng.integers(1, 3, (3, 140, 190))
    for connectivity in (1, 2):
        t = mgunet.connected_components(torch.from_numpy(maps).to(cuda), connectivity=connectivity, min_area=min_area)
        check_table(t, maps, connectivity, min_area=min_area)
        assert (t.area >= min_area).all()


def test_two_runs_identical_bytes(cuda):
    rng = np.random.default_rng(21)
    maps = torch.from_numpy((rng.random((4, 512, 512)) < 0.6).astype(np.int64)).to(cuda)
    runs = [mgunet.connected_components(maps) for _ in range(2)]
    for f in ("labels", "counts", "offsets", "class_id", "area", "bbox", "sums"):
        assert torch.equal(getattr(runs[0], f), getattr(runs[1], f)), f


def test_bad_arguments(cuda):
    x = torch.zeros((2, 8, 8), dtype=torch.int64, device=cuda)
    with pytest.raises(ValueError):
        mgunet.connected_components(x, connectivity=3)
    with pytest.raises(TypeError):
        mgunet.connected_components(torch.zeros((2, 3, 8, 8), dtype=torch.int64, device=cuda))
    with pytest.raises(RuntimeError):
        mgunet.connected_components(x.cpu())
