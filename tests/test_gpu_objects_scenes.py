"""The designed labelling scenes of tests/objects_cases.py on the MI355X (csrc/objects.hip): serpentines, combs, spirals, rings,
diagonals through and beside tile corners, corner and edge contacts between tiles, each alone, all as one batch and through the
fused-logits source; min_area at exact areas; batches of up to 65535 images through the chunk scan and the offsets loop; the int32
4-neighbour instantiation through mgunet.connect_regions; the capacity cut of mgu_object_stats and mgu_object_scores; and the
refusals of mgu_connected_components at the C-ABI.  Expected values come from objects_oracle (superpixels_oracle for the regions);
every comparison is exact.  tests/test_objects_cases_host.py shows on the host what each scene is there to catch."""
import numpy as np
import pytest
import torch

import mgunet
import objects_cases as OC
import objects_oracle as OO
import superpixels_oracle as SPO
from mgunet import _lib
from mgunet import objects as mobj
from test_gpu_yield import onehot_logits

pytestmark = pytest.mark.gpu

FIELDS = ("labels", "counts", "offsets", "class_id", "area", "bbox", "sums")
SENTINEL = -7


def components(cuda, maps, connectivity, min_area=0):
    return mgunet.connected_components(torch.from_numpy(np.array(maps)).to(cuda), connectivity=connectivity, min_area=min_area)


def check_table(t, labels, counts, offsets, cls, area, bbox, sums):
    """every field of table t equals the oracle's, bit for bit"""
    assert t.labels.dtype == torch.int32 and np.array_equal(t.labels.cpu().numpy(), labels)
    assert np.array_equal(t.counts.cpu().numpy(), counts) and np.array_equal(t.offsets.cpu().numpy(), offsets)
    assert int(t.offsets[-1]) == len(cls) == t.class_id.numel()             # offsets[B] is the number of objects
    for got, want, f in ((t.class_id, cls, "class"), (t.area, area, "area"), (t.bbox, bbox, "bbox"), (t.sums, sums, "sums")):
        assert np.array_equal(got.cpu().numpy(), want), f


def check_scene(t, name, size, connectivity, min_area=0):
    lab, stats = OC.expected(name, size, connectivity, min_area)
    n = int(lab.max(initial=0))
    check_table(t, lab[None], np.array([n]), np.array([0, n]), *stats)


# ---- the scenes, alone, as one batch and as logits --------------------------------------------------------------------------------
@pytest.mark.parametrize("size", OC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", OC.SCENE_NAMES)
def test_scene(cuda, name, size):
    for connectivity in (1, 2):
        check_scene(components(cuda, OC.scene(name, size), connectivity), name, size, connectivity)


@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("size", OC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_all_scenes_as_one_batch(cuda, size, connectivity):
    maps = OC.scene_batch(size)
    t = components(cuda, maps, connectivity)
    labels = np.stack([OC.expected(n, size, connectivity)[0] for n in OC.SCENE_NAMES])
    check_table(t, labels, *OC.table_of(labels, maps))
    off = t.offsets.tolist()
    for b, name in enumerate(OC.SCENE_NAMES):   # image b of the batch is the single-image call
        one = components(cuda, maps[b], connectivity)
        assert torch.equal(one.labels[0], t.labels[b]) and one.counts.tolist() == [off[b + 1] - off[b]], name
        for f in FIELDS[3:]:
            assert torch.equal(getattr(one, f), getattr(t, f)[off[b]:off[b + 1]]), (name, f)


@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("size", OC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fused_logits_equal_the_class_map(cuda, size, connectivity):
    maps = torch.from_numpy(np.array(OC.scene_batch(size)))
    a = mgunet.connected_components(onehot_logits(maps, 3, cuda, seed=size[0]), connectivity=connectivity)
    b = mgunet.connected_components(maps.to(cuda), connectivity=connectivity)
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert int(a.offsets[-1]) > len(OC.SCENE_NAMES)


# ---- min_area at exact areas ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_area", OC.MIN_AREAS)
def test_min_area_at_exact_areas(cuda, min_area):
    m = OC.area_map()
    for connectivity in (1, 2):
        t = components(cuda, m, connectivity, min_area)
        lab = OO.label(m, connectivity, min_area=min_area)
        n = max(0, 71 - min_area)
        assert t.counts.tolist() == [n]
        check_table(t, lab[None], np.array([n]), np.array([0, n]), *OO.stats(lab, m))
        assert sorted(t.area.tolist()) == list(range(max(1, min_area), 71))


@pytest.mark.parametrize("size", OC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_min_area_equal_to_a_serpentines_area(cuda, size):
    """one object across many waves and workgroups: kept at min_area = its area, dropped one above"""
    for name in ("row_serpentine", "col_serpentine"):
        m = OC.scene(name, size)
        A = int(m.sum())
        for connectivity in (1, 2):
            t = components(cuda, m, connectivity, A)
            assert t.counts.tolist() == [1] and t.area.tolist() == [A]
            check_scene(t, name, size, connectivity, A)
            t = components(cuda, m, connectivity, A + 1)
            assert t.counts.tolist() == [0] and t.offsets.tolist() == [0, 0] and not t.labels.any() and t.area.numel() == 0


# ---- large batches ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", OC.LARGE_BATCHES, ids=lambda s: "x".join(map(str, s)))
def test_large_batches(cuda, shape):
    maps = OC.random_batch(*shape)
    for connectivity in (1, 2):
        t = components(cuda, maps, connectivity)
        check_table(t, *OC.stacked_table(maps, connectivity))
        assert int(t.offsets[shape[0]]) == int(t.counts.sum()) == t.area.numel() > shape[0]


def test_65535_single_pixel_images(cuda):
    maps, labels, counts, offsets = OC.single_pixel_batch()
    B = len(maps)
    fg = np.flatnonzero(counts)
    zeros, ones = np.zeros(len(fg), np.int64), np.ones(len(fg), np.int64)
    for connectivity in (1, 2):
        t = components(cuda, maps, connectivity)
        check_table(t, labels, counts, offsets, ones, ones, np.stack([zeros, zeros, ones, ones], 1), np.stack([zeros, zeros], 1))
        assert int(t.offsets[B]) == 32768


# ---- the int32, 4-neighbour instantiation -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", OC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_connect_regions_on_the_scenes(cuda, size):
    """the scenes as raw label maps (0 is a label like any other); min_area 1 leaves no region small, so both rounds merge nothing"""
    raw = np.stack([OC.scene(n, size) for n in OC.REGION_SCENES]).astype(np.int32)
    labels, counts, offsets = mgunet.connect_regions(torch.from_numpy(raw).to(cuda), 1, 2)
    rl, rc, ro = SPO.connect(raw, 1, 2)
    assert labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), rl)
    assert np.array_equal(counts.cpu().numpy(), rc) and np.array_equal(offsets.cpu().numpy(), ro)
    for b, name in enumerate(OC.REGION_SCENES):   # the regions are the 4-connected components of the scene and of its background
        fgn = int(OC.expected(name, size, 1)[0].max(initial=0))
        bgn = int(OO.label(raw[b] == 0, 1).max(initial=0))
        assert rc[b] == fgn + bgn, name


# ---- capacity of the per-object arrays --------------------------------------------------------------------------------------------
CAP_SIZE = (70, 45)
CAP_SCENES = ("corner_nwse", "edge_h", "rings_compl")


def capacity_scene():
    """(maps, labels, counts, offsets, class, area, bbox, sums) of three scenes under 4-neighbours, from the oracle"""
    maps = np.stack([OC.scene(n, CAP_SIZE) for n in CAP_SCENES])
    labels = np.stack([OC.expected(n, CAP_SIZE, 1)[0] for n in CAP_SCENES])
    return (maps, labels) + OC.table_of(labels, maps)


def capacities(n):
    return [0, 1, n - 1, n, n + 5]


def test_object_stats_capacity(cuda):
    maps, labels, counts, offsets, cls, area, bbox, sums = capacity_scene()
    B, H, W = maps.shape
    n = len(cls)
    assert n > 8 and offsets[1] > 1 and offsets[2] < n - 1                 # the cut at n - 1 falls inside the last image
    dm, dl, do = (torch.from_numpy(np.array(a)).to(cuda) for a in (maps, labels, offsets))
    for k in capacities(n):
        rows = n + 8
        bufs = [torch.full(s, SENTINEL, device=cuda, dtype=dt) for s, dt in (((rows,), torch.int64), ((rows, 4), torch.int32),
                                                                              ((rows,), torch.int64), ((rows, 2), torch.int64))]
        mobj._stats(dl, dm, 0, B, H, W, 0, do, k, *bufs)
        m = min(k, n)
        for got, want, f in zip(bufs, (cls, bbox, area, sums), ("class", "bbox", "area", "sums")):
            got = got.cpu().numpy()
            assert np.array_equal(got[:m], want[:m]), (k, f)
            assert (got[m:] == SENTINEL).all(), (k, f)


def test_object_scores_capacity(cuda):
    maps, labels, counts, offsets, cls, area, bbox, sums = capacity_scene()
    B, H, W = maps.shape
    n, C = len(cls), 3
    probs = torch.rand((B, H, W, C), generator=torch.Generator().manual_seed(3))     # NHWC, as the entry point reads it
    bs, ys, xs = np.nonzero(labels)
    obj = offsets[bs] + labels[bs, ys, xs] - 1
    acc = np.zeros(n, np.uint64)                                                     # the fixed-point sum, as test_gpu_object_waves restates it
    np.add.at(acc, obj, np.rint(probs.numpy()[bs, ys, xs, cls[obj]].astype(np.float64) * 2.0 ** 32).astype(np.uint64))
    ref = ((acc.astype(np.float64) * 2.0 ** -32) / area.astype(np.float64)).astype(np.float32)
    dl, do, dc, da = (torch.from_numpy(np.array(a)).to(cuda) for a in (labels, offsets, cls, area))
    dp = probs.to(cuda)
    for k in capacities(n):
        scores = torch.full((n + 8,), float(SENTINEL), device=cuda, dtype=torch.float32)
        _lib.call("mgu_object_scores", cuda, dl, dp, B, H, W, C, do, k, dc, da, scores)
        got = scores.cpu().numpy()
        m = min(k, n)
        assert np.array_equal(got[:m].view(np.uint32), ref[:m].view(np.uint32)), k
        assert (got[m:] == float(SENTINEL)).all(), k
    assert (ref > 0).all() and (ref < 1).all()


# ---- refusals at the C-ABI --------------------------------------------------------------------------------------------------------
REFUSALS = {   # name -> (src_kind, B, H, W, C, connectivity, min_area)
    "connectivity_3": (0, 1, 4, 4, 0, 3, 0),
    "src_kind_2": (2, 1, 4, 4, 0, 2, 0),
    "logits_without_classes": (1, 1, 4, 4, 0, 2, 0),
    "negative_min_area": (0, 1, 4, 4, 0, 2, -1),
    "65536_images": (0, 65536, 1, 1, 0, 2, 0),
    "2^31_pixels": (0, 32768, 256, 256, 0, 2, 0),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_connected_components_refuses(cuda, name):
    kind, B, H, W, C, connectivity, min_area = REFUSALS[name]
    src = torch.ones(16, device=cuda, dtype=torch.float32 if kind == 1 else torch.int64)
    labels = torch.full((16,), SENTINEL, device=cuda, dtype=torch.int32)
    counts = torch.full((2,), SENTINEL, device=cuda, dtype=torch.int64)
    offsets = torch.full((3,), SENTINEL, device=cuda, dtype=torch.int64)
    with pytest.raises(ValueError):
        _lib.call("mgu_connected_components", cuda, src, kind, B, H, W, C, connectivity, 0, 0, min_area, labels, counts, offsets)
    torch.cuda.synchronize()
    for buf in (labels, counts, offsets):
        assert (buf == SENTINEL).all()
