"""The superpixel-graph stages (csrc/superpixels.hip, mgunet/superpixels.py) on the device against tests/superpixels_oracle.py, which
tests/test_superpixels_host.py pins: every comparison is bitwise.  Shapes are the smallest at which the kernels can still go wrong:
one centre, partial cells, a width that is no multiple of the wave or the 32 x 32 tile, several tiles and images, every distance tie,
drifting centres, negative sums, the widest and the narrowest step."""
import functools

import numpy as np
import pytest
import torch

import mgunet
import superpixels_oracle as SO
from mgunet import _lib
from mgunet import superpixels as SP

pytestmark = pytest.mark.gpu


def t32(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(cuda)


def t64(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(cuda)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(name):
    rng = np.random.default_rng(11)
    if name == "one":
        return rng.integers(0, 256, (1, 1, 1, 3), dtype=np.uint8)
    if name == "partial":
        return rng.integers(0, 256, (1, 7, 5, 3), dtype=np.uint8)
    if name == "two_images":
        a = SO.disc_scene(37, 67, seed=4)
        b = np.clip(rng.normal(128, 40, (37, 67, 3)), 0, 255).astype(np.uint8)
        return np.stack([a, b])
    if name == "uniform":
        return np.full((1, 40, 72, 3), 93, np.uint8)
    if name == "step":
        img = np.empty((1, 24, 40, 3), np.uint8)
        img[:, :, :13], img[:, :, 13:] = (200, 60, 50), (40, 70, 190)
        return img
    if name == "green_blue":
        img = np.empty((1, 20, 36, 3), np.float64)
        img[:, :, :18], img[:, :, 18:] = (20, 230, 30), (25, 20, 235)
        return np.clip(img + rng.integers(-20, 21, img.shape), 0, 255).astype(np.uint8)
    if name == "noise":
        return SO.disc_scene()[None]
    if name == "wide_step":
        return SO.disc_scene(20, 300, seed=8, discs=9)[None]
    if name == "many_centres":
        return SO.disc_scene(130, 70, seed=9, discs=8)[None]
    raise KeyError(name)


SLIC_CASES = [("one", 4, 40, 3), ("partial", 4, 40, 4), ("two_images", 8, 40, 5), ("uniform", 8, 40, 4), ("step", 8, 8, 6),
              ("green_blue", 6, 40, 4), ("noise", 8, 40, 1), ("noise", 8, 40, 2), ("noise", 8, 40, 6), ("wide_step", 128, 40, 3),
              ("many_centres", 4, 20, 4)]


@functools.lru_cache(maxsize=None)
def slic_ref(name, S, mq, T):
    return SO.slic(scene(name), S, mq, T)


@pytest.mark.parametrize("name,S,mq,T", SLIC_CASES)
def test_slic_labels_and_centres_bitwise(cuda, name, S, mq, T):
    img = scene(name)
    want, wcen = slic_ref(name, S, mq, T)
    raw, cen = mgunet.slic_labels(torch.from_numpy(img).to(cuda), step=S, compactness=mq / 4.0, iterations=T, return_centres=True)
    assert raw.dtype == torch.int32 and tuple(raw.shape) == img.shape[:3]
    assert np.array_equal(raw.cpu().numpy(), want)
    assert np.array_equal(cen.cpu().numpy(), wcen)
    if name == "step":                                  # the centres next to the colour step left their starting columns
        assert (wcen[0, :, 0] != np.minimum(np.arange(5) * 8 + 4, 39)[None].repeat(3, 0).ravel()).any()
    if name == "green_blue":
        assert wcen[0, :, 3].min() < 0 and wcen[0, :, 4].min() < 0
    if name == "two_images":                            # nothing leaks between images: each equals its own single-image run
        one = mgunet.slic_labels(img[1], step=S, compactness=mq / 4.0, iterations=T)
        assert np.array_equal(one.cpu().numpy()[0], want[1])


def test_n_segments_picks_the_step(cuda):
    img = scene("noise")
    a = mgunet.slic_labels(img, n_segments=96, iterations=2)          # sqrt(64 * 96 / 96) = 8
    assert np.array_equal(a.cpu().numpy(), slic_ref("noise", 8, 40, 2)[0])


# ---- connect ----------------------------------------------------------------------------------------------------------------------------
def hand_maps():
    enclosed = np.zeros((9, 11), np.int32)
    enclosed[3:6, 4:7] = 5
    tie = np.zeros((6, 9), np.int32)
    tie[:, 5:] = 1
    tie[0, 4:6] = 2
    only_small = np.zeros((8, 40), np.int32)
    only_small[3, 35], only_small[3, 36], only_small[3, 37] = 7, 8, 7          # 8 touches two small 7s above / beside and the large 0
    only_small[2, 36] = 7
    islands = np.zeros((5, 34), np.int32)
    islands[2, 1:4] = [3, 4, 3]
    islands[1, 2] = islands[3, 2] = 3                                           # 4 is enclosed by four single-pixel 3s: no large neighbour
    return {"checkerboard": (np.indices((6, 35)).sum(0) % 2).astype(np.int32), "enclosed": enclosed, "tie": tie, "only_small": only_small,
            "islands": islands}


CONNECT_SCENES = [("two_images", 8, 40, 5), ("noise", 8, 40, 6), ("uniform", 8, 40, 4), ("many_centres", 4, 20, 4)]


@pytest.mark.parametrize("rounds", [0, 1, 2])
@pytest.mark.parametrize("case", CONNECT_SCENES)
def test_connect_regions_on_slic_labels_bitwise(cuda, case, rounds):
    raw = slic_ref(*case)[0]
    min_area = case[1] * case[1] // 4
    want = SO.connect(raw, min_area, rounds)
    got = mgunet.connect_regions(t32(raw, cuda), min_area, rounds)
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)


@pytest.mark.parametrize("name", ["checkerboard", "enclosed", "tie", "only_small", "islands"])
@pytest.mark.parametrize("min_area,rounds", [(0, 2), (3, 1), (3, 2), (12, 2)])
def test_connect_regions_on_hand_made_maps_bitwise(cuda, name, min_area, rounds):
    raw = hand_maps()[name][None]
    want = SO.connect(raw, min_area, rounds)
    got = mgunet.connect_regions(t32(raw, cuda), min_area, rounds)
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)
    if name == "checkerboard":
        assert want[1][0] == raw.size
    if name == "tie" and min_area == 3:
        assert np.array_equal(want[0][0], (raw[0] == 1).astype(np.int32))       # equal borders: the earlier region takes it
    if name == "islands" and (min_area, rounds) == (3, 1):                      # its only neighbours are small: it stays this round
        assert want[1][0] == 2 and (want[0][0] == want[0][0, 2, 2]).sum() == 1
    if name == "islands" and (min_area, rounds) == (3, 2):
        assert want[1][0] == 1


# ---- adjacency --------------------------------------------------------------------------------------------------------------------------
def check_adjacency(cuda, labels, offsets, ncap, ecap=None):
    want = SO.adjacency(labels, offsets, ncap)
    rowptr, col, border, status = mgunet.region_adjacency(t32(labels, cuda), t64(offsets, cuda), ncap, ecap)
    E = int(want[0][-1])
    assert rowptr.dtype == col.dtype == border.dtype == torch.int32
    assert np.array_equal(rowptr.cpu().numpy(), want[0])
    n = min(E, col.numel())
    return want, col.cpu().numpy(), border.cpu().numpy(), int(status.item()), n


@pytest.mark.parametrize("case", CONNECT_SCENES)
def test_region_adjacency_of_connected_regions_bitwise(cuda, case):
    labels, counts, offsets = SO.connect(slic_ref(*case)[0], case[1] * case[1] // 4, 2)
    ncap = int(offsets[-1]) + 3
    want, col, border, status, n = check_adjacency(cuda, labels, offsets, ncap)
    assert status == 0 and n == want[1].size <= 6 * ncap
    assert np.array_equal(col[:n], want[1]) and np.array_equal(border[:n], want[2])


@pytest.mark.parametrize("name", ["checkerboard", "enclosed", "tie", "only_small", "islands"])
def test_region_adjacency_of_hand_made_maps_bitwise(cuda, name):
    labels, counts, offsets = SO.connect(hand_maps()[name][None], 0, 0)
    want, col, border, status, n = check_adjacency(cuda, labels, offsets, int(offsets[-1]))
    assert status == 0 and np.array_equal(col[:n], want[1]) and np.array_equal(border[:n], want[2])


def test_region_adjacency_of_connected_components_minus_one_and_of_one_region(cuda):
    """a mgu_connected_components output minus 1: the background (-1) takes no part; a one-region image has an empty row"""
    cls = np.zeros((2, 12, 40), np.int64)
    cls[0, 2:6, 3:9], cls[0, 2:6, 9:15], cls[0, 7:10, 20:39] = 1, 2, 1
    table = mgunet.connected_components(torch.from_numpy(cls).to(cuda), connectivity=1)
    labels = (table.labels - 1).cpu().numpy()
    offsets = table.offsets.cpu().numpy()
    assert offsets.tolist() == [0, 3, 3]
    want, col, border, status, n = check_adjacency(cuda, labels, offsets, 4)
    assert status == 0 and want[0].tolist() == [0, 1, 2, 2, 2] and col[:n].tolist() == [1, 0] and border[:n].tolist() == [4, 4]
    one = np.zeros((1, 5, 7), np.int32)
    want, col, border, status, n = check_adjacency(cuda, one, np.array([0, 1]), 1, 6)
    assert status == 0 and want[0].tolist() == [0, 0] and n == 0


def test_region_adjacency_overflow_keeps_rowptr_and_writes_nothing_past_a_capacity(cuda):
    labels, counts, offsets = SO.connect(slic_ref("noise", 8, 40, 6)[0], 16, 2)
    ncap = int(offsets[-1])
    want = SO.adjacency(labels, offsets, ncap)
    E = want[1].size
    ecap = E // 2
    # the arrays sit inside larger buffers whose words past the capacity are guards
    colbuf = torch.full((ecap + 64,), -77, device=cuda, dtype=torch.int32)
    borbuf = torch.full((ecap + 64,), -78, device=cuda, dtype=torch.int32)
    rowbuf = torch.full((ncap + 1 + 64,), -79, device=cuda, dtype=torch.int32)
    status = torch.zeros(1, device=cuda, dtype=torch.int32)
    _lib.call("mgu_regions_adjacency", cuda, t32(labels, cuda), t64(offsets, cuda), 1, 64, 96, ncap, ecap, rowbuf, colbuf, borbuf, status)
    assert int(status.item()) == 1
    assert np.array_equal(rowbuf[:ncap + 1].cpu().numpy(), want[0])
    assert np.array_equal(colbuf[:ecap].cpu().numpy(), want[1][:ecap]) and np.array_equal(borbuf[:ecap].cpu().numpy(), want[2][:ecap])
    assert bool((colbuf[ecap:] == -77).all()) and bool((borbuf[ecap:] == -78).all()) and bool((rowbuf[ncap + 1:] == -79).all())
    # node_capacity too small: status 2, the image contributes nothing
    rowptr, col, border, status = mgunet.region_adjacency(t32(labels, cuda), t64(offsets, cuda), ncap - 1)
    assert int(status.item()) == 2 and not rowptr.cpu().numpy().any()


# ---- features and pool --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("two_images", 8, 40, 5), ("green_blue", 6, 40, 4), ("noise", 8, 40, 6)])
def test_region_features_bitwise(cuda, case):
    img = scene(case[0])
    labels, counts, offsets = SO.connect(slic_ref(*case)[0], case[1] * case[1] // 4, 2)
    ncap = int(offsets[-1]) + 5
    wf, ws = SO.features(img, labels, offsets, ncap)
    feat, stats = mgunet.region_features(torch.from_numpy(img).to(cuda), t32(labels, cuda), t64(offsets, cuda), ncap, return_stats=True)
    assert np.array_equal(stats.cpu().numpy(), ws)
    assert np.array_equal(feat.cpu().numpy().view(np.uint32), wf.view(np.uint32))
    assert not wf[int(offsets[-1]):].any() and wf[:, 6:].max() == 0


@pytest.mark.parametrize("D", [4, 20])
def test_region_pool_bitwise_and_within_its_bound_of_float64(cuda, D):
    labels, counts, offsets = SO.connect(slic_ref("two_images", 8, 40, 5)[0], 16, 2)
    B, H, W = labels.shape
    ncap = int(offsets[-1]) + 2
    rng = np.random.default_rng(D)
    feat = (rng.standard_normal((B, H, W, D)) * rng.choice([1e-3, 1.0, 300.0], D)).astype(np.float32)
    feat[0, 0, 0, 0], feat[0, 1, 1, 1], feat[1, 2, 2, 2], feat[1, 3, 3, 3] = 65536.0, -65536.0, np.nan, 1e30
    want = SO.pool(feat, 0, D, labels, offsets, ncap)
    x = torch.from_numpy(feat).to(cuda).permute(0, 3, 1, 2)            # the NCHW view of NHWC storage
    got = mgunet.region_pool(x, t32(labels, cuda), t64(offsets, cuda), ncap)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    clean = np.where(np.isnan(feat), 0.0, np.clip(feat.astype(np.float64), -65536, 65536))
    for b in range(B):
        for k in range(int(counts[b])):
            mean = clean[b][labels[b] == k].mean(0)
            assert np.all(np.abs(want[offsets[b] + k] - mean) <= 2.0 ** -21 + 2.0 ** -24 * np.abs(mean))
    # a channel slice of a wider tensor is read in place (ld > D) and equals the oracle's slice; c_off > 0 through the entry point
    lo = D // 4
    sl = mgunet.region_pool(x[:, lo:lo + 3], t32(labels, cuda), t64(offsets, cuda), ncap)
    wsl = SO.pool(feat, lo, 3, labels, offsets, ncap)
    assert np.array_equal(sl.cpu().numpy().view(np.uint32), wsl.view(np.uint32))
    out = torch.empty((ncap, 3), device=cuda)
    _lib.call("mgu_regions_pool_nhwc", cuda, x.permute(0, 2, 3, 1), D, lo, 3, t32(labels, cuda), t64(offsets, cuda), B, H, W, ncap, out)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), wsl.view(np.uint32))


# ---- the composition --------------------------------------------------------------------------------------------------------------------
def launch_list(cuda, img, **kw):
    ctx = _lib.context(cuda)
    L = _lib.lib()
    _lib.check(L.mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        g = mgunet.superpixel_graph(img, **kw)
        torch.cuda.synchronize()
        return g, [(k["name"], k["launches"]) for k in _lib.read_kernel_stats(ctx)]
    finally:
        _lib.check(L.mgu_profile_enable(ctx.handle, 0), ctx.handle)


def test_superpixel_graph_matches_the_oracle_repeats_bitwise_and_launches_the_same_list(cuda):
    img = scene("noise")
    g1, l1 = launch_list(cuda, img, step=8, iterations=6)
    g2 = mgunet.superpixel_graph(torch.from_numpy(img).to(cuda), step=8, iterations=6)
    for f in ("labels", "counts", "offsets", "rowptr", "col", "border", "features", "graph_ptr", "status"):
        assert torch.equal(getattr(g1, f), getattr(g2, f)), f
    labels, counts, offsets = SO.connect(slic_ref("noise", 8, 40, 6)[0], 16, 2)
    assert np.array_equal(g1.labels.cpu().numpy(), labels) and np.array_equal(g1.offsets.cpu().numpy(), offsets)
    assert g1.node_capacity == 4 * 8 * 12 and g1.edge_capacity == 6 * g1.node_capacity and g1.check() is g1
    want = SO.adjacency(labels, offsets, g1.node_capacity)
    E = want[1].size
    assert np.array_equal(g1.rowptr.cpu().numpy(), want[0]) and np.array_equal(g1.col[:E].cpu().numpy(), want[1])
    assert np.array_equal(g1.features.cpu().numpy(), SO.features(img, labels, offsets, g1.node_capacity)[0])
    assert g1.graph_ptr.dtype == torch.int32 and g1.graph_ptr.cpu().tolist() == offsets.tolist()
    ei = g1.edge_index().cpu().numpy()
    assert ei.shape == (2, E) and np.array_equal(ei[0], want[1]) and np.array_equal(ei[1], np.repeat(np.arange(g1.node_capacity), np.diff(want[0])))
    # the launch list depends on neither the batch nor the contents
    _, l3 = launch_list(cuda, np.concatenate([img, img[:, ::-1], img[:, :, ::-1]]), step=8, iterations=6)
    _, lu = launch_list(cuda, np.full_like(img, 120), step=8, iterations=6)
    assert l1 == l3 == lu and dict(l1)["slic_assign"] == 6 and dict(l1)["slic_update"] == 5
    # a smoother changes what is segmented, not what the features are taken from
    gs = mgunet.superpixel_graph(img, step=8, iterations=6, smoother=mgunet.GaussianSmoother((5, 5), 1.0))
    blurred = mgunet.GaussianSmoother((5, 5), 1.0).smooth(img[0])[None]
    ls, cs, os_ = SO.connect(SO.slic(blurred, 8, 40, 6)[0], 16, 2)
    assert np.array_equal(gs.labels.cpu().numpy(), ls)
    assert np.array_equal(gs.features.cpu().numpy(), SO.features(img, ls, os_, gs.node_capacity)[0])


def test_gat_on_the_superpixel_csr_equals_the_coo_path(cuda):
    """the agreement tests/test_gpu_gat_schedules.py::test_gat_forward_csr_equals_network_forward asserts: the same bytes"""
    img = scene("two_images")
    n = int(mgunet.superpixel_graph(img, step=8, iterations=5).offsets[-1].item())
    g = mgunet.superpixel_graph(img, step=8, iterations=5, node_capacity=n).check()
    torch.manual_seed(3)
    fmap = torch.randn(2, 37, 67, 8, device=cuda).permute(0, 3, 1, 2)
    X = torch.cat([g.features, g.pool(fmap)], dim=1).contiguous()
    net = mgunet.GATNetwork(16, 16, 8, 2).to(cuda).eval()
    with torch.no_grad():
        ref = net(X, g.edge_index(), graph_ptr=g.graph_ptr)
        got = mgunet.gat_forward_csr(net, X, g.rowptr, g.col[:int(g.rowptr[-1].item())], g.graph_ptr)
    assert got.shape == ref.shape == (n, 8) and torch.equal(got, ref)


def test_feature_fusion_places_each_regions_row_at_its_pixels(cuda):
    img = scene("two_images")
    g = mgunet.superpixel_graph(img, step=8, iterations=5)
    n = int(g.offsets[-1].item())
    table = torch.randn(n, 8, device=cuda)
    fu = torch.randn(2, 4, 37, 67, device=cuda)
    fusion = mgunet.FeatureFusion([4], 8, "concat").to(cuda).eval()
    node = g.node_map()
    assert np.array_equal(node.cpu().numpy(), g.labels.cpu().numpy() + g.offsets.cpu().numpy()[:2, None, None])
    with torch.no_grad():
        got = fusion([fu], table, region_to_pixel_map=node)
        ref = fusion([fu], table[node].permute(0, 3, 1, 2).contiguous())
    assert torch.equal(got, ref)
    one = mgunet.superpixel_graph(img[0], step=8, iterations=5)               # a batch of one: the labels are the node ids themselves
    assert torch.equal(one.node_map()[0], one.labels[0].to(torch.int64))


def test_errors_are_raised_before_anything_is_launched(cuda):
    ctx = _lib.context(cuda)
    L = _lib.lib()
    img = torch.from_numpy(scene("noise")).to(cuda)
    raw = torch.zeros((1, 64, 96), device=cuda, dtype=torch.int32)
    _lib.check(L.mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        for kw in ({}, {"step": 8, "n_segments": 96}, {"step": 3}, {"step": 129}, {"n_segments": 0}):
            with pytest.raises(ValueError):
                mgunet.superpixel_graph(img, **kw)
            with pytest.raises(ValueError):
                mgunet.slic_labels(img, **kw)
        with pytest.raises(TypeError):
            mgunet.slic_labels(img.float(), step=8)
        with pytest.raises(TypeError):
            mgunet.superpixel_graph(img.cpu().numpy().astype(np.int16), step=8)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mgunet.connect_regions(raw.cpu(), 4)
        for bad in ({"compactness": 0.0}, {"compactness": 300.0}, {"iterations": 0}, {"iterations": 33}):
            with pytest.raises(ValueError):
                mgunet.slic_labels(img, step=8, **bad)
        with pytest.raises(ValueError):
            mgunet.connect_regions(raw, 4, rounds=9)
        # overlapping outputs: the labels on top of the raw labels, the raw labels on top of the image
        cnt, off = torch.zeros(1, device=cuda, dtype=torch.int64), torch.zeros(2, device=cuda, dtype=torch.int64)
        with pytest.raises(ValueError, match="overlaps"):
            _lib.call("mgu_regions_connect", cuda, raw, 1, 64, 96, 4, 1, raw, cnt, off)
        with pytest.raises(ValueError, match="overlaps"):
            _lib.call("mgu_slic_labels", cuda, img, 1, 64, 96, 8, 40, 2, *SP._table_args(), img, None)
        bad_f = mgunet.lab_tables()[2].copy()
        bad_f[7] = 2000
        with pytest.raises(ValueError, match="above 1024"):
            _lib.call("mgu_slic_labels", cuda, img, 1, 64, 96, 8, 40, 2, SP._table_args()[0], SP._table_args()[1], bad_f.ctypes.data, raw, None)
        torch.cuda.synchronize()
        assert _lib.read_kernel_stats(ctx) == []
        assert int(raw.abs().sum().item()) == 0
    finally:
        _lib.check(L.mgu_profile_enable(ctx.handle, 0), ctx.handle)
    # an empty batch is fine and touches nothing
    empty = mgunet.slic_labels(torch.zeros((0, 8, 8, 3), device=cuda, dtype=torch.uint8), step=4)
    assert tuple(empty.shape) == (0, 8, 8)
