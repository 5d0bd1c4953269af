"""Edge-aware refinement on the MI355X (csrc/refine.hip, mgunet.refine) against the numpy oracle of tests/refine_oracle.py.  Every
comparison is bitwise.  Shapes are the smallest that reach every path: single pixels and lines (every tap but the centre outside the
image), sides below the radius, one below / at / one above the kernel's tile and more than two tiles both ways (interior tiles exist only
there), for the 32 x 64 tile of 1..4 classes and the 16 x 32 tile of more; every specialised class count and the run-time one; one
iteration (outputs straight from the source), two (one plane set) and three (both plane sets)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mgunet
import mgunet_oracle as MO
import refine_oracle as R
from mgunet import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 3), (5, 70)]
GUARD = 4096                     # bytes of sentinel on both sides of every output
SENTINEL = 0xA5


def tile_of(Cls):                # csrc/refine.hip: rf_tile_h, rf_tile_w
    return (32, 64) if Cls <= 4 else (16, 32)


def all_shapes(Cls):
    TH, TW = tile_of(Cls)
    return SHAPES + [(TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 3, 2 * TW + 5)]


@functools.lru_cache(maxsize=None)
def tables(r, ss=None, sc=25.0):
    space, rng, shift = mgunet.bilateral_tables(r, ss if ss is not None else 1.0 + r / 2.0, sc)
    space.setflags(write=False), rng.setflags(write=False)
    return space, rng, shift


def guarded(nbytes, lead):
    buf = torch.full((lead + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    return buf, buf[lead:lead + nbytes]


def raw_call(src, is_prob, guide, B, H, W, Cls, G, r, space, rng, shift, T, probs, labels, conf, changed, dev=DEV):
    sp = None if space is None else np.ascontiguousarray(space, np.int32).reshape(-1)
    rl = None if rng is None else np.ascontiguousarray(rng, np.int32).reshape(-1)
    _lib.call("mgu_refine_probs", torch.device(dev), src, int(is_prob), guide, B, H, W, Cls, G, r,
              None if sp is None else sp.ctypes.data_as(C.c_void_p), None if rl is None else rl.ctypes.data_as(C.c_void_p), shift, T, probs, labels,
              conf, changed)


def device_refine(x, guide, tabs, T, is_prob=True, unaligned=False, want=("probs", "conf", "changed")):
    """mgu_refine_probs on numpy inputs (x (B, H, W, C) float32, guide (B, H, W, G) uint8) with every output inside a sentinel-filled
    buffer, at a 16-byte aligned offset or (unaligned) at the least alignment its type allows -> dict of numpy outputs; asserts that
    the bytes around every output are untouched and that an output that was not asked for does not appear"""
    space, rng, shift = tabs
    B, H, W, Cls = x.shape
    n = B * H * W
    src, g = torch.from_numpy(np.ascontiguousarray(x)).to(DEV), torch.from_numpy(np.ascontiguousarray(guide)).to(DEV)
    spec = {"probs": (n * Cls * 4, 4, np.float32, (B, H, W, Cls)), "labels": (n * 8, 8, np.int64, (B, H, W)),
            "conf": (n * 4, 4, np.float32, (B, H, W)), "changed": (B * 8, 8, np.int64, (B,))}
    bufs = {k: guarded(nb, GUARD - (al if unaligned else 0)) + (nb, al) for k, (nb, al, _, _) in spec.items() if k == "labels" or k in want}
    ptr = {k: (bufs[k][1] if k in bufs else None) for k in spec}
    raw_call(src, is_prob, g, B, H, W, Cls, guide.shape[3], space.shape[0] - 1, space, rng, shift, T, ptr["probs"], ptr["labels"], ptr["conf"],
             ptr["changed"])
    out = {}
    for k, (buf, view, nb, al) in bufs.items():
        host = buf.cpu().numpy()
        lead = GUARD - (al if unaligned else 0)
        assert (host[:lead] == SENTINEL).all() and (host[lead + nb:] == SENTINEL).all(), f"refine_probs wrote outside {k}"
        out[k] = host[lead:lead + nb].copy().view(spec[k][2]).reshape(spec[k][3])
    return out


def check(x, guide, tabs, T, tag, **kw):
    got = device_refine(x, guide, tabs, T, **kw)
    probs, labels, conf, changed, _ = R.refine(x, guide, *tabs, T)
    want = {"probs": probs, "labels": labels, "conf": conf, "changed": changed}
    for k, v in got.items():
        assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), (tag, k, int((v != want[k]).sum()))
    return got


def random_inputs(B, H, W, Cls, G, seed, kind="dirichlet"):
    rs = np.random.RandomState(seed)
    if kind == "dirichlet":
        e = rs.gamma(0.7, 1.0, (B, H, W, Cls)) + 1e-3
        x = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    else:
        x = rs.uniform(-0.3, 1.4, (B, H, W, Cls)).astype(np.float32)            # unnormalised, with values to clamp on both sides
    yy, xx = np.mgrid[0:H, 0:W]
    blobs = (128 + 100 * np.sin(yy / 3.0 + seed) * np.cos(xx / 4.0))[None, :, :, None]     # smooth regions and edges: every table bucket
    guide = np.clip(blobs + rs.randint(-25, 26, (B, H, W, G)), 0, 255).astype(np.uint8)
    return x, guide


# (radius, iterations, guide channels) by shape index: with the nine shapes of all_shapes every class count meets r in {1, 5, 7}, T in
# {1, 2, 3} and both G; the last shape (more than two tiles both ways) runs T = 3, the tile-sized ones T = 2 and 3
CASES = [(1, 1, 1), (5, 2, 3), (7, 3, 1), (1, 3, 3), (7, 1, 3), (5, 2, 1), (7, 2, 3), (1, 1, 3), (5, 3, 3)]


@pytest.mark.parametrize("Cls", [1, 2, 3, 4, 5, 16])
def test_every_shape_and_class_count_matches_the_oracle(Cls):
    for i, (H, W) in enumerate(all_shapes(Cls)):
        r, T, G = CASES[i]
        x, guide = random_inputs(1, H, W, Cls, G, 10 * i + Cls, "dirichlet" if i % 2 == 0 else "unnormalised")
        check(x, guide, tables(r), T, (Cls, H, W, r, T, G), unaligned=i % 2 == 1)
    H, W = all_shapes(Cls)[-1]                               # the multi-tile shape again: r = 7 with two iterations, r = 1 with three
    for r, T, G in ((7, 2, 3), (1, 3, 1)):
        x, guide = random_inputs(1, H, W, Cls, G, 99 + Cls + r, "unnormalised")
        check(x, guide, tables(r), T, (Cls, H, W, r, T, G))


@pytest.mark.parametrize("Cls,r,T", [(2, 5, 2), (3, 7, 1), (7, 3, 3)])
def test_a_batch_of_distinct_images_equals_the_single_image_runs(Cls, r, T):
    H, W = 37, 71
    x, guide = random_inputs(3, H, W, Cls, 3, 5 + Cls)
    assert not np.array_equal(x[0], x[1]) and not np.array_equal(guide[1], guide[2])
    got = check(x, guide, tables(r), T, ("batch", Cls))
    for b in range(3):
        one = device_refine(x[b:b + 1], guide[b:b + 1], tables(r), T)
        for k in got:
            assert np.array_equal(one[k][0], got[k][b]), (k, b)


def test_special_contents():
    H, W = 35, 70
    rs = np.random.RandomState(3)
    x, guide = random_inputs(1, H, W, 3, 3, 1, "unnormalised")
    x[0, ::3, ::5, 0] = np.nan
    x[0, 1::4, 2::3, 1] = -np.inf
    x[0, 2::5, 1::4, 2] = np.inf
    x[0, 0, 0, :] = np.nan
    check(x, guide, tables(5), 2, "nan, negatives, > 1")
    hot = np.eye(4, dtype=np.float32)[rs.randint(0, 4, (1, H, W))]
    check(hot, random_inputs(1, H, W, 4, 1, 2)[1], tables(7), 3, "one-hot")
    for Cls in (2, 5):
        flat = np.full((1, H, W, Cls), 0.3, np.float32)
        got = check(flat, random_inputs(1, H, W, Cls, 3, 4)[1], tables(5), 2, "all equal")
        assert not got["labels"].any() and got["changed"].tolist() == [0]                # the tie goes to class 0
    yy, xx = np.mgrid[0:H, 0:W]
    board = np.ascontiguousarray(np.broadcast_to((((yy + xx) % 2) * 255).astype(np.uint8)[None, :, :, None], (1, H, W, 3)))
    for sc in (4.0, 12.0):                                   # d2 = 195075 lands in the last bucket at shift 0 and at shift 1
        assert (195075 >> tables(5, 3.0, sc)[2]) > 1023
        check(random_inputs(1, H, W, 2, 3, 6)[0], board, tables(5, 3.0, sc), 2, ("checkerboard", sc))
    space, rng, shift = tables(7, 1e6, 1e6)                  # saturation: every weight 256, every numerator at the bound of 225 taps
    ones, grey = np.ones((1, 20, 37, 3), np.float32), np.full((1, 20, 37, 3), 77, np.uint8)
    for T in (1, 3):
        got = check(ones, grey, (space, rng, shift), T, "saturation")
        assert (got["probs"] == 1.0).all() and (got["conf"] == 1.0).all() and not got["labels"].any()


def test_optional_outputs_may_be_null():
    x, guide = random_inputs(2, 33, 65, 2, 3, 8)
    full = check(x, guide, tables(5), 2, "all outputs")
    for want in ((), ("probs",), ("conf",), ("changed",)):
        got = check(x, guide, tables(5), 2, want, want=want)
        assert set(got) == {"labels"} | set(want) and np.array_equal(got["labels"], full["labels"])


@pytest.mark.parametrize("Cls", [2, 3, 6])
def test_logits_path_equals_the_probabilities_of_the_devices_own_softmax(cuda, Cls):
    B, H, W = 2, 34, 67
    logits = torch.from_numpy((np.random.RandomState(Cls).standard_normal((B, H, W, Cls)) * 4).astype(np.float32)).to(cuda)
    p = torch.empty_like(logits)                             # one view, the identity: mgu_tta_merge's softmax of every pixel
    lab, cf = torch.empty((B, H, W), dtype=torch.int64, device=cuda), torch.empty((B, H, W), device=cuda)
    _lib.call("mgu_tta_merge", cuda, logits, None, B, Cls, H, W, 1, (C.c_int32 * 4)(0, 0, 0, 0), p, lab, cf)
    guide = torch.from_numpy(random_inputs(B, H, W, Cls, 3, 11)[1]).to(cuda)
    for T in (1, 3):                                         # T = 3: the count of moved pixels re-reads the logits in the last launch
        a = mgunet.refine_probs(logits.permute(0, 3, 1, 2), guide, radius=3, iterations=T, from_logits=True, return_changed=True)
        b = mgunet.refine_probs(p.permute(0, 3, 1, 2), guide, radius=3, iterations=T, return_changed=True)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        want = R.refine(p.cpu().numpy(), guide.cpu().numpy(), *mgunet.bilateral_tables(3, 3.0, 12.0), T)
        assert np.array_equal(a[1].cpu().numpy(), want[1]) and np.array_equal(a[3].cpu().numpy(), want[3])


@pytest.mark.parametrize("Cls,G,r,T", [(2, 3, 5, 2), (5, 1, 7, 3)])
def test_flips_and_the_transpose_commute_with_the_refinement(cuda, Cls, G, r, T):
    TH, TW = tile_of(Cls)
    H, W = TH + 9, 2 * TW + 3
    x, guide = random_inputs(2, H, W, Cls, G, 21 + Cls)
    xt, gt = torch.from_numpy(x).to(cuda).permute(0, 3, 1, 2), torch.from_numpy(guide).to(cuda)
    ref = mgunet.refine_probs(xt, gt, radius=r, iterations=T, return_changed=True)
    moves = {"hflip": (lambda t: t.flip(-1), lambda g: g.flip(2)), "vflip": (lambda t: t.flip(-2), lambda g: g.flip(1)),
             "transpose": (lambda t: t.transpose(-1, -2), lambda g: g.transpose(1, 2))}
    for name, (ft, fg) in moves.items():
        got = mgunet.refine_probs(ft(xt), fg(gt).contiguous(), radius=r, iterations=T, return_changed=True)
        for k in range(3):
            assert torch.equal(got[k], ft(ref[k])), (name, k)
        assert torch.equal(got[3], ref[3]), name


def test_api_shapes_dtypes_storage_and_errors(cuda):
    x, guide = random_inputs(2, 20, 30, 3, 3, 31)
    xt = torch.from_numpy(x).to(cuda).permute(0, 3, 1, 2)
    probs, labels, conf = mgunet.refine_probs(xt, guide)                                  # numpy guide
    assert tuple(probs.shape) == (2, 3, 20, 30) and probs.dtype == torch.float32 and probs.permute(0, 2, 3, 1).is_contiguous()
    assert tuple(labels.shape) == (2, 20, 30) and labels.dtype == torch.int64 and tuple(conf.shape) == (2, 20, 30) and conf.dtype == torch.float32
    want = R.refine(x, guide, *mgunet.bilateral_tables(5, 3.0, 12.0), 2)
    assert np.array_equal(probs.permute(0, 2, 3, 1).cpu().numpy(), want[0]) and np.array_equal(labels.cpu().numpy(), want[1])
    assert torch.equal(conf, probs.amax(1)) and torch.equal(conf, probs.gather(1, labels.unsqueeze(1))[:, 0])
    ref = mgunet.EdgeRefiner()
    assert all(torch.equal(u, v) for u, v in zip(ref(xt, torch.from_numpy(guide).to(cuda)), (probs, labels, conf)))
    assert all(torch.equal(u, v) for u, v in zip(mgunet.refine_probs(xt.contiguous(), guide), (probs, labels, conf)))   # NCHW storage: one copy
    one = mgunet.refine_probs(xt[:1], guide[0], return_changed=True)                      # (H, W, G) guide, batch of one
    assert torch.equal(one[1][0], labels[0]) and tuple(one[3].shape) == (1,) and one[3].dtype == torch.int64
    grey = mgunet.refine_probs(xt[:1], guide[0, :, :, 0])                                 # (H, W) guide
    assert torch.equal(grey[1], mgunet.refine_probs(xt[:1], guide[:1, :, :, :1])[1])
    empty = mgunet.refine_probs(xt[:0], guide[:0], return_changed=True)
    assert tuple(empty[0].shape) == (0, 3, 20, 30) and tuple(empty[3].shape) == (0,)
    with pytest.raises(TypeError):
        mgunet.refine_probs(xt.double(), guide)
    with pytest.raises(TypeError):
        mgunet.refine_probs(xt, guide.astype(np.float32))
    with pytest.raises(RuntimeError):
        mgunet.refine_probs(xt.cpu(), guide)
    for bad in (guide[:, :19], guide[:1], guide[..., :2], guide[0]):
        with pytest.raises(ValueError):
            mgunet.refine_probs(xt, bad)
    with pytest.raises(ValueError):
        mgunet.refine_probs(torch.zeros((1, 17, 4, 4), device=cuda), np.zeros((4, 4, 3), np.uint8))
    for kw in (dict(radius=8), dict(radius=0), dict(sigma_color=0.0), dict(iterations=0), dict(iterations=17)):
        with pytest.raises(ValueError):
            mgunet.refine_probs(xt, guide, **kw)


def profiled_launches(cuda, fn):
    """{kernel name: launches} the shared context records around fn()"""
    ctx, L = _lib.context(cuda), _lib.lib()
    _lib.check(L.mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        out = fn()
        torch.cuda.synchronize(cuda)
        return out, {k["name"]: k["launches"] for k in _lib.read_kernel_stats(ctx)}
    finally:
        _lib.check(L.mgu_profile_enable(ctx.handle, 0), ctx.handle)


def test_two_runs_are_identical_and_a_call_is_one_launch_per_iteration(cuda):
    x, guide = random_inputs(3, 70, 133, 2, 3, 41)
    xt, gt = torch.from_numpy(x).to(cuda).permute(0, 3, 1, 2), torch.from_numpy(guide).to(cuda)
    for Cls, T in ((2, 1), (2, 2), (2, 5)):
        first, n = profiled_launches(cuda, lambda: mgunet.refine_probs(xt, gt, iterations=T, return_changed=True))
        assert n == {"refine_kernel": T}, n                  # whatever B and the contents: T kernels (and one fill, which is no kernel)
        again = mgunet.refine_probs(xt, gt, iterations=T, return_changed=True)
        assert all(torch.equal(u, v) for u, v in zip(first, again))
    x6 = torch.from_numpy(random_inputs(1, 40, 50, 6, 1, 42)[0]).to(cuda).permute(0, 3, 1, 2)
    _, n = profiled_launches(cuda, lambda: mgunet.refine_probs(x6, gt[:1, :40, :50, :1].contiguous(), iterations=3))
    assert n == {"refine_kernel": 3}, n
    side = torch.cuda.Stream(cuda)                           # the call runs on the current stream and needs no synchronisation of its own
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        on_side = mgunet.refine_probs(xt, gt, iterations=3, return_changed=True)
    side.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(on_side, mgunet.refine_probs(xt, gt, iterations=3, return_changed=True)))


def test_refusals_return_the_error_launch_nothing_and_leave_the_outputs_alone(cuda):
    B, H, W, Cls, G, r = 1, 9, 11, 3, 3, 2
    x, guide = random_inputs(B, H, W, Cls, G, 51)
    src, g = torch.from_numpy(x).to(cuda), torch.from_numpy(guide).to(cuda)
    space, rng, shift = (np.array(t) if isinstance(t, np.ndarray) else t for t in tables(r))
    outs = {"probs": torch.full((B, H, W, Cls), -7.0, device=cuda), "labels": torch.full((B, H, W), -7, dtype=torch.int64, device=cuda),
            "conf": torch.full((B, H, W), -7.0, device=cuda), "changed": torch.full((B,), -7, dtype=torch.int64, device=cuda)}

    def call(**kw):
        a = dict(src=src, is_prob=1, guide=g, B=B, H=H, W=W, Cls=Cls, G=G, r=r, space=space, rng=rng, shift=shift, T=2, **outs)
        a.update(kw)
        raw_call(a["src"], a["is_prob"], a["guide"], a["B"], a["H"], a["W"], a["Cls"], a["G"], a["r"], a["space"], a["rng"], a["shift"], a["T"],
                 a["probs"], a["labels"], a["conf"], a["changed"], dev=cuda)

    def edited(t, at, v):
        t = t.copy()
        t.reshape(-1)[at] = v
        return t

    weak = edited(rng, 0, 0)                                 # centre weight (256 * 0 + 128) >> 8 = 0: a denominator could be 0
    sp, nsrc = src.data_ptr(), src.numel() * 4
    bad = [dict(Cls=0), dict(Cls=17), dict(G=2), dict(G=4), dict(G=0), dict(r=0), dict(r=8), dict(T=0), dict(T=17), dict(shift=-1), dict(shift=19),
           dict(space=edited(space, 1, 257)), dict(space=edited(space, 4, -1)), dict(rng=edited(rng, 1023, 300)), dict(rng=edited(rng, 5, -2)),
           dict(rng=weak), dict(space=edited(space, 0, 0)), dict(src=None), dict(guide=None), dict(labels=None), dict(space=None), dict(rng=None),
           dict(probs=sp), dict(probs=sp + nsrc - 4), dict(conf=sp + 20), dict(labels=sp + 8), dict(changed=sp + nsrc - 8), dict(probs=g.data_ptr()),
           dict(B=65536, H=1, W=1), dict(B=-1), dict(H=-1), dict(W=-1), dict(B=2, H=32768, W=32768), dict(B=1, H=65536, W=32768)]
    ctx, L = _lib.context(cuda), _lib.lib()
    _lib.check(L.mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        for kw in bad:
            with pytest.raises(ValueError):
                call(**kw)
        torch.cuda.synchronize(cuda)
        assert _lib.read_kernel_stats(ctx) == []             # none of them launched anything
    finally:
        _lib.check(L.mgu_profile_enable(ctx.handle, 0), ctx.handle)
    assert all(bool((t == -7).all()) for t in outs.values())
    for kw in (dict(B=0), dict(H=0), dict(W=0)):             # nothing to do: MGU_OK, nothing touched
        call(**kw)
    torch.cuda.synchronize(cuda)
    assert all(bool((t == -7).all()) for t in outs.values())
    call()                                                   # and the good call still works
    assert np.array_equal(outs["labels"].cpu().numpy(), R.refine(x, guide, space, rng, shift, 2)[1])


def unet(dev, cfg=(3, 2, 8, 2), seed=3):
    m = mgunet.UNet(*cfg)
    m.load_state_dict(MO.make_unet_params(*cfg, seed=seed))
    return m.to(dev).eval()


def test_predict_tiled_with_a_refiner(cuda):
    m = unet(cuda)
    img = np.random.default_rng(9).integers(0, 256, (70, 90, 3), dtype=np.uint8)
    kw = dict(tile=32, overlap=8, tiles_per_batch=4)
    plain = mgunet.predict_tiled(m, img, **kw)
    assert all(torch.equal(u, v) for u, v in zip(plain, mgunet.predict_tiled(m, img, refine=None, **kw)))
    ref = mgunet.EdgeRefiner(3, 2.0, 20.0, 3)
    got = mgunet.predict_tiled(m, img, refine=ref, **kw)
    want = ref(plain[0], img)
    assert len(got) == 3 and all(torch.equal(u, v) and u.dtype == v.dtype and u.stride() == v.stride() for u, v in zip(got, want))
    assert all(torch.equal(u, v) for u, v in zip(got, mgunet.refine_probs(plain[0], img, 3, 2.0, 20.0, 3)))
    swapped = mgunet.predict_tiled(m, img, bgr=True, **kw)                                 # bgr changes the network's input, not the guide
    assert all(torch.equal(u, v) for u, v in zip(mgunet.predict_tiled(m, img, bgr=True, refine=ref, **kw), ref(swapped[0], img)))
    assert all(torch.equal(u, v) for u, v in zip(ref(swapped[0], img), ref(swapped[0], img[:, :, ::-1].copy())))
    other = np.random.default_rng(10).integers(0, 256, (70, 90), dtype=np.uint8)          # a guide of the caller's, one channel
    assert all(torch.equal(u, v) for u, v in zip(mgunet.predict_tiled(m, img, refine=ref, guide=other, **kw), ref(plain[0], other)))
    x = mgunet.ImagePreprocessor(resize_dim=(70, 90)).preprocess(img).unsqueeze(0)
    with pytest.raises(ValueError, match="guide"):
        mgunet.predict_tiled(m, x, refine=ref, **kw)
    from_float = mgunet.predict_tiled(m, x, refine=ref, guide=img, **kw)
    assert all(torch.equal(u, v) for u, v in zip(from_float, ref(mgunet.predict_tiled(m, x, **kw)[0], img)))
    with pytest.raises(TypeError):
        mgunet.predict_tiled(m, img, refine=(3, 2.0, 20.0, 3), **kw)
    with pytest.raises(ValueError, match="guide"):
        mgunet.predict_tiled(m, img, guide=img, **kw)


@pytest.mark.parametrize("one_hot", [False, True])
def test_the_outline_snaps_onto_the_colour_edge_on_the_device(cuda, one_hot):
    x, guide = R.snap_scene(one_hot)
    xt = torch.from_numpy(x[None]).to(cuda).permute(0, 3, 1, 2)
    tabs = mgunet.bilateral_tables(5, 3.0, 12.0)
    for T, cols in ((4, {24}), (2, {24, 25} if one_hot else {25, 26})):
        probs, labels, conf, changed = mgunet.refine_probs(xt, guide, radius=5, sigma_space=3.0, sigma_color=12.0, iterations=T, return_changed=True)
        want = R.refine(x, guide, *tabs, T)
        assert np.array_equal(labels.cpu().numpy(), want[1]) and np.array_equal(probs.permute(0, 2, 3, 1).cpu().numpy(), want[0])
        assert changed.cpu().tolist() == want[3].tolist()
        assert set(R.outline_columns(labels[0].cpu().numpy())) == cols
