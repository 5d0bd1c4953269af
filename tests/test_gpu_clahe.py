"""CLAHE on the device (mgunet.CLAHE / mgu_clahe_u8), the fused per-patch column block (mgu_patch_clahe_mean_u8) and
patch_node_features(equalizer=...).  Every comparison is bitwise: the image and the tables against the numpy oracle of
tests/clahe_oracle.py, the fused block against patch_features_u8 of the equalised image.  Shapes are the smallest that reach every
path: single pixels and lines, tiles of one pixel (every extended index reflected more than once), OpenCV's extension of both axes,
tile sides that are no power of two (where a fused multiply-add gives other bytes: tests/test_clahe_host.py), tile widths one below /
at / one above the apply kernel's chunk width and cells taller than its chunk height, rows whose bytes are and are not multiples of 16
(the 16-byte and the byte-wise loads and stores), cells that start off a 16-pixel boundary inside such rows."""
import functools

import numpy as np
import pytest
import torch

import clahe_oracle as O
import mgunet
from mgunet import CLAHE, _lib
from mgunet.patch_inputs import feature_width

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHUNK_W, CHUNK_H, VEC = 64, 64, 16                         # csrc/clahe.hip: CL_CHUNK_W, CL_CHUNK_H, CL_VEC
GUARD = 4096
SENTINEL = 0xA5
# (H, W, grid_y, grid_x)
SHAPES = [(1, 1, 1, 1), (1, 7, 2, 2), (3, 5, 8, 8), (16, 16, 1, 1), (64, 64, 8, 8), (64, 60, 8, 8), (96, 96, 8, 8), (50, 70, 8, 8),
          (65, 129, 4, 3), (37, 41, 5, 7), (130, 70, 2, 64),
          (8, 2 * (CHUNK_W - 1), 2, 2), (8, 2 * CHUNK_W, 2, 2), (8, 2 * (CHUNK_W + 1), 2, 2),        # tile width 63, 64, 65; 128 x ch bytes: 16-byte rows
          (2 * (CHUNK_H + 1), 2 * VEC, 2, 2),                                                        # cells taller than a chunk, 16-byte rows
          (32, 160, 2, 2)]                                                                           # 16-byte rows, cells from x = 40: ragged edges
CLIPS = [0.0, 0.01, 2.0, 40.0, 1e6]


def guarded(n, lead):
    buf = torch.full((lead + n + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    return buf, buf[lead:lead + n]


def untouched(buf, lead, n):
    host = buf.cpu().numpy()
    return bool((host[:lead] == SENTINEL).all() and (host[lead + n:] == SENTINEL).all())


def device_clahe(batch, gy, gx, clip, lead=GUARD, with_luts=True):
    """mgu_clahe_u8 on a (B, H, W, C) numpy batch, the output and the tables each `lead` bytes into a sentinel-filled buffer ->
    (output, tables | None) as numpy; asserts that the bytes around both are untouched"""
    B, H, W, ch = batch.shape
    n, nl = batch.size, B * gy * gx * 256
    src = torch.from_numpy(np.array(batch)).to(DEV)
    obuf, out = guarded(n, lead)
    lbuf, luts = guarded(nl, lead)
    _lib.call("mgu_clahe_u8", src.device, src, B, H, W, ch, gy, gx, float(clip), out, luts if with_luts else None)
    assert untouched(obuf, lead, n), "the image wrote outside its output"
    assert untouched(lbuf, lead, nl), "the tables wrote outside their buffer"
    lh = luts.cpu().numpy().reshape(B, gy, gx, 256)
    if not with_luts:
        assert bool((lh == SENTINEL).all())
    return out.cpu().numpy().reshape(batch.shape), (lh if with_luts else None)


@functools.lru_cache(maxsize=None)
def image(H, W, ch, seed):
    a = np.random.RandomState(seed).randint(0, 256, (1, H, W, ch)).astype(np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def expected(H, W, ch, seed, gy, gx, clip):
    return O.clahe(image(H, W, ch, seed), gy, gx, clip)


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("clip", CLIPS)
def test_image_and_tables_match_the_oracle_on_every_shape(clip, ch):
    for i, (H, W, gy, gx) in enumerate(SHAPES):
        batch = image(H, W, ch, 100 * i + ch)
        want, wluts = expected(H, W, ch, 100 * i + ch, gy, gx, clip)
        got, luts = device_clahe(batch, gy, gx, clip, lead=GUARD if i % 2 == 0 else GUARD - 3)      # aligned and unaligned outputs
        assert np.array_equal(luts, wluts), (H, W, gy, gx, "tables")
        assert np.array_equal(got, want), (H, W, gy, gx, "image", int((got != want).sum()))
        alone, _ = device_clahe(batch, gy, gx, clip, lead=GUARD - 3 if i % 2 == 0 else GUARD, with_luts=False)   # tables in scratch
        assert np.array_equal(alone, want), (H, W, gy, gx, "image without luts_dev")


def contents(shape, seed):
    """random bytes (distinct images), all 0, all 255, constant 77, a 0 / 255 checkerboard, a horizontal ramp"""
    B, H, W, ch = shape
    yy, xx = np.mgrid[0:H, 0:W]
    board = np.broadcast_to((((yy + xx) % 2) * 255).astype(np.uint8)[None, :, :, None], shape)
    ramp = np.broadcast_to((xx * 255 // max(W - 1, 1)).astype(np.uint8)[None, :, :, None], shape)
    return {"random": np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8), "zeros": np.zeros(shape, np.uint8),
            "full": np.full(shape, 255, np.uint8), "const77": np.full(shape, 77, np.uint8), "checker": np.ascontiguousarray(board),
            "ramp": np.ascontiguousarray(ramp)}


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("H,W,gy,gx", [(65, 129, 4, 3), (50, 70, 8, 8)])
def test_a_batch_of_distinct_images_and_special_contents(H, W, gy, gx, ch):
    for name, batch in contents((3, H, W, ch), H + ch).items():
        for clip in (2.0, 40.0):
            want, wluts = O.clahe(batch, gy, gx, clip)
            got, luts = device_clahe(batch, gy, gx, clip)
            assert np.array_equal(luts, wluts) and np.array_equal(got, want), (name, clip)
        if name == "random":
            assert not np.array_equal(batch[0], batch[1])
            again, luts2 = device_clahe(batch, gy, gx, 40.0)
            assert np.array_equal(again, got) and np.array_equal(luts2, luts)                      # two runs, equal output
            for b in range(3):
                assert np.array_equal(device_clahe(batch[b:b + 1], gy, gx, 40.0)[0][0], got[b])
            t = torch.from_numpy(batch).to(DEV)                                                     # in place
            _lib.call("mgu_clahe_u8", t.device, t, 3, H, W, ch, gy, gx, 40.0, t, None)
            assert np.array_equal(t.cpu().numpy(), got)


@pytest.mark.parametrize("side,clip,probe", [(16, 255.0, [1, 1, 255, 255, 255]), (16, 128.0, [1, 39, 166, 192, 255]),
                                             (16, 100.0, [1, 77, 177, 228, 255]), (32, 64.0, None)])
def test_every_branch_of_the_redistribution(side, clip, probe):
    batch = np.full((1, side, side, 1), 77, np.uint8)
    want, wluts = O.clahe(batch, 1, 1, clip)
    got, luts = device_clahe(batch, 1, 1, clip)
    assert np.array_equal(luts, wluts) and np.array_equal(got, want)
    if probe is not None:
        assert luts[0, 0, 0][[0, 76, 77, 128, 255]].tolist() == probe
    assert bool((got == luts[0, 0, 0, 77]).all())


# ---- the fused per-patch column block ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rgb_batch(H, W):
    a = np.random.RandomState(H * 1000 + W).randint(0, 256, (3, H, W, 3)).astype(np.uint8)
    a[1] = (a[1] // 4 + 90).astype(np.uint8)                 # a flat image between two busy ones
    return torch.from_numpy(a).to(DEV)


@functools.lru_cache(maxsize=None)
def equalised(H, W, clip, grid):
    out = CLAHE(clip, grid).apply(rgb_batch(H, W))
    want, _ = O.clahe(rgb_batch(H, W).cpu().numpy(), grid[1], grid[0], clip)
    assert np.array_equal(out.cpu().numpy(), want)
    return out


@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("H,W,clip,grid", [(33, 40, 2.0, (8, 8)), (65, 129, 4.0, (3, 4))])
@pytest.mark.parametrize("p", [1, 7, 16, 64])
def test_fused_column_block_equals_patch_means_of_the_equalised_image(p, H, W, clip, grid, per_channel):
    c = CLAHE(clip, grid)
    batch = rgb_batch(H, W)
    eq = equalised(H, W, clip, grid)
    want = torch.cat([mgunet.patch_features_u8(eq[b], p, per_channel) for b in range(3)], 0)
    n = 3 if per_channel else 1
    got = mgunet.patch_clahe_features_u8(batch, p, c, per_channel)
    assert tuple(got.shape) == (want.shape[0], n) and torch.equal(got, want)
    wide = torch.full((want.shape[0], n + 5), -7.0, device=DEV)           # ld_out wider than used, col0 > 0: the rest keeps its sentinel
    r = mgunet.patch_clahe_features_u8(batch, p, c, per_channel, out=wide, col0=2)
    assert r is wide and torch.equal(wide[:, 2:2 + n], want)
    assert bool((wide[:, :2] == -7.0).all()) and bool((wide[:, 2 + n:] == -7.0).all())
    assert torch.equal(mgunet.patch_clahe_features_u8(batch, p, c, per_channel), got)                       # deterministic
    one = mgunet.patch_clahe_features_u8(batch[1].cpu().numpy(), p, c, per_channel)                         # numpy in, one image
    rows = want.shape[0] // 3
    assert torch.equal(one, want[rows:2 * rows])


@pytest.mark.parametrize("per_channel", [False, True])
def test_node_features_take_the_equalised_block_from_clahe(per_channel):
    batch = rgb_batch(33, 40)
    p = 16
    x = torch.from_numpy(np.random.RandomState(4).standard_normal((3, 3, 33, 40)).astype(np.float32)).to(DEV)
    feats = torch.from_numpy(np.random.RandomState(5).standard_normal((3 * 9, 6)).astype(np.float32)).to(DEV)
    kw = dict(images=x, unet_patch_feats=feats, per_channel=per_channel)
    base = mgunet.patch_node_features(batch, p, **kw)
    assert torch.equal(mgunet.patch_node_features(batch, p, equalizer=None, **kw), base)
    c = CLAHE(2.0, (8, 8))
    n = 3 if per_channel else 1
    e0 = 16 + 6 + 1                                                        # the equalised block's first column
    block = mgunet.patch_clahe_features_u8(batch, p, c, per_channel)
    got = mgunet.patch_node_features(batch, p, equalizer=c, **kw)
    assert got.shape == base.shape                                         # a GAT's Fin does not move
    assert torch.equal(got[:, :e0], base[:, :e0]) and torch.equal(got[:, e0 + n:], base[:, e0 + n:])
    assert torch.equal(got[:, e0:e0 + n], block) and not torch.equal(block, base[:, e0:e0 + n])
    s = mgunet.GaussianSmoother((5, 5), 1.0)                               # with the smoothed block behind it
    both = mgunet.patch_node_features(batch, p, equalizer=c, smoother=s, **kw)
    plain = mgunet.patch_node_features(batch, p, smoother=s, **kw)
    assert both.shape == plain.shape and both.shape[1] == feature_width(16, 6, per_channel, 4, True, smooth=True)
    assert torch.equal(both[:, :e0], plain[:, :e0]) and torch.equal(both[:, e0 + n:], plain[:, e0 + n:]) and torch.equal(both[:, e0:e0 + n], block)
    bare = mgunet.patch_node_features(batch, p, per_channel=per_channel, pad_to=1, equalizer=c)              # no images, no U-Net rows
    assert bare.shape[1] == 1 + n and torch.equal(bare[:, 1:], block)
    assert torch.equal(bare[:, :1], mgunet.patch_node_features(batch, p, per_channel=per_channel, pad_to=1)[:, :1])


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_nothing_is_written(cuda):
    img = torch.full((2, 8, 8, 3), 9, dtype=torch.uint8, device=cuda)
    obuf, out = guarded(img.numel(), GUARD)
    lbuf, luts = guarded(2 * 4 * 256, GUARD)

    def call(i=img, o=out, lu=luts, B=2, H=8, W=8, ch=3, gy=2, gx=2, clip=2.0):
        _lib.call("mgu_clahe_u8", cuda, i, B, H, W, ch, gy, gx, clip, o, lu)

    bad = [dict(ch=0), dict(ch=2), dict(ch=4), dict(gy=0), dict(gy=65), dict(gx=0), dict(gx=65), dict(clip=float("nan")), dict(clip=float("inf")),
           dict(clip=float("-inf")), dict(i=None), dict(o=None), dict(B=0), dict(H=0), dict(W=0), dict(H=65536, W=32768), dict(B=65536),
           dict(o=img.view(-1)[3:]), dict(lu=img), dict(lu=out)]
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
    assert bool((obuf == SENTINEL).all()) and bool((lbuf == SENTINEL).all()) and bool((img == 9).all())
    call()                                                                  # and the valid call goes through
    assert untouched(obuf, GUARD, img.numel()) and not bool((out == SENTINEL).all())
    feats = torch.full((2 * 4, 3), -7.0, device=cuda)

    def pcall(B=2, H=8, W=8, p=4, gy=2, gx=2, clip=2.0, pc=1, f=feats, ld=3, col0=0, i=img):
        _lib.call("mgu_patch_clahe_mean_u8", cuda, i, B, H, W, p, gy, gx, clip, pc, f, ld, col0)

    for kw in (dict(p=0), dict(p=65), dict(gy=0), dict(gx=65), dict(clip=float("nan")), dict(i=None), dict(f=None), dict(B=0), dict(B=65536),
               dict(H=65536, W=32768), dict(col0=1), dict(col0=-1), dict(ld=2)):
        with pytest.raises(ValueError):
            pcall(**kw)
    assert bool((feats == -7.0).all())
    pcall()
    assert not bool((feats == -7.0).any())


def test_two_launches_whatever_the_batch_the_grid_and_the_data(cuda):
    """the launches csrc/clahe.hip records while the context profiles: one table launch and one blend (or patch) launch per call"""
    ctx = _lib.context(cuda)

    def launches(fn):
        _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 1), ctx.handle)
        try:
            fn()
            return {k["name"]: k["launches"] for k in _lib.read_kernel_stats(ctx)}
        finally:
            _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 0), ctx.handle)

    for B, H, W, ch, gy, gx in ((1, 8, 8, 1, 1, 1), (5, 130, 70, 3, 2, 64), (2, 64, 64, 1, 8, 8)):
        img = torch.from_numpy(np.random.RandomState(B).randint(0, 256, (B, H, W, ch)).astype(np.uint8)).to(cuda)
        out = torch.empty_like(img)
        got = launches(lambda: _lib.call("mgu_clahe_u8", cuda, img, B, H, W, ch, gy, gx, 2.0, out, None))
        assert got == {"clahe_lut_kernel": 1, "clahe_apply_kernel": 1}, (B, H, W, got)
        if ch == 3:
            got = launches(lambda: mgunet.patch_clahe_features_u8(img, 16, CLAHE(2.0, (gx, gy)), True))
            assert got == {"clahe_lut_kernel": 1, "patch_clahe_mean_kernel": 1}, got


def test_apply_follows_the_array_in_array_out_convention(cuda):
    c = CLAHE(2.0, (4, 3))                                                  # (x, y): three tile rows, four tile columns
    rgb = np.random.RandomState(1).randint(0, 256, (33, 40, 3)).astype(np.uint8)
    want, wluts = O.clahe(rgb[None], 3, 4, 2.0)
    out = c.apply(rgb)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == rgb.shape and np.array_equal(out, want[0])
    assert not np.array_equal(out, O.clahe(rgb[None], 4, 3, 2.0)[0][0])
    tabs = c.tables(rgb)
    assert isinstance(tabs, np.ndarray) and tabs.shape == (1, 3, 4, 256) and np.array_equal(tabs, wluts)
    t = torch.from_numpy(rgb).to(cuda)
    out_t = c.apply(t)
    assert isinstance(out_t, torch.Tensor) and out_t.is_cuda and out_t.dtype == torch.uint8 and tuple(out_t.shape) == rgb.shape
    assert np.array_equal(out_t.cpu().numpy(), out) and np.array_equal(t.cpu().numpy(), rgb)
    assert torch.equal(c.tables(t), torch.from_numpy(wluts).to(cuda))
    grey = rgb[:, :, 1].copy()
    gwant = O.clahe(grey[None, :, :, None], 3, 4, 2.0)[0][0, :, :, 0]
    assert np.array_equal(c.apply(grey), gwant) and np.array_equal(c.apply(grey[:, :, None]), gwant[:, :, None])
    batch = np.random.RandomState(2).randint(0, 256, (3, 17, 70, 3)).astype(np.uint8)
    bt = torch.from_numpy(batch).to(cuda)
    assert np.array_equal(c.apply(bt).cpu().numpy(), O.clahe(batch, 3, 4, 2.0)[0])
    gb = np.ascontiguousarray(batch[..., 0])                                # a (B, H, W) grey batch: only when stated
    gbw = O.clahe(gb[..., None], 3, 4, 2.0)[0][..., 0]
    assert np.array_equal(c.apply(gb, channels=1), gbw) and np.array_equal(c.apply(gb[..., None]), gbw[..., None])
    with pytest.raises(ValueError):
        c.apply(gb)
    dst = np.zeros_like(rgb)
    assert c.apply(rgb, out=dst) is dst and np.array_equal(dst, out)
    dst_t = torch.zeros_like(t)
    assert c.apply(t, out=dst_t) is dst_t and np.array_equal(dst_t.cpu().numpy(), out)
    assert c.apply(t, out=t) is t and np.array_equal(t.cpu().numpy(), out)  # in place
    eq = mgunet.HistogramEqualizer()
    assert np.array_equal(eq.clahe_rgb(rgb, 2.0, (4, 3)), out) and np.array_equal(eq.clahe_gray(grey, 2.0, (4, 3)), gwant)
    assert np.array_equal(eq.clahe_rgb(rgb), O.clahe(rgb[None], 8, 8, 40.0)[0][0])                 # cv2's defaults
