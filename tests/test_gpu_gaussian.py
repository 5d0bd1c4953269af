"""Gaussian blur on the device (mgunet.GaussianSmoother / mgu_gaussian_blur_u8), the fused per-patch column block
(mgu_patch_smooth_mean_u8) and patch_node_features(smoother=...).  Every comparison is bitwise: the blur against the numpy oracle of
tests/gaussian_oracle.py, the fused block against patch_features_u8 of the blurred image.  Shapes are the smallest that reach every
path: single pixels and lines (every tap reflected, repeatedly), sides below the kernel radius, one below / at / one above the tile
height (32) and the tile width (256 / channels pixels; 64 for 3 channels), rows whose bytes are and are not multiples of 16 (the
16-byte and the byte-wise stores), more than one tile both ways."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gaussian_oracle as G
import mgunet
from mgunet import GaussianSmoother, _lib
from mgunet.patch_inputs import feature_width

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE_H, TILE_W = 32, {1: 256, 3: 64, 4: 64}                  # csrc/gaussian.hip: GS_TH, gs_tile_w
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 3), (5, 70), (33, 40), (64, 64), (65, 129)]
KERNELS = {"1x1": ((1, 1), 0, None), "3x3": ((3, 3), 0, None), "5x5s1": ((5, 5), 1.0, None), "5x5s0": ((5, 5), 0, None),
           "7x3": ((7, 3), 1.0, 2.5), "1x31": ((1, 31), 4.0, None), "31x1": ((31, 1), 4.0, None), "31x31s5": ((31, 31), 5.0, None)}
GUARD = 4096
SENTINEL = 0xA5


def taps(q):
    return (C.c_int32 * len(q))(*[int(v) for v in q]), len(q)


def device_blur(batch, kx, ky, lead=GUARD):
    """mgu_gaussian_blur_u8 on a (B, H, W, C) numpy batch with the output placed `lead` bytes into a sentinel-filled buffer -> the
    output (numpy); asserts that the bytes on both sides of it are untouched"""
    B, H, W, ch = batch.shape
    n = batch.size
    src = torch.from_numpy(np.ascontiguousarray(batch)).to(DEV)
    buf = torch.full((lead + n + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    out = buf[lead:lead + n]
    _lib.call("mgu_gaussian_blur_u8", src.device, src, B, H, W, ch, *taps(kx), *taps(ky), out)
    host = buf.cpu().numpy()
    assert (host[:lead] == SENTINEL).all() and (host[lead + n:] == SENTINEL).all(), "the blur wrote outside its output"
    return host[lead:lead + n].reshape(batch.shape)


def contents(shape, seed):
    """random bytes, all 0, all 255, a 0 / 255 checkerboard"""
    B, H, W, ch = shape
    yy, xx = np.mgrid[0:H, 0:W]
    board = np.broadcast_to((((yy + xx) % 2) * 255).astype(np.uint8)[None, :, :, None], shape)
    return {"random": np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8), "zeros": np.zeros(shape, np.uint8),
            "full": np.full(shape, 255, np.uint8), "checker": np.ascontiguousarray(board)}


@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("kname", list(KERNELS))
def test_blur_matches_the_oracle_on_every_shape(kname, ch):
    ks, sx, sy = KERNELS[kname]
    kx, ky = G.kernels(ks, sx, sy)
    tw = TILE_W[ch]
    shapes = SHAPES + [(TILE_H - 1, tw - 1), (TILE_H, tw), (TILE_H + 1, tw + 1)]
    for i, (H, W) in enumerate(shapes):
        batch = np.random.RandomState(100 * i + ch).randint(0, 256, (1, H, W, ch)).astype(np.uint8)
        got = device_blur(batch, kx, ky, lead=GUARD if i % 2 == 0 else GUARD - 3)      # aligned and unaligned outputs
        assert np.array_equal(got, G.blur(batch, kx, ky)), (kname, ch, H, W)


@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("kname", ["5x5s1", "7x3", "31x31s5"])
def test_blur_of_a_batch_of_distinct_images_and_of_special_contents(kname, ch):
    ks, sx, sy = KERNELS[kname]
    kx, ky = G.kernels(ks, sx, sy)
    for H, W in ((33, 40), (65, 129), (2, 3)):
        for name, batch in contents((3, H, W, ch), H + ch).items():
            if name == "random":
                assert not np.array_equal(batch[0], batch[1])
            got = device_blur(batch, kx, ky)
            assert np.array_equal(got, G.blur(batch, kx, ky)), (kname, ch, H, W, name)
            if name in ("zeros", "full"):
                assert np.array_equal(got, batch)
            if name == "random":
                assert np.array_equal(device_blur(batch, kx, ky), got)                  # two runs, equal output
                for b in range(3):
                    assert np.array_equal(device_blur(batch[b:b + 1], kx, ky)[0], got[b])


def test_smooth_follows_the_array_in_array_out_convention(cuda):
    s = GaussianSmoother((5, 5), 1.0)
    kx, ky = G.kernels((5, 5), 1.0)
    assert np.array_equal(np.asarray(s.kernels()[0], np.int64), kx)
    rgb = np.random.RandomState(1).randint(0, 256, (33, 40, 3)).astype(np.uint8)
    out = s.smooth(rgb)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == rgb.shape
    assert np.array_equal(out, G.blur(rgb, kx, ky))
    t = torch.from_numpy(rgb).to(cuda)
    out_t = s.smooth(t)
    assert isinstance(out_t, torch.Tensor) and out_t.is_cuda and out_t.dtype == torch.uint8 and tuple(out_t.shape) == rgb.shape
    assert np.array_equal(out_t.cpu().numpy(), out)
    grey = rgb[:, :, 1].copy()
    out_g = s.smooth(grey)
    assert out_g.shape == grey.shape and np.array_equal(out_g, G.blur(grey, kx, ky))
    batch = torch.from_numpy(np.random.RandomState(2).randint(0, 256, (3, 17, 70, 3)).astype(np.uint8)).to(cuda)
    out_b = s.smooth(batch)                                                               # one launch for the batch
    assert tuple(out_b.shape) == (3, 17, 70, 3) and np.array_equal(out_b.cpu().numpy(), G.blur(batch.cpu().numpy(), kx, ky))
    wide = GaussianSmoother((7, 3), 1.0, 2.5)                                            # kernel_size is (width, height)
    assert np.array_equal(wide.smooth(rgb), G.smooth(rgb, (7, 3), 1.0, 2.5))
    assert not np.array_equal(wide.smooth(rgb), G.smooth(rgb, (3, 7), 1.0, 2.5))
    with pytest.raises(NotImplementedError):
        s.smooth(t.float())
    with pytest.raises(ValueError):
        s.smooth(torch.zeros((4, 4, 5), dtype=torch.uint8, device=cuda))


def test_invalid_arguments_surface_as_exceptions(cuda):
    img = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=cuda)
    out = torch.empty_like(img)
    good = [14, 62, 104, 62, 14]

    def call(kx, ky, o=out, B=1, H=8, W=8, ch=3, kw=None, kh=None):
        a, na = taps(kx)
        b, nb = taps(ky)
        _lib.call("mgu_gaussian_blur_u8", cuda, img, B, H, W, ch, a, na if kw is None else kw, b, nb if kh is None else kh, o)

    call(good, good)
    for bad in ([64, 64, 64, 64], [15, 62, 104, 62, 14], [-2, 66, 128, 66, -2], [0] * 16 + [256] + [0] * 16):
        with pytest.raises(ValueError):
            call(bad, good)
        with pytest.raises(ValueError):
            call(good, bad)
    with pytest.raises(ValueError):
        call(good, good, kw=0)
    with pytest.raises(ValueError, match="alias"):
        call(good, good, o=img)
    two = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError, match="alias"):
        _lib.call("mgu_gaussian_blur_u8", cuda, two[:1], 1, 8, 8, 3, *taps(good), *taps(good), two.view(-1)[96:96 + 192])
    for kw in (dict(ch=0), dict(ch=5), dict(B=0), dict(H=0), dict(H=65536, W=32768)):
        with pytest.raises(ValueError):
            call(good, good, **kw)
    feats = torch.empty((4, 3), device=cuda)
    args = (cuda, img, 1, 8, 8, 4, *taps(good), *taps(good), 1, feats)
    _lib.call("mgu_patch_smooth_mean_u8", *args, 3, 0)
    for ld, col0 in ((3, 1), (2, 0), (3, -1)):
        with pytest.raises(ValueError):
            _lib.call("mgu_patch_smooth_mean_u8", *args, ld, col0)
    for p in (0, 65):
        with pytest.raises(ValueError):
            _lib.call("mgu_patch_smooth_mean_u8", cuda, img, 1, 8, 8, p, *taps(good), *taps(good), 1, feats, 3, 0)
    with pytest.raises(ValueError):
        _lib.call("mgu_patch_smooth_mean_u8", cuda, img, 1, 8, 8, 4, *taps([64] * 4), *taps(good), 1, feats, 3, 0)


# ---- the fused per-patch column block ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rgb_batch(H, W):
    a = np.random.RandomState(H * 1000 + W).randint(0, 256, (3, H, W, 3)).astype(np.uint8)
    a[1] = (a[1] // 4 + 90).astype(np.uint8)                 # a flat image between two busy ones
    return torch.from_numpy(a).to(DEV)


@functools.lru_cache(maxsize=None)
def smoothed(H, W, kname):
    ks, sx, sy = KERNELS[kname]
    return GaussianSmoother(ks, sx, sy).smooth(rgb_batch(H, W))


@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("kname", ["5x5s1", "31x31s5"])
@pytest.mark.parametrize("H,W", [(33, 40), (65, 129)])
@pytest.mark.parametrize("p", [1, 7, 16, 64])
def test_fused_column_block_equals_patch_means_of_the_blur(p, H, W, kname, per_channel):
    ks, sx, sy = KERNELS[kname]
    s = GaussianSmoother(ks, sx, sy)
    batch = rgb_batch(H, W)
    blurred = smoothed(H, W, kname)
    want = torch.cat([mgunet.patch_features_u8(blurred[b], p, per_channel) for b in range(3)], 0)
    n = 3 if per_channel else 1
    got = mgunet.patch_smooth_features_u8(batch, p, s, per_channel)
    assert tuple(got.shape) == (want.shape[0], n) and torch.equal(got, want)
    wide = torch.full((want.shape[0], n + 5), -7.0, device=DEV)           # ld_out wider than used, col0 > 0: the rest keeps its sentinel
    r = mgunet.patch_smooth_features_u8(batch, p, s, per_channel, out=wide, col0=2)
    assert r is wide and torch.equal(wide[:, 2:2 + n], want)
    assert bool((wide[:, :2] == -7.0).all()) and bool((wide[:, 2 + n:] == -7.0).all())
    assert torch.equal(mgunet.patch_smooth_features_u8(batch, p, s, per_channel), got)                     # deterministic


def test_fused_column_block_against_the_oracle():
    batch = rgb_batch(33, 40)
    host = batch.cpu().numpy()
    for kname in ("5x5s1", "31x31s5", "7x3"):
        ks, sx, sy = KERNELS[kname]
        kx, ky = G.kernels(ks, sx, sy)
        assert np.array_equal(smoothed(33, 40, kname).cpu().numpy(), G.blur(host, kx, ky))
        for pc in (False, True):
            want = np.concatenate([G.patch_mean(G.blur(host[b], kx, ky), 16, pc) for b in range(3)], 0)
            got = mgunet.patch_smooth_features_u8(batch, 16, GaussianSmoother(ks, sx, sy), pc).cpu().numpy()
            assert got.dtype == np.float32 and np.array_equal(got, want)
    one = mgunet.patch_smooth_features_u8(host[0], 16, GaussianSmoother(), True)                           # numpy in, one image
    assert torch.equal(one, mgunet.patch_smooth_features_u8(batch[:1], 16, GaussianSmoother(), True))


# ---- patch_node_features ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_channel", [False, True])
def test_node_features_without_a_smoother_are_unchanged_and_with_one_gain_the_block(per_channel):
    batch = rgb_batch(33, 40)
    p = 16
    x = torch.from_numpy(np.random.RandomState(4).standard_normal((3, 3, 33, 40)).astype(np.float32)).to(DEV)
    feats = torch.from_numpy(np.random.RandomState(5).standard_normal((3 * 9, 6)).astype(np.float32)).to(DEV)
    base = mgunet.patch_node_features(batch, p, images=x, unet_patch_feats=feats, per_channel=per_channel)
    assert torch.equal(mgunet.patch_node_features(batch, p, images=x, unet_patch_feats=feats, per_channel=per_channel, smoother=None), base)
    assert base.shape[1] == feature_width(16, 6, per_channel) == feature_width(16, 6, per_channel, smooth=False)
    s = GaussianSmoother((5, 5), 1.0)
    n = 3 if per_channel else 1
    used0 = 16 + 6 + 1 + n
    for pad_to in (1, 4, 16):
        got = mgunet.patch_node_features(batch, p, images=x, unet_patch_feats=feats, per_channel=per_channel, pad_to=pad_to, smoother=s)
        assert got.shape[1] == feature_width(16, 6, per_channel, pad_to, True, smooth=True) and got.shape[1] >= used0 + n
        assert torch.equal(got[:, :used0], base[:, :used0])
        assert torch.equal(got[:, used0:used0 + n], mgunet.patch_smooth_features_u8(batch, p, s, per_channel))
        assert bool((got[:, used0 + n:] == 0).all())
    bare = mgunet.patch_node_features(batch, p, per_channel=per_channel, pad_to=1, smoother=s)            # no images, no U-Net rows
    assert bare.shape[1] == feature_width(0, 0, per_channel, 1, False, smooth=True) == 1 + 2 * n
    assert torch.equal(bare[:, :1 + n], mgunet.patch_node_features(batch, p, per_channel=per_channel, pad_to=1))
    assert torch.equal(bare[:, 1 + n:], mgunet.patch_smooth_features_u8(batch, p, s, per_channel))
    out = torch.full((27, feature_width(16, 6, per_channel, 4, True, smooth=True)), 3.0, device=DEV)
    r = mgunet.patch_node_features(batch, p, images=x, unet_patch_feats=feats, per_channel=per_channel, out=out, smoother=s)
    assert r is out and torch.equal(out, mgunet.patch_node_features(batch, p, images=x, unet_patch_feats=feats, per_channel=per_channel, smoother=s))
