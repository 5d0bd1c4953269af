"""CPU tier of the training augmentation: the host half of ImagePreprocessor(apply_augmentation=True) and RandomFlipRotate.
pil_rotation_fixed plus a numpy restatement of PIL's fixed-point NEAREST gather equals live PIL and the fixture
(tools/make_augment_golden.py), draw_flip_rotate makes torchvision's two draws in its order, and the new C-ABI entries reject bad
arguments before any device work (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mgunet
from mgunet import _lib


def gather(img, flip, fix, fill=0):
    """numpy restatement of the device kernels: output (x, y) reads ((a2 + y a1 + x a0) >> 16, (a5 + y a4 + x a3) >> 16) of the
    (flipped) image when inside it, else `fill`."""
    h, w = img.shape[:2]
    a0, a1, a2, a3, a4, a5 = fix
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    xin, yin = (a2 + y * a1 + x * a0) >> 16, (a5 + y * a4 + x * a3) >> 16
    ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    src = img[:, ::-1] if flip else img
    out = np.full_like(img, fill)
    out[ok] = src[yin[ok], xin[ok]]
    return out


def test_fixed_point_rotation_equals_live_pil():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    n = 0
    for h, w in [(128, 128), (70, 93), (33, 500), (3, 5), (1, 1), (2, 7), (256, 64), (512, 512)]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        angles = [float(a) for a in rng.uniform(-15, 15, 6)] + [0.0, 15.0, -15.0, 1e-9, -7.5, -1e-20, 90.0, 180.0, -45.0]
        for angle in angles:
            for flip in (0, 1):
                pil = Image.fromarray(img)
                if flip:
                    pil = pil.transpose(Image.FLIP_LEFT_RIGHT)
                ref = np.asarray(pil.rotate(angle, Image.NEAREST, expand=False, center=None, fillcolor=(0, 0, 0)))
                got = gather(img, flip, mgunet.pil_rotation_fixed(angle, w, h))
                assert np.array_equal(got, ref), (h, w, angle, flip)
                n += 1
    assert n == 8 * 15 * 2


def test_fixed_point_rotation_equals_fixture(golden):
    g = golden["augment"]
    n = int(g["ncases"])
    flips, angles = set(), set()
    for k in range(n):
        H, W = (int(v) for v in g[f"{k}_dst"])
        flip, angle = int(g[f"{k}_flip"]), float(g[f"{k}_angle"])
        flips.add(flip), angles.add(angle)
        fix = mgunet.pil_rotation_fixed(angle, W, H)
        inb = gather(np.full((H, W), 255, np.uint8), flip, fix)
        assert np.array_equal(inb, g[f"{k}_inb"]), k
        # the flipped, rotated, nearest-resized mask (cv2 INTER_NEAREST index rule, as preprocess_mask)
        msrc = g[f"{k}_msrc"]
        Hs, Ws = msrc.shape
        sy = np.minimum(np.floor(np.arange(H) * (1.0 / (H / Hs))).astype(np.int64), Hs - 1)
        sx = np.minimum(np.floor(np.arange(W) * (1.0 / (W / Ws))).astype(np.int64), Ws - 1)
        assert np.array_equal(gather(np.ascontiguousarray(msrc[sy][:, sx]), flip, fix), g[f"{k}_mask"]), k
        assert g[f"{k}_img"].shape == (H, W, 3) and not g[f"{k}_img"][inb == 0].any()
    assert {0, 1} <= flips and {0.0, 15.0, -15.0} <= angles


def test_fixed_point_coefficients_and_size_limit():
    assert mgunet.pil_rotation_fixed(0.0, 64, 48) == (65536, 0, 32768, 0, 65536, 32768)   # identity, half-pixel centre
    mgunet.pil_rotation_fixed(-15.0, 8192, 8192)
    for w, h in [(8193, 16), (16, 8193), (0, 4), (4, 0)]:
        with pytest.raises(ValueError):
            mgunet.pil_rotation_fixed(3.0, w, h)
    with pytest.raises(ValueError):
        mgunet.RandomFlipRotate(degrees=15).draw(1, 9000, 8)


@pytest.mark.parametrize("p,degrees", [(0.5, 15), (0.0, 0), (1.0, 30.5), (0.25, 15)])
def test_draws_follow_torchvision_order(p, degrees):
    for seed in (0, 1, 1234):
        torch.manual_seed(seed)
        ref = []
        for _ in range(5):
            flip = torch.rand(1) < p                                        # RandomHorizontalFlip.forward
            angle = float(torch.empty(1).uniform_(float(-degrees), float(degrees)).item())   # RandomRotation.get_params
            ref.append((bool(flip), angle))
        after = torch.rand(3)
        torch.manual_seed(seed)
        got = [mgunet.draw_flip_rotate(p, degrees) for _ in range(5)]
        assert got == ref
        assert torch.equal(torch.rand(3), after)                            # the global generator is where the reference leaves it
        # an explicit generator gives the same sequence and leaves the global one alone
        g = torch.Generator().manual_seed(seed)
        torch.manual_seed(99)
        before = torch.get_rng_state()
        assert [mgunet.draw_flip_rotate(p, degrees, generator=g) for _ in range(5)] == ref
        assert torch.equal(torch.get_rng_state(), before)
    with pytest.raises(ValueError):
        mgunet.draw_flip_rotate(0.5, -1)


def test_batch_draw_table():
    aug = mgunet.RandomFlipRotate(p=0.5, degrees=15)
    t = aug.draw(6, 40, 30, generator=torch.Generator().manual_seed(5))
    g = torch.Generator().manual_seed(5)
    assert t.dtype == torch.int32 and tuple(t.shape) == (6, 7)
    for i in range(6):
        flip, angle = mgunet.draw_flip_rotate(0.5, 15, g)
        assert tuple(t[i].tolist()) == (int(flip),) + mgunet.pil_rotation_fixed(angle, 40, 30)
    fill = np.asarray(aug.fill, np.float32)
    m, s = np.float32([0.485, 0.456, 0.406]), np.float32([0.229, 0.224, 0.225])
    assert np.array_equal(fill, (np.float32(0) / np.float32(255) - m) / s)


def test_abi_rejects_null_ctx_and_bad_args():
    L = _lib.lib()
    INV = _lib.MGU_ERR_INVALID
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    st = (C.c_int64 * 4)(3 * 16 * 16, 256, 16, 1)
    fill = (C.c_float * 3)(0.0, 0.0, 0.0)
    fix = (C.c_int32 * 6)(65536, 0, 32768, 0, 65536, 32768)
    ms = (C.c_float * 3)(0.5, 0.5, 0.5)
    # null ctx: rejected before anything else
    assert L.mgu_augment_flip_rotate(None, p, p, 1, 3, 16, 16, st, st, fill, None, None, 0, p, None) == INV
    assert L.mgu_preprocess_image_u8_aug(None, p, 16, 16, 3, 1, 16, 16, ms, ms, p, 256, 16, 1, 0, fix, None) == INV
    assert L.mgu_preprocess_mask_u8_aug(None, p, 16, 16, 16, 16, 2, 0, fix, 0, p, None) == INV


def test_abi_argument_checks_precede_device_work():
    """With a (non-null) context the argument checks still come first.  Without a GPU no context can be created."""
    if not torch.cuda.is_available():
        pytest.skip("mgu_create needs a HIP device; the null-ctx checks above cover this tier")
    L = _lib.lib()
    INV = _lib.MGU_ERR_INVALID
    ctx = _lib.Context(0)
    a, b, q = (torch.zeros(64, dtype=torch.int64).data_ptr() for _ in range(3))
    st = (C.c_int64 * 4)(3 * 16 * 16, 256, 16, 1)
    fill = (C.c_float * 3)(0.0, 0.0, 0.0)
    fix = (C.c_int32 * 6)(65536, 0, 32768, 0, 65536, 32768)
    ms = (C.c_float * 3)(0.5, 0.5, 0.5)
    bad = [
        (None, b, 1, 3, 16, 16, st, st, fill, None, None, 0, q),      # null input
        (a, None, 1, 3, 16, 16, st, st, fill, None, None, 0, q),      # null output
        (a, b, 1, 3, 16, 16, None, st, fill, None, None, 0, q),       # null strides
        (a, b, 1, 3, 16, 16, st, st, None, None, None, 0, q),         # null fill
        (a, b, 1, 3, 16, 16, st, st, fill, None, None, 0, None),      # null parameter table
        (a, b, 1, 0, 16, 16, st, st, fill, None, None, 0, q),         # C < 1
        (a, b, 1, 17, 16, 16, st, st, fill, None, None, 0, q),        # C > 16
        (a, b, 0, 3, 16, 16, st, st, fill, None, None, 0, q),         # B < 1
        (a, b, 1, 3, 8193, 16, st, st, fill, None, None, 0, q),       # H above 8192
        (a, b, 1, 3, 16, 8193, st, st, fill, None, None, 0, q),       # W above 8192
        (a, b, 1, 3, 16, 16, st, st, fill, a, None, 0, q),            # mask in without mask out
        (a, a, 1, 3, 16, 16, st, st, fill, None, None, 0, q),         # in place
    ]
    for args in bad:
        assert L.mgu_augment_flip_rotate(ctx.handle, *args, None) == INV, args
        assert L.mgu_last_error(ctx.handle)
    for args in [(None, 16, 16, 3, 1, 16, 16, ms, ms, b, 256, 16, 1, 0, fix), (a, 16, 16, 3, 1, 16, 16, ms, ms, None, 256, 16, 1, 0, fix),
                 (a, 16, 16, 3, 1, 16, 16, ms, ms, b, 256, 16, 1, 0, None), (a, 16, 16, 2, 1, 16, 16, ms, ms, b, 256, 16, 1, 0, fix),
                 (a, 16, 16, 3, 1, 8193, 16, ms, ms, b, 256, 16, 1, 0, fix), (a, 16, 16, 3, 1, 16, 9000, ms, ms, b, 256, 16, 1, 0, fix)]:
        assert L.mgu_preprocess_image_u8_aug(ctx.handle, *args, None) == INV, args
    for args in [(None, 16, 16, 16, 16, 2, 0, fix, 0, b), (a, 16, 16, 16, 16, 2, 0, None, 0, b), (a, 16, 16, 16, 16, 0, 0, fix, 0, b),
                 (a, 16, 16, 8193, 16, 2, 0, fix, 0, b), (a, 16, 16, 16, 16, 2, 0, fix, 0, None)]:
        assert L.mgu_preprocess_mask_u8_aug(ctx.handle, *args, None) == INV, args
