"""CPU tier of the Gaussian blur: the package's Q8.8 weights against the definition and against the numpy oracle of the GPU tests
(gaussian_oracle.py), the oracle against the properties the definition promises and against a float64 scipy blur within the bound the
quantisation allows, and the C-ABI entries declared, bound and exported (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest
from scipy import ndimage

import gaussian_oracle as G
import mgunet
from mgunet import GaussianSmoother, _lib, gaussian_kernel_q8
from mgunet.patch_inputs import feature_width

KS = list(range(1, 32, 2))
SIGMAS = (0, 0.3, 0.5, 1, 1.5, 4, 20)
PAIRS = [((1, 1), 0, None), ((3, 3), 0, None), ((5, 5), 1.0, None), ((5, 5), 0, None), ((7, 3), 1.0, 2.0), ((1, 31), 0, None),
         ((31, 1), 3.0, None), ((31, 31), 5.0, None), ((9, 15), 20, 0.3)]


def test_the_class_is_exported_with_the_references_surface():
    s = GaussianSmoother()
    assert (s.kernel_size, s.sigma_x, s.sigma_y) == ((5, 5), 1.0, 1.0)
    s = GaussianSmoother(kernel_size=(7, 3), sigma_x=1.5, sigma_y=0.5)
    assert (s.kernel_size, s.sigma_x, s.sigma_y) == ((7, 3), 1.5, 0.5)
    assert "GaussianSmoother" in mgunet.__all__ and "gaussian_kernel_q8" in mgunet.__all__
    kx, ky = s.kernels()
    assert kx.dtype == np.int32 and ky.dtype == np.int32 and kx.size == 7 and ky.size == 3
    assert np.array_equal(kx, gaussian_kernel_q8(7, 1.5)) and np.array_equal(ky, gaussian_kernel_q8(3, 0.5))
    kx, ky = GaussianSmoother((5, 3), 1.0, -1.0).kernels()                 # sigma_y <= 0 takes sigma_x
    assert np.array_equal(ky, gaussian_kernel_q8(3, 1.0))


@pytest.mark.parametrize("ks", [(4, 5), (5, 4), (0, 3), (3, 0), (-3, 3), (3, -1), (2, 2)])
def test_even_or_non_positive_sizes_raise_the_references_error(ks):
    with pytest.raises(ValueError, match="Kernel size must be positive and odd."):
        GaussianSmoother(kernel_size=ks)


def test_sizes_above_the_limit_and_other_dtypes_are_not_implemented():
    with pytest.raises(NotImplementedError, match="31"):
        GaussianSmoother(kernel_size=(33, 3))
    with pytest.raises(NotImplementedError, match="31"):
        GaussianSmoother(kernel_size=(3, 33))
    GaussianSmoother(kernel_size=(31, 31))
    with pytest.raises(NotImplementedError, match="uint8"):
        GaussianSmoother().smooth(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError):
        gaussian_kernel_q8(4, 1.0)


def test_worked_weight_vectors():
    assert gaussian_kernel_q8(5, 1.0).tolist() == [14, 62, 104, 62, 14]     # plain rounding would sum to 257
    assert gaussian_kernel_q8(3, 0).tolist() == [64, 128, 64]
    assert gaussian_kernel_q8(5, 0).tolist() == [16, 64, 96, 64, 16]
    assert gaussian_kernel_q8(7, 0).tolist() == [8, 28, 56, 72, 56, 28, 8]
    assert gaussian_kernel_q8(1, 0).tolist() == [256] and gaussian_kernel_q8(1, 3.0).tolist() == [256]
    for k, sig in ((5, 1.0), (3, 0), (5, 0), (7, 0)):
        assert G.q8_kernel(k, sig).tolist() == gaussian_kernel_q8(k, sig).tolist()


@pytest.mark.parametrize("k", KS)
def test_weights_sum_symmetry_error_and_oracle(k):
    for sig in SIGMAS:
        q = gaussian_kernel_q8(k, sig)
        w = G.float_kernel(k, sig)
        assert q.dtype == np.int32 and q.shape == (k,)
        assert int(q.sum()) == 256, (k, sig)
        assert np.array_equal(q, q[::-1]) and int(q.min()) >= 0, (k, sig)
        assert float(np.abs(q - 256.0 * w).max()) <= 1.0, (k, sig)
        assert np.array_equal(q, G.q8_kernel(k, sig)), (k, sig)
        assert abs(float(w.sum()) - 1.0) <= 1e-12


def rand_img(shape, seed=0):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


@pytest.mark.parametrize("ks,sx,sy", PAIRS)
def test_oracle_keeps_constant_images(ks, sx, sy):
    kx, ky = G.kernels(ks, sx, sy)
    for v in (0, 1, 127, 128, 254, 255):
        img = np.full((6, 9, 2), v, np.uint8)
        assert np.array_equal(G.blur(img, kx, ky), img)


def test_oracle_identity_impulse_and_pass_order():
    img = rand_img((13, 17, 3))
    one = np.array([256])
    assert np.array_equal(G.blur(img, one, one), img)
    assert np.array_equal(G.smooth(img, (1, 1), 0), img)
    for ks, sx, sy in PAIRS:
        kx, ky = G.kernels(ks, sx, sy)
        H, W = 2 * len(ky) + 1, 2 * len(kx) + 1              # the impulse's support stays clear of the borders
        imp = np.zeros((H, W), np.uint8)
        imp[H // 2, W // 2] = 255
        want = np.zeros((H, W), np.int64)
        want[H // 2 - len(ky) // 2:H // 2 + len(ky) // 2 + 1, W // 2 - len(kx) // 2:W // 2 + len(kx) // 2 + 1] = \
            (255 * np.outer(ky, kx) + 32768) >> 16
        assert np.array_equal(G.blur(imp, kx, ky), want.astype(np.uint8))
        assert np.array_equal(G.blur(img, kx, ky), G.blur(img, kx, ky, vertical_first=True))
    batch = rand_img((3, 7, 5, 4), 3)
    kx, ky = G.kernels((5, 3), 1.0)
    assert np.array_equal(G.blur(batch, kx, ky), np.stack([G.blur(b, kx, ky) for b in batch]))


def test_oracle_on_images_narrower_than_the_radius():
    kx, ky = G.kernels((31, 31), 5.0)
    one = np.array([[200]], np.uint8)
    assert np.array_equal(G.blur(one, kx, ky), one)
    img = rand_img((2, 3), 5)
    got = G.blur(img, kx, ky)
    # the brute-force form: every tap through the repeated reflection, one pixel at a time
    want = np.zeros((2, 3), np.int64)
    for y in range(2):
        for x in range(3):
            want[y, x] = sum(int(ky[dy]) * sum(int(kx[dx]) * int(img[G.reflect(y + dy - 15, 2), G.reflect(x + dx - 15, 3)]) for dx in range(31))
                             for dy in range(31))
    assert np.array_equal(got, ((want + 32768) >> 16).astype(np.uint8))
    assert [G.reflect(i, 2) for i in range(-5, 6)] == [1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert [G.reflect(i, 3) for i in range(-5, 8)] == [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1]
    assert [G.reflect(i, 1) for i in (-20, 0, 20)] == [0, 0, 0]


@pytest.mark.parametrize("ks,sx,sy", PAIRS)
def test_oracle_stays_within_the_quantisation_bound_of_a_float64_blur(ks, sx, sy):
    """|fixed point - float64| <= 0.5 + 255 (ex + ey + ex ey), ex = sum |q_i / 256 - w_i|: the final rounding plus what the weight errors of
    the two passes can add to a value of at most 255.  The bound is computed per kernel (it reaches a few grey levels at 31 taps)."""
    sy_eff = sx if sy is None or sy <= 0 else sy
    wx, wy = G.float_kernel(ks[0], sx), G.float_kernel(ks[1], sy_eff)
    kx, ky = G.kernels(ks, sx, sy)
    ex, ey = float(np.abs(kx / 256.0 - wx).sum()), float(np.abs(ky / 256.0 - wy).sum())
    bound = 0.5 + 255.0 * (ex + ey + ex * ey)
    img = rand_img((40, 47), 11)
    img[:8, :8] = 255
    img[30:, 30:] = 0
    ref = ndimage.correlate1d(ndimage.correlate1d(img.astype(np.float64), wx, axis=1, mode="mirror"), wy, axis=0, mode="mirror")
    dev = float(np.abs(G.blur(img, kx, ky).astype(np.float64) - ref).max())
    print(f"kernel {ks} sigma ({sx}, {sy}): deviation {dev:.3f}, bound {bound:.3f}")
    assert dev <= bound + 1e-9


def test_feature_width_counts_the_smooth_block():
    assert feature_width() == 20 and feature_width(smooth=False) == 20
    assert feature_width(smooth=True) == 24                       # 16 + 1 + 3 + 3 -> 23 -> 24
    assert feature_width(smooth=True, pad_to=1) == 23
    assert feature_width(0, 0, False, 1, False, smooth=True) == 3
    assert feature_width(16, 8, True, 4, True, smooth=True) == 32  # 16 + 8 + 1 + 3 + 3 = 31


def test_entries_are_declared_bound_and_exported():
    protos = _lib.parse_header()
    for name, n_args in (("mgu_gaussian_blur_u8", 12), ("mgu_patch_smooth_mean_u8", 15)):
        assert name in protos
        res, args, takes_stream = protos[name]
        assert res is C.c_int and takes_stream and len(args) == n_args
        assert hasattr(_lib.lib(), name)
    assert protos["mgu_gaussian_blur_u8"][1][2:6] == [C.c_int] * 4 and protos["mgu_gaussian_blur_u8"][1][6] is C.c_void_p
