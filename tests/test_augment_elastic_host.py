"""CPU tier of the elastic deformation (RandomElasticAffineColor, mgu_augment_elastic_color, mgu_elastic_field): the names it adds, the
argument refusals, the weight table, elastic_control in Python integers, the draw order, the oracle's identities (zero and constant
control are the affine oracle), the factored field against the definition's double sum, thirteen wrong readings of the definition that
the shared cases tell apart, and the coverage the GPU tier relies on.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mgunet
import augment_affine_oracle as AO
import augment_elastic_cases as EC
import augment_elastic_oracle as EO
from mgunet import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AC_IDENT = EC.AC.IDENT_ROW      # reads the source pixel of the same index


def test_names_are_declared_bound_and_exported():
    for name in ("RandomElasticAffineColor", "bspline_weights_q14", "elastic_control", "elastic_field"):
        assert name in mgunet.__all__ and callable(getattr(mgunet, name)), name
    assert issubclass(mgunet.RandomElasticAffineColor, mgunet.RandomAffineColor)
    header = open(os.path.join(ROOT, "include", "mgunet.h")).read()
    for name in ("mgu_augment_elastic_color", "mgu_elastic_field"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(_lib.lib(), name)
    protos = mgunet._lib.parse_header()
    assert protos["mgu_augment_elastic_color"][2] and protos["mgu_elastic_field"][2]
    args, affine = protos["mgu_augment_elastic_color"][1], protos["mgu_augment_affine_color"][1]
    assert args[:19] == affine[:19] and len(args) == 26      # the affine entry's arguments, then labels, fill, nodes, gh, gw, stream
    assert args[19:25] == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.c_int]
    assert "augment_elastic.hip" in open(os.path.join(ROOT, "mingraph-unet_amd", "csrc", "Makefile")).read()
    for word in ("su = ((gw - 3) << 16) / W", "w_k = (2 * 16384 n_k + D) / (2 D)", "D = (acc + 2^27) >> 28", "sx = a2 + y a1 + x a0 + Dx"):
        assert word in header, word                          # the definition is in the header


def abi_args(**kw):
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    a = dict(img=p, B=1, Hs=16, Ws=16, bgr=0, mask=None, nc=0, out=p, H=16, W=16, st=(C.c_int64 * 4)(768, 256, 16, 1),
             mean=(C.c_float * 3)(0.5, 0.5, 0.5), std=(C.c_float * 3)(0.5, 0.5, 0.5), fill=(C.c_uint8 * 3)(0, 0, 0), mout=None, mfill=-100,
             params=p, need_mean=1, labels=None, lout=None, lfill=0, ctrl=p, gh=6, gw=6)
    for k, v in kw.items():
        a[k] = p if v == "set" else v
    return list(a.values())


@pytest.mark.parametrize("kw, message", [
    (dict(img=None), "null pointer"), (dict(out=None), "null pointer"), (dict(params=None), "null pointer"),
    (dict(B=0), ">= 1"), (dict(W=-3), ">= 1"), (dict(Hs=8193), "above 8192"), (dict(W=8193), "above 8192"),
    (dict(mask="set"), "mask_u8 and mask_out go together"), (dict(mout="set"), "mask_u8 and mask_out go together"),
    (dict(labels="set"), "labels_i32 and labels_out go together"), (dict(lout="set"), "labels_i32 and labels_out go together"),
    (dict(gh=3), "control nodes"), (dict(gw=33), "control nodes"), (dict(gh=0), "control nodes"), (dict(gw=0, gh=0), "control nodes"),
    (dict(ctrl=None), "control nodes"), (dict(ctrl=None, gh=0), "control nodes"),
    (dict(B=32768, H=8192, W=8192), "2^31"),
    ({}, "null context"), (dict(ctrl=None, gh=0, gw=0), "null context"), (dict(gh=4, gw=32), "null context"),
    (dict(labels="set", lout="set", mask="set", mout="set"), "null context")])
def test_each_refusal_returns_invalid_with_its_message_before_any_device_work(kw, message):
    L = _lib.lib()
    assert L.mgu_augment_elastic_color(None, *abi_args(**kw), None) == _lib.MGU_ERR_INVALID
    assert message in L.mgu_last_error(None).decode(), (kw, L.mgu_last_error(None))


def test_field_entry_refusals():
    L = _lib.lib()
    buf = (C.c_int64 * 8)()
    p = C.cast(buf, C.c_void_p)
    for args, message in (((None, 1, 6, 6, 8, 8, p), "null pointer"), ((p, 1, 6, 6, 8, 8, None), "null pointer"), ((p, 0, 6, 6, 8, 8, p), ">= 1"),
                          ((p, 1, 6, 6, 8, 8193, p), "above 8192"), ((p, 1, 3, 6, 8, 8, p), "control nodes"), ((p, 1, 6, 33, 8, 8, p), "control nodes"),
                          ((p, 32768, 6, 6, 8192, 8192, p), "2^31"), ((p, 1, 4, 32, 8, 8, p), "null context")):
        assert L.mgu_elastic_field(None, *args, None) == _lib.MGU_ERR_INVALID
        assert message in L.mgu_last_error(None).decode(), args


def test_cpu_tensors_and_bad_options_are_refused():
    aug = mgunet.RandomElasticAffineColor(16)
    with pytest.raises(RuntimeError, match="HIP device"):
        aug(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="HIP device"):
        mgunet.elastic_field(torch.zeros(1, 2, 6, 6, dtype=torch.int32), (8, 8))
    with pytest.raises(TypeError):
        mgunet.elastic_field(torch.zeros(1, 2, 6, 6), (8, 8))
    for kw in (dict(nodes=(3, 6)), dict(nodes=(6, 33)), dict(sigma=-1.0), dict(label_fill=2 ** 31)):
        with pytest.raises(ValueError):
            mgunet.RandomElasticAffineColor(16, **kw)


# ---- the weight table ---------------------------------------------------------------------------------------------------------------
def test_weight_table():
    w = mgunet.bspline_weights_q14()
    assert w.shape == (256, 4) and w.dtype == np.int32 and np.array_equal(w, EO.weights_q14())
    assert (w.sum(axis=1) == 16384).all() and w.min() >= 0
    assert w[0].tolist() == [2731, 10922, 2731, 0] and w[128].tolist() == [341, 7851, 7851, 341]
    raw = EO.weights_q14("weights_unnormalised")
    assert np.abs(16384 - raw.sum(axis=1)).max() == 1                          # the remainder is at most one unit
    t = np.arange(256) / 256.0                                                 # and the table is the cubic B-spline to half a unit
    f = np.stack([(1 - t) ** 3, 3 * t ** 3 - 6 * t ** 2 + 4, -3 * t ** 3 + 3 * t ** 2 + 3 * t + 1, t ** 3], axis=1) / 6.0
    assert np.abs(raw - f * 16384).max() <= 0.5 + 1e-9 and np.abs(w - f * 16384).max() <= 1.5 + 1e-9


def test_floor_keeps_the_last_pixel_inside_the_lattice():
    for g in (4, 5, 7, 32):
        for W in (1, 2, 3, 7, 31, 32, 33, 100, 511, 512, 513, 4095, 8191, 8192):
            su = ((g - 3) << 16) // W
            assert ((W - 1) * su + (su >> 1)) >> 16 <= g - 4, (g, W)


# ---- elastic_control and the draws ------------------------------------------------------------------------------------------------------
def test_elastic_control_equals_the_oracle_on_python_ints():
    rng = np.random.default_rng(3)
    for nodes, sigma, name, hw in (((4, 4), 10.0, "combined", ((40, 24), (33, 65))), ((6, 5), 3.0, "warp", ((24, 40), (64, 64))),
                                   ((32, 32), 0.37, "rot90", ((64, 64), (64, 64))), ((7, 9), 25.0, "zoom_half", ((96, 80), (64, 128)))):
        n = rng.standard_normal((2,) + nodes) * 2.0                            # some beyond +-3: clipped
        row = EC.row(name, *hw)
        got = mgunet.elastic_control(n, sigma, row, nodes)
        assert got.dtype == torch.int32 and tuple(got.shape) == (2,) + nodes
        cx, cy = EO.control(n, sigma, row)
        assert got[0].tolist() == cx and got[1].tolist() == cy, (nodes, name)
    assert bool((np.abs(n) > 3).any())
    # the identity row carries output pixels over unchanged: c = FIX16(sigma n); a flip negates x
    n = np.zeros((2, 4, 4))
    n[0, 1, 2], n[1, 3, 0] = 1.0, -3.5
    c = mgunet.elastic_control(n, 2.0, AC_IDENT, (4, 4))
    assert int(c[0, 1, 2]) == 2 << 16 and int(c[1, 3, 0]) == -(6 << 16) and int(c.abs().sum()) == 8 << 16
    flipped = (-65536,) + AC_IDENT[1:]
    assert int(mgunet.elastic_control(n, 2.0, flipped, (4, 4))[0, 1, 2]) == -(2 << 16)



def test_elastic_control_refusals():
    n = np.zeros((2, 4, 4))
    with pytest.raises(ValueError, match="nodes"):
        mgunet.elastic_control(np.zeros((2, 3, 4)), 1.0, AC_IDENT, (3, 4))
    with pytest.raises(ValueError, match="normals"):
        mgunet.elastic_control(np.zeros((2, 4, 5)), 1.0, AC_IDENT, (4, 4))
    n[0, 0, 0] = 3.0
    assert int(mgunet.elastic_control(n, 1024.0 / 3.0, AC_IDENT, (4, 4))[0, 0, 0]) == 1 << 26      # the limit itself passes
    with pytest.raises(ValueError, match="2\\^26"):
        mgunet.elastic_control(n, 342.0, AC_IDENT, (4, 4))


def test_draw_consumes_the_documented_draws():
    src = (45, 61)
    aug = mgunet.RandomElasticAffineColor((40, 52), nodes=(5, 7), sigma=4.0, degrees=20)
    g, h = torch.Generator().manual_seed(17), torch.Generator().manual_seed(17)
    params, ctrl = aug.draw(3, src, generator=g)
    assert params.dtype == torch.int32 and tuple(params.shape) == (3, 16) and ctrl.dtype == torch.int32 and tuple(ctrl.shape) == (3, 2, 5, 7)
    for b in range(3):                                                          # per image: rand(10), then randn(2 gh gw)
        r = torch.rand(10, dtype=torch.float64, generator=h)
        n = torch.randn(2 * 5 * 7, dtype=torch.float64, generator=h).reshape(2, 5, 7)
        assert tuple(params[b].tolist()) == aug.row(r.tolist(), src)
        cx, cy = EO.control(n.numpy(), 4.0, params[b].tolist())
        assert ctrl[b, 0].tolist() == cx and ctrl[b, 1].tolist() == cy
    assert torch.equal(torch.rand(3, generator=g), torch.rand(3, generator=h))                     # nothing more was drawn
    assert len({tuple(c.reshape(-1).tolist()) for c in ctrl}) == 3 and bool((ctrl != 0).any())
    # sigma = 0: no normals; the ten draws per image give the parent's rows
    flat = mgunet.RandomElasticAffineColor((40, 52), nodes=(5, 7), sigma=0.0, degrees=20)
    parent = mgunet.RandomAffineColor((40, 52), degrees=20)
    g, h = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    params, ctrl = flat.draw(3, src, generator=g)
    assert torch.equal(params, parent.draw(3, src, generator=h)) and tuple(ctrl.shape) == (3, 2, 5, 7) and not bool(ctrl.any())
    assert torch.equal(torch.rand(3, generator=g), torch.rand(3, generator=h))


# ---- the oracle's identities ---------------------------------------------------------------------------------------------------------
def affine_reference(img, masks, table, c, out_hw):
    return AO.augment(img, table, out_hw, EC.MEAN, EC.STD, masks=masks, fill=EC.FILL, mask_fill=EC.MASK_FILL, num_classes=c["num_classes"],
                      bgr=c["bgr"])


@pytest.mark.parametrize("shape", list(EC.SHAPES))
def test_zero_control_is_the_affine_oracle_bitwise(shape):
    for tag in (f"{shape}/zero", f"{shape}/batch"):
        img, masks, labels, table, ctrl, c = EC.inputs(tag)
        out_hw = EC.SHAPES[shape][1]
        want, wbytes, _, wmask = affine_reference(img, masks, table, c, out_hw)
        for z in (np.zeros_like(ctrl), None):
            out, byts, ms, ls = EO.augment(img, table, z, out_hw, EC.MEAN, EC.STD, masks=masks, labels=labels, fill=EC.FILL, mask_fill=EC.MASK_FILL,
                                           label_fill=EC.LABEL_FILL, num_classes=c["num_classes"], bgr=c["bgr"])
            assert np.array_equal(out.view(np.int32), want.view(np.int32)) and np.array_equal(byts, wbytes) and np.array_equal(ms, wmask)
            # labels: the nearest sample of the affine oracle, unclipped
            for b in range(len(img)):
                wl = AO.sample_mask(labels[b], table[b].tolist(), out_hw, EC.LABEL_FILL, 0)
                assert np.array_equal(ls[b], wl)


@pytest.mark.parametrize("shape", list(EC.SHAPES))
def test_constant_control_is_the_affine_oracle_at_shifted_offsets(shape):
    tag = f"{shape}/const"
    img, masks, labels, table, ctrl, c = EC.inputs(tag)
    out_hw = EC.SHAPES[shape][1]
    f = EC.reference(tag)[4]
    assert (f[:, 0] == EC.CONST[0]).all() and (f[:, 1] == EC.CONST[1]).all()      # a constant field is reproduced exactly
    shifted = table.copy()
    shifted[:, 2] += EC.CONST[0]
    shifted[:, 5] += EC.CONST[1]
    want, _, _, wmask = affine_reference(img, masks, shifted, c, out_hw)
    got = EC.reference(tag)
    assert np.array_equal(got[0].view(np.int32), want.view(np.int32)) and np.array_equal(got[2], wmask)
    plain = affine_reference(img, masks, table, c, out_hw)[0]
    assert not np.array_equal(plain.view(np.int32), want.view(np.int32))         # and the shift is seen


@pytest.mark.parametrize("tag", ["5x7/seeded", "9x11/spike", "40x24/seeded", "16x16/spike"])
def test_factored_field_equals_the_double_sum_of_the_definition(tag):
    ctrl = EC.inputs(tag)[4]
    out_hw = EC.SHAPES[EC.CASES[tag]["shape"]][1]
    dx, dy = EO.field_direct(ctrl[0], out_hw)
    f = EC.reference(tag)[4]
    assert np.array_equal(f[0, 0], dx) and np.array_equal(f[0, 1], dy)
    assert np.abs(f).max() <= EO.CTRL_LIMIT


# ---- wrong variants, coverage -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", EO.VARIANTS)
def test_the_cases_tell_each_wrong_variant_from_the_definition(variant):
    differing = [tag for tag in EC.CASES
                 if any(not np.array_equal(a, b) for a, b in zip(EC.reference(tag), EC.reference(tag, variant)))]
    assert differing, variant


def test_every_variant_is_named_once_and_the_definition_is_not_one():
    assert len(set(EO.VARIANTS)) == len(EO.VARIANTS) == 13 and None not in EO.VARIANTS


@pytest.mark.parametrize("tag", EC.SEEDED)
def test_seeded_cases_bend_the_image_inside_the_source(tag):
    img, _, _, table, ctrl, c = EC.inputs(tag)
    out_hw = EC.SHAPES[c["shape"]][1]
    n = out_hw[0] * out_hw[1]
    f = EC.reference(tag)[4][0]
    assert ((f[0] != 0) | (f[1] != 0)).sum() * 4 >= 3 * n                        # the field is there
    ax, ay = AO.coordinates(table[0].tolist(), out_hw)
    sx, sy = EO.coordinates(table[0].tolist(), ctrl[0], out_hw)
    moved = ((sx >> 16) != (ax >> 16)) | ((sy >> 16) != (ay >> 16))
    assert moved.sum() * 4 >= n, (tag, moved.mean())                             # another source pixel than the affine map alone reads
    inside = EO.interior(img.shape[1:3], sx, sy)
    assert inside.sum() * 2 >= n, (tag, inside.mean())                           # and not only fill


@pytest.mark.parametrize("tag", EC.SPIKE)
def test_spike_cases_leave_the_source(tag):
    img, _, _, table, ctrl, c = EC.inputs(tag)
    out_hw = EC.SHAPES[c["shape"]][1]
    assert np.abs(ctrl).max() == EO.CTRL_LIMIT and ctrl.min() == -EO.CTRL_LIMIT
    sx, sy = EO.coordinates(table[0].tolist(), ctrl[0], out_hw)
    outside = ~EO.interior(img.shape[1:3], sx, sy)
    assert outside.sum() * 10 >= out_hw[0] * out_hw[1], (tag, outside.mean())
    f = EC.reference(tag)[4]
    assert f.min() < -(1 << 24) and f.max() > (1 << 24)                          # large displacements of both signs reach the pixels


def test_labels_in_the_cases_carry_ids_no_float_or_clip_would_keep():
    for tag in EC.CASES:
        ls = EC.reference(tag)[3]
        assert ls.dtype == np.int32
    ls = np.concatenate([EC.reference(t)[3].reshape(-1) for t in EC.CASES])
    assert (ls > (1 << 24)).any() and (ls < 0).any() and (ls == EC.LABEL_FILL).any() and (ls == (1 << 30) + 7).any()
