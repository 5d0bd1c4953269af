"""The elastic deformation kernels (csrc/augment_elastic.hip) on the GPU against the numpy oracle (tests/augment_elastic_oracle.py) on the
shared cases (tests/augment_elastic_cases.py): the field exact, images BITWISE (compared as int32 views), masks and labels exact, on
NCHW / NHWC-strided / misaligned outputs; zero, absent and constant control against mgu_augment_affine_color itself; labels beyond
2^24 and below zero; the launch counts; run-to-run equality; RandomElasticAffineColor under a seeded generator; the refusals; and one
Trainer.train_step with the warped instance map."""
import numpy as np
import pytest
import torch

import mgunet
import mgunet_oracle as O
import augment_elastic_cases as EC
import augment_elastic_oracle as EO
from mgunet import _lib

pytestmark = pytest.mark.gpu
LAYOUTS = ("nchw", "nhwc", "misaligned")


def stage(c, out_hw, cls=None, **kw):
    return (cls or mgunet.RandomElasticAffineColor)(out_hw, mean=EC.MEAN, std=EC.STD, fill=EC.FILL, mask_fill=EC.MASK_FILL,
                                                    num_classes=c["num_classes"], bgr=c["bgr"], **kw)


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32)


def make_out(cuda, layout, B, H, W):
    """-> (the (B, 3, H, W) view the stage writes, the tensor that owns its memory)"""
    if layout == "nchw":
        o = torch.full((B, 3, H, W), float("nan"), device=cuda)
        return o, o
    if layout == "nhwc":
        o = torch.full((B, H, W, 3), float("nan"), device=cuda)
        return o.permute(0, 3, 1, 2), o
    o = torch.full((B, 3, H, W + 5), 777.0, device=cuda)      # rows start 4 bytes off a 16-byte boundary, pitch W + 5
    return o[..., 1:W + 1], o


def run_case(cuda, tag, layout="nchw", ctrl="case", table=None):
    """-> (images, masks, labels, owner of the images' memory); ctrl: "case" (the case's field), None or an int array"""
    img, masks, labels, tab, cc, c = EC.inputs(tag)
    out_hw = EC.SHAPES[c["shape"]][1]
    view, owner = make_out(cuda, layout, len(img), *out_hw)
    ctrl = cc if isinstance(ctrl, str) else ctrl
    r = stage(c, out_hw, label_fill=EC.LABEL_FILL)(torch.from_numpy(img).to(cuda), torch.from_numpy(masks).to(cuda), torch.from_numpy(labels).to(cuda),
                                                   out=view, params=i32(tab if table is None else table), ctrl=None if ctrl is None else i32(ctrl))
    return r + (owner,)


def run_affine(cuda, tag, table=None):
    img, masks, _, tab, _, c = EC.inputs(tag)
    out_hw = EC.SHAPES[c["shape"]][1]
    return stage(c, out_hw, cls=mgunet.RandomAffineColor)(torch.from_numpy(img).to(cuda), torch.from_numpy(masks).to(cuda),
                                                          params=i32(tab if table is None else table))


@pytest.mark.parametrize("tag", list(EC.CASES))
def test_field_exact(cuda, tag):
    ctrl, c = EC.inputs(tag)[4:]
    got = mgunet.elastic_field(i32(ctrl).to(cuda), EC.SHAPES[c["shape"]][1])
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy().astype(np.int64), EC.reference(tag)[4]), tag


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("tag", list(EC.CASES))
def test_images_bitwise_masks_and_labels_exact(cuda, tag, layout):
    want, _, wmask, wlab, _ = EC.reference(tag)
    out, ms, ls, owner = run_case(cuda, tag, layout)
    assert out.dtype == torch.float32 and ms.dtype == torch.int64 and ls.dtype == torch.int32
    assert np.array_equal(ls.cpu().numpy(), wlab), (tag, layout)
    assert np.array_equal(ms.cpu().numpy(), wmask), (tag, layout)
    assert np.array_equal(bits(out), want.view(np.int32)), (tag, layout)
    if layout == "misaligned":                                  # nothing beside the view is written
        W = out.shape[3]
        assert bool((owner[..., 0] == 777.0).all()) and bool((owner[..., W + 1:] == 777.0).all())


@pytest.mark.parametrize("shape", list(EC.SHAPES))
def test_zero_and_absent_control_equal_the_affine_entry(cuda, shape):
    tag = f"{shape}/batch"
    want, wmask = run_affine(cuda, tag)
    img, _, labels, tab, ctrl, _ = EC.inputs(tag)
    wlab = EO.augment(img, tab, None, EC.SHAPES[shape][1], EC.MEAN, EC.STD, labels=labels, label_fill=EC.LABEL_FILL)[3]
    for z in (np.zeros_like(ctrl), None):
        out, ms, ls, _ = run_case(cuda, tag, ctrl=z)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)) and torch.equal(ms, wmask), (shape, z is None)
        assert np.array_equal(ls.cpu().numpy(), wlab), (shape, z is None)


@pytest.mark.parametrize("shape", list(EC.SHAPES))
def test_constant_control_equals_the_affine_entry_at_shifted_offsets(cuda, shape):
    tag = f"{shape}/const"
    shifted = EC.inputs(tag)[3].copy()
    shifted[:, 2] += EC.CONST[0]
    shifted[:, 5] += EC.CONST[1]
    want, wmask = run_affine(cuda, tag, table=shifted)
    out, ms, _, _ = run_case(cuda, tag)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32)) and torch.equal(ms, wmask)
    assert not torch.equal(out.view(torch.int32), run_affine(cuda, tag)[0].view(torch.int32))


def test_labels_carry_large_and_negative_ids_and_the_fill(cuda):
    """every source id comes through as it is (no float on the way, no clip), and only label_fill is added"""
    for tag in ("24x40/seeded", "24x40/spike", "40x24/batch"):
        labels = EC.inputs(tag)[2]
        ls = run_case(cuda, tag)[2].cpu().numpy()
        assert np.array_equal(ls, EC.reference(tag)[3])
        assert set(np.unique(ls).tolist()) <= set(np.unique(labels).tolist()) | {EC.LABEL_FILL}
        assert (ls > (1 << 24)).any() and (ls < 0).any() and (ls == (1 << 30) + 7).any() and (ls == -(1 << 28)).any()
    assert (ls == EC.LABEL_FILL).any() and not (labels == EC.LABEL_FILL).any()


def test_images_only_and_labels_only(cuda):
    tag = "40x24/seeded"
    img, masks, labels, tab, ctrl, c = EC.inputs(tag)
    aug = stage(c, EC.SHAPES[c["shape"]][1], label_fill=EC.LABEL_FILL)
    want = EC.reference(tag)
    out = aug(torch.from_numpy(img).to(cuda), params=i32(tab), ctrl=i32(ctrl))
    assert isinstance(out, torch.Tensor) and np.array_equal(bits(out), want[0].view(np.int32))
    out, ls = aug(torch.from_numpy(img).to(cuda), labels=torch.from_numpy(labels).to(cuda), params=i32(tab), ctrl=i32(ctrl))
    assert np.array_equal(bits(out), want[0].view(np.int32)) and np.array_equal(ls.cpu().numpy(), want[3])


def count_launches(cuda, table, ctrl, hw=(9, 11), B=2, masks=True, labels=True, field=False):
    """as tests/test_gpu_augment_affine.py::count_launches: the context's launch records around one call"""
    rng = np.random.default_rng(1)
    img = torch.from_numpy(rng.integers(0, 256, (B,) + hw + (3,), dtype=np.uint8)).to(cuda)
    m = torch.from_numpy(rng.integers(0, 3, (B,) + hw, dtype=np.uint8)).to(cuda) if masks else None
    lab = torch.from_numpy(rng.integers(0, 9, (B,) + hw, dtype=np.int32)).to(cuda) if labels else None
    aug = mgunet.RandomElasticAffineColor((8, 12))
    ctx = _lib.context(cuda)
    _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        if field:
            mgunet.elastic_field(ctrl, (8, 12))
        else:
            aug(img, m, lab, params=table, ctrl=ctrl)
        torch.cuda.synchronize()
        stats = _lib.read_kernel_stats(ctx)
    finally:
        _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 0), ctx.handle)
    return {k["name"]: k["launches"] for k in stats}


def test_launch_counts(cuda):
    ident = torch.tensor([EC.AC.IDENT_ROW] * 2, dtype=torch.int32)
    with_k = ident.clone()
    with_k[1, 15] = -300
    ctrl = torch.full((2, 2, 6, 6), 70000, dtype=torch.int32)
    for masks, labels in ((True, True), (False, True), (True, False), (False, False)):
        assert count_launches(cuda, ident, ctrl, masks=masks, labels=labels) == {"augment elastic": 1}            # need_mean = 0: no luma kernel
        assert count_launches(cuda, with_k, ctrl, masks=masks, labels=labels) == {"augment luma": 1, "augment elastic": 1}
    assert count_launches(cuda, ident.to(cuda), ctrl.to(cuda)) == {"augment luma": 1, "augment elastic": 1}       # a device table is not inspected
    assert count_launches(cuda, with_k, None) == {"augment luma": 1, "augment elastic": 1}                        # labels without a field
    assert count_launches(cuda, None, ctrl.to(cuda), field=True) == {"elastic field": 1}


def test_two_runs_are_bitwise_equal(cuda):
    a = run_case(cuda, "24x40/batch")
    b = run_case(cuda, "24x40/batch")
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_seeded_generator_equals_the_oracle_on_its_own_draw(cuda):
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (3, 45, 61, 3), dtype=np.uint8)
    masks = rng.integers(0, 4, (3, 45, 61), dtype=np.uint8)
    labels = rng.integers(-5, 1 << 30, (3, 45, 61)).astype(np.int32)
    aug = mgunet.RandomElasticAffineColor((40, 52), nodes=(5, 7), sigma=6.0, label_fill=-1, num_classes=3, fill=(10, 200, 30))
    table, ctrl = aug.draw(3, (45, 61), generator=torch.Generator().manual_seed(21))
    assert len({tuple(r) for r in table.tolist()}) == 3 and bool((table[:, 15] != 0).any()) and bool((ctrl != 0).any())
    out, ms, ls = aug(torch.from_numpy(img).to(cuda), torch.from_numpy(masks).to(cuda), torch.from_numpy(labels).to(cuda),
                      generator=torch.Generator().manual_seed(21))
    want, _, wm, wl = EO.augment(img, table.numpy(), ctrl.numpy(), (40, 52), aug.mean, aug.std, masks=masks, labels=labels, fill=(10, 200, 30),
                                 mask_fill=-100, label_fill=-1, num_classes=3)
    assert np.array_equal(bits(out), want.view(np.int32)) and np.array_equal(ms.cpu().numpy(), wm) and np.array_equal(ls.cpu().numpy(), wl)
    assert tuple(out.shape) == (3, 3, 40, 52) and tuple(ms.shape) == (3, 40, 52) and tuple(ls.shape) == (3, 40, 52)
    plain = EO.augment(img, table.numpy(), None, (40, 52), aug.mean, aug.std)[0]
    assert not np.array_equal(plain.view(np.int32), want.view(np.int32))
    # sigma = 0 and no labels: the parent's call on the parent's draws
    flat = mgunet.RandomElasticAffineColor((40, 52), sigma=0.0, num_classes=3, fill=(10, 200, 30))
    parent = mgunet.RandomAffineColor((40, 52), num_classes=3, fill=(10, 200, 30))
    a = flat(torch.from_numpy(img).to(cuda), torch.from_numpy(masks).to(cuda), generator=torch.Generator().manual_seed(4))
    b = parent(torch.from_numpy(img).to(cuda), torch.from_numpy(masks).to(cuda), generator=torch.Generator().manual_seed(4))
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_bad_arguments_raise(cuda):
    aug = mgunet.RandomElasticAffineColor((8, 8))
    img = torch.zeros(2, 9, 9, 3, dtype=torch.uint8, device=cuda)
    ident = torch.tensor([EC.AC.IDENT_ROW] * 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="labels"):
        aug(img, labels=torch.zeros(2, 9, 9, dtype=torch.int64, device=cuda))
    with pytest.raises(ValueError, match="labels"):
        aug(img, labels=torch.zeros(2, 9, 8, dtype=torch.int32, device=cuda))
    with pytest.raises(ValueError, match="control nodes"):
        aug(img, params=ident, ctrl=torch.zeros(2, 2, 3, 6, dtype=torch.int32))
    with pytest.raises(ValueError, match="control nodes"):
        aug(img, params=ident, ctrl=torch.zeros(2, 2, 6, 33, dtype=torch.int32))
    with pytest.raises(ValueError, match="ctrl"):
        aug(img, params=ident, ctrl=torch.zeros(3, 2, 6, 6, dtype=torch.int32))
    with pytest.raises(ValueError, match="2\\^26"):
        aug(img, params=ident, ctrl=torch.full((2, 2, 6, 6), (1 << 26) + 1, dtype=torch.int32))
    # the library's own refusals, before any device work: the output keeps its bytes
    out = torch.full((2, 3, 8, 8), 5.0, device=cuda)
    lab = torch.zeros(2, 9, 9, dtype=torch.int32, device=cuda)
    lout = torch.zeros(2, 8, 8, dtype=torch.int32, device=cuda)
    ctrl = torch.zeros(2, 2, 6, 6, dtype=torch.int32, device=cuda)
    so, three, fill = (_lib.C.c_int64 * 4)(*out.stride()), (_lib.C.c_float * 3)(0.5, 0.5, 0.5), (_lib.C.c_uint8 * 3)(0, 0, 0)

    def entry(labels, labels_out, c, gh, gw):
        _lib.call("mgu_augment_elastic_color", cuda, img, 2, 9, 9, 0, None, 0, out, 8, 8, so, three, three, fill, None, -100, ident.to(cuda), 0,
                  labels, labels_out, 0, c, gh, gw)

    for args, message in (((None, None, ctrl, 3, 6), "control nodes"), ((None, None, ctrl, 6, 33), "control nodes"), ((lab, None, ctrl, 6, 6), "go together"),
                          ((None, lout, ctrl, 6, 6), "go together"), ((None, None, ctrl, 0, 6), "control nodes"), ((None, None, ctrl, 0, 0), "control nodes"),
                          ((None, None, None, 6, 6), "control nodes")):
        with pytest.raises(ValueError, match=message):
            entry(*args)
    with pytest.raises(ValueError, match="control nodes"):
        _lib.call("mgu_elastic_field", cuda, ctrl, 2, 6, 3, 8, 8, lout)
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    entry(lab, lout, ctrl, 6, 6)                                  # and the same call with good arguments runs
    torch.cuda.synchronize()
    assert not bool((out == 5.0).all())


def test_trainer_step_on_warped_batch_with_instances(cuda):
    cfg = (3, 2, 8, 2)
    rng = np.random.default_rng(2)
    img = torch.from_numpy(rng.integers(0, 256, (2, 80, 90, 3), dtype=np.uint8)).to(cuda)
    inst = np.zeros((2, 80, 90), np.int32)                         # two touching fruits and a third per image, ids of the dataset's own
    inst[:, 10:40, 10:45], inst[:, 10:40, 46:80], inst[:, 50:75, 30:60] = 1000001, 7, 42
    masks = torch.from_numpy((inst > 0).astype(np.uint8)).to(cuda)
    unet = mgunet.UNet(*cfg)
    unet.load_state_dict(O.make_unet_params(*cfg, seed=2))
    t = mgunet.Trainer(unet.to(cuda), lr=1e-3, border_w0=10.0)
    aug = mgunet.RandomElasticAffineColor((64, 64), scale=(0.9, 1.1), sigma=4.0, num_classes=2)
    x, y, ids = aug(img, masks, torch.from_numpy(inst).to(cuda), generator=torch.Generator().manual_seed(0))
    assert tuple(x.shape) == (2, 3, 64, 64) and ids.dtype == torch.int32 and tuple(ids.shape) == (2, 64, 64)
    assert {1000001, 7, 42} <= set(ids.unique().tolist()) <= {0, 1000001, 7, 42}
    assert torch.equal((ids > 0) & (y >= 0), y == 1)               # the instance map and the mask were bent alike
    loss = t.train_step(x, y, instances=ids)
    t.check()
    assert bool(torch.isfinite(loss).all())
