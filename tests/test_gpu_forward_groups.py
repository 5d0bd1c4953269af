"""The grouped eval forward (Tuning::fwd_groups, MGU_FWD_GROUPS=2; mgu_unet_forward in csrc/mgunet_api.hip): the batch walks the
network as two half-batch groups, group 0 on the caller's stream and group 1 on the context's side stream between a fork and a
join event.  The images are independent in eval mode and every kernel computes an image's pixels from that image alone, so the
split may not change a single bit.  The switch is read when a context is created: every arm below is a model of its own, built
with the variable set only around its construction.

What must hold, one-group context against two-group context:
  * logits, every skip, every decoder feature and the requested patch means are torch.equal -- no split (B = 1), an even split, an
    odd split with unequal slices of the shared conv1 temporary, several patches per workgroup, ragged sizes on the C++ fallback
    kernels with the odd-size concat memset in front of the fork, bf16 storage, and the node embeddings of the full model (the
    GAT on the caller's stream starts only after the join);
  * two forwards in a row without any synchronisation, each result cloned on the caller's stream right after its call, on the
    default and on another torch stream: a missing fork or join shows up as stale or torn data;
  * with profiling on the two-group context reports the kernel names and launch counts of the one-group context (it walks one
    group, so that the event pairs time kernels that do not wait for each other);
  * three back-to-back forwards at 4 x 64 x 64 still agree: the two groups are on different levels at the same time, so the
    shared conv1 temporary needs one fixed slice per group."""
import pytest
import torch

import mgunet
import mgunet_oracle as O
from mgunet import _lib

pytestmark = pytest.mark.gpu

CFG = (3, 2, 32, 4)
PATCH = 16
_ref = {}   # (B, H, W, dtype) -> the one-group context's result, computed once and left unchanged


def _unet(cuda, monkeypatch, groups, dtype=torch.float32):
    """a fresh eval model whose context was created under MGU_FWD_GROUPS=groups"""
    monkeypatch.setenv("MGU_FWD_GROUPS", str(groups))
    m = mgunet.UNet(*CFG, compute_dtype=dtype)
    m.load_state_dict(O.make_unet_params(*CFG, seed=3))
    m = m.to(cuda).eval()
    m._context(cuda)
    monkeypatch.delenv("MGU_FWD_GROUPS")
    return m


def _input(cuda, shape, tag="x"):
    B, H, W = shape
    return torch.from_numpy(O.formula_normal(f"forward_groups/{tag}", (B, 3, H, W), seed=H + W)).to(cuda)


def _run(m, x):
    """one forward with a patch-mean request -> [logits, skips..., decoder features..., patch means], cloned on the current stream"""
    B, _, H, W = x.shape
    pm = torch.full((B * ((H + PATCH - 1) // PATCH) * ((W + PATCH - 1) // PATCH), CFG[2]), float("nan"), device=x.device)
    _lib.call("mgu_unet_request_patch_mean", x.device, PATCH, pm, ctx=m._context(x.device))
    with torch.no_grad():
        lg, sk, ft = m(x)
    return [lg.clone()] + [t.clone() for t in sk] + [t.clone() for t in ft] + [pm]


def _reference(cuda, monkeypatch, shape, dtype=torch.float32, tag="x"):
    key = (shape, dtype, tag)
    if key not in _ref:
        _ref[key] = _run(_unet(cuda, monkeypatch, 1, dtype), _input(cuda, shape, tag))
        torch.cuda.synchronize(cuda)
    return _ref[key]


def _assert_equal(got, want, what):
    assert len(got) == len(want)
    for i, (u, v) in enumerate(zip(got, want)):
        assert torch.isfinite(u.float()).all(), f"{what}: tensor {i} is not finite"
        assert torch.equal(u, v), f"{what}: tensor {i} differs between one group and two"


@pytest.mark.parametrize("shape,dtype", [
    ((1, 32, 64), torch.float32),    # no split
    ((2, 32, 64), torch.float32),    # even split, one image each
    ((3, 32, 64), torch.float32),    # odd split: 2 + 1 images, unequal slices
    ((5, 32, 64), torch.float32),    # odd split: 3 + 2
    ((4, 48, 96), torch.float32),    # several patches per workgroup
    ((3, 20, 28), torch.float32),    # ragged: C++ fallback kernels, un-fused head, odd-size concat memset before the fork
    ((4, 32, 64), torch.bfloat16),   # bf16 kernel families, un-fused patch mean
])
def test_two_groups_equal_one_group(cuda, monkeypatch, shape, dtype):
    want = _reference(cuda, monkeypatch, shape, dtype)
    got = _run(_unet(cuda, monkeypatch, 2, dtype), _input(cuda, shape))
    torch.cuda.synchronize(cuda)
    _assert_equal(got, want, f"{shape} {dtype}")


def test_full_model_node_embeddings_equal(cuda, monkeypatch):
    x = _input(cuda, (4, 32, 64))
    outs = []
    for groups in (1, 2):
        gat = mgunet.GATNetwork(32, 128, 64, 4, 1)
        gat.load_state_dict(O.make_gat_params(32, 128, 64, 4, 1, seed=3))
        model = mgunet.MinGraphUNet(_unet(cuda, monkeypatch, groups), gat.to(cuda).eval(), PATCH).eval()
        with torch.no_grad():
            lg, sk, ft, emb = model(x)
        outs.append([lg.clone()] + [t.clone() for t in sk] + [t.clone() for t in ft] + [emb.clone()])
    torch.cuda.synchronize(cuda)
    _assert_equal(outs[1], outs[0], "MinGraphUNet 4 x 32 x 64")


@pytest.mark.parametrize("side_stream", [False, True])
def test_back_to_back_forwards_are_ordered(cuda, monkeypatch, side_stream):
    shape = (4, 32, 64)
    want1, want2 = _reference(cuda, monkeypatch, shape, tag="x"), _reference(cuda, monkeypatch, shape, tag="x2")
    x1, x2 = _input(cuda, shape, "x"), _input(cuda, shape, "x2")
    m = _unet(cuda, monkeypatch, 2)
    torch.cuda.synchronize(cuda)
    st = torch.cuda.Stream(cuda) if side_stream else torch.cuda.current_stream(cuda)
    with torch.cuda.stream(st):
        got1 = _run(m, x1)   # no synchronisation between the two calls: only the fork and the join order them
        got2 = _run(m, x2)
    st.synchronize()
    _assert_equal(got1, want1, "first of two forwards")
    _assert_equal(got2, want2, "second of two forwards")


def test_profiling_reports_the_one_group_schedule(cuda, monkeypatch):
    x = _input(cuda, (4, 32, 64))
    recs = []
    for groups in (1, 2):
        m = _unet(cuda, monkeypatch, groups)
        ctx, L = m._context(cuda), _lib.lib()
        _run(m, x)   # first call: weight folding and lazily built forms are not part of a step
        _lib.check(L.mgu_profile_enable(ctx.handle, 1), ctx.handle)
        got = _run(m, x)
        torch.cuda.synchronize(cuda)
        recs.append(sorted((k["name"], k["launches"]) for k in _lib.read_kernel_stats(ctx)))
        _lib.check(L.mgu_profile_enable(ctx.handle, 0), ctx.handle)
        _assert_equal(got, _reference(cuda, monkeypatch, (4, 32, 64)), f"profiled forward, {groups} group(s)")
    assert recs[0] and recs[0] == recs[1], recs


def test_shared_temporary_is_sliced_per_group(cuda, monkeypatch):
    shape = (4, 64, 64)
    want = _reference(cuda, monkeypatch, shape)
    x = _input(cuda, shape)
    m = _unet(cuda, monkeypatch, 2)
    runs = [_run(m, x) for _ in range(3)]   # back to back: group 1 of one forward also runs beside group 0 of the next level
    torch.cuda.synchronize(cuda)
    for r, got in enumerate(runs):
        _assert_equal(got, want, f"forward {r} of three")
