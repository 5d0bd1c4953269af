"""mgu_unet_backward as a network, against float64 with the forward's decisions pinned (tests/train_net_oracle.py: why, and the bars).

The whole-step tests of test_gpu_train.py hold the network gradient to 2e-2 of a norm, because a float64 reference that makes its own
ReLU and arg-max decisions is that far from any fp32 path.  Here the reference takes the decisions of the HIP forward itself -- read
through the test hooks mgu_unet_train_record_dims / mgu_unet_train_record_copy -- and every parameter gradient is held to
max(2e-5, 4 x the error of two CPU fp32 emulations) of its tensor's maximum.  That reaches what only the network contains: the backward
schedule of csrc/mgunet_train.hip, the routing of the d(cat) halves, the pad region of odd levels, the up-convolution bias sums, the
pool backward accumulating into the skip gradient, the head's padded column sum, the kernel picks at a network's widths, and the
scratch regions against the forward record.

Every (case, size) of train_net_oracle.CASES x sizes runs one fresh model with formula weights and one train-mode forward, then checks
  1. the forward record: z against the float64 convolution of the recorded input per element, mean / invstd against float64 statistics
     of the recorded z, the recorded tensors against the tensors the model returned and against each other bit for bit, zero pad rows
     and columns in every concat's upper half;
  2. the decisions against the float64 network's own, within the project's margins for a ReLU at its kink and a pool window near a tie;
  3. one mgu_unet_backward on dense dlogits into a NaN-prefilled flat gradient: every element finite;
  4. every parameter gradient against the pinned float64 network;
  5. the profiling records against the host restatement of the picks (train_net_oracle.backward_launches);
  6. the record after the backward, bit for bit, and a second backward returning the same bytes;
  7. the ReLU mask the BatchNorm backward recomputes from z against the forward's y > 0, as exact per-channel counts of live elements
     (backward_mask_counts: the pinned gradients would not show a single element the two kernels decide differently).

Figures of one MI355X run: NOTES.md, "Training step, network gradients pinned"."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import mgunet
import mgunet_oracle as O
import test_gpu_backward_kernels as K
import train_net_oracle as T
from mgunet import _lib

pytestmark = pytest.mark.gpu

MATRIX = [(case, size) for case in T.CASES for size in T.sizes(case)]
FIELDS = ("in", "z", "y", "mean", "invstd")
LAUNCHED = {}            # (case, size) -> profiling records of its backward, for the collecting test


def train_model(case, p, cuda, monkeypatch):
    """A fresh train-mode model whose context was created under the case's switches."""
    cfg, sw = T.CASES[case]
    for k in T.SWITCH_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in sw.items():
        monkeypatch.setenv(k, v)
    m = mgunet.UNet(*cfg)
    m.load_state_dict(p)
    m = m.to(cuda).train()
    m._context(cuda)
    for k in sw:
        monkeypatch.delenv(k)
    return m


def record_dims(ctx, layer):
    v = [C.c_int() for _ in range(5)]
    _lib.check(_lib.lib().mgu_unet_train_record_dims(ctx.handle, layer.encode(), *[C.byref(i) for i in v]), ctx.handle)
    return tuple(i.value for i in v)                             # B, H, W, Cin, Cout


def copy_record(ctx, cuda, depth):
    """{layer: {in, z, y (B, H, W, C) NHWC dense, mean, invstd (C)}} of the context's last train-mode forward, on the device; the
    up-convolutions and the head: {in}.  Prefilled with NaN: the hook writes every element."""
    nan = lambda *s: torch.full(s, float("nan"), device=cuda)
    rec = {}
    for layer in T.bn_layers(depth) + T.other_layers(depth):
        B, H, W, cin, cout = record_dims(ctx, layer)
        r = {"in": nan(B, H, W, cin)}
        if layer in T.bn_layers(depth):
            r.update(z=nan(B, H, W, cout), y=nan(B, H, W, cout), mean=nan(cout), invstd=nan(cout))
        _lib.call("mgu_unet_train_record_copy", cuda, layer.encode(), *[r.get(f) for f in FIELDS], ctx=ctx)
        rec[layer] = r
    torch.cuda.synchronize(cuda)
    return rec


def to_host(rec):
    """The record as the oracle reads it: NCHW views on the CPU."""
    return {layer: {f: (t.cpu().permute(0, 3, 1, 2) if t.dim() == 4 else t.cpu()) for f, t in r.items()} for layer, r in rec.items()}


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_record_links(rec, x, sk, ft, cats, depth):
    """Bit for bit: every recorded tensor that the model also returned, or that another layer recorded, is that tensor."""
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    bad = []

    def same(what, a, b):
        if not same_bytes(a, b):
            bad.append(what)

    enc = [f"encoder.encoder_blocks.{i}." for i in range(depth)]
    dec = [f"decoder.decoder_blocks.{b}." for b in range(depth)]
    same("input of the first convolution", rec[enc[0] + "conv1"]["in"], nhwc(x))
    for pre in T.block_prefixes(depth):
        same(pre + "conv2 reads conv1's y", rec[pre + "conv2"]["in"], rec[pre + "conv1"]["y"])
    for i in range(depth):
        same(f"skip {i}", rec[enc[i] + "conv2"]["y"], nhwc(sk[i]))
        nxt = enc[i + 1] if i + 1 < depth else "encoder.bottleneck."
        same(f"pooled {i}", rec[nxt + "conv1"]["in"], nhwc(F.max_pool2d(sk[i], 2)))
    for b in range(depth):
        lvl = depth - 1 - b
        below = rec["encoder.bottleneck.conv2"]["y"] if b == 0 else rec[dec[b - 1] + "conv_block.conv2"]["y"]
        same(f"input of up-convolution {b}", rec[dec[b] + "upsample"]["in"], below)
        same(f"concat {lvl}", rec[dec[b] + "conv_block.conv1"]["in"], cats[lvl])
        same(f"feat {lvl}", rec[dec[b] + "conv_block.conv2"]["y"], nhwc(ft[lvl]))
        Cc = cats[lvl].shape[3] // 2
        h, w = 2 * (cats[lvl].shape[1] // 2), 2 * (cats[lvl].shape[2] // 2)
        up = rec[dec[b] + "conv_block.conv1"]["in"][..., Cc:]
        if bool(up[:, h:].ne(0).any()) or bool(up[:, :, w:].ne(0).any()):
            bad.append(f"concat {lvl}: a pad row / column of the upper half is not zero")
    same("input of the head", rec["decoder.final_conv"]["in"], nhwc(ft[0]))
    return bad


def backward(ctx, cuda, dlogits, nparams, profile):
    """One mgu_unet_backward, as test_gpu_train.backward_as_trainer issues it, into a NaN-prefilled flat gradient."""
    grad = torch.full((nparams,), float("nan"), device=cuda)
    L, launched = _lib.lib(), None
    if profile:
        _lib.check(L.mgu_profile_enable(ctx.handle, 1), ctx.handle)
    _lib.call("mgu_unet_backward", cuda, dlogits, grad, ctx=ctx)
    torch.cuda.synchronize(cuda)
    if profile:
        launched = {k["name"]: k["launches"] for k in _lib.read_kernel_stats(ctx)}
        _lib.check(L.mgu_profile_enable(ctx.handle, 0), ctx.handle)
    return grad, launched


def backward_mask_counts(cuda, m, rec, depth):
    """{layer: (live elements per channel of the ReLU mask the BatchNorm backward recomputes, of the forward's y > 0)}.  The backward
    never reads y: chan_reduce_kernel<1> recomputes the sign from z and the forward's scale / shift, and agrees with the forward's
    fmaxf only if both kernels round that expression alike.  mgu_bn_relu_backward_nhwc runs that kernel on the recorded z, mean and
    invstd (its scale / shift are formed from them by the expressions of bn_finalize_kernel); with dy = 1 its dbeta is the number of
    live elements of every channel, an integer below 2^24 and so exact.  One element that the two kernels decide differently shows,
    unless a second one of the same channel goes the other way."""
    out, L, s = {}, _lib.lib(), _lib.current_stream_ptr(cuda)
    sd = dict(m.named_parameters())
    with K.context(cuda) as c2:
        for layer in T.bn_layers(depth):
            r = rec[layer]
            B, H, W, Cc = r["z"].shape
            M = B * H * W
            ones = torch.ones((M, Cc), device=cuda)
            dz = torch.empty((M, Cc), device=cuda)
            dgamma, dbeta, dbias = (torch.full((Cc,), float("nan"), device=cuda) for _ in range(3))
            gamma, beta = sd[T.bn_of(layer) + ".weight"].detach(), sd[T.bn_of(layer) + ".bias"].detach()
            _lib.check(L.mgu_bn_relu_backward_nhwc(c2.handle, ones.data_ptr(), Cc, r["z"].data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                                   r["mean"].data_ptr(), r["invstd"].data_ptr(), M, Cc, dz.data_ptr(), dgamma.data_ptr(),
                                                   dbeta.data_ptr(), dbias.data_ptr(), s), c2.handle)
            out[layer] = (dbeta.double().cpu(), (r["y"] > 0).sum((0, 1, 2)).double().cpu())
    return out


def split_flat(ctx, flat, named):
    """{name: gradient} from the flat vector at the offsets mgu_unet_param_offset gives."""
    out = {}
    for name, prm in named:
        off = int(_lib.lib().mgu_unet_param_offset(ctx.handle, name.encode()))
        assert off >= 0, name
        out[name] = flat[off:off + prm.numel()].reshape(prm.shape)
    assert sum(v.numel() for v in out.values()) == flat.numel()
    return out


@pytest.mark.parametrize("case,size", MATRIX)
def test_network_gradients_against_pinned_float64(cuda, monkeypatch, case, size):
    assert T.TOL == K.TOL
    cfg, sw = T.CASES[case]
    depth, shape, tag = cfg[3], T.sizes(case)[size], f"{case} {size}"
    p = O.make_unet_params(*cfg, seed=21)
    p64 = T.f64_params(p)
    x = torch.from_numpy(O.formula_normal(f"trainnet/{case}/x", shape, seed=21))
    m = train_model(case, p, cuda, monkeypatch)
    ctx = m._context(cuda)
    with torch.no_grad():
        lg, sk, ft = m(x.to(cuda))
    torch.cuda.synchronize(cuda)
    cats = m._train_outputs[1]
    problems = []

    # 1. the forward record
    rec = copy_record(ctx, cuda, depth)
    assert all(bool(torch.isfinite(t).all()) for r in rec.values() for t in r.values()), (tag, "the hook left an element unwritten")
    problems += check_record_links(rec, x.to(cuda), sk, ft, cats, depth)
    host = to_host(rec)
    rr = T.record_ratios(p64, host, depth)
    worst = max(rr, key=lambda k: rr[k] if rr[k] == rr[k] else float("inf"))
    print(f"    [{tag}] forward record: worst error / bar {rr[worst]:.3f} on {worst}")
    problems += [f"forward record: {k} at {v:.3f} of its bar" for k, v in rr.items() if not v <= 1.0]

    # 2. the decisions
    pins = T.pins_from(host, depth)
    total, differing, outside = T.compare_decisions(pins, T.free_decisions(p64, x, depth))
    print(f"    [{tag}] decisions {total}, differing from float64's {differing} (share {differing / total:.1e}), outside the margins {outside}")
    if outside:
        problems.append(f"decisions differ from float64's outside the margins: {outside}")
    if not differing / total <= T.DIFFER_CAP:
        problems.append(f"share of differing decisions {differing / total:.2e} > {T.DIFFER_CAP}")

    # 3. the backward
    dl_dev, dl = T.formula_dlogits(f"trainnet/{case}", shape, cfg[1])
    nparams = int(_lib.lib().mgu_unet_param_count(ctx.handle))
    flat, launched = backward(ctx, cuda, dl_dev.to(cuda), nparams, profile=True)
    assert bool(torch.isfinite(flat).all()), (tag, f"{int((~torch.isfinite(flat)).sum())} gradient elements are not finite")

    # 4. the gradients
    g = {k: v.cpu() for k, v in split_flat(ctx, flat, list(m.named_parameters())).items()}
    ref, dz, bar, emu = T.reference(p, x, dl, depth, pins)
    assert list(g) == list(ref)
    ratio = T.judge(g, ref, dz, bar, tag)
    problems += [f"gradient {k}: {ratio[k]:.3f} of its bar ({bar.get(k, T.BIAS_BOUND):.2e}; emulations " +
                 ", ".join(f"{e.get(k, float('nan')):.2e}" for e in emu.values()) + ")" for k in T.misses(ratio)]

    # 5. the launches
    want = T.backward_launches(cfg, shape, sw)
    LAUNCHED[(case, size)] = launched
    print(f"    [{tag}] launched {launched}")
    if launched != want:
        problems.append(f"launched {launched}, predicted {want}")

    # 6. the record survives
    after = copy_record(ctx, cuda, depth)
    problems += [f"{layer} {f} changed under the backward" for layer, r in rec.items() for f, t in r.items() if not same_bytes(t, after[layer][f])]
    again, _ = backward(ctx, cuda, dl_dev.to(cuda), nparams, profile=False)
    if not same_bytes(flat, again):
        problems.append("a second backward on the same record returns other bytes")

    # 7. the mask the backward recomputes is the forward's y > 0
    counts = backward_mask_counts(cuda, m, rec, depth)
    off = {layer: int((a - b).abs().sum()) for layer, (a, b) in counts.items() if not torch.equal(a, b)}
    print(f"    [{tag}] live elements, recomputed mask against y > 0: {int(sum(b.sum() for _, b in counts.values()))} in all, "
          f"channel counts that differ {off}")
    problems += [f"{layer}: the backward's recomputed ReLU mask and the forward's y > 0 differ by {n} in the channel counts" for layer, n in off.items()]
    assert not problems, (tag, problems)


def test_every_backward_kernel_family_is_launched_somewhere_in_the_matrix(cuda):
    """Every weight-gradient and data-gradient family occurs at least once: in the launches the restatement derives over the matrix,
    and -- every test above having held its profiling records to that restatement -- in the records of the (case, size) that ran in
    this session (all of them in a run of the whole file)."""
    derived = {(case, size): T.backward_launches(T.CASES[case][0], T.sizes(case)[size], T.CASES[case][1]) for case, size in MATRIX}
    for key, launched in LAUNCHED.items():
        assert launched == derived[key], key
    families = {T.WGRAD_THIN, T.WGRAD_WINO_X3, T.WGRAD_WINO, T.WGRAD_DIRECT, T.DGRAD_TILES, T.CONVT_DGRAD_X3, T.CONVT_DGRAD_TILES}
    for source in [derived] + ([LAUNCHED] if set(LAUNCHED) == set(MATRIX) else []):
        seen = set().union(*[set(v) for v in source.values()])
        assert families <= seen, families - seen
        assert seen & set(T.DGRAD_WINO), "no Winograd data gradient"
    print(f"    launches checked against the profiling records of {len(LAUNCHED)} of {len(MATRIX)} (case, size)")


def test_record_hook_error_returns(cuda, monkeypatch):
    cfg = (3, 2, 8, 2)
    L = _lib.lib()
    for k in T.SWITCH_NAMES:
        monkeypatch.delenv(k, raising=False)
    m = mgunet.UNet(*cfg)
    m.load_state_dict(O.make_unet_params(*cfg, seed=21))
    m = m.to(cuda).eval()
    ctx = m._context(cuda)
    s = _lib.current_stream_ptr(cuda)
    first, up, head = T.bn_layers(2)[0].encode(), T.other_layers(2)[0].encode(), b"decoder.final_conv"
    v = [C.c_int() for _ in range(5)]
    t = torch.zeros(2 * 16 * 16 * 64, device=cuda)
    dims = lambda name: L.mgu_unet_train_record_dims(ctx.handle, name, *[C.byref(i) for i in v])
    copy = lambda name, *ptrs: L.mgu_unet_train_record_copy(ctx.handle, name, *ptrs, s)
    IN, NO = t.data_ptr(), None
    assert dims(first) == _lib.MGU_ERR_STATE and copy(first, IN, NO, NO, NO, NO) == _lib.MGU_ERR_STATE          # before any forward
    x = torch.from_numpy(O.formula_normal("trainnet/hook/x", (2, 3, 16, 16), seed=21)).to(cuda)
    with torch.no_grad():
        m(x)
    assert dims(first) == _lib.MGU_ERR_STATE and copy(first, IN, NO, NO, NO, NO) == _lib.MGU_ERR_STATE          # an eval forward records nothing
    with torch.no_grad():
        m.train()(x)
    assert dims(first) == _lib.MGU_OK and tuple(i.value for i in v) == (2, 16, 16, 3, 8)
    assert dims(up) == _lib.MGU_OK and tuple(i.value for i in v) == (2, 4, 4, 32, 16)                            # a ConvTranspose's input grid
    assert dims(head) == _lib.MGU_OK and tuple(i.value for i in v) == (2, 16, 16, 8, 2)
    assert dims(b"encoder.encoder_blocks.2.conv1") == _lib.MGU_ERR_INVALID and dims(b"encoder.encoder_blocks.0.bn1") == _lib.MGU_ERR_INVALID
    assert dims(None) == _lib.MGU_ERR_INVALID and copy(None, IN, NO, NO, NO, NO) == _lib.MGU_ERR_INVALID
    assert copy(b"encoder.encoder_blocks.0", IN, NO, NO, NO, NO) == _lib.MGU_ERR_INVALID
    for name in (up, head):
        assert copy(name, IN, NO, NO, NO, NO) == _lib.MGU_OK
        for k in range(1, 5):                                    # z / y / mean / invstd of a layer without a BatchNorm
            ptrs = [NO] * 5
            ptrs[k] = IN
            assert copy(name, *ptrs) == _lib.MGU_ERR_INVALID, (name, FIELDS[k])
    assert copy(first, NO, NO, NO, NO, NO) == _lib.MGU_OK                                                        # nothing asked, nothing done
    torch.cuda.synchronize(cuda)
