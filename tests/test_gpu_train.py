"""Training-step parity (SURVEY 8a row L1 / BASELINE config 5) on the HIP path against the golden step
record generated from the reference (torch autograd + torch.optim.Adam on the reference UNet) and against
the oracle on ragged shapes.  Tolerances: loss <= 1e-4 relative, gradient norms <= 1e-3
relative, parameters after one Adam step <= 2e-5 absolute (|step| ~ lr = 1e-3), BN running stats <= 1e-5.

These references make their own ReLU and arg-max decisions, which is why the gradient bars here are loose (see check_against and
test_c5_*).  The network gradient is held tightly in test_gpu_train_net.py, against a float64 network that takes the decisions of the
HIP forward itself; the isolated kernels in test_gpu_backward_kernels.py."""
import os

import numpy as np
import pytest
import torch

import mgunet
import mgunet_oracle as O

pytestmark = pytest.mark.gpu


def pool_margin(p, x, depth):
    """Smallest gap between the two largest values of any 2x2 max-pool window with a positive maximum (fp64 oracle
    forward, train-mode BN).  MaxPool backward routes the whole gradient to the arg-max: where the top two are within
    rounding distance, ANY change of summation order (mkldnn vs MFMA tiles vs Winograd) may route it to the other pixel,
    which moves one gradient element -- up to ~20 % of a channel's gradient on these tiny shapes.  Such inputs do not
    test the kernels, so the cases below take the first seed whose forward is clear of near-ties."""
    q = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in p.items()}
    _, skips, _ = O.unet_forward(q, x.double(), depth, training=True, new_stats={})
    gap = float("inf")
    for sk in skips:
        B, C, H, W = sk.shape
        w = sk[:, :, : H // 2 * 2, : W // 2 * 2].reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
        top = w.topk(2, dim=-1).values
        live = top[..., 0] > 0
        if bool(live.any()):
            gap = min(gap, float((top[..., 0] - top[..., 1])[live].min()))
    return gap


def well_posed_case(cfg, shape, seed, tag="train"):
    for sd in range(seed, seed + 50):
        p = O.make_unet_params(*cfg, seed=sd)
        x = torch.from_numpy(O.formula_normal(tag + "/x", shape, seed=sd))
        if pool_margin(p, x, cfg[3]) > 5e-5:   # forward rounding differences are ~1e-5 at most
            return sd, p, x
    raise RuntimeError("no well-posed seed found")


def build(cfg, seed, dev):
    m = mgunet.UNet(*cfg)
    m.load_state_dict(O.make_unet_params(*cfg, seed=seed))
    return m.to(dev)


def flat_of(d, names):
    return torch.cat([d[k].reshape(-1).float().cpu() for k in names])


def check_against(tr, model, ref_loss, ref_grads, ref_newp, ref_stats, names, loss):
    assert abs(float(loss) - ref_loss) <= 1e-4 * abs(ref_loss), (float(loss), ref_loss)
    sd = dict(model.named_parameters())
    gmax = max(float(ref_grads[k].abs().max()) for k in names)
    for k in names:
        g = sd[k].grad.detach().cpu()
        rn, dn = float(ref_grads[k].norm()), float((g - ref_grads[k]).norm())
        assert dn <= 2e-2 * rn + 1e-6 * gmax * np.sqrt(g.numel()), (k, dn, rn)  # conditioning: see test_c5_*
    # Parameters after Adam.  At step 1 the update is lr*g/(|g|+eps): where |g + wd*p| is tiny the SIGN of a
    # 1e-9 gradient difference decides a 1e-3 step, so the comparison with the reference's parameters is
    # robust (99.9th percentile) while the Adam kernel itself is checked exactly in test_adam_kernel_exact.
    d = torch.cat([(sd[k].detach().cpu() - ref_newp[k]).abs().reshape(-1) for k in names])
    assert float(torch.quantile(d[torch.randperm(d.numel())[:200000]], 0.999)) <= 3e-5
    assert float(d.max()) <= 2.1e-3
    msd = model.state_dict()
    for k, v in ref_stats.items():
        assert float((msd[k].cpu() - v).abs().max()) <= 2e-5, k


@pytest.mark.parametrize("cfg,shape", [((3, 3, 8, 2), (2, 3, 37, 45)), ((1, 2, 8, 2), (1, 1, 32, 32)),
                                       ((3, 2, 16, 3), (2, 3, 48, 40))])
def test_train_step_vs_oracle_small_and_ragged(cuda, cfg, shape):
    seed, p, x = well_posed_case(cfg, shape, 21)
    y = torch.from_numpy(O.formula_labels("train/y", (shape[0], shape[2], shape[3]), cfg[1], seed=22))
    ref_loss, ref_g, ref_p, ref_stats, _, _ = O.train_step(p, x, y, cfg[3])
    names = list(ref_g.keys())
    model = build(cfg, seed, cuda)
    assert [n for n, _ in model.named_parameters()] == names
    tr = mgunet.Trainer(model, lr=1e-3, weight_decay=1e-4)
    loss = tr.train_step(x.to(cuda), y.to(cuda))
    check_against(tr, model, float(ref_loss), ref_g, ref_p, ref_stats, names, loss)
    nbt = [int(m.num_batches_tracked) for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert all(v == 1 for v in nbt)
    # eval forward after the step uses the UPDATED parameters and running statistics
    model.eval()
    with torch.no_grad():
        lg = model(x.to(cuda))[0]
        q = {k: v.clone() for k, v in ref_p.items()}
        olg = O.unet_forward(q, x, cfg[3])[0]
    assert float((lg.cpu() - olg).abs().max()) <= 1e-3


def test_second_step_uses_moments_and_updated_weights(cuda):
    cfg, shape = (3, 2, 8, 2), (2, 3, 32, 32)
    p = O.make_unet_params(*cfg, seed=23)
    x = torch.from_numpy(O.formula_normal("train2/x", shape, seed=23))
    y = torch.from_numpy(O.formula_labels("train2/y", (2, 32, 32), 2, seed=24))
    l1, _, p1, _, m1, v1 = O.train_step(p, x, y, 2)
    l2, g2, p2, s2, _, _ = O.train_step(p1, x, y, 2, step=2, exp_avg=m1, exp_avg_sq=v1)
    model = build(cfg, 23, cuda)
    tr = mgunet.Trainer(model)
    a = tr.train_step(x.to(cuda), y.to(cuda)).clone()
    b = tr.train_step(x.to(cuda), y.to(cuda)).clone()
    assert abs(float(a) - float(l1)) <= 1e-4 * float(l1) and abs(float(b) - float(l2)) <= 2e-4 * float(l2)
    sd = dict(model.named_parameters())
    d = torch.cat([(sd[k].detach().cpu() - p2[k]).abs().reshape(-1) for k in g2])
    assert float(torch.quantile(d, 0.999)) <= 6e-5 and float(d.max()) <= 4.2e-3


@pytest.mark.parametrize("tag,shape", [("s", (2, 3, 128, 128)), ("f", (4, 3, 512, 512))])
def test_c5_step_record_from_reference(cuda, golden, tag, shape):
    """BASELINE config 5 shard (4 images of 3x512x512 per GPU) and a small shard, vs the reference's own
    autograd/Adam step stored in tests/golden/c5.npz."""
    g = golden["c5"]
    cfg = (3, 2, 32, 4)
    model = build(cfg, 0, cuda)
    names = [str(n) for n in g["param_names"]]
    assert [n for n, _ in model.named_parameters()] == names
    x = torch.from_numpy(O.formula_normal(f"c5/{tag}/x", shape, seed=4)).to(cuda)
    y = torch.from_numpy(O.formula_labels(f"c5/{tag}/y", (shape[0], shape[2], shape[3]), 2, seed=5)).to(cuda)
    tr = mgunet.Trainer(model, lr=1e-3, weight_decay=1e-4)
    loss = tr.forward_backward(x, y)
    ref_loss = float(g[f"{tag}_loss"])
    assert abs(float(loss) - ref_loss) <= 1e-4 * ref_loss, (float(loss), ref_loss)
    params = dict(model.named_parameters())
    gn = np.array([float(params[k].grad.norm()) for k in names])
    # Conditioning: train-mode BatchNorm + ReLU masks make these gradients sensitive to 1e-7 perturbations; the
    # reference's OWN fp32 gradients sit `cond` (5e-3 .. 9e-3 relative L2) away from its float64 gradients
    # (recorded by oracle/make_golden.py).  The KERNELS are held to 2e-5 against float64 one by one in
    # test_gpu_backward_kernels.py and as a network, with the forward's decisions pinned, in test_gpu_train_net.py, where
    # nothing is ill-conditioned; this whole-step record is the integration check against the reference's own step: the
    # HIP path must be as close to the float64 truth as the reference's fp32 path is: per-parameter norm within
    # (2*cond + 1e-3) (measured worst deviation 2.7e-3 / 1.2e-3), sampled elements within (2*max cond + 2e-3)*max|g|, and the
    # aggregate error within 1.25x the reference's own on the default kernels (the A/B kernel selections -- MGU_WINO_PREC=0,
    # MGU_NO_WINOGRAD=1 ... -- are other fp32 summation orders of the same ill-conditioned quantity and land at 1.3-1.65x: 2x there).
    ref_gn, cond = g[f"{tag}_grad_norms64"], g[f"{tag}_cond"]
    big = ref_gn > 1e-4 * ref_gn.max()          # conv biases under BatchNorm have analytically zero gradient
    rel = np.abs(gn[big] / ref_gn[big] - 1)
    assert np.all(rel <= 2 * cond[big] + 1e-3), (rel.max(), [names[i] for i in np.where(big)[0][rel > 2 * cond[big] + 1e-3]])
    assert np.all(gn[~big] <= 1e-3 * ref_gn.max())
    idx = torch.from_numpy(g[f"{tag}_idx"])
    got = tr.grad.cpu()[idx].numpy()
    ref_s = g[f"{tag}_grad_s64"]
    cmax = float(cond[big].max())
    assert np.abs(got - ref_s).max() <= (2 * cmax + 2e-3) * np.abs(ref_s).max()
    # and in aggregate the HIP gradient is no further from float64 than the reference's fp32 gradient is
    err_hip = np.linalg.norm(got - ref_s) / np.linalg.norm(ref_s)
    err_ref = np.linalg.norm(g[f"{tag}_grad_s"] - ref_s) / np.linalg.norm(ref_s)
    print(f"[c5/{tag}] loss {float(loss):.6f} (ref {ref_loss:.6f}); sampled-grad rel L2 error vs float64: HIP {err_hip:.2e}, "
          f"reference fp32 {err_ref:.2e}; worst norm dev {rel.max():.2e}")
    ab = any(os.environ.get(k) for k in ("MGU_WINO_PREC", "MGU_NO_WINOGRAD", "MGU_NO_WINO_CP", "MGU_NO_WINO_DGRAD", "MGU_NO_WINO_WGRAD"))
    assert err_hip <= (2.0 if ab else 1.25) * err_ref + 1e-4   # measured r02: 7.7e-3 vs 7.4e-3 (128^2 shard), 4.5e-3 vs 4.3e-3 (512^2 shard)
    tr.optimizer_step(1.0)
    dp = np.abs(tr.flat.cpu()[idx].numpy() - g[f"{tag}_param_s"])
    assert np.quantile(dp, 0.99) <= 5e-5 and dp.max() <= 2.1e-3   # see check_against() on Adam conditioning
    sd = model.state_dict()
    assert np.abs(sd["encoder.encoder_blocks.0.bn1.running_mean"].cpu().numpy() - g[f"{tag}_bn_rm"]).max() <= 1e-5
    assert np.abs(sd["encoder.encoder_blocks.0.bn1.running_var"].cpu().numpy() - g[f"{tag}_bn_rv"]).max() <= 1e-5
    assert np.abs(sd["encoder.bottleneck.bn2.running_mean"].cpu().numpy() - g[f"{tag}_bn_rm_b"]).max() <= 1e-5
    assert np.abs(sd["encoder.bottleneck.bn2.running_var"].cpu().numpy() - g[f"{tag}_bn_rv_b"]).max() <= 1e-5


def test_one_off_and_batched_weight_packs_write_the_same_bytes(cuda):
    """The two launch paths of csrc/pack.hip fill a form with the same bytes.  After load_state_dict the first backward of a context
    packs its data-gradient forms one at a time (launch_pack_one: the Winograd U of every 3x3 layer, the three-piece fragments of
    both ConvTranspose layers, the final conv's panel), because the context had not trained when the weights were loaded; after a
    refresh with unchanged parameters the same forms come from the one batched launch.  Channels 32 / 64 / 128 admit the Winograd
    data gradient on every layer and the three-piece data gradient on both up-convolutions; 24 x 40 has edge patches at all three
    levels.  The sums of a step are repeatable, so the steps must agree bit for bit: (b) == (c) first, which tells "not repeatable"
    from "the paths differ"."""
    cfg, shape = (3, 2, 32, 2), (2, 3, 24, 40)
    model = build(cfg, 31, cuda)
    x = torch.from_numpy(O.formula_normal("pack/x", shape, seed=31)).to(cuda)
    y = torch.from_numpy(O.formula_labels("pack/y", (shape[0], shape[2], shape[3]), cfg[1], seed=32)).to(cuda)
    tr = mgunet.Trainer(model)

    def step():
        loss = tr.forward_backward(x, y)
        return loss.clone(), tr.grad.clone()

    a = step()                             # forms of the data gradient packed lazily, one launch each
    model.refresh_packed_weights(cuda)     # every form in the batched launch
    b = step()
    c = step()
    assert float(b[1].abs().max()) > 0 and bool(torch.isfinite(b[1]).all())
    assert torch.equal(b[0], c[0]) and torch.equal(b[1], c[1])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def backward_as_trainer(tr, logits, masks, dev):
    """the cross-entropy and mgu_unet_backward calls exactly as Trainer.forward_backward issues them, on the logits of a train-mode
    forward the caller has already run"""
    from mgunet import _lib
    ctx = tr.model._context(dev)
    B, Cc, H, W = logits.shape
    nhwc = logits.permute(0, 2, 3, 1)
    assert nhwc.is_contiguous()
    npix, ldd = B * H * W, (Cc + 3) // 4 * 4
    dlogits = torch.empty((npix, ldd), device=dev, dtype=torch.float32)
    _lib.call("mgu_cross_entropy", dev, nhwc, masks.contiguous(), npix, Cc, 1.0 / npix, dlogits, tr._loss, ctx=ctx)
    _lib.call("mgu_unet_backward", dev, dlogits, tr.grad, ctx=ctx)
    return tr.grad.clone()


def test_backward_follows_the_latest_forward(cuda):
    """The backward reads the record of the LAST train-mode forward of its context: a forward at another batch size and grid before
    the step leaves nothing behind.  The reductions are fixed-order, so the gradients agree bit for bit."""
    cfg = (3, 2, 8, 2)
    x1 = torch.from_numpy(O.formula_normal("record/x1", (2, 3, 16, 16), seed=51)).to(cuda)
    x2 = torch.from_numpy(O.formula_normal("record/x2", (1, 3, 24, 40), seed=52)).to(cuda)
    y2 = torch.from_numpy(O.formula_labels("record/y2", (1, 24, 40), cfg[1], seed=53)).to(cuda)
    grads = []
    for earlier_forward in (True, False):
        model = build(cfg, 51, cuda)
        tr = mgunet.Trainer(model)
        if earlier_forward:
            model.train()
            model(x1)
        tr.forward_backward(x2, y2)
        grads.append(tr.grad.clone())
    assert float(grads[1].abs().max()) > 0 and bool(torch.isfinite(grads[1]).all())
    assert torch.equal(grads[0], grads[1])


def test_building_block_between_forward_and_backward_leaves_the_step_alone(cuda):
    """A backward building block on the model's own context shares the reduction slots with the step, runs in the building-block
    scratch and describes its forward with a record of its own: called between the train-mode forward and mgu_unet_backward it
    changes no bit of the step's gradient."""
    from mgunet import _lib
    cfg, shape = (3, 2, 8, 2), (2, 3, 16, 16)
    x = torch.from_numpy(O.formula_normal("record/x1", shape, seed=51)).to(cuda)
    y = torch.from_numpy(O.formula_labels("record/y1", (2, 16, 16), cfg[1], seed=54)).to(cuda)
    B, H, W, Cc = 1, 8, 8, 8
    t = {k: torch.from_numpy(O.formula_normal("record/" + k, s, seed=55 + i)).to(cuda)
         for i, (k, s) in enumerate({"in": (B, H, W, Cc), "z": (B, H, W, Cc), "dy": (B, H, W, Cc), "w": (Cc, Cc, 3, 3), "gamma": (Cc,),
                                     "beta": (Cc,), "mean": (Cc,)}.items())}
    t["invstd"] = torch.full((Cc,), 0.75, device=cuda)
    grads = []
    for interleave in (True, False):
        model = build(cfg, 51, cuda)
        tr = mgunet.Trainer(model)
        model.train()
        logits = model(x)[0]
        if interleave:
            ctx = model._context(cuda)
            o = {k: torch.empty(s, device=cuda) for k, s in {"dz": (B, H, W, Cc), "dw": (Cc, Cc, 3, 3), "din": (B, H, W, Cc), "dgamma": (Cc,),
                                                             "dbeta": (Cc,), "dbias": (Cc,)}.items()}
            _lib.check(_lib.lib().mgu_bn_relu_conv_backward_nhwc(
                ctx.handle, t["in"].data_ptr(), Cc, t["z"].data_ptr(), t["dy"].data_ptr(), Cc, t["gamma"].data_ptr(), t["beta"].data_ptr(),
                t["mean"].data_ptr(), t["invstd"].data_ptr(), t["w"].data_ptr(), B, H, W, Cc, Cc, o["dz"].data_ptr(), o["dgamma"].data_ptr(),
                o["dbeta"].data_ptr(), o["dbias"].data_ptr(), o["dw"].data_ptr(), o["din"].data_ptr(), Cc, _lib.current_stream_ptr(cuda)),
                ctx.handle)
            assert float(o["dw"].abs().max()) > 0 and all(bool(torch.isfinite(v).all()) for v in o.values())
        grads.append(backward_as_trainer(tr, logits, y, cuda))
    assert float(grads[1].abs().max()) > 0 and bool(torch.isfinite(grads[1]).all())
    assert torch.equal(grads[0], grads[1])


def test_adam_kernel_exact(cuda):
    """mgu_adam_step against torch.optim.Adam(lr, weight_decay) semantics evaluated in float64 on the host."""
    from mgunet import _lib
    from mgunet.gat import _context
    n = 100003
    p = torch.from_numpy(O.formula_normal("adam/p", (n,), seed=1))
    g = torch.from_numpy(O.formula_normal("adam/g", (n,), seed=2)) * 1e-2
    m = torch.from_numpy(O.formula_normal("adam/m", (n,), seed=3)) * 1e-3
    v = torch.from_numpy(O.formula_uniform("adam/v", (n,), 0.0, 1e-4, seed=4))
    lr, b1, b2, eps, wd, step, gs = 1e-3, 0.9, 0.999, 1e-8, 1e-4, 7, 0.5
    P, G, M_, V = (t.double() for t in (p, g, m, v))
    gt = G * gs + wd * P
    M2, V2 = b1 * M_ + (1 - b1) * gt, b2 * V + (1 - b2) * gt * gt
    ref = P - (lr / (1 - b1 ** step)) * M2 / (V2.sqrt() / np.sqrt(1 - b2 ** step) + eps)
    dp, dg, dm, dv = (t.clone().to(cuda) for t in (p, g, m, v))
    ctx = _context(cuda)
    _lib.check(_lib.lib().mgu_adam_step(ctx.handle, dp.data_ptr(), dg.data_ptr(), dm.data_ptr(), dv.data_ptr(), n, lr, b1, b2,
                                        eps, wd, step, gs, _lib.current_stream_ptr(cuda)), ctx.handle)
    assert float((dp.cpu().double() - ref).abs().max()) <= 5e-7
    assert float((dm.cpu().double() - M2).abs().max()) <= 1e-8 and float((dv.cpu().double() - V2).abs().max()) <= 1e-9


def test_train_forward_returns_reference_tuple_and_batch_stats(cuda, golden):
    g = golden["unet_tiny"]
    cfg, shape = (3, 3, 8, 2), (2, 3, 37, 45)
    model = build(cfg, 11, cuda).train()
    x = torch.from_numpy(O.formula_normal("tiny/b/x", shape, seed=11)).to(cuda)
    lg, sk, ft = model(x)
    assert float(np.abs(lg.cpu().numpy() - g["b_train_logits"]).max()) <= 1e-3
    sd = model.state_dict()
    assert np.abs(sd["encoder.encoder_blocks.0.bn1.running_mean"].cpu().numpy() - g["b_bn_rm_first"]).max() <= 1e-5
    assert np.abs(sd["decoder.decoder_blocks.1.conv_block.bn2.running_var"].cpu().numpy() - g["b_bn_rv_last"]).max() <= 1e-5


def test_backward_without_forward_is_an_error(cuda):
    import ctypes as C
    from mgunet import _lib
    model = build((3, 2, 8, 2), 5, cuda).eval()
    model(torch.zeros(1, 3, 16, 16, device=cuda))
    ctx = model._context(cuda)
    t = torch.zeros(16, device=cuda)
    assert _lib.lib().mgu_unet_backward(ctx.handle, t.data_ptr(), t.data_ptr(), None) == _lib.MGU_ERR_STATE


def test_checkpoint_dict_resume_and_torch_adam_interchange(cuda, tmp_path):
    """train_segmentation.py:154-168: the checkpoint dict {'epoch', 'model_state_dict', 'optimizer_state_dict', 'loss'} written by a
    Trainer after two steps; a FRESH trainer that loads it continues exactly like the one that kept running, and the same file drives
    torch's own Adam on the oracle to the same parameters."""
    cfg, shape = (3, 2, 8, 2), (2, 3, 32, 32)
    x = torch.from_numpy(O.formula_normal("ck/x", shape, seed=23)).to(cuda)
    y = torch.from_numpy(O.formula_labels("ck/y", (2, 32, 32), 2, seed=24)).to(cuda)
    model = build(cfg, 23, cuda)
    tr = mgunet.Trainer(model, lr=1e-3, weight_decay=1e-4)
    sch = mgunet.StepLR(tr, step_size=1, gamma=0.5)
    tr.train_step(x, y)
    tr.train_step(x, y)
    sch.step()                                               # lr 5e-4 from here on
    path = str(tmp_path / "unet_segmentation_epoch_1.pth")
    tr.save_checkpoint(path, epoch=1, loss=0.5)
    ck = torch.load(path, map_location="cpu")
    assert sorted(ck) == ["epoch", "loss", "model_state_dict", "optimizer_state_dict"] and ck["epoch"] == 1
    assert ck["optimizer_state_dict"]["param_groups"][0]["lr"] == 5e-4
    assert float(ck["optimizer_state_dict"]["state"][0]["step"]) == 2.0
    # the reference's loaders accept the file (infer_segmentation.py:92-95)
    m2 = mgunet.UNet(*cfg)
    m2.load_state_dict(ck["model_state_dict"])
    # resume in a fresh trainer
    tr2 = mgunet.Trainer(build(cfg, 99, cuda), lr=123.0, weight_decay=0.0)     # everything wrong until the checkpoint is loaded
    tr2.load_checkpoint(path)
    assert tr2.lr == 5e-4 and tr2.wd == 1e-4 and tr2.step_count == 2
    l1 = tr.train_step(x, y).clone()
    l2 = tr2.train_step(x, y).clone()
    torch.cuda.synchronize()
    assert abs(float(l1) - float(l2)) <= 1e-6 * abs(float(l1))
    assert float((tr.flat - tr2.flat).abs().max()) <= 1e-6                      # same step from the same state (fp32 atomics order aside)
    # torch.optim.Adam resumes from the same file: one oracle step from the checkpointed weights / moments
    p0 = {k: v.clone() for k, v in ck["model_state_dict"].items()}
    names = [n for n, _ in m2.named_parameters()]
    m_, v_ = ({n: ck["optimizer_state_dict"]["state"][i][key] for i, n in enumerate(names)} for key in ("exp_avg", "exp_avg_sq"))
    _, _, p_ref, _, _, _ = O.train_step(p0, x.cpu(), y.cpu(), cfg[3], lr=5e-4, weight_decay=1e-4, step=3, exp_avg=m_, exp_avg_sq=v_)
    sd = dict(tr.model.named_parameters())
    d = torch.cat([(sd[k].detach().cpu() - p_ref[k]).abs().reshape(-1) for k in names])
    assert float(torch.quantile(d, 0.999)) <= 6e-5


def test_train_forward_when_winograd_grid_exceeds_statistics_rows(cuda, monkeypatch):
    """The Winograd epilogue accumulates BatchNorm batch statistics into one table row per workgroup (STAT_ROWS = 576).  A launch
    whose grid is larger (>= 19 images of 512^2 per GPU, or a small MGU_WINO_PPB_CAP as here: 4 x 192 x 256 at one patch per
    workgroup = 768 workgroups on the full-resolution layer) must take the separate statistics pass instead of failing, and give
    the same logits and running statistics (model/unet/unet_encoder.py:12-13, train mode)."""
    cfg, shape = (3, 2, 16, 2), (4, 3, 192, 256)
    x = torch.from_numpy(O.formula_normal("statrows/x", shape, seed=31)).to(cuda)
    out = {}
    for tag, capv in (("fused", None), ("capped", "1")):
        if capv is None:
            monkeypatch.delenv("MGU_WINO_PPB_CAP", raising=False)
        else:
            monkeypatch.setenv("MGU_WINO_PPB_CAP", capv)
        m = build(cfg, 31, cuda).train()   # a new model = a new mgu_ctx: the switch is read by mgu_create
        lg = m(x)[0].clone()
        out[tag] = (lg, {k: v.clone() for k, v in m.state_dict().items() if "running" in k})
    monkeypatch.delenv("MGU_WINO_PPB_CAP", raising=False)
    a, b = out["fused"], out["capped"]
    assert float((a[0] - b[0]).abs().max()) <= 2e-5 * float(a[0].abs().max())
    for k in a[1]:
        assert float((a[1][k] - b[1][k]).abs().max()) <= 1e-6 + 1e-5 * float(a[1][k].abs().max()), k


def test_optimizer_step_invalidates_the_models_other_contexts(cuda):
    """A model holds one library context per (device, storage dtype).  The Adam kernel updates the parameters in place without a
    version bump, and Trainer.optimizer_step repacks only the training context: the bf16-storage context the same model used
    before the step must not keep serving the old packed weights."""
    cfg, shape = (3, 2, 8, 2), (2, 3, 32, 32)
    x = torch.from_numpy(O.formula_normal("ctxinv/x", shape, seed=41)).to(cuda)
    y = torch.from_numpy(O.formula_labels("ctxinv/y", (2, 32, 32), 2, seed=42)).to(cuda)
    model = build(cfg, 41, cuda)
    tr = mgunet.Trainer(model, lr=5e-2, weight_decay=0.0)   # a step large enough to show in the logits
    model.eval().set_compute_dtype(torch.bfloat16)
    with torch.no_grad():
        before = model(x)[0].clone()                         # the bf16 context is created and loaded here
    model.set_compute_dtype(torch.float32)
    tr.train_step(x, y)
    model.eval().set_compute_dtype(torch.bfloat16)
    with torch.no_grad():
        after = model(x)[0].clone()
    fresh = mgunet.UNet(*cfg, compute_dtype=torch.bfloat16)
    fresh.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()})
    with torch.no_grad():
        want = fresh.to(cuda).eval()(x)[0]
    assert float((after - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()))
    assert float((after - before).abs().max()) > 1e-3   # the step really changed the output


def test_sgd_kernel_matches_torch_optim_sgd(cuda):
    """mgu_sgd_step against torch.optim.SGD(lr, momentum, weight_decay) itself (scripts/train_segmentation.py:97-98) over three steps:
    first step (buffer = gradient), later steps (momentum * buffer + gradient), and momentum 0 (no buffer)."""
    from mgunet import _lib
    from mgunet.gat import _context
    n = 50021
    p0 = torch.from_numpy(O.formula_normal("sgd/p", (n,), seed=1))
    grads = [torch.from_numpy(O.formula_normal(f"sgd/g{i}", (n,), seed=2 + i)) * 1e-2 for i in range(3)]
    ctx = _context(cuda)
    for momentum in (0.9, 0.0):
        ref = torch.nn.Parameter(p0.clone().double())
        opt = torch.optim.SGD([ref], lr=1e-2, momentum=momentum, weight_decay=1e-4)
        dp, buf = p0.clone().to(cuda), torch.zeros(n, device=cuda)
        for step, g in enumerate(grads, 1):
            ref.grad = g.double()
            opt.step()
            _lib.check(_lib.lib().mgu_sgd_step(ctx.handle, dp.data_ptr(), g.to(cuda).data_ptr(), buf.data_ptr() if momentum else None, n,
                                               1e-2, momentum, 1e-4, step, 1.0, _lib.current_stream_ptr(cuda)), ctx.handle)
            assert float((dp.cpu().double() - ref.detach()).abs().max()) <= 2e-7 * step
        if momentum:
            assert float((buf.cpu().double() - opt.state[ref]["momentum_buffer"]).abs().max()) <= 1e-8


def test_trainer_with_sgd_follows_torch_optim_sgd_and_interchanges_state(cuda):
    """Trainer(optimizer='sgd'): two train steps; the parameters follow torch.optim.SGD applied to the trainer's own gradients, and the
    optimizer state loads into a real torch.optim.SGD and back."""
    cfg, shape = (3, 2, 8, 2), (2, 3, 32, 32)
    x = torch.from_numpy(O.formula_normal("sgdt/x", shape, seed=31)).to(cuda)
    y = torch.from_numpy(O.formula_labels("sgdt/y", (2, 32, 32), 2, seed=32)).to(cuda)
    model = build(cfg, 31, cuda)
    tr = mgunet.Trainer(model, lr=5e-3, weight_decay=1e-4, optimizer="sgd", momentum=0.9)
    names = [n for n, _ in model.named_parameters()]
    shadow = [torch.nn.Parameter(p.detach().clone().double()) for _, p in model.named_parameters()]
    opt = torch.optim.SGD(shadow, lr=5e-3, momentum=0.9, weight_decay=1e-4)
    for step in range(2):
        tr.forward_backward(x, y)
        for s_, (_, p) in zip(shadow, model.named_parameters()):
            s_.grad = p.grad.detach().clone().double()
        opt.step()
        tr.optimizer_step()
        for n_, s_, (_, p) in zip(names, shadow, model.named_parameters()):
            assert float((p.detach().double() - s_.detach()).abs().max()) <= 1e-6, (step, n_)
            s_.data.copy_(p.detach().double())     # keep the shadow on the fp32 trajectory
    sd = tr.optimizer_state_dict()
    opt2 = torch.optim.SGD([torch.nn.Parameter(p.detach().clone()) for _, p in model.named_parameters()], lr=1.0, momentum=0.5)
    opt2.load_state_dict(sd)
    assert opt2.param_groups[0]["momentum"] == 0.9 and opt2.param_groups[0]["lr"] == 5e-3
    tr2 = mgunet.Trainer(build(cfg, 31, cuda), optimizer="sgd")
    tr2.load_optimizer_state_dict(opt2.state_dict())
    assert tr2.momentum == 0.9 and torch.equal(tr2.exp_avg, tr.exp_avg)
    with pytest.raises(ValueError):
        mgunet.Trainer(build(cfg, 31, cuda), optimizer="rmsprop")
