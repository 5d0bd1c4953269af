"""The optimizer step at the size of the flagship network, one process, one GPU: n = 7 766 018 fp32 parameters, the count of
UNet(3, 2, 32, 4).

  adam_step      mgu_adam_step, one launch: the yardstick (the step a default Trainer makes)
  optim_*        mgu_optim_step, three launches: neutral (Adam, every option off), clip (max_norm), clip_skip (+ skip_nonfinite),
                 adamw_clip_ema (AdamW + max_norm + EMA); each launch also between its own event pair (mgu_profile_enable), which
                 holds the gap to its neighbours, so the three add up to more than the call
  grad_norm      mgu_grad_norm alone, two launches
  copy_*         a device copy of the bytes the variant moves (a copy of k floats reads k and writes k): 7n for Adam (p, g, m, v in;
                 p, m, v out), 8n for mgu_optim_step (the gradient is read twice), 10n with the EMA, n for the norm
  torch          the same step composed on the device from torch: clip_grad_norm_ + torch.optim.AdamW.step + torch._foreach_lerp_
  train_step     Trainer.train_step on 4 x 512^2, default and with optimizer="adamw", max_grad_norm, skip_nonfinite, ema_decay
Device times are the median, minimum and maximum of `--runs` loops of `--iters` calls behind a parked stream.  Prints one JSON line
per measurement and, with --out, writes the same lines to that file."""
import argparse
import ctypes as C
import json
import statistics

import benchkit
import torch
from benchkit import median_spread

import mgunet
import mgunet_oracle as O
from mgunet import _lib

N_FLAGSHIP = 7_766_018
LINES = []


def line(**kw):
    benchkit.emit(**kw)
    LINES.append(json.dumps(kw))


def per_launch_us(ctx, fn, iters, runs):
    """{kernel name: median us per launch} from the context's event records"""
    per = {}
    for _ in range(runs):
        _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 1), ctx.handle)
        for _ in range(iters):
            fn()
        for k in _lib.read_kernel_stats(ctx):
            per.setdefault(k["name"], []).append(k["ms"] * 1e3 / k["launches"])
        _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 0), ctx.handle)
    return {k: round(statistics.median(v), 1) for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=N_FLAGSHIP)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, it, runs = args.n, args.iters, args.runs
    ctx = _lib.context(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    p = torch.randn(n, device=dev, generator=gen) * 1e-2
    g = torch.randn(n, device=dev, generator=gen) * 1e-3
    m, v, e = torch.zeros(n, device=dev), torch.zeros(n, device=dev), p.clone()
    lr, betas, eps, wd = 1e-3, (0.9, 0.999), 1e-8, 1e-4

    def copy_us(floats_moved):
        src = torch.empty(floats_moved // 2, device=dev)
        dst = torch.empty_like(src)
        return median_spread(lambda: dst.copy_(src), it, runs)

    us_adam = median_spread(lambda: _lib.call("mgu_adam_step", dev, p, g, m, v, n, lr, betas[0], betas[1], eps, wd, 7, 1.0), it, runs)
    us_copy7 = copy_us(7 * n)
    line(what="adam_step", n=n, launches=1, us_median=us_adam[0], us_min=us_adam[1], us_max=us_adam[2], copy_us_median=us_copy7[0],
         over_copy=round(us_adam[0] / us_copy7[0], 2), GBps=round(7 * n * 4 / us_adam[0] / 1e3, 1))

    variants = {"optim_neutral": (dict(kind=0), False, 8), "optim_clip": (dict(kind=0, max_norm=1.0), False, 8),
                "optim_clip_skip": (dict(kind=0, max_norm=1.0, skip_nonfinite=1), False, 8),
                "optim_adamw_clip_ema": (dict(kind=1, max_norm=1.0, ema_decay=0.999), True, 10)}
    for name, (opts, ema, moved) in variants.items():
        d = _lib.OptimDesc(opts["kind"], lr, betas[0], betas[1], eps, wd, 0.0, 1.0, opts.get("max_norm", 0.0), opts.get("skip_nonfinite", 0),
                           opts.get("ema_decay", 0.0), 0)
        ctrl = torch.zeros(_lib.OPTIM_CTRL_BYTES // 8, device=dev, dtype=torch.int64)

        def step():
            _lib.call("mgu_optim_step", dev, C.byref(d), p, g, m, v, e if ema else None, ctrl, n)

        us = median_spread(step, it, runs)
        each = per_launch_us(ctx, step, it, runs)
        us_copy = copy_us(moved * n)
        line(what=name, n=n, launches=3, us_median=us[0], us_min=us[1], us_max=us[2], partial_us=each.get("grad_norm_partial_kernel"),
             control_us=each.get("optim_control_kernel"), update_us=each.get("optim_update_kernel"), copy_us_median=us_copy[0],
             over_copy=round(us[0] / us_copy[0], 2), over_adam_step=round(us[0] / us_adam[0], 2), GBps=round(moved * n * 4 / us[0] / 1e3, 1),
             applied_steps=int(ctrl[0]))

    ctrl = torch.zeros(_lib.OPTIM_CTRL_BYTES // 8, device=dev, dtype=torch.int64)
    us = median_spread(lambda: _lib.call("mgu_grad_norm", dev, g, n, 1.0, ctrl), it, runs)
    us_copy = copy_us(n)
    line(what="grad_norm", n=n, launches=2, us_median=us[0], us_min=us[1], us_max=us[2], copy_us_median=us_copy[0],
         over_copy=round(us[0] / us_copy[0], 2), GBps=round(n * 4 / us[0] / 1e3, 1))

    w = torch.nn.Parameter(p.clone())
    w.grad = g.clone()
    opt = torch.optim.AdamW([w], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    avg = [w.detach().clone()]

    def torch_step():
        torch.nn.utils.clip_grad_norm_([w], 1.0)
        opt.step()
        torch._foreach_lerp_(avg, [w.detach()], 1.0 - 0.999)

    us = median_spread(torch_step, it, runs)
    line(what="torch_clip_adamw_lerp", n=n, us_median=us[0], us_min=us[1], us_max=us[2])

    cfg = (3, 2, 32, 4)
    B, S = args.batch, args.size
    x = torch.from_numpy(O.formula_normal("optbench/x", (B, 3, S, S), seed=3)).to(dev)
    y = torch.from_numpy(O.formula_labels("optbench/y", (B, S, S), cfg[1], seed=4)).to(dev)
    for name, kw in (("train_step_default", {}),
                     ("train_step_options", dict(optimizer="adamw", max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.999))):
        model = mgunet.UNet(*cfg)
        model.load_state_dict(O.make_unet_params(*cfg, seed=5))
        tr = mgunet.Trainer(model.to(dev), **kw)
        assert tr.flat.numel() == N_FLAGSHIP
        us = median_spread(lambda: tr.train_step(x, y), it, runs)
        line(what=name, B=B, H=S, W=S, us_median=us[0], us_min=us[1], us_max=us[2],
             applied_steps=tr.applied_steps() if tr.ctrl is not None else tr.step_count)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
