"""The driver's contract with bench.py: `python bench.py --gpus 1 --steps K --warmup W` prints ONE JSON line with the agreed keys, the
roofline object of the dominant kernel and (N = 1) the CPU baseline; the train mode does the same for BASELINE configs[4]."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
        "roofline", "cpu_baseline"}


def run_bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_default_forward_line(cuda):
    j = run_bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--sustained-seconds", "0")
    assert KEYS <= set(j), sorted(KEYS - set(j))
    assert j["n_gpus"] == 1 and j["steps"] == 3 and j["warmup"] == 1 and j["higher_is_better"] is True and j["scaling"] == "weak"
    assert j["unit"] == "Mpix/s" and j["dtype"] == "f32" and j["vs_baseline"] is None and "workload" in j["config"]
    assert abs(j["value"] - 8 * 512 * 512 / (j["ms_per_step"] * 1e-3) / 1e6) <= 1e-2 * j["value"]
    r = j["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and 0.0 < r["frac"] < 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert 0.0 < r["algorithmic_frac"] < r["frac"]          # Winograd + three-piece split: issued > algorithmic
    assert "3 bf16 pieces" in r["arithmetic"] and "bf16" in r["pipe"]


def test_train_line(cuda):
    j = run_bench("--gpus", "1", "--mode", "train", "--steps", "2", "--warmup", "1", "--no-cpu-baseline")
    assert KEYS <= set(j)
    assert j["unit"] == "Mpix/s" and j["steps"] == 2 and "configs[4]" in j["config"]["workload"]
    assert j["roofline"]["kernel"].startswith("wino") and 0.0 < j["roofline"]["frac"] < 1.0
    assert 0.0 < j["final_loss"] < 10.0


def test_dump_outputs_of_the_last_timed_step(cuda, tmp_path):
    """--dump-outputs: the forward's outputs as float32 .npy files under 64 MiB in all, and the same bytes from a run of one timed
    step and from the last of three (the inputs depend only on the workload arguments; the forward is deterministic)."""
    import numpy as np
    quiet = ("--gpus", "1", "--no-cpu-baseline", "--no-profile-pass", "--sustained-seconds", "0", "--spread-windows", "0")
    j1 = run_bench(*quiet, "--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path / "a"))
    j3 = run_bench(*quiet, "--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path / "b"))
    assert j1["steps"] == 1 and j3["steps"] == 3
    names = {"logits", "node_embeddings"} | {f"{k}_{i}" for k in ("skips", "decoder_feats") for i in range(4)}
    files = {p.stem for p in (tmp_path / "a").iterdir()}
    assert files == names == {p.stem for p in (tmp_path / "b").iterdir()}
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    b = {n: np.load(tmp_path / "b" / (n + ".npy")) for n in names}
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["logits"].shape == (8, 2, 512, 512) and a["node_embeddings"].shape == (8 * 1024, 64)
    for n in names:
        assert a[n].dtype == np.float32 and np.isfinite(a[n]).all(), n
        assert np.array_equal(a[n], b[n]), n


def test_plain_run_carries_cpu_baseline_and_other_configs(cuda):
    """What the driver runs at round end (no extra flags): the headline line plus the CPU baseline and the bf16 / train-step side measurements."""
    j = run_bench("--steps", "3", "--warmup", "1", "--sustained-seconds", "0")
    assert KEYS <= set(j)
    c = j["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == j["unit"] and c["value"] > 0 and c["cores"] >= 1 and "sample" in c
    o = j["other_configs"]
    assert not any(k.endswith("_error") for k in o), o
    assert len(o) == 2 and all(v["ms_per_step"] > 0 and v["mpix_per_s"] > 0 for v in o.values())


# Kernel-family labels of the profiling records (mgu_profile_read_kernels), which bench.py's kernel tables, dominant kernel and
# traffic lookup key on.  One small U-Net (1 x 64 x 256, depth 4: Winograd assembly kernels on the upper levels, the C++ kernels on
# the 4 x 16 bottleneck, the halo kernels under MGU_NO_WINOGRAD and in bf16) under each kernel-selection switch: forward, then one
# train step (fp32 only), as (label, launches, pipe) in the order of first launch.
FAMILY_CASES = {
    "default": ({}, "f32", {
        "forward": [
            ["conv3x3_first_mfma_kernel", 1, 1],
            ["mgu_wino_cp1r2_gfx950 (asm form of wino3x3_cp_kernel<1>)", 2, 1],
            ["mgu_wino_cp2_gfx950 (asm form of wino3x3_cp_kernel<2>)", 12, 1],
            ["wino3x3_cp_kernel<2>", 2, 1],
            ["convt2x2_x3_kernel", 4, 1],
            ["mgu_wino_cp1r4_gfx950 (asm form of wino3x3_cp_kernel<1>)", 1, 1],
            ["conv1x1_head_kernel", 1, -1]],
        "train": [
            ["conv3x3_first_mfma_kernel", 1, 1],
            ["wino3x3_cp_kernel<1>", 3, 1],
            ["wino3x3_cp_kernel<2>", 14, 1],
            ["convt2x2_x3_kernel", 4, 1],
            ["wino_wgrad_f32_kernel<X3>", 17, 1],
            ["wino3x3_cp_kernel<1> (dgrad)", 3, 1],
            ["wino3x3_cp_kernel<2> (dgrad)", 14, 1],
            ["convt2x2_x3_kernel (dgrad)", 4, 1],
            ["wgrad_thin kernels", 1, -1]],
    }),
    "wino_asm_0": ({"MGU_WINO_ASM": "0"}, "f32", {
        "forward": [
            ["conv3x3_first_mfma_kernel", 1, 1],
            ["wino3x3_cp_kernel<1>", 3, 1],
            ["wino3x3_cp_kernel<2>", 14, 1],
            ["convt2x2_x3_kernel", 4, 1],
            ["conv1x1_head_kernel", 1, -1]],
        "train": [
            ["conv3x3_first_mfma_kernel", 1, 1],
            ["wino3x3_cp_kernel<1>", 3, 1],
            ["wino3x3_cp_kernel<2>", 14, 1],
            ["convt2x2_x3_kernel", 4, 1],
            ["wino_wgrad_f32_kernel<X3>", 17, 1],
            ["wino3x3_cp_kernel<1> (dgrad)", 3, 1],
            ["wino3x3_cp_kernel<2> (dgrad)", 14, 1],
            ["convt2x2_x3_kernel (dgrad)", 4, 1],
            ["wgrad_thin kernels", 1, -1]],
    }),
    "wino_prec_0": ({"MGU_WINO_PREC": "0"}, "f32", {
        "forward": [
            ["conv3x3_first_mfma_kernel", 1, 1],
            ["wino3x3_f32_kernel<1,0>", 3, 0],
            ["wino3x3_f32_kernel<0,0>", 14, 0],
            ["igemm_kernel<f32> (ConvTranspose)", 4, 0],
            ["conv1x1_head_kernel", 1, -1]],
        "train": [
            ["conv3x3_first_mfma_kernel", 1, 1],
            ["wino3x3_f32_kernel<1,0>", 3, 0],
            ["wino3x3_f32_kernel<0,0>", 14, 0],
            ["igemm_kernel<f32> (ConvTranspose)", 4, 0],
            ["wino_wgrad_f32_kernel<X3>", 17, 1],
            ["wino3x3_f32_kernel<*,0> (dgrad)", 17, 0],
            ["igemm_kernel<f32> (ConvTranspose dgrad)", 4, 0],
            ["wgrad_thin kernels", 1, -1]],
    }),
    "no_winograd": ({"MGU_NO_WINOGRAD": "1"}, "f32", {
        "forward": [
            ["conv3x3_first_mfma_kernel", 1, 1],
            ["conv3x3_halo_kernel<f32>", 17, 0],
            ["convt2x2_x3_kernel", 4, 1],
            ["conv1x1_head_kernel", 1, -1]],
        "train": [
            ["conv3x3_first_mfma_kernel", 1, 1],
            ["conv3x3_halo_kernel<f32>", 17, 0],
            ["convt2x2_x3_kernel", 4, 1],
            ["wino_wgrad_f32_kernel<X3>", 17, 1],
            ["igemm/halo (dgrad)", 17, 0],
            ["convt2x2_x3_kernel (dgrad)", 4, 1],
            ["wgrad_thin kernels", 1, -1]],
    }),
    "no_wino_dgrad": ({"MGU_NO_WINO_DGRAD": "1"}, "f32", {
        "forward": [
            ["conv3x3_first_mfma_kernel", 1, 1],
            ["mgu_wino_cp1r2_gfx950 (asm form of wino3x3_cp_kernel<1>)", 2, 1],
            ["mgu_wino_cp2_gfx950 (asm form of wino3x3_cp_kernel<2>)", 12, 1],
            ["wino3x3_cp_kernel<2>", 2, 1],
            ["convt2x2_x3_kernel", 4, 1],
            ["mgu_wino_cp1r4_gfx950 (asm form of wino3x3_cp_kernel<1>)", 1, 1],
            ["conv1x1_head_kernel", 1, -1]],
        "train": [
            ["conv3x3_first_mfma_kernel", 1, 1],
            ["wino3x3_cp_kernel<1>", 3, 1],
            ["wino3x3_cp_kernel<2>", 14, 1],
            ["convt2x2_x3_kernel", 4, 1],
            ["wino_wgrad_f32_kernel<X3>", 17, 1],
            ["igemm/halo (dgrad)", 17, 0],
            ["convt2x2_x3_kernel (dgrad)", 4, 1],
            ["wgrad_thin kernels", 1, -1]],
    }),
    "bf16": ({}, "bf16", {
        "forward": [
            ["conv3x3_first_mfma_kernel", 1, 1],
            ["conv3x3_halo_kernel<bf16>", 17, 1],
            ["convt2x2_bf16_kernel", 4, 1],
            ["conv1x1_head_kernel", 1, -1]],
    }),
    "bf16_no_convt_frag": ({"MGU_NO_CONVT_FRAG": "1"}, "bf16", {
        "forward": [
            ["conv3x3_first_mfma_kernel", 1, 1],
            ["conv3x3_halo_kernel<bf16>", 17, 1],
            ["igemm_kernel<bf16> (ConvTranspose)", 4, 1],
            ["conv1x1_head_kernel", 1, -1]],
    }),
}


def profiled_families(dev, dtype, train):
    import torch
    import mgunet
    import mgunet_oracle as O
    from mgunet import _lib
    g = torch.Generator().manual_seed(7)
    x = torch.randn(1, 3, 64, 256, generator=g).to(dev)
    m = mgunet.UNet(3, 2, 32, 4, compute_dtype=torch.bfloat16 if dtype == "bf16" else torch.float32)
    m.load_state_dict(O.make_unet_params(3, 2, 32, 4, seed=3))
    m = m.to(dev).eval()
    ctx, L = m._context(dev), _lib.lib()

    def record(run):
        run()
        torch.cuda.synchronize(dev)
        L.mgu_profile_enable(ctx.handle, 1)
        run()
        torch.cuda.synchronize(dev)
        ks = _lib.read_kernel_stats(ctx)
        L.mgu_profile_enable(ctx.handle, 0)
        return [[k["name"], k["launches"], k["pipe"]] for k in ks]

    with torch.no_grad():
        out = {"forward": record(lambda: m(x))}
    if train:
        y = torch.randint(0, 2, (1, 64, 256), generator=g).to(dev)
        tr = mgunet.Trainer(m.train())
        out["train"] = record(lambda: tr.train_step(x, y))
    return out


@pytest.mark.parametrize("case", list(FAMILY_CASES))
def test_profiled_kernel_families(cuda, monkeypatch, case):
    env, dtype, want = FAMILY_CASES[case]
    for k in ("MGU_WINO_ASM", "MGU_WINO_PREC", "MGU_NO_WINOGRAD", "MGU_NO_WINO_DGRAD", "MGU_NO_CONVT_FRAG"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)   # read when the model's context is created
    assert profiled_families(cuda, dtype, dtype == "f32") == want


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_profiled_forward_flops_add_up_to_the_layer_walk(cuda, monkeypatch, dtype):
    """The profile records of one eval forward add up to mgu_unet_flops exactly: the launches and the layer walk that counts them
    cannot drift apart (every term is an integer far below 2^53, so the double sums are exact)."""
    import torch
    import mgunet
    import mgunet_oracle as O
    from mgunet import _lib
    for k in ("MGU_WINO_ASM", "MGU_WINO_PREC", "MGU_NO_WINOGRAD", "MGU_NO_WINO_DGRAD", "MGU_NO_CONVT_FRAG"):
        monkeypatch.delenv(k, raising=False)
    x = torch.randn(1, 3, 64, 256, generator=torch.Generator().manual_seed(7)).to(cuda)
    m = mgunet.UNet(3, 2, 32, 4, compute_dtype=torch.bfloat16 if dtype == "bf16" else torch.float32)
    m.load_state_dict(O.make_unet_params(3, 2, 32, 4, seed=3))
    m = m.to(cuda).eval()
    ctx, L = m._context(cuda), _lib.lib()
    with torch.no_grad():
        m(x)
        torch.cuda.synchronize(cuda)
        L.mgu_profile_enable(ctx.handle, 1)
        m(x)
        torch.cuda.synchronize(cuda)
    ks = _lib.read_kernel_stats(ctx)
    L.mgu_profile_enable(ctx.handle, 0)
    assert sum(k["flops_alg"] for k in ks) == L.mgu_unet_flops(ctx.handle, 1, 64, 256)
