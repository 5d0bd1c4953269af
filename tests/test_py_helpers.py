"""Guard against the next paste on the Python side, as test_csrc_helpers.py guards csrc/: the tensor-argument helpers live in
mgunet/_args.py, the evaluators' batch preamble in one base class, the timing and output functions of the bench tools in
tools/benchkit.py.  The guards read source text only (no GPU, no build); the tests of _args itself run on CPU tensors."""
import glob
import os
import re

import pytest
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
TOOLS = {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "tools", "*.py")))}
MGUNET = {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "mingraph-unet_amd", "mgunet", "*.py")))}

TOOL_TEXTS = ["def timed", "def median_ms", "def median_spread", "def emit", "def ellipse_scene", "torch.cuda._sleep", "Event(enable_timing"]
# bench_wino_layers.py interleaves its variants inside one event loop per layer and round; that loop is its own
TOOL_EXCEPTIONS = {("bench_wino_layers.py", "Event(enable_timing")}
MGUNET_TEXTS = ["must live on {self.device}", "does not match logits", "device.index is None", "reshape((1,) +"]
PERMUTE = "permute(0, 2, 3, 1)"
# the permutes that take no copy decision: a strided copy into a channel slice, and two views of storage a forward has just written
PERMUTE_ALLOWED = [("region.py", "out_nhwc[..., c_off:c_off + Cs] = src_nchw.permute(0, 2, 3, 1)"),
                   ("tiled.py", "plan.accumulate(out.permute(0, 2, 3, 1), t0,"),
                   ("tta.py", "logits.append(lg.permute(0, 2, 3, 1))")]


def test_bench_tools_take_timing_and_output_from_benchkit():
    others = {f: t for f, t in TOOLS.items() if f != "benchkit.py"}
    found = {(f, s) for f, t in others.items() for s in TOOL_TEXTS if s in t}
    assert found - TOOL_EXCEPTIONS == set()
    assert [(f, m.group(0)) for f, t in others.items() for m in re.finditer(r"from\s+\w*_bench\s+import", t)] == []
    kit = ["timed", "timed_each", "wall", "median_spread", "emit", "ellipse_scene", "logits_of"]
    assert [n for n in kit if len(re.findall(r"^def " + n + r"\(", TOOLS["benchkit.py"], re.M)) != 1] == []
    assert [f for f in others if f.endswith("_bench.py") and not re.search(r"^(?:import|from) benchkit\b", others[f], re.M)] == []


def test_tensor_argument_helpers_live_in_args_only():
    others = {f: t for f, t in MGUNET.items() if f != "_args.py"}
    assert [(f, s) for f, t in others.items() for s in MGUNET_TEXTS if s in t] == []
    assert [s for s in MGUNET_TEXTS[1:] + [PERMUTE] if s not in MGUNET["_args.py"]] == []
    assert [(f, frag) for f, frag in PERMUTE_ALLOWED if frag not in others[f]] == []
    copies = []
    for f, t in others.items():
        for m in re.finditer(re.escape(PERMUTE), t):
            line = t.rfind("\n", 0, m.start()) + 1
            stop = t.find("\n", t.find("\n", m.end()) + 1)          # the end of the next line
            here = t[line:t.find("\n", m.end())]
            if "contiguous" in t[m.end():stop] and not any(f == af and frag in here for af, frag in PERMUTE_ALLOWED):
                copies.append((f, here.strip()))
    assert copies == []


def test_one_class_defines_the_evaluators_batch_preamble():
    assert [f for f, t in MGUNET.items() for _ in re.finditer(r"def _batch\(", t)] == ["metrics.py"]
    for f, cls in (("metrics.py", "SegmentationEvaluator"), ("boundary.py", "BoundaryEvaluator"), ("objects.py", "_ObjectEvaluator")):
        assert re.search(r"^class " + cls + r"\(_Evaluator\):", MGUNET[f], re.M), cls
    assert len(re.findall(r"\(_ObjectEvaluator\):", MGUNET["objects.py"] + MGUNET["instances.py"])) == 2


# ---- mgunet._args on CPU tensors ----------------------------------------------------------------------------------------------

def _args():
    from mgunet import _args
    return _args


def test_nhwc_storage_returns_the_storage_or_one_copy():
    A = _args()
    g = torch.Generator().manual_seed(0)
    stored = torch.randn((2, 5, 7, 4), generator=g)                  # NHWC storage
    view = stored.permute(0, 3, 1, 2)
    out = A.nhwc_storage(view)
    assert out.data_ptr() == stored.data_ptr() and out.shape == stored.shape and out.is_contiguous()
    nchw = torch.randn((2, 4, 5, 7), generator=g)                    # NCHW storage: one copy
    out = A.nhwc_storage(nchw)
    assert out.is_contiguous() and out.data_ptr() != nchw.data_ptr() and torch.equal(out, nchw.permute(0, 2, 3, 1))
    out = A.nhwc_storage(view[:, :2])                                # two of four channels: NHWC-strided, yet not contiguous
    assert out.is_contiguous() and out.data_ptr() != stored.data_ptr() and torch.equal(out, stored[..., :2])


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.uint8])
def test_batched_map_takes_integer_maps(dtype):
    A = _args()
    one = torch.arange(12).reshape(3, 4).to(dtype)
    out = A.batched_map(one, "a class map")
    assert out.shape == (1, 3, 4) and out.dtype == dtype and out.data_ptr() == one.data_ptr() and torch.equal(out[0], one)
    two = torch.arange(24).reshape(2, 3, 4).to(dtype)
    assert A.batched_map(two, "a class map") is two


@pytest.mark.parametrize("bad", [torch.zeros((3, 4)), torch.zeros((3, 4), dtype=torch.bool), torch.zeros(4, dtype=torch.int64),
                                 torch.zeros((1, 2, 3, 4), dtype=torch.int64)], ids=["float", "bool", "1-D", "4-D"])
def test_batched_map_refuses(bad):
    with pytest.raises(TypeError, match=r"^the target must be an integer \(H, W\) or \(B, H, W\) tensor$"):
        _args().batched_map(bad, "the target")


def test_logits_and_masks_checks_the_device_first():
    A = _args()
    bad = torch.zeros((1, 8, 8), dtype=torch.float16)                # wrong in every later respect as well
    with pytest.raises(RuntimeError, match="^logits must live on cuda:0$"):
        A.logits_and_masks(bad, torch.zeros((1, 8, 7)), torch.device("cuda:0"), 2)
    with pytest.raises(ValueError, match=r"^masks shape \(1, 8, 7\) does not match logits \(1, 8, 8\)$"):
        A.check_masks(torch.zeros((1, 8, 7)), 1, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.resolve_device("cpu", "an evaluator")
    assert A.resolve_device("cuda:1", "an evaluator") == torch.device("cuda", 1)
