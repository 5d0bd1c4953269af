"""CPU side of tests/test_gpu_train_blocks.py: the figure that sizes its offset-channel inputs, R_OBS, recomputed from the float64
oracle.  The 4 x 512^2 shard, whose 5.06 / 5.14 set R_OBS, takes a minute on the CPU and is left to `python
tests/test_train_blocks_host.py f`; the 2 x 128^2 shard is checked here, before and after the golden step."""
import sys

import pytest
import torch

import mgunet_oracle as O
from test_gpu_train_blocks import R_OBS

CFG = (3, 2, 32, 4)
SHARDS = {"s": (2, 3, 128, 128), "f": (4, 3, 512, 512)}


def shard_ratios(tag):
    """max |mean| / std of z over the network, with the golden step's initial parameters and after its Adam step."""
    shape = SHARDS[tag]
    x = torch.from_numpy(O.formula_normal(f"c5/{tag}/x", shape, seed=4)).double()
    y = torch.from_numpy(O.formula_labels(f"c5/{tag}/y", (shape[0], shape[2], shape[3]), 2, seed=5))
    p = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in O.make_unet_params(*CFG, seed=0).items()}
    before = O.bn_input_ratio(p, x, CFG[3])
    newp = O.train_step(p, x, y, depth=CFG[3])[2]
    return before, O.bn_input_ratio(newp, x, CFG[3])


def test_observed_offset_ratio_of_the_small_shard():
    before, after = shard_ratios("s")
    print(f"[r_obs s] before {before:.3f} after {after:.3f} (R_OBS {R_OBS})")
    assert before == pytest.approx(4.60, abs=0.01) and after == pytest.approx(4.53, abs=0.01)   # NOTES.md "Train-forward block"
    assert max(before, after) <= R_OBS


if __name__ == "__main__":
    for t in sys.argv[1:] or list(SHARDS):
        b, a = shard_ratios(t)
        print(f"{t}: before {b:.3f} after {a:.3f} R_OBS {R_OBS}")
        assert round(max(b, a), 2) <= R_OBS   # R_OBS is the figure to two decimals
