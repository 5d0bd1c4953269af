"""Host side of the graph-branch inputs (mgunet.patch_node_features / patch_labels / E2ETrainer.step_images, the two mgu_patch_*
symbols): declaration, binding and export, the refusal of CPU tensors, and the numpy label-vote oracle the GPU tests compare against,
on hand-made cases.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import mgunet
import patch_inputs_oracle as PO
from mgunet import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mgu_patch_node_features_u8", "mgu_patch_labels"]


def test_new_symbols_declared_bound_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mgunet.h")).read(), flags=re.S)
    L = _lib.lib()
    for s in NEW:
        assert re.search(rf"\b{s}\s*\(", txt), s
        assert s in _lib._PROTOS and _lib._PROTOS[s][2], s          # declared, and takes the stream last
        assert hasattr(L, s), s


def test_entries_reject_a_null_context():
    L = _lib.lib()
    assert L.mgu_patch_node_features_u8(None, None, 1, 1, 1, 1, None, 0, 0, 0, 0, 0, None, 0, 1, None, 4, None) == _lib.MGU_ERR_INVALID
    assert L.mgu_patch_labels(None, None, 0, 1, 1, 1, 2, 1, None, None, None, None) == _lib.MGU_ERR_INVALID


def test_python_names_are_exported():
    for n in ("patch_node_features", "patch_labels"):
        assert callable(getattr(mgunet, n)) and n in mgunet.__all__
    assert callable(mgunet.E2ETrainer.step_images)


def test_cpu_tensors_are_refused():
    """the package's usual error: RuntimeError, "runs only on a HIP device" (there is no CPU fallback)"""
    u8 = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(RuntimeError, match="HIP device"):
        mgunet.patch_node_features(u8, 4, images=torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match="HIP device"):
        mgunet.patch_node_features(u8, 4, unet_patch_feats=torch.zeros(4, 8))
    with pytest.raises(RuntimeError, match="HIP device"):
        mgunet.patch_labels(torch.zeros(1, 8, 8, dtype=torch.int64), 4, 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        mgunet.patch_labels(torch.zeros(1, 2, 8, 8), 4)


def test_oracle_two_by_two_tie():
    lab, cnt, pur = PO.patch_label_vote(np.array([[0, 1], [1, 0]]), 2, 2)
    assert lab.tolist() == [0] and cnt.tolist() == [[2, 2]] and pur.dtype == np.float32 and pur.tolist() == [0.5]


def test_oracle_patch_that_is_partly_padding():
    """3 x 5 map, patch 2: the right column of patches is one pixel wide, the bottom row one pixel high, the corner a single pixel;
    purity divides by the REAL pixels"""
    m = np.array([[0, 0, 1, 1, 2],
                  [0, 1, 1, 1, 2],
                  [2, 2, 0, 1, 1]])
    lab, cnt, pur = PO.patch_label_vote(m, 2, 3)
    assert lab.tolist() == [0, 1, 2, 2, 0, 1]
    assert cnt.tolist() == [[3, 1, 0], [0, 4, 0], [0, 0, 2], [0, 0, 2], [1, 1, 0], [0, 1, 0]]
    assert pur.tolist() == [np.float32(0.75), 1.0, 1.0, 1.0, 0.5, 1.0]
    assert PO.patch_grid(3, 5, 2) == (2, 3)


def test_oracle_out_of_range_values():
    m = np.array([[-100, 7, 1, 1],
                  [7, -1, 7, 0]])
    lab, cnt, pur = PO.patch_label_vote(m, 2, 2)
    assert lab.tolist() == [0, 1] and cnt.tolist() == [[0, 0], [1, 2]]      # only out-of-range values: label 0, purity 0
    assert pur.tolist() == [0.0, 0.5]                                        # the dropped 7 still counts as a real pixel


def test_oracle_three_way_tie_and_pixel_mean():
    lab, cnt, _ = PO.patch_label_vote(np.array([[2, 1, 3], [3, 2, 1]]), 3, 4)
    assert lab.tolist() == [1] and cnt.tolist() == [[0, 2, 2, 2]]
    x = np.arange(3 * 3 * 5, dtype=np.float64).reshape(3, 3, 5)
    m = PO.patch_pixel_mean(x, 2)
    assert m.shape == (6,)
    assert m[0] == x[:, :2, :2].sum() / 12 and m[2] == x[:, :2, 4:].sum() / 12 and m[5] == x[:, 2:, 4:].sum() / 12
