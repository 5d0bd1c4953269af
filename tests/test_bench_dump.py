"""bench.py --dump-outputs, the host side (CPU only): what dump_arrays keeps of a step's outputs -- whole arrays up to
DUMP_FULL_MAX elements, a seeded sample of larger ones at the same positions on every call, float32 / float64 only, and the
64 MiB budget."""
import numpy as np
import pytest
import torch

import bench


def test_small_arrays_are_written_whole_in_float32_or_float64():
    lg = torch.randn(2, 5, 3, 4).permute(0, 3, 1, 2)          # a strided view, as the forward returns its NHWC storage
    d = bench.dump_arrays([("lg", lg), ("h", torch.randn(6, 7, dtype=torch.bfloat16)), ("d", torch.randn(3, dtype=torch.float64)),
                           ("loss", torch.tensor(0.25))])
    assert d["lg"].dtype == np.float32 and d["lg"].shape == (2, 4, 5, 3) and np.array_equal(d["lg"], lg.numpy())
    assert d["h"].dtype == np.float32                          # bf16 -> fp32 is exact
    assert d["d"].dtype == np.float64 and d["loss"].shape == () and float(d["loss"]) == 0.25


def test_large_arrays_are_sampled_at_fixed_positions():
    t = torch.arange(5 * (bench.DUMP_FULL_MAX // 5 + 1000), dtype=torch.float32).reshape(-1, 5)
    view = t.t()                                               # non-contiguous: flat index order is the caller's view
    a = bench.dump_arrays([("big", view)])["big"]
    b = bench.dump_arrays([("big", view.contiguous())])["big"]
    c = bench.dump_arrays([("other", view)])["other"]
    assert a.shape == (bench.DUMP_SAMPLE,) and a.dtype == np.float32
    assert np.array_equal(a, b)                                # same name and shape: same positions
    assert not np.array_equal(a, c)                            # the seed is the name
    # the values are the storage offsets (exact in fp32): map them back to flat positions in the view's order
    flat = view.contiguous().reshape(-1).numpy().astype(np.int64)
    where = np.empty_like(flat)
    where[flat] = np.arange(flat.size)
    pos = where[a.astype(np.int64)]
    assert (np.diff(pos) > 0).all()                            # distinct positions, in increasing order
    assert np.array_equal(pos, np.sort(np.random.default_rng(bench.zlib.crc32(b"big")).choice(flat.size, bench.DUMP_SAMPLE, replace=False)))


def test_budget_is_enforced():
    many = [(f"x{i}", torch.zeros(bench.DUMP_FULL_MAX)) for i in range(bench.DUMP_MAX_BYTES // (4 * bench.DUMP_FULL_MAX) + 1)]
    with pytest.raises(AssertionError):
        bench.dump_arrays(many)


def test_write_dump_round_trip(tmp_path):
    arrays = bench.dump_arrays([("logits", torch.randn(2, 2, 8, 8)), ("node_embeddings", torch.randn(4, 3))])
    bench.write_dump(str(tmp_path / "out"), arrays)
    for k, v in arrays.items():
        assert np.array_equal(np.load(tmp_path / "out" / (k + ".npy")), v)
