"""Host side of tiled inference (mgunet.tiled.tile_grid / tile_weights, the four mgu_tile_* symbols): the grid against a brute-force
restatement, the normalised window against its definition, and the C-ABI's declaration, binding and export.  No GPU."""
import os
import re

import numpy as np
import pytest

import mgunet
import tiled_oracle as TO
from mgunet import _lib
from mgunet import tiled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mgu_tile_gather", "mgu_tile_gather_u8", "mgu_tile_accumulate", "mgu_tile_finish"]

# (L, T, o): L < T, L == T, L == T + 1, o == 0, a shifted last tile, an exact fit, a stride of one
SWEEP = [(L, T, o) for T, os_ in ((8, (0, 1, 3, 7)), (16, (0, 4, 5, 15)), (96, (0, 32, 33)), (512, (0, 64, 100)))
         for o in os_ for L in sorted({1, 2, T - 1, T, T + 1, T + (T - o), T + (T - o) + 1, 2 * T, 2 * T + 3, 3 * T - 2 * o, 5 * T // 2 + 1})]


def test_origins_from_the_issue():
    assert mgunet.tile_grid(1200, 513, 512, 64) == ([0, 448, 688], [0, 1])
    assert mgunet.tile_grid(300, 512, 512, 64) == ([0], [0])
    assert mgunet.tile_grid(200, 264, (96, 128), 32) == ([0, 64, 104], [0, 96, 136])


@pytest.mark.parametrize("L,T,o", SWEEP)
def test_grid_matches_brute_force(L, T, o):
    oy, ox = mgunet.tile_grid(L, L, T, o)
    ref = TO.axis_origins(L, T, o)
    assert oy == ref and ox == ref
    assert oy[0] == 0 and oy[-1] == max(0, L - T)
    assert all(b > a for a, b in zip(oy, oy[1:]))
    assert all(b - a <= T - o for a, b in zip(oy, oy[1:]))           # no gap wider than the stride, so ...
    assert TO.coverage(L, T, oy).min() >= 1                          # ... every pixel is covered
    assert len(oy) == (1 if L <= T else -(-(L - T) // (T - o)) + 1)


@pytest.mark.parametrize("window", ["ramp", "flat"])
@pytest.mark.parametrize("L,T,o", SWEEP)
def test_weights(L, T, o, window):
    org = TO.axis_origins(L, T, o)
    w = mgunet.tile_weights(L, T, o, org, window)
    assert w.shape == (len(org), T) and w.dtype == np.float32
    total, cover = np.zeros(max(L, T)), TO.coverage(max(L, T), T, org)
    for k, y in enumerate(org):
        total[y:y + T] += w[k].astype(np.float64)
        assert np.all(w[k][cover[y:y + T] == 1] == np.float32(1.0))   # one tile: exactly 1
    assert np.all(w > 0)
    assert np.abs(total[:L] - 1.0).max() <= 2.0 ** -23               # 1 fp32 ulp at 1.0
    ref = TO.axis_weights(L, T, o, org, window)                       # the float64 definition, rounded once
    assert np.abs(w.astype(np.float64) - ref.astype(np.float64)).max() <= 2.0 ** -24


@pytest.mark.parametrize("L,T,o", [(1200, 512, 64), (264, 96, 32), (40, 16, 5), (100, 32, 16)])
def test_regular_ramp_seam(L, T, o):
    """Between two unshifted neighbours (origins k S and (k + 1) S) that alone cover a coordinate, the right tile's weight is
    (i + 1) / (o + 1) and the left one's (o - i) / (o + 1), each rounded to fp32."""
    org = TO.axis_origins(L, T, o)
    w = mgunet.tile_weights(L, T, o, org, "ramp")
    cover, S, seen = TO.coverage(L, T, org), T - o, 0
    for k in range(len(org) - 1):
        if org[k + 1] - org[k] != S:
            continue
        for i in range(o):
            if cover[org[k + 1] + i] != 2:
                continue
            assert w[k + 1][i] == np.float32((i + 1) / (o + 1))
            assert w[k][S + i] == np.float32((o - i) / (o + 1))
            seen += 1
    assert seen > 0


def test_weight_and_grid_refusals():
    with pytest.raises(ValueError):
        mgunet.tile_grid(100, 100, 32, 32)
    with pytest.raises(ValueError):
        mgunet.tile_grid(100, 100, (64, 16), 16)
    with pytest.raises(ValueError):
        mgunet.tile_grid(100, 100, 32, -1)
    with pytest.raises(ValueError):
        mgunet.tile_grid(0, 100, 32, 4)
    with pytest.raises(ValueError):
        mgunet.tile_weights(100, 32, 4, [0, 28, 56, 68], "hann")
    with pytest.raises(ValueError):
        mgunet.tile_weights(100, 32, 32, [0], "ramp")


def test_python_names_are_exported():
    for n in ("predict_tiled", "tile_grid", "tile_weights"):
        assert callable(getattr(mgunet, n)) and n in mgunet.__all__
    assert tiled.WINDOWS == ("ramp", "flat")


def test_new_symbols_declared_bound_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mgunet.h")).read(), flags=re.S)
    L = _lib.lib()
    for s in NEW:
        assert re.search(rf"\b{s}\s*\(", txt), s
        assert s in _lib._PROTOS and _lib._PROTOS[s][2], s          # declared, and takes the stream last
        assert hasattr(L, s), s


def test_entries_reject_a_null_context():
    L = _lib.lib()
    assert L.mgu_tile_gather(None, None, 1, 1, 1, 1, None, 1, 1, 0, 0, 0, 1, None, None) == _lib.MGU_ERR_INVALID
    assert L.mgu_tile_gather_u8(None, None, 1, 1, 1, 0, None, None, 1, 1, 0, 0, 0, 1, None, None) == _lib.MGU_ERR_INVALID
    assert L.mgu_tile_accumulate(None, None, 0, 1, 1, 1, 1, 1, 1, 0, 0, None, None, 0, 1, None, None, None, None) == _lib.MGU_ERR_INVALID
    assert L.mgu_tile_finish(None, None, 1, 1, 1, 1, None, None, None) == _lib.MGU_ERR_INVALID

