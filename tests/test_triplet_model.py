"""tests/triplet_model.py pinned: hand-written known answers where the order of the fold matters, and idempotence on the merged CSR of the
golden fixtures (the oracle library does not expose its raw triplets per row, so the fixtures cannot feed the model raw input)."""
import glob
import os

import numpy as np
import pytest

import triplet_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "*.npz")))


def test_left_fold_in_emission_order():
    vals = [1e16, 1.0, -1e16, 1.0]
    assert M.fold_column(vals) == 1.0                      # ((1e16 + 1) - 1e16) + 1: the first 1 is absorbed, the last survives
    assert M.fold_column(vals, fold="right") == 0.0        # ((1 - 1e16) + 1) + 1e16
    assert M.fold_column([1e16, -1e16, 1.0, 1.0]) == 2.0
    assert M.fold_column([3.5]) == 3.5


def test_float_steps():
    big = 2.0 ** 24
    assert M.fold_column([big, 1.0, 1.0], f32=True) == big                  # each float step ties to even
    assert M.fold_column([big, 1.0, 1.0], f32=True, fold="once") == big + 2  # fp64 sum, rounded once
    assert M.fold_column([1.0, 1.0, big], f32=True) == big + 2
    assert M.fold_column([big, 1.0, 1.0]) == big + 2                        # fp64
    assert M.fold_column([0.1], f32=True) == 0.1                            # a single entry is stored as it came
    a, b = float(np.float32(0.1)), float(np.float32(0.2))
    assert M.fold_column([a, b], f32=True) == float(np.float32(np.float32(0.1) + np.float32(0.2))) != a + b


def test_stable_sort_by_column():
    # columns 2 and 1 interleaved: each column keeps its emission order
    cols, vals = M.merge_row([2, 1, 2, 1, 2], [1e16, 5.0, 1.0, 7.0, -1e16])
    assert cols == [1, 2] and vals == [12.0, 0.0]
    cols, vals = M.merge_row([2, 1, 2, 1, 2], [1e16, 5.0, -1e16, 7.0, 1.0])
    assert cols == [1, 2] and vals == [12.0, 1.0]
    cols, vals = M.merge_row([9, 3, 2 ** 31 - 3, 0], [1.0, 2.0, 3.0, 4.0])
    assert cols == [0, 3, 9, 2 ** 31 - 3] and vals == [4.0, 2.0, 1.0, 3.0]


def test_rows_and_pointers():
    #            row 0: empty | row 1: one entry | row 2: a cancelling pair stays, as a zero | row 3: empty
    ptr, col, val = [0, 0, 1, 5, 5], [4, 8, 6, 8, 6], [0.5, 2.0, -3.0, -2.0, 1.0]
    rp, c, v = M.merge(ptr, col, val)
    assert rp.tolist() == [0, 0, 1, 3, 3] and rp.dtype == np.int64
    assert c.tolist() == [4, 6, 8] and c.dtype == np.int32
    assert v.tolist() == [0.5, -2.0, 0.0] and v.dtype == np.float64
    rp, c, v = M.merge([0], [], [])
    assert rp.tolist() == [0] and len(c) == 0 and len(v) == 0


def test_fixtures_exist():
    assert len(FIXTURES) == 3


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p) for p in FIXTURES])
def test_idempotent_on_golden_csr(path):
    g = np.load(path)
    for f32 in (False, True):
        val = g["val"].astype(np.float32).astype(np.float64) if f32 else g["val"]
        rp, col, v = M.merge(g["row_ptr"], g["col"], val, f32=f32)
        assert np.array_equal(rp, g["row_ptr"]) and np.array_equal(col, g["col"])
        assert np.array_equal(M.bits(v), M.bits(val))
