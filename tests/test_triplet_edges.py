"""The cases of tests/triplet_edges.py reach the paths they are named for -- worked out from the limits the kernels were compiled with and
the host model -- and their values tell a wrong fold from the right one.  All on the CPU; tests/test_gpu_triplet_merge.py runs the cases."""
import numpy as np
import pytest

import triplet_edges as E
import triplet_model as M

# cases without a column that occurs three times in a named row: nothing for a wrong fold order to change
NO_FOLD = {"len_0", "len_1", "len_2", "dup_asc", "dup_desc", "scan_top_pass_loops"}


@pytest.fixture(scope="module")
def L(built_lib):
    return E.limits()


def _wave_total(rp, n, w):
    return int(rp[min(n, 64 * w + 64)] - rp[64 * w])


def test_limits_are_consistent(L):
    assert 2 < L.fast < L.wave == 64 and L.lds >= 64 and L.tile >= 64 and L.long_waves >= 1


@pytest.mark.parametrize("name", E.NAMES)
def test_case_reaches_its_path(name, L):
    c = E.by_name(name)
    R = c.lengths()
    rp, col, _ = c.model()
    assert len(c.raw_col) == c.raw_ptr[-1] and c.raw_ptr[0] == 0 and np.all(R >= 0)
    assert c.raw_col.min() >= 0 and c.raw_col.max() <= 2 ** 31 - 3          # INT32_MAX pads, the sign bit marks
    mag = np.abs(c.arrays()[2])
    assert mag.min() >= 2.0 ** -20 and mag.max() < 2.0 ** 21 and {-1.0, 1.0} <= set(np.sign(c.arrays()[2]).tolist())
    for r, cls in c.rows.items():
        assert E.row_class(int(R[r]), L) == cls, (r, int(R[r]), cls)
    assert int((R > L.wave).sum()) == c.long_rows
    for w, want in c.staged.items():
        assert (_wave_total(rp, c.n, w) <= L.lds) == want, (w, _wave_total(rp, c.n, w))
    for w, want in c.seg_total.items():
        assert _wave_total(rp, c.n, w) == want
    if c.more_rows_than is not None:
        assert c.n > c.more_rows_than
    if c.more_long_than is not None:
        assert c.long_rows > c.more_long_than
    assert c.rows or c.staged or c.more_rows_than is not None, "the case names nothing it reaches"
    if c.f32:   # float values, and the same pattern
        v32 = c.arrays(True)[2]
        assert np.array_equal(v32.astype(np.float32).astype(np.float64), v32)
        rp32, col32, _ = c.model(True)
        assert np.array_equal(rp32, rp) and np.array_equal(col32, col)
    else:
        assert name in E.NO_F32


def test_row_lengths_and_row_counts_sit_at_the_limits(L):
    want = (0, 1, 2, L.fast - 1, L.fast, L.fast + 1, L.wave - 1, L.wave, L.wave + 1, 2 * L.wave - 1, 2 * L.wave, 2 * L.wave + 1, 3 * L.wave + 1, 1000)
    for name, r in zip(E.LENGTHS, want):
        R = E.by_name(f"len_{name}").lengths()
        assert len(R) == 64 and R[17] == r
        others = np.delete(R, 17)
        assert others.min() >= 15 and others.max() <= 17      # a wave of ordinary rows around it
    for name, n in zip(E.ROW_COUNTS, (1, 63, 64, 65, 255, 256, 257, L.tile + 1)):
        assert E.by_name(f"rows_{name}").n == n
    big = E.by_name("scan_top_pass_loops")
    assert big.n == E.TOP_TILES * L.tile + 65 and set(big.lengths().tolist()) == {0, 1, 2}
    assert big.model()[0][-1] < len(big.raw_col)               # some rows of two hold a duplicate pair


def test_duplicate_patterns(L):
    for pattern in ("asc", "desc", "one", "adjacent", "first_last"):
        c = E.by_name(f"dup_{pattern}")
        assert sorted(c.rows.values()) == ["long", "reg", "wave"]
        for r in c.rows:
            cols, _ = c.row(r)
            if pattern == "asc":
                assert all(a < b for a, b in zip(cols, cols[1:]))
            elif pattern == "desc":
                assert all(a > b for a, b in zip(cols, cols[1:]))
            elif pattern == "one":
                assert len(set(cols)) == 1
            elif pattern == "adjacent":
                assert all(cols[k] == cols[k + 1] == cols[k + 2] for k in range(0, len(cols) - 2, 3))
            else:
                assert cols.count(cols[-1]) == 1 and cols[-1] == min(cols) and len(set(cols)) < len(cols) - 2


def test_long_chunks_layout(L):
    c = E.by_name("long_chunks")
    (r, cls), = c.rows.items()
    cols, _ = c.row(r)
    assert cls == "long" and len(cols) > 3 * L.wave
    chunk = lambda p: p // L.wave
    px = [p for p, v in enumerate(cols) if v == E.CHUNKS_X]
    py = [p for p, v in enumerate(cols) if v == E.CHUNKS_Y]
    assert chunk(px[0]) == 0 and {1, 2} <= {chunk(p) for p in px[1:]}              # first in chunk 0, duplicates in chunks 1 and 2
    assert chunk(py[0]) >= 2 and len(py) > 1 and all(v > E.CHUNKS_Y for v in cols[:py[0]])  # first in a later chunk, below everything earlier


def test_wave_compositions(L):
    c = E.by_name("wave_rows_lanes_0_30_31_63")
    assert c.rows == {0: "wave", 30: "wave", 31: "wave", 63: "wave"} and c.n == 64
    c = E.by_name("mix_all_paths")
    assert sorted(c.rows.values()) == ["long", "reg", "wave"] and c.n == 64
    assert E.by_name("long_lanes_0_63").rows == {0: "long", 63: "long"}
    assert E.by_name("two_long_adjacent").rows == {31: "long", 32: "long"}
    c = E.by_name("long_first")
    first_long = np.nonzero(c.lengths() > L.wave)[0]
    assert first_long[0] == 0 and first_long[-1] < c.n - 64     # at the start of the numbering, none in the last wave
    c = E.by_name("many_long")
    assert c.n == L.long_waves + 1 and np.all(c.lengths() == L.wave + 1)
    c = E.by_name("staged_long_few_columns")
    (r, cls), = c.rows.items()
    rp = c.model()[0]
    assert cls == "long" and rp[r + 1] - rp[r] == 3 and c.staged == {0: True}
    c = E.by_name("unstaged_wave_rows_and_long")
    assert sorted(c.rows.values()) == ["long", "wave", "wave"] and c.staged == {0: False}
    c = E.by_name("big_columns")
    assert sorted(c.rows.values()) == ["long", "reg", "wave"]
    for r in c.rows:
        cols, _ = c.row(r)
        assert min(cols) == 2 ** 30 and max(cols) == 2 ** 31 - 3
    assert c.raw_col.min() >= 2 ** 30


@pytest.mark.parametrize("name", E.NAMES)
def test_wrong_folds_change_bits(name, L):
    """the model with the fold reversed, and for f32 the model that accumulates in fp64 and rounds once, differ in bits from the model in
    every row a case names for folding -- so a kernel with either error cannot pass the case"""
    c = E.by_name(name)
    assert bool(c.fold_rows) == (name not in NO_FOLD)
    for f32 in ((False, True) if c.f32 else (False,)):
        for r in c.fold_rows:
            cols, vals = c.row(r, f32)
            want = M.merge_row(cols, vals, f32)
            for fold in (("right", "once") if f32 else ("right",)):
                got = M.merge_row(cols, vals, f32, fold)
                assert got[0] == want[0]
                assert not np.array_equal(M.bits(got[1]), M.bits(want[1])), (name, r, f32, fold)
