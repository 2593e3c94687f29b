"""Host model of Eigen::SparseMatrix::setFromTriplets as the assembly performs it per row (csrc/avs_assembly.hip, K6b + K7; the oracle's
compress_row): stable sort by column, then the duplicates of a column folded LEFT TO RIGHT in emission order -- in fp64, or in float steps
((float)a + (float)b, widened) for SolveType = fpreal32.

Every addition is one scalar operation on Python / NumPy scalars, so the order is the one written here (np.sum and np.add.reduceat do not
define theirs).  `fold` selects the model ("left") or one of the two planted errors tests/test_triplet_edges.py uses to show that a case's
values can tell a wrong kernel from a right one: "right" folds a column's entries from the last to the first, "once" (f32 only) accumulates
in fp64 and rounds to float once.
"""
import numpy as np

FOLDS = ("left", "right", "once")


def _add32(a, b):
    return float(np.float32(a) + np.float32(b))


def fold_column(vals, f32=False, fold="left"):
    """the entries of one column, in emission order -> the merged value (a Python float holding an fp64, or a float value for f32)"""
    if fold == "right":
        vals = vals[::-1]
    acc = vals[0]
    if f32 and fold != "once":
        for v in vals[1:]:
            acc = _add32(acc, v)
        return acc
    for v in vals[1:]:
        acc = acc + v
    return float(np.float32(acc)) if f32 and len(vals) > 1 else acc


def merge_row(cols, vals, f32=False, fold="left"):
    """one row's raw triplets (lists, emission order) -> (columns ascending, merged values)"""
    order = sorted(range(len(cols)), key=cols.__getitem__)   # stable: equal columns stay in emission order
    out_c, out_v = [], []
    k = 0
    while k < len(order):
        c = cols[order[k]]
        run = []
        while k < len(order) and cols[order[k]] == c:
            run.append(vals[order[k]])
            k += 1
        out_c.append(c)
        out_v.append(fold_column(run, f32, fold))
    return out_c, out_v


def merge(raw_ptr, raw_col, raw_val, f32=False, fold="left"):
    """raw_ptr[n + 1], raw_col, raw_val (triplets grouped by row, emission order) -> (row_ptr int64, col int32, val float64)"""
    assert fold in FOLDS and (f32 or fold != "once")
    ptr = np.asarray(raw_ptr).tolist()
    cols = np.asarray(raw_col).tolist()
    vals = np.asarray(raw_val, dtype=np.float64).tolist()
    n = len(ptr) - 1
    row_ptr = [0] * (n + 1)
    out_c, out_v = [], []
    for r in range(n):
        a, b = ptr[r], ptr[r + 1]
        if b - a == 1:
            out_c.append(cols[a])
            out_v.append(vals[a])
        elif b > a:
            c, v = merge_row(cols[a:b], vals[a:b], f32, fold)
            out_c += c
            out_v += v
        row_ptr[r + 1] = len(out_c)
    return np.array(row_ptr, np.int64), np.array(out_c, np.int32).reshape(-1), np.array(out_v, np.float64).reshape(-1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
