"""Named CSR systems for avs_check_csr: clean ones, the matrices of tests/csr_edges.py as found, and planted ones -- one edit of a clean
system each, with the rule counts that edit must change (`expect`: rule -> count; every other count stays 0).

Corrupt systems are only ever read by the checker (and by the NumPy model): nothing here is handed to a solver.

Where the edges lie (csrc/avs_csr_check.hip): a row has a group of 16 lanes, four rows per wave, 16 rows per workgroup; longer rows loop;
grids stop growing at 2048 workgroups (32768 rows a trip).  So: row lengths 0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65 and one of 10,000
(`blocks`, `arrow`; length 0 in `empty_rows` and the planted `diag_removed_*` of `tri_1`), n = 1, 3, 4, 5, 63, 64, 65 (`tri_*`), and a
violation in the first and in the last wave of a grid, small (`tri_65`) and full (`tri_40000`: rows 0, 32767 and 39999).
"""
from __future__ import annotations

import functools

import numpy as np

import csr_edges
from csr_check_model import (ALL, COLUMN, DIAGONAL_RULE, ORDER_RULE, PATTERN, ROW_PTR, SYMMETRY_RULE, VALUE, VECTOR)

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
AS_FOUND = ("unsorted_repeated", "long_row", "empty_rows", "specials", "n_1", "n_3", "n_513", "random_cols")


class System:
    def __init__(self, name, row_ptr, col, val, b=None, x=None, tol=0.0, expect=None, base=None):
        self.name = name
        self.row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self.val = np.ascontiguousarray(val, dtype=np.float64)
        self.n, self.nnz = len(self.row_ptr) - 1, len(self.col)
        self.b = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
        self.x = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
        self.tol = tol          # the symmetry tolerance the case is checked with
        self.expect = expect    # planted: {rule: count}, every other count 0
        self.base = base        # planted: the clean system it was made from

    def __repr__(self):
        return f"System({self.name}, n={self.n}, nnz={self.nnz})"

    def edited(self, name, expect, **changes):
        f = dict(row_ptr=self.row_ptr.copy(), col=self.col.copy(), val=self.val.copy(), b=None if self.b is None else self.b.copy(),
                 x=None if self.x is None else self.x.copy(), tol=self.tol)
        f.update(changes)
        return System(name, expect=expect, base=self.name, **f)


def _vectors(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n), rng.standard_normal(n)


def _from_entries(name, n, rows, cols, seed):
    """a symmetric pattern (every (i, j) comes with (j, i) and every row has its diagonal) -> rows ascending, off-diagonal values
    -(0.25 + (1 + (i + j) % 8) / 32) in [-0.5, -0.28125] (exact, the same for (i, j) and (j, i), and one step towards zero is 2^-54 for
    all of them), diagonal = the number of entries of the row: strictly dominant"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    counts = np.bincount(rows, minlength=n)
    val = -(0.25 + (1 + (rows + cols) % 8) / 32.0)
    val[rows == cols] = counts[rows[rows == cols]].astype(np.float64)   # 1 + (count - 1)
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(counts)
    b, x = _vectors(n, seed)
    return System(name, rp, cols, val, b, x)


def tridiagonal(n):
    i = np.arange(n)
    return _from_entries(f"tri_{n}", n, np.concatenate([i, i[1:], i[:-1]]), np.concatenate([i, i[:-1], i[1:]]), 7000 + n)


def blocks():
    """dense diagonal blocks: every row of a block of size L has L entries"""
    rows, cols, at = [], [], 0
    for size in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65):
        i, j = np.meshgrid(np.arange(at, at + size), np.arange(at, at + size), indexing="ij")
        rows.append(i.ravel())
        cols.append(j.ravel())
        at += size
    return _from_entries("blocks", at, np.concatenate(rows), np.concatenate(cols), 7100)


def arrow(n=10000):
    """row 0 holds all n columns, row j > 0 holds (j, 0) and (j, j)"""
    j = np.arange(1, n)
    return _from_entries("arrow", n, np.concatenate([np.zeros(n, dtype=np.int64), j, j]), np.concatenate([np.arange(n), np.zeros(n - 1, dtype=np.int64), j]), 7200)


@functools.lru_cache(maxsize=None)
def _edge_cases():
    return {c.name: c for c in csr_edges.cases()}


SPD_NAMES = ["spd_" + name for name in csr_edges.SPD_NAMES]
SMALL_CLEAN_NAMES = [f"tri_{n}" for n in (1, 3, 4, 5, 63, 64, 65, 40000)] + ["blocks", "arrow", "n_0"]
CLEAN_NAMES = SPD_NAMES + SMALL_CLEAN_NAMES
AS_FOUND_NAMES = ["raw_" + name for name in AS_FOUND] + ["several"]


@functools.lru_cache(maxsize=None)
def clean_system(name):
    """a System that passes every rule with asymmetric_entries == 0"""
    if name.startswith("spd_"):
        rp, col, val, b = csr_edges.spd_version(_edge_cases()[name[4:]])
        return System(name, rp, col, val, b, np.zeros(len(b)))
    if name.startswith("tri_"):
        return tridiagonal(int(name[4:]))
    return {"blocks": blocks, "arrow": arrow, "n_0": lambda: System("n_0", [0], [], [])}[name]()


def clean(names=CLEAN_NAMES):
    return {name: clean_system(name) for name in names}


@functools.lru_cache(maxsize=None)
def as_found_system(name):
    """the raw csr_edges matrices: unordered, unsymmetric, with specials -- their counts are whatever the model says"""
    if name.startswith("raw_"):
        c = _edge_cases()[name[4:]]
        b, x = _vectors(c.n, 7300 + c.n)
        return System(name, c.row_ptr, c.col, c.val, b, x)
    # several rules at once, to pin `first_*`: an overwritten column (rules 1 and 6, and 4 behind it), a NaN off the diagonal, a bad b
    assert name == "several"
    t = tridiagonal(65)
    col, val, b = t.col.copy(), t.val.copy(), t.b.copy()
    col[t.row_ptr[40]] = INT32_MAX
    val[t.row_ptr[20] + 2] = np.nan
    b[3] = np.inf
    return System("several", t.row_ptr, col, val, b, t.x)


def as_found():
    return {name: as_found_system(name) for name in AS_FOUND_NAMES}


def _row_of(s, k):
    return int(np.searchsorted(s.row_ptr, k, side="right")) - 1


def _insert(s, row, k, c, v):
    """entry (c, v) of `row` put at position k (row_ptr[row] <= k <= row_ptr[row + 1])"""
    assert s.row_ptr[row] <= k <= s.row_ptr[row + 1]
    rp = s.row_ptr.astype(np.int64)
    rp[row + 1:] += 1
    return dict(row_ptr=rp, col=np.insert(s.col.astype(np.int64), k, c), val=np.insert(s.val, k, v))


def _delete(s, k):
    row = _row_of(s, k)
    rp = s.row_ptr.astype(np.int64)
    rp[row + 1:] -= 1
    return dict(row_ptr=rp, col=np.delete(s.col, k), val=np.delete(s.val, k))


def _swap(s, k):
    """entries k and k + 1 exchanged, values with them: the same matrix, one row out of order"""
    col, val = s.col.copy(), s.val.copy()
    col[[k, k + 1]] = col[[k + 1, k]]
    val[[k, k + 1]] = val[[k + 1, k]]
    return dict(col=col, val=val)


def _diag_entry(s, row):
    k0, k1 = int(s.row_ptr[row]), int(s.row_ptr[row + 1])
    return k0 + int(np.flatnonzero(s.col[k0:k1] == row)[0])


def _off_diagonal(s, k):
    """the first entry at or behind k that is off the diagonal"""
    while s.col[k] == _row_of(s, k):
        k += 1
    return k


def _partner(s, k):
    row = _row_of(s, k)
    j = int(s.col[k])
    k0, k1 = int(s.row_ptr[j]), int(s.row_ptr[j + 1])
    return k0 + int(np.flatnonzero(s.col[k0:k1] == row)[0])


@functools.lru_cache(maxsize=None)
def planted():
    """name -> System, made from the small clean systems only (cheap enough to build when tests are collected)"""
    out = []
    C = clean(SMALL_CLEAN_NAMES)
    t65, t5, blk, big = C["tri_65"], C["tri_5"], C["blocks"], C["tri_40000"]

    def rp_edit(s, index, value):
        rp = s.row_ptr.astype(np.int64)
        rp[index] = value
        return dict(row_ptr=rp)

    # rule 0
    for s in (t65, blk):
        mid = s.n // 2
        out.append(s.edited(f"{s.name}_rp_first", {ROW_PTR: 1}, **rp_edit(s, 0, 1)))
        out.append(s.edited(f"{s.name}_rp_last_short", {ROW_PTR: 1}, **rp_edit(s, s.n, s.nnz - 1)))
        out.append(s.edited(f"{s.name}_rp_last_long", {ROW_PTR: 1}, **rp_edit(s, s.n, s.nnz + 1)))
        out.append(s.edited(f"{s.name}_rp_decreasing", {ROW_PTR: 1}, **rp_edit(s, mid, int(s.row_ptr[mid + 1]) + 1)))
        out.append(s.edited(f"{s.name}_rp_negative", {ROW_PTR: 2}, **rp_edit(s, mid, -1)))             # index mid, and mid - 1 > it
        out.append(s.edited(f"{s.name}_rp_int32_min", {ROW_PTR: 2}, **rp_edit(s, mid, INT32_MIN)))
        out.append(s.edited(f"{s.name}_rp_over_nnz", {ROW_PTR: 1}, **rp_edit(s, mid, s.nnz + 5)))
        out.append(s.edited(f"{s.name}_rp_int32_max", {ROW_PTR: 1}, **rp_edit(s, mid, INT32_MAX)))
    out.append(C["tri_1"].edited("tri_1_rp_first", {ROW_PTR: 1}, **rp_edit(C["tri_1"], 0, 1)))
    out.append(C["n_0"].edited("n_0_rp_nonzero", {ROW_PTR: 1}, **rp_edit(C["n_0"], 0, 1)))

    # rule 1: an entry more, placed so that its row stays ascending (low columns at a row's start, high ones at its end) -- the pattern
    # and the order of everything else is as before
    for s in (t65, blk, big):
        mid, last = s.n // 2, s.n - 1
        start, end = int(s.row_ptr[mid]), int(s.row_ptr[mid + 1])
        for tag, row, k, c in (("minus1_first", 0, 0, -1), ("int32_min_first", 0, 0, INT32_MIN), ("n_last", last, s.nnz, s.n),
                               ("int32_max_last", last, s.nnz, INT32_MAX), ("minus1_row_start", mid, start, -1),
                               ("int32_min_row_start", mid, start, INT32_MIN), ("n_row_end", mid, end, s.n), ("int32_max_row_end", mid, end, INT32_MAX)):
            out.append(s.edited(f"{s.name}_col_{tag}", {COLUMN: 1}, **_insert(s, row, k, c, -0.5)))
    # the last row of the first trip of a full grid
    out.append(big.edited("tri_40000_col_minus1_row_32767", {COLUMN: 1}, **_insert(big, 32767, int(big.row_ptr[32767]), -1, -0.5)))

    # rules 2 and 3
    for s in (t65, big):
        ks = (1, int(s.row_ptr[s.n // 2]) + 0, s.nnz - 2) + ((int(s.row_ptr[32767]),) if s is big else ())   # off the diagonal
        for tag, bad in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf)):
            for k in ks:
                assert s.col[k] != _row_of(s, k)
                val = s.val.copy()
                val[k] = bad
                out.append(s.edited(f"{s.name}_val_{tag}_{k}", {VALUE: 1}, val=val))
            for row in (0, s.n // 2, s.n - 1):
                for which in ("b", "x"):
                    vec = getattr(s, which).copy()
                    vec[row] = bad
                    out.append(s.edited(f"{s.name}_{which}_{tag}_{row}", {VECTOR: 1}, **{which: vec}))
    b, x = t65.b.copy(), t65.x.copy()
    b[7], x[7] = np.nan, np.inf
    out.append(t65.edited("tri_65_b_and_x_row_7", {VECTOR: 1}, b=b, x=x))   # a row counts once

    # rule 4: the same matrix with two neighbours exchanged, or an entry stored twice
    for s in (t65, blk, C["arrow"]):
        for row in (1 if s is blk else 0, s.n // 2, s.n - 1):   # (row 0 of `blocks` has one entry)
            k0, k1 = int(s.row_ptr[row]), int(s.row_ptr[row + 1])
            assert k1 - k0 >= 2
            out.append(s.edited(f"{s.name}_swap_start_{row}", {ORDER_RULE: 1}, **_swap(s, k0)))
            out.append(s.edited(f"{s.name}_swap_end_{row}", {ORDER_RULE: 1}, **_swap(s, k1 - 2)))
            out.append(s.edited(f"{s.name}_repeat_start_{row}", {ORDER_RULE: 1}, **_insert(s, row, k0 + 1, int(s.col[k0]), float(s.val[k0]))))
            out.append(s.edited(f"{s.name}_repeat_end_{row}", {ORDER_RULE: 1}, **_insert(s, row, k1, int(s.col[k1 - 1]), float(s.val[k1 - 1]))))

    # rule 5
    for s in (t65, blk, big, C["tri_1"]):
        for row in sorted({0, s.n - 1}):
            k = _diag_entry(s, row)
            out.append(s.edited(f"{s.name}_diag_removed_{row}", {DIAGONAL_RULE: 1}, **_delete(s, k)))
            for tag, bad, more in (("zero", 0.0, {}), ("negative", -2.0, {}), ("nan", np.nan, {VALUE: 1})):
                val = s.val.copy()
                val[k] = bad
                out.append(s.edited(f"{s.name}_diag_{tag}_{row}", {DIAGONAL_RULE: 1, **more}, val=val))
    # the LAST entry with col == row decides: a good diagonal behind a bad one passes rule 5, a bad one behind a good one does not
    # (two entries with the row's own column are rule 4's as well)
    k = _diag_entry(t5, 2)
    twice = _insert(t5, 2, k + 1, 2, 3.0)
    twice["val"][k] = -1.0
    out.append(t5.edited("tri_5_diag_twice_last_good", {ORDER_RULE: 1}, **twice))
    out.append(t5.edited("tri_5_diag_twice_last_bad", {ORDER_RULE: 1, DIAGONAL_RULE: 1}, **_insert(t5, 2, k + 1, 2, -1.0)))

    # rules 6 and 7
    ulp = 2.0 ** -54   # one step towards zero from a value in [-0.5, -0.25)
    for s in (t65, blk, big, C["arrow"]):
        for k in sorted({_off_diagonal(s, 1), _off_diagonal(s, int(s.row_ptr[s.n // 2])), _off_diagonal(s, s.nnz - 2)}):
            out.append(s.edited(f"{s.name}_pair_deleted_{k}", {PATTERN: 1}, **_delete(s, _partner(s, k))))
            val = s.val.copy()
            assert -0.5 <= val[k] < -0.25
            val[k] = np.nextafter(val[k], 0.0)
            assert abs(val[k] - s.val[k]) == ulp
            out.append(s.edited(f"{s.name}_ulp_above_tol_{k}", {SYMMETRY_RULE: 2}, val=val, tol=ulp / 2))   # both entries of the pair
            out.append(s.edited(f"{s.name}_ulp_equal_tol_{k}", {}, val=val, tol=ulp))
            out.append(s.edited(f"{s.name}_ulp_below_tol_{k}", {}, val=val, tol=2 * ulp))
    # the partner's row is out of order: found by the scan from the row's start.  (Two edits: the exchange is rule 4's, see above.)
    for s in (blk, C["arrow"]):
        row = 0 if s.name == "arrow" else s.n - 1
        k0 = int(s.row_ptr[row])
        sw = s.edited("tmp", None, **_swap(s, k0 + 3))
        out.append(s.edited(f"{s.name}_scan_finds_partners", {ORDER_RULE: 1}, col=sw.col, val=sw.val))
        k = k0 + 3   # an entry of the unordered row: its partner in row col[k] now differs by an ulp from it
        p = _partner(sw, k)
        val = sw.val.copy()
        val[p] = np.nextafter(val[p], 0.0)
        out.append(s.edited(f"{s.name}_scan_ulp", {ORDER_RULE: 1, SYMMETRY_RULE: 2}, col=sw.col, val=val, tol=0.0))
        # ... the same from the other side
        val = sw.val.copy()
        val[k] = np.nextafter(val[k], 0.0)
        out.append(s.edited(f"{s.name}_scan_ulp_in_row", {ORDER_RULE: 1, SYMMETRY_RULE: 2}, col=sw.col, val=val, tol=0.0))
        # ... and an entry elsewhere whose partner is missing from the unordered row: the scan runs to the row's end
        out.append(s.edited(f"{s.name}_scan_pair_deleted", {ORDER_RULE: 1, PATTERN: 1}, **_delete(sw, k0 + 6)))
    return {s.name: s for s in out}


def system(name):
    if name in CLEAN_NAMES:
        return clean_system(name)
    if name in AS_FOUND_NAMES:
        return as_found_system(name)
    return planted()[name]


def all_names():
    return CLEAN_NAMES + AS_FOUND_NAMES + list(planted())


def expected_violations(s):
    v = [0] * 8
    for rule, count in s.expect.items():
        v[rule] = count
    return tuple(v)
