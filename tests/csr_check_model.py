"""The rules of avs_check_csr (include/avs.h) in NumPy: the model the device report has to equal exactly.

`analyse(...)` evaluates every rule once (no Python loop over entries); `Analysis.report(what, tol)` composes the report a call with those
bits gives -- the fields of avs_csr_check as a dict (struct_size left out).  Partner lookup for rules 6 / 7 goes through a stable sort of
the keys row * n + col of the entries whose column is in range: the first position of key j * n + i in that order is the first entry of
row j with column i, which is what the device finds by bisection in a strictly ascending row and by a scan from the row's start otherwise.
"""
from __future__ import annotations

import numpy as np

VALUES, ORDER, DIAGONAL, SYMMETRY, ALL = 1, 2, 4, 8, 15
ROW_PTR, COLUMN, VALUE, VECTOR, ORDER_RULE, DIAGONAL_RULE, PATTERN, SYMMETRY_RULE = range(8)
RULES = 8
FIELDS = ("passed", "evaluated", "first_rule", "first_index", "first_row", "first_col", "violations", "empty_rows", "longest_row",
          "asymmetric_entries", "max_abs_value", "max_abs_asymmetry")
WHATS = (ALL, VALUES, ORDER, DIAGONAL, SYMMETRY, 0)


def rules_asked(what, vectors):
    """bit r: rule r is evaluated once rule 0 holds"""
    e = 1 << ROW_PTR | 1 << COLUMN
    if what & VALUES:
        e |= 1 << VALUE | (1 << VECTOR if vectors else 0)
    if what & ORDER:
        e |= 1 << ORDER_RULE
    if what & DIAGONAL:
        e |= 1 << DIAGONAL_RULE
    if what & SYMMETRY:
        e |= 1 << PATTERN | 1 << SYMMETRY_RULE
    return e


def _blank():
    return dict(passed=1, evaluated=1, first_rule=-1, first_index=-1, first_row=-1, first_col=-1, violations=(0,) * RULES, empty_rows=0,
                longest_row=0, asymmetric_entries=0, max_abs_value=0.0, max_abs_asymmetry=0.0)


class Analysis:
    """every rule evaluated on one system; report(what, tol) picks"""

    def __init__(self, row_ptr, col, val, b=None, x=None, nnz=None):
        rp = np.asarray(row_ptr, dtype=np.int64)
        self.n = n = len(rp) - 1
        self.nnz = nnz = len(col) if nnz is None else int(nnz)
        self.vectors = b is not None or x is not None
        col = np.asarray(col, dtype=np.int64)[:nnz]       # entry nnz and beyond is never looked at
        val = np.asarray(val, dtype=np.float64)[:nnz]
        bad0 = (rp < 0) | (rp > nnz)
        bad0[0] |= rp[0] != 0
        bad0[n] |= rp[n] != nnz
        bad0[:-1] |= rp[:-1] > rp[1:]
        self.bad = {ROW_PTR: np.flatnonzero(bad0)}
        if len(self.bad[ROW_PTR]) or n == 0:
            return
        lens = np.diff(rp)
        self.empty_rows, self.longest_row = int((lens == 0).sum()), int(lens.max())
        self.rows = rows = np.repeat(np.arange(n, dtype=np.int64), lens)
        self.col = col
        in_range = (col >= 0) & (col < n)
        self.bad[COLUMN] = np.flatnonzero(~in_range)
        finite = np.isfinite(val)
        self.bad[VALUE] = np.flatnonzero(~finite)
        v3 = np.zeros(n, dtype=bool)
        for vec in (b, x):
            if vec is not None:
                v3 |= ~np.isfinite(np.asarray(vec, dtype=np.float64)[:n])
        self.bad[VECTOR] = np.flatnonzero(v3)
        not_first = np.ones(nnz, dtype=bool)
        not_first[rp[:-1][lens > 0]] = False
        v4 = np.zeros(nnz, dtype=bool)
        v4[1:] = col[1:] <= col[:-1]
        self.bad[ORDER_RULE] = np.flatnonzero(v4 & not_first)
        last_diag = np.full(n, -1, dtype=np.int64)
        kd = np.flatnonzero(col == rows)
        np.maximum.at(last_diag, rows[kd], kd)
        v5 = last_diag < 0
        have = np.flatnonzero(~v5)
        v5[have] = ~(val[last_diag[have]] > 0.0)
        self.bad[DIAGONAL_RULE] = np.flatnonzero(v5)
        # rules 6 / 7: the partner of entry k = (i, j), j in range and j != i, is the first entry of row j with column i
        kin = np.flatnonzero(in_range)
        keys = rows[kin] * n + col[kin]
        order = np.argsort(keys, kind="stable")
        skeys, sk = keys[order], kin[order]
        kc = np.flatnonzero(in_range & (col != rows))
        want = col[kc] * n + rows[kc]
        pos = np.searchsorted(skeys, want, side="left")
        found = np.zeros(len(kc), dtype=bool)
        ok = pos < len(skeys)
        found[ok] = skeys[pos[ok]] == want[ok]
        self.bad[PATTERN] = kc[~found]
        k, p = kc[found], sk[pos[found]]
        both = finite[k] & finite[p]
        k, p = k[both], p[both]
        with np.errstate(over="ignore", invalid="ignore"):
            self.pair_k, self.pair_d = k, np.abs(val[k] - val[p])
        self.asymmetric_entries = int((val[k] != val[p]).sum())
        self.max_abs_asymmetry = float(self.pair_d.max()) if len(k) else 0.0
        self.max_abs_value = float(np.abs(val[finite]).max()) if finite.any() else 0.0

    def report(self, what=ALL, tol=0.0):
        r = _blank()
        if len(self.bad[ROW_PTR]):
            v = [0] * RULES
            v[ROW_PTR] = len(self.bad[ROW_PTR])
            r.update(passed=0, first_rule=ROW_PTR, first_index=int(self.bad[ROW_PTR][0]), violations=tuple(v))
            return r
        if self.n == 0:
            return r
        r["evaluated"] = asked = rules_asked(what, self.vectors)
        bad = dict(self.bad)
        bad[SYMMETRY_RULE] = self.pair_k[self.pair_d > tol]
        r["violations"] = tuple(len(bad[rule]) if asked >> rule & 1 else 0 for rule in range(RULES))
        r["empty_rows"], r["longest_row"] = self.empty_rows, self.longest_row
        if what & SYMMETRY:
            r.update(asymmetric_entries=self.asymmetric_entries, max_abs_value=self.max_abs_value, max_abs_asymmetry=self.max_abs_asymmetry)
        for rule in range(RULES):
            if r["violations"][rule]:
                idx = int(bad[rule].min())
                r.update(passed=0, first_rule=rule, first_index=idx)
                if rule in (VECTOR, DIAGONAL_RULE):
                    r.update(first_row=idx, first_col=-1)
                else:
                    c = int(self.col[idx])
                    r.update(first_row=int(self.rows[idx]), first_col=int(np.int64(c).astype(np.int32)))
                break
        return r


def check(row_ptr, col, val, b=None, x=None, what=ALL, tol=0.0, nnz=None):
    return Analysis(row_ptr, col, val, b, x, nnz).report(what, tol)
