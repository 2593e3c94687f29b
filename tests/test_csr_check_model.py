"""tests/csr_check_model.py -- the NumPy statement of the rules of avs_check_csr that the device report has to equal -- pinned on systems
small enough to judge by eye, on the planted cases (each changes the counts it names and no other) and against scipy."""
import numpy as np
import pytest

import csr_check_cases as cc
import csr_check_model as m

NAN, INF = float("nan"), float("inf")


def report(**fields):
    r = dict(passed=1, evaluated=1, first_rule=-1, first_index=-1, first_row=-1, first_col=-1, violations=(0,) * 8, empty_rows=0,
             longest_row=0, asymmetric_entries=0, max_abs_value=0.0, max_abs_asymmetry=0.0)
    r.update(fields)
    return r


# 3 x 3, tridiagonal (2, -1): nothing to find
CLEAN3 = dict(row_ptr=[0, 2, 5, 7], col=[0, 1, 0, 1, 2, 1, 2], val=[2., -1., -1., 2., -1., -1., 2.], b=[1., 2., 3.])
# 4 x 4:  row 0: (0, 4) (2, -1)   row 1: (3, -2) (1, 0)   row 2: (0, -1.5) (2, NaN)   row 3: empty
#   entry 3 follows a larger column; rows 1, 2, 3 have a zero, a NaN, no diagonal; entry 5 is the NaN; entry 2 = (1, 3) has no (3, 1);
#   entries 1 = (0, 2) and 4 = (2, 0) differ by 0.5; b[1] and x[3] are not finite
FAULTY4 = dict(row_ptr=[0, 2, 4, 6, 6], col=[0, 2, 3, 1, 0, 2], val=[4., -1., -2., 0., -1.5, NAN], b=[1., INF, 0., 0.], x=[0., 0., 0., NAN])
# 2 x 2 with two columns out of range: row 0: (0, 1) (5, 2)   row 1: (-1, 3) -- and so no diagonal in row 1
COLUMNS2 = dict(row_ptr=[0, 2, 3], col=[0, 5, -1], val=[1., 2., 3.])
# row_ptr runs backwards at index 1
BACKWARDS3 = dict(row_ptr=[0, 3, 2, 4], col=[0, 1, 2, 2], val=[1., 1., 1., 1.], b=[NAN, 0., 0.])


@pytest.mark.parametrize("system, what, tol, want", [
    (CLEAN3, m.ALL, 0.0, report(evaluated=255, longest_row=3, max_abs_value=2.0)),
    (CLEAN3, 0, 0.0, report(evaluated=3, longest_row=3)),
    (FAULTY4, m.ALL, 0.25, report(passed=0, evaluated=255, first_rule=2, first_index=5, first_row=2, first_col=2, violations=(0, 0, 1, 2, 1, 3, 1, 2),
                                  empty_rows=1, longest_row=2, asymmetric_entries=2, max_abs_value=4.0, max_abs_asymmetry=0.5)),
    (FAULTY4, m.ALL, 0.5, report(passed=0, evaluated=255, first_rule=2, first_index=5, first_row=2, first_col=2, violations=(0, 0, 1, 2, 1, 3, 1, 0),
                                 empty_rows=1, longest_row=2, asymmetric_entries=2, max_abs_value=4.0, max_abs_asymmetry=0.5)),
    (FAULTY4, m.ORDER, 0.0, report(passed=0, evaluated=19, first_rule=4, first_index=3, first_row=1, first_col=1, violations=(0, 0, 0, 0, 1, 0, 0, 0),
                                   empty_rows=1, longest_row=2)),
    (FAULTY4, m.DIAGONAL, 0.0, report(passed=0, evaluated=35, first_rule=5, first_index=1, first_row=1, first_col=-1,
                                      violations=(0, 0, 0, 0, 0, 3, 0, 0), empty_rows=1, longest_row=2)),
    (FAULTY4, m.SYMMETRY, 0.0, report(passed=0, evaluated=195, first_rule=6, first_index=2, first_row=1, first_col=3, violations=(0, 0, 0, 0, 0, 0, 1, 2),
                                      empty_rows=1, longest_row=2, asymmetric_entries=2, max_abs_value=4.0, max_abs_asymmetry=0.5)),
    (FAULTY4, 0, 0.0, report(evaluated=3, empty_rows=1, longest_row=2)),
    (COLUMNS2, m.ALL, 0.0, report(passed=0, evaluated=247, first_rule=1, first_index=1, first_row=0, first_col=5, violations=(0, 2, 0, 0, 0, 1, 0, 0),
                                  longest_row=2, max_abs_value=3.0)),
    (COLUMNS2, 0, 0.0, report(passed=0, evaluated=3, first_rule=1, first_index=1, first_row=0, first_col=5, violations=(0, 2, 0, 0, 0, 0, 0, 0),
                              longest_row=2)),
    (BACKWARDS3, m.ALL, 0.0, report(passed=0, first_rule=0, first_index=1, violations=(1, 0, 0, 0, 0, 0, 0, 0))),
])
def test_hand_written_systems(system, what, tol, want):
    assert m.check(**system, what=what, tol=tol) == want


def test_nothing_at_or_behind_nnz_is_looked_at():
    s = CLEAN3
    got = m.check(s["row_ptr"], s["col"] + [-7, 99], s["val"] + [NAN, INF], s["b"], nnz=7)
    assert got == m.check(**s)
    # ... and row_ptr is judged against the stated nnz, not against the arrays
    assert m.check(s["row_ptr"], s["col"], s["val"], nnz=6)["violations"][0] == 1


def test_vectors_only_count_when_given():
    s = dict(FAULTY4)
    assert m.check(**s)["violations"][m.VECTOR] == 2
    s["x"] = None
    assert m.check(**s)["violations"][m.VECTOR] == 1
    s["b"] = None
    r = m.check(**s)
    assert r["violations"][m.VECTOR] == 0 and not r["evaluated"] >> m.VECTOR & 1


@pytest.mark.parametrize("name", cc.SMALL_CLEAN_NAMES + ["spd_n_3", "spd_n_513", "spd_long_row", "spd_unsorted_repeated", "spd_empty_rows"])
def test_clean_cases_pass_and_measure_what_scipy_measures(name):
    import scipy.sparse as sp
    s = cc.system(name)
    a = m.Analysis(s.row_ptr, s.col, s.val, s.b, s.x)
    for what in m.WHATS:
        r = a.report(what, 0.0)
        assert r["passed"] == 1 and r["violations"] == (0,) * 8 and r["asymmetric_entries"] == 0 and r["first_rule"] == -1, (what, r)
    if s.n == 0:
        return
    A = sp.csr_matrix((s.val, s.col, s.row_ptr), shape=(s.n, s.n))
    r = a.report()
    assert r["max_abs_asymmetry"] == abs(A - A.T).max() == 0.0
    assert r["max_abs_value"] == abs(A).max()
    assert r["longest_row"] == np.diff(s.row_ptr).max() and r["empty_rows"] == 0
    # the same with one value moved: the model's maximum is scipy's
    if s.nnz > s.n:
        val = s.val.copy()
        k = cc._off_diagonal(s, s.nnz // 2)
        val[k] += 0.125
        A = sp.csr_matrix((val, s.col, s.row_ptr), shape=(s.n, s.n))
        r = m.check(s.row_ptr, s.col, val)
        assert r["max_abs_asymmetry"] == abs(A - A.T).max() == 0.125 and r["asymmetric_entries"] == 2 and r["violations"][m.SYMMETRY_RULE] == 2


@pytest.mark.parametrize("name", list(cc.planted()))
def test_planted_cases_change_the_named_counts_and_no_other(name):
    s = cc.system(name)
    base = cc.system(s.base)
    assert m.check(base.row_ptr, base.col, base.val, base.b, base.x, tol=s.tol)["violations"] == (0,) * 8
    r = m.check(s.row_ptr, s.col, s.val, s.b, s.x, tol=s.tol)
    assert r["violations"] == cc.expected_violations(s)
    assert r["passed"] == (0 if s.expect else 1)
    if s.expect:
        assert r["first_rule"] == min(s.expect)


def _slow_first(s, what, tol):
    """(rule, index) of the first violation, entry by entry in plain Python (small systems)"""
    rp, col, val, n = s.row_ptr.tolist(), s.col.tolist(), s.val.tolist(), s.n
    asked = m.rules_asked(what, s.b is not None or s.x is not None)
    hits = []
    for i in range(n):
        row = col[rp[i]:rp[i + 1]]
        if asked >> m.VECTOR & 1 and not all(np.isfinite(v[i]) for v in (s.b, s.x) if v is not None):
            hits.append((m.VECTOR, i))
        diag = [k for k in range(rp[i], rp[i + 1]) if col[k] == i]
        if asked >> m.DIAGONAL_RULE & 1 and (not diag or not val[diag[-1]] > 0):
            hits.append((m.DIAGONAL_RULE, i))
        for k in range(rp[i], rp[i + 1]):
            j = col[k]
            if not 0 <= j < n:
                hits.append((m.COLUMN, k))
            if asked >> m.VALUE & 1 and not np.isfinite(val[k]):
                hits.append((m.VALUE, k))
            if asked >> m.ORDER_RULE & 1 and k > rp[i] and col[k] <= col[k - 1]:
                hits.append((m.ORDER_RULE, k))
            if asked >> m.PATTERN & 1 and 0 <= j < n and j != i:
                partner = [p for p in range(rp[j], rp[j + 1]) if col[p] == i]
                if not partner:
                    hits.append((m.PATTERN, k))
                elif np.isfinite(val[k]) and np.isfinite(val[partner[0]]) and abs(val[k] - val[partner[0]]) > tol:
                    hits.append((m.SYMMETRY_RULE, k))
    return min(hits) if hits else None, sorted(hits)


@pytest.mark.parametrize("name", ["several", "raw_n_3", "raw_n_513", "raw_specials", "raw_empty_rows"])
@pytest.mark.parametrize("what", m.WHATS)
def test_first_is_the_minimum_by_rule_and_index(name, what):
    s = cc.system(name)
    r = m.check(s.row_ptr, s.col, s.val, s.b, s.x, what=what, tol=0.01)
    first, hits = _slow_first(s, what, 0.01)
    assert r["violations"] == tuple(sum(1 for h in hits if h[0] == rule) for rule in range(8))
    if first is None:
        assert r["passed"] == 1 and r["first_rule"] == r["first_index"] == r["first_row"] == r["first_col"] == -1
        return
    assert (r["first_rule"], r["first_index"]) == first and r["passed"] == 0
    if first[0] in (m.VECTOR, m.DIAGONAL_RULE):
        assert (r["first_row"], r["first_col"]) == (first[1], -1)
    else:
        assert r["first_row"] == int(np.searchsorted(s.row_ptr, first[1], side="right")) - 1 and r["first_col"] == int(s.col[first[1]])
    if name == "several" and what == m.ALL:   # rules 1, 2, 3, 4 and 6 are violated: the column comes first
        assert r["violations"] == (0, 1, 1, 1, 1, 0, 1, 0) and (r["first_rule"], r["first_index"], r["first_row"], r["first_col"]) == (1, 119, 40, 2**31 - 1)
