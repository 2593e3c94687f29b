"""tests/solution_check_model.py, the reference of the GPU tests of avs_check_solution, pinned without a GPU: against an entry-by-entry
restatement in plain Python floats on every case, against known answers, and -- case by case -- that each case of
solution_check_cases.py has the property it is there for.  Plus the layout of avs_solution_check against the ctypes mirror."""
import math
import os
import subprocess

import numpy as np
import pytest

import solution_check_cases as sc
import solution_check_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sc.NAMES)
def test_model_equals_the_entry_by_entry_restatement(name):
    c = sc.case(name)
    got, want = M.evaluate(*c.arrays()), M.evaluate_entry_by_entry(*c.arrays())
    assert got["evaluated"] == 1 and got["n"] == c.n and got["nnz"] == c.nnz
    assert M.same_floats(got["residual"], want["residual"]) and M.same_floats(got["y"], want["y"])
    for f in ("nonfinite_x", "nonfinite_b", "nonfinite_residual", "rows_summed", "max_residual_row") + M.MAXIMA + M.SUMS + ("relative_residual",):
        assert got[f] == want[f], (f, got[f], want[f])
    for f in M.SUMS:
        assert got[f + "_abs"] >= abs(got[f])


@pytest.mark.parametrize("name", sc.SEAM_A_ONLY)
def test_seam_a_refuses_what_rules_0_and_1_refuse(name):
    c = sc.case(name)
    got = M.evaluate(*c.arrays())
    assert got["evaluated"] == 0 and got["residual"] is None and got["rows_summed"] == 0 and got["residual_norm2"] == 0.0


def test_every_case_has_its_property():
    ev = {name: M.evaluate(*sc.case(name).arrays()) for name in sc.NAMES}
    assert ev["n_0"]["rows_summed"] == 0 and ev["n_0"]["max_residual_row"] == -1 and ev["n_0"]["relative_residual"] == 0.0
    assert ev["n_1"]["residual"].tolist() == [1.0 - 4.0 * 0.3] and ev["n_1"]["max_residual_row"] == 0 and ev["n_1"]["update_norm2"] == 0.3 * 0.3
    for n in (255, 256, 257, 65537):
        assert ev[f"tri_{n}"]["rows_summed"] == n
    assert -(-65537 // sc.CHUNK) == 257 > 256
    e = sc.case("empty_rows")
    assert e.row_ptr[150] == e.row_ptr[151] and e.row_ptr[299] == e.row_ptr[300] == e.nnz
    assert ev["empty_rows"]["residual"][150] == e.b[150] and ev["empty_rows"]["residual"][299] == e.b[299]
    l = sc.case("long_row_4097")
    assert np.diff(l.row_ptr).max() == sc.TILE + 1 and l.row_ptr[2500] % sc.TILE != 0
    t = sc.case("tile_straddle")
    first_chunk = t.row_ptr[:sc.CHUNK + 1]
    assert first_chunk[-1] > sc.TILE and not (first_chunk == sc.TILE).any()         # the boundary lies inside a row
    u = sc.case("unordered_repeated")
    unordered = repeated = 0
    for i in range(u.n):
        cols = u.col[u.row_ptr[i]:u.row_ptr[i + 1]]
        unordered += bool((np.diff(cols) < 0).any())
        repeated += len(set(cols.tolist())) < len(cols)
    assert unordered > 10 and repeated > 10
    assert ev["cancellation"]["y"].tolist() == [0.0, 1.0, 1.0] and ev["cancellation"]["residual"].tolist() == [0.0, -1.0, -1.0]
    assert ev["cancellation"]["max_residual_row"] == 1                                # the smallest of the two rows that attain 1
    assert (ev["nan_x_own_row"]["nonfinite_x"], ev["nan_x_own_row"]["nonfinite_residual"], ev["nan_x_own_row"]["rows_summed"]) == (1, 1, 299)
    assert (ev["nan_x_three_rows"]["nonfinite_x"], ev["nan_x_three_rows"]["nonfinite_residual"], ev["nan_x_three_rows"]["rows_summed"]) == (1, 3, 297)
    assert (ev["inf_b"]["nonfinite_b"], ev["inf_b"]["nonfinite_residual"], ev["inf_b"]["rows_summed"]) == (1, 1, 299)
    full = M.evaluate(*sc.case("nan_x0").arrays()[:5], x0=np.where(np.isnan(sc.case("nan_x0").x0), 0.0, sc.case("nan_x0").x0))
    assert ev["nan_x0"]["rows_summed"] == 300 and ev["nan_x0"]["residual_norm2"] == full["residual_norm2"]
    assert ev["nan_x0"]["update_norm2"] < full["update_norm2"]
    z = sc.case("neg_zero")
    assert sum(int(np.signbit(a[a == 0]).sum()) for a in (z.val, z.x, z.b, z.x0)) == 7
    assert ev["b0_x0"]["relative_residual"] == 0.0 and ev["b0_x0"]["residual_norm2"] == 0.0
    assert ev["b0_x_nonzero"]["relative_residual"] == math.inf and ev["b0_x_nonzero"]["rhs_norm2"] == 0.0
    d = ev["diagonal_exact"]
    assert not d["residual"].any() and d["max_abs_residual"] == 0.0 and d["max_residual_row"] == 0 and d["relative_residual"] == 0.0
    assert ev["tri_257_no_x0"]["update_norm2"] == 0.0 and ev["tri_257_no_x0"]["max_abs_update"] == 0.0 and ev["tri_257"]["update_norm2"] > 0


def test_known_answers():
    """an exact diagonal solve, and a planted residual: x = x* + e_j gives r = -A e_j, column j of A"""
    n, j = 600, 321
    c = sc.case("diagonal_exact")
    x = c.x.copy()
    x[j] += 1.0
    got = M.evaluate(c.row_ptr, c.col, c.val, c.b, x, c.x0)
    want_rj = c.b[j] - c.val[j] * x[j]
    assert got["max_residual_row"] == j and got["max_abs_residual"] == abs(want_rj) and got["residual_norm2"] == want_rj * want_rj
    assert np.count_nonzero(got["residual"]) == 1 and got["rows_summed"] == n
    # tridiagonal, integer-valued data so that every operation is exact: x* = 0, b = 0, x = e_j
    t = sc.case("tri_257")
    val = np.round(t.val * 32.0)                                                      # the off-diagonals are multiples of 1/32
    e = np.zeros(t.n)
    e[j - 100] = 1.0
    got = M.evaluate(t.row_ptr, t.col, val, np.zeros(t.n), e, np.zeros(t.n))
    col_j = np.zeros(t.n)
    for i in range(t.n):
        for k in range(t.row_ptr[i], t.row_ptr[i + 1]):
            if t.col[k] == j - 100:
                col_j[i] += val[k]
    assert np.array_equal(got["residual"], -col_j) and np.count_nonzero(col_j) == 3
    assert got["max_residual_row"] == j - 100 and got["max_abs_residual"] == val[t.row_ptr[j - 100] + 1] == 96.0      # the diagonal: 3 entries x 32
    assert got["residual_norm2"] == float((col_j ** 2).sum()) and got["relative_residual"] == math.inf
    assert got["x_dot_ax"] == 96.0 and got["x_dot_b"] == 0.0 and got["update_norm2"] == 1.0 and got["max_abs_update"] == 1.0 and got["max_abs_x"] == 1.0


def test_struct_layout_matches_the_binding(tmp_path):
    """sizeof and the offsets of avs_solution_check in C (gcc compiles include/avs.h as plain C) == the ctypes mirror"""
    import ctypes

    from adaptiveviscositysolver_amd import capi
    T = capi.SolutionCheck
    fields = [f for f, _ in T._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "avs.h"\nint main(void){printf("%zu", sizeof(avs_solution_check));\n'
                   + "".join(f'printf(" %zu", offsetof(avs_solution_check, {f}));\n' for f in fields)
                   + 'printf(" %d %d %d %d\\n", AVS_CHECK_OF_SOLUTION, AVS_CHECK_OF_INITIAL_GUESS, AVS_RATES_OF_SOLUTION, AVS_RATES_OF_INITIAL_GUESS);'
                     'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == ctypes.sizeof(T) == 160 and T().struct_size == 160
    assert got[1:1 + len(fields)] == [getattr(T, f).offset for f in fields]
    assert [getattr(T, f).offset for f in fields] == [0, 4, 8, 12, 16, 20] + list(range(24, 160, 8))
    assert got[1 + len(fields):] == [capi.CHECK_OF_SOLUTION, capi.CHECK_OF_INITIAL_GUESS, capi.RATES_OF_SOLUTION, capi.RATES_OF_INITIAL_GUESS] == [0, 1, 0, 1]
    assert (M.SOLUTION, M.INITIAL_GUESS) == (capi.CHECK_OF_SOLUTION, capi.CHECK_OF_INITIAL_GUESS)
