"""tests/spectrum_model.py and tests/spectrum_cases.py: the model against a plain-Python restatement and against numpy's dense
eigenvalues, every case has the property it is named for, and the spread of the extreme Ritz values between summation orders -- what the
tolerances of tests/test_gpu_spectrum.py are measured against (spectrum_cases.spread; profiles/spectrum.md records the figures)."""
import math

import numpy as np
import pytest

import spectrum_cases as sc
import spectrum_model as M


def test_hash_vector_is_splitmix64():
    v = M.hash_vector(1000)
    for i in (0, 1, 2, 255, 256, 999):
        assert v[i] == (M.splitmix64(i) >> 11) * 2.0 ** -53 - 0.5
    assert M.splitmix64(0) == 0xE220A8397B1DCDAF          # the first output of the generator seeded with 0
    assert (v >= -0.5).all() and (v < 0.5).all() and abs(v.mean()) < 0.05


@pytest.mark.parametrize("op", sc.BOTH)
@pytest.mark.parametrize("name", ["tri_12", "tri_257", "blocks", "unordered_repeated"])
def test_model_equals_the_entry_by_entry_restatement(name, op):
    c = sc.case(name)
    got, want = sc.model(name, op), M.lanczos_entry_by_entry(c.row_ptr, c.col, c.val, c.b, c.x0, op, c.steps)
    k = got["steps_taken"]
    assert k == len(want["alpha"]) and got["scale"].tobytes() == want["scale"].tobytes() and got["gershgorin_max"] == want["gershgorin_max"]
    assert got["alpha"][:k].tobytes() == want["alpha"].tobytes() and got["beta"][:k + 1].tobytes() == want["beta"].tobytes()
    assert len(got["basis"]) == len(want["basis"]) and all(a.tobytes() == b.tobytes() for a, b in zip(got["basis"], want["basis"]))


def test_every_case_has_its_property():
    for name in sc.ALL_NAMES:
        assert sc.case(name).why
    for name, op in sc.runs():
        c, m = sc.case(name), sc.model(name, op)
        if name in sc.SEAM_A_ONLY:
            assert m["evaluated"] == 0 and m["steps_taken"] == 0 and m["iteration_bound"] == 0
            continue
        if name in sc.BAD_DIAGONAL:
            assert m["evaluated"] == 0 and m["bad_diagonal"] == sc.BAD_DIAGONAL[name] and (m["scale"] == 0).sum() == m["bad_diagonal"]
            continue
        assert m["evaluated"] == 1 and m["bad_diagonal"] == 0
        if name in sc.NO_STEP:
            assert m["steps_taken"] == 0 and m["iteration_bound"] == -1 and m["nonfinite"] == (name == "nan_start")
        elif name == "nan_value":
            assert m["steps_taken"] == 1 and m["nonfinite"] == 1 and math.isnan(m["alpha"][0]) and math.isinf(m["gershgorin_max"])
            assert math.isnan(m["lambda_min"]) and m["iteration_bound"] == -1
        elif (name, op) in sc.BREAKDOWN_AT:
            for order in M.ORDERS:
                o = sc.model(name, op, order)
                assert o["breakdown"] == 1 and o["steps_taken"] == sc.BREAKDOWN_AT[name, op], (name, op, order)
        else:
            assert m["steps_taken"] == min(c.steps, c.n) and not m["breakdown"] and not m["nonfinite"]
            assert len(m["basis"]) == m["steps_taken"] + 1
        if m["steps_taken"] and name != "nan_value":
            assert m["indefinite"] == (name == "indefinite")
            if name != "indefinite":
                assert 0 < m["lambda_min"] <= m["lambda_max"] <= m["gershgorin_max"] * (1 + 2.0 ** -40)
    rp = sc.case("blocks").row_ptr
    assert rp[sc.CHUNK] > sc.TILE and not np.isin(sc.TILE, rp)
    a = sc.case("arrow")
    assert np.diff(a.row_ptr)[100] > sc.TILE and np.diff(a.row_ptr).argmax() == 100
    u = sc.case("unordered_repeated")
    d, _ = M.diagonal(u.row_ptr, u.col, u.val)
    assert d[200] == 2.25 and (u.col[u.row_ptr[200]:u.row_ptr[201]] == 200).sum() == 2 and (u.col[u.row_ptr[40]:u.row_ptr[41]] == 41).sum() == 2
    assert sum((np.diff(u.col[u.row_ptr[i]:u.row_ptr[i + 1]]) < 0).any() for i in range(u.n)) > 100
    assert (len(sc.case("tri_65537").row_ptr) - 1 + sc.CHUNK - 1) // sc.CHUNK == 257
    z = sc.case("zero_start")
    assert (z.b == z.val * z.x0).all()


@pytest.mark.parametrize("name", ["tri_12", "tri_257", "blocks", "arrow", "unordered_repeated", "laplace_1000", "indefinite"])
def test_cases_are_symmetric(name):
    c = sc.case(name)
    for op in c.ops:
        a = M.dense_operator(c.row_ptr, c.col, c.val, op)
        assert np.abs(a - a.T).max() <= 2.0 ** -52 * np.abs(a).max()


@pytest.mark.parametrize("op", sc.BOTH)
def test_twelve_steps_on_twelve_rows_give_every_eigenvalue(op):
    c, m = sc.case("tri_12"), sc.model("tri_12", op)
    true = np.linalg.eigvalsh(M.dense_operator(c.row_ptr, c.col, c.val, op))
    assert m["steps_taken"] == 12
    assert np.abs(m["ritz"] - true).max() <= 1e-12 * np.abs(true).max()       # (the basis of 12 steps has lost little of its orthogonality)


@pytest.mark.parametrize("name,op", [(n, o) for n, o in sc.runs() if n in ("tri_255", "tri_257", "blocks", "arrow", "unordered_repeated", "laplace_1000",
                                                                             "indefinite", "tri_257_hash")])
def test_ritz_extremes_lie_inside_the_true_interval(name, op):
    c, m = sc.case(name), sc.model(name, op)
    true = np.linalg.eigvalsh(M.dense_operator(c.row_ptr, c.col, c.val, op))
    slack = 64 * 2.0 ** -52 * np.abs(true).max()
    assert true[0] - slack <= m["lambda_min"] and m["lambda_max"] <= true[-1] + slack
    # an eigenvalue within the bound of each extreme (the bound is of the computed recurrence: rounding added)
    assert np.abs(true - m["lambda_max"]).min() <= m["lambda_max_bound"] + slack
    assert np.abs(true - m["lambda_min"]).min() <= m["lambda_min_bound"] + slack
    assert m["lambda_max"] <= m["gershgorin_max"] * (1 + 2.0 ** -40)
    if not m["indefinite"]:
        assert m["condition_estimate"] <= (true[-1] / true[0]) * (1 + 1e-12)     # a LOWER bound of the condition number


def test_laplace_1000_against_its_analytic_spectrum():
    m = sc.model("laplace_1000", M.MATRIX)
    lam = 2 - 2 * np.cos(np.arange(1, 1001) * np.pi / 1001)
    assert m["steps_taken"] == 64 and m["lambda_max"] <= lam[-1] + 1e-14 and m["lambda_min"] >= lam[0] - 1e-14
    assert m["gershgorin_max"] == 4.0 and 4e5 < lam[-1] / lam[0] < 4.1e5
    assert m["iteration_bound"] == M.iteration_bound(m["condition_estimate"], 1e-3) > 0


def test_iteration_bound_edges():
    assert M.iteration_bound(1.0, 1e-3) == math.ceil(0.5 * math.log(2000.0)) and M.iteration_bound(4.0, 0.5) == 2
    for kappa, tol in ((math.inf, 1e-3), (math.nan, 1e-3), (0.5, 1e-3), (10.0, 0.0), (10.0, 1.0), (10.0, -1.0), (10.0, math.nan)):
        assert M.iteration_bound(kappa, tol) == -1


def test_spread_between_summation_orders():
    """recorded (profiles/spectrum.md), and bounded by what was measured when the cases were written: <= 1e-15 relative on the tri_* cases
    of one and two chunks, <= 3e-12 for lambda_min of laplace_1000; nothing above 1e-10"""
    for name, op in sc.runs():
        lo, hi, ritz = sc.spread(name, op)
        print(f"{name:20s} op {op}  lambda_min {lo:.3e}  lambda_max {hi:.3e}  ritz {ritz:.3e}")
        assert max(lo, hi, ritz) <= 1e-10
        if name in ("tri_255", "tri_256", "tri_257"):
            assert max(lo, hi) <= 1e-15
    assert sc.spread("laplace_1000", M.MATRIX)[0] <= 3e-12
