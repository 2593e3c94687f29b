"""The host model of the CU-resident loop (tests/resident_model.py) and the tolerance rule it carries, on every edge system.

(a) the fp64 row sums are the C oracle's, bit for bit; (b) the model run to 1e-10 agrees with the oracle's PCG; (c) the rule -- a loop
may deviate from the long-double run by 32 max(s_k, 2^-50), s_k the distance of two fp64 summation orders from it -- has teeth: three
planted errors that a converged solve cannot see each leave it by a factor of 100 at least, at some checked k or in `error`, on every
case of 64 rows or more; (d) the loose tolerances of the exit checks are clear of r.r on both sides in every run.  Prints the scales.
"""
import numpy as np
import pytest

import resident_edges as R
import resident_model as M
from oracle import oracle as O
from util import rel_l2

MUTATIONS = ("drop_row", "stale_u", "skip_x")


def mutation_ratios(case, model, ks):
    """{kind: how far (in bounds) the mutated fp64 run leaves the rule, at its worst checked k, in x or in error}"""
    out = {}
    passes = max(ks)
    lens = R.row_lengths(case)
    row = case.n // 2 + int(np.argmax(lens[case.n // 2:] > 1))      # the first row from the middle on that has an off-diagonal entry
    for kind in MUTATIONS:
        q = M.run(model.A, case.b, case.x0, 0.0, passes, "asc64", M.Mutation(kind, at=2, row=row, dot="wu"))
        worst = 0.0
        for k in ks:
            if k > q.passes:
                continue
            worst = max(worst, M.x_dev(q.x[k], model.ld, k) / model.bound_x(k), M.error_dev(q.error[k], model.ld, k) / model.bound_error(k))
        out[kind] = worst
    return out


@pytest.mark.parametrize("name", R.NAMES)
def test_model_and_rule(name):
    c = R.get(name)
    model = R.model_of(c)
    A = model.A
    rp64 = c.row_ptr.astype(np.int64)
    # (a) row sums: left to right, multiply then add -- the oracle's bits
    x = np.random.default_rng(c.n).standard_normal(c.n) * 10.0 ** np.random.default_rng(c.n + 1).integers(-2, 3, c.n)
    assert np.array_equal(A.row_sums(x).view(np.uint64), O.spmv_csr(rp64, c.col, c.val, x).view(np.uint64))
    # (b) the recurrence solves what the oracle's PCG solves
    tol = 1e-10
    xo, io = O.pcg_csr(rp64, c.col, c.val, c.b, c.x0, tol, 2000)
    q = M.run(A, c.b, c.x0, tol, 2000, "asc64")
    assert q.converged[-1] and abs(q.iterations[-1] - io.iterations) <= 3, (q.iterations[-1], io.iterations)
    assert rel_l2(q.x[-1], xo) < 1e-8
    # the two orders are two samples: the runs differ, and stay close to the long-double run
    ks = R.checked_ks(c, model)
    assert ks[0] == 0 and (c.few_rows or ks == R.KS), ks
    print(f"\n{name}: n = {c.n}, checked k = {ks[0]}..{ks[-1]}")
    for k in ks:
        sx, se = model.s[k]
        print(f"  k = {k:2d}  s_k(x) = {sx:.2e}  s_k(error) = {se:.2e}  error = {float(model.ld.error[k]):.3e}")
        assert model.ld.iterations[k] == k and not model.ld.converged[k]
        assert sx < 1e-9, (k, sx)       # (an fp64 run that strays this far is a bug of the model, not a summation order)
    assert np.array_equal(model.ld.x[0].astype(np.float64), c.x0)
    # (c) teeth
    if c.n >= 64:
        ratios = mutation_ratios(c, model, ks)
        print("  mutation ratios (deviation / bound): " + ", ".join(f"{k} {v:.2e}" for k, v in ratios.items()))
        for kind, ratio in ratios.items():
            assert ratio >= 100.0, (kind, ratio)
    # (d) the exits: one at an odd and one at an even `iterations`, the threshold 1e-6 clear of r.r on both sides in all three runs
    # (a system of <= 5 rows has converged after at most n passes: it has the exits that exist)
    exits = model.exit_tolerances()
    if c.n > 5:
        assert sorted(e[1] % 2 for e in exits) == [0, 1], exits
    if True:
        for tol_e, iters, passes in exits:
            assert passes == iters + 1 and model.exits_are_clear(tol_e, iters, 1e-6)
            for mode in M.MODES:
                qe = M.run(A, c.b, c.x0, tol_e, 100, mode)
                assert qe.converged[-1] and qe.iterations[-1] == iters and qe.passes == passes, (mode, tol_e, iters, qe.iterations[-1])
            print(f"  exit: tol = {tol_e:.6e} -> iterations = {iters} after {passes} passes")


def test_model_edges():
    """b = 0 gives x = 0; a converged initial guess is kept"""
    c = R.get("rows_65")
    A = M.Matrix(c.row_ptr, c.col, c.val)
    q = M.run(A, np.zeros(c.n), c.x0, 1e-10, 10, "asc64")
    assert q.passes == 0 and q.converged[0] and not q.x[0].any() and q.error[0] == 0 and q.iterations[0] == 0
    done = M.run(A, c.b, c.x0, 1e-13, 500, "asc64")
    assert done.converged[-1]
    q = M.run(A, c.b, done.x[-1], 1e-10, 10, "asc64")
    assert q.passes == 0 and q.converged[0] and q.iterations[0] == 0 and np.array_equal(q.x[0], done.x[-1])
