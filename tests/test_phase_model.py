"""The host model of the launch-per-phase PCG loop (tests/phase_model.py) and the tolerance rule it carries.

(a) the "asc64" run of the model against the C oracle's PCG (Eigen's operation order, serial dot products) under max_iterations = 1, 8,
33, 64 on three cases: the same `iterations`, x within the rule of the long-double run -- this ties the model to the reference's
recurrence without a GPU; (b) the rule -- a loop may deviate from the long-double run by 32 max(s_k, 2^-50), s_k the distance of two fp64
summation orders from it -- has teeth: every planted error of phase_model.Mutation leaves it by a factor of 100 at least at some checked k
of the case it is planted in, in x or in `error` (the two x-update mutations: at every targeted exit); (c) b = 0 and a converged initial
guess.

Mutation ratios (deviation / bound at the worst checked k) of this file's run, the smallest over the cases of MUTATION_CASES:
    swap_rho at 5            2.6e+11      drop_row p.t at 4        2.6e+09
    stale_alpha at 33        6.1e+09      drop_row r.r at 4        1.0e+08  (in `error` only: r.r feeds the test, not the recurrence)
    skip_x   (every exit)    2.7e+08      drop_row r.z at 4        1.9e+09
    double_x (every exit)    2.7e+08
"""
import numpy as np
import pytest

import phase_edges as R
import phase_model as P
from oracle import oracle as O

ORACLE_CASES = ("rows_513", "form_coded", "form_dictionary")
ORACLE_KS = (1, 8, 33, 64)
MUTATION_CASES = ("rows_257", "rows_513", "nb_264", "form_coded", "form_dictionary")
DROP_AT, SWAP_AT = 4, 5


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_model_follows_the_oracle(name):
    c = R.get(name)
    model = R.model_of(c)
    rp64 = c.row_ptr.astype(np.int64)
    q = model.f64[0]                                    # the "asc64" run
    # the row sums: left to right, multiply then add -- the oracle's bits
    x = np.random.default_rng(c.n).standard_normal(c.n) * 10.0 ** np.random.default_rng(c.n + 1).integers(-2, 3, c.n)
    assert np.array_equal(model.A.row_sums(x).view(np.uint64), O.spmv_csr(rp64, c.col, c.val, x).view(np.uint64))
    for k in ORACLE_KS:
        xo, io = O.pcg_csr(rp64, c.col, c.val, c.b, c.x0, 0.0, k)
        dx, dm = P.x_dev(xo, model.ld, k), P.x_dev(q.x[k], model.ld, k)
        de = P.error_dev(io.error, model.ld, k)
        print(f"{name} k {k}: oracle dev_x {dx:.3e} dev_e {de:.3e}, asc64 dev_x {dm:.3e}, bound_x {model.bound_x(k):.3e}")
        assert io.iterations == q.iterations[k] == k and not q.converged[k], (k, io.iterations, q.iterations[k])
        assert dx <= model.bound_x(k) and dm <= model.bound_x(k), (k, dx, dm, model.bound_x(k))
        assert de <= model.bound_error(k), (k, de, model.bound_error(k))
    # and to a tolerance: the same count, the same solution
    tol = 1e-10
    xo, io = O.pcg_csr(rp64, c.col, c.val, c.b, c.x0, tol, 2000)
    done = P.run(model.A, c.b, c.x0, tol, 2000, "asc64")
    assert done.converged[-1] and abs(done.iterations[-1] - io.iterations) <= 1, (done.iterations[-1], io.iterations)
    assert P._dev(done.x[-1], xo) < 1e-8


def mutation_ratios(case, model, ks):
    """{label: how far (in bounds) the mutated "asc64" run leaves the rule at its worst checked k, in x or in error}"""
    assert case.n % 2 == 1, "the default row of drop_row is the lone last row of an odd n"
    planted = [("swap_rho", P.Mutation("swap_rho", at=SWAP_AT))]
    planted += [(f"drop_row {d}", P.Mutation("drop_row", at=DROP_AT, dot=d)) for d in P.DOTS]
    if max(ks) > P.K_CHUNK + 1:
        planted.append(("stale_alpha", P.Mutation("stale_alpha")))
    out = {}
    for label, mut in planted:
        q = P.run(model.A, case.b, case.x0, 0.0, max(ks), "asc64", mut)
        out[label] = max(max(P.x_dev(q.x[k], model.ld, k) / model.bound_x(k), P.error_dev(q.error[k], model.ld, k) / model.bound_error(k))
                         for k in ks if k <= q.passes)
    for kind in ("skip_x", "double_x"):     # the converging iteration's x update: at every targeted exit
        for tol, iters, it in R.exit_targets(case, model):
            q = P.run(model.A, case.b, case.x0, tol, R.EXIT_MAX_ITERATIONS, "asc64", P.Mutation(kind))
            assert q.converged[-1] and q.iterations[-1] == iters and q.passes == it
            ratio = P.x_dev(q.x[-1], model.ld, it) / model.bound_x(it)
            out[kind] = min(out.get(kind, np.inf), ratio)
    return out


@pytest.mark.parametrize("name", MUTATION_CASES)
def test_rule_has_teeth(name):
    c = R.get(name)
    model = R.model_of(c)
    ks = R.checked_ks(c, model)
    assert DROP_AT in ks and max(ks) >= SWAP_AT
    # unplanted, the fp64 runs are inside the rule by construction (s_k is their distance): a mutated run is judged against the same bound
    ratios = mutation_ratios(c, model, ks)
    print(f"\n{name}: mutation ratios (deviation / bound): " + ", ".join(f"{k} {v:.2e}" for k, v in ratios.items()))
    want = {"swap_rho", "drop_row pt", "drop_row rr", "drop_row rz"} | ({"stale_alpha"} if max(ks) > P.K_CHUNK + 1 else set()) | \
        ({"skip_x", "double_x"} if c.exits else set())
    assert set(ratios) == want, (sorted(ratios), sorted(want))
    for label, ratio in ratios.items():
        assert ratio >= 100.0, (label, ratio)


def test_mutations_change_only_what_they_name():
    """a mutation leaves the iterates before its iteration bit-identical, and one that never fires leaves the whole run so"""
    c = R.get("rows_257")
    A = P.Matrix(c.row_ptr, c.col, c.val)
    plain = P.run(A, c.b, c.x0, 0.0, 40, "asc64")
    for mut in (P.Mutation("swap_rho", at=7), P.Mutation("drop_row", at=7, dot="pt"), P.Mutation("stale_alpha"), P.Mutation("skip_x"),
                P.Mutation("double_x"), P.Mutation("swap_rho", at=1000)):
        q = P.run(A, c.b, c.x0, 0.0, 40, "asc64", mut)
        first = next((k for k in range(41) if not np.array_equal(q.x[k], plain.x[k])), None)
        # (x_k holds alpha_k p_{k-1}: a wrong alpha shows in its own iteration, a wrong beta or p.t partner one later)
        want = {"swap_rho": mut.at + 1, "drop_row": mut.at, "stale_alpha": mut.at}.get(mut.kind) if mut.at <= 40 else None
        if mut.kind in ("skip_x", "double_x"):
            want = None
        assert first == want, (mut.kind, mut.at, first)


def test_model_edges():
    """b = 0 gives x = 0; a converged initial guess is kept; the converging iteration updates x and leaves `iterations`"""
    c = R.get("rows_257")
    A = P.Matrix(c.row_ptr, c.col, c.val)
    q = P.run(A, np.zeros(c.n), c.x0, 1e-10, 10, "asc64")
    assert q.passes == 0 and q.converged[0] and not q.x[0].any() and q.error[0] == 0 and q.iterations[0] == 0
    done = P.run(A, c.b, c.x0, 1e-13, 2000, "asc64")
    assert done.converged[-1] and done.iterations[-1] == done.passes - 1
    assert not np.array_equal(done.x[-1], done.x[-2])
    q = P.run(A, c.b, done.x[-1], 1e-10, 10, "asc64")
    assert q.passes == 0 and q.converged[0] and q.iterations[0] == 0 and np.array_equal(q.x[0], done.x[-1])
    # a cap equal to the converging iteration changes nothing
    capped = P.run(A, c.b, c.x0, 1e-13, done.passes, "asc64")
    assert capped.converged[-1] and capped.iterations[-1] == done.iterations[-1] and np.array_equal(capped.x[-1], done.x[-1])
