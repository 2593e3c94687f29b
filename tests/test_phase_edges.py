"""The named systems of tests/phase_edges.py have the properties their names claim, and the conditions the GPU test relies on hold --
all on the host: symmetric, sorted columns, every row with its diagonal, a palette of at most 1,023 off-diagonal values; the value form,
the partial sums nb, the vector grid g and the place of the alpha step that avs_phase_loop_info must report; every case live up to its
largest checked k, with a bound of at most 1e-9 there (so a loose rule cannot pass for a tight one); every targeted exit admissible and met
exactly by all three runs of the model."""
import numpy as np
import pytest

import csr_edges as E
import phase_edges as R
import phase_model as P


def test_case_list():
    assert [f"rows_{n}" for n in (1, 2, 3, 255, 256, 257, 511, 512, 513)] == [n for n in R.NAMES if n.startswith("rows_")]
    assert {"nb_264", "nb_2056", "nb_4104", "form_coded", "form_plain", "form_dictionary", "form_tile_tables", "beta0_graph0", "beta0_graph1",
            "beta1_graph0", "beta1_graph1"} <= set(R.NAMES)
    assert R.KS == (0, 1, 2, 3, 4, 7, 8) and R.KS_CHUNKS == (31, 32, 33, 64, 65, 90, 96, 97) and R.KS_NB == (33, 34)
    # what the checked k are chosen for: 64 captures the graph, 96 is the first pure replay, 90 and 97 end in a partial chunk
    assert (R.replayed_chunks(64), R.launched_chunks(64)) == (1, 1) and (R.replayed_chunks(96), R.launched_chunks(96)) == (2, 1)
    assert (R.replayed_chunks(90), R.launched_chunks(90)) == (1, 2) and (R.replayed_chunks(97), R.launched_chunks(97)) == (2, 2)
    assert R.replayed_chunks(33) == 0 and R.replayed_chunks(97, graph=False) == 0 and R.launched_chunks(97, graph=False) == 4
    assert R.replayed_chunks(9 * 32) == 7       # (chunk 8 is enqueued launch by launch again)


@pytest.mark.parametrize("name", R.NAMES)
def test_case_is_what_its_name_claims(name):
    c = R.get(name)
    n, rp, col, val = c.n, c.row_ptr.astype(np.int64), c.col.astype(np.int64), c.val
    rows = np.repeat(np.arange(n), np.diff(rp))
    # tridiagonal, sorted, symmetric, the diagonal = 0.02 - the row's off-diagonals, which lie in (-1, -0.75]
    assert int(rp[-1]) == 3 * n - 2 if n > 1 else int(rp[-1]) == 1
    assert np.all(np.abs(rows - col) <= 1) and np.all(np.diff(col)[rows[1:] == rows[:-1]] > 0)
    off = rows != col
    assert np.all((val[off] > -1.0) & (val[off] <= -0.75))
    per_tile = E._per_tile_unique(rows[off] // R.TILE_ROWS, val[off].view(np.uint64), -(-n // R.TILE_ROWS)) if n > 1 else np.zeros(1)
    assert (per_tile.max() if name == "form_tile_tables" else len(np.unique(val[off]))) <= 1023
    upper, lower = off & (col > rows), off & (col < rows)
    assert np.array_equal(val[upper], val[lower]) and np.array_equal(rows[upper], col[lower])
    diag = val[~off]
    assert len(diag) == n and np.allclose(diag + np.bincount(rows[off], weights=val[off], minlength=n), R.SHIFT, rtol=0, atol=4e-15)
    assert np.all((np.abs(c.x0) >= 0.5) & (np.abs(c.x0) <= 1.5)) and c.b.shape == (n,)
    assert c.env["AVS_CG_RESIDENT"] == "0" and c.env["AVS_PCG_FUSE_VECTORS"] == "0" and set(c.env) <= set(R.PHASE_ENV)

    p, e, fmt = c.props, c.expect(), c.format()
    assert p["n"] == n
    assert e["g"] == R.vec_grid(n) == min(-(-n // 256), 2048)
    codes = fmt["value_table_size"] > 0
    if name.startswith("rows_"):
        assert c.few_rows and e["g"] == p["g"] and -(-n // R.TILE_ROWS) == p["tiles"] and e["coded"] == 1 and e["nb"] == 8 * p["tiles"]
    if name.startswith("nb_"):
        assert n % 2 == 1 and e["coded"] == 1 and e["nb"] == p["nb"] == 8 * -(-n // R.TILE_ROWS) and e["alpha_folded"] == p["alpha_folded"]
        assert (n - 1) % R.TILE_ROWS == 0, "the smallest n with that many tiles"
        assert (p["nb"] > R.BLOCK, p["nb"] > R.FOLD_BATCH * R.BLOCK, p["nb"] > R.FUSE_ALPHA_MAX) == \
            {"nb_264": (True, False, False), "nb_2056": (True, True, False), "nb_4104": (True, True, True)}[name]
        assert p["nb"] - 8 <= {"nb_264": R.BLOCK, "nb_2056": R.FOLD_BATCH * R.BLOCK, "nb_4104": R.FUSE_ALPHA_MAX}[name]
        assert c.ks == R.KS + R.KS_NB
    if "form" in p:
        assert n == R.N_SWITCH or name == "form_tile_tables"
        distinct = len(np.unique(val.view(np.uint64)))
        if p["form"] == "one dictionary, coded diagonal":
            assert codes and not fmt["tile_local_tables"] and distinct == fmt["value_table_size"] <= R.CODED_MAX and e["coded"] == 1
        elif p["form"] == "plain":
            assert not codes and e["coded"] == 0 and e["nb"] == -(-n // R.TILE_ROWS) and c.env["AVS_VALUE_INDEX"] == "0"
        elif p["form"] == "one dictionary, plain diagonal":
            assert codes and not fmt["tile_local_tables"] and R.CODED_MAX < distinct == fmt["value_table_size"] <= E.DICT_MAX and e["coded"] == 0
        elif p["form"] == "tile-local tables":
            assert codes and fmt["tile_local_tables"] == 1 and distinct > p["distinct_over"] == 65536 and e["coded"] == 0 and n % 2 == 1
        else:
            raise AssertionError(p["form"])
        if n == R.N_SWITCH:
            assert c.ks == R.KS + R.KS_CHUNKS and c.exits and e["nb"] == (72 if codes else 9) and e["g"] == 17
    if "same_matrix_as" in p:
        o = R.get(p["same_matrix_as"])
        assert np.array_equal(o.val, val) and np.array_equal(o.col, c.col) and np.array_equal(o.b, c.b) and np.array_equal(o.x0, c.x0)
    if name.startswith("beta"):
        assert e["fuse_beta"] == int(name[4]) and c.graph == bool(int(name[-1])) and e["alpha_folded"] == bool(e["fuse_beta"])


@pytest.mark.parametrize("name", R.NAMES)
def test_case_conditions(name):
    c = R.get(name)
    model = R.model_of(c)
    ks = R.checked_ks(c, model)
    live = model.live_passes()
    print(f"\n{name}: n = {c.n}, model passes {model.passes}, live {live}, checked k = {ks[0]}..{ks[-1]} ({len(ks)})")
    assert ks[0] == 0 and np.array_equal(model.ld.x[0].astype(np.float64), c.x0)
    if c.few_rows:
        assert ks == tuple(range(live + 1)) and (c.n < 255) == (live < R.FEW_ROWS_PASSES)
    else:
        assert ks == c.ks and live >= ks[-1], (ks, live)      # every case is live up to its largest checked k
    for k in ks:
        sx, se = model.s[k]
        print(f"  k = {k:3d}  s_k(x) = {sx:.2e}  s_k(error) = {se:.2e}  bound_x = {model.bound_x(k):.2e}  error = {float(model.ld.error[k]):.3e}")
        assert model.ld.iterations[k] == k and not model.ld.converged[k]
        assert model.bound_x(k) <= 1e-9 and model.bound_error(k) <= 1e-9, (k, model.bound_x(k), model.bound_error(k))
    # the exits: every target admissible for this seed, and met exactly by the three runs; the cap equal to the converging iteration too
    targets = R.exit_targets(c, model)
    assert len(targets) == (len(R.EXIT_ITERATIONS) if c.exits else 0) and all(t is not None for t in targets), targets
    if c.exits:
        its = [t[2] for t in targets]
        assert its[0] in (3, 4) and its[1:5] == [31, 32, 33, 34] and 2 * R.K_CHUNK < its[5] <= 3 * R.K_CHUNK, its
    for tol_e, iters, it in targets:
        rr = [float(v) for v in model.ld.rr]
        assert it == iters + 1 and rr[it] < min(rr[:it]) and model.exits_are_clear(tol_e, iters, 1e-6)
        for mode in P.MODES:
            for cap in (R.EXIT_MAX_ITERATIONS, it):
                q = P.run(model.A, c.b, c.x0, tol_e, cap, mode)
                assert q.converged[-1] and q.iterations[-1] == iters and q.passes == it, (mode, cap, tol_e, iters, q.iterations[-1])
        print(f"  exit: tol = {tol_e:.6e} -> converges in iteration {it} (position {(it - 1) % R.K_CHUNK} of chunk {(it - 1) // R.K_CHUNK})")
