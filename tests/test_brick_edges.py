"""The planted cases of tests/brick_edges.py reach the edges they name -- checked with the model (tests/brick_model.py), without a GPU."""
import numpy as np
import pytest

import brick_edges as E
import brick_model as M

pytestmark = pytest.mark.usefixtures("built_lib")


def test_the_limits_come_from_the_probe_library():
    """every case is placed from avs_brick_form_probe's limits-only call: a changed constant moves the cases (or fails the table below)"""
    L = E.limits()
    assert L.ready == 0 and L.tiles == 0           # the call built nothing
    for k in ("run_len", "max_runs", "fast_runs", "pat_max", "pat_words", "pat_words_vc", "pat_len", "x_slots", "park_words", "emode_words",
              "emode_words_mixed", "min_rows", "max_rows", "etile_rows", "tile_vals", "table_max", "block_words", "header_words"):
        assert getattr(L, k) > 0, k
    assert L.emode_words == M.LOFF[-1] + (-M.LOFF[-1]) % 16          # the lattices, padded to 16 slots
    assert L.fast_runs < L.max_runs and L.park_words < 2 * 512 < L.emode_words
    assert tuple(E.cases()) == E.NAMES


def test_every_edge_is_reached_on_each_side(capsys):
    cases, missing, lines = E.cases(), [], []
    for edge, side, name, fact in E.edges():
        c = cases[name]
        ok = bool(fact(c.target_tiles(), c.model().tiles))
        lines.append(f"{'ok ' if ok else 'NOT'}  {edge:66s} {side:32s} {name}")
        if not ok:
            missing.append((edge, side, name))
    with capsys.disabled():
        print("\nedges of the brick form and the case on each side:\n" + "\n".join(lines))
    assert not missing, missing
    by_edge = {}
    for edge, side, name, _ in E.edges():
        by_edge.setdefault(edge, []).append(side)
    assert all(len(s) >= 1 for s in by_edge.values())
    assert set(n for _, _, n, _ in E.edges()) == set(E.NAMES), set(E.NAMES) - set(n for _, _, n, _ in E.edges())   # no case without an edge


def test_exactly_one_racy_case():
    racy = [c.name for c in E.cases().values() if c.racy_extras]
    assert racy == ["extras_racy"]
    assert [c.name for c in E.cases().values() if c.model().racy] == racy        # and the model agrees: nothing else overflows the candidate set


@pytest.mark.parametrize("name", E.NAMES)
def test_case_is_valid(name):
    c = E.cases()[name]
    assert c.n_rows < 60000 and c.n_cols >= c.n_rows and len(c.col) < 2 ** 24
    assert c.row_ptr[0] == 0 and np.all(np.diff(c.row_ptr) > 0)                   # no empty row
    assert c.col.min() >= 0 and c.col.max() < c.n_cols
    for r in (0, c.n_rows // 2, c.n_rows - 1):
        cols = c.col[c.row_ptr[r]:c.row_ptr[r + 1]]
        assert r in cols and len(set(cols.tolist())) == len(cols)                 # the diagonal, no duplicate column
    brick = M.geometry(c.dof, c.nx, c.ny, c.nz)[5]
    assert np.all(np.diff(brick[:c.n_rows]) >= 0)                                 # brick-major
    assert len({tuple(d) for d in c.dof.tolist()}) == c.n_cols                    # a face per column
    assert np.array_equal(c.val, c.val.astype(np.float32).astype(np.float64))   # float values: every kernel may run it
    assert name.startswith("golden") or np.all(c.val != 0)                       # (an assembled matrix stores a few explicit zeros)
    assert c.model().ready and (c.n_cols > c.n_rows) == name.startswith("halo")


def test_golden_dof_table_is_the_oracles():
    """the dof table a golden case derives from the fixture's index fields is what the CPU oracle reports for the fixture's scene"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden
    from util import oracle_for_scene
    c = E.cases()["golden_sphere16_L3"]
    o = oracle_for_scene(make_golden.scene_from_fixture(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sphere16_L3.npz"))))
    o.prepass()
    o.hot_path()
    assert np.array_equal(o.dof_table(0), c.ref_dof)
