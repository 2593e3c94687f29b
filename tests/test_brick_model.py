"""tests/brick_model.py against lattices small enough to derive every count by hand (the expected numbers below come from the geometry, worked
out in the comments -- not from the model)."""
import numpy as np
import pytest

import brick_edges as E
import brick_model as M
from oracle import oracle as O

pytestmark = pytest.mark.usefixtures("built_lib")


def build(faces, links, nb, vals=(1.0, 2.0)):
    """faces: [(level, axis, i, j, k)] in row order; links: row -> [row]; the diagonal gets vals[0], every other entry vals[1]"""
    dof = np.array([[l | (a << 8), i, j, k] for l, a, i, j, k in faces], np.int32)
    rp, col, val = [0], [], []
    for r in range(len(faces)):
        cols = sorted({r} | set(links.get(r, ())))
        col += cols
        val += [vals[0] if c == r else vals[1] for c in cols]
        rp.append(len(col))
    return M.model(np.array(rp), np.array(col), np.array(val), dof, len(faces), 8 * nb[0], 8 * nb[1], 8 * nb[2], E.limits())


def facts(T):
    return (T.kind, T.row0, T.nrows, T.npat, T.nruns, T.npq, T.nprow, T.nsrows, T.nsw)


def test_lattice_constants():
    assert M.LOFF.tolist() == [0, 3000, 3648, 3840, 3921]       # 3 x 10^3, + 3 x 6^3, + 3 x 4^3, + 3 x 3^3
    ob = (2, 1, 0)
    one = lambda l, a, i, j, k: int(M.lattice_slot(*[np.array([v]) for v in (l, a, i, j, k)], ob)[0])
    assert one(0, 0, 16, 8, 0) == ((1 * 10 + 1) * 10 + 1) * 3              # the brick's first cell sits at (1, 1, 1) of the padded lattice
    assert one(0, 2, 15, 7, 0) == ((1 * 10 + 0) * 10 + 0) * 3 + 2          # one cell outside in x and y
    assert one(0, 0, 14, 8, 0) == -1 and one(0, 0, 25, 8, 0) == -1         # two cells outside: off the lattice
    assert one(1, 1, 8, 4, 0) == 3000 + ((1 * 6 + 1) * 6 + 1) * 3 + 1
    assert one(3, 0, 2, 1, 0) == 3840 + ((1 * 3 + 1) * 3 + 1) * 3
    assert one(4, 0, 1, 0, 0) == -1                                        # no lattice of level 4


def test_full_brick():
    """8^3 cells x 3 faces = 1536 rows, cell-major; a row reads itself and the face of its axis one cell further in x (not at x = 7).
    Tiles: rows 0 .. 1023 and 1024 .. 1535, one origin.  Patterns: per axis one of two entries and one of one entry (x = 7): 6, a quad each.
    Row 1023 is (cell 341, axis 0); cell 340 = (4, 2, 5) reads cell 341: its axis-0 face is row 1023 (own), its faces of axes 1 and 2 are
    rows 1024 and 1025 of the second tile -- consecutive slots, consecutive columns: ONE fill run.  The second tile reads forward only: none."""
    faces = [(0, a, x, y, z) for z in range(8) for y in range(8) for x in range(8) for a in range(3)]
    links = {r: [r + 3] for r, f in enumerate(faces) if f[2] < 7}
    m = build(faces, links, (1, 1, 1))
    assert [facts(T) for T in m.tiles] == [("G", 0, 1024, 6, 1, 6, 1024, 0, 0), ("G", 1024, 512, 6, 0, 6, 512, 0, 0)]
    assert m.tiles[0].origin == m.tiles[1].origin == (0, 0, 0)
    assert (m.patterns, m.pattern_rows, m.streamed_rows, m.streamed_words, m.order) == (6, 1536, 0, 0, [0, 1])
    assert m.headers[1, :12].tolist() == [1024, 512, 6, 0, 6, 512, 1024, 0, 0, 0, 1024, 0]


def test_two_small_bricks():
    """30 + 33 rows in two bricks: a run of small bricks, ONE E tile of 63 rows whose words are all the entries (63 + 20 links)"""
    faces = [(0, a, x, 0, 0) for x in range(8) for a in range(3)] + [(0, a, x, 1, 0) for x in range(2) for a in range(3)]
    faces += [(0, a, 8 + x, 0, 0) for x in range(8) for a in range(3)] + [(0, a, 8 + x, 1, 0) for x in range(3) for a in range(3)]
    links = {r: [r + 1] for r in range(0, 60, 3)}
    m = build(faces, links, (2, 1, 1))
    assert [facts(T) for T in m.tiles] == [("E", 0, 63, 0, 0, 0, 0, 63, 83)]
    assert (m.patterns, m.pattern_rows, m.streamed_rows, m.streamed_words) == (0, 0, 63, 83)


def test_brick_with_a_coarse_neighbour():
    """brick 0: 22 level-0 cells (66 rows, a G tile); brick 1: ONE level-3 cell (3 rows, an E tile).  The rows of the cells at x = 7 (cells
    7 and 15: 6 rows) read the level-3 face of their axis.  On brick 0's level-3 lattice (3 cells per axis, origin cell at 1) that cell is
    (2, 1, 1): slot 3840 + 3 ((1 x 3 + 1) x 3 + 2) + a = 3882 + a; every level-0 row's base there is 3840 + 3 ((1 x 3 + 1) x 3 + 1) = 3879: delta 3 + a for
    both cells, so 3 patterns of two entries + 3 of one.  The three coarse faces are consecutive slots and consecutive columns 66, 67, 68:
    one fill run.  Execution order: 60 rows of one entry (level-0 only), then 6 of two (not level-0 only): the first wave of 64 mixes them."""
    cells = [(x, y, 0) for y in range(3) for x in range(8)][:22]
    faces = [(0, a) + c for c in cells for a in range(3)] + [(3, a, 1, 0, 0) for a in range(3)]
    links = {r: [66 + f[1]] for r, f in enumerate(faces[:66]) if f[2] == 7}
    m = build(faces, links, (2, 1, 1))
    assert [facts(T) for T in m.tiles] == [("G", 0, 66, 6, 1, 6, 66, 0, 0), ("E", 66, 3, 0, 0, 0, 0, 3, 3)]
    assert m.tiles[0].mixed_waves == 1 and m.patterns == 6
    assert m.headers[1, :12].tolist() == [66, 3, 0, 0, 0, 0, 66, 3, 0, 3, 66, 0]


def test_the_patterns_a_tile_keeps_are_a_prefix():
    """the first pattern that does not fit ends the prefix: a later, shorter one is not kept either (k_bk_tile: `i == kept`)"""
    L = E.limits()
    c = E.cases()["patwords_cap+"]
    T = c.target_tiles()[0]
    assert T.npat_seen - T.npat == 1 and 4 * T.npq == L.pat_words and T.nsrows == 2


def test_reference_row_sums_are_left_to_right():
    """the oracle's spmv_csr, the reference of the GPU test, adds in stored order without FMA: checked against Python floats"""
    c = E.cases()["shapes"]
    y = O.spmv_csr(c.row_ptr.astype(np.int64), c.col, c.val, c.x)
    for r in (0, 301, c.n_rows - 1):
        s = 0.0
        for k in range(c.row_ptr[r], c.row_ptr[r + 1]):
            s += float(c.val[k]) * float(c.x[c.col[k]])
        assert s == y[r]
