"""Named small systems for avs_check_solution / avs_check_csr_solution: the smallest shapes at which k_solution_check can go wrong.

A chunk is 256 consecutive rows (one workgroup trip), a tile 4096 products in LDS (kStreamCap), the fold adds 256 partial sums per trip.
Every case carries the property it is there for in `why`; test_solution_check_model.py proves from the model that it has it."""
import functools

import numpy as np

import csr_check_cases as cc

CHUNK, TILE = 256, 4096


class Case:
    def __init__(self, name, why, row_ptr, col, val, b, x, x0=None, seam_a_only=False):
        self.name, self.why = name, why
        self.row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        self.col = np.ascontiguousarray(col, np.int32)
        self.val = np.ascontiguousarray(val, np.float64)
        self.n, self.nnz = len(self.row_ptr) - 1, len(self.col)
        self.b = np.ascontiguousarray(b, np.float64)
        self.x = np.ascontiguousarray(x, np.float64)
        self.x0 = None if x0 is None else np.ascontiguousarray(x0, np.float64)
        self.seam_a_only = seam_a_only      # rules 0 / 1 of avs_check_csr are violated: evaluated = 0

    def __repr__(self):
        return f"Case({self.name}, n={self.n}, nnz={self.nnz})"

    def arrays(self):
        return self.row_ptr, self.col, self.val, self.b, self.x, self.x0


def _vectors(n, seed, count=3):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n) for _ in range(count)]


def _tri(n, name=None, why="", edit=None, x0=True):
    """the strictly dominant tridiagonal system of csr_check_cases with an x near nothing in particular and an initial guess"""
    t = cc.tridiagonal(n)
    b, x, g = _vectors(n, 8100 + n)
    f = dict(row_ptr=t.row_ptr.copy(), col=t.col.copy(), val=t.val.copy(), b=b, x=x, x0=g if x0 else None)
    if edit:
        edit(f)
    return Case(name or f"tri_{n}", why, **f)


def _drop_rows(f, rows):
    rp, keep = f["row_ptr"].astype(np.int64), np.ones(len(f["col"]), bool)
    for r in rows:
        keep[rp[r]:rp[r + 1]] = False
    length = np.diff(rp)
    length[list(rows)] = 0
    f["row_ptr"] = np.concatenate([[0], np.cumsum(length)])
    f["col"], f["val"] = f["col"][keep], f["val"][keep]


def _from_rows(name, why, n, rows, seed, **kw):
    """rows: {row: (cols, vals)}; every other row is empty"""
    length = np.zeros(n, np.int64)
    for r, (c, _) in rows.items():
        length[r] = len(c)
    rp = np.concatenate([[0], np.cumsum(length)])
    col = np.concatenate([np.asarray(rows[r][0], np.int64) for r in sorted(rows)] or [np.zeros(0, np.int64)])
    val = np.concatenate([np.asarray(rows[r][1], np.float64) for r in sorted(rows)] or [np.zeros(0)])
    b, x, g = _vectors(n, seed)
    f = dict(b=b, x=x, x0=g)
    f.update(kw)
    return Case(name, why, rp, col, val, **f)


def _long_row():
    n, rng = 5000, np.random.default_rng(8201)
    rows = {i: ([i], [2.0 + (i % 5)]) for i in range(n)}
    rows[2500] = (rng.permutation(n)[:TILE + 1], rng.standard_normal(TILE + 1))
    return _from_rows("long_row_4097", "one row of 4,097 entries: longer than one LDS tile, and its chunk has rows before and behind it", n, rows, 8202)


def _tile_straddle():
    n, per, rng = 300, 17, np.random.default_rng(8203)      # chunk 0: 256 rows x 17 = 4,352 entries; entry 4,096 is entry 16 of row 240
    rows = {i: ((i + 7 * np.arange(per)) % n, rng.standard_normal(per)) for i in range(n)}
    return _from_rows("tile_straddle", "a chunk of 4,352 entries: the tile boundary falls inside row 240", n, rows, 8204)


def _unordered_repeated():
    n, rng = 70, np.random.default_rng(8205)
    rows = {}
    for i in range(n):
        c = rng.integers(0, n, size=int(rng.integers(0, 9)))
        if len(c) >= 2:
            c[-1] = c[0]                                      # a repeated column, apart from each other
        rows[i] = (c, rng.standard_normal(len(c)))
    return _from_rows("unordered_repeated", "unordered rows with repeated columns (and a few empty rows)", n, rows, 8206)


def _cancellation():
    rows = {0: ([0, 1, 2], [1e16, 1.0, -1e16]), 1: ([0, 2, 1], [1e16, -1e16, 1.0]), 2: ([2, 0, 1], [-1e16, 1e16, 1.0])}
    return _from_rows("cancellation", "[1e16, 1, -1e16] . [1, 1, 1]: 0, 1 or 1 by the order alone", 3, rows, 8207, x=np.ones(3), b=np.zeros(3), x0=np.zeros(3))


def _diagonal(name, why, n, seed, edit=None, exact=False):
    i = np.arange(n)
    d = 2.0 ** ((i % 7) - 3)                                   # powers of two: b / d is exact
    b, x, g = _vectors(n, seed)
    if exact:
        x = b / d
    f = dict(row_ptr=np.arange(n + 1), col=i, val=d, b=b, x=x, x0=g)
    if edit:
        edit(f)
    return Case(name, why, **f)


def _set(key, index, value):
    def edit(f):
        f[key] = f[key].copy()
        f[key][index] = value
    return edit


def _neg_zero(f):
    f["val"][f["row_ptr"][10]] = -0.0
    f["val"][f["row_ptr"][11] + 1] = -0.0
    f["x"][12], f["x"][13], f["b"][13], f["b"][14], f["x0"][12] = -0.0, -0.0, -0.0, -0.0, -0.0


def _zero(*keys):
    def edit(f):
        for k in keys:
            f[k] = np.zeros_like(f[k])
    return edit


def _bad_column(f):
    f["col"][f["row_ptr"][200] + 1] = len(f["b"])


def _bad_row_ptr(f):
    f["row_ptr"][100] = f["row_ptr"][101] + 1


BUILDERS = {
    "n_0": lambda: Case("n_0", "no rows", [0], [], [], [], [], []),
    "n_1": lambda: Case("n_1", "one row, diagonal only", [0, 1], [0], [4.0], [1.0], [0.3], [0.0]),
    "tri_255": lambda: _tri(255, why="one chunk, its last lane idle"),
    "tri_256": lambda: _tri(256, why="exactly one chunk"),
    "tri_257": lambda: _tri(257, why="a second chunk of one row"),
    "tri_257_no_x0": lambda: _tri(257, "tri_257_no_x0", "no initial guess: the update figures are 0", x0=False),
    "tri_65537": lambda: _tri(65537, why="257 chunks: the fold takes a second trip per thread"),
    "empty_rows": lambda: _tri(300, "empty_rows", "an empty row in the middle and one as the last row: r_i = b_i", lambda f: _drop_rows(f, (150, 299))),
    "long_row_4097": _long_row,
    "tile_straddle": _tile_straddle,
    "unordered_repeated": _unordered_repeated,
    "cancellation": _cancellation,
    "nan_x_own_row": lambda: _diagonal("nan_x_own_row", "NaN in an x_i that only its own row reads: one row leaves the sums", 300, 8208, _set("x", 17, np.nan)),
    "nan_x_three_rows": lambda: _tri(300, "nan_x_three_rows", "NaN in an x_i that three rows read", _set("x", 100, np.nan)),
    "inf_b": lambda: _tri(300, "inf_b", "Inf in one b_i", _set("b", 5, np.inf)),
    "nan_x0": lambda: _tri(300, "nan_x0", "NaN in one x0_i: the row leaves the update figures only", _set("x0", 7, np.nan)),
    "neg_zero": lambda: _tri(64, "neg_zero", "-0.0 among val, x, b and x0", _neg_zero),
    "b0_x0": lambda: _tri(40, "b0_x0", "b = 0 and x = 0: relative residual 0", _zero("b", "x")),
    "b0_x_nonzero": lambda: _tri(40, "b0_x_nonzero", "b = 0, x != 0: relative residual +Inf", _zero("b")),
    "diagonal_exact": lambda: _diagonal("diagonal_exact", "x the exact solution of a diagonal system: r == 0 in every row", 600, 8209, exact=True),
    "bad_column": lambda: _tri(300, "bad_column", "one column == n: rule 1 of avs_check_csr", _bad_column),
    "bad_row_ptr": lambda: _tri(300, "bad_row_ptr", "a row pointer that runs backwards: rule 0 of avs_check_csr", _bad_row_ptr),
}
SEAM_A_ONLY = ("bad_column", "bad_row_ptr")
NAMES = [n for n in BUILDERS if n not in SEAM_A_ONLY]
ALL_NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    c.seam_a_only = name in SEAM_A_ONLY
    assert c.name == name
    return c
