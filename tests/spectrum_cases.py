"""Named small systems for avs_estimate_spectrum / avs_estimate_csr_spectrum: the smallest shapes at which its kernels can go wrong.

A chunk is 256 consecutive rows (one workgroup trip and one partial sum), a tile 4096 products in LDS (kStreamCap), the fold adds 256
partial sums per trip.  Every case is symmetric with a positive diagonal unless it is there for the opposite, runs with both operators
unless `ops` says otherwise, and carries the property it is there for in `why`; test_spectrum_model.py proves from the model that it has it."""
import functools

import numpy as np

import csr_check_cases as cc
import spectrum_model as M

CHUNK, TILE = 256, 4096
BOTH = (M.JACOBI, M.MATRIX)


class Case:
    def __init__(self, name, why, row_ptr, col, val, b, x0, ops=BOTH, steps=12, start=M.RESIDUAL, given=None):
        self.name, self.why = name, why
        self.row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        self.col = np.ascontiguousarray(col, np.int32)
        self.val = np.ascontiguousarray(val, np.float64)
        self.n, self.nnz = len(self.row_ptr) - 1, len(self.col)
        self.b = np.ascontiguousarray(b, np.float64)
        self.x0 = np.ascontiguousarray(x0, np.float64)
        self.given = None if given is None else np.ascontiguousarray(given, np.float64)
        self.ops, self.steps, self.start = tuple(ops), steps, start
        self.seam_a_only = False            # rules 0 / 1 of avs_check_csr are violated: evaluated = 0

    def __repr__(self):
        return f"Case({self.name}, n={self.n}, nnz={self.nnz}, steps={self.steps})"

    def model(self, op, order="fsum", steps=None, tolerance=1e-3):
        return M.estimate(self.row_ptr, self.col, self.val, self.b, self.x0, self.given, op, self.start, self.steps if steps is None else steps,
                          tolerance, order)


def _vectors(n, seed, count=2):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n) for _ in range(count)]


def _of(system, name, why, edit=None, seed=None, **kw):
    """a csr_check_cases.System (symmetric pattern, strictly dominant, rows ascending) with a right-hand side and a guess of its own"""
    b, x0 = _vectors(system.n, 9100 + system.n if seed is None else seed)
    f = dict(row_ptr=system.row_ptr.copy(), col=system.col.copy(), val=system.val.copy(), b=b, x0=x0)
    if edit:
        edit(f)
    return Case(name, why, **f, **kw)


def _tri(n, name=None, why="", edit=None, **kw):
    return _of(cc.tridiagonal(n), name or f"tri_{n}", why, edit, **kw)


def _arrow():
    n, hub = 5000, 100
    j = np.delete(np.arange(n), hub)
    rows = np.concatenate([np.full(n, hub), j, j])
    cols = np.concatenate([np.arange(n), np.full(n - 1, hub), j])
    def spread_diagonal(f):                                             # (diagonal 2 everywhere else: a Krylov space of three dimensions)
        at = np.repeat(np.arange(n), np.diff(f["row_ptr"]))
        f["val"][f["col"] == at] += (at[f["col"] == at] % 7) * 0.5

    return _of(cc._from_entries("arrow", n, rows, cols, 9200), "arrow",
               "row 100 holds all 5,000 columns: longer than one LDS tile, with rows before and behind it in its chunk", spread_diagonal, steps=8)


def _unordered_repeated(f):
    rp, rng = f["row_ptr"].astype(np.int64), np.random.default_rng(9201)
    col, val = f["col"].astype(np.int64), f["val"].copy()
    for i in range(len(rp) - 1):                                        # the entries permuted inside their rows
        p = rng.permutation(rp[i + 1] - rp[i]) + rp[i]
        col[rp[i]:rp[i + 1]], val[rp[i]:rp[i + 1]] = col[p], val[p]

    def split(row, column, first):
        """entry (row, column) becomes two entries of that column: `first` of its value at the start of the row, the rest where it was"""
        k = rp[row] + int(np.flatnonzero(col[rp[row]:rp[row + 1]] == column)[0])
        keep = val[k] * (1 - first)
        return np.insert(col, rp[row], column), np.insert(np.concatenate([val[:k], [keep], val[k + 1:]]), rp[row], val[k] * first)

    col, val = split(40, 41, 0.25)                                      # an off-diagonal in two parts: the operator stays symmetric
    rp[41:] += 1
    col, val = split(200, 200, 0.25)                                    # a diagonal in two parts: d_200 is the LAST one, 0.75 of the sum
    rp[201:] += 1
    f.update(row_ptr=rp, col=col, val=val)


def _diagonal(name, why, n, d, seed, exact=False, **kw):
    b, x0 = _vectors(n, seed)
    if exact:
        b = d * x0
    return Case(name, why, np.arange(n + 1), np.arange(n), d, b, x0, **kw)


def _laplace(n):
    i = np.arange(n)
    rows, cols = np.concatenate([i, i[1:], i[:-1]]), np.concatenate([i, i[:-1], i[1:]])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    b, x0 = _vectors(n, 9300)
    return Case(f"laplace_{n}", "tridiag(-1, 2, -1): condition 4e5, eigenvalues 2 - 2 cos(k pi / 1001) known", rp, cols, np.where(rows == cols, 2.0, -1.0), b, x0,
                ops=(M.MATRIX,), steps=64)


def _drop_row(row):
    def edit(f):
        rp = f["row_ptr"].astype(np.int64)
        keep = np.ones(len(f["col"]), bool)
        keep[rp[row]:rp[row + 1]] = False
        length = np.diff(rp)
        length[row] = 0
        f.update(row_ptr=np.concatenate([[0], np.cumsum(length)]), col=f["col"][keep], val=f["val"][keep])
    return edit


def _set_diagonal(row, value):
    def edit(f):
        rp = f["row_ptr"]
        k = rp[row] + int(np.flatnonzero(f["col"][rp[row]:rp[row + 1]] == row)[0])
        f["val"][k] = value
    return edit


def _shift(by):
    def edit(f):
        rows = np.repeat(np.arange(len(f["row_ptr"]) - 1), np.diff(f["row_ptr"]))
        f["val"][f["col"] == rows] += by
    return edit


def _nan_pair(f):
    rp = f["row_ptr"]
    f["val"][rp[10] + 2] = np.nan           # (10, 11)
    f["val"][rp[11]] = np.nan               # (11, 10)


def _set(key, index, value):
    def edit(f):
        f[key][index] = value
    return edit


def _bad_column(f):
    f["col"][f["row_ptr"][200] + 1] = len(f["b"])


def _bad_row_ptr(f):
    f["row_ptr"][100] = f["row_ptr"][101] + 1


BUILDERS = {
    "n_0": lambda: Case("n_0", "no rows", [0], [], [], [], []),
    "n_1": lambda: Case("n_1", "one row: a Krylov space of dimension 1, breakdown at step 1", [0, 1], [0], [4.0], [1.0], [0.0]),
    "tri_3": lambda: _tri(3, why="n < steps: three steps are taken", steps=8),
    "tri_12": lambda: _tri(12, why="12 steps on 12 rows: every eigenvalue", steps=12),
    "tri_255": lambda: _tri(255, why="one chunk, its last lane idle"),
    "tri_256": lambda: _tri(256, why="exactly one chunk"),
    "tri_257": lambda: _tri(257, why="a second chunk of one row"),
    "tri_257_hash": lambda: _tri(257, "tri_257_hash", "the hash start vector", start=M.HASH),
    "tri_257_vector": lambda: _tri(257, "tri_257_vector", "a start vector of the caller's", start=M.VECTOR, given=_vectors(257, 9202, 1)[0]),
    "tri_65537": lambda: _tri(65537, why="257 chunks: the fold takes a second trip per thread", steps=8),
    "blocks": lambda: _of(cc.blocks(), "blocks", "chunk 0 holds 7,814 products: a tile boundary falls inside a row"),
    "arrow": _arrow,
    "unordered_repeated": lambda: _tri(300, "unordered_repeated", "unordered rows, an off-diagonal and a diagonal in two entries: the LAST diagonal entry scales",
                                       _unordered_repeated),
    "identity_600": lambda: _diagonal("identity_600", "a diagonal matrix under the Jacobi scale is the identity to rounding: breakdown at step 1", 600,
                                      2.0 + (np.arange(600) % 5), 9203, ops=(M.JACOBI,)),
    "laplace_1000": lambda: _laplace(1000),
    "no_diagonal": lambda: _tri(300, "no_diagonal", "an empty row: bad_diagonal = 1", _drop_row(150), ops=(M.JACOBI,)),
    "negative_diagonal": lambda: _tri(300, "negative_diagonal", "one diagonal < 0: bad_diagonal = 1", _set_diagonal(7, -3.0), ops=(M.JACOBI,)),
    "nan_diagonal": lambda: _tri(300, "nan_diagonal", "one NaN diagonal (and a zero one): bad_diagonal = 2",
                                 lambda f: (_set_diagonal(299, np.nan)(f), _set_diagonal(0, 0.0)(f)), ops=(M.JACOBI,)),
    "indefinite": lambda: _tri(300, "indefinite", "tri_300 - 4 I: every eigenvalue negative, indefinite = 1", _shift(-4.0), ops=(M.MATRIX,)),
    "zero_start": lambda: _diagonal("zero_start", "b = A x0 exactly (powers of two): the start vector is 0, no step", 300, 2.0 ** ((np.arange(300) % 7) - 3),
                                    9204, exact=True),
    "nan_start": lambda: _tri(300, "nan_start", "NaN in one b_i: the start norm is not finite, no step", _set("b", 5, np.nan)),
    "nan_value": lambda: _tri(300, "nan_value", "a NaN pair off the diagonal under the hash start: alpha[0] is not finite, one step", _nan_pair, start=M.HASH),
    "bad_column": lambda: _tri(300, "bad_column", "one column == n: rule 1 of avs_check_csr", _bad_column),
    "bad_row_ptr": lambda: _tri(300, "bad_row_ptr", "a row pointer that runs backwards: rule 0 of avs_check_csr", _bad_row_ptr),
}
SEAM_A_ONLY = ("bad_column", "bad_row_ptr")
BAD_DIAGONAL = {"no_diagonal": 1, "negative_diagonal": 1, "nan_diagonal": 2}
# (case, operator) -> the step of the breakdown, the same under all three summation orders.  The Jacobi-scaled arrow is the identity plus
# a matrix of rank two: a Krylov space of three dimensions.
BREAKDOWN_AT = {("n_1", M.JACOBI): 1, ("n_1", M.MATRIX): 1, ("tri_3", M.JACOBI): 3, ("tri_3", M.MATRIX): 3, ("tri_12", M.JACOBI): 12,
                ("tri_12", M.MATRIX): 12, ("identity_600", M.JACOBI): 1, ("arrow", M.JACOBI): 3}
NO_STEP = ("n_0", "zero_start", "nan_start")
ALL_NAMES = list(BUILDERS)
NAMES = [n for n in ALL_NAMES if n not in SEAM_A_ONLY]


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    c.seam_a_only = name in SEAM_A_ONLY
    assert c.name == name
    return c


@functools.lru_cache(maxsize=None)
def runs():
    """every (case, operator) pair"""
    return tuple((name, op) for name in ALL_NAMES for op in case(name).ops)


@functools.lru_cache(maxsize=None)
def model(name, op, order="fsum"):
    """the model's answer, computed once and left unchanged"""
    return case(name).model(op, order)


@functools.lru_cache(maxsize=None)
def spread(name, op):
    """what a correct device may differ by: the relative spread between the forward and the reverse sums of (lambda_min, lambda_max, the
    Ritz values against the largest of them); 0 where no step is taken or the two orders stop at different steps"""
    f, r = model(name, op, "forward"), model(name, op, "reverse")
    if not f["steps_taken"] or f["steps_taken"] != r["steps_taken"] or f["nonfinite"]:
        return 0.0, 0.0, 0.0
    lo, hi = (abs(f[k] - r[k]) / max(abs(f[k]), abs(r[k])) for k in ("lambda_min", "lambda_max"))
    return lo, hi, float(np.abs(f["ritz"] - r["ritz"]).max() / np.abs(f["ritz"]).max())
