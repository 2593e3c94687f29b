"""Named edge cases of the device triplet merge (csrc/avs_assembly.hip: k_wave_slots, k_unique_rows, k_unique_long, k_merge_rows,
k_merge_long), placed from the limits the kernels were compiled with (avs_merge_triplets_probe's info struct) and a fixed seed.

A case is a set of rows of raw triplets (emission order) plus what it is meant to reach: the row-length class of named rows ("reg": one
thread in registers, "wave": the whole wave, "long": the list of long rows), whether named 64-row waves are staged in LDS, the number of
long rows, and the rows whose values must expose a wrong fold (tests/test_triplet_edges.py checks all of that on the CPU;
tests/test_gpu_triplet_merge.py runs the cases).  Values are +-[1, 2) x 2^-20..2^20, so additions round visibly; Case.arrays(f32=True)
narrows them to float values, which is what the row sweep stores for SolveType = fpreal32.
"""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

import triplet_model as M

SEED = 20261018
Limits = namedtuple("Limits", "fast wave lds tile long_waves")
TOP_TILES = 256   # tiles one trip of the scan's single-block top pass takes (its block size)
CHUNKS_X, CHUNKS_Y = 50, 7   # the two columns planted in the long_chunks row (every other column of that row is >= 100)

# the cases by name (fixed here so that tests can be parametrised without the library; cases() checks the list): row lengths and row counts
# are named after the limit they sit at
LENGTHS = ("0", "1", "2", "fast-1", "fast", "fast+1", "wave-1", "wave", "wave+1", "2wave-1", "2wave", "2wave+1", "3wave+1", "1000")
ROW_COUNTS = ("1", "63", "64", "65", "255", "256", "257", "tile+1")
NO_F32 = ("many_long", "scan_top_pass_loops")     # the two large cases run in fp64 only
NAMES = tuple([f"len_{r}" for r in LENGTHS] + [f"dup_{p}" for p in ("asc", "desc", "one", "adjacent", "first_last")] +
              ["long_chunks", "wave_rows_lanes_0_30_31_63", "mix_all_paths", "long_lanes_0_63", "two_long_adjacent", "long_first", "many_long",
               "staged_exact", "staged_plus_1", "staged_long_few_columns", "unstaged_wave_rows_and_long"] + [f"rows_{n}" for n in ROW_COUNTS] +
              ["scan_top_pass_loops", "big_columns"])
RUNS = tuple((name, f32) for name in NAMES for f32 in (False, True) if not (f32 and name in NO_F32))   # what the GPU test runs


@functools.lru_cache(None)
def limits():
    """the limits of the built kernels; the call touches no device"""
    from adaptiveviscositysolver_amd import capi
    lib = capi.load_probe()
    info = capi.TripletMergeInfo()
    capi.check(lib.avs_merge_triplets_probe(0, None, None, None, 0, None, None, None, 0, None, C.byref(info), None))
    return Limits(info.fast_limit, info.wave_limit, info.merge_lds, info.scan_tile, info.long_grid_waves)


def row_class(R, L):
    return "reg" if R <= L.fast else ("wave" if R <= L.wave else "long")


class Case:
    def __init__(self, name, raw_ptr, raw_col, raw_val, rows=None, staged=None, seg_total=None, fold_rows=(), f32=True,
                 long_rows=0, more_rows_than=None, more_long_than=None):
        self.name = name
        self.raw_ptr = np.ascontiguousarray(raw_ptr, np.int32)
        self.raw_col = np.ascontiguousarray(raw_col, np.int32)
        self._val = np.ascontiguousarray(raw_val, np.float64)
        self.n = len(self.raw_ptr) - 1
        self.rows = dict(rows or {})            # row -> class it must fall in
        self.staged = dict(staged or {})        # 64-row wave -> its merged rows are staged in LDS
        self.seg_total = dict(seg_total or {})  # 64-row wave -> merged entries it must total
        self.fold_rows = tuple(fold_rows)       # rows whose values must tell a wrong fold from the right one
        self.f32 = f32                          # the case is run with f32 set as well
        self.long_rows = long_rows              # rows k_unique_rows must list
        self.more_rows_than, self.more_long_than = more_rows_than, more_long_than
        self._model = {}

    def arrays(self, f32=False):
        val = self._val.astype(np.float32).astype(np.float64) if f32 else self._val
        return self.raw_ptr, self.raw_col, val

    def row(self, r, f32=False):
        ptr, col, val = self.arrays(f32)
        return col[ptr[r]:ptr[r + 1]].tolist(), val[ptr[r]:ptr[r + 1]].tolist()

    def lengths(self):
        return np.diff(self.raw_ptr.astype(np.int64))

    def model(self, f32=False):
        """(row_ptr, col, val) of tests/triplet_model.py, computed once and not to be written to"""
        if f32 not in self._model:
            out = M.merge(*self.arrays(f32), f32=f32)
            for a in out:
                a.setflags(write=False)
            self._model[f32] = out
        return self._model[f32]


def _values(rng, k):
    return np.where(rng.random(k) < 0.5, -1.0, 1.0) * (1.0 + rng.random(k)) * 2.0 ** rng.integers(-20, 21, k)


def _distinct(rng, k, lo, hi):
    return (rng.choice(hi - lo, k, replace=False) + lo).tolist()


def _row(rng, R, U=None, pattern="mixed", lo=0, hi=4096, telling=True):
    """R raw entries over U distinct columns of [lo, hi): (columns, values) in emission order"""
    if R == 0:
        return [], []
    if pattern in ("asc", "desc"):
        cols = sorted(_distinct(rng, R, lo, hi), reverse=pattern == "desc")
    elif pattern == "one":
        cols = _distinct(rng, 1, lo, hi) * R
    elif pattern == "adjacent":     # runs of three equal columns (the last run takes the rest), the runs in no order
        runs = _distinct(rng, max(1, R // 3), lo, hi)
        cols = [c for c in runs for _ in range(3)][:R]
        cols += [runs[-1]] * (R - len(cols))
    elif pattern == "first_last":   # the last entry is the first occurrence of its column -- the smallest of the row
        cols, _ = _row(rng, R - 1, U, "mixed", lo + 1, hi)
        cols = cols + [min(cols) - 1 if cols else lo]
    else:
        U = max(1, R // 3) if U is None else U
        d = _distinct(rng, U, lo, hi)
        own = min(6, R - U)             # one column takes up to six of the duplicates: a fold long enough to depend on its order
        extra = [d[0]] * own + rng.choice(d, R - U - own).tolist()
        cols = d + extra
        cols = [cols[i] for i in rng.permutation(R)]
    return cols, _telling_values(rng, cols) if telling else _values(rng, R).tolist()


def _wrong_folds_show(cols, vals):
    """both planted fold errors (tests/triplet_model.py) change bits of this row, in fp64 and with float values"""
    for f32 in (False, True):
        v = np.asarray(vals, np.float32).astype(np.float64).tolist() if f32 else vals
        want = M.bits(M.merge_row(cols, v, f32)[1])
        for fold in (("right", "once") if f32 else ("right",)):
            if np.array_equal(M.bits(M.merge_row(cols, v, f32, fold)[1]), want):
                return False
    return True


def _telling_values(rng, cols):
    """values for a row; where a column occurs three times or more they are redrawn until a wrong fold order shows in the row's bits (some
    draws round the same way in either order) -- tests/test_triplet_edges.py checks the outcome for the rows a case names"""
    vals = _values(rng, len(cols)).tolist()
    if max(cols.count(c) for c in set(cols)) >= 3:
        for _ in range(200):
            if _wrong_folds_show(cols, vals):
                break
            vals = _values(rng, len(cols)).tolist()
    return vals


def _ordinary(rng, lo=0, hi=4096, U=None):
    """what the octree's interior rows look like to the merge: 15..17 raw entries, a few columns several times"""
    R = int(rng.integers(15, 18))
    return _row(rng, R, R - int(rng.integers(3, 8)) if U is None else U, "mixed", lo, hi, telling=False)


def _pack(rows):
    ptr = np.zeros(len(rows) + 1, np.int64)
    ptr[1:] = np.cumsum([len(c) for c, _ in rows])
    col = np.array([c for cs, _ in rows for c in cs], np.int64)
    val = np.array([v for _, vs in rows for v in vs], np.float64)
    assert ptr[-1] < 2 ** 31 and (len(col) == 0 or (col.min() >= 0 and col.max() <= 2 ** 31 - 3))
    return ptr, col, val


def _case(name, rng, n, special, **kw):
    """n rows: `special` (row -> (columns, values)) among ordinary ones"""
    rows = [special[r] if r in special else _ordinary(rng) for r in range(n)]
    return Case(name, *_pack(rows), **kw)


@functools.lru_cache(None)
def cases():
    L = limits()
    out = []
    count = [0]

    def rng():
        count[0] += 1
        return np.random.default_rng([SEED, count[0]])

    def classes(special):
        return {r: row_class(len(cv[0]), L) for r, cv in special.items()}

    def nlong(special):
        return sum(1 for cv in special.values() if len(cv[0]) > L.wave)

    def add(name, g, n, special, fold=None, **kw):
        kw.setdefault("rows", classes(special))
        out.append(_case(name, g, n, special, fold_rows=sorted(special) if fold is None else fold, long_rows=nlong(special), **kw))

    # --- row length: one row of every length around the limits, in a wave of ordinary rows
    for name, R in zip(LENGTHS, (0, 1, 2, L.fast - 1, L.fast, L.fast + 1, L.wave - 1, L.wave, L.wave + 1, 2 * L.wave - 1, 2 * L.wave,
                                 2 * L.wave + 1, 3 * L.wave + 1, 1000)):
        g = rng()
        add(f"len_{name}", g, 64, {17: _row(g, R)}, fold=[17] if R >= 6 else [])
    # --- duplicate patterns, one row per path: registers, whole wave, long
    R3 = {5: L.fast - 2, 20: (L.fast + L.wave) // 2 + 1, 40: 2 * L.wave + 22}
    for pattern in ("asc", "desc", "one", "adjacent", "first_last"):
        g = rng()
        add(f"dup_{pattern}", g, 64, {r: _row(g, R, None, pattern) for r, R in R3.items()}, fold=[] if pattern in ("asc", "desc") else None)
    # a long row over four 64-entry chunks: column X first in the first chunk with duplicates in the second and the third (and the last),
    # column Y first in the third chunk, below everything earlier, with a duplicate as the last entry
    g = rng()
    R = 3 * L.wave + 8
    cols, vals = _row(g, R, 60, "mixed", 100, 4096)
    X, Y = CHUNKS_X, CHUNKS_Y
    CHUNK_X, CHUNK_Y = (3, L.wave + 6, L.wave + 36, 2 * L.wave + 2, R - 10), (2 * L.wave + 12, R - 1)
    for p in CHUNK_X:
        cols[p] = X
    for p in CHUNK_Y:
        cols[p] = Y
    add("long_chunks", g, 64, {9: (cols, vals)})
    # --- wave composition
    g = rng()
    add("wave_rows_lanes_0_30_31_63", g, 64, {r: _row(g, L.fast + 3 + i * 7) for i, r in enumerate((0, 30, 31, 63))})
    g = rng()
    add("mix_all_paths", g, 64, {3: _row(g, L.wave - 9), 4: _row(g, L.wave + 30), 5: _row(g, L.fast)})
    g = rng()
    add("long_lanes_0_63", g, 64, {0: _row(g, L.wave + 5), 63: _row(g, 2 * L.wave + 9)})
    g = rng()
    add("two_long_adjacent", g, 64, {31: _row(g, 2 * L.wave + 3), 32: _row(g, L.wave + 2)})
    g = rng()
    add("long_first", g, 3 * 64, {0: _row(g, L.wave + 1), 1: _row(g, 2 * L.wave), 2: _row(g, L.wave + 40), 64: _row(g, L.wave + 7)})
    g = rng()   # more long rows than the long grids have waves: the grid-stride loops take a second trip
    nl = L.long_waves + 1
    add("many_long", g, nl, {r: _row(g, L.wave + 1, 20) for r in range(nl)}, fold=[0, L.long_waves], f32=False,
        rows={0: "long", L.long_waves: "long"}, more_long_than=L.long_waves)
    # --- staging: the wave's merged entries total exactly kMergeLds / one more
    for name, more in (("staged_exact", 0), ("staged_plus_1", 1)):
        g = rng()
        U = [L.lds // 64 + (1 if r < L.lds % 64 else 0) for r in range(64)]
        U[63] += more
        add(name, g, 64, {r: _row(g, U[r] + 6, U[r]) for r in range(64)}, fold=[0, 63], rows={},
            staged={0: more == 0}, seg_total={0: L.lds + more})
    g = rng()
    add("staged_long_few_columns", g, 64, {10: _row(g, 2 * L.wave + 22, 3)}, staged={0: True})
    g = rng()
    sp = {1: _row(g, L.wave, L.wave - 6), 2: _row(g, L.wave - 4, L.wave - 10), 3: _row(g, 5 * L.wave - 20, L.lds // 4 + 8)}
    sp.update({r: _ordinary(g, U=12) for r in range(64) if r not in sp})
    add("unstaged_wave_rows_and_long", g, 64, sp, fold=[1, 2, 3], rows=classes({r: sp[r] for r in (1, 2, 3)}), staged={0: False})
    # --- row count: the unique kernel's grid covers n + 1; the last row needs the whole wave
    for name, n in zip(ROW_COUNTS, (1, 63, 64, 65, 255, 256, 257, L.tile + 1)):
        g = rng()
        add(f"rows_{name}", g, n, {n - 1: _row(g, L.fast + 5)}, more_rows_than=L.tile if n > L.tile else None)
    # the row-pointer scan's top pass loops: more than 256 tiles of rows, 0..2 entries each
    g = rng()
    n = TOP_TILES * L.tile + 65
    R = g.integers(0, 3, n)
    ptr = np.concatenate([[0], np.cumsum(R)])
    col = g.integers(0, 3, int(ptr[-1])) + np.repeat(np.arange(n), R)    # (a row of two holds a duplicate pair now and then)
    out.append(Case("scan_top_pass_loops", ptr, col, _values(g, int(ptr[-1])), f32=False, more_rows_than=TOP_TILES * L.tile))
    # --- columns right below the pad (INT32_MAX) with bit 30 set: the sign bit is the long rows' duplicate mark
    g = rng()
    lo, hi = 2 ** 30, 2 ** 31 - 2
    sp = {7: _row(g, L.wave - 3, None, "mixed", lo, hi), 8: _row(g, 2 * L.wave + 17, None, "mixed", lo, hi), 9: _row(g, L.fast, None, "mixed", lo, hi)}
    for cols, _ in sp.values():
        order = np.argsort(cols, kind="stable")
        lo_c, hi_c = cols[order[0]], cols[order[-1]]
        for k in range(len(cols)):      # the row's smallest column becomes 2^30, its largest 2^31 - 3, duplicates included
            cols[k] = lo if cols[k] == lo_c else (hi - 1 if cols[k] == hi_c else cols[k])
    sp.update({r: _ordinary(g, lo, hi) for r in range(64) if r not in sp})
    add("big_columns", g, 64, sp, fold=[7, 8, 9], rows=classes({r: sp[r] for r in (7, 8, 9)}))
    assert tuple(c.name for c in out) == NAMES and all(c.f32 == (c.name not in NO_F32) for c in out)
    return tuple(out)


def by_name(name):
    return next(c for c in cases() if c.name == name)
