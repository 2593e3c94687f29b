"""Named small systems at the edges of the CU-resident PCG plan (resident_prepare, csrc/avs_pcg_resident.inl, driving the host planner
csrc/avs_resident_plan.cpp), for seam A.

The plan gives every lane of a 1024-lane workgroup up to 6 consecutive rows in 15 register quads of 5 words (a row takes whole quads; a
row of more than W = 75 words sits alone and leaves its tail in memory), streams the rows that do not fit once the lanes exceed 93 % of
1024 x G, keeps 4 - NG vectors of a workgroup's rows + its remote columns in ~154 KB of LDS (tiers NG = 0 .. 3), fills the remote
columns 4 x 1024 per trip from a source list of 16,384 (32,768 with streams), re-encodes the columns in bitmap passes of a multiple of
512 columns, and -- with AVS_RESIDENT_LOCAL_TABLES -- gives a workgroup (<= 4,096 values) or each of its waves (<= 2,048) a value table.
The octree scenes reach whichever of these edges the octree happens to have; the cases here sit on one edge each, with the smallest
matrix that still reaches it, and say in `expect` what the reported plan (avs_pcg_csr_plan) must show for that.

Every case is symmetric and strictly diagonally dominant: off-diagonal entries -palette in (-1, -0.25], the diagonal = the number of
entries of its row, columns sorted, every row with its diagonal.  Unless `many_values`, a case holds at most 1,023 distinct values and
the default plan takes it (packed single dictionary).  `props` carries the facts a name claims; tests/test_resident_edges.py checks
them on the host.  Seeded numpy only.

Two builders: block-circulant (a block of m rows with columns i +- 1 .. h, + the antipode i + m / 2 for even lengths: every row of
exactly L entries; an optional symmetric permutation scatters rows and columns) and random-symmetric with "arrow" rows of an exact length.
"""
from __future__ import annotations

import numpy as np

from csr_edges import _palette

QUAD_WORDS, QUADS, ROWS_MAX, W = 5, 15, 6, 75
LANES, FILL, SRC_LIST, SRC_LIST_STREAM = 1024, 4 * 1024, 16384, 32768
KS = (0, 1, 2, 3, 4, 7, 8)          # max_iterations of the iterate checks
PASSES = 14                         # passes the model keeps (the loose-tolerance exits are chosen among them)
FEW_ROWS = (1, 2, 3, 5, 63, 64, 65, 1023, 1024, 1025)
PACK_LENGTHS = (1, 4, 5, 6, 10, 11, 24, 25, 26, 50, 51, 74, 75)
RESIDENT_ENV = ("AVS_CG_RESIDENT", "AVS_CG_RESIDENT_CUS", "AVS_CG_RESIDENT_MAX_QUADS", "AVS_CG_RESIDENT_COHERENT_FILL",
                "AVS_CG_RESIDENT_REMAP_CHUNK", "AVS_CG_RESIDENT_NO_STREAM", "AVS_CG_RESIDENT_MAX_GLOBAL", "AVS_RESIDENT_LOCAL_TABLES",
                "AVS_RESIDENT_F32", "AVS_CG_RESIDENT_EQUAL_LANES", "AVS_CG_RESIDENT_LANE_FILL", "AVS_CG_RESIDENT_REMOTE_COST",
                "AVS_CG_RESIDENT_STREAM_COST", "AVS_CG_RESIDENT_TIMERS", "AVS_CG_RESIDENT_VERBOSE", "AVS_VALUE_INDEX", "AVS_VALUE_PACK",
                "AVS_COLUMN_WINDOWS", "AVS_TILE_TABLES")   # cleared before a case's own environment is set


class Case:
    def __init__(self, name, csr, env=None, props=None, expect=None, few_rows=False, seed=0):
        self.name = name
        self.row_ptr, self.col, self.val = csr
        self.n = len(self.row_ptr) - 1
        self.env = dict(env or {})
        self.props = dict(props or {})
        self.expect = dict(expect or {})     # what the reported plan must show
        self.few_rows = few_rows             # iterates at every k up to convergence
        rng = np.random.default_rng(1000 + seed + self.n)
        self.b = rng.standard_normal(self.n)
        self.x0 = rng.uniform(0.5, 1.5, self.n) * rng.choice([-1.0, 1.0], self.n)

    def __repr__(self):
        return f"Case({self.name}, n={self.n}, nnz={int(self.row_ptr[-1])}, env={self.env})"


# ---------------------------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------------------------
def _sym_csr(n, a, b, w):
    """CSR of the symmetric matrix with off-diagonal entries w at (a, b) and (b, a) -- each unordered pair given once --, the diagonal
    = the row's number of entries L (its L - 1 off-diagonals are each < 1 in magnitude: strictly dominant), columns sorted"""
    a, b, w = np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(w, np.float64)
    assert np.all(a != b) and len(np.unique(np.minimum(a, b) * n + np.maximum(a, b))) == len(a)
    m = np.bincount(np.concatenate([a, b]), minlength=n)
    rows = np.concatenate([a, b, np.arange(n)])
    cols = np.concatenate([b, a, np.arange(n)])
    vals = np.concatenate([w, w, 1.0 + m])
    order = np.lexsort((cols, rows))
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return rp.astype(np.int32), cols[order].astype(np.int32), vals[order]


def _pair_values(a, b, pal):
    """-palette entry of the unordered pair (a, b): a hash of the pair, so that both triangles agree"""
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return -pal[((lo * 1000003 + hi) % 2147483647) * 48271 % 2147483647 % len(pal)]


def _circulant_pairs(r0, m, L):
    """the unordered pairs of a block of m rows at r0 whose rows have exactly L entries each"""
    h, anti = (L - 1) // 2, (L - 1) % 2
    assert L == 1 or (m > 2 * h + anti and (not anti or (m % 2 == 0 and m // 2 > h))), (m, L)
    i = np.arange(m, dtype=np.int64)
    a = [np.tile(i, h)] if h else []
    b = [((i[None, :] + np.arange(1, h + 1)[:, None]) % m).ravel()] if h else []
    if anti:
        a.append(i[:m // 2])
        b.append(i[:m // 2] + m // 2)
    if not a:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return r0 + np.concatenate(a), r0 + np.concatenate(b)


def block_circulant(blocks, seed, permute=False, palette=12, value_of=None):
    """blocks: [(rows, L)] -- consecutive blocks, every row of a block with exactly L entries.  permute: a seeded symmetric permutation
    of rows and columns.  value_of(a, b, pal): the pair's (negative) value (default: a hash of the pair)."""
    rng = np.random.default_rng(seed)
    pal = _palette(palette, rng)
    a, b, r0 = [], [], 0
    for m, L in blocks:
        pa, pb = _circulant_pairs(r0, m, L)
        a.append(pa)
        b.append(pb)
        r0 += m
    n = r0
    a, b = np.concatenate(a), np.concatenate(b)
    w = (value_of or _pair_values)(a, b, pal)
    if permute:     # (after the values: the permuted matrix is P A P^T of the plain one)
        perm = rng.permutation(n)
        a, b = perm[a], perm[b]
    return _sym_csr(n, a, b, w)


def random_symmetric(n, degree, arrows, seed, palette=12):
    """about `degree` random symmetric off-diagonal entries per ordinary row; arrows: {row: L or (L, [columns that must be among them])}
    -- rows of exactly L entries whose columns are ordinary rows"""
    rng = np.random.default_rng(seed)
    pal = _palette(palette, rng)
    ordinary = np.setdiff1d(np.arange(n), np.array(sorted(arrows), dtype=np.int64))
    a = ordinary[rng.integers(0, len(ordinary), n * degree // 2)]
    b = ordinary[rng.integers(0, len(ordinary), n * degree // 2)]
    keep = a != b
    lo, hi = np.minimum(a[keep], b[keep]), np.maximum(a[keep], b[keep])
    key = np.unique(lo * n + hi)
    a, b = [key // n], [key % n]
    for r, spec in sorted(arrows.items()):
        L, must = spec if isinstance(spec, tuple) else (spec, [])
        rest = np.setdiff1d(ordinary, np.array(must, dtype=np.int64))
        cols = np.concatenate([np.array(must, dtype=np.int64), rng.choice(rest, L - 1 - len(must), replace=False)])
        a.append(np.full(L - 1, r, dtype=np.int64))
        b.append(cols)
    a, b = np.concatenate(a), np.concatenate(b)
    return _sym_csr(n, a, b, _pair_values(a, b, pal))


def row_lengths(case_or_rp):
    rp = case_or_rp.row_ptr if hasattr(case_or_rp, "row_ptr") else case_or_rp
    return np.diff(np.asarray(rp, dtype=np.int64))


def lanes_in_registers(lens, max_quads=QUADS):
    """(lanes, long-row lanes, longest tail) of a plan without streamed rows: form_lanes(T = 0) of csrc/avs_resident_plan.cpp restated
    (tests/test_resident_plan_host.py compares the two without a GPU)"""
    w = max_quads * QUAD_WORDS
    lanes = long_lanes = tail = 0
    i, n = 0, len(lens)
    while i < n:
        if lens[i] > w:
            long_lanes += 1
            tail = max(tail, int(lens[i]) - w)
            lanes += 1
            i += 1
            continue
        rows = used = 0
        while i < n and rows < ROWS_MAX and lens[i] <= w:
            k = -(-int(lens[i]) // QUAD_WORDS)
            if used + k > max_quads:
                break
            used += k
            rows += 1
            i += 1
        lanes += 1
    return lanes, long_lanes, tail


def parts_read(case, g):
    """g x g bool: an equal split of the rows in g parts -- part p reads a column of part q"""
    n = case.n
    part = lambda i: np.minimum(i * g // n, g - 1)
    rows = np.repeat(np.arange(n, dtype=np.int64), row_lengths(case))
    m = np.zeros((g, g), dtype=bool)
    m[part(rows), part(case.col.astype(np.int64))] = True
    return m


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases: name -> builder
# ---------------------------------------------------------------------------------------------------------------------------------------
_BUILDERS = {}


def _case(fn):
    _BUILDERS[fn.__name__.lstrip("_")] = fn
    return fn


def _register(name, fn):
    _BUILDERS[name] = fn


# ---- quad and lane packing (whole chip) ----
def _pack_cycle_csr(permute):
    return block_circulant([(80, L) for _ in range(2) for L in PACK_LENGTHS], seed=11, permute=permute)


_register("pack_cycle", lambda: Case("pack_cycle", _pack_cycle_csr(False), props={"row_lengths": list(PACK_LENGTHS)},
                                     expect={"long_row_lanes": 0}))
_register("pack_cycle_permuted", lambda: Case("pack_cycle_permuted", _pack_cycle_csr(True),
                                              props={"row_lengths": list(PACK_LENGTHS), "permutation_of": "pack_cycle"},
                                              expect={"long_row_lanes": 0}))
# only <= 5-word rows: 6 rows fit a lane, kResRowsMax binds before the quads do (3000 rows -> 500 lanes of 6 quads)
_register("pack_rows6", lambda: Case("pack_rows6", block_circulant([(1000, 1), (1000, 4), (1000, 5)], seed=12),
                                     props={"row_lengths": [1, 4, 5]}, expect={"lanes": 500}))
# only 25-word rows: 3 rows fill the 15 quads exactly
_register("pack_25", lambda: Case("pack_25", block_circulant([(3000, 25)], seed=13), props={"row_lengths": [25]}, expect={"lanes": 1000}))
# 26-word rows (6 quads): the third row does not fit
_register("pack_26", lambda: Case("pack_26", block_circulant([(3000, 26)], seed=14), props={"row_lengths": [26]}, expect={"lanes": 1500}))

# ---- long rows at the real 15 quads: arrow rows of 76, 77, 80, 150, 1000 entries (tails 1, 2, 5, 75, 925), first, last, mid-matrix ----
ARROWS = {0: 76, 2999: 77, 700: 80, 1500: 150, 2200: 1000}


def _long_csr():
    return random_symmetric(3000, 4, ARROWS, seed=21)


_register("long_arrows", lambda: Case("long_arrows", _long_csr(), props={"arrows": ARROWS},
                                      expect={"long_row_lanes": 5, "longest_tail": 925, "max_quads": 15}))
# the same matrix with one quad per lane: every row of more than 5 words takes the tail path
_register("long_arrows_1quad", lambda: Case("long_arrows_1quad", _long_csr(), env={"AVS_CG_RESIDENT_MAX_QUADS": "1"}, props={"arrows": ARROWS},
                                            expect={"long_row_lanes": "rows_over_5", "longest_tail": 995, "max_quads": 1}))


# ---- few rows: on the whole chip (most workgroups own nothing) and on one CU ----
def _few_csr(n):
    if n <= 5:      # a full matrix
        return block_circulant([(n, n)], seed=30 + n)
    return block_circulant([(n, 5)], seed=30 + n, permute=True)


for _n in FEW_ROWS:
    for _tag, _env in (("", {}), ("_1cu", {"AVS_CG_RESIDENT_CUS": "1"})):
        _register(f"rows_{_n}{_tag}", lambda n=_n, env=_env, tag=_tag: Case(f"rows_{n}{tag}", _few_csr(n), env=env, props={"n": n},
                                                                         expect={"workgroups": 1} if env else {}, few_rows=True))

# ---- remote columns ----
# random columns on 8 CUs: every workgroup depends on every other one
_register("remote_random", lambda: Case("remote_random", block_circulant([(20000, 5)], seed=41, permute=True), env={"AVS_CG_RESIDENT_CUS": "8"},
                                        props={"row_lengths": [5], "all_parts_read_all": 8}, expect={"workgroups": 8, "fill_trips": 2}))
# two workgroups that read 4 (even) and 1 (odd) remote columns each: a band that wraps / a chain that does not
_register("remote_even", lambda: Case("remote_even", block_circulant([(4000, 5)], seed=42), env={"AVS_CG_RESIDENT_CUS": "2"},
                                      props={"row_lengths": [5]}, expect={"workgroups": 2, "max_remote": 4}))


def _chain_csr(n):
    i = np.arange(n - 1, dtype=np.int64)
    return _sym_csr(n, i, i + 1, _pair_values(i, i + 1, _palette(12, np.random.default_rng(43))))


_register("remote_odd", lambda: Case("remote_odd", _chain_csr(4000), env={"AVS_CG_RESIDENT_CUS": "2"}, props={"row_lengths": [2, 3]},
                                     expect={"workgroups": 2, "max_remote": 1}))
# caches that take 2 and 3 trips of the fill (4 x 1024 slots each): 4 CUs, random columns -- 2,250 rows read ~5.0 k of the other 6,750
# columns, 4,500 rows ~9.9 k of 13,500; each also with plain loads behind an L2 invalidate
for _tag, _env in (("", {}), ("_plain_fill", {"AVS_CG_RESIDENT_COHERENT_FILL": "0"})):
    _register(f"fill_2trips{_tag}", lambda env=_env, tag=_tag: Case(f"fill_2trips{tag}", block_circulant([(9000, 5)], seed=44, permute=True),
                                                                  env={"AVS_CG_RESIDENT_CUS": "4", **env}, props={"row_lengths": [5]},
                                                                  expect={"workgroups": 4, "fill_trips": 2}))
    _register(f"fill_3trips{_tag}", lambda env=_env, tag=_tag: Case(f"fill_3trips{tag}", block_circulant([(18000, 5)], seed=45, permute=True),
                                                                  env={"AVS_CG_RESIDENT_CUS": "4", **env}, props={"row_lengths": [5]},
                                                                  expect={"workgroups": 4, "fill_trips": 3}))
# ten bitmap passes of 512 columns; row 3000 (second workgroup of two) reads the columns on both sides of the first two pass boundaries
REMAP_COLUMNS = [511, 512, 1023, 1024]
_register("remap_10passes", lambda: Case("remap_10passes", random_symmetric(5000, 4, {3000: (9, REMAP_COLUMNS)}, seed=46),
                                         env={"AVS_CG_RESIDENT_CUS": "2", "AVS_CG_RESIDENT_REMAP_CHUNK": "512"},
                                         props={"arrows": {3000: 9}, "entries": [(3000, c) for c in REMAP_COLUMNS]},
                                         expect={"workgroups": 2, "remap_passes": 10}))

# ---- tiers and streams: one case per fp64 instantiation k_cg_resident<NG, STREAM, double> ----
# Footprint of a workgroup: (4 - NG) rows + remote columns, in doubles, against 19.8 k (and the sum over the workgroups against 88 % of
# it).  Without streams a workgroup has at most 0.93 x 1024 lanes x 6 rows = 5.7 k rows, so tiers 2 and 3 need remote columns: random
# columns on 4 CUs (4 k rows + ~8.8 k remote; 5 k rows + ~11 k remote).  With streams the rows alone do it, on a band.
# The streamed rows: 1-quad rows (ng2), 3-quad rows (ng1), 5-quad rows (ng0), and ng3 cycles 1-, 3-, 4-, 5- and 6-quad blocks (the
# last-quad bit, the padding to the wave's longest lane) around an arrow row of 1,000 entries, whose lane streams nothing.  (A lane's
# stream takes any row of which it is owed half the quads -- with ~37 streamed quads per lane here that swallowed an arrow row of 80
# entries, 16 quads, as a streamed row; 200 quads are never owed.)
def _tier(name, csr, cus, ng, stream, props, extra_env=None, extra_expect=None):
    return Case(name, csr, env={"AVS_CG_RESIDENT_CUS": str(cus), **(extra_env or {})}, props=props,
                expect={"workgroups": cus, "ng": ng, "stream": stream, "local_tables": 0, **(extra_expect or {})})


_register("tier_ng0", lambda: _tier("tier_ng0", block_circulant([(8000, 5)], seed=50), 2, 0, False, {"row_lengths": [5]}))
_register("tier_ng1", lambda: _tier("tier_ng1", block_circulant([(11000, 5)], seed=51), 2, 1, False, {"row_lengths": [5]}))
_register("tier_ng2", lambda: _tier("tier_ng2", block_circulant([(16000, 5)], seed=52, permute=True), 4, 2, False, {"row_lengths": [5]}))
_register("tier_ng3", lambda: _tier("tier_ng3", block_circulant([(20000, 5)], seed=53, permute=True), 4, 3, False, {"row_lengths": [5]}))
_register("tier_ng0_stream", lambda: _tier("tier_ng0_stream", block_circulant([(8000, 25)], seed=54), 2, 0, True, {"row_lengths": [25]}))
_register("tier_ng1_stream", lambda: _tier("tier_ng1_stream", block_circulant([(11000, 11)], seed=55), 2, 1, True, {"row_lengths": [11]}))
_register("tier_ng2_stream", lambda: _tier("tier_ng2_stream", block_circulant([(16000, 5)], seed=56), 2, 2, True, {"row_lengths": [5]}))
NG3_LENGTHS = (5, 15, 20, 25, 30)


def _ng3_stream_csr():
    """24,000 rows: blocks of 400 rows cycling 1-, 3-, 4-, 5- and 6-quad rows; row 12,345 rewired into an arrow row of 1,000 entries"""
    rp, col, val = block_circulant([(400, L) for _ in range(12) for L in NG3_LENGTHS], seed=57)
    n = len(rp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    r = 12345
    off = (rows != col) & (rows != r) & (col != r)            # drop the row's own pairs, then give it 999 others all over the matrix
    a, b, w = rows[off & (rows < col)], col[off & (rows < col)].astype(np.int64), val[off & (rows < col)]
    far = np.arange(999, dtype=np.int64) * 24 + 17
    pal = _palette(12, np.random.default_rng(57))
    return _sym_csr(n, np.concatenate([a, np.full(999, r)]), np.concatenate([b, far]), np.concatenate([w, _pair_values(np.full(999, r), far, pal)]))


_register("tier_ng3_stream", lambda: _tier("tier_ng3_stream", _ng3_stream_csr(), 2, 3, True, {"arrows": {12345: 1000}},
                                           extra_expect={"long_row_lanes": 1, "longest_tail": 925}))

# ---- local value tables (AVS_RESIDENT_LOCAL_TABLES=1, more than 2,048 distinct values) ----
LT = {"AVS_RESIDENT_LOCAL_TABLES": "1"}


def _local_values(a, b, pal):
    """values that follow the rows: a wave's few hundred rows see few of them, a workgroup's thousands of rows more than 2,048; the
    antipode pairs draw from the upper half of the palette"""
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    half = len(pal) // 2
    return -pal[np.where(hi - lo > 64, half + (lo // 3) % half, (lo // 3) % half)]


def _lt(name, csr, cus, stream, gpw, props):
    return Case(name, csr, env={"AVS_CG_RESIDENT_CUS": str(cus), **LT}, props={"many_values": True, **props},
                expect={"workgroups": cus, "stream": stream, "local_tables": 1, "tables_per_workgroup": gpw})


# a table per workgroup: 3,000 values, 3 k rows + a few remote columns (12 column bits) next to 12 code bits
_register("lt_workgroup", lambda: _lt("lt_workgroup", block_circulant([(6000, 5)], seed=60, palette=3000), 2, False, 1, {"row_lengths": [5]}))
_register("lt_workgroup_stream", lambda: _lt("lt_workgroup_stream", block_circulant([(6000, 25)], seed=61, palette=3000), 2, True, 1,
                                             {"row_lengths": [25]}))
# a table per wave: every row reads its antipode, so a workgroup of 4.5 k rows has 4.5 k remote columns (14 column bits) and ~3,000
# values (12 code bits): 26 bits
_register("lt_wave", lambda: _lt("lt_wave", block_circulant([(9000, 4)], seed=62, palette=9000, value_of=_local_values), 2, False, 16,
                                 {"row_lengths": [4]}))
_register("lt_wave_stream", lambda: _lt("lt_wave_stream", block_circulant([(9000, 26)], seed=63, palette=9000, value_of=_local_values), 2, True, 16,
                                        {"row_lengths": [26]}))


# ---- declines: the call still solves (resident == 0) and says why ----
def _decline(name, csr, env, why, props):
    return Case(name, csr, env=env, props=props, expect={"declined": why})


# 8 CUs, 5.5 k rows of 10 random columns each: ~28 k remote columns per workgroup, a source list holds 16,384
_register("decline_source_list", lambda: _decline("decline_source_list", block_circulant([(44000, 10)], seed=70, permute=True),
                                                  {"AVS_CG_RESIDENT_CUS": "8"}, "more remote columns than its source list holds", {"row_lengths": [10]}))


def _distinct_values(a, b, pal):
    return -pal[np.arange(len(a)) % len(pal)]


# 75-word rows, a value per pair: a wave's 64 rows hold ~3,000 distinct values
_register("decline_wave_values", lambda: _decline("decline_wave_values",
                                                  block_circulant([(3000, 75)], seed=71, palette=111000, value_of=_distinct_values),
                                                  {"AVS_CG_RESIDENT_CUS": "4", **LT}, "has more than 2048 distinct values",
                                                  {"row_lengths": [75], "many_values": True}))
_register("decline_no_stream", lambda: _decline("decline_no_stream", block_circulant([(8000, 25)], seed=54),
                                                {"AVS_CG_RESIDENT_CUS": "2", "AVS_CG_RESIDENT_NO_STREAM": "1"},
                                                "too many rows for the register files", {"row_lengths": [25], "same_matrix_as": "tier_ng0_stream"}))
_register("decline_max_global", lambda: _decline("decline_max_global", block_circulant([(20000, 5)], seed=53, permute=True),
                                                 {"AVS_CG_RESIDENT_CUS": "4", "AVS_CG_RESIDENT_MAX_GLOBAL": "0"},
                                                 "do not fit the LDS", {"row_lengths": [5], "same_matrix_as": "tier_ng3"}))

NAMES = list(_BUILDERS)


def get(name):
    return _BUILDERS[name]()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the host model of a case (tests/resident_model.py), shared by the tests of one process
# ---------------------------------------------------------------------------------------------------------------------------------------
FEW_ROWS_PASSES = 30
_models = {}


def model_of(case):
    """resident_model.Model of the case's system (the last few are kept: cases that share a matrix share the runs)"""
    import resident_model as M
    key = (case.n, int(case.row_ptr[-1]), case.val[:64].tobytes(), case.col[-64:].tobytes())
    if key not in _models:
        while len(_models) >= 2:
            _models.pop(next(iter(_models)))
        A = M.Matrix(case.row_ptr, case.col, case.val)
        _models[key] = M.Model(A, case.b, case.x0, FEW_ROWS_PASSES if case.few_rows else PASSES)
    return _models[key]


def checked_ks(case, model):
    """max_iterations at which the iterates are compared: KS, or every k up to convergence for the few-row cases"""
    if case.few_rows:
        return tuple(range(model.live_passes() + 1))
    return tuple(k for k in KS if k <= model.passes)
