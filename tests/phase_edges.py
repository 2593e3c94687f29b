"""Named systems at the edges of the launch-per-phase PCG loop (pcg_solve_phases and enqueue_chunk, csrc/avs_pcg.hip), for seam A.

The loop's moving parts are on the host: chunks of kChunk = 32 iterations, every chunk but each 8th replayed from a captured hipGraph;
r.z in two slots chosen by an iteration's position in its chunk; the alpha step folded into k_update_r or launched on its own once the
SpMV leaves more than kFuseAlphaMax = 4096 partial sums; the beta step folded into k_update_xp or launched as OP_BETA; a coded or a
plain inverse diagonal; done == 2 ("converged, x += alpha p pending").  The cases sit on one edge each, with the smallest n that reaches
it, and say in `props` what the name claims (checked on the host by tests/test_phase_edges.py) and in `expect` what the loop's own report
(avs_phase_loop_info) must show on the device.

Every system is a symmetric tridiagonal one: off-diagonal entries -(0.75 + 0.25 u) from a palette of at most 1,023 values (csr_edges.
_palette), the diagonal 0.02 - (the sum of the row's off-diagonals), columns sorted, x0 uniform in +-[0.5, 1.5], b standard normal.  (The
dominant block-circulant systems of resident_edges.py reach the fp64 floor in about 45 iterations; this one is at 1e-2 after 32
iterations, below 1e-4 after 64 and at a few 1e-7 after 100: the iterates of the third and fourth chunk are still iterates.)  A periodic
assignment of the palette keeps the distinct values -- off-diagonals AND the diagonals they add up to -- under 2,048, the limit of the
coded diagonal; random draws, or a palette per tile, give the other value forms.  Seeded numpy only.
"""
from __future__ import annotations

import numpy as np

import csr_edges as E
from csr_edges import _palette
from resident_edges import RESIDENT_ENV

K_CHUNK, TIMED_EVERY = 32, 8                 # kChunk, kTimedChunkEvery
FUSE_ALPHA_MAX = 4096                        # kFuseAlphaMax
BLOCK, VEC_GRID, FOLD_BATCH = 256, 2048, 8   # kBlock, kVecGrid, kFoldBatch
TILE_ROWS = E.TILE_ROWS                      # rows per SpMV tile
CODED_MAX = E.LDS_TABLE                      # kViLdsTable: the largest dictionary with a coded diagonal
SHIFT = 0.02

KS = (0, 1, 2, 3, 4, 7, 8)                                  # max_iterations of the iterate checks, everywhere
KS_CHUNKS = (31, 32, 33, 64, 65, 90, 96, 97)                # + at n = 4,099: 64 captures the graph, 96 is the first pure replay, 90 and 97
                                                            #   end in a partial chunk
KS_NB = (33, 34)                                            # + on the three partial-sum cases
FEW_ROWS = (1, 2, 3, 255, 256, 257, 511, 512, 513)
FEW_ROWS_PASSES = 100                                       # iterations the model keeps of a few-row case (every k up to there is checked)
# converging iterations of the exit checks at n = 4,099: a few iterations in, the last two launches of the first chunk (an odd and an even
# position), the first two of the second -- inside a replayed graph --, and one inside the third
EXIT_ITERATIONS = ((4, 3), (31,), (32,), (33,), (34,), (70, 71, 69, 72, 68))
EXIT_MAX_ITERATIONS = 200                                   # a whole chunk of no-op launches follows every exit
N_SWITCH = 4099

# cleared before a case's own environment is set
PHASE_ENV = RESIDENT_ENV + ("AVS_PCG_GRAPH", "AVS_PCG_FUSE_BETA", "AVS_PCG_FUSE_VECTORS", "AVS_PCG_FUSED_TIMEOUT_MS", "AVS_F32_VECTORS",
                            "AVS_MIXED_PRECISION", "AVS_BRICK", "AVS_TRACE_PHASES", "AVS_PCG_FUSED_FAKE_FAULT", "AVS_CG_RESIDENT_FAKE_FAULT")
BASE_ENV = {"AVS_CG_RESIDENT": "0", "AVS_PCG_FUSE_VECTORS": "0"}     # every case: this loop, its two vector launches


class Case:
    def __init__(self, name, csr, env=None, props=None, ks=KS, few_rows=False, exits=False, seed=0):
        self.name = name
        self.row_ptr, self.col, self.val = csr
        self.n = len(self.row_ptr) - 1
        self.env = {**BASE_ENV, **(env or {})}
        self.props = dict(props or {})
        self.ks = tuple(ks)
        self.few_rows = few_rows            # iterates at every k up to convergence (at most FEW_ROWS_PASSES)
        self.exits = exits                  # the targeted exits of EXIT_ITERATIONS
        rng = np.random.default_rng(2000 + seed + self.n)
        self.b = rng.standard_normal(self.n)
        self.x0 = rng.uniform(0.5, 1.5, self.n) * rng.choice([-1.0, 1.0], self.n)

    def __repr__(self):
        return f"Case({self.name}, n={self.n}, nnz={int(self.row_ptr[-1])}, env={self.env})"

    @property
    def graph(self):
        return self.env.get("AVS_PCG_GRAPH", "1") != "0"

    @property
    def fuse_beta(self):
        return self.env.get("AVS_PCG_FUSE_BETA", "1") != "0"

    def format(self):
        return E.expected_format(self.row_ptr, self.col, self.val, self.env)

    def expect(self):
        """what avs_phase_loop_info must report of a solve of this case"""
        fmt = self.format()
        codes = fmt["value_table_size"] > 0
        tiles = -(-self.n // TILE_ROWS)
        nb = tiles * (TILE_ROWS // 64) if codes else tiles
        return {"nb": nb, "g": vec_grid(self.n), "coded": int(codes and not fmt["tile_local_tables"] and fmt["value_table_size"] <= CODED_MAX),
                "fuse_beta": int(self.fuse_beta), "alpha_folded": self.fuse_beta and nb <= FUSE_ALPHA_MAX, "float_vectors": 0}


def vec_grid(n):
    return min(max(-(-n // BLOCK), 1), VEC_GRID)


def replayed_chunks(enqueued, graph=True):
    """chunks replayed from the graph when `enqueued` iterations were enqueued: the full chunks but every TIMED_EVERY-th"""
    return sum(1 for j in range(enqueued // K_CHUNK) if j % TIMED_EVERY != 0) if graph else 0


def launched_chunks(enqueued, graph=True):
    return -(-enqueued // K_CHUNK) - replayed_chunks(enqueued, graph)


# ---------------------------------------------------------------------------------------------------------------------------------------
# builder
# ---------------------------------------------------------------------------------------------------------------------------------------
def tridiagonal(n, seed, palette=64, assign="periodic"):
    """assign: "periodic" -- entry i of the off-diagonal takes palette[i % palette] (a seeded order): palette off-diagonal and about as
    many diagonal values; "random" -- seeded draws: about n diagonal values; "tiles" -- periodic inside every SpMV tile of 512 rows, a
    palette of its own per tile (disjoint value ranges)"""
    rng = np.random.default_rng(seed)
    i = np.arange(max(n - 1, 0), dtype=np.int64)
    if assign == "periodic":
        off = rng.permutation(_palette(palette, rng, 0.75, 1.0))[i % palette]
    elif assign == "random":
        off = _palette(palette, rng, 0.75, 1.0)[rng.integers(0, palette, len(i))]
    elif assign == "tiles":
        tiles = -(-n // TILE_ROWS)
        pals = np.stack([rng.permutation(_palette(palette, rng, 0.75 + 0.25 * t / tiles, 0.75 + 0.25 * (t + 1) / tiles)) for t in range(tiles)])
        off = pals[i // TILE_ROWS, i % palette]
    else:
        raise ValueError(assign)
    left = np.concatenate([[0.0], off])          # row i: -off[i - 1] at column i - 1, -off[i] at column i + 1
    right = np.concatenate([off, [0.0]])
    diag = (SHIFT + left) + right
    rows = np.concatenate([i + 1, np.arange(n), i])
    cols = np.concatenate([i, np.arange(n), i + 1])
    vals = np.concatenate([-off, diag, -off])
    order = np.lexsort((cols, rows))
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return rp.astype(np.int32), cols[order].astype(np.int32), vals[order]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases: name -> builder
# ---------------------------------------------------------------------------------------------------------------------------------------
_BUILDERS = {}


def _register(name, fn):
    _BUILDERS[name] = fn


# ---- few rows: n = 1 has no row pair, an odd n takes the lone last row, vec_grid goes from 1 to 2 workgroups at 257, the SpMV from 1 to 2
# tiles at 513 ----
for _n in FEW_ROWS:
    _register(f"rows_{_n}", lambda n=_n: Case(f"rows_{n}", tridiagonal(n, 100 + n), few_rows=True,
                                              props={"n": n, "g": 1 if n <= 256 else (2 if n <= 512 else 3), "tiles": 1 if n <= 512 else 2}))

# ---- SpMV partial sums nb of the coded form (8 per tile of 512 rows) ----
# 264 > 256: the second slot of vec_fold's batch; 2,056 > kFoldBatch * kBlock: its tail loop; 4,104 > kFuseAlphaMax: the alpha step is a
# launch of its own (OP_ALPHA, OP_ALPHA_ODD on the odd positions) and the unfused k_update_r is followed by the fused k_update_xp
for _n, _nb in ((16385, 264), (131073, 2056), (262145, 4104)):
    _register(f"nb_{_nb}", lambda n=_n, nb=_nb: Case(f"nb_{nb}", tridiagonal(n, 200 + nb), ks=KS + KS_NB,
                                                     props={"n": n, "nb": nb, "alpha_folded": nb <= FUSE_ALPHA_MAX}))

# ---- diagonal and value forms at n = 4,099 ----
_register("form_coded", lambda: Case("form_coded", tridiagonal(N_SWITCH, 300), ks=KS + KS_CHUNKS, exits=True,
                                     props={"n": N_SWITCH, "form": "one dictionary, coded diagonal"}))
# the plain CSR: an 8-B inverse per row, one partial sum per 512 rows
_register("form_plain", lambda: Case("form_plain", tridiagonal(N_SWITCH, 300), env={"AVS_VALUE_INDEX": "0"}, ks=KS + KS_CHUNKS, exits=True,
                                     props={"n": N_SWITCH, "form": "plain", "same_matrix_as": "form_coded"}))
# one dictionary of more than kViLdsTable values: codes without a coded diagonal
_register("form_dictionary", lambda: Case("form_dictionary", tridiagonal(N_SWITCH, 301, palette=1023, assign="random"), ks=KS + KS_CHUNKS,
                                          exits=True, props={"n": N_SWITCH, "form": "one dictionary, plain diagonal"}))
# tile-local tables, more than 65,536 distinct values in all: 184 tiles of about 362 values (a tile's table may hold a quarter of its 1,536
# non-zeros) + the lone last row; k_inv_diag reads the diagonal through tab_ptr
N_TILE_TABLES = 184 * TILE_ROWS + 1
_register("form_tile_tables", lambda: Case("form_tile_tables", tridiagonal(N_TILE_TABLES, 302, palette=180, assign="tiles"),
                                           props={"n": N_TILE_TABLES, "form": "tile-local tables", "distinct_over": E.DICT_MAX}))

# ---- loop switches at n = 4,099, coded: the beta step folded or launched x chunks replayed or enqueued launch by launch ----
for _fb in (0, 1):
    for _gr in (0, 1):
        _register(f"beta{_fb}_graph{_gr}", lambda fb=_fb, gr=_gr: Case(
            f"beta{fb}_graph{gr}", tridiagonal(N_SWITCH, 300), env={"AVS_PCG_FUSE_BETA": str(fb), "AVS_PCG_GRAPH": str(gr)},
            ks=KS + KS_CHUNKS, exits=True, props={"n": N_SWITCH, "form": "one dictionary, coded diagonal", "same_matrix_as": "form_coded"}))

NAMES = list(_BUILDERS)


def get(name):
    return _BUILDERS[name]()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the host model of a case (tests/phase_model.py), shared by the tests of one process
# ---------------------------------------------------------------------------------------------------------------------------------------
_models = {}


def model_of(case):
    """phase_model.Model of the case's system (the last few are kept: cases that share a matrix share the runs)"""
    import phase_model as P
    passes = FEW_ROWS_PASSES if case.few_rows else max(max(case.ks), max(max(e) for e in EXIT_ITERATIONS) + 1 if case.exits else 0)
    key = (case.n, int(case.row_ptr[-1]), case.val[:64].tobytes(), case.val[-64:].tobytes(), passes)
    if key not in _models:
        while len(_models) >= 2:
            _models.pop(next(iter(_models)))
        _models[key] = P.Model(P.Matrix(case.row_ptr, case.col, case.val), case.b, case.x0, passes)
    return _models[key]


def checked_ks(case, model):
    """max_iterations at which the iterates are compared: the case's ks, or every k up to convergence for the few-row cases"""
    if case.few_rows:
        return tuple(range(model.live_passes() + 1))
    return tuple(k for k in case.ks if k <= model.passes)


def exit_targets(case, model):
    """[(tol, iterations, iteration)], one per entry of EXIT_ITERATIONS: the first admissible of its candidates (None: none is)"""
    if not case.exits:
        return []
    return [next(iter(model.exit_tolerances(cands)), None) for cands in EXIT_ITERATIONS]
