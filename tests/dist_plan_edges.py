"""Named edge cases of the device partition planners (csrc/avs_dist_plan.hip: plan_from_source and dist_tail_from_rows, through
avs_dist_plan_probe), placed from the limits the code was compiled with (the probe's limits-only call) and a fixed seed.

A case is a CSR matrix over n ids plus what the planner needs -- PLAN: one dof record per id, an optional perm, levels, extent, world;
TAIL: an owner byte per id, split, an optional dom list -- and a predicate that proves FROM THE MODEL ALONE (tests/dist_plan_model.py) that
the case reaches the edge it is named after.  tests/test_dist_plan_model.py checks the predicates and the model on the CPU,
tests/test_gpu_dist_plan_edges.py runs every case and every rank of its world on the device.  No case has more than 6,000 rows.

The dofs lie on a line along the cut axis: id i has level 0 (unless the case says otherwise) and the coordinate xs[i] on the cut axis, so
its plane is min(xs[i], extent - 1) >> (levels - 1).
"""
import functools
from collections import namedtuple

import numpy as np

import dist_plan_model as M

SEED = 20261019
MAX_ROWS = 6000
Limits = namedtuple("Limits", "lds_planes scan_tile T group max_world")
REFUSED = "refused: a column outside the window"   # what Case.plans() holds for a rank the tail core must refuse (AVS_EINTERNAL)
ROW_LENGTHS = (0, 1, 15, 16, 17, 33, 300)     # around the row groups of 16 lanes (and two and many trips of a group)

PLAN_NAMES = ("world_1", "world_above_planes", "trailing_empty_plane", "trailing_empty_plane_interior_rank", "empty_planes_lead_and_middle",
              "extent_not_multiple_of_granule", "faces_at_extent", "several_levels", "planes_lds_limit", "planes_lds_limit_plus_1",
              "planes_4096", "world_32_ends_exchange", "non_neighbour_peers", "send_only_and_receive_only_peers", "row_lengths",
              "n_scan_tile_minus_1", "n_scan_tile", "n_scan_tile_plus_1",
              "own_T-1_halo_row_last", "own_T_halo_row_T-1", "own_T+1_halo_row_T-1", "own_T+1_halo_row_T", "own_2T+1_halo_row_T-1",
              "own_2T+1_halo_row_T", "perm_not_identity", "cut_axis_2", "special_values")
TAIL_NAMES = ("tail_split_0", "tail_split_1", "tail_all_interior", "tail_none_interior", "tail_empty_rank", "tail_world_1_split",
              "tail_dom_shorter_than_ids", "tail_row_lengths_split", "tail_world_32_ends_exchange",
              "tail_own_T+1_halo_row_T-1", "tail_own_T+1_halo_row_T", "tail_own_2T+1_halo_row_T_split", "tail_n_scan_tile_plus_1_split",
              "tail_special_values_split")
REFUSED_TAIL_NAMES = ("tail_column_outside_window",)
NAMES = PLAN_NAMES + TAIL_NAMES + REFUSED_TAIL_NAMES


@functools.lru_cache(None)
def limits():
    """the limits of the built planners; the call touches no device"""
    from adaptiveviscositysolver_amd import capi
    i = capi.dist_plan_limits()
    return Limits(i.lds_planes, i.scan_tile, i.spmv_tile_rows, i.row_group, i.max_world)


class Case:
    def __init__(self, name, rows, *, xs=None, world=1, levels=1, extent=1, level=None, perm=None, cut_axis=0, val=None,
                 owner=None, split=0, dom=None, predicate=None):
        self.name = name
        self.tail = owner is not None
        lens = np.array([len(r) for r in rows], np.int64)
        self.n = len(rows)
        self.row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        self.col = (np.concatenate([np.asarray(r, np.int64) for r in rows]) if lens.sum() else np.zeros(0)).astype(np.int32)
        nnz = len(self.col)
        # values that tell every entry from every other one (the planner must move them unchanged)
        self.val = np.ascontiguousarray(val, np.float64) if val is not None else 1.0 + np.arange(nnz) / 4096.0
        self.world, self.levels, self.extent, self.cut_axis, self.split = world, levels, extent, cut_axis, split
        self.perm = None if perm is None else np.ascontiguousarray(perm, np.int32)
        self.dof = None
        if not self.tail:
            dof = np.zeros((self.n, 4), np.int32)       # one record per DOF: row i stands for the DOF perm[i]
            dof[:, 0] = (0 if level is None else np.asarray(level)) | (cut_axis << 8)
            dof[:, 1 + cut_axis] = xs
            for a in range(3):                          # the other coordinates must not matter
                if a != cut_axis:
                    dof[:, 1 + a] = (np.arange(self.n) * (7 + a)) % 5
            if perm is not None:
                placed = np.zeros_like(dof)
                placed[self.perm] = dof                 # xs / level describe ROWS: put row i's record where perm[i] points
                dof = placed
            self.dof = dof
        self.owner = None if owner is None else np.ascontiguousarray(owner, np.uint8)
        self.dom = None if dom is None else np.ascontiguousarray(dom, np.int32)
        self.predicate = predicate or (lambda c, plans: True)
        assert self.n <= MAX_ROWS, (name, self.n)
        assert nnz == 0 or (self.col.min() >= 0 and self.col.max() < self.n), name

    # ---- the model's side ------------------------------------------------------------------------------------------------------------
    @functools.lru_cache(None)
    def owners(self):
        """PLAN: (weights, plane_owner, owner per row) of the model; TAIL: (None, None, the case's owner bytes)"""
        if self.tail:
            return None, None, self.owner.astype(np.int32)
        return M.owners(self.row_ptr, self.dof, self.perm, self.levels, self.cut_axis, self.extent, self.world)

    @functools.lru_cache(None)
    def plans(self):
        """the model's plan of every rank (computed once, shared by the tests, never written to)"""
        T = limits().T
        owner = self.owners()[2]
        if self.tail:
            def one(r):
                try:
                    return M.tail_plan(self.row_ptr, self.col, self.val, owner, r, self.world, self.split, self.dom, T)
                except M.OutsideWindow:
                    return REFUSED
            return tuple(one(r) for r in range(self.world))
        return tuple(M.plan(self.row_ptr, self.col, self.val, owner, r, self.world, T) for r in range(self.world))

    def reaches_its_edge(self):
        return bool(self.predicate(self, self.plans()))

    def symmetric(self):
        pairs = set()
        for i in range(self.n):
            for c in self.col[self.row_ptr[i]:self.row_ptr[i + 1]]:
                pairs.add((i, int(c)))
        return all((c, r) in pairs for r, c in pairs)


# ---- patterns ------------------------------------------------------------------------------------------------------------------------------
def band(n, extra=()):
    """rows {i - 1, i, i + 1} (clipped) plus the symmetric couplings in `extra`"""
    rows = [[j for j in (i - 1, i, i + 1) if 0 <= j < n] for i in range(n)]
    for a, b in extra:
        rows[a].append(b)
        rows[b].append(a)
    return rows


def diagonal(n):
    return [[i] for i in range(n)]


def spread(n, extent):
    """n coordinates 0 .. extent - 1, non-decreasing, every value of [0, extent) taken when n >= extent"""
    return (np.arange(n, dtype=np.int64) * extent) // n


def n_own(plans):
    return [len(p["own_global"]) for p in plans]


def peers_of(plans, r):
    return [int(q) for q in plans[r]["peers"]]


def as_tail(name, plan_case, split, **kw):
    """the TAIL twin of a PLAN case with a symmetric pattern: same matrix, the model's owners as owner bytes"""
    rows = [list(plan_case.col[plan_case.row_ptr[i]:plan_case.row_ptr[i + 1]]) for i in range(plan_case.n)]
    return Case(name, rows, world=plan_case.world, owner=plan_case.owners()[2], split=split, val=plan_case.val, **kw)


def _tile_case(name, own, halo_row, L):
    """two planes, two ranks: rank 0 owns `own` diagonal rows of which only `halo_row` reads rank 1 (and is read by it)"""
    T = L.T
    n = own + 3
    rows = diagonal(n)
    rows[halo_row].append(own + 1)
    rows[own + 1].append(halo_row)
    xs = np.array([0] * own + [1] * 3)

    def pred(c, plans):
        p = plans[0]
        reading = [l for l in range(own) if (p["col_local"][p["row_ptr_local"][l]:p["row_ptr_local"][l + 1]] >= own).any()]
        return n_own(plans)[0] == own and reading == [halo_row] and list(p["tiles_bnd"]) == [halo_row // T] and \
            len(p["tiles_int"]) == -(-own // T) - 1
    return Case(name, rows, xs=xs, world=2, extent=2, predicate=pred)


def _row_length_rows(n, rng):
    """every length of ROW_LENGTHS in both halves of the ids, columns anywhere (duplicates included), the rest of the rows a band"""
    rows = band(n)
    for half in (0, 1):
        for k, R in enumerate(ROW_LENGTHS):
            i = half * (n // 2) + 5 + 3 * k
            rows[i] = list(rng.integers(0, n, R))
    return rows


def _symmetric_row_lengths(n):
    """the same lengths at the same rows in a SYMMETRIC pattern: a chosen row of length R is coupled with R other rows (none of them chosen,
    none twice, on both sides of the middle), which read it back; everything else is a band"""
    chosen = {half * (n // 2) + 5 + 3 * k: R for half in (0, 1) for k, R in enumerate(ROW_LENGTHS)}
    rows = [[j for j in (i - 1, i, i + 1) if 0 <= j < n and j not in chosen] if i not in chosen else [] for i in range(n)]
    others = [i for i in range(n) if i not in chosen]
    for d, R in chosen.items():
        start = (7 * d) % len(others)
        partners = [others[(start + (len(others) // 2 + 1) * k) % len(others)] if R <= 33 else others[(start + k) % len(others)] for k in range(R)]
        assert len(set(partners)) == R
        rows[d] = partners
        for p in partners:
            rows[p].append(d)
    return rows


def _special_values(nnz):
    """-0.0, denormals, infinities and NaNs with payloads: the planner moves 64-bit patterns"""
    bits = np.array([0x8000000000000000, 0x0000000000000001, 0x800fffffffffffff, 0x7ff8000000000001, 0xfff4dead0000beef, 0x7ff0000000000000,
                     0x7ff00000000000a5, 0x3ff0000000000000], np.uint64)
    return (bits[np.arange(nnz) % len(bits)] ^ (np.arange(nnz, dtype=np.uint64) << np.uint64(13) & np.uint64(0x000ffffffff00000))).view(np.float64)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def cases():
    L = limits()
    T = L.T
    rng = np.random.default_rng(SEED)
    out = []
    add = out.append

    add(Case("world_1", band(50), xs=spread(50, 8), world=1, extent=8,
             predicate=lambda c, P: n_own(P) == [50] and len(P[0]["peers"]) == 0 and len(P[0]["halo_global"]) == 0))
    # three planes of weight 5 for five ranks: the planes go to ranks 1, 2 and 3
    add(Case("world_above_planes", [[0, 1, 2]] * 3, xs=[0, 1, 2], world=5, extent=3,
             predicate=lambda c, P: list(c.owners()[0]) == [5, 5, 5] and list(c.owners()[1]) == [1, 2, 3] and n_own(P) == [0, 1, 1, 1, 0]))
    # weights [0, 0, 7, 0, 9, 0]: the last plane weighs nothing and is all the last rank gets
    two = [[0, 1, 0, 1, 0], [1, 0, 1, 0, 1, 0, 1]]
    add(Case("trailing_empty_plane", two, xs=[2, 4], world=3, extent=6,
             predicate=lambda c, P: list(c.owners()[0]) == [0, 0, 7, 0, 9, 0] and list(c.owners()[1]) == [0, 0, 0, 1, 1, 2] and n_own(P) == [1, 1, 0]))
    add(Case("trailing_empty_plane_interior_rank", two, xs=[2, 4], world=4, extent=6,
             predicate=lambda c, P: list(c.owners()[1]) == [0, 0, 0, 1, 2, 3] and n_own(P) == [1, 0, 1, 0]))
    xs = np.array([4, 5, 6] * 10 + [10, 11, 12] * 10)
    add(Case("empty_planes_lead_and_middle", band(60), xs=np.sort(xs), world=2, extent=16,
             predicate=lambda c, P: (c.owners()[0][[0, 1, 2, 3, 7, 8, 9]] == 0).all() and min(n_own(P)) > 0))
    add(Case("extent_not_multiple_of_granule", band(40), xs=spread(40, 10), world=3, levels=3, extent=10,
             predicate=lambda c, P: len(c.owners()[0]) == 3 and c.extent % 4 != 0 and min(n_own(P)) > 0))
    # faces on the upper border (pos == extent), fine and coarse: they belong to the last plane
    xs = np.concatenate([spread(30, 8), [8, 8, 2, 1]])
    lv = np.concatenate([np.zeros(30, np.int64), [0, 0, 2, 3]])
    add(Case("faces_at_extent", band(34), xs=xs, level=lv, world=2, levels=2, extent=8,
             predicate=lambda c, P, xs=xs, lv=lv: (c.owners()[2][30:] == c.owners()[1][-1]).all() and ((xs << lv)[30:] == 8).all()))
    lv = np.arange(90) % 3
    xs = spread(90, 32) >> lv
    add(Case("several_levels", band(90), xs=xs, level=lv, world=4, levels=3, extent=32,
             predicate=lambda c, P, lv=lv: min(n_own(P)) > 0 and len(set(lv)) == 3))
    for name, extent in (("planes_lds_limit", L.lds_planes), ("planes_lds_limit_plus_1", L.lds_planes + 1), ("planes_4096", 2 * L.lds_planes)):
        n = 3000
        xs = spread(n, extent)
        xs[-1] = extent - 1
        add(Case(name, band(n), xs=xs, world=4, extent=extent,
                 predicate=lambda c, P, e=extent: len(c.owners()[0]) == e and c.owners()[0][-1] > 0 and min(n_own(P)) > 0))
    n = 32 * 20
    add(Case("world_32_ends_exchange", band(n, extra=[(3, n - 2), (7, n - 9)]), xs=spread(n, 32), world=L.max_world, extent=32,
             predicate=lambda c, P: min(n_own(P)) > 0 and 31 in peers_of(P, 0) and 0 in peers_of(P, 31) and 1 in peers_of(P, 0)))
    add(Case("non_neighbour_peers", band(80, extra=[(2, 45), (3, 70), (25, 75)]), xs=spread(80, 4), world=4, extent=4,
             predicate=lambda c, P: peers_of(P, 0) == [1, 2, 3] and peers_of(P, 3) == [0, 1, 2] and peers_of(P, 2) == [0, 1, 3]))
    # block-diagonal but for one entry: a row of rank 0 reads an id of rank 1, and nobody of rank 1 reads rank 0
    rows = diagonal(40)
    rows[5] = [5, 30]
    add(Case("send_only_and_receive_only_peers", rows, xs=spread(40, 2), world=2, extent=2,
             predicate=lambda c, P: list(P[0]["send_counts"]) == [0] and list(P[0]["recv_counts"]) == [1] and
             list(P[1]["send_counts"]) == [1] and list(P[1]["recv_counts"]) == [0] and not c.symmetric()))
    n = 420
    rl = _row_length_rows(n, rng)

    def lengths_on_both_sides(c, P):
        owner = c.owners()[2]
        R = np.diff(c.row_ptr)
        return all(any(R[i] == want and owner[i] == q for i in range(c.n)) for want in ROW_LENGTHS for q in (0, 1))
    add(Case("row_lengths", rl, xs=spread(n, 2), world=2, extent=2, predicate=lengths_on_both_sides))
    for name, n in (("n_scan_tile_minus_1", L.scan_tile - 1), ("n_scan_tile", L.scan_tile), ("n_scan_tile_plus_1", L.scan_tile + 1)):
        add(Case(name, band(n, extra=[(0, n - 1)]), xs=spread(n, 3), world=3, extent=3,
                 predicate=lambda c, P, n=n: c.n == n and min(n_own(P)) > 0 and owner_of_last_is_last(c)))
    add(_tile_case("own_T-1_halo_row_last", T - 1, T - 2, L))
    add(_tile_case("own_T_halo_row_T-1", T, T - 1, L))
    add(_tile_case("own_T+1_halo_row_T-1", T + 1, T - 1, L))
    add(_tile_case("own_T+1_halo_row_T", T + 1, T, L))
    add(_tile_case("own_2T+1_halo_row_T-1", 2 * T + 1, T - 1, L))
    add(_tile_case("own_2T+1_halo_row_T", 2 * T + 1, T, L))
    n = 120
    perm = rng.permutation(n)
    add(Case("perm_not_identity", band(n, extra=[(4, 100)]), xs=spread(n, 6), perm=perm, world=3, extent=6,
             predicate=lambda c, P: (c.perm != np.arange(c.n)).any() and min(n_own(P)) > 0 and
             # read without the perm the dof records give other owners
             not np.array_equal(M.owners(c.row_ptr, c.dof, None, 1, 0, 6, 3)[2], c.owners()[2])))
    add(Case("cut_axis_2", band(60), xs=spread(60, 12), cut_axis=2, world=3, levels=2, extent=12,
             predicate=lambda c, P: min(n_own(P)) > 0 and (c.dof[:, 0] >> 8 == 2).all()))
    rows = band(64, extra=[(1, 60), (20, 40)])
    nnz = sum(len(r) for r in rows)
    sv = _special_values(nnz)
    add(Case("special_values", rows, xs=spread(64, 4), world=4, extent=4, val=sv,
             predicate=lambda c, P: np.isnan(c.val).any() and (c.val.view(np.uint64) == np.uint64(1) << np.uint64(63)).any() and
             ((np.abs(c.val) < 2.3e-308) & (c.val != 0)).any()))

    # ---- TAIL: owner bytes given, symmetric patterns ----
    by = {c.name: c for c in out}
    base = Case("tail_base", band(200, extra=[(3, 150), (60, 190), (10, 120)]), xs=spread(200, 4), world=4, extent=4)
    has_both = lambda c, P: all(0 < p["n_interior"] < len(p["own_global"]) for p in P)
    add(as_tail("tail_split_0", base, 0, predicate=lambda c, P: all(p["n_interior"] == -1 for p in P) and peers_of(P, 0) == [1, 2, 3]))
    add(as_tail("tail_split_1", base, 1, predicate=lambda c, P: has_both(c, P) and
                any((np.diff(p["own_global"]) < 0).any() for p in P)))     # the split really reorders
    blocks = [[j for j in (i - 1, i, i + 1) if 0 <= j < 90 and j // 30 == i // 30] for i in range(90)]
    add(Case("tail_all_interior", blocks, world=3, owner=np.arange(90) // 30, split=1,
             predicate=lambda c, P: all(p["n_interior"] == 30 and len(p["peers"]) == 0 and len(p["tiles_bnd"]) == 0 for p in P)))
    pairs = [[i, (i + 40) % 80] for i in range(80)]
    add(Case("tail_none_interior", pairs, world=2, owner=np.arange(80) // 40, split=1,
             predicate=lambda c, P: all(p["n_interior"] == 0 and len(p["own_global"]) == 40 for p in P)))
    add(Case("tail_empty_rank", band(50), world=4, owner=np.where(np.arange(50) < 25, 0, 3), split=1,
             predicate=lambda c, P: n_own(P) == [25, 0, 0, 25] and peers_of(P, 0) == [3] and len(P[1]["row_ptr_local"]) == 1))
    add(Case("tail_world_1_split", band(30), world=1, owner=np.zeros(30), split=1,
             predicate=lambda c, P: P[0]["n_interior"] == 30 and np.array_equal(P[0]["own_global"], np.arange(30))))
    # a window: ids 0 .. 19 and 100 .. 119 lie outside (owner 0xFF) and nothing inside reads them; dom lists the window in an order of its own
    owner = np.full(120, M.OUTSIDE)
    owner[20:100] = (np.arange(80) // 20)
    rows = [[i] for i in range(120)]
    for i in range(20, 100):
        rows[i] = [j for j in (i - 1, i, i + 1) if 20 <= j < 100]
    for a, b in ((25, 70), (26, 90), (45, 95), (27, 72), (28, 74), (29, 61), (30, 66)):
        rows[a].append(b)
        rows[b].append(a)
    dom = 20 + rng.permutation(80)
    add(Case("tail_dom_shorter_than_ids", rows, world=4, owner=owner, split=1, dom=dom,
             predicate=lambda c, P: len(c.dom) < c.n and all(not p["unnumbered_halo"] for p in P) and dom_order_shows(P)))
    sym = Case("tail_rl_base", _symmetric_row_lengths(len(rl)), xs=spread(len(rl), 2), world=2, extent=2)
    add(as_tail("tail_row_lengths_split", sym, 1, predicate=lambda c, P: has_both(c, P) and lengths_on_both_sides(c, P)))
    add(as_tail("tail_world_32_ends_exchange", by["world_32_ends_exchange"], 1,
                predicate=lambda c, P: 31 in peers_of(P, 0) and 0 in peers_of(P, 31) and has_both(c, P)))
    add(as_tail("tail_own_T+1_halo_row_T-1", by["own_T+1_halo_row_T-1"], 0,
                predicate=lambda c, P: list(P[0]["tiles_bnd"]) == [0] and list(P[0]["tiles_int"]) == [1]))
    add(as_tail("tail_own_T+1_halo_row_T", by["own_T+1_halo_row_T"], 0,
                predicate=lambda c, P: list(P[0]["tiles_bnd"]) == [1] and list(P[0]["tiles_int"]) == [0]))
    # with the split the one halo-reading row becomes the last local row: the last tile holds nothing else
    add(as_tail("tail_own_2T+1_halo_row_T_split", by["own_2T+1_halo_row_T"], 1,
                predicate=lambda c, P: P[0]["n_interior"] == 2 * T and P[0]["own_global"][-1] == T and list(P[0]["tiles_bnd"]) == [2]))
    add(as_tail("tail_n_scan_tile_plus_1_split", by["n_scan_tile_plus_1"], 1, predicate=has_both))
    add(as_tail("tail_special_values_split", by["special_values"], 1, predicate=lambda c, P: has_both(c, P) and np.isnan(c.val).any()))
    # refused for rank 1 alone: its row 45 reads id 5, which lies outside every window
    owner = np.concatenate([np.full(10, M.OUTSIDE), np.arange(80) // 20 % 4])
    rows = band(90)
    rows[9].remove(10)
    rows[10].remove(9)
    rows[45].append(5)
    rows[5].append(45)
    add(Case("tail_column_outside_window", rows, world=4, owner=owner, split=1,
             predicate=lambda c, P: [p == REFUSED for p in P] == [False, True, False, False]))

    assert tuple(c.name for c in out) == NAMES, [c.name for c in out]
    return tuple(out)


def owner_of_last_is_last(c):
    return int(c.owners()[2][-1]) == c.world - 1


def dom_order_shows(P):
    """some rank's halo group is not ascending: the halo follows the order of dom"""
    for p in P:
        off = 0
        for cnt in p["recv_counts"]:
            if (np.diff(p["halo_global"][off:off + cnt]) < 0).any():
                return True
            off += cnt
    return False


def by_name(name):
    return {c.name: c for c in cases()}[name]
