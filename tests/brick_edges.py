"""Planted cases for the brick-structured SpMV form (csrc/avs_brick_build.hip builds it, csrc/avs_brick.hip multiplies with it), placed from
the limits the code was compiled with (avs_brick_form_probe's limits-only call) and a fixed seed.

A case is a small lattice of faces: a few 8^3 bricks, chosen cells at levels 0 .. 4, every face of a cell a row.  A row reads itself and the
faces it is LINKED to; links are geometric, so translated rows share a pattern, and a per-row choice among a stencil's subsets gives as many
patterns as a case needs.  Values come from a palette indexed by the geometric offset (one dictionary) or are random per entry (value-code
variant); all are float values, so the float kernel may run every case.  EDGES names, per edge of the tile form, the cases on each side of it
and the fact of the model (tests/brick_model.py) that puts them there: tests/test_brick_edges.py checks every line on the CPU,
tests/test_gpu_brick_edges.py runs the cases.

Edges the lattice cannot produce (stated here instead of planted):
  * a slot delta outside -4096 .. 4095: the delta of a lattice slot is taken against the row's base on the SAME lattice, and the largest
    lattice has 3000 slots: |delta| < 3000.  An extra slot (3936 .. 4095) is taken against the row's level-0 base, which is at least
    3 (S^2 + S + 1) = 333 for a row with an own slot (bx, by, bz >= 1, S = 10) and at most 2999: 937 <= delta <= 3762.  The 13-bit field
    never overflows; neither -4096 / -4097 nor 4095 / 4096 can be reached from a valid matrix.
  * 384 patterns in a tile of the value-code variant: 384 patterns of one quad each are exactly its word cap, and the cases' stencil has only
    93 subsets per axis that short; the pattern-count edge is planted for the dictionary variant, the word cap for both.
"""
import functools
import os
from collections import namedtuple

import numpy as np

import brick_model as M

SEED = 20261019
TGT = (1, 1, 0)                      # the target brick of the standard scene (4 x 3 x 1 bricks)
RANDOM_VALUES = 300
FAR = (3, 1, 0)                      # two bricks away: its columns have no slot in the target's tiles


@functools.lru_cache(None)
def limits():
    """the limits of the built code; the call touches no device"""
    from adaptiveviscositysolver_amd import capi
    info = capi.brick_form_limits()
    return namedtuple("Limits", [k for k, _ in info._fields_])(*[getattr(info, k) for k, _ in info._fields_])


class Case:
    def __init__(self, name, b, values="palette", vc=False, racy_extras=False, target=TGT, env=None):
        self.name, self.vc, self.racy_extras, self.target = name, vc, racy_extras, target
        self.env = dict(env or {})
        self.nx, self.ny, self.nz = 8 * b.nb[0], 8 * b.nb[1], 8 * b.nb[2]
        self.levels = 5
        rng = np.random.default_rng([SEED, sum(map(ord, name))])
        own = np.array(b.keys, np.int64).reshape(-1, 5)
        dof = np.stack([own[:, 0] | (own[:, 1] << 8), own[:, 2], own[:, 3], own[:, 4]], axis=1)
        brick = M.geometry(dof, self.nx, self.ny, self.nz)[5]
        order = np.argsort(brick, kind="stable")            # brick-major, the order of insertion inside a brick
        keys = [b.keys[i] for i in order] + list(b.halo)
        self.n_rows, self.n_cols = len(b.keys), len(keys)
        ids = {k: i for i, k in enumerate(keys)}
        assert len(ids) == len(keys), "a face was added twice"
        ka = np.array(keys, np.int64).reshape(-1, 5)
        self.dof = np.ascontiguousarray(np.stack([ka[:, 0] | (ka[:, 1] << 8), ka[:, 2], ka[:, 3], ka[:, 4]], axis=1), np.int32)
        palette = (rng.choice([-1.0, 1.0], 7) * (1.0 + rng.random(7))).astype(np.float32).astype(np.float64)
        diag = float(np.float32(4.0 + palette[0]))
        rp, col, val = [0], [], []
        for r in range(self.n_rows):
            k = keys[r]
            cols = sorted({ids[k]} | {ids[c] for c in b.links.get(k, ())})
            for c in cols:
                kc = keys[c]
                off = (kc[0], kc[1], (kc[2] << kc[0]) - (k[2] << k[0]), (kc[3] << kc[0]) - (k[3] << k[0]), (kc[4] << kc[0]) - (k[4] << k[0]))
                val.append(palette[(off[0] * 5 + off[1] * 3 + off[2] * 7 + off[3] * 11 + off[4] * 13) % 7] if c != r else diag)
            col += cols
            rp.append(len(col))
        self.row_ptr = np.array(rp, np.int32)
        self.col = np.array(col, np.int32)
        self.val = np.array(val, np.float64)
        self.force_vc = values == "random"     # (too few values overall to reach the variant: the probe's flag asks for it)
        if values == "random":     # per entry, drawn from a table of RANDOM_VALUES values per brick: a tile's table holds them
            brick_of_row = M.geometry(self.dof, self.nx, self.ny, self.nz)[5][:self.n_rows]
            erow = np.repeat(np.arange(self.n_rows), np.diff(self.row_ptr))
            pick = brick_of_row[erow] * RANDOM_VALUES + rng.integers(0, RANDOM_VALUES, len(col))
            pal = (rng.choice([-1.0, 1.0], int(pick.max()) + 1) * (1.0 + rng.random(int(pick.max()) + 1))).astype(np.float32).astype(np.float64)
            self.val = pal[pick]
        elif isinstance(values, int):   # `values` distinct values in the target brick's rows, other values elsewhere
            pal = (1.0 + np.arange(1, values + 1) / 1024.0).astype(np.float32).astype(np.float64)
            brick_of_row = M.geometry(self.dof, self.nx, self.ny, self.nz)[5][:self.n_rows]
            tb = (target[2] * b.nb[1] + target[1]) * b.nb[0] + target[0]
            erow = np.repeat(np.arange(self.n_rows), np.diff(self.row_ptr))
            inside = brick_of_row[erow] == tb
            self.val = -(2.0 + rng.random(len(col))).astype(np.float32).astype(np.float64)
            self.val[inside] = pal[np.arange(int(inside.sum())) % values]
        self.x = (rng.choice([-1.0, 1.0], self.n_cols) * (1.0 + rng.random(self.n_cols)) * 2.0 ** rng.integers(-3, 4, self.n_cols))
        self._model = {}

    @classmethod
    def golden(cls, scene):
        """a scene of tests/golden: the oracle's matrix (the fixture's row_ptr / col / val) and dof table (the fixture's velocity index
        fields: test_brick_edges.py checks them against orc_get_dof_table), permuted to brick-major order with the key of k_brick_keys
        (csrc/avs_reorder.hip: brick, then z, y, x of the face's clamped position inside the brick; a stable sort).  The values are rounded
        to float so that the float kernel may run the case."""
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", scene + ".npz"))
        self = cls.__new__(cls)
        self.name, self.racy_extras, self.target, self.env, self.force_vc = "golden_" + scene, False, None, {}, False
        self.nx, self.ny, self.nz = (int(v) for v in g["res"])
        self.levels = int(g["levels"])
        n = int(g["counts"][0])
        dof = np.full((n, 4), -1, np.int32)
        for l in range(self.levels):
            for a in range(3):
                v = g[f"vidx{l}_{a}"]                      # [z][y][x] -> dof id, negative: no dof
                at = np.argwhere(v >= 0)
                dof[v[v >= 0]] = np.stack([np.full(len(at), l | (a << 8)), at[:, 2], at[:, 1], at[:, 0]], axis=1)
        assert dof.min() >= 0
        self.ref_dof = dof
        level, axis, i, j, k, brick = M.geometry(dof, self.nx, self.ny, self.nz)
        px, py, pz = np.minimum(i << level, self.nx - 1), np.minimum(j << level, self.ny - 1), np.minimum(k << level, self.nz - 1)
        key = (brick << 9) | ((pz & 7) << 6) | ((py & 7) << 3) | (px & 7)
        perm = np.argsort(key, kind="stable")              # new -> old
        inv = np.empty(n, np.int64)
        inv[perm] = np.arange(n)
        rp, col, val = g["row_ptr"].astype(np.int64), g["col"], g["val"]
        lens = np.diff(rp)[perm]
        self.row_ptr = np.r_[0, np.cumsum(lens)].astype(np.int32)
        src = np.repeat(rp[:-1][perm], lens) + (np.arange(int(lens.sum())) - np.repeat(self.row_ptr[:-1].astype(np.int64), lens))
        self.col = inv[col[src]].astype(np.int32)          # (the stored order of a row's entries is kept)
        self.val = val[src].astype(np.float32).astype(np.float64)
        self.dof = np.ascontiguousarray(dof[perm])
        self.n_rows = self.n_cols = n
        nvals = len(np.unique(self.val))
        assert not 1500 <= nvals < limits().table_max, "the dictionary may or may not fit the workgroup's LDS: the variant is not certain"
        self.vc = nvals >= limits().table_max             # more values than one dictionary holds: the value-code variant
        rng = np.random.default_rng([SEED, n])
        self.x = (rng.choice([-1.0, 1.0], n) * (1.0 + rng.random(n)) * 2.0 ** rng.integers(-3, 4, n))
        self._model = {}
        return self

    def model(self, vc=None):
        """the model's tiles for this case (computed once; not to be written to); vc: the value-code variant (default: what the case reaches)"""
        vc = self.vc if vc is None else vc
        if vc not in self._model:
            self._model[vc] = M.model(self.row_ptr, self.col, self.val, self.dof, self.n_rows, self.nx, self.ny, self.nz, limits(), vc=vc)
        return self._model[vc]

    def target_tiles(self):
        return [T for T in self.model().tiles if T.origin == self.target and T.kind != "E"]


class Builder:
    def __init__(self, nb=(4, 3, 1)):
        self.nb, self.keys, self.halo, self.links, self.have = nb, [], [], {}, set()

    def face(self, key, halo=False):
        if key not in self.have:
            self.have.add(key)
            (self.halo if halo else self.keys).append(key)

    def cells(self, cells, level=0, axis_major=False, halo=False):
        cells = list(cells)
        faces = [(level, a) + c for a in range(3) for c in cells] if axis_major else [(level, a) + c for c in cells for a in range(3)]
        for k in faces:
            self.face(k, halo)
        return faces

    def link(self, row, colkey):
        assert row in self.have and colkey in self.have, (row, colkey)
        self.links.setdefault(row, []).append(colkey)

    def link_x(self, rows=None):
        """every row (or the given ones) reads its same-axis neighbours at x - 1 and x + 1 where they exist"""
        for k in (self.keys if rows is None else rows):
            for d in (-1, 1):
                n = (k[0], k[1], k[2] + d, k[3], k[4])
                if n in self.have and k[0] == 0:
                    self.link(k, n)


def brick_cells(ob, xs=range(8), ys=range(8), zs=range(8)):
    return [(8 * ob[0] + x, 8 * ob[1] + y, 8 * ob[2] + z) for z in zs for y in ys for x in xs]


# ---------------------------------------------------------------------------------------------------------------------------------
# the standard scene: target brick (8 x 8 x Z cells, cell-major), its x neighbours, a far brick, and a run of small bricks in front
# ---------------------------------------------------------------------------------------------------------------------------------
def std(Z=5, nrows=None, sides=True, small=True, ring_axis_major=False):
    b = Builder()
    if small:   # bricks (0..3, 0, 0): 63 rows each -> a run of small bricks, one E tile in front of the G tiles
        for bx in range(4):
            b.cells(brick_cells((bx, 0, 0), zs=range(1), ys=range(3))[:21])
    t = b.cells(brick_cells(TGT, zs=range(Z)))
    if nrows is not None:
        keep, drop = set(t[:nrows]), set(t[nrows:])
        b.keys = [k for k in b.keys if k not in drop]
        b.have = set(b.keys)
        t = t[:nrows]
    if sides:
        b.cells(brick_cells((0, 1, 0), zs=range(Z)), axis_major=ring_axis_major)
        b.cells(brick_cells((2, 1, 0), zs=range(Z)), axis_major=ring_axis_major)
    far = b.cells(brick_cells(FAR, zs=range(1), ys=range(3))[:22])
    return b, t, far


OFFS = [(dx, a) for dx in (-1, 0, 1) for a in range(3)]
SUBSETS = sorted(range(256), key=lambda s: (bin(s).count("1"), s))     # subsets of a row's 8 optional offsets, shortest first


def plant_patterns(b, t, per_axis, sizes=None):
    """row r of the target (cell r // 3, axis r % 3) reads the subset number (r // 3) % per_axis[axis] of its x-stencil (x - 1, x, x + 1; three
    axes): per_axis[0] + per_axis[1] + per_axis[2] distinct patterns, first used in the order (cell, axis)"""
    subs = [s for s in SUBSETS if sizes is None or bin(s).count("1") in sizes]
    for r, k in enumerate(t):
        a = k[1]
        opt = [o for o in OFFS if o != (0, a)]
        s = subs[(r // 3) % per_axis[a]]
        for bit, (dx, a2) in enumerate(opt):
            if s >> bit & 1:
                b.link(k, (0, a2, k[2] + dx, k[3], k[4]))


def plant_sets(b, t, per_axis):
    """the same for the value-code variant, whose patterns carry no value: the rows of axis a take, in turn, the first per_axis[a] of the
    sets of 5 .. 8 stencil offsets whose lowest same-cell member is the row itself -- every (axis, set) pair is another delta sequence"""
    lists = [[], [], []]
    for m in range(1 << len(OFFS)):
        S = [o for bit, o in enumerate(OFFS) if m >> bit & 1]
        own = [a for dx, a in S if dx == 0]
        if 5 <= len(S) <= 8 and own:
            lists[min(own)].append(S)
    for a in range(3):
        lists[a].sort(key=lambda S: (len(S), S))
        assert per_axis[a] <= len(lists[a])
    for r, k in enumerate(t):
        for dx, a2 in lists[k[1]][(r // 3) % per_axis[k[1]]]:
            if (dx, a2) != (0, k[1]):
                b.link(k, (0, a2, k[2] + dx, k[3], k[4]))


def split_words(W, longest=64):
    """row lengths (2 .. longest each) that total W"""
    out = [longest] * (W // longest)
    rem = W % longest
    if rem == 1:
        out[-1] -= 1
        rem = 2
    if rem:
        out.append(rem)
    return out


def plant_streamed(b, t, far, lengths, first=100, step=7):
    """rows first, first + step, ... of the target read far columns (no slot: streamed rows) and have the given lengths"""
    for i, ln in enumerate(lengths):
        for c in far[:ln - 1]:
            b.link(t[first + i * step], c)


def case_rows(name, nrows):
    b, t, far = std(Z=8, nrows=nrows, sides=False)
    b.link_x()
    return Case(name, b)


def case_erun(name, rows):
    """G brick | small bricks totalling `rows` rows | G brick | small brick | G brick: E tiles between G tiles"""
    b = Builder((10, 1, 1))
    b.cells(brick_cells((0, 0, 0), zs=range(1))[:22])
    left = rows
    for bx in range(1, 7):
        m = min(left, 51)
        faces = [(0, a) + c for c in brick_cells((bx, 0, 0), zs=range(1))[:18] for a in range(3)][:m]
        for k in faces:
            b.face(k)
        left -= m
    assert left == 0
    b.cells(brick_cells((7, 0, 0), zs=range(1))[:22])
    b.cells(brick_cells((8, 0, 0), zs=range(1))[:5])
    b.cells(brick_cells((9, 0, 0), zs=range(1))[:30])
    b.link_x()
    return Case(name, b, target=(0, 0, 0))


def case_rowlen(name, length):
    b, t, far = std()
    b.link_x(t[300:])
    row = t[3 * (8 * 3 + 3)]       # cell (3, 3, 0) of the target: all of it on the lattice
    others = [k for k in t[:400] if k != row][:length - 1]
    for k in others:
        b.link(row, k)
    return Case(name, b)


def case_level4(name):
    """a level-4 face in a neighbour brick, read by rows of the target: no lattice holds it, it takes an extra slot"""
    b, t, far = std()
    b.link_x()
    k4 = (4, 1, 1, 1, 0)               # a level-4 cell covers 16 fine cells: this one's corner, fine cell (16, 16, 0), lies in brick (2, 2, 0)
    b.face(k4)
    b.link(k4, t[0])
    b.link(t[10], k4)
    b.link(t[500], k4)
    return Case(name, b)


def case_level4_in_tile(name):
    """the target brick's own rows hold a face the lattices do not (level 4 needs i << 4 inside the brick: the grid is clamped at its end)"""
    b = Builder((2, 1, 1))
    t = b.cells(brick_cells((1, 0, 0), zs=range(3)))
    b.cells(brick_cells((0, 0, 0), zs=range(3)))
    b.link_x()
    k4 = (4, 2, 1, 0, 0)               # fine position 16 >= nx: clamped to 15 -> brick (1, 0, 0), the target
    b.face(k4)
    b.link(k4, t[5])
    b.link(t[7], k4)
    return Case(name, b, target=(1, 0, 0))


def case_extras(name, n, racy=False):
    """n off-lattice columns of the neighbour bricks (cells x - 2, x - 3, ... of the target's brick) read by the target's rows"""
    b, t, far = std()
    b.link_x()
    tx = 8 * TGT[0]
    cand = [(0, a, x, 8 * TGT[1] + y, z) for x in (tx - 2, tx + 9, tx - 3, tx + 10, tx - 4, tx + 11) for z in range(5) for y in range(8) for a in range(3)]
    assert len(cand) >= n
    for j, c in enumerate(cand[:n]):
        b.link(t[(5 * j) % len(t)], c)
    return Case(name, b, racy_extras=racy)


def case_patterns(name, per_axis, sizes=None, vc=False):
    b, t, far = std()
    if vc:
        plant_sets(b, t, per_axis)
    else:
        plant_patterns(b, t, per_axis, sizes)
    tset = set(t)
    b.link_x([k for k in b.keys if k not in tset])
    return Case(name, b, values="random" if vc else "palette", vc=vc)


def case_prow(name, nrows):
    b, t, far = std(nrows=nrows)
    b.link_x()
    return Case(name, b)


def case_runs(name, nruns):
    """nruns halo faces around the target, every one a fill run of its own: the ring bricks are numbered axis-major, so consecutive slots
    (the three axes of a cell) never have consecutive columns"""
    b = Builder((4, 3, 1))
    Z = 5
    t = b.cells(brick_cells(TGT, zs=range(Z)))
    tx, ty = 8 * TGT[0], 8 * TGT[1]
    ring = []   # (halo cell, the target cell that reads it)
    for z in range(Z):
        for y in range(8):
            ring += [((tx - 1, ty + y, z), (tx, ty + y, z)), ((tx + 8, ty + y, z), (tx + 7, ty + y, z))]
        for x in range(8):
            ring += [((tx + x, ty - 1, z), (tx + x, ty, z)), ((tx + x, ty + 8, z), (tx + x, ty + 7, z))]
        ring += [((tx - 1, ty - 1, z), (tx, ty, z)), ((tx + 8, ty - 1, z), (tx + 7, ty, z)), ((tx - 1, ty + 8, z), (tx, ty + 7, z)),
                 ((tx + 8, ty + 8, z), (tx + 7, ty + 7, z))]
    by_brick = {}
    for h, _ in ring:
        by_brick.setdefault((h[0] >> 3, h[1] >> 3), []).append(h)
    for ob, cs in sorted(by_brick.items()):
        b.cells(cs, axis_major=True)
    assert 3 * len(ring) >= nruns
    j = 0
    for h, c in ring:
        for a in range(3):
            if j < nruns:
                b.link((0, 0) + c, (0, a) + h)
                j += 1
    return Case(name, b)


def case_no_pattern(name):
    """no row of the target is a pattern (every one reads a far column): a G tile that runs in e-mode"""
    b, t, far = std()
    for k in t:
        b.link(k, far[0])
    tset = set(t)
    b.link_x([k for k in b.keys if k not in tset])
    return Case(name, b)


def case_streamed_exact(name, W, vc=False):
    """the target's streamed rows total exactly W words (x links are given to the other rows only)"""
    b, t, far = std()
    lengths = split_words(W, 64)
    planted = {t[100 + i * 7] for i in range(len(lengths))}
    b.link_x([k for k in b.keys if k not in planted])
    plant_streamed(b, t, far, lengths)
    return Case(name, b, values="random" if vc else "palette", vc=vc)


def case_emode(name, W):
    """the E tile of the standard scene (4 small bricks, 252 rows) with exactly W words"""
    b, t, far = std()
    b.link_x(t)
    e = [k for k in b.keys if k[3] < 8]     # the small bricks (0..3, 0, 0)
    n = len(e)
    base, extra = divmod(W - n, n)
    for i, k in enumerate(e):
        for d in range(1, base + 1 + (1 if i < extra else 0)):
            b.link(k, e[(i + d) % n])
    return Case(name, b)


SHAPE_LENGTHS = (4, 5, 8, 9, 64)


def case_shapes(name, vc):
    """rows of 1, 4, 5 and 64 entries among the pattern rows (a pattern of exactly q quads, one of 4 q + 1 padded with the zero code)"""
    b, t, far = std()
    geo = [(dx, dy, dz, a) for dz in (0, -1, 1) for dy in (0, -1, 1) for dx in (0, -1, 1) for a in range(3)]
    for i, k in enumerate(t):
        x, y, z = k[2] - 8 * TGT[0], k[3] - 8 * TGT[1], k[4]
        if not (1 <= x <= 6 and 1 <= y <= 6 and 1 <= z <= 3):
            continue                   # (a row of one entry)
        want = SHAPE_LENGTHS[(i // 3) % len(SHAPE_LENGTHS)]
        for dx, dy, dz, a in [g for g in geo if g != (0, 0, 0, k[1])][:want - 1]:
            b.link(k, (0, a, k[2] + dx, k[3] + dy, k[4] + dz))
    tset = set(t)
    b.link_x([k for k in b.keys if k not in tset])
    return Case(name, b, values="random" if vc else "palette", vc=vc)


def case_values(name, nvals, forced=True):
    """value-code variant: the target tile's rows hold exactly nvals distinct values"""
    b, t, far = std()
    b.link_x()
    return Case(name, b, values=nvals, vc=True)


def case_coarse(name):
    """a brick of level-1 cells next to the target: the target's rows at x = 0 read level-1 faces (patterns that are not level-0 only)"""
    b = Builder((2, 1, 1))
    c1 = b.cells([(x, y, z) for z in range(2) for y in range(4) for x in range(4)], level=1)
    t = b.cells(brick_cells((1, 0, 0), zs=range(4)))
    b.link_x()
    for k in t:
        if k[2] == 8 and k[1] != 1:
            b.link(k, (1, k[1], 3, k[3] >> 1, k[4] >> 1))
    for k in c1:
        if k[2] == 3:
            b.link(k, (0, k[1], 8, 2 * k[3], 2 * k[4]))
    return Case(name, b, target=(1, 0, 0))


def case_halo(name, vc=False):
    """a partitioned rank's local system: columns >= n_rows read by pattern rows (through fill runs) and by streamed rows"""
    b, t, far = std(sides=False)
    tx, ty = 8 * TGT[0], 8 * TGT[1]
    h = b.cells([(tx - 1, ty + y, z) for z in range(5) for y in range(8)], halo=True)
    hf = b.cells([(tx - 5, ty + y, 0) for y in range(8)], halo=True)     # off the target's lattice, too many for ... no: extra slots
    b.link_x()
    plant_streamed(b, t, far, [9, 17])
    b.link(t[100], hf[0])           # a streamed row reads a halo column
    small = [k for k in b.keys if k[3] < 8]
    b.link(small[3], h[0])          # ... and so does a row of the E tile in front
    return Case(name, b, values="random" if vc else "palette", vc=vc)


def case_mix_walk(name, vc=False):
    """G, E, G with streamed rows, E, G: what one workgroup of a small grid meets in one walk, in both orders"""
    b = Builder((8, 1, 1))
    far = b.cells(brick_cells((7, 0, 0), zs=range(1))[:30])
    kinds = []
    for bx, kind in enumerate("GeSeGSe"):
        n = {"G": 128, "S": 96, "e": 20}[kind]
        f = b.cells(brick_cells((bx, 0, 0), zs=range(3))[:n])
        kinds.append((kind, f))
    b.link_x()
    for kind, f in kinds:
        if kind == "S":
            for i in range(5, len(f), 9):
                for c in far[:1 + i % 11]:
                    b.link(f[i], c)
    return Case(name, b, values="random" if vc else "palette", vc=vc, target=(0, 0, 0))


def case_many_tiles(name, vc=False):
    """40 bricks -> 36 tiles of every kind: grids of 8 and 16 workgroups walk several tiles each, under every walk"""
    b = Builder((10, 4, 1))
    bricks = []
    for by in range(4):
        for bx in range(10):
            kind = "GSGeeGSGGe"[(bx + 3 * by) % 10]
            n = {"G": 40, "S": 30, "e": 10}[kind]
            bricks.append((kind, (bx, by, 0), b.cells(brick_cells((bx, by, 0), zs=range(2))[:n])))
    b.link_x()
    for kind, ob, f in bricks:
        if kind == "S":
            other = next(g for k2, o2, g in bricks if o2 == ((ob[0] + 3) % 10, ob[1], 0))
            for i in range(2, len(f), 5):
                for c in other[:1 + (7 * i) % 23]:
                    b.link(f[i], c)
    return Case(name, b, values="random" if vc else "palette", vc=vc, target=(0, 0, 0))


# ---------------------------------------------------------------------------------------------------------------------------------

def streamed_word_counts(L):
    return (("511", 511), ("512", 512), ("513", 513), ("park-1", L.park_words - 1), ("park", L.park_words), ("park+1", L.park_words + 1),
            ("1023", 1023), ("1024", 1024), ("1025", 1025), ("2park+1", 2 * L.park_words + 1))


@functools.lru_cache(None)
def cases():
    L = limits()
    pw8, pwv8 = L.pat_words // 8, L.pat_words_vc // 8
    split3 = lambda n: ((n + 2) // 3, (n + 1) // 3, n // 3)
    out = [
        case_rows("rows_min-1", L.min_rows - 1), case_rows("rows_min", L.min_rows),
        case_rows("rows_max", L.max_rows), case_rows("rows_max+1", L.max_rows + 1), case_rows("rows_full_brick", 1536),
        case_erun("erun_etile-1", L.etile_rows - 1), case_erun("erun_etile", L.etile_rows), case_erun("erun_etile+1", L.etile_rows + 1),
        case_rowlen("rowlen_patlen", L.pat_len), case_rowlen("rowlen_patlen+1", L.pat_len + 1),
        case_level4("level4_column"), case_level4_in_tile("level4_row"),
        case_extras("extras_xslots", L.x_slots), case_extras("extras_xslots+1", L.x_slots + 1),
        case_extras("extras_racy", M.XSET + 60, racy=True),
        case_patterns("patterns_max", split3(L.pat_max), sizes=(0, 1, 2, 3, 4)),
        case_patterns("patterns_max+1", split3(L.pat_max + 1), sizes=(0, 1, 2, 3, 4)),
        case_patterns("patwords_cap", split3(pw8), sizes=(4, 5, 6, 7)), case_patterns("patwords_cap+", split3(pw8 + 1), sizes=(4, 5, 6, 7)),
        case_patterns("patwords_vc_cap", (pwv8 - 40, 20, 20), vc=True), case_patterns("patwords_vc_cap+", (pwv8 - 39, 20, 20), vc=True),
        case_prow("prow_512", 512), case_prow("prow_513", 513),
        case_coarse("coarse_neighbour"),
        case_runs("runs_fast", L.fast_runs), case_runs("runs_fast+1", L.fast_runs + 1),
        case_runs("runs_max", L.max_runs), case_runs("runs_max+1", L.max_runs + 1),
    ]
    for label, W in streamed_word_counts(L):
        out.append(case_streamed_exact(f"sw_{label}", W))
    out += [
        case_streamed_exact("sw_vc_park+1", L.park_words + 1, vc=True),
        case_emode("emode_cap", L.emode_words), case_emode("emode_cap+1", L.emode_words + 1),
        case_no_pattern("g_no_pattern"),
        case_shapes("shapes", vc=False), case_shapes("shapes_vc", vc=True),
        case_values("vals_tilevals", L.tile_vals), case_values("vals_tilevals+1", L.tile_vals + 1),
        case_halo("halo"), case_halo("halo_vc", vc=True),
        case_mix_walk("mix_walk"), case_mix_walk("mix_walk_vc", vc=True),
        case_many_tiles("many_tiles"), case_many_tiles("many_tiles_vc", vc=True),
    ]
    out += [Case.golden(s) for s in GOLDEN]
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return {c.name: c for c in out}


def case_names():
    """fixed here so that tests can be parametrised without building the cases"""
    return NAMES


GOLDEN = ("sphere16_L3", "beam32_L2_wall_varvisc", "sphere32_obstacle_rho_usolid")
NAMES = ("rows_min-1", "rows_min", "rows_max", "rows_max+1", "rows_full_brick", "erun_etile-1", "erun_etile", "erun_etile+1", "rowlen_patlen",
         "rowlen_patlen+1", "level4_column", "level4_row", "extras_xslots", "extras_xslots+1", "extras_racy", "patterns_max", "patterns_max+1",
         "patwords_cap", "patwords_cap+", "patwords_vc_cap", "patwords_vc_cap+", "prow_512", "prow_513", "coarse_neighbour", "runs_fast",
         "runs_fast+1", "runs_max", "runs_max+1", "sw_511", "sw_512", "sw_513", "sw_park-1", "sw_park", "sw_park+1", "sw_1023", "sw_1024",
         "sw_1025", "sw_2park+1", "sw_vc_park+1", "emode_cap", "emode_cap+1", "g_no_pattern", "shapes", "shapes_vc", "vals_tilevals",
         "vals_tilevals+1", "halo", "halo_vc", "mix_walk", "mix_walk_vc", "many_tiles", "many_tiles_vc") + tuple("golden_" + s for s in GOLDEN)


# ---------------------------------------------------------------------------------------------------------------------------------
# the edges: (edge, side, case, fact of the model that puts the case on that side).  T: the target brick's tiles (G or redone as E), A: all tiles
# ---------------------------------------------------------------------------------------------------------------------------------
def _spans(W, cap):
    """a planted streamed row (split_words) lies across the pass boundary at `cap` words"""
    ends = np.cumsum(split_words(W))
    return any(e - ln < cap < e for e, ln in zip(ends, split_words(W)))


def edges():
    L = limits()
    E = []

    def add(edge, side, case, fact):
        E.append((edge, side, case, fact))

    first_e = lambda A: next(t for t in A if t.kind == "E")
    add("brick rows >= min_rows: G tile", "below", "rows_min-1", lambda T, A: not T and all(t.kind == "E" for t in A[:-1]))
    add("brick rows >= min_rows: G tile", "at", "rows_min", lambda T, A: [t.nrows for t in T] == [L.min_rows] and T[0].kind == "G")
    add("brick rows > max_rows: cut in two", "at", "rows_max", lambda T, A: [t.nrows for t in T] == [L.max_rows])
    add("brick rows > max_rows: cut in two", "past", "rows_max+1", lambda T, A: [t.nrows for t in T] == [L.max_rows, 1])
    add("brick rows > max_rows: cut in two", "full brick", "rows_full_brick", lambda T, A: [t.nrows for t in T] == [L.max_rows, 1536 - L.max_rows] and T[0].origin == T[1].origin)
    for side, d in (("below", -1), ("at", 0), ("past", 1)):
        want = [L.etile_rows + d] if d <= 0 else [L.etile_rows, d]
        add("run of small bricks > etile_rows: next E tile", side, f"erun_etile{'%+d' % d if d else ''}",
            lambda T, A, want=want: [t.nrows for t in A if t.kind == "E"][:len(want)] == want and
            "GEG" in "".join(t.kind for t in A).replace("EE", "E"))
    add("row length <= pat_len: pattern row", "at", "rowlen_patlen", lambda T, A: T[0].nsrows == 0 and T[0].npq >= L.pat_len // 4)
    add("row length <= pat_len: pattern row", "past", "rowlen_patlen+1", lambda T, A: (T[0].nsrows, T[0].nsw) == (1, L.pat_len + 1))
    add("own face without a slot (level 4): streamed", "without", "level4_row", lambda T, A: (T[0].nsrows, T[0].nsw) == (1, 2))
    add("own face without a slot (level 4): streamed", "with", "rows_min", lambda T, A: T[0].nsrows == 0)
    add("own row without a lattice slot, read by a pattern row of its tile: a fill run of its extra slot", "planted", "level4_row",
        lambda T, A: T[0].ncand == 1 and T[0].nruns == 25 and T[0].nprow == T[0].nrows - 1)
    add("level-4 column in a neighbour brick: extra slot", "planted", "level4_column", lambda T, A: T[0].ncand == 1 and T[0].nsrows == 0)
    add("extra slots <= x_slots", "at", "extras_xslots", lambda T, A: T[0].ncand == L.x_slots and T[0].nsrows == 0)
    add("extra slots <= x_slots", "past", "extras_xslots+1", lambda T, A: T[0].ncand == L.x_slots + 1 and T[0].nsrows == 1)
    add("extra slots <= x_slots", "candidates overflow the set", "extras_racy", lambda T, A: T[0].ncand > M.XSET and T[0].racy)
    add("patterns per tile <= pat_max", "at", "patterns_max", lambda T, A: T[0].npat == T[0].npat_seen == L.pat_max and T[0].nsrows == 0)
    add("patterns per tile <= pat_max", "past", "patterns_max+1", lambda T, A: T[0].npat == L.pat_max and T[0].npat_seen == L.pat_max + 1 and T[0].nsrows > 0)
    for v, cap in (("", L.pat_words), ("_vc", L.pat_words_vc)):
        add(f"pattern words <= cap ({cap})", "at", f"patwords{v}_cap", lambda T, A, cap=cap: 4 * T[0].npq == T[0].pat_words_seen == cap and T[0].nsrows == 0)
        add(f"pattern words <= cap ({cap})", "past", f"patwords{v}_cap+",
            lambda T, A, cap=cap: 4 * T[0].npq == cap and T[0].pat_words_seen == cap + 8 and T[0].npat == T[0].npat_seen - 1 and T[0].nsrows > 0)
    add("pattern of 4 q / 4 q + 1 entries (padded with the zero code)", "both", "shapes", lambda T, A: T[0].nsrows == 0 and T[0].npat == 3 * (len(SHAPE_LENGTHS) + 1))
    add("pattern of 4 q / 4 q + 1 entries (padded with the zero code)", "both, value codes", "shapes_vc", lambda T, A: T[0].nsrows == 0 and T[0].ntv > 0)
    add("pattern rows per tile > 512: second row per thread", "at", "prow_512", lambda T, A: T[0].nprow == 512)
    add("pattern rows per tile > 512: second row per thread", "past", "prow_513", lambda T, A: T[0].nprow == 513)
    add("wave mixing level-0-only patterns with others", "mixed", "coarse_neighbour", lambda T, A: T[0].mixed_waves > 0)
    add("wave mixing level-0-only patterns with others", "none", "prow_512", lambda T, A: T[0].mixed_waves == 0)
    add("fill runs <= fast_runs: register batches", "at", "runs_fast", lambda T, A: T[0].nruns == L.fast_runs)
    add("fill runs <= fast_runs: register batches", "past", "runs_fast+1", lambda T, A: T[0].nruns == L.fast_runs + 1)
    add("fill runs <= max_runs", "at", "runs_max", lambda T, A: T[0].nruns == L.max_runs and T[0].kind == "G")
    add("fill runs <= max_runs", "past (redone as an E tile)", "runs_max+1", lambda T, A: T[0].kind == "GE" and T[0].nruns_seen == L.max_runs + 1 and T[0].nprow == 0)
    for label, W in streamed_word_counts(L):
        add("streamed words of a G tile: 512 per preload, park_words per pass", label, f"sw_{label}",
            lambda T, A, W=W: T[0].kind == "G" and T[0].npat > 0 and T[0].nsw == W)
    add("streamed row across a pass boundary", "G tile", "sw_park+1", lambda T, A: _spans(L.park_words + 1, L.park_words))
    add("streamed row across a pass boundary", "G tile, value codes", "sw_vc_park+1", lambda T, A: T[0].nsw == L.park_words + 1 and T[0].ntv > 0)
    add("e-mode capacity (emode_words)", "at", "emode_cap", lambda T, A: first_e(A).nsw == L.emode_words)
    add("e-mode capacity (emode_words)", "past", "emode_cap+1", lambda T, A: first_e(A).nsw == L.emode_words + 1)
    add("G tile without a pattern row (e-mode)", "planted", "g_no_pattern", lambda T, A: T[0].kind == "G" and T[0].npat == 0 and T[0].nsrows == T[0].nrows)
    add("values per tile <= tile_vals", "at", "vals_tilevals", lambda T, A: T[0].kind == "G" and T[0].nvals == L.tile_vals and T[0].ntv == L.tile_vals)
    add("values per tile <= tile_vals", "past (E tile)", "vals_tilevals+1", lambda T, A: T[0].kind == "GE" and T[0].nvals == L.tile_vals + 1)
    for v in ("", "_vc"):
        add("halo columns" + (", value codes" if v else ""), "flagged tiles last", "halo" + v,
            lambda T, A: T[0].halo and T[0].nruns > 0 and T[0].nsrows > 0 and [t.halo for t in A] == [True, True, False])
        add("one walk meets G, E, G with streamed rows in both orders" + (", value codes" if v else ""), "planted", "mix_walk" + v,
            lambda T, A: "".join("E" if t.kind == "E" else ("S" if t.nsw else "G") for t in A) == "GESEGSEG")
        add("more tiles than a grid of 16: several trips of the persistent loop" + (", value codes" if v else ""), "planted", "many_tiles" + v,
            lambda T, A: len(A) > 32 and {"E", "G"} <= {t.kind for t in A} and any(t.kind == "G" and t.nsw for t in A))
    for s in GOLDEN:
        add("assembled scene: T-junction rows across levels, the tiles an octree makes", "realistic", "golden_" + s,
            lambda T, A: any(t.kind == "G" and t.mixed_waves for t in A) and sum(t.nprow for t in A) > 0 and sum(t.nsrows for t in A) > 0)
    return E


@functools.lru_cache(None)
def edge_of(name):
    """the edges a case plants, for the messages of the tests"""
    return "; ".join(dict.fromkeys(f"{edge} [{side}]" for edge, side, case, _ in edges() if case == name))
