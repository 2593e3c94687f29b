"""NumPy model of avs_check_stress_indices / avs_prepass_check_stress_indices (include/avs.h; kernels: csrc/avs_stress_check.hip).

Nine rules over the edge and centre stress index pyramids (reference: edgeStressUnitTest and centerStresUnitTest, cpp:3001-3298).  Arrays
are [z, y, x]; `labels[l]` has the shape of level 0 shifted right by l; `vidx[l][f]` has one more entry along axis f (numpy dimension
2 - f); `eidx[l][a]` one more along the two axes other than a; `cidx[l]` the shape of the labels.  A cell outside its lattice reads as
INACTIVE, an index outside its lattice as UNASSIGNED.  A count is the number of lattice entries (rules 3 and 8: ids) that break the rule at
least once; the first violation is the smallest (rule, level, axis, linear index).  Centre rules report axis 0, the numbering rules level
0, axis 0 and ijk = (id, 0, 0).

The model gathers, for all entries that carry an id at once, the neighbours the rule names: whole-array NumPy over coordinate lists, written
rule by rule from the text of the rules, not from the kernels.  `check_slow` restates the same rules entry by entry in plain Python loops;
tests/test_stress_check_model.py holds the two against each other.  BRANCHES counts how often each branch of rules 1, 2, 6 and 7 was
taken, so that a test can tell that a rule did not pass vacuously."""
from dataclasses import dataclass

import numpy as np

INACTIVE, ACTIVE, UP, DOWN = 0, 1, 2, 3
UNASSIGNED, SOLIDBOUNDARY, OUTSIDE = -1, -2, -3
CHECK_EDGE_INDICES, CHECK_CENTER_INDICES = 1, 2
(RULE_EDGE_VALUE, RULE_EDGE_CELLS, RULE_EDGE_FACES, RULE_EDGE_NUMBERING, RULE_CENTER_VALUE, RULE_CENTER_LABEL, RULE_CENTER_FACES,
 RULE_CENTER_EDGES, RULE_CENTER_NUMBERING) = range(9)
RULES = 9
RULE_NAMES = ("EDGE_VALUE", "EDGE_CELLS", "EDGE_FACES", "EDGE_NUMBERING", "CENTER_VALUE", "CENTER_LABEL", "CENTER_FACES", "CENTER_EDGES",
              "CENTER_NUMBERING")
# the branches a clean pyramid can take (the others report a violation wherever they are reached)
BRANCHES = ("cells_inside", "cells_outside", "edge_face_id", "edge_face_skipped", "edge_face_sentinel_l0", "edge_face_unassigned_odd",
            "edge_face_unassigned_even", "center_face_border", "center_face_id", "center_face_sentinel_l0", "center_face_children", "center_edge_assigned",
            "center_edge_children_l1", "center_edge_children_l2", "center_edge_grandchildren")


@dataclass(frozen=True)
class Report:
    passed: int
    violations: tuple          # RULES counts
    first: tuple               # (rule, level, axis, i, j, k); six times -1 when passed
    active_edges: int
    active_centers: int

    def fired(self):
        return {r for r in range(RULES) if self.violations[r]}


def passed_report(active_edges=0, active_centers=0):
    return Report(1, (0,) * RULES, (-1,) * 6, active_edges, active_centers)


def _others(a):
    return (a + 1) % 3, (a + 2) % 3


def _unit(a):
    e = np.zeros(3, np.int64)
    e[a] = 1
    return e


def _read(arr, xyz, fill):
    """arr[z, y, x] at the coordinates xyz (N, 3: x, y, z); outside the lattice: fill"""
    nz, ny, nx = arr.shape
    inside = (xyz >= 0).all(axis=1) & (xyz[:, 0] < nx) & (xyz[:, 1] < ny) & (xyz[:, 2] < nz)
    out = np.full(len(xyz), fill, np.int64)
    q = xyz[inside]
    out[inside] = arr[q[:, 2], q[:, 1], q[:, 0]]
    return out, inside


def _entries(v):
    """coordinates (N, 3: x, y, z) of the entries with a value >= 0, in lattice order"""
    return np.argwhere(v >= 0)[:, ::-1].astype(np.int64)


def _mask(v, xyz, bad):
    m = np.zeros(v.shape, bool)
    q = xyz[bad]
    m[q[:, 2], q[:, 1], q[:, 0]] = True
    return m


def value_violations(v, n):
    return ~((v == UNASSIGNED) | (v == OUTSIDE) | ((v >= 0) & (v < n)))


def edge_cells_violations(labels, l, a, v, took=None):
    """the reference's walk (cpp:3038-3044): e - 1_b - 1_c, e - 1_c, e - 1_b, e, up to the first cell outside the lattice"""
    b, c = _others(a)
    e = _entries(v)
    bad = np.zeros(len(e), bool)
    walking = np.ones(len(e), bool)
    for sb, sc in ((1, 1), (0, 1), (1, 0), (0, 0)):
        cell = e - sb * _unit(b) - sc * _unit(c)
        lab, inside = _read(labels[l], cell, INACTIVE)
        walking &= inside
        bad |= walking & (lab != ACTIVE) & (lab != UP)
        if took is not None:
            took["cells_inside"] += int(walking.sum())
            took["cells_outside"] += int((~walking).sum())
    return _mask(v, e, bad)


def edge_faces_violations(labels, vidx, l, a, v, took=None):
    L = len(labels)
    b, c = _others(a)
    e = _entries(v)
    bad = np.zeros(len(e), bool)
    examined = e[:, b] != labels[l].shape[2 - b]          # (on the upper border plane of b the walk of rule 1 ends after one cell)
    for f, o in ((b, c), (c, b)):
        n_o, n_f = labels[l].shape[2 - o], labels[l].shape[2 - f]
        for d in (0, 1):
            face = e - d * _unit(o)
            look = examined & (face[:, o] >= 0) & (face[:, o] < n_o) & (face[:, f] != 0) & (face[:, f] != n_f)   # (no border plane)
            w, _ = _read(vidx[l][f], face, UNASSIGNED)
            sentinel = look & ((w == SOLIDBOUNDARY) | (w == OUTSIDE))
            unassigned = look & (w == UNASSIGNED)
            odd = unassigned & (e[:, f] % 2 != 0)
            even = unassigned & (e[:, f] % 2 == 0)
            bad |= look & (w < OUTSIDE)
            if l != 0:
                bad |= sentinel
            if l == L - 1:
                bad |= unassigned
            else:
                parent, _ = _read(labels[l + 1], face >> 1, INACTIVE)
                bad |= odd & (parent != ACTIVE)
                coarse, _ = _read(vidx[l + 1][f], face >> 1, UNASSIGNED)
                bad |= even & (coarse == UNASSIGNED)
            if took is not None:
                took["edge_face_skipped"] += int((~look).sum())
                took["edge_face_id"] += int((look & (w >= 0)).sum())
                took["edge_face_sentinel_l0"] += int(sentinel.sum()) if l == 0 else 0
                took["edge_face_unassigned_odd"] += int(odd.sum()) if l < L - 1 else 0
                took["edge_face_unassigned_even"] += int(even.sum()) if l < L - 1 else 0
    return _mask(v, e, bad)


def center_label_violations(labels, l, v):
    return (v >= 0) & (labels[l] != ACTIVE)


def center_faces_violations(vidx, l, v, took=None):
    e = _entries(v)
    bad = np.zeros(len(e), bool)
    for a in range(3):
        b, c = _others(a)
        for d in (0, 1):
            face = e + d * _unit(a)
            look = (face[:, a] != 0) & (face[:, a] != v.shape[2 - a])      # (not on a border plane of the face lattice)
            w, _ = _read(vidx[l][a], face, UNASSIGNED)
            unassigned = look & (w == UNASSIGNED)
            sentinel = look & ((w == OUTSIDE) | (w == SOLIDBOUNDARY))
            bad |= look & (w < OUTSIDE)
            if l == 0:
                bad |= unassigned
            else:
                bad |= sentinel
                for q in range(4):
                    child, _ = _read(vidx[l - 1][a], 2 * face + (q & 1) * _unit(b) + (q >> 1) * _unit(c), UNASSIGNED)
                    bad |= unassigned & (child < 0)
            if took is not None:
                took["center_face_border"] += int((~look).sum())
                took["center_face_id"] += int((look & (w >= 0)).sum())
                took["center_face_sentinel_l0"] += int(sentinel.sum()) if l == 0 else 0
                took["center_face_children"] += int(unassigned.sum()) if l > 0 else 0
    return _mask(v, e, bad)


def center_edges_violations(eidx, l, v, took=None):
    e = _entries(v)
    bad = np.zeros(len(e), bool)
    for a in range(3):
        b, c = _others(a)
        for q in range(4):
            edge = e + (q & 1) * _unit(b) + (q >> 1) * _unit(c)
            w, _ = _read(eidx[l][a], edge, UNASSIGNED)
            unassigned = w == UNASSIGNED
            if took is not None:
                took["center_edge_assigned"] += int((~unassigned).sum())
                took["center_edge_children_l1"] += int(unassigned.sum()) if l == 1 else 0
                took["center_edge_children_l2"] += int(unassigned.sum()) if l >= 2 else 0
            if l == 0:
                bad |= unassigned
                continue
            for h in (0, 1):
                child = 2 * edge + h * _unit(a)
                cw, _ = _read(eidx[l - 1][a], child, UNASSIGNED)
                down = unassigned & (cw < 0)
                if l == 1:
                    bad |= down
                    continue
                if took is not None:
                    took["center_edge_grandchildren"] += int(down.sum())
                for g in (0, 1):
                    gw, _ = _read(eidx[l - 2][a], 2 * child + g * _unit(a), UNASSIGNED)
                    bad |= down & (gw < 0)
    return _mask(v, e, bad)


def numbering_violations(lattices, n):
    counts = np.zeros(n, np.int64)
    for v in lattices:
        ids = v[(v >= 0) & (v < n)]
        counts += np.bincount(ids, minlength=n)
    return counts != 1


def _first(mask):
    flat = np.flatnonzero(mask.ravel())
    if mask.ndim == 1:
        return (int(flat[0]), 0, 0)
    k, j, i = np.unravel_index(int(flat[0]), mask.shape)
    return (int(i), int(j), int(k))


def _check_shapes(labels, vidx, eidx, cidx):
    base = labels[0].shape
    for l, lab in enumerate(labels):
        cell = tuple(n >> l for n in base)
        assert lab.shape == cell and min(cell) >= 1, (l, lab.shape, base)
        for a in range(3):
            assert vidx[l][a].shape == tuple(n + (1 if 2 - d == a else 0) for d, n in enumerate(cell)), (l, a, vidx[l][a].shape)
            assert eidx[l][a].shape == tuple(n + (1 if 2 - d != a else 0) for d, n in enumerate(cell)), (l, a, eidx[l][a].shape)
        assert cidx is None or cidx[l].shape == cell


def check(labels, vidx, eidx, cidx, n_edge, n_center, what=CHECK_EDGE_INDICES | CHECK_CENTER_INDICES, took=None):
    """the report of avs_check_stress_indices for these lattices; took: a dict that receives the BRANCHES counters"""
    L = len(labels)
    counts = [0] * RULES
    first = None
    if took is not None:
        for name in BRANCHES:
            took.setdefault(name, 0)

    def record(rule, level, axis, mask):
        nonlocal first
        c = int(mask.sum())
        counts[rule] += c
        if c and (first is None or (rule, level, axis) < first[:3]):
            first = (rule, level, axis) + _first(mask)

    if L == 0 or what == 0:
        return passed_report()
    labels = [np.asarray(a, np.int8) for a in labels]
    vidx = [[np.asarray(v, np.int32) for v in per_level] for per_level in vidx]
    eidx = [[np.asarray(v, np.int32) for v in per_level] for per_level in eidx]
    centers = bool(what & CHECK_CENTER_INDICES)
    cidx = [np.asarray(v, np.int32) for v in cidx] if centers else None
    _check_shapes(labels, vidx, eidx, cidx)
    active_edges = active_centers = 0
    if what & CHECK_EDGE_INDICES:
        n_edge = int(n_edge)
        active_edges = sum(int((v >= 0).sum()) for per_level in eidx for v in per_level)
        for l in range(L):
            for a in range(3):
                record(RULE_EDGE_VALUE, l, a, value_violations(eidx[l][a], n_edge))
        for l in range(L):
            for a in range(3):
                record(RULE_EDGE_CELLS, l, a, edge_cells_violations(labels, l, a, eidx[l][a], took))
        for l in range(L):
            for a in range(3):
                record(RULE_EDGE_FACES, l, a, edge_faces_violations(labels, vidx, l, a, eidx[l][a], took))
        record(RULE_EDGE_NUMBERING, 0, 0, numbering_violations([v for per_level in eidx for v in per_level], n_edge))
    if centers:
        n_center = int(n_center)
        active_centers = sum(int((v >= 0).sum()) for v in cidx)
        for l in range(L):
            record(RULE_CENTER_VALUE, l, 0, value_violations(cidx[l], n_center))
        for l in range(L):
            record(RULE_CENTER_LABEL, l, 0, center_label_violations(labels, l, cidx[l]))
        for l in range(L):
            record(RULE_CENTER_FACES, l, 0, center_faces_violations(vidx, l, cidx[l], took))
        for l in range(L):
            record(RULE_CENTER_EDGES, l, 0, center_edges_violations(eidx, l, cidx[l], took))
        record(RULE_CENTER_NUMBERING, 0, 0, numbering_violations(cidx, n_center))
    passed = int(not any(counts))
    return Report(passed, tuple(counts), (-1,) * 6 if passed else first, active_edges, active_centers)


# ---- the same rules, one entry at a time ------------------------------------------------------------------------------------------------
def check_slow(labels, vidx, eidx, cidx, n_edge, n_center, what=CHECK_EDGE_INDICES | CHECK_CENTER_INDICES):
    """check() in plain Python loops over the entries: slow, and shares nothing with check() but the constants"""
    L = len(labels)
    if L == 0 or what == 0:
        return passed_report()
    res = labels[0].shape[::-1]                          # level-0 cells per axis x, y, z

    def cells(l):
        return [n >> l for n in res]

    def label(l, p):
        n = cells(l)
        return int(labels[l][p[2], p[1], p[0]]) if all(0 <= p[d] < n[d] for d in range(3)) else INACTIVE

    def velocity(l, f, p):
        n = cells(l)
        n[f] += 1
        return int(vidx[l][f][p[2], p[1], p[0]]) if all(0 <= p[d] < n[d] for d in range(3)) else UNASSIGNED

    def edge(l, a, p):
        n = [m + (1 if d != a else 0) for d, m in enumerate(cells(l))]
        return int(eidx[l][a][p[2], p[1], p[0]]) if all(0 <= p[d] < n[d] for d in range(3)) else UNASSIGNED

    def moved(p, axis, by):
        q = list(p)
        q[axis] += by
        return q

    counts = [0] * RULES
    keys = []
    active = [0, 0]

    def violation(rule, l, a, p, shape):
        counts[rule] += 1
        keys.append((rule, l, a, p[0] + shape[2] * (p[1] + shape[1] * p[2]), tuple(p)))

    def value_ok(v, n):
        return v in (UNASSIGNED, OUTSIDE) or 0 <= v < n

    if what & CHECK_EDGE_INDICES:
        occ = [0] * n_edge
        for l in range(L):
            for a in range(3):
                lat = eidx[l][a]
                b, c = (a + 1) % 3, (a + 2) % 3
                for k, j, i in np.argwhere(lat != UNASSIGNED):       # (an UNASSIGNED entry breaks no rule and carries no id)
                    v, p = int(lat[k, j, i]), [int(i), int(j), int(k)]
                    if not value_ok(v, n_edge):
                        violation(RULE_EDGE_VALUE, l, a, p, lat.shape)
                    if v < 0:
                        continue
                    active[0] += 1
                    if v < n_edge:
                        occ[v] += 1
                    n = cells(l)
                    bad = False
                    for sb, sc in ((1, 1), (0, 1), (1, 0), (0, 0)):
                        cell = moved(moved(p, b, -sb), c, -sc)
                        if not all(0 <= cell[d] < n[d] for d in range(3)):
                            break
                        if label(l, cell) not in (ACTIVE, UP):
                            bad = True
                    if bad:
                        violation(RULE_EDGE_CELLS, l, a, p, lat.shape)
                    bad = False
                    for f in (b, c):
                        o = 3 - f - a
                        for d in (0, 1):
                            face = moved(p, o, -d)
                            if p[b] == n[b] or face[o] < 0 or face[o] >= n[o] or face[f] in (0, n[f]):
                                continue
                            w = velocity(l, f, face)
                            if w >= 0:
                                continue
                            if w in (SOLIDBOUNDARY, OUTSIDE):
                                bad = bad or l != 0
                            elif w == UNASSIGNED:
                                up = [x >> 1 for x in face]
                                if l == L - 1:
                                    bad = True
                                elif p[f] % 2:
                                    bad = bad or label(l + 1, up) != ACTIVE
                                else:
                                    bad = bad or velocity(l + 1, f, up) == UNASSIGNED
                            else:
                                bad = True
                    if bad:
                        violation(RULE_EDGE_FACES, l, a, p, lat.shape)
        for i, times in enumerate(occ):
            if times != 1:
                counts[RULE_EDGE_NUMBERING] += 1
                keys.append((RULE_EDGE_NUMBERING, 0, 0, i, (i, 0, 0)))
    if what & CHECK_CENTER_INDICES:
        occ = [0] * n_center
        for l in range(L):
            lat = cidx[l]
            for k, j, i in np.argwhere(lat != UNASSIGNED):
                v, p = int(lat[k, j, i]), [int(i), int(j), int(k)]
                if not value_ok(v, n_center):
                    violation(RULE_CENTER_VALUE, l, 0, p, lat.shape)
                if v < 0:
                    continue
                active[1] += 1
                if v < n_center:
                    occ[v] += 1
                if label(l, p) != ACTIVE:
                    violation(RULE_CENTER_LABEL, l, 0, p, lat.shape)
                bad = False
                for a in range(3):
                    b, c = (a + 1) % 3, (a + 2) % 3
                    for d in (0, 1):
                        face = moved(p, a, d)
                        if face[a] in (0, cells(l)[a]):
                            continue
                        w = velocity(l, a, face)
                        if w == UNASSIGNED:
                            if l == 0:
                                bad = True
                                continue
                            for sb in (0, 1):
                                for sc in (0, 1):
                                    child = moved(moved([2 * x for x in face], b, sb), c, sc)
                                    bad = bad or velocity(l - 1, a, child) < 0
                        elif w in (OUTSIDE, SOLIDBOUNDARY):
                            bad = bad or l != 0
                        elif w < 0:
                            bad = True
                if bad:
                    violation(RULE_CENTER_FACES, l, 0, p, lat.shape)
                bad = False
                for a in range(3):
                    b, c = (a + 1) % 3, (a + 2) % 3
                    for sb in (0, 1):
                        for sc in (0, 1):
                            e = moved(moved(p, b, sb), c, sc)
                            if edge(l, a, e) != UNASSIGNED:
                                continue
                            if l == 0:
                                bad = True
                                continue
                            for h in (0, 1):
                                child = moved([2 * x for x in e], a, h)
                                if edge(l - 1, a, child) >= 0:
                                    continue
                                if l == 1:
                                    bad = True
                                    continue
                                for g in (0, 1):
                                    bad = bad or edge(l - 2, a, moved([2 * x for x in child], a, g)) < 0
                if bad:
                    violation(RULE_CENTER_EDGES, l, 0, p, lat.shape)
        for i, times in enumerate(occ):
            if times != 1:
                counts[RULE_CENTER_NUMBERING] += 1
                keys.append((RULE_CENTER_NUMBERING, 0, 0, i, (i, 0, 0)))
    if not keys:
        return passed_report(*active)
    rule, l, a, _, p = min(keys)
    return Report(0, tuple(counts), (rule, l, a) + p, active[0], active[1])
