"""NumPy model of avs_check_octree / avs_prepass_check_octree (include/avs.h; kernels: csrc/avs_check.hip).

Eight rules over a label pyramid and its velocity index pyramid (reference: HDK_OctreeGrid::unitTest, oct.cpp:984-1304, and
octreeVelocityUnitTest, cpp:2896-2999).  Arrays are [z, y, x]; `labels[l]` has the shape of level 0 shifted right by l; `vidx[l][a]` has one more
entry along axis a (numpy dimension 2 - a).  A cell outside its lattice counts as INACTIVE.  A count is the number of lattice entries (rule 7:
ids) that break the rule at least once; the first violation is the smallest (rule, level, axis, linear index).  Label rules report axis 0,
rule 1 level 0, rule 7 level 0, axis 0 and ijk = (id, 0, 0).

The model is whole-array NumPy, written rule by rule from the text of the rules, not from the kernels: it shares no code with them.
tests/test_octree_check_model.py pins it with hand-derived counts on a 4^3 pyramid."""
from dataclasses import dataclass

import numpy as np

INACTIVE, ACTIVE, UP, DOWN = 0, 1, 2, 3
UNASSIGNED, SOLIDBOUNDARY, OUTSIDE = -1, -2, -3
CHECK_LABELS, CHECK_VELOCITY_INDICES = 1, 2
(RULE_LABEL_VALUE, RULE_COLUMN, RULE_UP, RULE_ACTIVE, RULE_INDEX_VALUE, RULE_FACE, RULE_SENTINEL, RULE_NUMBERING) = range(8)
RULES = 8
RULE_NAMES = ("LABEL_VALUE", "COLUMN", "UP", "ACTIVE", "INDEX_VALUE", "FACE", "SENTINEL", "NUMBERING")


@dataclass(frozen=True)
class Report:
    passed: int
    violations: tuple          # RULES counts
    first: tuple               # (rule, level, axis, i, j, k); six times -1 when passed

    def fired(self):
        return {r for r in range(RULES) if self.violations[r]}


def _check_shapes(labels):
    base = labels[0].shape
    for l, lab in enumerate(labels):
        assert lab.ndim == 3 and lab.shape == tuple(n >> l for n in base) and min(lab.shape) >= 1, (l, lab.shape, base)


def _shift(a, d, s, fill=0):
    """a[index + s along dimension d]; outside the lattice: fill.  Second result: the neighbour is inside the lattice."""
    out = np.full_like(a, fill)
    inside = np.zeros(a.shape, bool)
    src, dst = [slice(None)] * 3, [slice(None)] * 3
    if s > 0:
        dst[d], src[d] = slice(0, -1), slice(1, None)
    else:
        dst[d], src[d] = slice(1, None), slice(0, -1)
    out[tuple(dst)] = a[tuple(src)]
    inside[tuple(dst)] = True
    return out, inside


def _ancestor(hi, up, shape):
    """hi[index >> up] for every index of a lattice of `shape` (the ancestor `up` levels above every cell)"""
    iz, iy, ix = (np.arange(n) >> up for n in shape)
    return hi[iz[:, None, None], iy[None, :, None], ix[None, None, :]]


def _block_all(m, dims):
    """for every entry: all entries of its aligned block of two along each dimension of `dims` are set (entries beyond the lattice are not)"""
    shape = list(m.shape)
    pad = [(0, 0)] * 3
    for d in dims:
        pad[d] = (0, shape[d] & 1)
    p = np.pad(m, pad, constant_values=False)
    for d in dims:
        n = p.shape[d]
        view = np.moveaxis(p, d, 0).reshape((n // 2, 2) + tuple(np.moveaxis(p, d, 0).shape[1:]))
        both = view.all(axis=1)
        p = np.moveaxis(np.repeat(both, 2, axis=0), 0, d)
    return p[:shape[0], :shape[1], :shape[2]]


def label_value_violations(labels, l):
    return (labels[l] < 0) | (labels[l] > 3)


def column_violations(labels):
    L = len(labels)
    base = labels[0]
    bad = ~np.isin(base, (INACTIVE, ACTIVE, UP))          # DOWN (or no label at all) at level 0
    found = np.zeros(base.shape, bool)                    # INACTIVE columns: a DOWN was seen; UP columns: the ACTIVE was seen
    ina, act, up = base == INACTIVE, base == ACTIVE, base == UP
    for l in range(1, L):
        a = _ancestor(labels[l], l, base.shape)
        bad |= ina & ~((a == DOWN) | ((a == INACTIVE) & ~found))
        bad |= act & (a != DOWN)
        bad |= up & (((a == ACTIVE) & found) | ((a == UP) & found) | ((a == DOWN) & ~found) | ~np.isin(a, (ACTIVE, UP, DOWN)))
        found = np.where(ina, found | (a == DOWN), np.where(up, found | (a == ACTIVE), found))
    bad |= up & ~found
    return bad


def up_violations(labels, l):
    L = len(labels)
    lab = labels[l]
    up = lab == UP
    if l == L - 1:
        return up.copy()
    bad = up & ~_block_all(up, (0, 1, 2))
    for d in range(3):
        for s in (-1, 1):
            nb, inside = _shift(lab, d, s)
            bad |= up & inside & (nb != ACTIVE) & (nb != UP)
    return bad


def active_violations(labels, l):
    L = len(labels)
    lab = labels[l]
    act = lab == ACTIVE
    bad = np.zeros(lab.shape, bool)
    parent_active = _ancestor(labels[l + 1], 1, lab.shape) == ACTIVE if l < L - 1 else None
    for d in range(3):
        others = tuple(x for x in range(3) if x != d)
        for s in (-1, 1):
            nb, inside = _shift(lab, d, s)
            down = act & inside & (nb == DOWN)
            if l == 0:
                bad |= down
            else:
                fine = labels[l - 1] == ACTIVE
                sl = [slice(None)] * 3
                sl[d] = slice(0 if s > 0 else 1, None, 2)        # the children's plane that faces this cell
                plane = fine[tuple(sl)]
                sub = list(others)                               # 2 x 2 children of every cell of the plane
                four = _block_all(plane, sub)
                take = [slice(None)] * 3
                for o in others:
                    take[o] = slice(0, None, 2)
                four = four[tuple(take)]                         # one entry per level-l cell: its four facing children are ACTIVE
                assert four.shape == lab.shape
                ok, _ = _shift(four, d, s, fill=False)
                bad |= down & ~ok
            upn = act & inside & (nb == UP)
            if l == L - 1:
                bad |= upn
            else:
                ok, _ = _shift(parent_active, d, s, fill=False)
                bad |= upn & ~ok
    return bad


def index_value_violations(v, n_velocity):
    return (v < OUTSIDE) | (v >= n_velocity)


def face_violations(labels, l, a, v):
    L = len(labels)
    lab = labels[l]
    d = 2 - a
    assert v.shape == tuple(n + (1 if x == d else 0) for x, n in enumerate(lab.shape)), (v.shape, lab.shape, a)

    def sides(cell):
        back = np.zeros(v.shape, cell.dtype)
        fwd = np.zeros(v.shape, cell.dtype)
        sb, sf = [slice(None)] * 3, [slice(None)] * 3
        sb[d], sf[d] = slice(1, None), slice(0, -1)
        back[tuple(sb)] = cell
        fwd[tuple(sf)] = cell
        return back, fwd

    b, f = sides(lab)
    ok = (b == ACTIVE) & (f == ACTIVE)
    if l < L - 1:
        pb, pf = sides(_ancestor(labels[l + 1], 1, lab.shape) == ACTIVE)
        ok |= (b == ACTIVE) & (f == UP) & pf
        ok |= (b == UP) & (f == ACTIVE) & pb
    return (v >= 0) & ~ok


def sentinel_violations(l, v):
    if l == 0:
        return np.zeros(v.shape, bool)
    return (v == OUTSIDE) | (v == SOLIDBOUNDARY)


def numbering_violations(vidx, n_velocity):
    counts = np.zeros(n_velocity, np.int64)
    for per_level in vidx:
        for v in per_level:
            ids = v[(v >= 0) & (v < n_velocity)]
            counts += np.bincount(ids, minlength=n_velocity)
    return counts != 1


def _first(mask):
    flat = np.flatnonzero(mask.ravel())
    if not len(flat):
        return None
    if mask.ndim == 1:
        return (int(flat[0]), 0, 0)
    k, j, i = np.unravel_index(int(flat[0]), mask.shape)
    return (int(i), int(j), int(k))


def check(labels, vidx=None, n_velocity=None, what=CHECK_LABELS | CHECK_VELOCITY_INDICES):
    """the report of avs_check_octree for these lattices"""
    labels = [np.asarray(a, np.int8) for a in labels]
    L = len(labels)
    counts = [0] * RULES
    first = None

    def record(rule, level, axis, mask):
        nonlocal first
        c = int(mask.sum())
        counts[rule] += c
        if c and (first is None or (rule, level, axis) < first[:3]):
            first = (rule, level, axis) + _first(mask)

    if L == 0 or what == 0:
        return Report(1, tuple(counts), (-1,) * 6)
    _check_shapes(labels)
    if what & CHECK_LABELS:
        for l in range(L):
            record(RULE_LABEL_VALUE, l, 0, label_value_violations(labels, l))
        record(RULE_COLUMN, 0, 0, column_violations(labels))
        for l in range(L):
            record(RULE_UP, l, 0, up_violations(labels, l))
        for l in range(L):
            record(RULE_ACTIVE, l, 0, active_violations(labels, l))
    if what & CHECK_VELOCITY_INDICES:
        vidx = [[np.asarray(v, np.int32) for v in per_level] for per_level in vidx]
        n_velocity = int(n_velocity)
        for l in range(L):
            for a in range(3):
                record(RULE_INDEX_VALUE, l, a, index_value_violations(vidx[l][a], n_velocity))
        for l in range(L):
            for a in range(3):
                record(RULE_FACE, l, a, face_violations(labels, l, a, vidx[l][a]))
        for l in range(L):
            for a in range(3):
                record(RULE_SENTINEL, l, a, sentinel_violations(l, vidx[l][a]))
        record(RULE_NUMBERING, 0, 0, numbering_violations(vidx, n_velocity))
    passed = int(not any(counts))
    return Report(passed, tuple(counts), (-1,) * 6 if passed else first)


def reciprocity_failures(labels):
    """The reciprocity loop of activeUnitTest (oct.cpp:1250-1269), which the checker does not run: for every ACTIVE cell C and every cell
    getFaceAdjacentCells (oct.cpp:923-978) lists across one of its faces, the list taken from that cell in the opposite direction must
    hold C.  Returns the number of (cell, face) pairs for which it does not."""
    labels = [np.asarray(a, np.int8) for a in labels]
    L = len(labels)
    _check_shapes(labels)
    fails = 0
    for l in range(L):
        lab = labels[l]
        act = lab == ACTIVE
        for d in range(3):
            others = [x for x in range(3) if x != d]
            for s in (-1, 1):
                nb, inside = _shift(lab, d, s)
                # neighbour ACTIVE: it lists C, because C is ACTIVE.  Neighbour UP: its parent P is listed; P's list holds C when P's
                # neighbour towards C is DOWN, is C's parent, and C is ACTIVE on the facing plane (it is: C touches the UP cell)
                c = np.argwhere(act & inside & (nb == UP))
                if len(c):
                    if l == L - 1:
                        fails += len(c)
                    else:
                        n = c.copy()
                        n[:, d] += s
                        pc, pn = c >> 1, n >> 1
                        plab = labels[l + 1][pc[:, 0], pc[:, 1], pc[:, 2]]
                        fails += int((~((pc[:, d] == pn[:, d] - s) & (plab == DOWN))).sum())
                # neighbour DOWN: its ACTIVE facing children are listed; each lists C when its neighbour towards C (a child of C) is UP
                c = np.argwhere(act & inside & (nb == DOWN))
                if len(c) and l > 0:
                    fine = labels[l - 1]
                    for o0 in (0, 1):
                        for o1 in (0, 1):
                            ch = c.copy()
                            ch[:, d] += s
                            ch *= 2
                            ch[:, d] += 0 if s > 0 else 1
                            ch[:, others[0]] += o0
                            ch[:, others[1]] += o1
                            listed = fine[ch[:, 0], ch[:, 1], ch[:, 2]] == ACTIVE
                            back = ch.copy()
                            back[:, d] -= s
                            fails += int((listed & (fine[back[:, 0], back[:, 1], back[:, 2]] != UP)).sum())
    return fails
