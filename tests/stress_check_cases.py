"""Pyramids for the stress index check tests (test_stress_check_model.py, test_gpu_stress_check.py): the oracle's pre-pass on the scenes the
rules were validated on, and named mutations of a pyramid.  A Pyramid holds labels[l] int8 [z, y, x], vidx[l][a] / eidx[l][a] int32 on the
face / edge lattice of axis a, cidx[l] int32 on the cell lattice, and the two counts."""
import functools
from dataclasses import dataclass, field

import numpy as np

import stress_check_model as M
from adaptiveviscositysolver_amd import scenes
from oracle import oracle as O
from util import oracle_for_scene


@dataclass
class Pyramid:
    labels: list
    vidx: list
    eidx: list
    cidx: list
    n_edge: int
    n_center: int
    edits: list = field(default_factory=list)        # (kind, level, axis) of every lattice a mutation wrote to

    @property
    def levels(self):
        return len(self.labels)

    def lattice(self, kind, l, a=0):
        return {"labels": lambda: self.labels[l], "vidx": lambda: self.vidx[l][a], "eidx": lambda: self.eidx[l][a], "cidx": lambda: self.cidx[l]}[kind]()

    def put(self, kind, l, a, at, value):
        """one entry; at: (k, j, i)"""
        self.lattice(kind, l, a)[tuple(at)] = value
        if (kind, l, a) not in self.edits:
            self.edits.append((kind, l, a))

    def args(self):
        return self.labels, self.vidx, self.eidx, self.cidx, self.n_edge, self.n_center

    def copy(self):
        return Pyramid([a.copy() for a in self.labels], [[v.copy() for v in lv] for lv in self.vidx], [[v.copy() for v in lv] for lv in self.eidx],
                       [v.copy() for v in self.cidx], self.n_edge, self.n_center)


# ---- oracle scenes ---------------------------------------------------------------------------------------------------------------------
def leaving_box_scene():
    from test_oracle_known_answers import leaving_box_scene as make
    return make()


SCENES = {
    "sphere16_L2": lambda: scenes.sphere(16, 2),
    "sphere32_L3": lambda: scenes.sphere(32, 3),
    "sphere64_L4": lambda: scenes.sphere(64, 4),
    "tank32_L3": lambda: scenes.tank(32, 3),
    "beam64_L3_wall": lambda: scenes.fat_beam(64, 3, wall=True),
    "beam64x32x16_L2_wall": lambda: scenes.fat_beam(32, 2, wall=True, res=(64, 32, 16)),     # three different extents
    "leaving_box": leaving_box_scene,
}
NON_CUBIC = "beam64x32x16_L2_wall"
MUTATED_SCENES = ("sphere16_L2", "sphere32_L3")      # the two smallest


@functools.lru_cache(maxsize=None)
def _oracle_pyramid(name):
    sc = SCENES[name]()
    o = oracle_for_scene(sc)
    o.prepass()
    L = o.levels
    pyr = Pyramid([o.labels(l) for l in range(L)], [[o.index(O.I_VELOCITY, l, a) for a in range(3)] for l in range(L)],
                  [[o.index(O.I_EDGE, l, a) for a in range(3)] for l in range(L)], [o.index(O.I_CENTER, l) for l in range(L)],
                  o.count(O.I_EDGE), o.count(O.I_CENTER))
    return sc, pyr


def oracle_pyramid(name):
    """the oracle's pre-pass as a Pyramid: a fresh copy, computed once per scene"""
    return _oracle_pyramid(name)[1].copy()


def scene(name):
    return _oracle_pyramid(name)[0]


# ---- mutations -------------------------------------------------------------------------------------------------------------------------
# each takes a Pyramid, edits it in place through Pyramid.put, and returns the rules that must fire; a mutation that finds no site in
# the pyramid (a rule about level l >= 2 in a two-level pyramid) returns None and is left out for that scene
def _xyz(at):
    return np.asarray(at[::-1], np.int64)


def _kji(p):
    return tuple(int(x) for x in p[::-1])


def _unit(a):
    return M._unit(a)


def _inside(lat, p):
    return all(0 <= int(p[d]) < lat.shape[2 - d] for d in range(3))


def _active(v, which):
    """entry number which * (count - 1) of the entries that carry an id, in lattice order; (k, j, i)"""
    at = np.argwhere(v >= 0)
    return tuple(int(x) for x in at[int(round(which * (len(at) - 1)))]) if len(at) else None


def _top_level(pyr, lattice_of):
    """the highest level at which a lattice of this kind carries an id"""
    return max(l for l in range(pyr.levels) if any((v >= 0).any() for v in lattice_of(l)))


def m_value(kind, where, value, top=False):
    """rule 0 / 4: the first, the last or a middle entry of a lattice becomes SOLIDBOUNDARY, n or n + 5"""
    def mutate(pyr):
        rule = M.RULE_EDGE_VALUE if kind == "eidx" else M.RULE_CENTER_VALUE
        n = pyr.n_edge if kind == "eidx" else pyr.n_center
        a = 2 if kind == "eidx" and top else 0
        l = _top_level(pyr, (lambda l: pyr.eidx[l]) if kind == "eidx" else (lambda l: [pyr.cidx[l]])) if top else 0
        lat = pyr.lattice(kind, l, a)
        at = {"first": (0, 0, 0), "last": tuple(s - 1 for s in lat.shape), "middle": _active(lat, 0.5)}[where]
        pyr.put(kind, l, a, at, {"sb": M.SOLIDBOUNDARY, "n": n, "n5": n + 5}[value])
        return {rule}
    return mutate


def _edge_sites(pyr, levels, want):
    """(l, a, edge xyz, f, face xyz) of the first active edge, walking the levels given, one of whose four faces satisfies want(l, f, e, face, w)"""
    for l in levels:
        for a in range(3):
            b, c = M._others(a)
            for k, j, i in np.argwhere(pyr.eidx[l][a] >= 0):
                e = np.asarray((i, j, k), np.int64)
                for f, o in ((b, c), (c, b)):
                    for d in (0, 1):
                        face = e - d * _unit(o)
                        if face[o] < 0 or face[o] >= pyr.labels[l].shape[2 - o]:
                            continue
                        if want(l, f, e, face, int(pyr.vidx[l][f][_kji(face)])):
                            return l, a, e, f, face
    return None


def m_edge_cell_down(top):
    """rule 1: a cell around an active edge becomes DOWN"""
    def mutate(pyr):
        l = _top_level(pyr, lambda l: pyr.eidx[l]) if top else 0
        at = _active(pyr.eidx[l][0], 0.5)
        e = _xyz(at)
        cell = e - _unit(1) - _unit(2)
        if not _inside(pyr.labels[l], cell):
            cell = e
        pyr.put("labels", l, 0, _kji(cell), M.DOWN)
        return {M.RULE_EDGE_CELLS}
    return mutate


def m_edge_id_at(where):
    """rule 1 at the corners of the lattice: the first / last entry of the z edges of level 0, in the far field, gets id 0.  One of the four
    cells is inside the lattice there.  At the last entry it is the cell the walk starts with (INACTIVE: rule 1 fires); at the first
    entry the walk starts outside the lattice and ends there, as the reference's does: only the numbering notices the id"""
    def mutate(pyr):
        lat = pyr.eidx[0][2]
        at = (0, 0, 0) if where == "first" else tuple(s - 1 for s in lat.shape)
        assert lat[at] < 0
        pyr.put("eidx", 0, 2, at, 0)
        return {M.RULE_EDGE_NUMBERING} | ({M.RULE_EDGE_CELLS} if where == "last" else set())
    return mutate


def m_edge_face_sentinel(pyr):
    """rule 2: a face of an active level-1 edge becomes SOLIDBOUNDARY"""
    site = _edge_sites(pyr, [1], lambda l, f, e, face, w: w >= 0)
    if site is None:
        return None
    l, a, e, f, face = site
    pyr.put("vidx", l, f, _kji(face), M.SOLIDBOUNDARY)
    return {M.RULE_EDGE_FACES}


def m_edge_face_odd(pyr):
    """rule 2: the coarse cell that holds a T-junction face of an active edge stops being ACTIVE"""
    site = _edge_sites(pyr, range(pyr.levels - 1), lambda l, f, e, face, w: w == M.UNASSIGNED and e[f] % 2 == 1)
    if site is None:
        return None
    l, a, e, f, face = site
    pyr.put("labels", l + 1, 0, _kji(face >> 1), M.DOWN)
    return {M.RULE_EDGE_FACES}


def m_edge_face_even(pyr):
    """rule 2: the parent face of an UNASSIGNED face of an active edge loses its id"""
    site = _edge_sites(pyr, range(pyr.levels - 1), lambda l, f, e, face, w: w == M.UNASSIGNED and e[f] % 2 == 0)
    if site is None:
        return None
    l, a, e, f, face = site
    pyr.put("vidx", l + 1, f, _kji(face >> 1), M.UNASSIGNED)
    return {M.RULE_EDGE_FACES}


def m_edge_face_top_unassigned(pyr):
    """rule 2 at the highest level that has edges: no level above can explain an UNASSIGNED face ... unless it is not the last level"""
    l = pyr.levels - 1
    site = _edge_sites(pyr, [l], lambda l, f, e, face, w: w >= 0)
    if site is None:
        return None
    l, a, e, f, face = site
    pyr.put("vidx", l, f, _kji(face), M.UNASSIGNED)
    return {M.RULE_EDGE_FACES}


def m_edge_face_other_negative(pyr):
    """rule 2: a face of an active edge holds -4, which is no sentinel"""
    l, a, e, f, face = _edge_sites(pyr, [0], lambda l, f, e, face, w: w >= 0)
    pyr.put("vidx", l, f, _kji(face), -4)
    return {M.RULE_EDGE_FACES}


def m_id_repeated(kind):
    def mutate(pyr):
        v = pyr.lattice(kind, 0, 0)
        a, b = _active(v, 0.25), _active(v, 0.75)
        assert v[a] != v[b]
        pyr.put(kind, 0, 0, b, int(v[a]))
        return {M.RULE_EDGE_NUMBERING if kind == "eidx" else M.RULE_CENTER_NUMBERING}
    return mutate


def m_id_missing(kind):
    def mutate(pyr):
        v = pyr.lattice(kind, 0, 1 if kind == "eidx" else 0)
        pyr.put(kind, 0, 1 if kind == "eidx" else 0, _active(v, 0.5), M.UNASSIGNED)
        return {M.RULE_EDGE_NUMBERING if kind == "eidx" else M.RULE_CENTER_NUMBERING}
    return mutate


def m_center_label(top):
    """rule 5: the cell under an active centre becomes UP"""
    def mutate(pyr):
        l = _top_level(pyr, lambda l: [pyr.cidx[l]]) if top else 0
        pyr.put("labels", l, 0, _active(pyr.cidx[l], 0.5), M.UP)
        return {M.RULE_CENTER_LABEL}
    return mutate


def _center_sites(pyr, levels, want, which=0.0):
    """(l, cell xyz, a, face xyz) of an active centre, walking the levels given, one of whose six faces satisfies want(l, a, face, w)"""
    for l in levels:
        found = []
        for k, j, i in np.argwhere(pyr.cidx[l] >= 0):
            cell = np.asarray((i, j, k), np.int64)
            for a in range(3):
                for d in (0, 1):
                    face = cell + d * _unit(a)
                    if want(l, a, face, int(pyr.vidx[l][a][_kji(face)])):
                        found.append((l, cell, a, face))
        if found:
            return found[int(round(which * (len(found) - 1)))]
    return None


def m_center_face_unassigned_l0(pyr):
    """rule 6: a face of an active level-0 centre loses its id"""
    l, cell, a, face = _center_sites(pyr, [0], lambda l, a, face, w: w >= 0, 0.5)
    pyr.put("vidx", 0, a, _kji(face), M.UNASSIGNED)
    return {M.RULE_CENTER_FACES}


def m_center_face_child(pyr):
    """rule 6: one of the four child faces under an UNASSIGNED face of an active coarse centre loses its id"""
    site = _center_sites(pyr, range(pyr.levels - 1, 0, -1), lambda l, a, face, w: w == M.UNASSIGNED)
    if site is None:
        return None
    l, cell, a, face = site
    b, c = M._others(a)
    pyr.put("vidx", l - 1, a, _kji(2 * face + _unit(b) + _unit(c)), M.UNASSIGNED)
    return {M.RULE_CENTER_FACES}


def m_center_face_sentinel(pyr):
    """rule 6: a face of an active centre at the highest level that has centres becomes OUTSIDE"""
    site = _center_sites(pyr, range(pyr.levels - 1, 0, -1), lambda l, a, face, w: w >= 0)
    if site is None:
        return None
    l, cell, a, face = site
    pyr.put("vidx", l, a, _kji(face), M.OUTSIDE)
    return {M.RULE_CENTER_FACES}


def m_center_face_other_negative(pyr):
    """rule 6: a face of an active centre holds -7"""
    l, cell, a, face = _center_sites(pyr, [0], lambda l, a, face, w: w >= 0, 1.0)
    pyr.put("vidx", 0, a, _kji(face), -7)
    return {M.RULE_CENTER_FACES}


def _center_edge_sites(pyr, l, want):
    """(cell xyz, a, edge xyz) of the first active centre of level l one of whose twelve edges satisfies want(a, edge, w)"""
    for k, j, i in np.argwhere(pyr.cidx[l] >= 0):
        cell = np.asarray((i, j, k), np.int64)
        for a in range(3):
            b, c = M._others(a)
            for q in range(4):
                edge = cell + (q & 1) * _unit(b) + (q >> 1) * _unit(c)
                if want(a, edge, int(pyr.eidx[l][a][_kji(edge)])):
                    return cell, a, edge
    return None


def m_center_edge_l0(pyr):
    """rule 7 at l = 0: an edge of an active level-0 centre loses its id"""
    cell, a, edge = _center_edge_sites(pyr, 0, lambda a, edge, w: w >= 0)
    pyr.put("eidx", 0, a, _kji(edge), M.UNASSIGNED)
    return {M.RULE_CENTER_EDGES, M.RULE_EDGE_NUMBERING}


def m_center_edge_l1(pyr):
    """rule 7 at l = 1: a child edge under an UNASSIGNED edge of an active level-1 centre loses its id"""
    if pyr.levels < 2:
        return None
    site = _center_edge_sites(pyr, 1, lambda a, edge, w: w == M.UNASSIGNED)
    if site is None:
        return None
    cell, a, edge = site
    child = 2 * edge + _unit(a)
    assert pyr.eidx[0][a][_kji(child)] >= 0
    pyr.put("eidx", 0, a, _kji(child), M.UNASSIGNED)
    return {M.RULE_CENTER_EDGES, M.RULE_EDGE_NUMBERING}


def m_center_edge_l2(pyr):
    """rule 7 at l >= 2: a grandchild edge under an UNASSIGNED edge of an active level-2 centre, whose child carries no id either, loses
    its id"""
    if pyr.levels < 3:
        return None
    for h in (0, 1):
        site = _center_edge_sites(pyr, 2, lambda a, edge, w: w == M.UNASSIGNED and pyr.eidx[1][a][_kji(2 * edge + h * _unit(a))] < 0)
        if site is not None:
            cell, a, edge = site
            grand = 2 * (2 * edge + h * _unit(a)) + _unit(a)
            assert pyr.eidx[0][a][_kji(grand)] >= 0
            pyr.put("eidx", 0, a, _kji(grand), M.UNASSIGNED)
            return {M.RULE_CENTER_EDGES, M.RULE_EDGE_NUMBERING}
    return None


def m_two_edge_values(pyr):
    """two entries at once: `first` is the one with the smaller key (level 0, axis 0 before level 0, axis 2)"""
    m_value("eidx", "last", "sb", top=True)(pyr)
    m_value("eidx", "middle", "n5")(pyr)
    return {M.RULE_EDGE_VALUE}


def m_two_rules(pyr):
    """a centre value and an edge face: `first` is the edge rule"""
    m_value("cidx", "first", "sb")(pyr)
    return m_edge_face_other_negative(pyr) | {M.RULE_CENTER_VALUE}


MUTATIONS = {
    **{f"{kind}_{where}_{value}": m_value(kind, where, value) for kind in ("eidx", "cidx") for where in ("first", "last", "middle") for value in ("sb", "n", "n5")},
    **{f"{kind}_top_{where}_{value}": m_value(kind, where, value, top=True) for kind in ("eidx", "cidx") for where, value in (("first", "n"), ("last", "sb"), ("middle", "n5"))},
    "edge_cell_down": m_edge_cell_down(False),
    "edge_cell_down_top": m_edge_cell_down(True),
    "edge_id_at_first": m_edge_id_at("first"),
    "edge_id_at_last": m_edge_id_at("last"),
    "edge_face_sentinel_l1": m_edge_face_sentinel,
    "edge_face_odd": m_edge_face_odd,
    "edge_face_even": m_edge_face_even,
    "edge_face_top_unassigned": m_edge_face_top_unassigned,
    "edge_face_other_negative": m_edge_face_other_negative,
    "edge_id_repeated": m_id_repeated("eidx"),
    "edge_id_missing": m_id_missing("eidx"),
    "center_label": m_center_label(False),
    "center_label_top": m_center_label(True),
    "center_face_unassigned_l0": m_center_face_unassigned_l0,
    "center_face_child": m_center_face_child,
    "center_face_sentinel": m_center_face_sentinel,
    "center_face_other_negative": m_center_face_other_negative,
    "center_edge_l0": m_center_edge_l0,
    "center_edge_l1": m_center_edge_l1,
    "center_edge_l2": m_center_edge_l2,
    "center_id_repeated": m_id_repeated("cidx"),
    "center_id_missing": m_id_missing("cidx"),
    "two_edge_values": m_two_edge_values,
    "two_rules": m_two_rules,
}
ONLY_WITH_THREE_LEVELS = ("center_edge_l2",)


@functools.lru_cache(maxsize=None)
def mutated(scene_name, mutation):
    """(Pyramid, rules that must fire, the model's report), or None where the pyramid has no site for the mutation -- computed once, shared
    by the tests, never written"""
    pyr = oracle_pyramid(scene_name)
    must = MUTATIONS[mutation](pyr)
    if must is None:
        return None
    return pyr, must, M.check(*pyr.args())


def applicable():
    """(scene, mutation) pairs that have a site"""
    return [(s, m) for s in MUTATED_SCENES for m in MUTATIONS if not (m in ONLY_WITH_THREE_LEVELS and s == "sphere16_L2")]
