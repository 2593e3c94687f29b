"""Pyramids for the octree check tests (test_octree_check_model.py, test_gpu_octree_check.py): the hand-built 4^3 pyramid, the oracle's
pre-pass on the scenes the rules were validated on, and named single-entry mutations of a pyramid.  A pyramid is (labels, vidx, n_velocity):
labels[l] int8 [z, y, x], vidx[l][a] int32 on the face lattice of axis a."""
import functools

import numpy as np

import octree_check_model as M
from adaptiveviscositysolver_amd import scenes
from oracle import oracle as O
from util import oracle_for_scene


# ---- the hand-built pyramid ------------------------------------------------------------------------------------------------------------
def number_faces(labels):
    """ids, in lattice order, on every face rule 5 allows (levels ascending, axes x, y, z); UNASSIGNED elsewhere"""
    L = len(labels)
    vidx, n = [], 0
    for l in range(L):
        per_level = []
        for a in range(3):
            shape = list(labels[l].shape)
            shape[2 - a] += 1
            probe = np.zeros(shape, np.int32)                      # an id everywhere: what survives rule 5 is a valid face
            ok = ~M.face_violations(labels, l, a, probe)
            v = np.full(shape, M.UNASSIGNED, np.int32)
            v[ok] = n + np.arange(int(ok.sum()), dtype=np.int32)
            n += int(ok.sum())
            per_level.append(v)
        vidx.append(per_level)
    return vidx, n


def hand_pyramid():
    """4^3, two levels: coarse cell (0, 0, 0) is ACTIVE and its eight children are UP; the seven other coarse cells are DOWN and their
    children ACTIVE"""
    fine = np.full((4, 4, 4), M.ACTIVE, np.int8)
    fine[:2, :2, :2] = M.UP
    coarse = np.full((2, 2, 2), M.DOWN, np.int8)
    coarse[0, 0, 0] = M.ACTIVE
    labels = [fine, coarse]
    vidx, n = number_faces(labels)
    return labels, vidx, n


# ---- oracle scenes ---------------------------------------------------------------------------------------------------------------------
def leaving_box_scene():
    from test_oracle_known_answers import leaving_box_scene as make
    return make()


SCENES = {
    "sphere16_L2": lambda: scenes.sphere(16, 2),
    "sphere32_L3": lambda: scenes.sphere(32, 3),
    "sphere64_L4": lambda: scenes.sphere(64, 4),
    "beam16_L2": lambda: scenes.fat_beam(16, 2),
    "beam32_L4": lambda: scenes.fat_beam(32, 4),
    "beam64_L3_wall": lambda: scenes.fat_beam(64, 3, wall=True),
    "tank32_L3": lambda: scenes.tank(32, 3),
    "sphere_obstacle64_L4": lambda: scenes.sphere_with_obstacle(64, 4),
    "sheet64_one_level": lambda: scenes.thin_sheet(64, 4, thickness_cells=6),
    "viscous_beam_c4": lambda: scenes.viscous_beam_scene(coarsen=4),
    "viscous_buckling_c4": lambda: scenes.viscous_buckling_scene(coarsen=4),
    "leaving_box": leaving_box_scene,
}


@functools.lru_cache(maxsize=None)
def _oracle_pyramid(name):
    sc = SCENES[name]()
    o = oracle_for_scene(sc)
    o.prepass()
    L = o.levels
    labels = [o.labels(l) for l in range(L)]
    vidx = [[o.index(O.I_VELOCITY, l, a) for a in range(3)] for l in range(L)]
    return sc, labels, vidx, o.count(O.I_VELOCITY)


def oracle_pyramid(name):
    """(labels, vidx, n_velocity) of the oracle's pre-pass: fresh copies, computed once per scene"""
    _, labels, vidx, n = _oracle_pyramid(name)
    return [a.copy() for a in labels], [[v.copy() for v in per_level] for per_level in vidx], n


def scene(name):
    return _oracle_pyramid(name)[0]


# ---- mutations -------------------------------------------------------------------------------------------------------------------------
# each takes (labels, vidx, n_velocity), edits ONE entry in place, and returns the rules that must fire
def _pick(mask, which=0.5):
    """one entry of the mask, in lattice order (which: position in the list of candidates, 0 .. 1)"""
    at = np.argwhere(mask)
    assert len(at), "the pyramid offers no entry for this mutation"
    return tuple(at[min(int(which * len(at)), len(at) - 1)])


def m_up_to_active(labels, vidx, n):
    labels[0][_pick(labels[0] == M.UP)] = M.ACTIVE
    return {M.RULE_COLUMN, M.RULE_UP}


def m_down_to_active_l1(labels, vidx, n):
    labels[1][_pick(labels[1] == M.DOWN)] = M.ACTIVE
    return {M.RULE_COLUMN, M.RULE_ACTIVE}


def m_active_to_down_l0(labels, vidx, n):
    labels[0][_pick(labels[0] == M.ACTIVE)] = M.DOWN
    return {M.RULE_COLUMN}


def m_nephew_inactive(labels, vidx, n):
    """the child at (2 i + 2, 2 j, 2 k) of the DOWN neighbour towards +x of a level-1 leaf (i, j, k)"""
    lab = labels[1]
    nb, inside = M._shift(lab, 2, 1)
    k, j, i = _pick((lab == M.ACTIVE) & inside & (nb == M.DOWN))
    assert labels[0][2 * k, 2 * j, 2 * i + 2] == M.ACTIVE
    labels[0][2 * k, 2 * j, 2 * i + 2] = M.INACTIVE
    return {M.RULE_UP, M.RULE_ACTIVE}


def m_label_7(labels, vidx, n):
    labels[0][_pick(labels[0] == M.ACTIVE)] = 7
    return {M.RULE_LABEL_VALUE}


def _border(level, i_of, value, rules):
    def mutate(labels, vidx, n):
        lab = labels[level]
        nz, ny, nx = lab.shape
        lab[nz // 2, ny // 2, i_of(nx)] = value
        return set(rules)
    return mutate


def m_id_duplicated(labels, vidx, n):
    v = vidx[0][0]
    a, b = _pick(v >= 0, 0.25), _pick(v >= 0, 0.75)
    assert v[a] != v[b]
    v[b] = v[a]
    return {M.RULE_NUMBERING}


def m_id_removed(labels, vidx, n):
    v = vidx[0][1]
    v[_pick(v >= 0)] = M.UNASSIGNED
    return {M.RULE_NUMBERING}


def m_id_n_velocity(labels, vidx, n):
    v = vidx[0][2]
    v[_pick(v >= 0)] = n
    return {M.RULE_INDEX_VALUE}


def m_id_between_inactive(labels, vidx, n):
    lab = labels[0]
    nb, inside = M._shift(lab, 1, -1)                   # the cell below along y
    k, j, i = _pick((lab == M.INACTIVE) & inside & (nb == M.INACTIVE), 0.1)
    assert vidx[0][1][k, j, i] < 0
    vidx[0][1][k, j, i] = 0
    return {M.RULE_FACE}


def m_sentinel_l1(labels, vidx, n):
    v = vidx[1][0]
    v[_pick(v == M.UNASSIGNED)] = M.SOLIDBOUNDARY
    return {M.RULE_SENTINEL}


def m_id_on_last_plane(labels, vidx, n):
    v = vidx[0][0]
    nz, ny, nxp = v.shape
    v[nz // 2, ny // 2, nxp - 1] = 1                    # face i = n: its forward cell lies outside the lattice
    return {M.RULE_FACE}


def _first(n):
    return 0


def _last(n):
    return n - 1


MUTATIONS = {
    "up_to_active": m_up_to_active,
    "down_to_active_l1": m_down_to_active_l1,
    "active_to_down_l0": m_active_to_down_l0,
    "nephew_inactive": m_nephew_inactive,
    "label_7": m_label_7,
    # edits at cells i = 0 and i = n - 1: the neighbour towards the border does not exist.  (A lone ACTIVE cell at level 0 under DOWN
    # ancestors is a valid leaf: -> ACTIVE at level 0 is no violation and is not in the list.)
    "i0_to_up": _border(0, _first, M.UP, (M.RULE_COLUMN, M.RULE_UP)),
    "ilast_to_up": _border(0, _last, M.UP, (M.RULE_COLUMN, M.RULE_UP)),
    "i0_to_down": _border(0, _first, M.DOWN, (M.RULE_COLUMN,)),
    "ilast_to_down": _border(0, _last, M.DOWN, (M.RULE_COLUMN,)),
    "i0_to_7": _border(0, _first, 7, (M.RULE_LABEL_VALUE,)),
    "ilast_to_7": _border(0, _last, 7, (M.RULE_LABEL_VALUE,)),
    "i0_l1_to_active": _border(1, _first, M.ACTIVE, (M.RULE_COLUMN,)),
    "ilast_l1_to_active": _border(1, _last, M.ACTIVE, (M.RULE_COLUMN,)),
    "id_duplicated": m_id_duplicated,
    "id_removed": m_id_removed,
    "id_n_velocity": m_id_n_velocity,
    "id_between_inactive": m_id_between_inactive,
    "sentinel_l1": m_sentinel_l1,
    "id_on_last_plane": m_id_on_last_plane,
}
MUTATED_SCENES = ("sphere16_L2", "sphere64_L4", "leaving_box")


@functools.lru_cache(maxsize=None)
def mutated(scene_name, mutation):
    """(labels, vidx, n_velocity, rules that must fire, the model's report) -- computed once, shared by the tests, never written"""
    labels, vidx, n = oracle_pyramid(scene_name)
    must = MUTATIONS[mutation](labels, vidx, n)
    return labels, vidx, n, must, M.check(labels, vidx, n)
