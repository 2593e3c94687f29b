"""tests/octree_check_model.py, the NumPy statement of the rules of avs_check_octree (include/avs.h), pinned without a GPU:
(a) by hand-derived counts on a 4^3 two-level pyramid, (b) by the oracle's pre-pass on every scene the rules were validated on (zero
violations, and the reciprocity loop of oct.cpp:1250-1269, which the checker leaves out, never fails there), (c) by named single-entry
mutations that must fire their rule.  test_gpu_octree_check.py compares the device report with this model, entry for entry."""
import numpy as np
import pytest

import octree_check_cases as K
import octree_check_model as M

ZERO = (0,) * M.RULES


def counts(**by_name):
    return tuple(by_name.get(n, 0) for n in M.RULE_NAMES)


# ---- (a) the hand-built pyramid -------------------------------------------------------------------------------------------------------
def test_hand_pyramid_passes():
    labels, vidx, n = K.hand_pyramid()
    # ids: the faces between two ACTIVE fine cells and the twelve faces between the UP block and its ACTIVE neighbours; none at level 1
    assert all((v < 0).all() for v in vidx[1])
    assert n == sum(int((v >= 0).sum()) for v in vidx[0])
    rep = M.check(labels, vidx, n)
    assert rep == M.Report(1, ZERO, (-1,) * 6)
    assert M.reciprocity_failures(labels) == 0
    assert M.check(labels, None, None, M.CHECK_LABELS) == rep and M.check(labels, vidx, n, 0) == rep


def test_hand_pyramid_label_7():
    """cell (2, 0, 0), ACTIVE, becomes 7: not a label (rule 0), not a level-0 label of a column (rule 1), the UP cell (1, 0, 0) has a
    neighbour that is neither ACTIVE nor UP (rule 2), the coarse leaf (0, 0, 0) has a DOWN neighbour towards +x one of whose four facing children is not ACTIVE (rule 3), and the
    four faces of the cell that carry an id (towards -x, +x, +y, +z; -y and -z are the lattice border) lose their ACTIVE side (rule 5)"""
    labels, vidx, n = K.hand_pyramid()
    labels[0][0, 0, 2] = 7
    rep = M.check(labels, vidx, n)
    assert rep.violations == counts(LABEL_VALUE=1, COLUMN=1, UP=1, ACTIVE=1, FACE=4) and rep.passed == 0
    assert rep.first == (M.RULE_LABEL_VALUE, 0, 0, 2, 0, 0)
    assert M.check(labels, vidx, n, M.CHECK_VELOCITY_INDICES).first == (M.RULE_FACE, 0, 0, 2, 0, 0)   # the face between (1,0,0) and (2,0,0)
    assert M.check(labels, vidx, n, M.CHECK_LABELS).violations == counts(LABEL_VALUE=1, COLUMN=1, UP=1, ACTIVE=1)


def test_hand_pyramid_coarse_leaf_to_down():
    """coarse (0, 0, 0) ACTIVE -> DOWN: the eight UP columns have no ACTIVE ancestor (rule 1); the UP cells themselves keep their block
    and their neighbours (rule 2); the twelve fine ACTIVE cells that touch the block see an UP neighbour whose parent is not ACTIVE
    (rule 3), and the twelve faces between them carry ids (rule 5)"""
    labels, vidx, n = K.hand_pyramid()
    labels[1][0, 0, 0] = M.DOWN
    rep = M.check(labels, vidx, n)
    assert rep.violations == counts(COLUMN=8, ACTIVE=12, FACE=12)
    assert rep.first == (M.RULE_COLUMN, 0, 0, 0, 0, 0)


def test_hand_pyramid_up_to_active():
    """fine (0, 0, 0) UP -> ACTIVE: an ACTIVE column under an ACTIVE ancestor (rule 1), seven UP cells with a sibling that is not UP
    (rule 2); the new ACTIVE cell's UP neighbours have an ACTIVE parent (rule 3 holds) and its faces carry no id (rule 5 holds)"""
    labels, vidx, n = K.hand_pyramid()
    labels[0][0, 0, 0] = M.ACTIVE
    rep = M.check(labels, vidx, n)
    assert rep.violations == counts(COLUMN=1, UP=7)
    assert rep.first == (M.RULE_COLUMN, 0, 0, 0, 0, 0)


def test_hand_pyramid_up_at_the_top_level_and_down_at_level_0():
    labels, vidx, n = K.hand_pyramid()
    labels[1][1, 1, 1] = M.UP            # coarse (1, 1, 1): UP at level L-1 (rule 2); its eight ACTIVE columns want a DOWN there (rule 1);
    rep = M.check(labels, None, None, M.CHECK_LABELS)      # no ACTIVE coarse cell touches it (rule 3)
    assert rep.violations == counts(COLUMN=8, UP=1) and rep.first == (M.RULE_COLUMN, 0, 0, 2, 2, 2)
    labels, vidx, n = K.hand_pyramid()
    labels[0][3, 3, 3] = M.DOWN          # DOWN at level 0 (rule 1); its three ACTIVE neighbours see a DOWN at level 0 (rule 3)
    rep = M.check(labels, None, None, M.CHECK_LABELS)
    assert rep.violations == counts(COLUMN=1, ACTIVE=3) and rep.first == (M.RULE_COLUMN, 0, 0, 3, 3, 3)


def test_hand_pyramid_index_edits():
    labels, vidx, n = K.hand_pyramid()
    where = {int(v): tuple(int(x) for x in at) for at, v in np.ndenumerate(vidx[0][0]) if v >= 0}
    v = vidx[0][0]
    v[where[1]] = 0                      # id 0 twice, id 1 never
    rep = M.check(labels, vidx, n)
    assert rep.violations == counts(NUMBERING=2) and rep.first == (M.RULE_NUMBERING, 0, 0, 0, 0, 0)
    v[where[1]] = n                      # one past the last id (rule 4); id 1 is still missing (rule 7)
    rep = M.check(labels, vidx, n)
    k, j, i = where[1]
    assert rep.violations == counts(INDEX_VALUE=1, NUMBERING=1) and rep.first == (M.RULE_INDEX_VALUE, 0, 0, i, j, k)
    v[where[1]] = -4                     # below AVS_OUTSIDE
    assert M.check(labels, vidx, n).violations == counts(INDEX_VALUE=1, NUMBERING=1)
    v[where[1]] = 1
    vidx[1][2][2, 0, 0] = M.OUTSIDE      # a sentinel at level 1, on the last plane of the z faces
    rep = M.check(labels, vidx, n)
    assert rep.violations == counts(SENTINEL=1) and rep.first == (M.RULE_SENTINEL, 1, 2, 0, 0, 2)
    vidx[1][2][2, 0, 0] = M.UNASSIGNED
    vidx[0][0][3, 3, 4] = 5              # an id on the last x plane, i = n: the forward cell is outside (rule 5), id 5 twice (rule 7)
    rep = M.check(labels, vidx, n)
    assert rep.violations == counts(FACE=1, NUMBERING=1) and rep.first == (M.RULE_FACE, 0, 0, 4, 3, 3)
    assert M.check(labels, vidx, n, M.CHECK_LABELS).passed == 1


def test_one_level_pyramid():
    labels = [np.full((2, 2, 4), M.ACTIVE, np.int8)]
    vidx, n = K.number_faces(labels)
    assert n == 2 * 2 * 3 + 2 * 4 + 2 * 4
    assert M.check(labels, vidx, n).passed == 1
    labels[0][0, 0, 0] = M.UP            # no level above: rule 1 (no ACTIVE ancestor) and rule 2 (l = L-1); its three ACTIVE neighbours
    assert M.check(labels, vidx, n).violations == counts(COLUMN=1, UP=1, ACTIVE=3, FACE=3)   # see UP at l = L-1: rule 3; their faces: rule 5


# ---- (b) the oracle's pre-pass ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.SCENES))
def test_oracle_scenes_pass(name):
    labels, vidx, n = K.oracle_pyramid(name)
    if name == "sheet64_one_level":
        assert len(labels) == 1
    if name == "leaving_box":
        assert len(labels) == 3 and labels[0].shape == (64, 32, 64) and (labels[0][-1] != M.INACTIVE).any()   # liquid on the border
    rep = M.check(labels, vidx, n)
    assert rep == M.Report(1, ZERO, (-1,) * 6), rep
    assert M.reciprocity_failures(labels) == 0


# ---- (c) mutations ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutation", list(K.MUTATIONS))
@pytest.mark.parametrize("name", K.MUTATED_SCENES)
def test_mutations_fire_their_rules(name, mutation):
    labels, vidx, n, must, rep = K.mutated(name, mutation)
    assert rep.passed == 0 and must <= rep.fired(), (must, rep)
    assert rep.first[0] == min(rep.fired())
    clean = K.oracle_pyramid(name)
    changed = sum(int((a != b).sum()) for a, b in zip(labels, clean[0])) + sum(int((a != b).sum()) for la, lb in zip(vidx, clean[1]) for a, b in zip(la, lb))
    assert changed == 1


def test_rule_pairs_on_sphere16():
    """the pairs of label rules seen when the rules were validated"""
    fired = {m: M.check(K.mutated("sphere16_L2", m)[0], None, None, M.CHECK_LABELS) for m in ("up_to_active", "down_to_active_l1", "nephew_inactive")}
    assert fired["up_to_active"].fired() == {M.RULE_COLUMN, M.RULE_UP}
    assert fired["down_to_active_l1"].fired() == {M.RULE_COLUMN, M.RULE_ACTIVE} and fired["down_to_active_l1"].violations[M.RULE_COLUMN] == 8
    assert fired["nephew_inactive"].fired() == {M.RULE_UP, M.RULE_ACTIVE}
