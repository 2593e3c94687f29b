"""tests/stress_check_model.py, the NumPy statement of the rules of avs_check_stress_indices (include/avs.h), pinned without a GPU:
(a) by the oracle's pre-pass on the scenes the rules were validated on (zero violations, every branch a clean pyramid can take is taken),
(b) by an entry-by-entry restatement in plain Python loops that must agree with the vectorised model, (c) by named mutations that must
fire their rule.  test_gpu_stress_check.py compares the device report with this model, entry for entry."""
import pytest

import stress_check_cases as K
import stress_check_model as M

BOTH = M.CHECK_EDGE_INDICES | M.CHECK_CENTER_INDICES
WHATS = (BOTH, M.CHECK_EDGE_INDICES, M.CHECK_CENTER_INDICES)
ZERO = (0,) * M.RULES


# ---- (a) the oracle's pre-pass ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.SCENES))
def test_clean_scenes_pass(name):
    """Every scene passes for the three values of `what`, and the active counts are the dof counts.

    leaving_box is why rules 1, 2 and 6 are narrower on the border of the grid than the issue first stated them (include/avs.h says how).
    Liquid leaves the grid through its upper z border while the top level is still coarse there.  Stated as the reference asserts them,
    rule 2 fires on 119 edges (z faces on the border plane, UNASSIGNED at levels 1 and 2 with an UNASSIGNED parent, and twelve edges on
    that plane next to a DOWN cell whose face at the top level is UNASSIGNED), rule 6 on 63 coarse ACTIVE cells whose outer face and its
    children are UNASSIGNED, and the strict form of rule 1 on the twelve edges."""
    pyr = K.oracle_pyramid(name)
    if name == K.NON_CUBIC:
        assert len(set(pyr.labels[0].shape)) == 3
    for what in WHATS:
        rep = M.check(*pyr.args(), what)
        print(name, what, rep)
        assert rep == M.passed_report(pyr.n_edge if what & M.CHECK_EDGE_INDICES else 0, pyr.n_center if what & M.CHECK_CENTER_INDICES else 0), rep
    assert M.check(*pyr.args(), 0) == M.passed_report()


def test_every_branch_is_taken_on_a_clean_scene():
    """a rule that never reaches one of its branches on any clean pyramid would pass vacuously.  (The branches that are left out report
    a violation wherever they are reached -- a negative value that is no sentinel, an UNASSIGNED edge of a level-0 centre, ... --: the
    mutations reach them.)"""
    took = {}
    for name in ("sphere16_L2", "sphere32_L3", "sphere64_L4", "tank32_L3", "beam64_L3_wall", K.NON_CUBIC):
        pyr = K.oracle_pyramid(name)
        assert M.check(*pyr.args(), took=took).passed == 1
    print(took)
    assert set(took) == set(M.BRANCHES)
    assert all(took[name] > 0 for name in M.BRANCHES), took


def test_the_strict_form_of_rule_1_differs_only_on_the_border():
    """on every scene but leaving_box all four cells of every edge with an id lie in the lattice or are ACTIVE / UP: the walk that ends at
    the first cell outside the lattice and the test of all four cells agree"""
    for name in K.SCENES:
        pyr = K.oracle_pyramid(name)
        strict = 0
        for l in range(pyr.levels):
            for a in range(3):
                b, c = M._others(a)
                e = M._entries(pyr.eidx[l][a])
                for q in range(4):
                    lab, inside = M._read(pyr.labels[l], e - (q & 1) * M._unit(b) - (q >> 1) * M._unit(c), M.INACTIVE)
                    strict += int((inside & (lab != M.ACTIVE) & (lab != M.UP)).sum())
        assert strict == (12 if name == "leaving_box" else 0), (name, strict)
        assert M.check(*pyr.args(), M.CHECK_EDGE_INDICES).violations[M.RULE_EDGE_CELLS] == 0


# ---- (b) the entry-by-entry restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.MUTATED_SCENES)
def test_slow_model_agrees_on_clean_scenes(name):
    pyr = K.oracle_pyramid(name)
    for what in WHATS:
        assert M.check_slow(*pyr.args(), what) == M.check(*pyr.args(), what)


@pytest.mark.parametrize("name,mutation", K.applicable())
def test_slow_model_agrees_on_mutations(name, mutation):
    pyr, _, want = K.mutated(name, mutation)
    assert M.check_slow(*pyr.args()) == want


# ---- (c) mutations ---------------------------------------------------------------------------------------------------------------------
def test_only_the_listed_mutations_find_no_site():
    for name in K.MUTATED_SCENES:
        for mutation in K.MUTATIONS:
            assert (K.mutated(name, mutation) is None) == ((name, mutation) not in K.applicable()), (name, mutation)


@pytest.mark.parametrize("name,mutation", K.applicable())
def test_mutations_fire_their_rules(name, mutation):
    pyr, must, rep = K.mutated(name, mutation)
    print(name, mutation, rep)
    assert rep.passed == 0 and must <= rep.fired(), (must, rep)
    assert rep.first[0] == min(rep.fired())
    clean = K.oracle_pyramid(name)
    changed = 0
    for kind in ("labels", "vidx", "eidx", "cidx"):
        for l in range(pyr.levels):
            for a in range(3 if kind in ("vidx", "eidx") else 1):
                diff = int((pyr.lattice(kind, l, a) != clean.lattice(kind, l, a)).sum())
                assert (diff > 0) == ((kind, l, a) in pyr.edits)
                changed += diff
    assert changed == (2 if mutation.startswith("two_") else 1)
    # a rule of the other kind fires only through the lattices both kinds read, and never when it was not asked for
    edge_only, center_only = M.check(*pyr.args(), M.CHECK_EDGE_INDICES), M.check(*pyr.args(), M.CHECK_CENTER_INDICES)
    assert edge_only.violations == rep.violations[:4] + (0,) * 5 and center_only.violations == (0,) * 4 + rep.violations[4:]
    assert edge_only.active_centers == 0 and center_only.active_edges == 0


def test_value_mutations_at_the_ends_of_a_lattice():
    """first entry, last entry, a middle entry; SOLIDBOUNDARY, n and n + 5: rule 0 / 4 reports that entry"""
    for name in K.MUTATED_SCENES:
        for kind, rule in (("eidx", M.RULE_EDGE_VALUE), ("cidx", M.RULE_CENTER_VALUE)):
            for value in ("sb", "n", "n5"):
                pyr, _, rep = K.mutated(name, f"{kind}_first_{value}")
                assert rep.first == (rule, 0, 0, 0, 0, 0) and rep.violations[rule] == 1
                pyr, _, rep = K.mutated(name, f"{kind}_last_{value}")
                nz, ny, nx = pyr.lattice(kind, 0, 0).shape
                assert rep.first == (rule, 0, 0, nx - 1, ny - 1, nz - 1) and rep.violations[rule] == 1


def test_two_mutations_report_the_smaller_key():
    for name in K.MUTATED_SCENES:
        pyr, _, rep = K.mutated(name, "two_edge_values")
        assert rep.violations[M.RULE_EDGE_VALUE] == 2
        assert rep.first[:3] == (M.RULE_EDGE_VALUE, 0, 0) and rep.first == K.mutated(name, "eidx_middle_n5")[2].first
        assert K.mutated(name, "eidx_top_last_sb")[2].first[1] == pyr.levels - 1
        pyr, _, rep = K.mutated(name, "two_rules")
        assert rep.first[0] == M.RULE_EDGE_FACES and rep.violations[M.RULE_CENTER_VALUE] == 1
        assert M.check(*pyr.args(), M.CHECK_CENTER_INDICES).first == (M.RULE_CENTER_VALUE, 0, 0, 0, 0, 0)


def test_rule_7_is_reached_at_every_level():
    assert K.mutated("sphere16_L2", "center_edge_l0")[2].violations[M.RULE_CENTER_EDGES] > 0
    assert K.mutated("sphere16_L2", "center_edge_l1")[2].violations[M.RULE_CENTER_EDGES] > 0
    assert K.mutated("sphere32_L3", "center_edge_l2")[2].violations[M.RULE_CENTER_EDGES] > 0
    # ... by a centre of level 1 and of level 2
    pyr = K.mutated("sphere32_L3", "center_edge_l1")[0]
    assert M.center_edges_violations(pyr.eidx, 1, pyr.cidx[1]).any()
    pyr = K.mutated("sphere32_L3", "center_edge_l2")[0]
    assert M.center_edges_violations(pyr.eidx, 2, pyr.cidx[2]).any()
