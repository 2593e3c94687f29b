"""CPU proofs about the planted pyramids (tests/planted_pyramids.py), the branch census (tests/hotpath_census.py) and the FIFO restriction
model (tests/restriction_model.py): every case is what it claims to be before tests/test_gpu_planted_hotpath.py hands it to the kernels.

Branches that NO pyramid accepted by the hot path can reach (UNREACHABLE below; DESIGN 4.0a has the same arguments):

* edge_slot_dof_transition_face_outside -- "a DOF at a transition whose face is outside", the `.5` arm of cpp:1814-1827.  isAtTransition and
  isFaceOutside are indexed by the GRADIENT axis, and a gradient axis has exactly two slots (the two directions of one face axis,
  cpp:1745-1754).  The slot that is a DOF sets neither flag; the one slot left cannot be both UNASSIGNED (isAtTransition) and a sentinel or
  out of the lattice (isFaceOutside).  With isAtTransition set, a DOF slot always takes the `.25 / .25` pair.
* edge_slot_unassigned_odd_parent_sentinel -- a dangling edge whose level-(l+1) face is OUTSIDE or SOLIDBOUNDARY: sentinels are written at
  level 0 only (cpp:1210-1215, 1301-1319; rule SENTINEL of the octree check), and l + 1 >= 1.
* edge_slot_top_level_unassigned -- an UNASSIGNED slot of a top-level edge: the reference indexes past its level array (cpp:1853, 1888).
  Reached by the REFUSED cases only, as it must be.
* row_cell_out_of_lattice, volume_side_out_of_lattice -- a row is a face with an id; a face on the border of its lattice has one cell only
  and is never given an id (cpp:1210-1215), so both cells of a row are inside.
* SOLIDBOUNDARY terms at levels > 0 (asked for in the issue) are the same sentinel argument: edge_slot_solidboundary and
  center_slot_solidboundary are reached at level 0 only (test_sentinels_stay_at_level_0).

The restriction's weights: "multiplied in double without the fp32 rounding per level" CANNOT change a bit, on any case.  The weights are
products of 1/16 and 1/8, powers of two, so (float)(rw * (double)w) is exact down to 2^-126, level 31; the test asserts that this wrong
model is bit-identical on every list instead of pretending that a case could tell.  The two other wrong models (reverse fold, unclamped
border read) are caught.
"""
import os

import numpy as np
import pytest

import hotpath_census as H
import octree_check_model as OM
import planted_pyramids as P
import restriction_model as R
import stress_check_model as SM
from independent import check_linear_shear, check_scatter_form
from oracle import oracle as O

ACCEPTED = P.names(refused=False)
REFUSED = P.names(refused=True)
UNREACHABLE = ("edge_slot_dof_transition_face_outside", "edge_slot_unassigned_odd_parent_sentinel", "edge_slot_top_level_unassigned",
               "row_cell_out_of_lattice", "volume_side_out_of_lattice")
# refused pyramids that both checkers accept (the finding); zero_edge_weights is caught by the stress check's CENTER_EDGES rule
PASS_BOTH_CHECKERS = ("border_64_L5", "border_64_L6", "top_only_32_L3", "solid_sibling_32_L3")
_census = {}


def census_of(name):
    if name not in _census:
        from triplet_edges import limits
        lim = limits()
        c = P.cases()[name]
        _census[name] = H.census(P.classified(name)[1], c.scene.use_enhanced_gradients, lim.fast, lim.wave)
    return _census[name]


def hot(name):
    o, pyr = P.classified(name)
    if not getattr(o, "_hot", False):
        o.hot_path()
        o._hot = True
    return o, pyr


def test_case_list_is_what_the_issue_asks_for():
    c = P.cases()
    assert len(ACCEPTED) >= 15 and len(REFUSED) >= 4
    for n, case in c.items():
        assert max(case.scene.res) <= 64 or n == "shell1_128_L5", n       # level-4 rows need 128 cells across with an air margin
    assert {c[n].refused for n in REFUSED} >= {"cpp1878", "cpp1820", "cpp2680", "cpp1853_top_level"}
    assert set(c[n].levels for n in ACCEPTED) >= {3, 4, 5}
    assert len(set(c["shell1_64x32x16_L3"].scene.res)) == 3


def test_labels_of_a_hand_written_leaf_map():
    leaf = np.zeros((4, 4, 4), np.int8)
    leaf[:2, :2, :2] = 1                  # one level-1 leaf
    leaf[2:, 2:, 2:] = -1                 # one empty block
    lab = P.pyramid_from_leaf_levels(leaf, 3)
    assert (lab[0][:2, :2, :2] == P.UP).all() and (lab[0][2:, 2:, 2:] == P.INACTIVE).all() and (lab[0] == P.ACTIVE).sum() == 48
    assert lab[1][0, 0, 0] == P.ACTIVE and lab[1][1, 1, 1] == P.INACTIVE and (lab[1] == P.DOWN).sum() == 6
    assert lab[2].shape == (1, 1, 1) and lab[2][0, 0, 0] == P.DOWN
    with pytest.raises(AssertionError):
        bad = leaf.copy()
        bad[0, 0, 0] = 0                  # a level-1 block that is not uniform
        P.pyramid_from_leaf_levels(bad, 3)


@pytest.mark.parametrize("name", ACCEPTED)
def test_accepted_case_passes_both_checkers_and_the_hot_path(name):
    o, pyr = hot(name)
    r = OM.check(pyr.labels, pyr.vidx, pyr.n_velocity)
    assert r.passed, (r.violations, r.first)
    r = SM.check(*pyr.args())
    assert r.passed, (r.violations, r.first)
    cs = census_of(name)
    assert cs.asserts == {}
    top = max(l for l in range(pyr.levels) if (pyr.labels[l] == P.ACTIVE).any())
    assert top == pyr.levels - 1, "the top level holds no cell"


@pytest.mark.parametrize("name", ACCEPTED)
def test_census_lists_are_the_oracles_stencil_lists(name):
    """the census builds every stencil's face list from the rule; the oracle's lists are the same, entry by entry and in the same order,
    and the raw triplet count of the row sweep is the census's"""
    o, pyr = hot(name)
    cs = census_of(name)
    for got, st in ((cs.edge_lists, o.edge_stencils()), (cs.center_lists, o.center_stencils())):
        assert np.array_equal(got[0], st["cnt"])
        used = np.arange(st["idx"].shape[0])[:, None] < st["cnt"][None, :]
        assert np.array_equal(got[1], np.where(used, st["idx"], -1))
    assert int(cs.raw_row_lengths.sum()) == o.raw_triplets


@pytest.mark.parametrize("name", REFUSED)
def test_refused_case_is_refused_with_the_assert_the_census_predicts(name):
    case = P.cases()[name]
    o, pyr = P.classified(name)
    cs = census_of(name)
    fired = cs.refused_by()
    print(name, {a: cs.asserts[a] for a in fired})
    assert case.refused in fired
    both = OM.check(pyr.labels, pyr.vidx, pyr.n_velocity).passed and SM.check(*pyr.args()).passed
    assert both == (name in PASS_BOTH_CHECKERS)
    if set(fired) & set(H.STENCIL_ASSERTS):
        with pytest.raises(RuntimeError, match="build_stencils failed with code 12"):
            o.build_stencils()
    else:
        o.build_stencils()
        o.build_initial_guess()
        with pytest.raises(RuntimeError, match="assemble failed with code 10"):
            o.assemble()


@pytest.mark.parametrize("name", REFUSED)
def test_follower_of_a_refused_case_is_accepted(name):
    case = P.follower(name)
    o, pyr = P.classify(case)
    assert case.scene.res == P.cases()[name].scene.res and pyr.levels == P.cases()[name].levels
    assert OM.check(pyr.labels, pyr.vidx, pyr.n_velocity).passed and SM.check(*pyr.args()).passed
    assert H.census(pyr, True).asserts == {}
    o.hot_path()


def test_border_case_fires_where_the_issue_says():
    """coarse liquid cells on the domain border: a dangling level-l edge on a transition plane whose level-(l+1) border face is UNASSIGNED
    and whose children are no DOFs (cpp:1878), at several levels"""
    cs = census_of("border_64_L5")
    n, first = cs.asserts["cpp1878"]
    assert n > 0 and first[0] >= 1


def test_every_branch_is_reached_by_an_accepted_case(capsys):
    rows = {n: census_of(n) for n in ACCEPTED}
    with capsys.disabled():
        print()
        print(H.table(rows))
    total = {b: sum(c.counts[b] for c in rows.values()) for b in H.BRANCHES + H.PARITY}
    missing = [b for b, n in total.items() if n == 0 and b not in UNREACHABLE]
    assert missing == []
    assert [b for b in UNREACHABLE if total[b]] == []
    # the refused cases reach the one branch that is an assert
    assert census_of("top_only_32_L3").counts["edge_slot_top_level_unassigned"] > 0


def test_sentinels_stay_at_level_0():
    pyr = P.classified("solid_slab_32_L3")[1]
    for l in range(1, pyr.levels):
        for a in range(3):
            assert not np.isin(pyr.vidx[l][a], (H.SOLIDBOUNDARY, H.OUTSIDE)).any()
    st = hot("solid_slab_32_L3")[0]
    e, c = st.edge_stencils(), st.center_stencils()
    print("boundary terms in one stencil: edge", int(e["bcnt"].max()), "centre", int(c["bcnt"].max()))
    assert e["bcnt"].max() == O.EDGE_BCAP and c["bcnt"].max() == O.CENTER_BCAP      # up to the caps in one stencil
    lv = st.dof_table(O.I_EDGE)[:, 0] & 0xff
    assert (e["bcnt"][lv > 0] == 0).all()


def test_batch_sizes_and_merge_limits_are_the_kernels():
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adaptiveviscositysolver_amd", "csrc", "avs_assembly.hip")
    with open(src) as f:
        assert H.batch_sizes(f.read()) == (H.DRY_BATCH, H.EMIT_BATCH)
    from triplet_edges import limits
    lim = limits()
    total = {b: sum(census_of(n).counts[b] for n in ACCEPTED) for b in H.LENGTHS}
    for b in H.LENGTHS:
        assert total[b] > 0, b
    lengths = np.concatenate([census_of(n).raw_row_lengths for n in ACCEPTED])
    for edge in (lim.fast, lim.wave):                  # rows right at each limit and right past it
        assert (lengths <= edge).any() and (lengths > edge).any()


@pytest.mark.parametrize("name", ACCEPTED)
def test_restriction_model_gives_the_oracles_initial_guess(name):
    o, pyr = hot(name)
    sc = P.cases()[name].scene
    vel = [v.numpy() for v in sc.velocity]
    x0 = R.initial_guess(pyr.vidx, vel, pyr.n_velocity)
    assert not np.isnan(x0).any()
    assert np.array_equal(x0, o.initial_guess())


@pytest.mark.parametrize("name", P.RESTRICTION_NAMES)
def test_restriction_model_on_planted_dof_lists(name):
    """hand-written index pyramids: the FIFO model gives the oracle's bits up to level MAX_LEVEL, and the wrong models differ where they
    can (module docstring: unrounded weights never can)"""
    rl = P.restriction_list(name)
    o = P.oracle_for_restriction(rl)
    o.build_initial_guess()
    x = o.initial_guess()
    lv = rl.row_levels()
    k = lv <= R.MAX_LEVEL
    m = R.initial_guess(rl.vidx, rl.velocity, rl.n_velocity)
    assert np.array_equal(m[k], x[k]) and np.isnan(m[~k]).all()
    assert np.isfinite(x).all() and (x[lv > 0] != 0).all()
    if k.any():
        unrounded = R.initial_guess(rl.vidx, rl.velocity, rl.n_velocity, round_weights=False)
        assert np.array_equal(unrounded[k], x[k])
        if (lv[k] > 0).any():
            assert (R.initial_guess(rl.vidx, rl.velocity, rl.n_velocity, reverse=True)[k] != x[k]).any()
            assert (R.initial_guess(rl.vidx, rl.velocity, rl.n_velocity, clamp=False)[k] != x[k]).any()


def test_planted_lists_are_placed_where_they_claim():
    lv = P.restriction_list("levels_0_to_6_128_L8").row_levels()
    assert set(lv) == set(range(7)) and set(P.restriction_list("level_7_128_L8").row_levels()) == {7}
    for name in ("levels_0_to_6_128_L8", "level_7_128_L8"):
        rl = P.restriction_list(name)
        for l, a, p in rl.sites:                       # first or last entry of the lattice along every axis
            shape = rl.vidx[l][a].shape[::-1]
            assert all(p[d] in (0, shape[d] - 1) for d in range(3))
        assert {a for _, a, _ in rl.sites} == {0, 1, 2}
    for n in (1, 15, 16, 17, 33):
        assert int((P.restriction_list(f"coarse_rows_{n}").row_levels() >= 3).sum()) == n
    lv = P.restriction_list("groups_mix_levels_3_4_5").row_levels()
    for g in range(0, len(lv), 16):                    # consecutive ids: whatever 16 the list append keeps together mix the levels
        assert set(lv[g:g + 16]) == {3, 4, 5}
    lv = P.restriction_list("wave_lane_patterns").row_levels()
    waves = (lv >= 3).reshape(-1, 64)
    assert (waves[0] == (np.arange(64) % 2 == 1)).all() and waves[1].sum() == 1 and waves[1][0] and waves[2].sum() == 1 and waves[2][63]
    assert waves[3].all() and not waves[4].any() and 0 < waves[5].sum() < 64 and (waves[6] == (np.arange(64) % 2 == 0)).all()


def test_wrong_restrictions_show_on_classified_cases_too():
    """rows of a classified pyramid never read beyond the lattice (module docstring), so only the fold order can show there"""
    o, pyr = hot("shell1_32_L3")
    vel = [v.numpy() for v in P.cases()["shell1_32_L3"].scene.velocity]
    x = o.initial_guess()
    assert (R.initial_guess(pyr.vidx, vel, pyr.n_velocity, reverse=True) != x).any()
    assert np.array_equal(R.initial_guess(pyr.vidx, vel, pyr.n_velocity, clamp=False), x)


@pytest.mark.parametrize("name", ACCEPTED)
def test_independent_checks_pass_on_the_oracles_system(name):
    o, pyr = hot(name)
    case = P.cases()[name]
    A = o.csr()
    e, c = o.edge_stencils(), o.center_stencils()
    r = check_scatter_form(A.row_ptr, A.col, A.val, A.rhs, o.initial_guess(), e, c, pyr.n_center)
    # a face weight of exactly 0 (planted_weights) leaves A_ii - S_ii = 0 up to the rounding of two differently ordered sums, which
    # check_scatter_form itself bounds by its default rtol * scale
    assert r["mass_min"] >= -1e-12 * r["scale"] and r["mass_positive_fraction"] > 0.5 and r["dups"] == 0
    a = 3.0
    r = check_linear_shear(o.dof_table(O.I_VELOCITY), o.dof_table(O.I_EDGE), case.scene.dx, e, c, pyr.n_center, a=a)
    print(name, r)
    assert r["edge_uniform_n"] > 0 and r["edge_uniform_max"] <= 1e-9 * a
    assert r["center_n"] > 0 and r["center_max"] <= 1e-9 * a
    assert r["edge_transition_n"] > 0, "no planted transition counts towards the complete stencils"
    if case.scene.use_enhanced_gradients:
        assert r["edge_transition_max"] <= 1e-9 * a, r
    else:
        assert r["edge_transition_bad"] > 0
