"""The assembly kernels (k_edge_stencils, k_center_stencils, k_initial_guess, k_initial_guess_coarse, k_rows with apply_stencil and
face_octree_volume; csrc/avs_assembly.hip) on PLANTED pyramids: tests/planted_pyramids.py places the cases, tests/test_planted_pyramids.py
proves on the CPU which branch each of them reaches (tests/hotpath_census.py) and that the oracle agrees with two statements of the rule
that share no code with it (the census's stencil lists, the FIFO restriction of tests/restriction_model.py).  Here the device is asked
for the oracle's bits, for the independent checks on its own system, and for AVS_EINTERNAL on the pyramids the hot path must
refuse.

Which case would catch which wrong kernel:
* a swapped .25 / .0625 coefficient: every accepted case with levels >= 2 (edge_slot_unassigned_odd_parent_id and _four_children are both
  reached, e.g. pocket_coarse_16_L2 for the four children, stair_* for both) -- coef differs, and check_linear_shear fails at the T-junctions;
* a self-entry search that stops at the batch: every case with self_past_dry_batch / self_past_emit_batch > 0 (all but plain_gradients for
  the emit batch): the row finds no own entry and the assembly reports a reference assert, or val / rhs differ;
* a `pw` that is not reduced: groups_mix_levels_3_4_5 and levels_0_to_6_128_L8 (levels >= 4 take more than one digit);
* a carry taken from the wrong lane: every list with a row of level >= 3 (coarse_rows_*: one to 33 rows, partial groups);
* a missing clamp: levels_0_to_6_128_L8 and level_7_128_L8 (every row sits on the first or last entry of its lattice along every axis).

Not reachable at these sizes: the second trip of k_initial_guess_coarse's persistent loop needs more than 256 workgroups x 4 waves x 16 rows
= 16,384 coarse rows in one list.
"""
import numpy as np
import pytest

import planted_pyramids as P
import restriction_model as R
from adaptiveviscositysolver_amd import ViscositySolve, capi
from independent import check_linear_shear, check_scatter_form
from oracle import oracle as O
from util import oracle_for_scene, oracle_from_pyramid

pytestmark = pytest.mark.gpu

ACCEPTED = P.names(refused=False)
REFUSED = P.names(refused=True)
RUNS = [(n, f32) for n in ACCEPTED for f32 in (False, True) if not (f32 and P.cases()[n].large)]


def oracle_of(case, pyr, f32):
    """util.oracle_from_pyramid for the fp64 oracle; the same inputs with SolveType = fpreal32 otherwise"""
    if not f32:
        o = oracle_from_pyramid(case.scene, pyr)
    else:
        o = oracle_for_scene(case.scene, f32=True)
        o.set_levels(pyr.levels)
        o.set_field(O.F_CENTERW, pyr.center_weights)
        for a in range(3):
            o.set_field(O.F_EDGEW + a, pyr.edge_weights[a])
            o.set_field(O.F_FACEW + a, pyr.face_weights[a])
        for l in range(pyr.levels):
            o.set_labels(l, pyr.labels[l])
            for a in range(3):
                o.set_index(O.I_VELOCITY, l, a, pyr.vidx[l][a])
                o.set_index(O.I_EDGE, l, a, pyr.eidx[l][a])
            o.set_index(O.I_CENTER, l, 0, pyr.cidx[l])
        o.finalize_indices()
    return o


def context_for(case, f32=False):
    sc = case.scene
    return ViscositySolve(sc.res, sc.dx, sc.dt, sc.levels, use_enhanced_gradients=sc.use_enhanced_gradients, device=0,
                          precision=capi.PRECISION_F32 if f32 else capi.PRECISION_F64)


def assert_oracles_bits(s, ai, o):
    for got, want in ((s.edge_stencils(), o.edge_stencils()), (s.center_stencils(), o.center_stencils())):
        for k in ("cnt", "idx", "bcnt", "coef", "bval", "weight"):
            assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(s.initial_guess(), o.initial_guess())
    rp, col, val, rhs = s.csr()
    A = o.csr()
    assert ai.n_velocity == A.n and ai.nnz == len(A.col) and ai.raw_triplets == o.raw_triplets
    assert np.array_equal(rp, A.row_ptr.astype(np.int32))
    assert np.array_equal(col, A.col)
    assert np.array_equal(val, A.val)
    assert np.array_equal(rhs, A.rhs)


def assemble_accepted(s, case, pyr):
    s.set_pyramid(pyr)
    s.set_scene_fields(case.scene)
    return s.assemble()


@pytest.mark.parametrize("name,f32", RUNS, ids=[f"{n}-{'f32' if f else 'f64'}" for n, f in RUNS])
def test_accepted_case_assembles_to_the_oracles_bits(name, f32, built_lib):
    case = P.cases()[name]
    pyr = P.classified(name)[1]
    s = context_for(case, f32)
    ai = assemble_accepted(s, case, pyr)
    o = oracle_of(case, pyr, f32)
    o.hot_path()
    assert_oracles_bits(s, ai, o)
    assert s.check_octree().passed and s.check_stress_indices().passed
    if not f32:
        # the independent checks on the DEVICE's own system.  mass_min: a face weight of exactly 0 leaves A_ii - S_ii = 0 up to the rounding
        # of two differently ordered sums, which check_scatter_form itself bounds by rtol * scale (its default rtol)
        rp, col, val, rhs = s.csr()
        e, c = s.edge_stencils(), s.center_stencils()
        r = check_scatter_form(rp, col, val, rhs, s.initial_guess(), e, c, pyr.n_center)
        assert r["mass_min"] >= -1e-12 * r["scale"] and r["mass_positive_fraction"] > 0.5 and r["dups"] == 0
        a = 3.0
        r = check_linear_shear(s.dof_table(capi.INDEX_VELOCITY), s.dof_table(capi.INDEX_EDGE), case.scene.dx, e, c, pyr.n_center, a=a)
        assert r["edge_uniform_n"] > 0 and r["edge_uniform_max"] <= 1e-9 * a
        assert r["center_n"] > 0 and r["center_max"] <= 1e-9 * a
        assert r["edge_transition_n"] > 0
        if case.scene.use_enhanced_gradients:
            assert r["edge_transition_max"] <= 1e-9 * a, r
        else:
            assert r["edge_transition_bad"] > 0
    s.close()


@pytest.mark.parametrize("name", REFUSED)
def test_refused_case_returns_einternal_and_the_context_stays_usable(name, built_lib):
    """pyramids the reference asserts on (which assert: the census, tests/test_planted_pyramids.py): an ordinary error return, and the
    next accepted pyramid on the same context assembles to the oracle's bits"""
    case = P.cases()[name]
    pyr = P.classified(name)[1]
    s = context_for(case)
    s.set_pyramid(pyr)
    s.set_scene_fields(case.scene)
    with pytest.raises(capi.AvsError) as e:
        s.assemble()
    assert e.value.status == capi.EINTERNAL
    nxt = P.follower(name)
    o, npyr = P.classify(nxt)
    ai = assemble_accepted(s, nxt, npyr)
    o.hot_path()
    assert_oracles_bits(s, ai, o)
    s.close()


# the two 128-cube lists (rows of 12^6 and 12^7 leaves, a second or more each in the oracle) run in fp64 only: the float context differs in
# the last narrowing alone, which the other lists check
RESTRICTION_RUNS = [(n, f32) for n in P.RESTRICTION_NAMES for f32 in (False, True) if not (f32 and n.endswith("_128_L8"))]


@pytest.mark.parametrize("name,f32", RESTRICTION_RUNS, ids=[f"{n}-{'f32' if f else 'f64'}" for n, f in RESTRICTION_RUNS])
def test_restriction_on_planted_dof_lists(name, f32, built_lib):
    """build_initial_guess alone on hand-written index pyramids (P.restriction_list).  Reference: the FIFO model up to its MAX_LEVEL, the
    oracle above; the two agree up to MAX_LEVEL on the CPU (tests/test_planted_pyramids.py) and here."""
    rl = P.restriction_list(name)
    dx = 1.0 / max(rl.res)
    s = ViscositySolve(rl.res, dx, 1.0 / 60.0, rl.levels, device=0, precision=capi.PRECISION_F32 if f32 else capi.PRECISION_F64)
    for l in range(rl.levels):
        s.set_labels(l, rl.labels[l])
        for a in range(3):
            s.set_index_field(capi.INDEX_VELOCITY, l, a, rl.vidx[l][a])
            s.set_index_field(capi.INDEX_EDGE, l, a, rl.eidx[l][a])
        s.set_index_field(capi.INDEX_CENTER, l, 0, rl.cidx[l])
    s.set_dof_counts(rl.n_velocity, 1, 1)
    for a in range(3):
        s.set_field(capi.FIELD_VELOCITY, a, rl.velocity[a])
    s.build_initial_guess()
    got = s.initial_guess()
    s.close()
    lv = rl.row_levels()
    k = lv <= R.MAX_LEVEL
    want = R.initial_guess(rl.vidx, rl.velocity, rl.n_velocity, f32=f32)
    assert np.array_equal(got[k], want[k])
    if not k.all() or name.startswith("coarse_rows") or name == "wave_lane_patterns":
        o = P.oracle_for_restriction(rl, f32=f32)
        o.build_initial_guess()
        assert np.array_equal(got, o.initial_guess())
