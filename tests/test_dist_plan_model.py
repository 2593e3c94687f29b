"""The plain model of the partition plan (tests/dist_plan_model.py) and the edge cases (tests/dist_plan_edges.py), without a GPU:
the model equals the host planner (avs_plan_owners + avs_plan_create, C++) array for array on every PLAN case and rank, every case reaches
the edge it is named after, and the model's plans keep the invariants tests/test_dist_plan.py asks of the host planner's."""
import numpy as np
import pytest

import dist_plan_edges as E
import dist_plan_model as M
from adaptiveviscositysolver_amd import capi

PLAN_ARRAYS = ("own_global", "halo_global", "row_ptr_local", "col_local", "send_idx", "peers", "send_counts", "recv_counts")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_the_case_list_is_the_named_one(built_lib):
    assert tuple(c.name for c in E.cases()) == E.NAMES
    assert all(c.tail == (c.name in E.TAIL_NAMES + E.REFUSED_TAIL_NAMES) for c in E.cases())
    assert all(c.n <= E.MAX_ROWS for c in E.cases())
    L = E.limits()
    assert L.group == 16 and L.max_world == 32 and L.T == capi.load().avs_spmv_tile_rows()
    assert L.lds_planes >= 1 and L.scan_tile >= 1


@pytest.mark.parametrize("name", E.NAMES)
def test_case_reaches_its_edge(name, built_lib):
    c = E.by_name(name)
    assert c.reaches_its_edge()
    if c.tail:
        assert c.symmetric()        # what the tail core relies on (the probe refuses anything else)


def test_greedy_cuts_of_scarce_and_empty_planes():
    """planes scarcer than ranks, a zero-weight plane as the last rank's only one, and a plain balanced cut"""
    assert list(M.plane_owners([5, 5, 5], 5)) == [1, 2, 3]
    assert list(M.plane_owners([0, 0, 7, 0, 9, 0], 3)) == [0, 0, 0, 1, 1, 2]
    assert list(M.plane_owners([1] * 8, 4)) == [0, 0, 1, 1, 2, 2, 3, 3]
    assert list(M.plane_owners([4, 1, 1], 1)) == [0, 0, 0]


@pytest.mark.parametrize("name", E.PLAN_NAMES)
def test_model_equals_the_host_planner(name, built_lib):
    c = E.by_name(name)
    w, po, owner = c.owners()
    tab = c.dof if c.perm is None else c.dof[c.perm]      # the host planner takes the records in row order
    host_owner = capi.plan_owners(tab, c.row_ptr, c.levels, c.cut_axis, c.extent, c.world)
    assert np.array_equal(owner, host_owner)
    assert w.sum() == len(c.col) + 2 * c.n and len(w) == len(po) == M.plane_count(c.levels, c.extent)
    for r, p in enumerate(c.plans()):
        h = capi.plan_create(c.row_ptr, c.col, host_owner, r, c.world)
        for k in PLAN_ARRAYS:
            assert np.array_equal(p[k], h[k]), (name, r, k)
        assert np.array_equal(bits(p["val_local"]), bits(c.val[h["val_src"]])), (name, r)
        # tile lists: the host planner's rule (avs_dist_plan.hip: plan_on_host) on the host planner's arrays
        T, n_own = E.limits().T, len(h["own_global"])
        bnd = [t for t in range(-(-n_own // T))
               if (h["col_local"][h["row_ptr_local"][t * T]:h["row_ptr_local"][min((t + 1) * T, n_own)]] >= n_own).any()]
        assert list(p["tiles_bnd"]) == bnd
        assert sorted(list(p["tiles_int"]) + bnd) == list(range(-(-n_own // T)))


@pytest.mark.parametrize("name", E.PLAN_NAMES + E.TAIL_NAMES)
def test_model_plans_are_consistent(name, built_lib):
    """each id owned once; what q sends to r is what r receives from q, in order; the local product on [owned | halo] is the owned rows
    of the global product bit for bit"""
    c = E.by_name(name)
    plans = c.plans()
    owner = c.owners()[2]
    inside = np.flatnonzero(owner != M.OUTSIDE)
    assert np.array_equal(np.sort(np.concatenate([p["own_global"] for p in plans])), inside)
    x = np.random.default_rng(E.SEED).standard_normal(c.n)
    y_ref = M.spmv(c.row_ptr, c.col, c.val, x)
    for r, p in enumerate(plans):
        n_own, n_halo = len(p["own_global"]), len(p["halo_global"])
        ho = owner[p["halo_global"]]
        assert (ho != r).all() and (np.diff(ho) >= 0).all()
        if c.dom is None:
            for q in np.unique(ho):
                assert (np.diff(p["halo_global"][ho == q]) > 0).all()
        assert list(p["peers"]) == sorted(set(p["peers"])) and r not in p["peers"]
        assert p["recv_counts"].sum() == n_halo and p["send_counts"].sum() == len(p["send_idx"])
        roff = 0
        for i, q in enumerate(p["peers"]):
            cnt = p["recv_counts"][i]
            mine = p["halo_global"][roff:roff + cnt]
            roff += cnt
            pq = plans[q]
            assert r in pq["peers"], (r, q)
            j = list(pq["peers"]).index(r)
            soff = int(pq["send_counts"][:j].sum())
            theirs = pq["own_global"][pq["send_idx"][soff:soff + pq["send_counts"][j]]]
            if c.dom is None:
                assert np.array_equal(mine, theirs), (r, q)
            else:   # the halo follows dom, the send list the sender's row order: the slab-local assembly makes the two agree by
                assert np.array_equal(np.sort(mine), np.sort(theirs)), (r, q)   # sorting its rows in dom's order; the sets must agree
        x_ext = np.concatenate([x[p["own_global"]], x[p["halo_global"]]])
        y_loc = M.spmv(p["row_ptr_local"], p["col_local"], p["val_local"], x_ext)
        assert np.array_equal(bits(y_loc), bits(y_ref[p["own_global"]])), (name, r)
        assert p["col_local"].min(initial=0) >= 0 and p["col_local"].max(initial=-1) < n_own + n_halo
        assert sorted(list(p["tiles_int"]) + list(p["tiles_bnd"])) == list(range(-(-n_own // E.limits().T)))


@pytest.mark.parametrize("name", [n for n in E.TAIL_NAMES])
def test_tail_without_split_is_the_plan(name, built_lib):
    """the symmetric-pattern shortcut itself: from its own rows alone a rank finds the send lists the whole matrix gives it.  Every TAIL
    case is rebuilt with split = 0 and no dom and compared with the PLAN model under the same owners."""
    c = E.by_name(name)
    owner = c.owners()[2]
    T = E.limits().T
    for r in range(c.world):
        t = M.tail_plan(c.row_ptr, c.col, c.val, owner, r, c.world, 0, None, T)
        p = M.plan(c.row_ptr, c.col, c.val, owner, r, c.world, T)
        for k in PLAN_ARRAYS + ("tiles_int", "tiles_bnd"):
            assert np.array_equal(t[k], p[k]), (name, r, k)
        assert np.array_equal(bits(t["val_local"]), bits(p["val_local"]))
        assert np.array_equal(t["local_ref"], np.concatenate([p["own_global"], p["halo_global"]]))


def test_split_order_is_stable_and_complete(built_lib):
    for name in E.TAIL_NAMES:
        c = E.by_name(name)
        owner = c.owners()[2]
        for r, p in enumerate(c.plans()):
            k = p["n_interior"]
            own = p["own_global"]
            assert np.array_equal(np.sort(own), np.flatnonzero(owner == r))
            if k < 0:
                assert (np.diff(own) > 0).all()
                continue
            assert (np.diff(own[:k]) > 0).all() and (np.diff(own[k:]) > 0).all()
            reads_halo = np.array([(p["col_local"][p["row_ptr_local"][l]:p["row_ptr_local"][l + 1]] >= len(own)).any() for l in range(len(own))], bool)
            assert not reads_halo[:k].any() and reads_halo[k:].all()
            assert np.array_equal(p["rhs_local"], own.astype(np.float64))
