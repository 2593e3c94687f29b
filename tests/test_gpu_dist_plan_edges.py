"""The device partition planners (csrc/avs_dist_plan.hip) on the edge cases of tests/dist_plan_edges.py, through avs_dist_plan_probe
(libavs_probe.so): plan_from_source, the core of avs_dist_partition's device planner, and dist_tail_from_rows, everything avs_dist_assemble
does behind assemble_rows, on the caller's arrays -- every case, every rank of its world.

It is all integer work and moved values: every array must EQUAL the model's (tests/dist_plan_model.py), values as 64-bit patterns, and none
of the guard bytes the probe puts behind every array the planner fills may have changed."""
import numpy as np
import pytest
import torch

import dist_plan_edges as E
from adaptiveviscositysolver_amd import capi

pytestmark = pytest.mark.gpu

INT_ARRAYS = ("own_global", "halo_global", "row_ptr_local", "col_local", "send_idx", "peers", "send_counts", "recv_counts", "tiles_int",
              "tiles_bnd")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _device(c):
    dev = torch.device("cuda:0")
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(row_ptr=up(c.row_ptr), col=up(c.col), val=up(c.val), dof=up(c.dof), perm=up(c.perm), owner=up(c.owner), dom=up(c.dom))


def _probe(c, d, rank, **over):
    if c.tail:
        kw = dict(owner=d["owner"], dom=d["dom"], split=c.split)
        mode = capi.DIST_PLAN_PROBE_TAIL
    else:
        kw = dict(dof=d["dof"], perm=d["perm"], levels=c.levels, cut_axis=c.cut_axis, extent=c.extent)
        mode = capi.DIST_PLAN_PROBE_PLAN
    kw.update(over)
    world = kw.pop("world", c.world)
    return capi.dist_plan_probe(mode, kw.pop("row_ptr", d["row_ptr"]), kw.pop("col", d["col"]), d["val"], rank, world, **kw)


def _compare(c, rank, info, got, want):
    L = E.limits()
    assert (info.lds_planes, info.scan_tile, info.spmv_tile_rows, info.row_group, info.max_world) == tuple(L)
    assert info.guard_bytes_hit == 0, (c.name, rank, info.guard_bytes_hit)
    assert (info.n_own, info.n_halo, info.n_send, info.nnz_local, info.n_peers, info.n_tiles_int, info.n_tiles_bnd) == (
        len(want["own_global"]), len(want["halo_global"]), len(want["send_idx"]), len(want["col_local"]), len(want["peers"]),
        len(want["tiles_int"]), len(want["tiles_bnd"])), (c.name, rank)
    for k in INT_ARRAYS:
        assert np.array_equal(got[k], want[k]), (c.name, rank, k, got[k][:16], want[k][:16])
    bad = np.nonzero(bits(got["val_local"]) != bits(want["val_local"]))[0]
    assert len(bad) == 0, (c.name, rank, len(bad), bad[:8])


@pytest.mark.parametrize("name", E.PLAN_NAMES)
def test_plan_equals_the_model(name, built_lib):
    c = E.by_name(name)
    d = _device(c)
    w, po, owner = c.owners()
    for rank, want in enumerate(c.plans()):
        info, got = _probe(c, d, rank)
        assert info.nplanes == len(w)
        assert np.array_equal(got["weights"], w), (name, rank)
        assert np.array_equal(got["plane_owner"], po), (name, rank)
        assert np.array_equal(got["owner"], owner), (name, rank)
        assert info.n_interior == -1
        _compare(c, rank, info, got, want)


@pytest.mark.parametrize("name", E.TAIL_NAMES + E.REFUSED_TAIL_NAMES)
def test_tail_equals_the_model(name, built_lib):
    c = E.by_name(name)
    d = _device(c)
    for rank, want in enumerate(c.plans()):
        if want == E.REFUSED:      # a column outside the window: the core's own refusal, not a crash
            with pytest.raises(capi.AvsError) as e:
                _probe(c, d, rank)
            assert e.value.status == capi.EINTERNAL and "outside the rank's window" in str(e.value)
            continue
        info, got = _probe(c, d, rank)
        assert info.n_interior == want["n_interior"], (name, rank)
        assert np.array_equal(got["local_ref"], want["local_ref"]), (name, rank)
        assert np.array_equal(bits(got["rhs_local"]), bits(want["rhs_local"])), (name, rank)
        _compare(c, rank, info, got, want)


def test_bad_arguments_are_refused_on_the_host(built_lib):
    dev = torch.device("cuda:0")
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
    plan, tail = E.by_name("non_neighbour_peers"), E.by_name("tail_split_1")
    dp, dt = _device(plan), _device(tail)

    def refused(c, d, rank, **over):
        with pytest.raises(capi.AvsError) as e:
            _probe(c, d, rank, **over)
        assert e.value.status == capi.EINVAL, e.value
    for c, d in ((plan, dp), (tail, dt)):
        refused(c, d, c.world)                          # rank >= world
        refused(c, d, -1)
        refused(c, d, 0, world=33)                      # world > 32
        refused(c, d, 0, world=0)
        col = c.col.copy()
        col[len(col) // 2] = c.n                        # a column outside [0, n)
        refused(c, d, 0, col=i32(col))
        col[len(col) // 2] = -1
        refused(c, d, 0, col=i32(col))
        rp = c.row_ptr.copy()
        rp[5] = rp[4] - 1                               # decreasing row pointers
        refused(c, d, 0, row_ptr=i32(rp))
    refused(plan, dp, 0, levels=0)
    refused(plan, dp, 0, levels=9)
    refused(plan, dp, 0, cut_axis=3)
    refused(plan, dp, 0, extent=0)
    refused(plan, dp, 0, extent=65536)                  # more than 65,535 planes at levels == 1
    perm = np.arange(plan.n)
    perm[3] = plan.n
    refused(plan, dp, 0, perm=i32(perm))
    # TAIL: an asymmetric pattern, an owner byte that is no rank, a dom entry listed twice
    asym = E.by_name("send_only_and_receive_only_peers")
    da = _device(asym)
    owner = torch.from_numpy(asym.owners()[2].astype(np.uint8)).to(dev)
    with pytest.raises(capi.AvsError) as e:
        capi.dist_plan_probe(capi.DIST_PLAN_PROBE_TAIL, da["row_ptr"], da["col"], da["val"], 0, asym.world, owner=owner, split=1)
    assert e.value.status == capi.EINVAL and "not symmetric" in str(e.value)
    bad_owner = tail.owner.copy()
    bad_owner[7] = tail.world
    refused(tail, dt, 0, owner=torch.from_numpy(bad_owner).to(dev))
    refused(tail, dt, 0, dom=i32([1, 2, 2]))
    # and the cases themselves still run afterwards (nothing was left behind by a refusal)
    info, got = _probe(plan, dp, 0)
    _compare(plan, 0, info, got, plan.plans()[0])


def test_small_capacity_is_refused(built_lib):
    c = E.by_name("non_neighbour_peers")
    d = _device(c)
    want = c.plans()[0]
    with pytest.raises(capi.AvsError) as e:
        _probe(c, d, 0, send_capacity=len(want["send_idx"]) - 1)
    assert e.value.status == capi.EINVAL and "send_idx" in str(e.value)
