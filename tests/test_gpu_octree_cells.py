"""avs_get_octree_cells / avs_prepass_get_octree_cells: the octree's ACTIVE cells as points, on the device (avs_cells.hip).

Reference: tests/octree_cells_model.py (NumPy; pinned to a serial sweep and to the oracle's fixtures by test_octree_cells_model.py), fed
with the label lattices the library itself holds.  Every array is compared bit for bit: the records are integers or one fp64 -> fp32
rounding the model reproduces exactly, so there is no tolerance anywhere in this module."""
import ctypes as C
import os
import threading

import numpy as np
import pytest
import torch

from adaptiveviscositysolver_amd import DevicePrepass, ViscositySolve, capi, scenes

import octree_cells_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ORIGIN = (0.1, -3.7, 12.3)      # not representable in binary: the fp64 sum is rounded, then narrowed once
SENTINEL = -123456789           # int32 pattern every buffer of the capacity tests is filled with (a NaN-free float pattern too)
NAMES = ("position", "pscale", "level", "ijk")


def same(got, want):
    """position, pscale, level, ijk, per_level: identical bytes"""
    assert len(got) == len(want) == 5
    for name, g, w in zip(NAMES + ("per_level",), got, want):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), name


def raw(fn, handle, capacity, arrays, where, origin=None, per_level=True):
    """one call of either entry; arrays: four pointers (or None).  Returns (status, n_cells, per_level, last error)"""
    org = None if origin is None else np.ascontiguousarray(origin, np.float64)
    n = C.c_int64(-1)
    pl = np.full(capi.MAX_LEVELS, -1, np.int64)
    st = fn(handle, None if org is None else org.ctypes.data, capacity, *arrays, C.byref(n), pl.ctypes.data if per_level else None, where)
    err = capi.load().avs_last_error().decode() if st != capi.OK else ""
    return st, int(n.value), pl, err


# ---- 1. hand-made labels through avs_set_labels ---------------------------------------------------------------------------------------
RES, LEVELS, DX = (64, 32, 16), 3, 1.0 / 64       # lattices 64x32x16 (4x2x1 tiles), 32x16x8 (partial in z), 16x8x4 (partial in y and z)


def lattice_shape(l):
    return (RES[2] >> l, RES[1] >> l, RES[0] >> l)


def zeros():
    return [np.zeros(lattice_shape(l), np.int8) for l in range(LEVELS)]


def random_labels(seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4, lattice_shape(l)).astype(np.int8) for l in range(LEVELS)]


def not_active(seed):
    rng = np.random.default_rng(seed)
    return [rng.choice(np.array([0, 2, 3], np.int8), lattice_shape(l)) for l in range(LEVELS)]


def case_one_level(level, value):
    labs = random_labels(10 + level)
    labs[level][...] = value
    return labs


def case_single(level, kji):
    labs = not_active(20 + level)
    labs[level][kji] = M.ACTIVE
    return labs


def case_row_ends():
    labs = not_active(30)
    labs[0][3, 5, 31] = M.ACTIVE     # x = 15 of one row of tile (1, 0, 0) ...
    labs[0][3, 6, 16] = M.ACTIVE     # ... and x = 0 of the next
    return labs


HAND_CASES = {
    "random": lambda: random_labels(1),
    "random_again": lambda: random_labels(2),
    "level0_inactive": lambda: case_one_level(0, 0),
    "level1_inactive": lambda: case_one_level(1, 0),
    "level2_inactive": lambda: case_one_level(2, 0),
    "level0_active": lambda: case_one_level(0, 1),
    "level1_active": lambda: case_one_level(1, 1),
    "level2_active": lambda: case_one_level(2, 1),
    "first_voxel_of_first_tile": lambda: case_single(0, (0, 0, 0)),
    "last_voxel_of_last_partial_tile": lambda: case_single(2, (3, 7, 15)),
    "none_active": lambda: not_active(40),
    "all_inactive": zeros,
    "row_ends": case_row_ends,
}


@pytest.fixture(scope="module")
def hand_ctx(built_lib):
    s = ViscositySolve(RES, DX, 1.0 / 60.0, LEVELS, device=0)      # no pre-pass, no index pyramids, no assembly
    yield s
    s.close()


@pytest.mark.parametrize("case", list(HAND_CASES))
def test_hand_made_labels(hand_ctx, case):
    labs = HAND_CASES[case]()
    for l in range(LEVELS):
        hand_ctx.set_labels(l, labs[l])
    want = M.cells(labs, DX, ORIGIN)
    if case in ("none_active", "all_inactive"):
        assert len(want[2]) == 0
    if case in ("first_voxel_of_first_tile", "last_voxel_of_last_partial_tile"):
        assert len(want[2]) == 1
    if case == "row_ends":
        assert want[3].tolist() == [[31, 5, 3], [16, 6, 3]]
    same(hand_ctx.octree_cells(ORIGIN), want)
    same(hand_ctx.octree_cells(ORIGIN, device_arrays=True), want)
    same(hand_ctx.octree_cells(), M.cells(labs, DX))


# ---- 1b. production-sized index paths on hand-made labels ----------------------------------------------------------------------------
# Resolutions are powers of two (avs_create), so a level's tile count along x is one too.  256 cells along x are 16 tiles = two strips of
# eight: strips with sx > 0, lanes with piece 4 .. 7 that own a tile, the strip -> (sx, ty, tz) decomposition.  16 x 8 x 16 = 2048 tiles,
# every one non-empty under random labels: more than the emit grid (1024 workgroups), so its walk takes a second tile per workgroup.
BIG_RES = (256, 128, 256)


def big_labels():
    rng = np.random.default_rng(77)
    return [rng.integers(0, 4, (BIG_RES[2], BIG_RES[1], BIG_RES[0])).astype(np.int8)]


@pytest.fixture(scope="module")
def big_case():
    labs = big_labels()
    return labs, M.cells(labs, 1.0 / 256, ORIGIN)


@pytest.mark.parametrize("grid_cap", [0, 3], ids=["default_grids", "grids_of_3"])
def test_strips_and_persistent_walks(built_lib, big_case, grid_cap, monkeypatch):
    """grid_cap 3: AVS_CELLS_GRID_CAP caps both persistent grids at three workgroups, so twelve waves walk the 256 strips (the count
    loop wraps 21 times) and three workgroups the 2048 listed tiles."""
    labs, want = big_case
    if grid_cap:
        monkeypatch.setenv("AVS_CELLS_GRID_CAP", str(grid_cap))     # read at avs_create
    s = ViscositySolve(BIG_RES, 1.0 / 256, 1.0 / 60.0, 1, device=0)
    s.set_labels(0, labs[0])
    assert len(want[2]) > 2_000_000
    same(s.octree_cells(ORIGIN, device_arrays=True), want)
    same(s.octree_cells(ORIGIN), want)
    s.close()


@pytest.mark.parametrize("grid_cap", [0, 2], ids=["default_grids", "grids_of_2"])
def test_two_strips_on_every_level_and_sparse_tiles(built_lib, grid_cap, monkeypatch):
    """three levels, 256 / 128 / 64 cells along x (two strips, one strip, half a strip), one tile in seven non-empty"""
    res, L = (256, 32, 64), 3
    rng = np.random.default_rng(78)
    labs = []
    for l in range(L):
        shp = (res[2] >> l, res[1] >> l, res[0] >> l)
        lab = rng.integers(0, 4, shp).astype(np.int8)
        tz, ty, tx = ((n + 15) // 16 for n in shp)
        keep = rng.integers(0, 7, (tz, ty, tx)) == 0
        keep[-1, -1, -1] = True                     # (the small upper levels have a handful of tiles: never none)
        keep = np.repeat(np.repeat(np.repeat(keep, 16, 0), 16, 1), 16, 2)[:shp[0], :shp[1], :shp[2]]
        lab[~keep & (lab == M.ACTIVE)] = 3
        labs.append(lab)
    if grid_cap:
        monkeypatch.setenv("AVS_CELLS_GRID_CAP", str(grid_cap))
    s = ViscositySolve(res, 1.0 / 256, 1.0 / 60.0, L, device=0)
    for l in range(L):
        s.set_labels(l, labs[l])
    want = M.cells(labs, 1.0 / 256, ORIGIN)
    assert all(want[4][:L] > 0)
    same(s.octree_cells(ORIGIN, device_arrays=True), want)
    s.close()


@pytest.mark.parametrize("res", [(8, 32, 16), (4, 64, 8), (32, 8, 128)], ids=lambda r: "x".join(map(str, r)))
def test_rows_shorter_than_a_tile(built_lib, res):
    """x extents of 8, 4, 2 and 1 cells (levels 0 .. 2): the bytewise row path, partial tiles along x; and 32 / 16 / 8 along x: a level
    that switches from 16-byte loads to bytes"""
    L = 3
    rng = np.random.default_rng(sum(res))
    labs = [rng.integers(0, 4, (res[2] >> l, res[1] >> l, res[0] >> l)).astype(np.int8) for l in range(L)]
    s = ViscositySolve(res, 0.125, 1.0 / 60.0, L, device=0)
    for l in range(L):
        s.set_labels(l, labs[l])
    want = M.cells(labs, 0.125, ORIGIN)
    assert all(want[4][:L] > 0)
    same(s.octree_cells(ORIGIN), want)
    same(s.octree_cells(ORIGIN, device_arrays=True), want)
    s.close()


# ---- 2. pre-pass scenes ---------------------------------------------------------------------------------------------------------------
def golden_scene(name):
    g = np.load(os.path.join(HERE, "golden", name + ".npz"))
    solid = torch.from_numpy(g["solid"]) if g["solid"].size else None
    return dict(res=tuple(int(v) for v in g["res"]), dx=float(g["dx"]), levels=int(g["desired_levels"]), liquid=torch.from_numpy(g["liquid"]),
                solid=solid, field_res=None, want_labels=[g[f"labels{l}"] for l in range(int(g["levels"]))])


def synthetic(sc):
    return dict(res=sc.res, dx=sc.dx, levels=sc.levels, liquid=sc.liquid, solid=sc.solid, field_res=None, want_labels=None)


def padded_scene():
    res, fres, dx = (32, 32, 64), (24, 20, 40), 1.0 / 32
    liquid = scenes.box_sdf(fres, dx, center=(12 * dx, 10 * dx, 20 * dx), half=(7 * dx, 5 * dx, 14 * dx))   # on the SIMULATION grid
    return dict(res=res, dx=dx, levels=2, liquid=liquid, solid=None, field_res=fres, want_labels=None)


SCENES = {
    "golden_sphere16": lambda: golden_scene("sphere16_L3"),
    "golden_wall_beam32": lambda: golden_scene("beam32_L2_wall_varvisc"),
    "noncubic_32x16x64": lambda: synthetic(scenes.fat_beam(64, 2, res=(32, 16, 64))),
    "padded_24x20x40_in_32x32x64": padded_scene,
    "beam64_L3": lambda: synthetic(scenes.fat_beam(64, 3)),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_prepass_scenes(name, built_lib):
    d = SCENES[name]()
    pp = DevicePrepass(d["res"], d["dx"], d["levels"], field_res=d["field_res"])
    info = pp.run(d["liquid"].cuda(), None if d["solid"] is None else d["solid"].cuda())
    L = int(info.levels)
    assert L >= 2
    labels = [pp.labels(l) for l in range(L)]
    if d["want_labels"] is not None:       # the fixture's own pyramid: the export is the model on the ORACLE's labels
        assert len(d["want_labels"]) == L and all(np.array_equal(a, b) for a, b in zip(labels, d["want_labels"]))
    want = M.cells(labels, d["dx"], ORIGIN)
    assert len(want[2]) > 0 and all(want[4][:L] > 0)
    same(pp.octree_cells(ORIGIN), want)
    same(pp.octree_cells(ORIGIN, device_arrays=True), want)
    if d["field_res"] is not None:         # no cell reaches beyond the simulation grid
        pos, ps, lev, ijk, _ = want
        assert ((ijk.astype(np.int64) + 1) << lev[:, None] <= np.asarray(d["field_res"])[None, :]).all()
        hi = np.asarray(ORIGIN) + np.asarray(d["field_res"]) * d["dx"]
        assert (pos.astype(np.float64) < hi[None, :]).all() and (pos.astype(np.float64) > np.asarray(ORIGIN)[None, :]).all()
    s = ViscositySolve(d["res"], d["dx"], 1.0 / 60.0, L, device=0, field_res=d["field_res"])
    pp.apply(s)                             # lent lattices: the same bytes through the context entry
    same(s.octree_cells(ORIGIN), want)
    same(s.octree_cells(ORIGIN, device_arrays=True), want)
    s.close()
    pp.close()


def test_prepass_entry_with_wrapping_walks(built_lib, monkeypatch):
    """the pre-pass object with both persistent grids capped at two workgroups: 64^3 + 32^3 + 16^3 lattices are 73 tiles"""
    monkeypatch.setenv("AVS_CELLS_GRID_CAP", "2")     # read at avs_prepass_create
    sc = scenes.to_device(scenes.fat_beam(64, 3), torch.device("cuda:0"))
    pp = DevicePrepass(sc.res, sc.dx, sc.levels)
    L = int(pp.run(sc.liquid, sc.solid).levels)
    want = M.cells([pp.labels(l) for l in range(L)], sc.dx, ORIGIN)
    same(pp.octree_cells(ORIGIN), want)
    same(pp.octree_cells(ORIGIN, device_arrays=True), want)
    pp.close()


# ---- 3. origin ------------------------------------------------------------------------------------------------------------------------
def test_origin_is_added_in_fp64_and_rounded_once(hand_ctx):
    labs = random_labels(3)
    for l in range(LEVELS):
        hand_ctx.set_labels(l, labs[l])
    pos, ps, lev, ijk, _ = hand_ctx.octree_cells(ORIGIN)
    h = DX * np.exp2(lev.astype(np.float64))
    want = (np.asarray(ORIGIN, np.float64)[None, :] + (ijk.astype(np.float64) + 0.5) * h[:, None]).astype(np.float32)
    assert pos.tobytes() == want.tobytes()
    assert ps.tobytes() == h.astype(np.float32).tobytes()
    assert not np.array_equal(pos, hand_ctx.octree_cells()[0])


# ---- 4. capacity protocol -------------------------------------------------------------------------------------------------------------
def sentinel_buffers(capacity, device):
    shapes = ((capacity, 3), (capacity,), (capacity,), (capacity, 3))
    if device:
        bufs = [torch.full(s, SENTINEL, dtype=torch.int32, device="cuda:0") for s in shapes]
        torch.cuda.synchronize()
        return bufs, [b.data_ptr() for b in bufs]
    bufs = [np.full(s, SENTINEL, np.int32) for s in shapes]
    return bufs, [b.ctypes.data for b in bufs]


def host_bytes(bufs):
    torch.cuda.synchronize()
    return [(b.cpu().numpy() if isinstance(b, torch.Tensor) else b) for b in bufs]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_capacity_protocol(hand_ctx, device):
    labs = random_labels(4)
    for l in range(LEVELS):
        hand_ctx.set_labels(l, labs[l])
    want = M.cells(labs, DX, ORIGIN)
    n = len(want[2])
    fn, h, where = hand_ctx.lib.avs_get_octree_cells, hand_ctx.h, capi.MEM_DEVICE if device else capi.MEM_HOST
    # count query: NULL arrays
    st, got_n, pl, _ = raw(fn, h, 0, [None] * 4, where, ORIGIN)
    assert st == capi.OK and got_n == n and np.array_equal(pl, want[4])
    st, got_n, _, _ = raw(fn, h, 0, [None] * 4, where, ORIGIN, per_level=False)
    assert st == capi.OK and got_n == n
    # one record short: AVS_EINVAL, the count is reported, nothing is written
    bufs, ptrs = sentinel_buffers(n - 1, device)
    st, got_n, pl, err = raw(fn, h, n - 1, ptrs, where, ORIGIN)
    assert st == capi.EINVAL and got_n == n and np.array_equal(pl, want[4]) and err
    assert all((b == SENTINEL).all() for b in host_bytes(bufs))
    # 64 records of room: exactly n are written, the 64 behind them keep the sentinel
    bufs, ptrs = sentinel_buffers(n + 64, device)
    st, got_n, _, _ = raw(fn, h, n + 64, ptrs, where, ORIGIN)
    assert st == capi.OK and got_n == n
    for b, w in zip(host_bytes(bufs), want[:4]):
        assert b[:n].tobytes() == w.tobytes() and (b[n:] == SENTINEL).all()
    # every array NULL in turn (ijk first)
    for skip in (3, 0, 1, 2):
        bufs, ptrs = sentinel_buffers(n, device)
        ptrs[skip] = None
        st, got_n, _, _ = raw(fn, h, n, ptrs, where, ORIGIN)
        assert st == capi.OK and got_n == n
        for k, (b, w) in enumerate(zip(host_bytes(bufs), want[:4])):
            assert (b == SENTINEL).all() if k == skip else b.tobytes() == w.tobytes(), (skip, k)


# ---- 5. frame loop --------------------------------------------------------------------------------------------------------------------
def test_frame_loop_leaves_no_stale_scratch(built_lib):
    dev = torch.device("cuda:0")
    A = scenes.to_device(scenes.fat_beam(64, 3), dev)
    B = scenes.to_device(scenes.sphere(64, 3), dev)
    pp = DevicePrepass(A.res, A.dx, 3)
    counts = []
    for sc in (A, B, A):
        pp.run(sc.liquid, sc.solid)
        got = pp.octree_cells(ORIGIN)
        fresh = DevicePrepass(sc.res, sc.dx, 3)
        fresh.run(sc.liquid, sc.solid)
        same(got, fresh.octree_cells(ORIGIN))
        fresh.close()
        same(pp.octree_cells(ORIGIN), got)           # two calls in a row
        same(pp.octree_cells(ORIGIN, device_arrays=True), got)
        counts.append(len(got[2]))
    assert counts[0] == counts[2] != counts[1] and min(counts) > 0
    pp.close()


# ---- 6. composition with avs_sample_velocity ------------------------------------------------------------------------------------------
def test_cell_centres_go_straight_into_the_sampler(built_lib):
    dev = torch.device("cuda:0")
    sc = scenes.to_device(scenes.sphere(32, 3), dev)
    pp = DevicePrepass(sc.res, sc.dx, sc.levels)
    info = pp.run(sc.liquid, sc.solid)
    s = ViscositySolve(sc.res, sc.dx, sc.dt, info.levels, device=0)
    pp.apply(s)
    s.set_scene_fields(sc)
    s.assemble()
    assert s.solve(1e-8, 3000).converged == 1
    pos, ps, lev, ijk, per_level = s.octree_cells(ORIGIN, device_arrays=True)
    assert pos.is_cuda and pos.shape == (int(per_level.sum()), 3)
    vel, inside = s.sample_velocity(pos, ORIGIN)      # device arrays in, nothing crosses to the host in between
    assert bool((inside == 1).all())
    pos_h, _, lev_h, _, _ = s.octree_cells(ORIGIN)
    fine = lev_h == 0
    assert fine.sum() > 1000
    vel_h, inside_h = s.sample_velocity(pos_h[fine], ORIGIN)
    assert inside_h.all() and np.array_equal(vel.cpu().numpy()[fine], vel_h) and np.abs(vel_h).max() > 0
    s.close()
    pp.close()


# ---- 7. state errors ------------------------------------------------------------------------------------------------------------------
def test_state_errors(built_lib):
    lib = capi.load()
    s = ViscositySolve(RES, DX, 1.0 / 60.0, LEVELS, device=0)
    labs = random_labels(5)
    for l in (0, 2):                                  # level 1 missing
        s.set_labels(l, labs[l])
    st, _, _, err = raw(lib.avs_get_octree_cells, s.h, 0, [None] * 4, capi.MEM_HOST)
    assert st == capi.ESTATE and err
    s.set_labels(1, labs[1])
    st, n, _, _ = raw(lib.avs_get_octree_cells, s.h, 0, [None] * 4, capi.MEM_HOST)
    assert st == capi.OK and n == len(M.cells(labs, DX)[2])
    st, _, _, err = raw(lib.avs_get_octree_cells, s.h, 0, [None] * 4, 7)          # a bad memory space
    assert st == capi.EINVAL and err
    s.close()
    pp = DevicePrepass((32, 32, 32), 1.0 / 32, 2)     # has not run
    st, _, _, err = raw(lib.avs_prepass_get_octree_cells, pp.h, 0, [None] * 4, capi.MEM_HOST)
    assert st == capi.ESTATE and err
    st, _, _, err = raw(lib.avs_prepass_get_octree_cells, pp.h, 0, [None] * 4, 7)
    assert st == capi.EINVAL and err
    pp.close()


def test_no_liquid_gives_no_cells(built_lib):
    liquid = torch.full((16, 16, 16), 10.0, dtype=torch.float32, device="cuda:0")
    pp = DevicePrepass((16, 16, 16), 1 / 16, 3)
    assert pp.run(liquid).levels == 0
    st, n, pl, _ = raw(pp.lib.avs_prepass_get_octree_cells, pp.h, 0, [None] * 4, capi.MEM_HOST)
    assert st == capi.OK and n == 0 and not pl.any()
    got = pp.octree_cells()
    assert all(len(a) == 0 for a in got[:4])
    pp.close()


def test_slab_local_objects_are_refused(built_lib):
    """Two virtual ranks of an in-process group, bound the way tests/test_gpu_slab.py binds them: the labels of a slab-local pre-pass and
    of the context it was applied to are defined inside the rank's window only."""
    dev = torch.device("cuda:0")
    world, axis = 2, 0
    sc = scenes.to_device(scenes.fat_beam(32, 2), dev)
    lib = capi.load()
    pp0 = DevicePrepass(sc.res, sc.dx, sc.levels)
    lv = pp0.run(sc.liquid, sc.solid).levels
    pp0.close()
    grp = C.c_void_p()
    capi.check(lib.avs_local_group_create(world, C.byref(grp)))
    cuts = np.asarray([0, 16, 32], np.int32)
    results, errors, objs = [None] * world, [], []

    def rank_fn(r):
        try:
            pp = DevicePrepass(sc.res, sc.dx, sc.levels)
            s = ViscositySolve(sc.res, sc.dx, sc.dt, lv, device=0)
            objs.append((s, pp))
            s.dist_init_local(grp, r)
            s.dist_bind_prepass(pp, cuts, axis)
            a = raw(lib.avs_prepass_get_octree_cells, pp.h, 0, [None] * 4, capi.MEM_HOST)       # refused at entry, before any run
            assert pp.run(sc.liquid, sc.solid).levels == lv
            pp.apply(s)
            b = raw(lib.avs_prepass_get_octree_cells, pp.h, 0, [None] * 4, capi.MEM_HOST)
            c = raw(lib.avs_get_octree_cells, s.h, 0, [None] * 4, capi.MEM_HOST)
            results[r] = (a, b, c)
        except Exception as e:  # pragma: no cover
            import traceback
            errors.append((r, e, traceback.format_exc()))

    th = [threading.Thread(target=rank_fn, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errors, errors
    for res in results:
        assert res is not None
        for st, _, _, err in res:
            assert st == capi.ESTATE and err
    for s, pp in objs:
        s.close()
        pp.close()
    lib.avs_local_group_destroy(grp)
