"""The pre-pass's fine layer bandwidth (avs_prepass_set_option) and indicator-driven refinement (avs_prepass_set_refinement) on the
device, against the model of tests/refine_model.py: the flags at every edge of the bit lattice, the pyramids of widened and flagged
masks bit for bit, the same pyramids down the pipeline against the oracle's hot path, on / off on one object, the solver's own shear
rate as the indicator, the refusals, and slab-local windows with flags set."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import refine_model as RM
from adaptiveviscositysolver_amd import DevicePrepass, ViscositySolve, capi, scenes
from test_gpu_slab import _compare_window, _run_threads, _uniform_cuts
from util import oracle_from_pyramid

pytestmark = pytest.mark.gpu

SCENES = {
    "beam32_L3": lambda dev: scenes.fat_beam(32, 3, device=dev),
    "beam64_L4": lambda dev: scenes.fat_beam(64, 4, device=dev),
    "beam64_wall": lambda dev: scenes.fat_beam(64, 3, wall=True, device=dev),
    "sphere64_L4": lambda dev: scenes.sphere(64, 4, device=dev),
    "noncubic": lambda dev: scenes.fat_beam(64, 3, res=(64, 32, 32), device=dev),
}
SETTINGS = [(3, None), (4, None), (6, None), (2, 0), (2, 1), (2, 3)]   # (bandwidth, dilate of the two-seed indicator or None)
THRESHOLD = 0.5


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. flags at their edges
# ---------------------------------------------------------------------------------------------------------------------------------
GRIDS = {   # octree grid, simulation grid
    "128x16x16": ((128, 16, 16), None),
    "16x16x16": ((16, 16, 16), None),            # rows shorter than a word
    "48x40x24_in_64x64x32": ((64, 64, 32), (48, 40, 24)),
}


def edge_indicator(fres):
    """seeds at the word and ballot boundaries along x and at the first and last y and z; NaN, -inf and a cell equal to the threshold
    (no seeds), +inf (a seed)"""
    nx, ny, nz = fres
    ind = np.zeros((nz, ny, nx), np.float32)
    for x in (0, 31, 32, 63, 64, nx - 1):
        if x < nx:
            ind[nz // 2, ny // 2, x] = 1.0
    ind[0, 0, nx // 3] = 2.0
    ind[nz - 1, ny - 1, nx // 3 + 1] = 3.0
    ind[0, ny - 1, nx - 1] = np.nextafter(np.float32(THRESHOLD), np.float32(1))
    ind[nz - 1, 0, 0] = np.inf
    ind[1, 1, 1] = np.nan
    ind[nz - 2, 1, nx - 2] = -np.inf
    ind[2, ny - 2, 2] = THRESHOLD
    return ind


@pytest.mark.parametrize("dilate", [0, 1, 16])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_flags_equal_the_model_at_every_edge(grid, dilate, built_lib):
    res, fres = GRIDS[grid]
    ind = edge_indicator(fres or res)
    want, n_seeds, n_flagged = RM.flags(ind, THRESHOLD, dilate, res)
    assert n_seeds == int((ind > THRESHOLD).sum()) >= 6
    pp = DevicePrepass(res, 1.0 / res[0], 2, field_res=fres)
    for field in (ind, torch.from_numpy(ind), torch.from_numpy(ind).to("cuda:0")):   # host (numpy, torch) and device memory
        pp.set_refinement(field, THRESHOLD, dilate)
        got = pp.refinement()
        assert got.shape == want.shape and np.array_equal(got, want)
        info = pp.refinement_info()
        assert (info.active, info.dilate_cells, info.threshold) == (1, dilate, THRESHOLD)
        assert (info.seeds, info.flagged) == (n_seeds, n_flagged)
        pp.set_refinement(None)
        assert not pp.refinement().any() and pp.refinement_info().active == 0
    if fres is not None:    # nothing outside the simulation grid, however far the dilation reaches
        assert not want[fres[2]:].any() and not want[:, fres[1]:].any() and not want[:, :, fres[0]:].any()
    # the device getter
    pp.set_refinement(ind, THRESHOLD, dilate)
    t = torch.full(want.shape, 7, dtype=torch.int8, device="cuda:0")
    capi.check(pp.lib.avs_prepass_get_refinement(pp.h, t.data_ptr(), capi.MEM_DEVICE))
    assert np.array_equal(t.cpu().numpy(), want)
    pp.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. + 3. pyramids, and the same pyramids down the pipeline
# ---------------------------------------------------------------------------------------------------------------------------------
_MODEL = {}


def model(name, bw, dil):
    """(device scene, flags or None, the model's pyramid on the device, the default mask): computed once, shared, left unchanged"""
    key = (name, bw, dil)
    if key not in _MODEL:
        sc = SCENES[name](torch.device("cuda:0"))
        fl = None if dil is None else RM.flags(RM.two_seed_indicator(sc.res), THRESHOLD, dil, sc.res)[0]
        pyr = RM.build_pyramid(sc, bandwidth=bw, flagged=fl, weights_key=name)
        _MODEL[key] = (sc, fl, pyr, RM.build_mask(sc.liquid, sc.solid, sc.dx))
    return _MODEL[key]


def configure(pp, sc, bw, dil):
    pp.set_option(capi.PREPASS_OPTION_FINE_BANDWIDTH, bw)
    pp.set_refinement(None if dil is None else RM.two_seed_indicator(sc.res), THRESHOLD, dil or 0)


def assert_pyramid(pp, info, pyr):
    assert info.levels == pyr.levels
    assert (info.n_velocity, info.n_edge, info.n_center) == (pyr.n_velocity, pyr.n_edge, pyr.n_center)
    assert np.array_equal(pp.mask(), pyr.mask.cpu().numpy())
    for l in range(pyr.levels):
        assert np.array_equal(pp.labels(l), pyr.labels[l].cpu().numpy()), l
        for a in range(3):
            assert np.array_equal(pp.index(capi.INDEX_VELOCITY, l, a), pyr.vidx[l][a].cpu().numpy()), (l, a)
            assert np.array_equal(pp.index(capi.INDEX_EDGE, l, a), pyr.eidx[l][a].cpu().numpy()), (l, a)
        assert np.array_equal(pp.index(capi.INDEX_CENTER, l), pyr.cidx[l].cpu().numpy()), l


@pytest.mark.parametrize("bw,dil", SETTINGS)
@pytest.mark.parametrize("name", list(SCENES))
def test_pyramids_equal_the_model(name, bw, dil, built_lib):
    sc, fl, pyr, default_mask = model(name, bw, dil)
    pp = DevicePrepass(sc.res, sc.dx, sc.levels)
    configure(pp, sc, bw, dil)
    info = pp.run(sc.liquid, sc.solid)
    assert_pyramid(pp, info, pyr)
    rinfo = pp.refinement_info()
    if dil is None:
        assert rinfo.active == 0 and rinfo.refined == 0
        assert int((pyr.mask != default_mask).sum()) > 0       # (the bandwidth did widen the fine layer)
    else:
        assert rinfo.refined == int((pyr.mask != default_mask).sum()) > 0
    pp.close()


@pytest.mark.parametrize("bw,dil", [(4, None), (2, 3)])
@pytest.mark.parametrize("name", list(SCENES))
def test_down_the_pipeline(name, bw, dil, built_lib):
    sc, fl, pyr, _ = model(name, bw, dil)
    pp = DevicePrepass(sc.res, sc.dx, sc.levels)
    configure(pp, sc, bw, dil)
    info = pp.run(sc.liquid, sc.solid)
    assert pp.check_octree().passed and pp.check_stress_indices().passed
    s = ViscositySolve(sc.res, sc.dx, sc.dt, info.levels, device=0)
    pp.apply(s)
    s.set_scene_fields(sc)
    s.assemble()
    o = oracle_from_pyramid(SCENES[name]("cpu"), pyr)
    o.hot_path()
    A = o.csr()
    rp, col, val, rhs = s.csr()
    assert np.array_equal(rp, A.row_ptr.astype(np.int32)) and np.array_equal(col, A.col)
    assert np.array_equal(val, A.val) and np.array_equal(rhs, A.rhs)
    # symmetry to 1e-12 of the largest entry: the bar of tests/test_gpu_csr_check.py and tests/test_oracle_known_answers.py (an entry and its
    # mirror are summed in different orders: A is symmetric to rounding, not bitwise, on the default octree too)
    exact = s.check_system()
    assert exact.evaluated == 255 and exact.violations[:7] == (0,) * 7, exact
    for rep in (s.check_octree(), s.check_stress_indices(), s.check_system(symmetry_tolerance=1e-12 * exact.max_abs_value)):
        assert rep.passed and not any(rep.violations), rep
    tol = 1e-8
    sinfo = s.solve(tol, 5000)
    assert sinfo.converged == 1
    rep = s.check_solution()
    print(name, bw, dil, "true relative residual", rep.relative_residual, "claimed", sinfo.error, "iterations", sinfo.iterations)
    assert rep.evaluated and rep.relative_residual < tol
    s.close()
    pp.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. off means off, and it is reversible
# ---------------------------------------------------------------------------------------------------------------------------------
def snapshot(pp, info):
    out = {"counts": np.asarray([info.levels, info.n_velocity, info.n_edge, info.n_center, info.n_regular]),
           "cw": pp.weights(capi.FIELD_CENTER_WEIGHTS), "mask": pp.mask()}
    for a in range(3):
        out[f"ew{a}"] = pp.weights(capi.FIELD_EDGE_WEIGHTS, a)
        out[f"fw{a}"] = pp.weights(capi.FIELD_FACE_WEIGHTS, a)
        out[f"r{a}"] = pp.regular_index(a)
    for l in range(info.levels):
        out[f"lab{l}"] = pp.labels(l)
        out[f"c{l}"] = pp.index(capi.INDEX_CENTER, l)
        for a in range(3):
            out[f"v{l}{a}"] = pp.index(capi.INDEX_VELOCITY, l, a)
            out[f"e{l}{a}"] = pp.index(capi.INDEX_EDGE, l, a)
    return out


def test_off_means_off_and_it_is_reversible(built_lib):
    """One object through default -> flagged -> bandwidth 4 -> cleared -> flagged -> cleared: after every run everything it holds equals
    what a fresh object with the same settings computes -- the fine region grows and shrinks under the index tiles' temporal reuse."""
    sc = SCENES["beam64_L4"](torch.device("cuda:0"))
    sequence = [(2, None), (2, 3), (4, None), (2, None), (2, 3), (2, None)]
    fresh = {}
    for bw, dil in set(sequence):
        f = DevicePrepass(sc.res, sc.dx, sc.levels)
        configure(f, sc, bw, dil)
        fresh[(bw, dil)] = snapshot(f, f.run(sc.liquid, sc.solid))
        f.close()
    assert not np.array_equal(fresh[(2, None)]["mask"], fresh[(2, 3)]["mask"]) and not np.array_equal(fresh[(2, None)]["mask"], fresh[(4, None)]["mask"])
    pp = DevicePrepass(sc.res, sc.dx, sc.levels)
    for k, (bw, dil) in enumerate(sequence):
        if k > 0:
            configure(pp, sc, bw, dil)
        got, want = snapshot(pp, pp.run(sc.liquid, sc.solid)), fresh[(bw, dil)]
        assert got.keys() == want.keys(), k
        for key in want:
            assert np.array_equal(got[key], want[key]), (k, key)
    pp.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. from the solver's own field
# ---------------------------------------------------------------------------------------------------------------------------------
def test_shear_rate_of_a_solve_refines_the_next_octree(built_lib):
    sc = SCENES["beam64_L4"](torch.device("cuda:0"))
    pp = DevicePrepass(sc.res, sc.dx, sc.levels)
    info = pp.run(sc.liquid, sc.solid)
    s = ViscositySolve(sc.res, sc.dx, sc.dt, info.levels, device=0)
    pp.apply(s)
    s.set_scene_fields(sc)
    s.assemble()
    assert s.solve(1e-8, 5000).converged == 1
    rate = s.shear_rate_field(device_array=True)
    host = rate.cpu().numpy()
    thr = float(np.quantile(host[sc.liquid.cpu().numpy() <= 0], 0.98))
    pp.set_refinement(rate, thr, 2)
    want, n_seeds, n_flagged = RM.flags(host, thr, 2, sc.res)
    assert n_seeds > 0
    assert np.array_equal(pp.refinement(), want)
    rinfo = pp.refinement_info()
    assert (rinfo.seeds, rinfo.flagged) == (n_seeds, n_flagged)
    pyr = RM.build_pyramid(sc, flagged=want, weights_key="beam64_L4")
    assert_pyramid(pp, pp.run(sc.liquid, sc.solid), pyr)
    assert pp.refinement_info().refined == int((pyr.mask != RM.build_mask(sc.liquid, sc.solid, sc.dx)).sum())
    s.close()
    pp.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. errors
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(built_lib):
    name, bw, dil = "beam32_L3", 2, 1
    sc, fl, pyr, _ = model(name, bw, dil)
    lib = capi.load()
    pp = DevicePrepass(sc.res, sc.dx, sc.levels)
    # before any set call: no flags
    assert not pp.refinement().any()
    first = pp.refinement_info()
    assert (first.active, first.seeds, first.flagged, first.refined) == (0, 0, 0, 0)
    ind = RM.two_seed_indicator(sc.res)
    pp.set_refinement(ind, THRESHOLD, dil)
    flags = pp.refinement()
    assert np.array_equal(flags, fl)
    state = lambda i: (i.active, i.dilate_cells, i.threshold, i.seeds, i.flagged, i.refined, i.set_ms)
    before = state(pp.refinement_info())
    other = np.ones_like(ind)
    for status in (lib.avs_prepass_set_option(pp.h, capi.PREPASS_OPTION_FINE_BANDWIDTH, float("nan")),
                   lib.avs_prepass_set_option(pp.h, capi.PREPASS_OPTION_FINE_BANDWIDTH, float("inf")),
                   lib.avs_prepass_set_option(pp.h, capi.PREPASS_OPTION_FINE_BANDWIDTH, float("-inf")),
                   lib.avs_prepass_set_option(pp.h, 1, 4.0),
                   lib.avs_prepass_set_option(pp.h, -1, 4.0),
                   lib.avs_prepass_set_refinement(pp.h, other.ctypes.data, 0.0, -1, capi.MEM_HOST),
                   lib.avs_prepass_set_refinement(pp.h, other.ctypes.data, 0.0, 17, capi.MEM_HOST),
                   lib.avs_prepass_set_refinement(pp.h, other.ctypes.data, 0.0, 1, 2),
                   lib.avs_prepass_set_refinement(pp.h, other.ctypes.data, 0.0, 1, -1)):
        assert status == capi.EINVAL
        assert lib.avs_last_error()
    out = np.zeros(flags.shape, np.int8)
    assert lib.avs_prepass_get_refinement(pp.h, out.ctypes.data, 2) == capi.EINVAL
    assert state(pp.refinement_info()) == before and np.array_equal(pp.refinement(), flags)
    with pytest.raises(ValueError):
        pp.set_refinement(ind[:-1], THRESHOLD, dil)
    # ... the bandwidth included: the next run is the one of bandwidth 2 and these flags
    assert_pyramid(pp, pp.run(sc.liquid, sc.solid), pyr)
    pp.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. slab-local windows
# ---------------------------------------------------------------------------------------------------------------------------------
def test_slab_windows_with_flags_equal_the_single_rank_run(built_lib):
    """Two ranks cut along x (the way tests/test_gpu_slab.py runs ranks on one GPU): the set call flags the whole lattice on every rank, a
    rank's window reads them, and inside it labels and index lattices are the single-rank run's; `refined` covers the window."""
    dev = torch.device("cuda:0")
    sc = scenes.fat_beam(64, 3, device=dev)
    world, axis, dil = 2, 0, 3
    ind = RM.two_seed_indicator(sc.res)
    ref_pp = DevicePrepass(sc.res, sc.dx, sc.levels)
    ref_pp.set_refinement(ind, THRESHOLD, dil)
    info = ref_pp.run(sc.liquid, sc.solid)
    L = info.levels
    ref = {"labels": [ref_pp.labels(l) for l in range(L)],
           "vidx": [[ref_pp.index(capi.INDEX_VELOCITY, l, a) for a in range(3)] for l in range(L)],
           "eidx": [[ref_pp.index(capi.INDEX_EDGE, l, a) for a in range(3)] for l in range(L)],
           "cidx": [ref_pp.index(capi.INDEX_CENTER, l) for l in range(L)],
           "cw": [ref_pp.weights(capi.FIELD_CENTER_WEIGHTS)],
           "ew": [ref_pp.weights(capi.FIELD_EDGE_WEIGHTS, a) for a in range(3)],
           "fw": [ref_pp.weights(capi.FIELD_FACE_WEIGHTS, a) for a in range(3)],
           "ridx": [ref_pp.regular_index(a) for a in range(3)]}
    counts = (info.levels, info.n_velocity, info.n_edge, info.n_center, info.n_regular)
    changed = ref_pp.mask() != RM.build_mask(sc.liquid, sc.solid, sc.dx).cpu().numpy()
    assert ref_pp.refinement_info().refined == int(changed.sum()) > 0
    # (the flags did change the octree: the default run differs)
    ref_pp.set_refinement(None)
    assert ref_pp.run(sc.liquid, sc.solid).n_velocity != counts[1]
    ref_pp.close()
    cuts = _uniform_cuts(sc.res[axis], world)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    barrier = threading.Barrier(world)
    shared = {}
    lock = threading.Lock()

    def make_allreduce(rank):
        def allreduce(ptr, count, stream):
            assert hip.hipStreamSynchronize(C.c_void_p(stream)) == 0
            mine = np.empty(count, np.int32)
            assert hip.hipMemcpy(mine.ctypes.data, C.c_void_p(ptr), count * 4, 2) == 0   # device to host
            barrier.wait()
            if rank == 0:
                shared["sum"] = np.zeros(count, np.int64)
            barrier.wait()
            with lock:
                shared["sum"] += mine
            barrier.wait()
            tot = shared["sum"].astype(np.int32)
            assert hip.hipMemcpy(C.c_void_p(ptr), tot.ctypes.data, count * 4, 1) == 0    # host to device
            barrier.wait()
        return allreduce

    def rank_fn(r):
        pp = DevicePrepass(sc.res, sc.dx, sc.levels)
        pp.set_slab(axis, cuts, r, make_allreduce(r))
        pp.set_refinement(ind, THRESHOLD, dil)
        refined = []
        for frame in range(2):   # (the second frame runs on the temporal-reuse records)
            rinfo = pp.run(sc.liquid, sc.solid)
            assert (rinfo.levels, rinfo.n_velocity, rinfo.n_edge, rinfo.n_center, rinfo.n_regular) == counts, (r, frame)
            lo, hi, _ = pp.window()
            _compare_window(pp, ref, rinfo.levels, axis, lo, hi, sc.res)
            assert pp.refinement_info().refined == int(changed[:, :, int(lo[0]):int(hi[0])].sum()), (r, frame)
            refined.append(pp.refinement_info().refined)
        pp.close()
        return refined

    res = _run_threads(world, rank_fn)
    assert sum(r[-1] for r in res) >= int(changed.sum())
