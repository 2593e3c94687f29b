"""The pre-pass's "Apply Solid Weights" option (AVS_PREPASS_OPTION_APPLY_SOLID_WEIGHTS: the SOLID instantiations of the P1 kernels in
avs_prepass.hip) against its model (tests/solid_weights_model.py) and, downstream of the weights, against the oracle.  Everything is
compared bit for bit; nothing here has a tolerance."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import solid_weights_model as SM
from adaptiveviscositysolver_amd import DevicePrepass, ViscositySolve, capi, scenes
from oracle import oracle as O
from test_gpu_prepass import _same, _snapshot
from test_gpu_slab import _compare_window, _run_threads, _uniform_cuts
from util import oracle_for_scene

pytestmark = pytest.mark.gpu

ON = capi.PREPASS_OPTION_APPLY_SOLID_WEIGHTS
SCENES = {
    "beam_wall": lambda: scenes.fat_beam(32, 3, wall=True),
    "tank": lambda: scenes.tank(32, 3),
    "obstacle": lambda: scenes.sphere_with_obstacle(32, 3),
}


def _padded_case():
    """simulation grid 24 x 20 x 28 inside the 32^3 octree lattice: a liquid box clear of the grid's border on a ground plane in y"""
    fres, dx = (24, 20, 28), 1.0 / 32
    liquid = scenes.box_sdf(fres, dx, (12 * dx, 9 * dx, 14 * dx), (8 * dx, 6 * dx, 9 * dx))
    y = (torch.arange(fres[1], dtype=torch.float32) + 0.5) * dx
    solid = (6.3 * dx - y)[None, :, None].expand(fres[2], fres[1], fres[0]).to(torch.float32).contiguous()
    return liquid, solid, dx, fres


def _inputs(name):
    """(liquid, solid, dx, octree res, field_res or None) on the host"""
    if name == "planted":
        liquid, solid, dx = SM.planted_case()
        return liquid, solid, dx, (64, 32, 32), None
    if name == "padded":
        liquid, solid, dx, fres = _padded_case()
        return liquid, solid, dx, (32, 32, 32), fres
    sc = SCENES[name]()
    return sc.liquid, sc.solid, sc.dx, sc.res, None


_models = {}


def _model(name, n_super=3, ext=0.5, enabled=True, with_solid=True):
    key = (name, n_super, ext, enabled, with_solid)
    if key not in _models:
        liquid, solid, dx, res, fres = _inputs(name)
        if fres is not None:      # the SDFs are read with clamped coordinates outside their grid
            pad = (0, res[0] - fres[0], 0, res[1] - fres[1], 0, res[2] - fres[2])
            liquid, solid = (torch.nn.functional.pad(t[None, None], pad, mode="replicate")[0, 0].contiguous() for t in (liquid, solid))
        _models[key] = SM.solid_weights(liquid, solid if with_solid else None, dx, ext, n_super, enabled)
    return _models[key]


def _info_tuple(i):
    return (int(i.enabled), int(i.applied), float(i.extrapolation), [int(v) for v in i.modified], [int(v) for v in i.zeroed],
            [int(v) for v in i.above_one], [float(v) for v in i.max_weight], int(i.near_bricks))


def _assert_weights(pp, m, tag):
    def same(got, want, what):
        assert np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32)), (tag, what, int((got != want.numpy()).sum()))
    same(pp.weights(capi.FIELD_CENTER_WEIGHTS), m.center, "centre")
    for a in range(3):
        same(pp.weights(capi.FIELD_EDGE_WEIGHTS, a), m.edge[a], ("edge", a))
        same(pp.weights(capi.FIELD_FACE_WEIGHTS, a), m.face[a], ("face", a))
    got, want = _info_tuple(pp.solid_weights_info()), _info_tuple(m.info)
    print(tag, got)
    assert got == want, (tag, got, want)


PARITY = ([(name, 3, 0.5, "device") for name in ("beam_wall", "tank", "obstacle", "planted", "padded")]
          + [("tank", n, 0.5, "device") for n in (1, 2, 4)]
          + [("tank", 3, e, "device") for e in (0.0, 1.3)]
          + [("beam_wall", 3, 0.5, "host"), ("padded", 3, 0.5, "host")])


@pytest.mark.parametrize("name,n_super,ext,where", PARITY)
def test_weights_and_info_equal_the_model(name, n_super, ext, where, built_lib):
    """all seven lattices and every field of avs_solid_weights_info; a second run of the same object (far bricks skipped by the temporal
    reuse) reports the same numbers, and so does the run after the option went off and on again"""
    liquid, solid, dx, res, fres = _inputs(name)
    if where == "device":
        liquid, solid = liquid.cuda(), solid.cuda()
    else:
        liquid, solid = liquid.numpy(), solid.numpy()
    pp = DevicePrepass(res, dx, 3, n_super=n_super, extrapolation=ext, field_res=fres)
    pp.set_option(ON, 1)
    m = _model(name, n_super, ext)
    for frame in range(2):
        pp.run(liquid, solid)
        _assert_weights(pp, m, (name, n_super, ext, where, frame))
    assert m.info.applied == 1 and sum(m.info.modified) > 0
    pp.set_option(ON, 0)
    pp.run(liquid, solid)
    _assert_weights(pp, _model(name, n_super, ext, enabled=False), (name, "off"))
    pp.set_option(ON, 1)
    pp.run(liquid, solid)
    _assert_weights(pp, m, (name, "on again"))
    pp.close()


def test_off_means_off_and_toggling_is_invisible(built_lib):
    """Option 0, and option 1 without a solid SDF, give the bytes of an object the option was never set on.  Then ONE object runs a
    sequence of different scenes with the option off, on, on, off, on -- applies in between, so that its allocations alternate and the brick
    records of one setting meet runs of the other -- and equals a fresh object per frame: every lattice, every pyramid, the counts."""
    dev = torch.device("cuda:0")
    tank = scenes.to_device(scenes.tank(32, 3), dev)
    plain = DevicePrepass(tank.res, tank.dx, 3)
    pinfo = plain.run(tank.liquid, tank.solid)
    want = _snapshot(plain, pinfo.levels)
    for value, solid in ((0, tank.solid), (1, None)):
        pp = DevicePrepass(tank.res, tank.dx, 3)
        pp.set_option(ON, value)
        ref = plain
        if solid is None:
            ref = DevicePrepass(tank.res, tank.dx, 3)
            ref.run(tank.liquid, None)
        info = pp.run(tank.liquid, solid)
        _same(_snapshot(pp, info.levels), want if solid is not None else _snapshot(ref, info.levels))
        si = pp.solid_weights_info()
        assert (si.enabled, si.applied) == (value, 0) and _info_tuple(si)[3:7] == ([0] * 4, [0] * 4, [0] * 4, [0.0] * 4)
        pp.close()
    plain.close()

    frames = [scenes.tank(32, 3), scenes.fat_beam(32, 3, wall=True), scenes.sphere_with_obstacle(32, 3), scenes.tank(32, 3),
              scenes.fat_beam(32, 3, wall=True), scenes.fat_beam(32, 3), scenes.tank(32, 3)]
    options = [0, 1, 1, 0, 1, 1, 1]
    assert len({f.dx for f in frames}) == 1 and frames[5].solid is None
    pp = DevicePrepass((32, 32, 32), frames[0].dx, 3)
    held = []
    changed = 0
    for k, (sc_h, opt) in enumerate(zip(frames, options)):
        sc = scenes.to_device(sc_h, dev)
        pp.set_option(ON, opt)
        info = pp.run(sc.liquid, sc.solid)
        fresh = DevicePrepass(sc.res, sc.dx, 3)
        fresh.set_option(ON, opt)
        finfo = fresh.run(sc.liquid, sc.solid)
        assert (info.levels, info.n_velocity, info.n_edge, info.n_center, info.n_regular) == \
               (finfo.levels, finfo.n_velocity, finfo.n_edge, finfo.n_center, finfo.n_regular), k
        _same(_snapshot(pp, info.levels), _snapshot(fresh, finfo.levels))
        assert _info_tuple(pp.solid_weights_info()) == _info_tuple(fresh.solid_weights_info()), k
        changed += pp.solid_weights_info().applied
        fresh.close()
        if k != 2:     # (frame 2 is not applied: the next run then refills the SAME allocations)
            s = ViscositySolve(sc.res, sc.dx, sc.dt, info.levels, device=0)
            pp.apply(s)
            s.set_scene_fields(sc)
            s.assemble()
            held.append((s, [x.copy() for x in s.csr()]))
        for s, csr in held[-3:]:      # what was lent keeps the frame it was lent in
            s.assemble()
            for got, w in zip(s.csr(), csr):
                assert np.array_equal(got, w), k
    assert changed == 4
    pp.close()
    for s, _ in held:
        s.close()


@pytest.mark.parametrize("name", ["tank", "beam_wall"])
def test_downstream_of_the_scaled_weights_equals_the_oracle(name, built_lib):
    """The oracle never applies solid weights, but its entry points accept preset ones: it gets the device's scaled centre and edge weights
    (its own face weights), then builds octree and indices itself.  Labels, index pyramids and DOF counts equal the device's; after apply
    and assemble the CSR, rhs and x0 equal the oracle's hot path bit for bit; the device checkers pass and a solve converges to the error
    it claims."""
    dev = torch.device("cuda:0")
    sc_h = SCENES[name]()
    sc = scenes.to_device(sc_h, dev)
    off = DevicePrepass(sc.res, sc.dx, sc.levels)
    off_info = off.run(sc.liquid, sc.solid)
    off_counts = (off_info.n_velocity, off_info.n_edge, off_info.n_center)
    off.close()
    pp = DevicePrepass(sc.res, sc.dx, sc.levels)
    pp.set_option(ON, 1)
    info = pp.run(sc.liquid, sc.solid)
    o = oracle_for_scene(sc_h)
    o.build_weights(3, True)
    for a in range(3):
        assert np.array_equal(pp.weights(capi.FIELD_FACE_WEIGHTS, a).ravel(), o.get_field(O.F_FACEW + a))
        o.set_field(O.F_EDGEW + a, pp.weights(capi.FIELD_EDGE_WEIGHTS, a))
    o.set_field(O.F_CENTERW, pp.weights(capi.FIELD_CENTER_WEIGHTS))
    o.build_octree(0.5)
    o.build_indices(0.5)
    assert info.levels == o.levels
    counts = (info.n_velocity, info.n_edge, info.n_center)
    assert counts == (o.count(0), o.count(1), o.count(2))
    print(name, "DOFs off", off_counts, "on", counts)
    if name == "tank":
        assert counts != off_counts
    assert np.array_equal(pp.mask(), o.mask())
    for l in range(o.levels):
        assert np.array_equal(pp.labels(l), o.labels(l)), l
        for a in range(3):
            assert np.array_equal(pp.index(capi.INDEX_VELOCITY, l, a), o.index(O.I_VELOCITY, l, a)), (l, a)
            assert np.array_equal(pp.index(capi.INDEX_EDGE, l, a), o.index(O.I_EDGE, l, a)), (l, a)
        assert np.array_equal(pp.index(capi.INDEX_CENTER, l), o.index(O.I_CENTER, l)), l
    assert pp.check_octree().passed and pp.check_stress_indices().passed
    s = ViscositySolve(sc.res, sc.dx, sc.dt, info.levels, device=0)
    pp.apply(s)
    s.set_scene_fields(sc)
    s.assemble()
    o.hot_path()
    A = o.csr()
    rp, col, val, rhs = s.csr()
    assert np.array_equal(rp, A.row_ptr.astype(np.int32)) and np.array_equal(col, A.col)
    assert np.array_equal(val, A.val) and np.array_equal(rhs, A.rhs)
    assert np.array_equal(s.initial_guess(), o.initial_guess())
    # all rules; symmetry at the suite's bar (tests/test_gpu_refine.py, test_oracle_known_answers.py): 1e-12 of the largest entry.  The
    # matrix carries the oracle's bits (above), so what asymmetry there is -- rounding of products with weights like 27/26 -- is the
    # reference arithmetic's own.
    exact = s.check_system()
    print(name, "asymmetric entries", exact.asymmetric_entries, "max", exact.max_abs_asymmetry, "of", exact.max_abs_value)
    assert s.check_system(symmetry_tolerance=1e-12 * exact.max_abs_value).passed
    # a solve to 1e-8; the true residual (avs_check_solution, fp64 from the CSR) against the recurrence's claim: the two drift apart by
    # accumulated rounding only, an order of magnitude is the room given here (the suite's own scenes need 2.5x to 4.6x)
    tol = 1e-8
    sinfo = s.solve(tol, 3000)
    assert sinfo.converged == 1 and sinfo.error <= tol
    rep = s.check_solution()
    print(name, "claimed", sinfo.error, "true", rep.relative_residual, "iterations", sinfo.iterations)
    assert rep.evaluated and rep.claimed_error == sinfo.error and rep.relative_residual <= 10 * tol, rep
    s.close()
    pp.close()


@pytest.mark.parametrize("world", [2, 3])
def test_slab_windows_equal_the_single_rank_run(world, built_lib):
    """ranks cut along x on the 64^3 wall scene, the option on: inside a rank's window every lattice is the single-rank run's (the solid
    signs are gathered on the same brick box as the liquid's), and a rank reports the same counts frame after frame"""
    dev = torch.device("cuda:0")
    sc = scenes.to_device(scenes.fat_beam(64, 3, wall=True), dev)
    axis = 0
    pp = DevicePrepass(sc.res, sc.dx, sc.levels)
    pp.set_option(ON, 1)
    info = pp.run(sc.liquid, sc.solid)
    L = info.levels
    ref = {"labels": [pp.labels(l) for l in range(L)],
           "vidx": [[pp.index(capi.INDEX_VELOCITY, l, a) for a in range(3)] for l in range(L)],
           "eidx": [[pp.index(capi.INDEX_EDGE, l, a) for a in range(3)] for l in range(L)],
           "cidx": [pp.index(capi.INDEX_CENTER, l) for l in range(L)],
           "cw": [pp.weights(capi.FIELD_CENTER_WEIGHTS)],
           "ew": [pp.weights(capi.FIELD_EDGE_WEIGHTS, a) for a in range(3)],
           "fw": [pp.weights(capi.FIELD_FACE_WEIGHTS, a) for a in range(3)],
           "ridx": [pp.regular_index(a) for a in range(3)]}
    counts = (info.levels, info.n_velocity, info.n_edge, info.n_center, info.n_regular)
    whole = _info_tuple(pp.solid_weights_info())
    assert whole[1] == 1 and sum(whole[3]) > 0
    pp.set_option(ON, 0)
    off = pp.run(sc.liquid, sc.solid)
    assert (off.n_edge, off.n_center) != counts[2:4]     # (the option did change the system: stress samples inside the wall lost their DOFs)
    pp.close()
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
        rp = DevicePrepass(sc.res, sc.dx, sc.levels)
        rp.set_slab(axis, cuts, r, make_allreduce(r))
        rp.set_option(ON, 1)
        seen = []
        for frame in range(2):   # (the second frame runs on the temporal-reuse records)
            rinfo = rp.run(sc.liquid, sc.solid)
            assert (rinfo.levels, rinfo.n_velocity, rinfo.n_edge, rinfo.n_center, rinfo.n_regular) == counts, (r, frame)
            lo, hi, _ = rp.window()
            _compare_window(rp, ref, rinfo.levels, axis, lo, hi, sc.res)
            seen.append(_info_tuple(rp.solid_weights_info()))
        rp.close()
        assert seen[0] == seen[1] and seen[0][1] == 1
        return seen[0]

    res = _run_threads(world, rank_fn)
    for k in range(4):      # whole bricks of the windows: together they cover the lattice at least once
        assert sum(r[3][k] for r in res) >= whole[3][k] and all(r[3][k] <= whole[3][k] for r in res)
        assert max(r[6][k] for r in res) == whole[6][k]


def test_arguments(built_lib):
    dev = torch.device("cuda:0")
    sc = scenes.to_device(scenes.tank(32, 3), dev)
    lib = capi.load()
    pp = DevicePrepass(sc.res, sc.dx, sc.levels)
    # info before any run: all zero but the size
    first = pp.solid_weights_info()
    assert first.struct_size == C.sizeof(capi.SolidWeightsInfo)
    assert _info_tuple(first) == (0, 0, 0.0, [0] * 4, [0] * 4, [0] * 4, [0.0] * 4, 0)
    pp.set_option(ON, 1)
    assert pp.solid_weights_info().enabled == 1 and pp.solid_weights_info().applied == 0
    for bad in (2.0, -1.0, 0.5, 1.0000001, float("nan"), float("inf"), float("-inf")):
        assert lib.avs_prepass_set_option(pp.h, ON, bad) == capi.EINVAL, bad
        assert lib.avs_last_error()
        assert pp.solid_weights_info().enabled == 1      # nothing changed
    assert lib.avs_prepass_set_option(pp.h, 2, 1.0) == capi.EINVAL
    pp.run(sc.liquid, sc.solid)
    full = pp.solid_weights_info()
    assert full.applied == 1 and full.modified[0] > 0
    # struct_size: too small is refused, a shorter struct gets only that many bytes
    raw = (C.c_ubyte * C.sizeof(capi.SolidWeightsInfo))()
    as_info = C.cast(raw, C.POINTER(capi.SolidWeightsInfo))
    for size in (0, 3, -1, 4097):
        as_info.contents.struct_size = size
        assert lib.avs_prepass_get_solid_weights_info(pp.h, as_info) == capi.EINVAL, size
    short = capi.SolidWeightsInfo.modified.offset + 8      # up to and including modified[0]
    C.memset(raw, 0xAB, len(raw))
    as_info.contents.struct_size = short
    capi.check(lib.avs_prepass_get_solid_weights_info(pp.h, as_info))
    assert bytes(raw[short:]) == b"\xab" * (len(raw) - short)
    assert bytes(raw[4:short]) == bytes(C.string_at(C.addressof(full), C.sizeof(full))[4:short])
    assert as_info.contents.struct_size == short and as_info.contents.modified[0] == full.modified[0]
    assert lib.avs_prepass_get_solid_weights_info(pp.h, None) == capi.EINVAL
    pp.close()
