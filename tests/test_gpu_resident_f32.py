"""The CU-resident PCG on float vectors (AVS_OPTION_RESIDENT_F32, k_cg_resident<.., float>, csrc/avs_pcg_resident.inl): the float
system of an AVS_PRECISION_F32 context iterated as Eigen's float CG does (HDK_Utilities.h:25-37, cpp:613-630), in the one cooperative
launch that takes systems which fit the chip.
* the default is unchanged: float contexts run the fp64 resident loop, or the launch-per-phase float loop with F32_VECTORS = 1;
* with the option: resident == 1 and float_vectors == 1, a float solution, repeatable bits, the oracle's float CG iteration count to a
  few per cent and its distance to the converged fp64 solution;
* the same recurrence as the partitioned float loop (world-1 direct transport), the streamed-row and long-row plans, switching the
  option on one context, the fault fallback to the launch-per-phase float loop, and two ranks as two processes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from adaptiveviscositysolver_amd import ViscositySolve, capi, scenes
from util import build_pyramid, feed, oracle_from_pyramid, rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-5
# (maker, iteration count pinned to the oracle's float CG).  On the scene equivalents the oracle's float CG -- its dots summed left to
# right in float over 0.5-0.8 M terms -- takes 906 / 832 iterations at 1e-5 where every GPU float loop, the launch-per-phase one
# included, takes 786 / 588-738 (their dots: a thread's terms in float, the rest in double).  There the count is pinned to the
# partitioned float loop with the same single-reduction recurrence (world-1 direct transport) instead; the accuracy bound stays the oracle's.
CASES = {
    "beam64_L3_wall": (lambda: scenes.fat_beam(64, 3, wall=True), True),
    "beam128_L3": (lambda: scenes.fat_beam(128, 3), True),                        # BASELINE configs[1]
    "hip_buckling": (lambda: scenes.viscous_buckling_scene(), False),            # its LDS is nearly full in fp64
    "viscous_beam_hip_coarse": (lambda: scenes.viscous_beam_scene(coarsen=2), False),
}
_ORACLE = {}   # oracle float CG runs, shared by the tests of this module


def _context(sc, probe=False, resident_f32=None, world_1=False):
    dsc = scenes.to_device(sc, torch.device("cuda:0"))
    pyr = build_pyramid(dsc)
    s = ViscositySolve(sc.res, sc.dx, sc.dt, pyr.levels, device=0, field_res=sc.field_res, probe=probe, precision=capi.PRECISION_F32)
    feed(s, pyr)
    s.set_scene_fields(scenes.crop_to_field(dsc))
    if resident_f32 is not None:
        s.set_solver_option(capi.OPTION_RESIDENT_F32, resident_f32)
    if world_1:   # a partitioned group of one rank (direct transport), as test_resident_direct_transport_world_1
        buf = (C.c_uint8 * capi.UNIQUE_ID_BYTES)()
        capi.check(s.lib.avs_dist_get_unique_id(buf))
        capi.check(s.lib.avs_dist_init(s.h, buf, 0, 1))
    s.assemble()
    return s, pyr


def _oracle_float_cg(name, sc, pyr):
    if name not in _ORACLE:
        o = oracle_from_pyramid(sc, pyr)
        o.L.orc_set_precision(o.h, 1)
        o.hot_path()
        xo, io = o.solve(TOL, 5000)
        _ORACLE[name] = (np.array(xo, copy=True), int(io.iterations))
    return _ORACLE[name]


def _is_float(x):
    return np.array_equal(x, x.astype(np.float32).astype(np.float64))


def _fp64_reference(s):
    """the fp64 iteration on the same float system, converged far below float accuracy (F32_VECTORS = 0: the fp64 resident loop)"""
    s.set_solver_option(capi.OPTION_F32_VECTORS, 0)
    info = s.solve(1e-9, 8000)
    assert info.converged == 1
    x = np.array(s.solution(), copy=True)
    s.set_solver_option(capi.OPTION_F32_VECTORS, -1)
    return x


def test_default_stays_the_same(built_lib):
    sc = scenes.fat_beam(64, 3)
    s, _ = _context(sc)
    info = s.solve(TOL, 5000)
    assert info.converged == 1 and info.resident == 1 and int(s.matrix_format().float_vectors) == 0   # fp64 resident loop
    s.set_solver_option(capi.OPTION_F32_VECTORS, 1)
    s.set_solver_option(capi.OPTION_RESIDENT_F32, 0)
    info = s.solve(TOL, 5000)
    assert info.converged == 1 and info.resident == 0 and int(s.matrix_format().float_vectors) == 1   # launch-per-phase float loop
    s.close()


@pytest.mark.parametrize("name", list(CASES))
def test_resident_float_loop_against_the_oracle_float_cg(name, built_lib):
    make, pin_to_oracle = CASES[name]
    sc = make()
    s, pyr = _context(sc, resident_f32=1, world_1=not pin_to_oracle)
    info = s.solve(TOL, 5000)
    x = np.array(s.solution(), copy=True)
    assert info.resident == 1 and int(s.matrix_format().float_vectors) == 1, "the float resident loop did not run"
    assert info.converged == 1 and _is_float(x)                                  # Eigen::VectorXf
    again = s.solve(TOL, 5000)                                                   # fixed reduction order: same count, same bits
    assert again.resident == 1 and again.iterations == info.iterations and np.array_equal(s.solution().view(np.int64), x.view(np.int64))
    xo, io = _oracle_float_cg(name, sc, pyr)
    x64 = _fp64_reference(s)
    if pin_to_oracle:
        want = io
    else:
        s.set_solver_option(capi.OPTION_DIST_F32_VECTORS, 1)
        s.set_solver_option(capi.OPTION_RESIDENT_F32, 0)
        s.dist_assemble()
        sr = s.dist_solve(TOL, 5000)
        assert sr.converged == 1 and sr.resident == 0 and int(s.matrix_format().float_vectors) == 1
        want = sr.iterations
    e_gpu, e_orc = rel_l2(x, x64), rel_l2(xo, x64)
    print(f"{name}: iterations {info.iterations} (oracle float CG {io}, reference {want}); error vs the converged fp64 solution: "
          f"resident float {e_gpu:.2e}, oracle float CG {e_orc:.2e}")
    assert abs(info.iterations - want) <= max(3, int(0.03 * want)), (info.iterations, want, io)
    assert e_gpu <= max(1.5 * e_orc, 5e-5), (e_gpu, e_orc)
    s.close()


def test_same_recurrence_as_the_partitioned_float_loop(built_lib):
    """world-1 direct transport, DIST_F32_VECTORS = 1 without the resident loop: the same Chronopoulos-Gear float iteration,
    only the order of additions inside the dot products differs"""
    sc = scenes.fat_beam(64, 3)
    s, _ = _context(sc, resident_f32=1, world_1=True)
    ref = s.solve(TOL, 5000)
    xref = np.array(s.solution(), copy=True)
    assert ref.resident == 1 and int(s.matrix_format().float_vectors) == 1
    s.set_solver_option(capi.OPTION_RESIDENT_F32, 0)
    s.set_solver_option(capi.OPTION_DIST_F32_VECTORS, 1)      # (latched by the partition below)
    s.dist_assemble()
    info = s.dist_solve(TOL, 5000)
    assert info.resident == 0 and info.converged == 1 and int(s.matrix_format().float_vectors) == 1
    assert abs(info.iterations - ref.iterations) <= 2, (info.iterations, ref.iterations)
    assert rel_l2(s.dist_solution(), xref) <= 1e-5
    s.close()


@pytest.mark.parametrize("mode", ["streamed_rows", "long_rows", "tiny_workgroups"])
def test_resident_float_plan_edges(mode, monkeypatch, built_lib):
    """streamed rows: the 128^3 beam on 64 CUs with a 64 K-column bitmap chunk (as test_resident_streamed_rows); long rows: 4 register
    quads per lane, every transition row reads its tail from memory (as test_resident_long_row_path); tiny workgroups: a 640-row system
    with ONE quad per lane -- one row per lane (most of them long rows) -- split over every CU: workgroups of 2-4 rows at every offset
    modulo 4, so the float write-through of u (16 B = 4 entries) has workgroups with fewer rows than entries before their first 16-B
    boundary"""
    if mode == "streamed_rows":
        monkeypatch.setenv("AVS_CG_RESIDENT_CUS", "64")
        monkeypatch.setenv("AVS_CG_RESIDENT_REMAP_CHUNK", "65536")
        sc = scenes.fat_beam(128, 3)
    elif mode == "long_rows":
        monkeypatch.setenv("AVS_CG_RESIDENT_MAX_QUADS", "4")
        sc = scenes.sphere(64, 4)
    else:
        monkeypatch.setenv("AVS_CG_RESIDENT_MAX_QUADS", "1")
        sc = scenes.fat_beam(8, 1)
    s, _ = _context(sc, resident_f32=1)
    if mode == "long_rows":
        assert int(np.diff(s.csr()[0]).max()) > 20
    if mode == "tiny_workgroups":
        assert len(s.csr()[0]) - 1 < 3 * 256
    info = s.solve(TOL, 5000)
    x = np.array(s.solution(), copy=True)
    assert info.resident == 1 and info.converged == 1 and int(s.matrix_format().float_vectors) == 1 and _is_float(x)
    s.set_solver_option(capi.OPTION_RESIDENT_F32, 0)
    s.set_solver_option(capi.OPTION_F32_VECTORS, 1)
    lpp = s.solve(TOL, 5000)                                  # the launch-per-phase float loop
    x_lpp = np.array(s.solution(), copy=True)
    assert lpp.resident == 0 and lpp.converged == 1
    assert abs(info.iterations - lpp.iterations) <= max(3, int(0.03 * lpp.iterations)), (info.iterations, lpp.iterations)
    x64 = _fp64_reference(s)
    e_res, e_lpp = rel_l2(x, x64), rel_l2(x_lpp, x64)
    print(f"{mode}: iterations {info.iterations} (launch-per-phase float {lpp.iterations}); error vs fp64: {e_res:.2e} / {e_lpp:.2e}")
    assert e_res <= max(1.5 * e_lpp, 5e-5), (e_res, e_lpp)
    assert rel_l2(x, x_lpp) <= 5e-5 + 2 * e_lpp
    s.close()


def test_option_switch_on_one_context(built_lib):
    """RESIDENT_F32 1 -> 0 -> 1 between solves, no re-assembly: the plan is laid out again for each vector type"""
    sc = scenes.fat_beam(64, 3, wall=True)
    s, _ = _context(sc, resident_f32=1)
    a = s.solve(TOL, 5000)
    xa = np.array(s.solution(), copy=True)
    assert a.resident == 1 and int(s.matrix_format().float_vectors) == 1
    s.set_solver_option(capi.OPTION_RESIDENT_F32, 0)
    b = s.solve(TOL, 5000)
    xb = np.array(s.solution(), copy=True)
    assert b.resident == 1 and int(s.matrix_format().float_vectors) == 0
    s.set_solver_option(capi.OPTION_RESIDENT_F32, 1)
    c = s.solve(TOL, 5000)
    assert c.resident == 1 and int(s.matrix_format().float_vectors) == 1
    assert c.iterations == a.iterations and np.array_equal(s.solution().view(np.int64), xa.view(np.int64))
    s.close()
    # the fp64 solve in between is the one a context that never saw the option computes, bit for bit
    f, _ = _context(sc)
    d = f.solve(TOL, 5000)
    assert d.resident == 1 and d.iterations == b.iterations and np.array_equal(f.solution().view(np.int64), xb.view(np.int64))
    f.close()


def test_fault_is_redone_by_the_float_launch_per_phase_loop(monkeypatch, built_lib):
    """AVS_CG_RESIDENT_FAKE_FAULT (probe build): the float resident launch counts as faulted, the same call restores the initial guess and
    solves with pcg_solve_phases<float> -- exactly what F32_VECTORS = 1 without the option computes"""
    sc = scenes.fat_beam(64, 3)
    s, _ = _context(sc, probe=True, resident_f32=1)
    good = s.solve(TOL, 5000)          # the float plan is built and its kernel launched on this very context ...
    assert good.converged == 1 and good.resident == 1 and int(s.matrix_format().float_vectors) == 1
    monkeypatch.setenv("AVS_CG_RESIDENT_FAKE_FAULT", "1")
    info = s.solve(TOL, 5000)          # ... so this solve launches it again, and the hook marks that launch faulted
    x = np.array(s.solution(), copy=True)
    monkeypatch.delenv("AVS_CG_RESIDENT_FAKE_FAULT")
    assert info.converged == 1 and info.resident == 0 and int(s.matrix_format().float_vectors) == 1
    again = s.solve(TOL, 5000)         # the fault branch retired the plan: the context stays on the launch-per-phase float loop
    assert again.converged == 1 and again.resident == 0 and again.iterations == info.iterations
    s.close()
    p, _ = _context(sc, probe=True, resident_f32=0)
    p.set_solver_option(capi.OPTION_F32_VECTORS, 1)
    ref = p.solve(TOL, 5000)
    assert ref.resident == 0 and ref.iterations == info.iterations
    assert np.array_equal(p.solution().view(np.int64), x.view(np.int64))
    p.close()


@pytest.mark.parametrize("scene", ["beam64", "hip_beam_coarse"])
def test_resident_float_loop_across_ranks(scene, tmp_path, built_lib):
    """two ranks as two processes on one GPU, 96 CUs each, direct transport (tests/hosted_rank_resident_f32.py)"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from hosted_rank_resident_f32 import make_context
    tol, world = 1e-6, 2
    s = make_context(scene, torch.device("cuda:0"))
    s.set_solver_option(capi.OPTION_RESIDENT_F32, 1)
    s.assemble()
    ref = s.solve(tol, 5000)
    xref = np.array(s.solution(), copy=True)
    assert ref.resident == 1 and ref.converged == 1 and int(s.matrix_format().float_vectors) == 1
    s.close()
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", AVS_DIST_TIMEOUT_MS="8000", AVS_CG_RESIDENT_CUS="96",
               AVS_DIST_F32_VECTORS="1", AVS_RESIDENT_F32="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(here, "hosted_rank_resident_f32.py"), str(tmp_path), str(r), str(world), scene,
                               repr(tol)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(world)]
    outs = [p.communicate(timeout=200) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    x = np.zeros_like(xref)
    runs = set()
    for r in range(world):
        x += np.load(tmp_path / f"x_{r}.npy")
        it1, c1, res1, err1, it2, c2, res2, err2, fv = np.load(tmp_path / f"info_{r}.npy")
        assert res1 == 1 and res2 == 1, "the float resident loop did not run on every rank"
        assert c1 == 1 and c2 == 1 and it1 == it2 and err1 == err2 and fv == 1
        runs.add((int(it1), float(err1)))
    assert len(runs) == 1, runs          # every rank: the same iterations and the same error
    assert _is_float(x)
    d = rel_l2(x, xref)
    print(f"{scene}: ranks {runs}, single-GPU float resident {ref.iterations}; rel L2 to it {d:.2e}")
    assert d <= 1e-5, d
