"""CU-resident PCG with LOCAL VALUE TABLES (AVS_OPTION_RESIDENT_LOCAL_TABLES, k_cg_resident<.., true>, k_resident_local_tables in
csrc/avs_pcg_resident.inl): matrices without one small dictionary -- a viscosity field, a sampled density -- run the resident loop
with a value table per workgroup (or per wave) built by the plan.  Opt-in: without the option they are refused as before
(tests/test_gpu_resident.py::test_resident_refuses_what_does_not_fit).  The bars are the resident loop's own (tests/test_gpu_resident.py,
tests/test_gpu_resident_f32.py).  Scenes of at most 128^3."""
import ctypes as C

import numpy as np
import pytest
import torch

from adaptiveviscositysolver_amd import ViscositySolve, capi, scenes
from util import build_pyramid, feed, oracle_from_pyramid, rel_l2

pytestmark = pytest.mark.gpu

CASES = {
    "beam64_L3_varvisc": lambda: scenes.fat_beam(64, 3, variable_viscosity=True),            # 83,740 rows, 3,667 distinct values
    "beam128_L3_varvisc": lambda: scenes.fat_beam(128, 3, variable_viscosity=True),          # 380,088 rows, 7,659
    "sphere_obstacle_rho_usolid": lambda: scenes.with_sampled_fields(scenes.sphere_with_obstacle(64, 4)),   # 59,527 rows, 21,886
}


def _context(sc, local_tables=None, precision=None, world_1=False, options=()):
    dsc = scenes.to_device(sc, torch.device("cuda:0"))
    pyr = build_pyramid(dsc)
    kw = {} if precision is None else {"precision": precision}
    s = ViscositySolve(sc.res, sc.dx, sc.dt, pyr.levels, device=0, field_res=sc.field_res, **kw)
    feed(s, pyr)
    s.set_scene_fields(scenes.crop_to_field(dsc))
    if local_tables is not None:
        s.set_solver_option(capi.OPTION_RESIDENT_LOCAL_TABLES, local_tables)
    for k, v in options:
        s.set_solver_option(k, v)
    if world_1:
        buf = (C.c_uint8 * capi.UNIQUE_ID_BYTES)()
        capi.check(s.lib.avs_dist_get_unique_id(buf))
        capi.check(s.lib.avs_dist_init(s.h, buf, 0, 1))
    s.assemble()
    return s, pyr


def test_default_is_unchanged(built_lib):
    """option untouched: a viscosity field keeps the launch-per-phase loop"""
    s, _ = _context(CASES["beam64_L3_varvisc"]())
    info = s.solve(1e-3, 2500)
    assert info.resident == 0 and info.converged == 1
    s.close()


@pytest.mark.parametrize("name", list(CASES))
def test_local_tables_solve_matches_oracle(name, built_lib):
    sc = CASES[name]()
    s, pyr = _context(sc, local_tables=1)
    o = oracle_from_pyramid(sc, pyr)
    o.hot_path()
    for tol in (1e-10, 1e-3):
        info = s.solve(tol, 5000)
        assert info.resident == 1, "the resident loop did not run (the plan declined?)"
        xo, io = o.solve(tol, 5000)
        print(f"{name} tol {tol:g}: iterations {info.iterations} (oracle {io.iterations}), error {info.error:.3e}")
        assert info.converged == 1 and info.error <= tol
        assert abs(info.iterations - io.iterations) <= max(3, io.iterations // 100), (info.iterations, io.iterations)
        if tol < 1e-6:
            d = rel_l2(s.solution(), xo)
            print(f"{name}: rel L2 to the oracle {d:.3e}")
            assert d < 1e-7
    x_res = s.solution()
    s.set_solver_option(capi.OPTION_RESIDENT_LOOP, 0)    # the same context through the launch-per-phase loop
    info2 = s.solve(1e-3, 5000)
    assert info2.resident == 0
    assert rel_l2(s.solution(), x_res) < 1e-2 * 1e-3 * 50   # both within tol of the same solution
    s.close()


def test_uniform_systems_run_the_ordinary_plan(built_lib):
    """one small dictionary: the option changes nothing -- same iteration count, same solution bits"""
    sc = scenes.fat_beam(64, 3, wall=True)
    out = []
    for opt in (0, 1):
        s, _ = _context(sc, local_tables=opt)
        info = s.solve(1e-10, 5000)
        assert info.resident == 1 and info.converged == 1
        out.append((info.iterations, np.array(s.solution(), copy=True)))
        s.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1].view(np.int64), out[1][1].view(np.int64))


@pytest.mark.parametrize("mode", ["long_rows", "streamed_rows", "bitmap_passes", "few_large_workgroups"])
def test_local_tables_plan_edges(mode, monkeypatch, built_lib):
    """long rows: 4 register quads per lane, every transition row reads its tail from memory (test_resident_long_row_path); streamed
    rows: the 128^3 beam on 64 CUs with a 64 K-column bitmap chunk (test_resident_streamed_rows) -- workgroups of ~6 k rows, whose
    tables do not fit the word next to 14 column bits, so this is also the per-wave granularity; bitmap passes: 16 K-column chunks on
    the 64^3 beam (six passes); few large workgroups: the 64^3 beam on 64 CUs.  Against the launch-per-phase loop of the same context."""
    big = mode == "streamed_rows"
    if mode == "long_rows":
        monkeypatch.setenv("AVS_CG_RESIDENT_MAX_QUADS", "4")
    elif mode == "streamed_rows":
        monkeypatch.setenv("AVS_CG_RESIDENT_CUS", "64")
        monkeypatch.setenv("AVS_CG_RESIDENT_REMAP_CHUNK", "65536")
    elif mode == "bitmap_passes":
        monkeypatch.setenv("AVS_CG_RESIDENT_REMAP_CHUNK", "16384")
    else:
        monkeypatch.setenv("AVS_CG_RESIDENT_CUS", "64")
    sc = scenes.fat_beam(128 if big else 64, 3, variable_viscosity=True)
    s, _ = _context(sc, local_tables=1)
    if mode == "long_rows":
        assert int(np.diff(s.csr()[0]).max()) > 20
    info = s.solve(1e-9, 5000)
    x = np.array(s.solution(), copy=True)
    assert info.resident == 1 and info.converged == 1 and info.error <= 1e-9
    s.set_solver_option(capi.OPTION_RESIDENT_LOOP, 0)
    lpp = s.solve(1e-9, 5000)
    assert lpp.resident == 0 and lpp.converged == 1
    print(f"{mode}: iterations {info.iterations} (launch-per-phase {lpp.iterations}), rel L2 between them {rel_l2(x, s.solution()):.3e}")
    assert abs(info.iterations - lpp.iterations) <= max(3, lpp.iterations // 100), (info.iterations, lpp.iterations)
    assert rel_l2(x, s.solution()) < 1e-7
    s.close()


def test_local_tables_are_deterministic(built_lib):
    """two fresh contexts: the same tables and words, hence the same iteration count and solution bits"""
    sc = CASES["sphere_obstacle_rho_usolid"]()
    out = []
    for _ in range(2):
        s, _ = _context(sc, local_tables=1)
        info = s.solve(1e-9, 5000)
        assert info.resident == 1 and info.converged == 1
        out.append((info.iterations, np.array(s.solution(), copy=True)))
        s.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])


def test_local_tables_follow_a_reassembly(built_lib):
    """test_resident_plan_follows_a_reassembly with a changed viscosity FIELD and the same DOF count: the tables and the words of the
    plan belong to the old values and must be rebuilt"""
    sc = scenes.fat_beam(64, 3, variable_viscosity=True)
    s, _ = _context(sc, local_tables=1)
    assert s.solve(1e-9, 5000).resident == 1
    x1 = s.solution()
    visc = scenes.to_device(sc, torch.device("cuda:0")).viscosity
    s.set_field(capi.FIELD_VISCOSITY, 0, (visc.flip(2) * 0.01).contiguous())     # the gradient reversed, 100x smaller
    s.assemble()
    info = s.solve(1e-9, 5000)
    assert info.resident == 1 and info.converged == 1
    x2 = s.solution()
    s.set_solver_option(capi.OPTION_RESIDENT_LOOP, 0)
    ref = s.solve(1e-9, 5000)
    assert ref.resident == 0 and abs(ref.iterations - info.iterations) <= 2
    assert rel_l2(x2, s.solution()) < 1e-7
    assert rel_l2(x2, x1) > 1e-6                              # (it is another system)
    s.close()


def test_local_tables_float_vectors(built_lib):
    """AVS_PRECISION_F32, RESIDENT_F32 = 1: k_cg_resident<.., float, true> against the float launch-per-phase loop of the same context
    (the margins of test_gpu_resident_f32.py::test_resident_float_plan_edges)"""
    tol = 1e-5
    sc = CASES["beam128_L3_varvisc"]()
    s, _ = _context(sc, local_tables=1, precision=capi.PRECISION_F32, options=((capi.OPTION_RESIDENT_F32, 1),))
    info = s.solve(tol, 5000)
    x = np.array(s.solution(), copy=True)
    assert info.resident == 1 and info.converged == 1 and int(s.matrix_format().float_vectors) == 1
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    s.set_solver_option(capi.OPTION_RESIDENT_F32, 0)
    s.set_solver_option(capi.OPTION_F32_VECTORS, 1)
    lpp = s.solve(tol, 5000)                                  # the launch-per-phase float loop
    x_lpp = np.array(s.solution(), copy=True)
    assert lpp.resident == 0 and lpp.converged == 1
    s.set_solver_option(capi.OPTION_RESIDENT_LOOP, 0)
    s.set_solver_option(capi.OPTION_F32_VECTORS, 0)           # the fp64 iteration on the same float system, far below float accuracy
    r64 = s.solve(1e-9, 8000)
    assert r64.converged == 1
    x64 = np.array(s.solution(), copy=True)
    e_res, e_lpp = rel_l2(x, x64), rel_l2(x_lpp, x64)
    print(f"float vectors: iterations {info.iterations} (launch-per-phase float {lpp.iterations}); error vs fp64: {e_res:.2e} / {e_lpp:.2e}")
    assert abs(info.iterations - lpp.iterations) <= max(3, int(0.03 * lpp.iterations)), (info.iterations, lpp.iterations)
    assert e_res <= max(1.5 * e_lpp, 5e-5), (e_res, e_lpp)
    s.close()


def test_local_tables_direct_transport_world_1(built_lib):
    """the partitioned path (direct transport, one rank) plans the rank's local system the same way"""
    sc = CASES["beam128_L3_varvisc"]()
    s, _ = _context(sc, local_tables=1, world_1=True)
    ref = s.solve(1e-9, 5000)
    xref = s.solution()
    assert ref.resident == 1 and ref.converged == 1
    s.dist_assemble()
    info = s.dist_solve(1e-9, 5000)
    assert info.resident == 1 and info.converged == 1 and abs(info.iterations - ref.iterations) <= 3
    assert rel_l2(s.dist_solution(), xref) < 1e-7
    info = s.dist_solve(1e-9, 5000)          # again: the plan is re-used
    assert info.resident == 1 and abs(info.iterations - ref.iterations) <= 3
    s.close()


def test_local_tables_across_ranks(tmp_path, built_lib):
    """two ranks as two processes on one GPU, 96 CUs each, direct transport (tests/hosted_rank_resident_local_tables.py): every rank
    plans its slab -- owned rows, halo columns -- with local tables"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    from hosted_rank_resident_local_tables import make_context
    tol, world, scene = 1e-9, 2, "beam64_varvisc"
    s = make_context(scene, torch.device("cuda:0"))
    s.set_solver_option(capi.OPTION_RESIDENT_LOCAL_TABLES, 1)
    s.assemble()
    ref = s.solve(tol, 5000)
    xref = np.array(s.solution(), copy=True)
    assert ref.resident == 1 and ref.converged == 1
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", AVS_DIST_TIMEOUT_MS="8000", AVS_CG_RESIDENT_CUS="96", AVS_RESIDENT_LOCAL_TABLES="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(here, "hosted_rank_resident_local_tables.py"), str(tmp_path), str(r), str(world),
                               scene, repr(tol)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(world)]
    outs = [p.communicate(timeout=200) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    x = np.zeros_like(xref)
    runs = set()
    for r in range(world):
        x += np.load(tmp_path / f"x_{r}.npy")
        it1, c1, res1, err1, it2, c2, res2, err2 = np.load(tmp_path / f"info_{r}.npy")
        assert res1 == 1 and res2 == 1, "the resident loop did not run on every rank"
        assert c1 == 1 and c2 == 1 and it1 == it2 and err1 == err2
        runs.add((int(it1), float(err1)))
    assert len(runs) == 1, runs          # every rank: the same iterations and the same error
    it = next(iter(runs))[0]
    d = rel_l2(x, xref)
    print(f"{scene}: ranks {runs}, single GPU {ref.iterations}; rel L2 to it {d:.2e}")
    assert abs(it - ref.iterations) <= 3 and d < 1e-7


def test_local_tables_through_seam_a(monkeypatch, built_lib):
    """avs_pcg_csr on the caller's CSR (no context: the environment is the option): the same plan from the caller's plain values"""
    from adaptiveviscositysolver_amd.solver import pcg_csr
    s, _ = _context(CASES["beam64_L3_varvisc"]())
    rp, col, val, rhs = s.csr()
    s.close()
    x0 = np.zeros_like(rhs)
    monkeypatch.delenv("AVS_RESIDENT_LOCAL_TABLES", raising=False)
    x_ref, ref = pcg_csr(rp, col, val, rhs, x0, 1e-9, 5000)
    assert ref.resident == 0 and ref.converged == 1
    monkeypatch.setenv("AVS_RESIDENT_LOCAL_TABLES", "1")
    x, info = pcg_csr(rp, col, val, rhs, x0, 1e-9, 5000)
    assert info.resident == 1 and info.converged == 1 and info.error <= 1e-9
    assert abs(info.iterations - ref.iterations) <= max(3, ref.iterations // 100), (info.iterations, ref.iterations)
    assert rel_l2(x, x_ref) < 1e-7
