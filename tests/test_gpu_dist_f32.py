"""Partitioned solves of AVS_PRECISION_F32 contexts on float vectors (AVS_OPTION_DIST_F32_VECTORS = 1, csrc/avs_pcg.hip).

The single-GPU float loop (AVS_OPTION_F32_VECTORS = 1) iterates as Eigen's float CG does; with the option, the partitioned
single-reduction loops do the same over both transports.  Checked here:
* virtual ranks (in-process transport) and one process per rank (direct transport): every rank converges in the same iteration,
  reports float_vectors, returns float values, takes about as many iterations as the single-GPU float loop and is about as accurate
  against the fp64 loop on the same float system; a second solve repeats the count and the bits;
* without the option the partitioned F32 solve is the fp64 iteration it always was (float_vectors == 0, same bits as a context that
  never saw the option, the single-GPU fp64 loop's solution);
* a pending avs_cancel stops every rank before the first iteration."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from adaptiveviscositysolver_amd import ViscositySolve, capi, scenes
from util import build_pyramid, feed, rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-5
SCENES = {
    "beam64": lambda dev: scenes.fat_beam(64, 3, device=dev),
    "varvisc64": lambda dev: scenes.fat_beam(64, 3, variable_viscosity=True, device=dev),
    "beam128L4": lambda dev: scenes.fat_beam(128, 4, device=dev),
}


def _context(sc, pyr):
    s = ViscositySolve(sc.res, sc.dx, sc.dt, pyr.levels, device=0, precision=capi.PRECISION_F32)
    feed(s, pyr)
    s.set_scene_fields(sc)
    return s


def _single(sc, pyr, f32_vectors, tol):
    """single-GPU solve of the float system: the float loop (1) or the fp64 loop (0)"""
    s = _context(sc, pyr)
    s.set_solver_option(capi.OPTION_F32_VECTORS, f32_vectors)
    s.assemble()
    info = s.solve(tol, 5000)
    x = s.solution()
    fv = int(s.matrix_format().float_vectors)
    s.close()
    return info, x, fv


def _references(sc, pyr):
    info_f, x_f, fv = _single(sc, pyr, 1, TOL)
    assert fv == 1 and info_f.converged == 1
    _, x64, fv64 = _single(sc, pyr, 0, 1e-9)
    assert fv64 == 0
    return info_f.iterations, x_f, x64, rel_l2(x_f, x64)


def _partitioned(sc, pyr, world, mode, option=None, cancel=False, tol=TOL, solves=2):
    """world virtual ranks; option: value of AVS_OPTION_DIST_F32_VECTORS (None: never set).  Per rank: [(info, x, fmt)] per solve."""
    lib = capi.load()
    grp = C.c_void_p()
    capi.check(lib.avs_local_group_create(world, C.byref(grp)))
    solvers = [_context(sc, pyr) for _ in range(world)]
    results, errors = [None] * world, []

    def run(r):
        try:
            s = solvers[r]
            if option is not None:
                s.set_solver_option(capi.OPTION_DIST_F32_VECTORS, option)
            s.dist_init_local(grp, r)
            if mode == "partition":
                s.assemble()
                s.dist_partition()
            else:
                s.dist_assemble()
            out = []
            for _ in range(solves):
                if cancel:
                    capi.check(lib.avs_cancel(s.h))
                info = s.dist_solve(tol, 5000)
                out.append((info, s.dist_solution(), s.matrix_format()))
            results[r] = out
        except Exception as e:  # pragma: no cover
            errors.append((r, e))

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=240)
    for s in solvers:
        s.close()
    lib.avs_local_group_destroy(grp)
    assert not errors, errors
    assert all(r is not None for r in results)
    return results


def _check_float_run(results, iters_f, err_f, x64):
    its = set()
    for out in results:
        (i1, x1, f1), (i2, x2, _) = out
        assert i1.converged == 1 and i1.cancelled == 0
        assert int(f1.float_vectors) == 1
        assert np.array_equal(x1, x1.astype(np.float32).astype(np.float64))       # Eigen::VectorXf
        assert i2.iterations == i1.iterations and np.array_equal(x1.view(np.int64), x2.view(np.int64))
        its.add(i1.iterations)
        assert abs(i1.iterations - iters_f) <= max(3, int(0.03 * iters_f)), (i1.iterations, iters_f)
        assert rel_l2(x1, x64) <= max(2 * err_f, 5e-5), (rel_l2(x1, x64), err_f)
    assert len(its) == 1   # every rank stops in the same iteration


@pytest.mark.parametrize("scene,world,mode", [("beam64", 2, "partition"), ("varvisc64", 3, "partition"), ("beam128L4", 2, "assemble")])
def test_virtual_ranks_iterate_on_float_vectors(scene, world, mode, monkeypatch, built_lib):
    monkeypatch.setenv("AVS_BRICK", "1")   # (beam128L4 through avs_dist_assemble: the brick form of the local rows, float kernel)
    sc = SCENES[scene](torch.device("cuda:0"))
    pyr = build_pyramid(sc)
    iters_f, _, x64, err_f = _references(sc, pyr)
    results = _partitioned(sc, pyr, world, mode, option=1)
    _check_float_run(results, iters_f, err_f, x64)
    if scene == "beam128L4":
        assert all(int(out[0][2].brick_tiles) > 0 for out in results)


def test_default_partitioned_f32_solve_is_unchanged(built_lib):
    sc = SCENES["beam64"](torch.device("cuda:0"))
    pyr = build_pyramid(sc)
    _, x64, _ = _single(sc, pyr, 0, 1e-10)
    never = _partitioned(sc, pyr, 2, "partition", option=None, tol=1e-10, solves=1)
    off = _partitioned(sc, pyr, 2, "partition", option=0, tol=1e-10, solves=1)
    for a, b in zip(never, off):
        (ia, xa, fa), = a
        (ib, xb, fb), = b
        assert int(fa.float_vectors) == 0 and int(fb.float_vectors) == 0
        assert ia.converged == 1 and ia.iterations == ib.iterations
        assert np.array_equal(xa.view(np.int64), xb.view(np.int64))
        assert rel_l2(xa, x64) < 1e-8


def test_pending_cancel_stops_every_rank(built_lib):
    sc = SCENES["beam64"](torch.device("cuda:0"))
    pyr = build_pyramid(sc)
    results = _partitioned(sc, pyr, 2, "partition", option=1, cancel=True, solves=1)
    for out in results:
        (info, _, _), = out
        assert info.iterations == 0 and info.cancelled == 1 and info.converged == 0


@pytest.mark.parametrize("scene", ["beam", "beam128L4_brick"])
def test_processes_direct_transport_float_vectors(scene, tmp_path, monkeypatch, built_lib):
    """One process per rank (both on cuda:0), hosted group: the direct transport's float loop (tests/hosted_rank_f32.py)."""
    world = 2
    dev = torch.device("cuda:0")
    sc = {"beam": lambda: scenes.fat_beam(64, 3, device=dev), "beam128L4_brick": lambda: scenes.fat_beam(128, 4, device=dev)}[scene]()
    monkeypatch.setenv("AVS_BRICK", "1" if scene.endswith("_brick") else "0")
    pyr = build_pyramid(sc)
    iters_f, _, x64, err_f = _references(sc, pyr)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", AVS_DIST_TIMEOUT_MS="30000", AVS_DIST_F32_VECTORS="1")
    here = os.path.dirname(os.path.abspath(__file__))
    procs = [subprocess.Popen([sys.executable, os.path.join(here, "hosted_rank_f32.py"), str(tmp_path), str(r), str(world), scene, repr(TOL)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(world)]
    outs = [p.communicate(timeout=200) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    x = np.zeros_like(x64)
    x_again = np.zeros_like(x64)
    its = set()
    for r in range(world):
        x += np.load(tmp_path / f"x_{r}.npy")
        x_again += np.load(tmp_path / f"x2_{r}.npy")
        it1, c1, it2, c2, own, halo, direct, rccl_calls, st_rounds, st_bad, fv, brick_tiles = np.load(tmp_path / f"info_{r}.npy")
        assert direct == 1 and rccl_calls == 0 and st_rounds > 0 and st_bad == 0    # the self-test passed over the mapped blocks
        assert fv == 1 and c1 == 1 and c2 == 1 and it1 == it2 and halo > 0
        assert (brick_tiles > 0) == scene.endswith("_brick")
        assert abs(it1 - iters_f) <= max(3, int(0.03 * iters_f)), (it1, iters_f)
        its.add(int(it1))
    assert len(its) == 1
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    assert np.array_equal(x.view(np.int64), x_again.view(np.int64))
    assert rel_l2(x, x64) <= max(2 * err_f, 5e-5), (rel_l2(x, x64), err_f)
