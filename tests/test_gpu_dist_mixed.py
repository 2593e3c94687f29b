"""Partitioned solves of fp64 contexts on float vectors with fp64 reliable updates (AVS_OPTION_DIST_MIXED_PRECISION = 1, csrc/avs_pcg.hip:
pcg_solve_single_reduction<float, true>, pcg_solve_direct<float, true>; the scheme: tests/dist_mixed_model.py).

The yardstick is always the fp64 partitioned loop of the same world, mode and scene on contexts that never saw the option.  Virtual ranks
(in-process transport) and one process per rank (direct transport, tests/hosted_rank_mixed.py).  Every world is made once per module and
runs all the solves the tests look at (`_world`)."""
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

TIGHT = 1e-10
SCENES = {
    "beam64": (lambda dev: scenes.fat_beam(64, 3, device=dev), "0"),
    "varvisc64": (lambda dev: scenes.fat_beam(64, 3, variable_viscosity=True, device=dev), "0"),
    "beam128L4": (lambda dev: scenes.fat_beam(128, 4, device=dev), "1"),        # AVS_BRICK=1: the brick form of the local rows, mixed kernel
    "sphere32": (lambda dev: scenes.sphere(32, 3, radius=0.36, device=dev), "0"),  # thousands of values: the streaming kernel, one inverse per row
}
CASES = [("beam64", 2, "partition"), ("varvisc64", 3, "partition"), ("beam128L4", 2, "assemble"), ("sphere32", 2, "partition")]
_cache = {}


def _residual_and_bound(rp, col, val, b, x):
    """|b - A x| / |b| in numpy, and the bound on the difference of two fp64 evaluations of it that add in different orders:
    2 (m + 2) 2^-53 | |A||x| + |b| |_2 / |b|_2, m = the longest row"""
    rp = np.asarray(rp, dtype=np.int64)
    ax = np.add.reduceat(val * x[col], rp[:-1])
    absax = np.add.reduceat(np.abs(val) * np.abs(x[col]), rp[:-1])
    m = int((rp[1:] - rp[:-1]).max())
    nb = float(np.linalg.norm(b))
    return float(np.linalg.norm(b - ax)) / nb, 2.0 * (m + 2) * 2.0 ** -53 * float(np.linalg.norm(absax + np.abs(b))) / nb


def _scene(name):
    """scene, pre-pass, and a single-GPU context's CSR, initial guess and fp64 solution at 1e-10 (once per module)"""
    if ("scene", name) not in _cache:
        make, brick = SCENES[name]
        sc = make(torch.device("cuda:0"))
        pyr = build_pyramid(sc)
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("AVS_BRICK", brick)
            s = ViscositySolve(sc.res, sc.dx, sc.dt, pyr.levels, device=0)
        feed(s, pyr)
        s.set_scene_fields(sc)
        s.assemble()
        info = s.solve(TIGHT, 20000)
        assert info.converged == 1
        _cache[("scene", name)] = (sc, pyr, brick, s.csr(), s.initial_guess(), s.solution())
        s.close()
    return _cache[("scene", name)]


def _partitioned(scene, world, mode, jobs, option=None, options=(), env=None, precision=capi.PRECISION_F64):
    """world virtual ranks; option: value of AVS_OPTION_DIST_MIXED_PRECISION (None: never set); jobs(r, solve) runs the rank's solves --
    solve(tol, max_iters, cancel=False) returns (info, gathered x, matrix format)."""
    sc, pyr, brick, *_ = _scene(scene)
    lib = capi.load()
    grp = C.c_void_p()
    capi.check(lib.avs_local_group_create(world, C.byref(grp)))
    with pytest.MonkeyPatch.context() as mp:      # (the environment is read once, at avs_create)
        mp.setenv("AVS_BRICK", brick)
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        solvers = []
        for _ in range(world):
            s = ViscositySolve(sc.res, sc.dx, sc.dt, pyr.levels, device=0, precision=precision)
            feed(s, pyr)
            s.set_scene_fields(sc)
            solvers.append(s)
    results, errors = [None] * world, []

    def run(r):
        try:
            s = solvers[r]
            if option is not None:
                s.set_solver_option(capi.OPTION_DIST_MIXED_PRECISION, option)
            for o, v in options:
                s.set_solver_option(o, v)
            s.dist_init_local(grp, r)
            if mode == "partition":
                s.assemble()
                s.dist_partition()
            else:
                s.dist_assemble()

            def solve(tol, max_iters=5000, cancel=False):
                if cancel:
                    capi.check(lib.avs_cancel(s.h))
                info = s.dist_solve(tol, max_iters)
                return info, s.dist_solution(), s.matrix_format()

            results[r] = jobs(r, solve)
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


def _world(scene, world, mode):
    """the yardstick (1e-5, 1e-10) and every mixed solve of one world: dict of per-rank results"""
    key = ("world", scene, world, mode)
    if key not in _cache:
        yard = _partitioned(scene, world, mode, lambda r, solve: {"loose": solve(1e-5), "tight": solve(TIGHT)})
        it_tight = yard[0]["tight"][0].iterations

        def jobs(r, solve):
            out = {"loose": solve(1e-5), "again": solve(1e-5), "tight": solve(TIGHT, 2 * it_tight)}
            if scene == "beam64":
                out["capped"] = solve(TIGHT, 40)
                out["cancelled"] = solve(TIGHT, 5000, cancel=True)
                out["later"] = solve(1e-5)
            return out

        _cache[key] = (yard, _partitioned(scene, world, mode, jobs, option=1))
    return _cache[key]


@pytest.mark.parametrize("scene,world,mode", CASES)
def test_default_tolerance_matches_the_fp64_loop(scene, world, mode, built_lib):
    yard, mixed = _world(scene, world, mode)
    its = set()
    for y, m in zip(yard, mixed):
        (iy, _, fy), (i1, x1, f1), (i2, x2, f2) = y["loose"], m["loose"], m["again"]
        assert iy.converged == 1 and int(fy.float_vectors) == 0 and int(fy.reliable_updates) == 0
        assert i1.converged == 1 and i1.cancelled == 0 and i1.resident == 0 and i1.error < 1e-5
        assert int(f1.float_vectors) == 1 and int(f1.reliable_updates) >= i1.iterations // 32
        print(f"{scene} x{world} {mode}: tol 1e-5: mixed {i1.iterations} iterations, {int(f1.reliable_updates)} updates; fp64 loop {iy.iterations}")
        assert abs(i1.iterations - iy.iterations) <= max(3, iy.iterations // 100), (i1.iterations, iy.iterations)
        assert i2.iterations == i1.iterations and int(f2.reliable_updates) == int(f1.reliable_updates)
        assert np.array_equal(x1.view(np.int64), x2.view(np.int64))
        if scene == "beam128L4":
            assert int(f1.brick_tiles) > 0
        its.add(i1.iterations)
    assert len(its) == 1   # every rank stops in the same iteration


@pytest.mark.parametrize("scene,world,mode", CASES)
def test_tight_tolerance_reports_the_fp64_residual(scene, world, mode, built_lib):
    """tol 1e-10 within twice the yardstick's iterations (a condition, not a target: the model needs <= 1.37 x).
    Measured ratios (mixed / fp64 partitioned loop, MI355X): DESIGN.md section 6."""
    _, _, _, (rp, col, val, rhs), _, x64 = _scene(scene)
    yard, mixed = _world(scene, world, mode)
    for y, m in zip(yard, mixed):
        (iy, xy, _), (im, xm, fm) = y["tight"], m["tight"]
        res, bound = _residual_and_bound(rp, col, val, rhs, xm)
        print(f"{scene} x{world} {mode}: tol 1e-10: mixed {im.iterations} iterations, {int(fm.reliable_updates)} updates; fp64 loop {iy.iterations}; "
              f"ratio {im.iterations / iy.iterations:.3f}; info.error {im.error:.3e}, numpy residual {res:.3e} (bound {bound:.1e}); "
              f"rel_l2 vs single-GPU fp64 {rel_l2(xm, x64):.2e} (fp64 loop: {rel_l2(xy, x64):.2e})")
        assert im.converged == 1 and im.error < TIGHT
        assert int(fm.float_vectors) == 1 and int(fm.reliable_updates) >= im.iterations // 32
        assert abs(res - im.error) <= bound, (res, im.error, bound)
        assert rel_l2(xm, x64) < 1e-8


def test_exits_leave_the_last_iterate_and_its_residual(built_lib):
    _, _, _, (rp, col, val, rhs), x0, _ = _scene("beam64")
    _, mixed = _world("beam64", 2, "partition")
    for m in mixed:
        info, x, fmt = m["capped"]
        assert info.iterations == 40 and info.converged == 0 and int(fmt.reliable_updates) == 2
        res, bound = _residual_and_bound(rp, col, val, rhs, x)
        assert abs(res - info.error) <= bound, (res, info.error, bound)
        info, x, fmt = m["cancelled"]
        assert info.iterations == 0 and info.cancelled == 1 and info.converged == 0
        assert np.array_equal(x.view(np.int64), x0.view(np.int64))
        info, _, _ = m["later"]
        assert info.converged == 1 and info.cancelled == 0 and info.iterations == m["loose"][0].iterations


def _bits(results):
    return [(r[0].iterations, int(r[2].float_vectors), int(r[2].reliable_updates), r[1].view(np.int64)) for r in results]


def _same(a, b):
    return all(p[:3] == q[:3] and np.array_equal(p[3], q[3]) for p, q in zip(_bits(a), _bits(b)))


def test_option_off_is_the_fp64_loop(built_lib):
    yard, _ = _world("beam64", 2, "partition")
    off = _partitioned("beam64", 2, "partition", lambda r, solve: solve(1e-5), option=0)
    never = [y["loose"] for y in yard]
    assert _same(never, off)
    assert all(int(r[2].float_vectors) == 0 and int(r[2].reliable_updates) == 0 for r in off)
    # AVS_OPTION_MIXED_PRECISION alone: no effect on avs_dist_solve
    single = _partitioned("beam64", 2, "partition", lambda r, solve: solve(1e-5), options=[(capi.OPTION_MIXED_PRECISION, 1)])
    assert _same(never, single)


@pytest.mark.parametrize("what", ["standard_cg", "paranoid", "f32_context"])
def test_option_is_not_taken(what, built_lib):
    """AVS_DIST_CG=standard, paranoid mode and AVS_PRECISION_F32 contexts run the loop they ran before, bit for bit"""
    kw = {"standard_cg": dict(env={"AVS_DIST_CG": "standard"}), "paranoid": dict(options=[(capi.OPTION_PARANOID, 1)]),
          "f32_context": dict(precision=capi.PRECISION_F32)}[what]
    off = _partitioned("beam64", 2, "partition", lambda r, solve: solve(1e-5), option=0, **kw)
    on = _partitioned("beam64", 2, "partition", lambda r, solve: solve(1e-5), option=1, **kw)
    assert _same(off, on)
    assert all(int(r[2].float_vectors) == 0 and int(r[2].reliable_updates) == 0 and r[0].converged == 1 for r in on)


@pytest.mark.parametrize("scene", ["beam128L4", "beam64"])
def test_local_product(scene, built_lib, monkeypatch):
    """one hosted rank (0 of 2), no peer needed: the mixed local product on an [owned | halo] vector of float values against the fp64
    product of the same rank on a context without the option; fused_dot & 2: the fp64 product of the reliable updates, bit for bit"""
    sc, pyr, brick, *_ = _scene(scene)
    monkeypatch.setenv("AVS_BRICK", brick)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    out, x, xh = {}, None, None
    for option in (None, 1):
        s = ViscositySolve(sc.res, sc.dx, sc.dt, pyr.levels, device=0, probe=True)
        feed(s, pyr)
        s.set_scene_fields(sc)
        if option is not None:
            s.set_solver_option(capi.OPTION_DIST_MIXED_PRECISION, option)
        capi.check(s.lib.avs_dist_init_hosted(s.h, 0, 2))
        s.dist_assemble(0)
        sz = s.plan_sizes
        n_own, n_ext = int(sz.n_own), int(sz.n_own + sz.n_halo)
        assert sz.n_halo > 0 and (s.matrix_format().brick_tiles > 0) == (brick == "1")
        if x is None:
            xh = (rng.standard_normal(n_ext) * 10.0 ** rng.integers(-3, 4, n_ext)).astype(np.float32).astype(np.float64)
            x = torch.from_numpy(xh).to(dev)
        assert len(xh) == n_ext
        for flags in (0, 1, 2):
            y = torch.full((n_own,), float("nan"), dtype=torch.float64, device=dev)
            dot = C.c_double()
            capi.check(s.lib.avs_dist_spmv_local_form(s.h, x.data_ptr(), y.data_ptr(), flags, C.byref(dot)))
            out[(option, flags)] = (y.cpu().numpy(), dot.value)
        s.close()
    y64 = out[(None, 0)][0]
    assert np.array_equal(out[(1, 2)][0].view(np.int64), y64.view(np.int64))     # the updates' product on the walk laid out for the mixed kernel
    assert np.array_equal(out[(None, 2)][0].view(np.int64), y64.view(np.int64))
    want = y64.astype(np.float32)
    for flags in (0, 1):
        got, dot = out[(1, flags)]
        assert np.array_equal(got, got.astype(np.float32).astype(np.float64))     # y is a float vector
        ulps = np.abs(got - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
        print(f"{scene}: fused {flags}: rows that differ from the rounded fp64 row sum: {int((got.astype(np.float32) != want).sum())}, worst {float(ulps.max()):.2f} ulp")
        assert float(ulps.max()) <= 1.0
        if flags:
            terms = xh[:len(y64)] * y64
            assert abs(dot - float(terms.sum())) <= 1e-10 * max(1.0, float(np.abs(terms).sum()))


@pytest.mark.parametrize("scene", ["beam", "beam128L4_brick"])
def test_processes_direct_transport(scene, tmp_path, monkeypatch, built_lib):
    """One process per rank (both on cuda:0), hosted group: the direct transport's mixed loop (tests/hosted_rank_mixed.py: tol 1e-5 twice,
    then 1e-10); the yardstick is the same pair of processes without the option."""
    world = 2
    name = "beam64" if scene == "beam" else "beam128L4"
    *_, x64 = _scene(name)
    here = os.path.dirname(os.path.abspath(__file__))
    infos, xs = {}, {}
    for option in ("0", "1"):
        d = tmp_path / option
        d.mkdir()
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", AVS_DIST_TIMEOUT_MS="30000", AVS_DIST_MIXED_PRECISION=option,
                   AVS_BRICK="1" if scene.endswith("_brick") else "0")
        procs = [subprocess.Popen([sys.executable, os.path.join(here, "hosted_rank_mixed.py"), str(d), str(r), str(world), scene, repr(1e-5)],
                                  env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(world)]
        outs = [p.communicate(timeout=200) for p in procs]
        for p, (so, se) in zip(procs, outs):
            assert p.returncode == 0, se[-3000:]
        infos[option] = [dict(zip(np.load(d / f"names_{r}.npy"), np.load(d / f"info_{r}.npy"))) for r in range(world)]
        xs[option] = [np.load(d / f"x_{r}.npy") for r in range(world)]          # rows: first, second, tight solve
    its = set()
    for y, m in zip(infos["0"], infos["1"]):
        assert y["float_vectors"] == 0 and y["reliable_updates"] == 0 and y["converged1"] == 1 and y["direct"] == 1
        assert m["direct"] == 1 and m["rccl_calls"] == 0 and m["selftest_rounds"] > 0 and m["selftest_bad"] == 0   # the self-test passed
        assert m["float_vectors"] == 1 and m["reliable_updates"] > 0 and m["resident"] == 0 and m["n_halo"] > 0
        assert m["converged1"] == 1 and m["converged2"] == 1 and m["iterations1"] == m["iterations2"] and m["error1"] < 1e-5
        assert (m["brick_tiles"] > 0) == scene.endswith("_brick")
        print(f"{scene}: direct transport: tol 1e-5: mixed {int(m['iterations1'])} / fp64 loop {int(y['iterations1'])}; tol 1e-10: mixed "
              f"{int(m['iterations3'])} ({int(m['reliable_updates3'])} updates) / fp64 loop {int(y['iterations3'])}, ratio {m['iterations3'] / y['iterations3']:.3f}")
        assert abs(m["iterations1"] - y["iterations1"]) <= max(3, int(y["iterations1"]) // 100), (m["iterations1"], y["iterations1"])
        assert m["converged3"] == 1 and m["error3"] < TIGHT
        its.add((int(m["iterations1"]), int(m["iterations3"])))
    assert len(its) == 1
    first, second, tight = (sum(x[k] for x in xs["1"]) for k in range(3))
    assert np.array_equal(first.view(np.int64), second.view(np.int64))      # the second solve replays the graph
    assert rel_l2(tight, x64) < 1e-8
