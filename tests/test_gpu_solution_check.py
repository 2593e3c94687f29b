"""avs_check_solution / avs_check_csr_solution: the true residual b - A x in fp64 on the device (avs_solution_check.hip).

Reference: tests/solution_check_model.py (NumPy; pinned by test_solution_check_model.py).  Tolerances: `residual` bit for bit (the same
operations in the same order, one rounding each; a NaN stands for any NaN: IEEE 754 leaves the sign and payload of a generated NaN open);
counters, maxima, max_residual_row and evaluated exact; a sum S within rows_summed * 2^-53 * sum |term| of the exact sum of its terms
(math.fsum): the worst-case bound of a sum of that many terms in any order, derived, not tuned.

The claim against the truth (fp64 paths, tolerance 1e-8): relative_residual <= m * max(rho_oracle, tol), rho_oracle the true relative
residual of the oracle's PCG on the same system.  m = twice the oracle's largest per-iteration reduction of the true residual over its last
eight iterations, measured on the CPU (profiles/solution_check.md): sphere16_L2 2.27 -> m = 4.6, beam32_L3 1.25 -> m = 2.5 -- two correct
fp64 loops may stop one iteration apart."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from adaptiveviscositysolver_amd import DevicePrepass, ViscositySolve, capi, check_csr_solution, scenes

import solution_check_cases as sc
import solution_check_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = -7.25
TOL = 1e-8
CLAIM_FACTOR = {"sphere16_L2": 4.6, "beam32_L3": 2.5}
SCENES = {"sphere16_L2": lambda: scenes.sphere(16, 2), "beam32_L3": lambda: scenes.fat_beam(32, 3)}
PATHS = ("default", "launch_per_phase", "mixed", "f32")
REPORT_INTS = ("which", "evaluated", "n", "nnz", "nonfinite_x", "nonfinite_b", "nonfinite_residual", "rows_summed", "max_residual_row")


def ptr(a):
    if a is None or len(a) == 0:
        return None
    return a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data


def on_device(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


def host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else a


def call(c, arrays, where, x0=True, residual=None, rep=None, n=None, nnz=None, device=0):
    """avs_check_csr_solution on the arrays of a case (or their device copies) -> status, report, message"""
    lib = capi.load()
    rep = capi.SolutionCheck() if rep is None else rep
    rp, col, val, b, x, g = arrays
    st = lib.avs_check_csr_solution(c.n if n is None else n, c.nnz if nnz is None else nnz, ptr(rp), ptr(col), ptr(val), ptr(b), ptr(x),
                                    ptr(g) if x0 else None, ptr(residual), where, device, None, C.byref(rep) if rep is not False else None)
    return st, rep, (lib.avs_last_error().decode() if st != capi.OK else "")


@pytest.fixture(scope="module")
def expected():
    """the model's answer, computed once per (case, with x0)"""
    made = {}

    def get(name, x0=True):
        if (name, x0) not in made:
            c = sc.case(name)
            made[name, x0] = M.evaluate(c.row_ptr, c.col, c.val, c.b, c.x, c.x0 if x0 else None)
        return made[name, x0]
    return get


def agree(rep, res, want, claim=None):
    """a capi.SolutionCheck and the residual array against the model's dict"""
    for f in REPORT_INTS:
        assert getattr(rep, f) == want[f], (f, getattr(rep, f), want[f])
    assert rep.reserved == 0 and rep.struct_size == C.sizeof(capi.SolutionCheck)
    if claim is None:
        assert rep.claimed_converged == -1 and rep.claimed_iterations == -1 and math.isnan(rep.claimed_error)
    else:
        assert (rep.claimed_converged, rep.claimed_iterations, rep.claimed_error) == claim
    if res is not None and want["residual"] is not None:
        assert M.same_floats(res, want["residual"])
    for f in M.MAXIMA:
        assert getattr(rep, f) == want[f] and not np.signbit(getattr(rep, f)), (f, getattr(rep, f), want[f])
    for f in M.SUMS:
        got, bound = getattr(rep, f), want["rows_summed"] * 2.0 ** -53 * want[f + "_abs"]
        print(f, got, "exact", want[f], "bound", bound)
        assert abs(got - want[f]) <= bound, (f, got, want[f], bound)
    assert rep.relative_residual == M.relative_residual(rep.residual_norm2, rep.rhs_norm2) or \
        (math.isnan(rep.relative_residual) and math.isnan(rep.residual_norm2))


# ---- 1. every case, host and device arrays, with and without x0, twice -------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", sc.ALL_NAMES)
def test_report_equals_the_model(built_lib, expected, name, where):
    c = sc.case(name)
    arrays = c.arrays()
    if where == "device":
        arrays = tuple(on_device(a) for a in arrays)
    mem = capi.MEM_DEVICE if where == "device" else capi.MEM_HOST
    for x0 in (True, False):
        want = expected(name, x0)
        res = np.full(c.n, POISON)
        if where == "device":
            res = on_device(res)
            torch.cuda.synchronize()
        st, rep, err = call(c, arrays, mem, x0, res)
        torch.cuda.synchronize()
        assert st == capi.OK, err
        agree(rep, host(res), want)
        if name in sc.SEAM_A_ONLY:                                     # nothing was gathered, nothing written
            assert rep.evaluated == 0 and (host(res) == POISON).all()
            assert bytes(rep)[12:152] == bytes(capi.SolutionCheck(n=c.n, nnz=c.nnz, claimed_converged=-1, claimed_iterations=-1))[12:152]
        res2 = np.full(c.n, POISON)
        res2 = on_device(res2) if where == "device" else res2
        torch.cuda.synchronize()
        st, again, err = call(c, arrays, mem, x0, res2)
        torch.cuda.synchronize()
        assert st == capi.OK and bytes(again) == bytes(rep) and host(res2).tobytes() == host(res).tobytes(), "second call"
        st, alone, err = call(c, arrays, mem, x0, None)                # the report without the residual
        assert st == capi.OK and bytes(alone) == bytes(rep)


def test_python_wrapper(built_lib, expected):
    c = sc.case("tile_straddle")
    r = check_csr_solution(c.row_ptr, c.col, c.val, c.b, c.x, c.x0, residual=True)
    want = expected("tile_straddle")
    assert r.evaluated and r.rows_summed == c.n and M.same_floats(r.residual, want["residual"]) and r.max_residual_row == want["max_residual_row"]
    assert r.energy == 0.5 * r.x_dot_ax - r.x_dot_b and math.isnan(r.claimed_error) and r.claimed_iterations == -1
    r = check_csr_solution(c.row_ptr, c.col, c.val, c.b, c.x)
    assert r.residual is None and r.update_norm2 == 0.0 and r.relative_residual > 0
    b = sc.case("bad_column")
    assert not check_csr_solution(b.row_ptr, b.col, b.val, b.b, b.x).evaluated


# ---- 2. the report does not depend on the persistent grid ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tri_65537", "long_row_4097", "tile_straddle", "nan_x_three_rows", "cancellation"])
def test_capped_grid_gives_the_same_bytes(built_lib, monkeypatch, name):
    """AVS_CELLS_GRID_CAP (read when a context-free entry starts): one, three and seven workgroups walk the chunks -- 257 trips of one
    workgroup on tri_65537.  A partial sum belongs to a chunk and the arg-max to a total order, so every byte stays."""
    c = sc.case(name)
    arrays = tuple(on_device(a) for a in c.arrays())
    outs = []
    for cap in (None, "1", "3", "7"):
        if cap is not None:
            monkeypatch.setenv("AVS_CELLS_GRID_CAP", cap)
        res = torch.full((c.n,), POISON, dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        st, rep, err = call(c, arrays, capi.MEM_DEVICE, True, res)
        torch.cuda.synchronize()
        assert st == capi.OK, err
        outs.append((bytes(rep), res.cpu().numpy().tobytes()))
    monkeypatch.delenv("AVS_CELLS_GRID_CAP")
    assert all(o == outs[0] for o in outs[1:])


# ---- 3. the caller's arrays: read in place inside larger buffers, and left as they are -----------------------------------------------------
@pytest.mark.parametrize("name", ["tri_257", "long_row_4097", "unordered_repeated", "empty_rows", "bad_column", "bad_row_ptr", "n_0"])
def test_device_arrays_are_interior_slices_and_stay_untouched(built_lib, expected, name):
    c = sc.case(name)
    pad = {"rp": (3, 5), "col": (1, 7), "val": (1, 3), "b": (3, 1), "x": (1, 2), "x0": (5, 1), "res": (1, 3)}   # 4- and 8-byte starts only
    src = {"rp": (c.row_ptr, -1), "col": (c.col, -2**31), "val": (c.val, np.nan), "b": (c.b, np.nan), "x": (c.x, np.nan), "x0": (c.x0, np.nan),
           "res": (np.full(c.n, POISON), POISON)}
    bufs, views = {}, {}
    for k, (a, poison) in src.items():
        before, behind = pad[k]
        bufs[k] = torch.from_numpy(np.concatenate([np.full(before, poison, a.dtype), a, np.full(behind, poison, a.dtype)])).to(DEV)
        views[k] = bufs[k][before:before + len(a)]
    copies = {k: b.clone() for k, b in bufs.items()}
    torch.cuda.synchronize()
    st, rep, err = call(c, tuple(views[k] for k in ("rp", "col", "val", "b", "x", "x0")), capi.MEM_DEVICE, True, views["res"])
    torch.cuda.synchronize()
    assert st == capi.OK, err
    agree(rep, views["res"].cpu().numpy(), expected(name))
    for k in bufs:
        if k != "res":
            assert bufs[k].cpu().numpy().tobytes() == copies[k].cpu().numpy().tobytes(), k
    before, behind = pad["res"]
    frame = bufs["res"].cpu().numpy()
    assert (frame[:before] == POISON).all() and (frame[before + c.n:] == POISON).all()
    if name in sc.SEAM_A_ONLY:
        assert (frame == POISON).all()


# ---- 4. the report struct and the arguments ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [12, 16, 24, 40, 96, 152, 160])
def test_only_struct_size_bytes_are_written(built_lib, size):
    c = sc.case("tri_257")
    st, full, err = call(c, c.arrays(), capi.MEM_HOST)
    assert st == capi.OK and full.rows_summed == 257, err
    rep = capi.SolutionCheck()
    C.memset(C.byref(rep), 0x5a, C.sizeof(rep))
    rep.struct_size = size
    st, _, err = call(c, c.arrays(), capi.MEM_HOST, rep=rep)
    assert st == capi.OK, err
    got, want = bytes(rep), bytes(full)
    assert rep.struct_size == size and got[4:size] == want[4:size] and got[size:] == b"\x5a" * (C.sizeof(rep) - size)


def test_argument_errors_have_messages(built_lib):
    c = sc.case("tri_255")
    good = dict(c=c, arrays=c.arrays(), where=capi.MEM_HOST)
    assert call(**good)[0] == capi.OK
    small, absurd = capi.SolutionCheck(), capi.SolutionCheck()
    small.struct_size, absurd.struct_size = 8, 5000
    rp, col, val, b, x, g = c.arrays()
    bad = [dict(rep=small), dict(rep=absurd), dict(rep=False), dict(rep=False, residual=np.zeros(c.n)), dict(n=-1), dict(nnz=-1), dict(n=2**31),
           dict(nnz=2**31), dict(arrays=(None, col, val, b, x, g)), dict(arrays=(rp, None, val, b, x, g)), dict(arrays=(rp, col, None, b, x, g)),
           dict(arrays=(rp, col, val, None, x, g)), dict(arrays=(rp, col, val, b, None, g)), dict(device=-1),
           dict(device=torch.cuda.device_count()), dict(where=7)]
    for change in bad:
        st, _, err = call(**{**good, **change})
        assert st == capi.EINVAL and err, (change.keys(), st, err)
    st, rep, err = call(c, (np.zeros(2, np.int32), None, None, np.ones(1), np.ones(1), None), capi.MEM_HOST, False, n=1, nnz=0)   # nothing to read in col / val
    assert st == capi.OK and rep.evaluated == 1 and rep.residual_norm2 == 1.0 and rep.relative_residual == 1.0, err
    assert call(**good)[0] == capi.OK


# ---- 5. the system a context assembled and the solution a loop left ----------------------------------------------------------------------
class Frame:
    """one scene assembled and solved through one path"""

    def __init__(self, scene, path, check_first=False):
        scn = scenes.to_device(SCENES[scene](), torch.device(DEV))
        self.pp = pp = DevicePrepass(scn.res, scn.dx, scn.levels, device=0)
        info = pp.run(scn.liquid, scn.solid)
        self.s = s = ViscositySolve(scn.res, scn.dx, scn.dt, info.levels, device=0,
                                    precision=capi.PRECISION_F32 if path == "f32" else capi.PRECISION_F64)
        pp.apply(s)
        s.set_scene_fields(scn)
        lib, rep = capi.load(), capi.SolutionCheck()
        self.before_assemble = lib.avs_check_solution(s.h, capi.CHECK_OF_SOLUTION, None, C.byref(rep), capi.MEM_HOST), lib.avs_last_error()
        if path in ("launch_per_phase", "mixed"):
            s.set_solver_option(capi.OPTION_RESIDENT_LOOP, 0)
        if path == "mixed":
            s.set_solver_option(capi.OPTION_MIXED_PRECISION, 1)
        s.assemble()
        self.before_solve = lib.avs_check_solution(s.h, capi.CHECK_OF_SOLUTION, None, C.byref(rep), capi.MEM_HOST), lib.avs_last_error()
        if check_first:
            self.guess_report = s.check_solution(capi.CHECK_OF_INITIAL_GUESS, residual=True)
        self.info = s.solve(TOL, 3000 if path != "f32" else 600)

    def close(self):
        self.s.close()
        self.pp.close()


@pytest.fixture(scope="module")
def frames(built_lib):
    made = {}

    def get(scene, path):
        if (scene, path) not in made:
            made[scene, path] = Frame(scene, path)
        return made[scene, path]
    yield get
    for f in made.values():
        f.close()


def raw_report(s, which, residual, where=capi.MEM_HOST):
    rep = capi.SolutionCheck()
    capi.check(s.lib.avs_check_solution(s.h, which, ptr(residual), C.byref(rep), where))
    return rep


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("scene", list(SCENES))
def test_context_entry_equals_the_model(frames, scene, path):
    f = frames(scene, path)
    s, info = f.s, f.info
    assert f.before_assemble[0] == capi.ESTATE and f.before_assemble[1] and f.before_solve[0] == capi.ESTATE and f.before_solve[1]
    rp, col, val, rhs = s.csr()
    x, g = s.solution(), s.initial_guess()
    n = len(rhs)
    want = M.evaluate(rp, col, val, rhs, x, g, seam_a=False)
    res = np.full(n, POISON)
    rep = raw_report(s, capi.CHECK_OF_SOLUTION, res)
    print(scene, path, "n", n, "nnz", len(col), "iterations", info.iterations, "converged", info.converged, "claimed", info.error, "true",
          rep.relative_residual, "ratio", rep.relative_residual / info.error)
    agree(rep, res, want, claim=(int(info.converged), int(info.iterations), float(info.error)))
    assert rep.rows_summed == n and rep.nonfinite_residual == 0
    dres = torch.full((n,), POISON, dtype=torch.float64, device=DEV)           # device destination, the same bytes; a second call
    torch.cuda.synchronize()
    drep = raw_report(s, capi.CHECK_OF_SOLUTION, dres, capi.MEM_DEVICE)
    torch.cuda.synchronize()
    assert bytes(drep) == bytes(rep) and dres.cpu().numpy().tobytes() == res.tobytes()
    assert bytes(raw_report(s, capi.CHECK_OF_SOLUTION, None)) == bytes(rep)
    st = s.lib.avs_check_solution(s.h, capi.CHECK_OF_SOLUTION, ptr(res), None, capi.MEM_HOST)                     # the residual alone
    assert st == capi.OK and M.same_floats(res, want["residual"])
    w = s.check_solution(residual=True)
    assert w.relative_residual == rep.relative_residual and w.claimed_error == info.error and w.residual.tobytes() == res.tobytes()
    assert s.check_solution(residual=True, device_arrays=True).residual.cpu().numpy().tobytes() == res.tobytes()
    # the initial guess: x = x0, so the update is zero
    gres = np.full(n, POISON)
    grep = raw_report(s, capi.CHECK_OF_INITIAL_GUESS, gres)
    gwant = M.evaluate(rp, col, val, rhs, g, g, which=M.INITIAL_GUESS, seam_a=False)
    agree(grep, gres, gwant)
    assert grep.update_norm2 == 0.0 and grep.max_abs_update == 0.0 and grep.relative_residual > rep.relative_residual
    # the claim belongs to the x the solve left: a solution handed in drops it, the figures stay
    s.set_solution(x)
    after = raw_report(s, capi.CHECK_OF_SOLUTION, None)
    assert after.claimed_iterations == -1 and after.claimed_converged == -1 and math.isnan(after.claimed_error)
    assert bytes(after)[24:152] == bytes(rep)[24:152]
    # argument errors of this entry
    lib, r = s.lib, capi.SolutionCheck()
    for which, resid, report, where in ((2, None, C.byref(r), capi.MEM_HOST), (-1, None, C.byref(r), capi.MEM_HOST), (0, None, None, capi.MEM_HOST),
                                        (0, None, C.byref(r), 7)):
        assert lib.avs_check_solution(s.h, which, resid, report, where) == capi.EINVAL and lib.avs_last_error()
    r.struct_size = 8
    assert lib.avs_check_solution(s.h, 0, None, C.byref(r), capi.MEM_HOST) == capi.EINVAL and lib.avs_last_error()
    assert lib.avs_check_solution(None, 0, None, C.byref(capi.SolutionCheck()), capi.MEM_HOST) == capi.EINVAL


@pytest.fixture(scope="module")
def oracle_residual():
    """rho_oracle: the true relative residual of the oracle's PCG on a context's own system, once per scene"""
    from util import O
    made = {}

    def get(scene, s):
        if scene not in made:
            rp, col, val, rhs = s.csr()
            g = s.initial_guess()
            xo, io = O.pcg_csr(rp, col, val, rhs, g, TOL, 3000)
            made[scene] = M.evaluate(rp, col, val, rhs, xo, g, seam_a=False)["relative_residual"], io
        return made[scene]
    return get


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("scene", list(SCENES))
def test_the_claim_against_the_truth(frames, oracle_residual, scene, path):
    """fp64 paths: relative_residual <= m * max(rho_oracle, tol) (module docstring).  The float context is reported, not asserted."""
    f = frames(scene, path)
    rho, io = oracle_residual(scene, f.s)
    rep = raw_report(f.s, capi.CHECK_OF_SOLUTION, None)
    m = CLAIM_FACTOR[scene]
    print(scene, path, "true", rep.relative_residual, "claimed", f.info.error, "iterations", f.info.iterations, "oracle: true", rho, "claimed", io.error,
          "iterations", io.iterations, "m", m, "bound", m * max(rho, TOL))
    if path == "f32":
        return
    assert f.info.converged == 1 and f.info.error < TOL
    assert rep.relative_residual <= m * max(rho, TOL)


def test_fresh_context_and_capped_grid_give_the_same_bytes(frames, monkeypatch):
    f = frames("sphere16_L2", "launch_per_phase")
    s = f.s
    s.set_solution(s.solution())                                                     # (no claim in either context)
    res = np.full(int(s.info().n_velocity), POISON)
    want = raw_report(s, capi.CHECK_OF_SOLUTION, res)
    g = Frame("sphere16_L2", "launch_per_phase")
    try:
        assert g.info.iterations == f.info.iterations
        g.s.set_solution(s.solution())
        gres = np.full(len(res), POISON)
        assert bytes(raw_report(g.s, capi.CHECK_OF_SOLUTION, gres)) == bytes(want) and gres.tobytes() == res.tobytes()
        for cap in ("1", "3"):
            monkeypatch.setenv("AVS_CELLS_GRID_CAP", cap)
            try:
                g.s.set_solver_option(capi.OPTION_RELOAD_ENVIRONMENT, 1)             # (the environment is read at avs_create)
                cres = np.full(len(res), POISON)
                assert bytes(raw_report(g.s, capi.CHECK_OF_SOLUTION, cres)) == bytes(want) and cres.tobytes() == res.tobytes()
            finally:
                monkeypatch.delenv("AVS_CELLS_GRID_CAP")
                g.s.set_solver_option(capi.OPTION_RELOAD_ENVIRONMENT, 1)
    finally:
        g.close()


def test_a_checked_context_solves_as_an_unchecked_one(built_lib):
    def frame(checked):
        f = Frame("beam32_L3", "default", check_first=checked)
        s = f.s
        if checked:
            assert s.check_solution(residual=True).claimed_iterations == f.info.iterations
            again = s.solve(TOL, 3000)                                                  # ... and once more behind a check of the solution
            assert (again.iterations, again.converged, again.error) == (f.info.iterations, f.info.converged, f.info.error)
            assert s.check_solution().claimed_error == again.error
        out = [s.csr(), s.initial_guess(), s.solution(), (f.info.iterations, f.info.converged, f.info.error)]
        f.close()
        return out

    (csr_a, g_a, x_a, i_a), (csr_b, g_b, x_b, i_b) = frame(False), frame(True)
    assert i_a == i_b and i_a[1] == 1
    assert all(a.tobytes() == b.tobytes() for a, b in zip(csr_a, csr_b))
    assert g_a.tobytes() == g_b.tobytes() and x_a.tobytes() == x_b.tobytes() and np.abs(x_a).max() > 0


def test_partitioned_solutions_carry_no_claim_and_local_systems_are_refused(built_lib):
    """world = 1: a gathered partitioned solution is checked against the global matrix, but no avs_solve claimed it; after
    avs_dist_assemble there is no global matrix to check against"""
    f = Frame("beam32_L3", "launch_per_phase")
    s = f.s
    try:
        assert raw_report(s, capi.CHECK_OF_SOLUTION, None).claimed_iterations == f.info.iterations
        buf = (C.c_uint8 * capi.UNIQUE_ID_BYTES)()
        capi.check(s.lib.avs_dist_get_unique_id(buf))
        capi.check(s.lib.avs_dist_init(s.h, buf, 0, 1))
        s.dist_partition()
        assert raw_report(s, capi.CHECK_OF_SOLUTION, None).claimed_iterations == f.info.iterations       # x is still what avs_solve left
        assert s.dist_solve(TOL, 3000).converged == 1
        x = s.dist_solution()                                                                            # ... and now what the ranks gathered
        rp, col, val, rhs = s.csr()
        res = np.full(len(rhs), POISON)
        rep = raw_report(s, capi.CHECK_OF_SOLUTION, res)
        agree(rep, res, M.evaluate(rp, col, val, rhs, x, s.initial_guess(), seam_a=False))
        assert rep.relative_residual <= CLAIM_FACTOR["beam32_L3"] * TOL
        s.dist_assemble()
        for which in (capi.CHECK_OF_SOLUTION, capi.CHECK_OF_INITIAL_GUESS):
            r = capi.SolutionCheck()
            assert s.lib.avs_check_solution(s.h, which, None, C.byref(r), capi.MEM_HOST) == capi.ESTATE
            assert b"no system" in s.lib.avs_last_error()
    finally:
        f.close()
