"""avs_estimate_spectrum / avs_estimate_csr_spectrum: Lanczos on D^-1/2 A D^-1/2 or A in fp64 on the device (avs_spectrum.hip).

Reference: tests/spectrum_model.py (NumPy; pinned by test_spectrum_model.py).  Tolerances, derived, not tuned:
  * step by step, no error propagation: from the device's own scale, v_j, v_{j-1}, alpha and beta the model forms t_j and w_j bit for bit
    (the same operations in the same order, one rounding each).  A sum S of n terms added in any order lies within n * 2^-53 * sum |term| of
    the exact sum (math.fsum): the bound test_gpu_solution_check.py applies.  beta is a rounded square root of such a sum and is squared
    again here: beta^2 within that bound plus 4 * 2^-53 of the sum (three roundings and their products).  v_{j+1} = w / beta bit for bit.
  * scale within 1 ulp of numpy's 1 / sqrt(d); gershgorin_max, the counters and the flags exact.
  * end to end against the model run with exact sums: relative 8 x the case's spread between forward and reverse sums
    (spectrum_cases.spread, recorded by test_spectrum_model.py), at least 64 * 2^-52 -- the margin covers a third summation order.
  * ritz against numpy's eigenvalues of the tridiagonal of the device's own alpha and beta: 4 k 2^-52 |T|_inf, both methods being backward
    stable to O(k) eps |T|; lambda_*_bound = beta[k] |last component| with that perturbation over the gap to the next eigenvalue."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from adaptiveviscositysolver_amd import DevicePrepass, ViscositySolve, capi, estimate_csr_spectrum, scenes

import spectrum_cases as sc
import spectrum_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = -7.25
EPS = 2.0 ** -52
SCENES = {"beam32_L3": lambda: scenes.fat_beam(32, 3), "sphere32": lambda: scenes.sphere(32, 3)}


def ptr(a):
    if a is None or len(a) == 0:
        return None
    return a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data


def on_device(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


def host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else a


class Outputs:
    """poisoned destinations: alpha, beta, ritz on the host, scale and basis where `device` says"""

    def __init__(self, n, steps, device, scale=True, basis=True, small=True):
        room = max(steps, 1)
        self.alpha, self.beta, self.ritz = (np.full(k, POISON) if small else None for k in (room, room + 1, room))
        self.scale = np.full(n, POISON) if scale else None
        self.basis = np.full((room + 1) * n, POISON) if basis else None
        if device:
            self.scale, self.basis = on_device(self.scale), on_device(self.basis)
            torch.cuda.synchronize()
        self.n, self.steps = n, steps

    def pointers(self):
        return ptr(self.alpha), ptr(self.beta), ptr(self.ritz), ptr(self.scale), ptr(self.basis)

    def columns(self):
        return host(self.basis).reshape(-1, self.n) if self.n else np.zeros((self.steps + 1, 0))


def call_csr(c, arrays, where, op, out, steps=None, start=None, tolerance=1e-3, rep=None, n=None, nnz=None, device=0):
    """avs_estimate_csr_spectrum on (row_ptr, col, val, b, x0, given) -> status, report, message"""
    lib = capi.load()
    rep = capi.Spectrum() if rep is None else rep
    rp, col, val, b, x0, given = arrays
    st = lib.avs_estimate_csr_spectrum(c.n if n is None else n, c.nnz if nnz is None else nnz, ptr(rp), ptr(col), ptr(val), ptr(b), ptr(x0), ptr(given),
                                       op, c.start if start is None else start, c.steps if steps is None else steps, tolerance, *out.pointers(), where,
                                       device, None, C.byref(rep) if rep is not False else None)
    torch.cuda.synchronize()
    return st, rep, (lib.avs_last_error().decode() if st != capi.OK else "")


def arrays_of(c, device=False):
    a = (c.row_ptr, c.col, c.val, c.b, c.x0, c.given)
    return tuple(on_device(x) for x in a) if device else a


def sum_bound(terms, n):
    return n * 2.0 ** -53 * math.fsum(np.abs(terms))


def step_by_step(rp, col, val, start, b, x0, given, rep, alpha, beta, scale, columns, want_scale):
    """check 1 of the module docstring on one call's outputs; columns: the basis, row j = v_j"""
    n, k = len(rp) - 1, rep.steps_taken
    assert (np.abs(scale - want_scale) <= np.spacing(want_scale)).all(), "scale: more than one ulp from 1 / sqrt(d)"
    assert rep.gershgorin_max == M.gershgorin(rp, col, val, scale)
    v = M.start_vector(rp, col, val, scale, start, b, x0, given)
    sq = math.fsum(v * v)
    print("beta[0]^2", beta[0] * beta[0], "exact", sq, "bound", sum_bound(v * v, n))
    assert abs(beta[0] * beta[0] - sq) <= sum_bound(v * v, n) + 4 * 2.0 ** -53 * sq and rep.start_norm == beta[0]
    assert (v / beta[0]).tobytes() == columns[0].tobytes(), "v_0"
    stopped = bool(rep.breakdown or rep.nonfinite)
    for j in range(k):
        t = M.form_t(rp, col, val, scale, columns[j], columns[j - 1] if j else None, beta[j], j)
        terms = columns[j] * t
        print("step", j, "alpha", alpha[j], "exact", math.fsum(terms), "bound", sum_bound(terms, n), "beta", beta[j + 1])
        assert abs(alpha[j] - math.fsum(terms)) <= sum_bound(terms, n), ("alpha", j)
        w = t - alpha[j] * columns[j]
        sq = math.fsum(w * w)
        assert abs(beta[j + 1] * beta[j + 1] - sq) <= sum_bound(w * w, n) + 4 * 2.0 ** -53 * sq, ("beta", j + 1)
        halts = not beta[j + 1] > M.BREAKDOWN * (abs(alpha[j]) + beta[j])
        assert halts == (rep.breakdown == 1 and j == k - 1), ("the stop decision on the device's own alpha and beta", j)
        if j < k - 1 or not stopped:
            assert (w / beta[j + 1]).tobytes() == columns[j + 1].tobytes(), ("v", j + 1)


def host_part_agrees(rep, alpha, beta, ritz, steps):
    """ritz, the extremes, their bounds, the condition estimate and the iteration bound against numpy on the device's own alpha and beta"""
    k = rep.steps_taken
    assert (ritz[k:steps] == 0).all() and (alpha[k:steps] == 0).all() and (beta[k + 1:steps + 1] == 0).all()
    if k == 0:
        assert (rep.lambda_min, rep.lambda_max, rep.lambda_min_bound, rep.lambda_max_bound, rep.condition_estimate, rep.iteration_bound, rep.indefinite) == \
            (0, 0, 0, 0, 0, -1, 0)
        return
    if rep.nonfinite:
        assert np.isnan(ritz[:k]).all() and math.isnan(rep.lambda_min) and math.isnan(rep.lambda_max) and math.isnan(rep.condition_estimate)
        assert rep.iteration_bound == -1 and rep.indefinite == 0
        return
    t = M.tridiagonal(alpha, beta, k)
    theta, z = np.linalg.eigh(t)
    tol = 4 * k * EPS * np.abs(t).sum(axis=1).max()
    assert np.abs(ritz[:k] - theta).max() <= tol and (np.diff(ritz[:k]) >= 0).all()
    assert rep.lambda_min == ritz[0] and rep.lambda_max == ritz[k - 1] and rep.indefinite == (ritz[0] <= 0)
    for got, i, near in ((rep.lambda_min_bound, 0, 1), (rep.lambda_max_bound, k - 1, k - 2)):
        gap = abs(theta[near] - theta[i]) if k > 1 else 1.0
        print("bound", got, "numpy", beta[k] * abs(z[-1, i]), "gap", gap)
        assert abs(got - beta[k] * abs(z[-1, i])) <= beta[k] * (tol / gap + 4 * k * EPS)
    if rep.indefinite:
        assert rep.condition_estimate == math.inf and rep.iteration_bound == -1
    else:
        assert rep.condition_estimate == rep.lambda_max / rep.lambda_min
        assert rep.iteration_bound == M.iteration_bound(rep.condition_estimate, rep.tolerance)


# ---- 1. and 2.: every case, both operators, host and device arrays ---------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name,op", sc.runs())
def test_case_equals_the_model(built_lib, name, op, where):
    c, want = sc.case(name), sc.model(name, op)
    device = where == "device"
    mem = capi.MEM_DEVICE if device else capi.MEM_HOST
    out = Outputs(c.n, c.steps, device)
    st, rep, err = call_csr(c, arrays_of(c, device), mem, op, out)
    assert st == capi.OK, err
    for f in ("evaluated", "op", "start", "steps_asked", "n", "nnz", "bad_diagonal", "steps_taken", "breakdown", "nonfinite", "indefinite", "tolerance"):
        assert getattr(rep, f) == want[f], (f, getattr(rep, f), want[f])
    assert rep.struct_size == C.sizeof(capi.Spectrum)
    scale, columns = host(out.scale), out.columns()
    if not rep.evaluated:
        assert bytes(rep)[40:] == bytes(capi.Spectrum(bad_diagonal=want["bad_diagonal"], n=c.n, nnz=c.nnz, tolerance=1e-3))[40:]
        assert (out.alpha == 0).all() and (out.beta == 0).all() and (out.ritz == 0).all()
        if name in sc.SEAM_A_ONLY:                                       # nothing was followed, nothing written
            assert (scale == POISON).all() and (columns == POISON).all()
        else:                                                            # the scale says where: s_i = 0 in the rows counted
            assert ((scale == 0) == (want["scale"] == 0)).all() and (np.abs(scale - want["scale"]) <= np.spacing(want["scale"])).all()
        return
    if c.n == 0:
        host_part_agrees(rep, out.alpha, out.beta, out.ritz, c.steps)
        return
    want_scale = np.ones(c.n) if op == M.MATRIX else 1.0 / np.sqrt(M.diagonal(c.row_ptr, c.col, c.val)[0])
    if rep.steps_taken == 0:                                             # zero_start, nan_start
        assert (np.abs(scale - want_scale) <= np.spacing(want_scale)).all() and rep.gershgorin_max == M.gershgorin(c.row_ptr, c.col, c.val, scale)
        assert (out.beta[0] == 0 and want["start_norm"] == 0) or (not math.isfinite(out.beta[0]) and rep.nonfinite == 1)
        assert (out.alpha == 0).all() and (out.beta[1:] == 0).all()
    elif name == "nan_value":
        assert math.isnan(out.alpha[0]) and rep.gershgorin_max == math.inf and rep.start_norm == out.beta[0] > 0
        assert (M.hash_vector(c.n) / out.beta[0]).tobytes() == columns[0].tobytes()
    else:
        step_by_step(c.row_ptr, c.col, c.val, c.start, c.b, c.x0, c.given, rep, out.alpha, out.beta, scale, columns, want_scale)
    host_part_agrees(rep, out.alpha, out.beta, out.ritz, c.steps)
    # end to end against the model with exact sums
    if rep.steps_taken and not rep.nonfinite:
        k = rep.steps_taken
        lo, hi, mid = (max(8 * s, 64 * EPS) for s in sc.spread(name, op))
        print(name, op, "lambda_min", rep.lambda_min, want["lambda_min"], "tolerance", lo, "lambda_max", rep.lambda_max, want["lambda_max"], "tolerance", hi)
        assert abs(rep.lambda_min - want["lambda_min"]) <= lo * abs(want["lambda_min"])
        assert abs(rep.lambda_max - want["lambda_max"]) <= hi * abs(want["lambda_max"])
        assert np.abs(out.ritz[:k] - want["ritz"]).max() <= mid * np.abs(want["ritz"]).max()
        if not rep.indefinite:
            assert abs(rep.condition_estimate - want["condition_estimate"]) <= (lo + hi) * want["condition_estimate"]
    # the report alone, and a second call: the same bytes
    bare = Outputs(c.n, c.steps, device, scale=False, basis=False, small=False)
    st, alone, err = call_csr(c, arrays_of(c, device), mem, op, bare)
    assert st == capi.OK and bytes(alone) == bytes(rep), err
    again = Outputs(c.n, c.steps, device)
    st, rep2, err = call_csr(c, arrays_of(c, device), mem, op, again)
    assert st == capi.OK and bytes(rep2) == bytes(rep)
    for f in ("alpha", "beta", "ritz"):
        assert M.SM.same_floats(getattr(again, f), getattr(out, f)), f
    k = rep.steps_taken
    filled = k + (0 if rep.breakdown or rep.nonfinite or not k else 1)
    assert host(again.scale).tobytes() == scale.tobytes() and again.columns()[:filled].tobytes() == columns[:filled].tobytes()


# ---- 3. determinism: calls, contexts, grids ---------------------------------------------------------------------------------------------------
def test_capped_grid_gives_the_same_bytes(built_lib, monkeypatch):
    """AVS_CELLS_GRID_CAP (read when a context-free entry starts): one and three workgroups walk the 257 chunks of tri_65537.  A partial
    sum belongs to a chunk, so every byte stays."""
    c = sc.case("tri_65537")
    arrays = arrays_of(c, True)
    outs = []
    for cap in (None, None, "1", "3"):
        if cap is not None:
            monkeypatch.setenv("AVS_CELLS_GRID_CAP", cap)
        out = Outputs(c.n, c.steps, True)
        st, rep, err = call_csr(c, arrays, capi.MEM_DEVICE, M.JACOBI, out)
        assert st == capi.OK and rep.steps_taken == c.steps, err
        outs.append((bytes(rep), out.alpha.tobytes(), out.beta.tobytes(), out.ritz.tobytes(), host(out.basis).tobytes()))
    monkeypatch.delenv("AVS_CELLS_GRID_CAP")
    assert all(o == outs[0] for o in outs[1:])


class Frame:
    """one scene assembled (and asked before it was)"""

    def __init__(self, scene, precision=capi.PRECISION_F64, estimate_first=False):
        scn = scenes.to_device(SCENES[scene](), torch.device(DEV))
        self.pp = pp = DevicePrepass(scn.res, scn.dx, scn.levels, device=0)
        info = pp.run(scn.liquid, scn.solid)
        self.s = s = ViscositySolve(scn.res, scn.dx, scn.dt, info.levels, device=0, precision=precision)
        pp.apply(s)
        s.set_scene_fields(scn)
        rep = capi.Spectrum()
        self.before_assemble = s.lib.avs_estimate_spectrum(s.h, 0, 0, 8, 1e-3, None, None, None, None, None, capi.MEM_HOST, C.byref(rep)), s.lib.avs_last_error()
        s.assemble()
        self.first = s.estimate_spectrum(steps=8, scale=True, basis=True) if estimate_first else None

    def close(self):
        self.s.close()
        self.pp.close()


@pytest.fixture(scope="module")
def frames(built_lib):
    made = {}

    def get(scene, precision=capi.PRECISION_F64):
        if (scene, precision) not in made:
            made[scene, precision] = Frame(scene, precision)
        return made[scene, precision]
    yield get
    for f in made.values():
        f.close()


def raw_call(s, op, start, steps, out, where=capi.MEM_HOST, tolerance=1e-3):
    rep = capi.Spectrum()
    capi.check(s.lib.avs_estimate_spectrum(s.h, op, start, steps, tolerance, *out.pointers(), where, C.byref(rep)))
    torch.cuda.synchronize()
    return rep


# ---- 4. the system a context assembled --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [capi.PRECISION_F64, capi.PRECISION_F32])
@pytest.mark.parametrize("scene", list(SCENES))
def test_context_entry_equals_the_model(frames, scene, precision):
    f = frames(scene, precision)
    s = f.s
    assert f.before_assemble[0] == capi.ESTATE and f.before_assemble[1]
    rp, col, val, rhs = s.csr()
    g = s.initial_guess()
    n = len(rhs)
    want_scale = {M.MATRIX: np.ones(n), M.JACOBI: 1.0 / np.sqrt(M.diagonal(rp, col, val)[0])}
    for op in sc.BOTH:
        for start in (M.RESIDUAL, M.HASH):
            head = Outputs(n, 4, False)                                  # the first four steps with the basis: step by step
            rep4 = raw_call(s, op, start, 4, head)
            assert rep4.steps_taken == 4 and rep4.evaluated == 1 and (rep4.n, rep4.nnz) == (n, len(col))
            step_by_step(rp, col, val, start, rhs, g, None, rep4, head.alpha, head.beta, head.scale, head.columns(), want_scale[op])
            host_part_agrees(rep4, head.alpha, head.beta, head.ritz, 4)
            out = Outputs(n, 32, False, basis=False)                      # 32 steps without it
            rep = raw_call(s, op, start, 32, out)
            print(scene, precision, "op", op, "start", start, "n", n, "lambda", rep.lambda_min, rep.lambda_max, "bounds", rep.lambda_min_bound,
                  rep.lambda_max_bound, "gershgorin", rep.gershgorin_max, "kappa", rep.condition_estimate, "iterations", rep.iteration_bound)
            assert rep.steps_taken == 32 and not rep.breakdown and not rep.nonfinite and rep.bad_diagonal == 0 and rep.indefinite == 0
            assert out.scale.tobytes() == head.scale.tobytes() and rep.gershgorin_max == rep4.gershgorin_max
            assert out.alpha[:4].tobytes() == head.alpha.tobytes() and out.beta[:5].tobytes() == head.beta.tobytes()     # the same recurrence, longer
            host_part_agrees(rep, out.alpha, out.beta, out.ritz, 32)
            assert 0 < rep.lambda_min <= rep.lambda_max <= rep.gershgorin_max * (1 + 2.0 ** -40)
            slack = 64 * EPS * rep.lambda_max                             # T_4 is the leading block of T_32: the Ritz interval only grows
            assert rep.lambda_min <= rep4.lambda_min + slack and rep.lambda_max >= rep4.lambda_max - slack
            dev = Outputs(n, 4, True)                                     # device destinations: the same bytes
            drep = raw_call(s, op, start, 4, dev, capi.MEM_DEVICE)
            assert bytes(drep) == bytes(rep4) and host(dev.scale).tobytes() == head.scale.tobytes() and host(dev.basis).tobytes() == head.basis.tobytes()
            assert dev.alpha.tobytes() == head.alpha.tobytes() and dev.beta.tobytes() == head.beta.tobytes() and dev.ritz.tobytes() == head.ritz.tobytes()
    # all 32 steps step by step once per context: the Jacobi-scaled operator from the initial residual
    deep = Outputs(n, 32, False)
    rep = raw_call(s, M.JACOBI, M.RESIDUAL, 32, deep)
    step_by_step(rp, col, val, M.RESIDUAL, rhs, g, None, rep, deep.alpha, deep.beta, deep.scale, deep.columns(), want_scale[M.JACOBI])


def test_fresh_context_and_capped_grid_give_the_same_bytes(frames, monkeypatch):
    s = frames("beam32_L3").s
    n = int(s.info().n_velocity)
    want = Outputs(n, 16, False)
    rep = raw_call(s, M.JACOBI, M.RESIDUAL, 16, want)
    g = Frame("beam32_L3")
    try:
        def same():
            got = Outputs(n, 16, False)
            r = raw_call(g.s, M.JACOBI, M.RESIDUAL, 16, got)
            return bytes(r) == bytes(rep) and all(getattr(got, f).tobytes() == getattr(want, f).tobytes() for f in ("alpha", "beta", "ritz", "scale", "basis"))
        assert same() and same()
        for cap in ("1", "3"):
            monkeypatch.setenv("AVS_CELLS_GRID_CAP", cap)
            try:
                g.s.set_solver_option(capi.OPTION_RELOAD_ENVIRONMENT, 1)             # (the environment is read at avs_create)
                assert same(), cap
            finally:
                monkeypatch.delenv("AVS_CELLS_GRID_CAP")
                g.s.set_solver_option(capi.OPTION_RELOAD_ENVIRONMENT, 1)
    finally:
        g.close()


# ---- 5. no side effects -------------------------------------------------------------------------------------------------------------------------
def test_an_estimating_context_solves_as_one_that_does_not(built_lib):
    def frame(estimating):
        f = Frame("beam32_L3", estimate_first=estimating)
        s = f.s
        info = s.solve(1e-8, 3000)
        if estimating:
            assert f.first.steps_taken == 8 and s.estimate_spectrum(op=capi.SPECTRUM_OF_MATRIX, start=capi.SPECTRUM_START_HASH, steps=8).steps_taken == 8
            again = s.solve(1e-8, 3000)                                                 # ... and once more behind an estimate
            assert (again.iterations, again.converged, again.error) == (info.iterations, info.converged, info.error)
        out = [s.csr(), s.initial_guess(), s.solution(), (info.iterations, info.converged, info.error)]
        f.close()
        return out

    (csr_a, g_a, x_a, i_a), (csr_b, g_b, x_b, i_b) = frame(False), frame(True)
    assert i_a == i_b and i_a[1] == 1
    assert all(a.tobytes() == b.tobytes() for a, b in zip(csr_a, csr_b))
    assert g_a.tobytes() == g_b.tobytes() and x_a.tobytes() == x_b.tobytes() and np.abs(x_a).max() > 0


@pytest.mark.parametrize("name", ["tri_257", "tri_257_vector", "arrow", "unordered_repeated", "bad_column", "bad_row_ptr", "n_0"])
def test_device_arrays_are_interior_slices_and_stay_untouched(built_lib, name):
    c = sc.case(name)
    op = c.ops[-1]
    given = c.given if c.given is not None else np.zeros(c.n)
    pad = {"rp": (3, 5), "col": (1, 7), "val": (1, 3), "b": (3, 1), "x0": (5, 1), "given": (1, 2), "scale": (1, 3), "basis": (3, 2)}   # 4- and 8-byte starts only
    src = {"rp": (c.row_ptr, -1), "col": (c.col, -2**31), "val": (c.val, np.nan), "b": (c.b, np.nan), "x0": (c.x0, np.nan), "given": (given, np.nan),
           "scale": (np.full(c.n, POISON), POISON), "basis": (np.full((c.steps + 1) * c.n, POISON), POISON)}
    bufs, views = {}, {}
    for k, (a, poison) in src.items():
        before, behind = pad[k]
        bufs[k] = torch.from_numpy(np.concatenate([np.full(before, poison, a.dtype), a, np.full(behind, poison, a.dtype)])).to(DEV)
        views[k] = bufs[k][before:before + len(a)]
    copies = {k: b.clone() for k, b in bufs.items()}
    torch.cuda.synchronize()
    out = Outputs(c.n, c.steps, False, scale=False, basis=False)
    out.scale, out.basis = views["scale"], views["basis"]
    st, rep, err = call_csr(c, tuple(views[k] for k in ("rp", "col", "val", "b", "x0", "given")), capi.MEM_DEVICE, op, out)
    assert st == capi.OK, err
    want = sc.model(name, op)
    assert rep.evaluated == want["evaluated"] and rep.steps_taken == want["steps_taken"]
    for k in ("rp", "col", "val", "b", "x0", "given"):
        assert bufs[k].cpu().numpy().tobytes() == copies[k].cpu().numpy().tobytes(), k
    for k in ("scale", "basis"):
        before, behind = pad[k]
        frame = bufs[k].cpu().numpy()
        assert (frame[:before] == POISON).all() and (frame[len(frame) - behind:] == POISON).all(), k
        if not rep.evaluated:
            assert (frame == POISON).all()
    if rep.evaluated and c.n:
        ref = Outputs(c.n, c.steps, False)
        st, rep2, err = call_csr(c, arrays_of(c), capi.MEM_HOST, op, ref)
        filled = (rep.steps_taken + 1) * c.n
        assert st == capi.OK and bytes(rep2) == bytes(rep) and host(views["scale"]).tobytes() == ref.scale.tobytes()
        assert host(views["basis"])[:filled].tobytes() == ref.basis[:filled].tobytes() and out.alpha.tobytes() == ref.alpha.tobytes()
        assert (host(views["basis"])[filled:] == POISON).all()               # device columns behind the last vector stay untouched


@pytest.mark.parametrize("size", [8, 12, 40, 64, 128, 136, 144])
def test_only_struct_size_bytes_are_written(built_lib, size):
    c = sc.case("tri_257")
    small = Outputs(c.n, c.steps, False, scale=False, basis=False)
    st, full, err = call_csr(c, arrays_of(c), capi.MEM_HOST, M.JACOBI, small)
    assert st == capi.OK and full.steps_taken == c.steps, err
    rep = capi.Spectrum()
    C.memset(C.byref(rep), 0x5a, C.sizeof(rep))
    rep.struct_size = size
    st, _, err = call_csr(c, arrays_of(c), capi.MEM_HOST, M.JACOBI, small, rep=rep)
    assert st == capi.OK, err
    got, want = bytes(rep), bytes(full)
    assert rep.struct_size == size and got[4:size] == want[4:size] and got[size:] == b"\x5a" * max(C.sizeof(rep) - size, 0)


# ---- 6. errors and state ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_have_messages(built_lib):
    c = sc.case("tri_255")
    out = Outputs(c.n, c.steps, False)
    good = dict(c=c, arrays=arrays_of(c), where=capi.MEM_HOST, op=M.JACOBI, out=out)
    assert call_csr(**good)[0] == capi.OK
    tiny, absurd = capi.Spectrum(), capi.Spectrum()
    tiny.struct_size, absurd.struct_size = 4, 5000
    rp, col, val, b, x0, given = arrays_of(c)
    bad = [dict(rep=tiny), dict(rep=absurd), dict(rep=False), dict(n=-1), dict(nnz=-1), dict(n=2**31), dict(nnz=2**31), dict(op=2), dict(op=-1),
           dict(start=3), dict(start=-1), dict(steps=0), dict(steps=-1), dict(steps=capi.SPECTRUM_MAX_STEPS + 1),
           dict(arrays=(None, col, val, b, x0, None)), dict(arrays=(rp, None, val, b, x0, None)), dict(arrays=(rp, col, None, b, x0, None)),
           dict(arrays=(rp, col, val, None, x0, None)), dict(arrays=(rp, col, val, b, None, None)), dict(start=M.VECTOR), dict(device=-1),
           dict(device=torch.cuda.device_count()), dict(where=7)]
    for change in bad:
        st, _, err = call_csr(**{**good, **change})
        assert st == capi.EINVAL and err, (change.keys(), st, err)
    st, rep, err = call_csr(c, (rp, col, val, None, None, None), capi.MEM_HOST, M.JACOBI, out, start=M.HASH)      # the hash start reads neither b nor x0
    assert st == capi.OK and rep.steps_taken == c.steps, err
    st, rep, err = call_csr(c, arrays_of(c), capi.MEM_HOST, M.JACOBI, Outputs(c.n, 512, False, basis=False), steps=512)   # the largest number of steps: n decides
    assert st == capi.OK and 0 < rep.steps_taken <= c.n and rep.steps_asked == 512, err
    assert call_csr(**good)[0] == capi.OK


def test_states_are_refused_with_messages(frames):
    f = Frame("beam32_L3")
    s, lib = f.s, f.s.lib
    rep = capi.Spectrum()
    call = lambda h, op=0, start=0, steps=8, where=capi.MEM_HOST, report=rep: lib.avs_estimate_spectrum(
        h, op, start, steps, 1e-3, None, None, None, None, None, where, C.byref(report) if report is not None else None)
    try:
        assert f.before_assemble[0] == capi.ESTATE and b"no system" in f.before_assemble[1]
        assert call(s.h) == capi.OK and rep.steps_taken == 8
        tiny = capi.Spectrum()
        tiny.struct_size = 4
        for kw in (dict(op=2), dict(start=M.VECTOR), dict(start=5), dict(steps=0), dict(steps=513), dict(where=7), dict(report=None), dict(report=tiny)):
            assert call(s.h, **kw) == capi.EINVAL and lib.avs_last_error(), kw
        assert call(None) == capi.EINVAL
        buf = (C.c_uint8 * capi.UNIQUE_ID_BYTES)()
        capi.check(lib.avs_dist_get_unique_id(buf))
        capi.check(lib.avs_dist_init(s.h, buf, 0, 1))
        s.dist_partition()
        assert call(s.h) == capi.OK                                              # the global matrix is still there
        s.dist_assemble()
        assert call(s.h) == capi.ESTATE and b"no system" in lib.avs_last_error()
    finally:
        f.close()
    # a slab-local context (this rank's window of the lattices only)
    scn = scenes.to_device(SCENES["sphere32"](), torch.device(DEV))
    pp = DevicePrepass(scn.res, scn.dx, scn.levels, device=0)
    pp.set_slab(0, [0, scn.res[0] // 2, scn.res[0]], 0, lambda p, count, stream: None)
    info = pp.run(scn.liquid, scn.solid)
    s2 = ViscositySolve(scn.res, scn.dx, scn.dt, info.levels, device=0)
    try:
        pp.apply(s2)
        assert call(s2.h) == capi.ESTATE and b"slab" in lib.avs_last_error()
    finally:
        s2.close()
        pp.close()


# ---- 7. the Python wrappers ------------------------------------------------------------------------------------------------------------------
def test_python_wrappers(frames):
    c = sc.case("blocks")
    out = Outputs(c.n, c.steps, False)
    st, rep, err = call_csr(c, arrays_of(c), capi.MEM_HOST, M.JACOBI, out)
    assert st == capi.OK, err
    r = estimate_csr_spectrum(c.row_ptr, c.col, c.val, c.b, c.x0, steps=c.steps, scale=True, basis=True)
    for f in ("evaluated", "steps_taken", "lambda_min", "lambda_max", "lambda_min_bound", "lambda_max_bound", "gershgorin_max", "condition_estimate",
              "iteration_bound", "start_norm", "breakdown", "indefinite"):
        assert getattr(r, f) == getattr(rep, f), f
    assert r.alpha.tobytes() == out.alpha.tobytes() and r.beta.tobytes() == out.beta.tobytes() and r.ritz.tobytes() == out.ritz.tobytes()
    assert r.scale.tobytes() == out.scale.tobytes() and r.basis.tobytes() == out.basis.tobytes() and r.basis.shape == (c.steps + 1, c.n)
    assert estimate_csr_spectrum(c.row_ptr, c.col, c.val, steps=4).start == capi.SPECTRUM_START_HASH
    v = sc.case("tri_257_vector")
    assert estimate_csr_spectrum(v.row_ptr, v.col, v.val, start_vector=v.given, op=capi.SPECTRUM_OF_MATRIX, steps=v.steps).lambda_max == \
        call_csr(v, arrays_of(v), capi.MEM_HOST, M.MATRIX, Outputs(v.n, v.steps, False))[1].lambda_max
    b = sc.case("bad_column")
    assert not estimate_csr_spectrum(b.row_ptr, b.col, b.val, b.b, b.x0).evaluated
    s = frames("sphere32").s
    n = int(s.info().n_velocity)
    raw = Outputs(n, 8, False)
    rep = raw_call(s, M.JACOBI, M.RESIDUAL, 8, raw, tolerance=1e-8)
    w = s.estimate_spectrum(steps=8, tolerance=1e-8, scale=True, basis=True)
    assert (w.lambda_min, w.lambda_max, w.condition_estimate, w.iteration_bound, w.steps_taken) == \
        (rep.lambda_min, rep.lambda_max, rep.condition_estimate, rep.iteration_bound, 8)
    assert w.ritz.tobytes() == raw.ritz.tobytes() and w.scale.tobytes() == raw.scale.tobytes() and w.basis.tobytes() == raw.basis.tobytes()
    d = s.estimate_spectrum(steps=8, tolerance=1e-8, scale=True, basis=True, device_arrays=True)
    assert d.basis.cpu().numpy().tobytes() == raw.basis.tobytes() and d.scale.cpu().numpy().tobytes() == raw.scale.tobytes() and d.lambda_min == rep.lambda_min
