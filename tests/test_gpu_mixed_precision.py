"""AVS_OPTION_MIXED_PRECISION (csrc/avs_pcg_mixed.inl): fp64 contexts iterate on float vectors; the answer and the stopping test stay fp64
through a reliable update (x += xf, r = b - A x in fp64, p kept) behind every chunk of 32 iterations.

Scenes as in test_gpu_f32_loop.py.  Every scene's pre-pass, oracle and assembly are made once per module (`case`): the context first runs
the fp64 launch-per-phase loop (option 0: the yardstick every test compares with, taken before the context has ever seen the option), then
is assembled again with the option set."""
import ctypes as C

import numpy as np
import pytest
import torch

from adaptiveviscositysolver_amd import ViscositySolve, capi, scenes
from util import build_pyramid, feed, oracle_from_pyramid, rel_l2

pytestmark = pytest.mark.gpu

SCENES = {
    "beam128_L4": (lambda: scenes.fat_beam(128, 4), True),                                     # brick form, one dictionary
    "sheet128_L4": (lambda: scenes.thin_sheet(128, 4, thickness_cells=12), True),
    "beam128_L4_varvisc": (lambda: scenes.fat_beam(128, 4, variable_viscosity=True), True),    # brick form, value-code variant
    "beam64_L3_stream": (lambda: scenes.fat_beam(64, 3), False),                               # no form: the streaming kernel, one dictionary
    "sphere32_L3_stream": (lambda: scenes.sphere(32, 3, radius=0.36), False),                  # ... thousands of values
    "beam32_varvisc_stream": (lambda: scenes.fat_beam(32, 2, wall=True, variable_viscosity=True), False),
}
TIGHT = 1e-10


def _make(sc, pyr, brick, probe=True, precision=capi.PRECISION_F64, env=None):
    """a context created under AVS_BRICK = 1 / 0 (the environment is read once, at avs_create), resident loop off"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("AVS_BRICK", "1" if brick else "0")
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        dsc = scenes.to_device(sc, torch.device("cuda:0"))
        s = ViscositySolve(sc.res, sc.dx, sc.dt, pyr.levels, device=0, probe=probe, precision=precision)
    feed(s, pyr)
    s.set_scene_fields(dsc)
    s.set_solver_option(capi.OPTION_RESIDENT_LOOP, 0)
    return s


def _product(s, x, flags):
    dev = torch.device("cuda:0")
    dx = torch.from_numpy(x).to(dev)
    dy = torch.full((len(x),), float("nan"), dtype=torch.float64, device=dev)
    dot = C.c_double()
    capi.check(s.lib.avs_spmv_solver_form(s.h, dx.data_ptr(), dy.data_ptr(), flags, C.byref(dot)))
    return dy.cpu().numpy(), dot.value


def _row_sums64(rp, col, val, x):
    """s = 0.; s += val[k] * x[col[k]] for k in the row's stored order: one fp64 multiply, one fp64 add per entry"""
    rp = np.asarray(rp, dtype=np.int64)
    length = rp[1:] - rp[:-1]
    s = np.zeros(len(rp) - 1)
    for j in range(int(length.max())):
        m = length > j
        k = rp[:-1][m] + j
        s[m] = s[m] + val[k] * x[col[k]]
    return s


def _residual_and_bound(rp, col, val, b, x):
    """|b - A x| / |b| in numpy, and the bound on the difference of two fp64 evaluations of it that add in different orders:
    2 (m + 2) 2^-53 | |A||x| + |b| |_2 / |b|_2, m = the longest row"""
    rp = np.asarray(rp, dtype=np.int64)
    ax = np.add.reduceat(val * x[col], rp[:-1])
    absax = np.add.reduceat(np.abs(val) * np.abs(x[col]), rp[:-1])
    m = int((rp[1:] - rp[:-1]).max())
    nb = float(np.linalg.norm(b))
    return float(np.linalg.norm(b - ax)) / nb, 2.0 * (m + 2) * 2.0 ** -53 * float(np.linalg.norm(absax + np.abs(b))) / nb


class Case:
    pass


@pytest.fixture(scope="module", params=list(SCENES))
def case(request, built_lib):
    name = request.param
    make, brick = SCENES[name]
    c = Case()
    c.name, c.brick = name, brick
    c.sc = make()
    c.pyr = build_pyramid(c.sc)
    c.s = s = _make(c.sc, c.pyr, brick)
    ai = s.assemble()
    c.n = int(ai.n_velocity)
    c.rp, c.col, c.val, c.rhs = s.csr()
    c.x0 = s.initial_guess()
    rng = np.random.default_rng(11)
    c.xprobe = (rng.standard_normal(c.n) * (10.0 ** rng.integers(-3, 4, c.n))).astype(np.float32).astype(np.float64)
    # the fp64 launch-per-phase loop on a context that has never seen the option
    c.y64, _ = _product(s, c.xprobe, 0)
    c.fresh = {}
    for tol in (1e-5, TIGHT):
        info = s.solve(tol, 20000)
        fmt = s.matrix_format()
        assert info.converged == 1 and info.resident == 0 and fmt.float_vectors == 0 and fmt.reliable_updates == 0
        c.fresh[tol] = (int(info.iterations), s.solution())
    c.oracle = oracle_from_pyramid(c.sc, c.pyr)
    c.oracle.hot_path()
    s.set_solver_option(capi.OPTION_MIXED_PRECISION, 1)
    s.assemble()
    yield c
    s.close()


def test_mixed_product(case):
    """the loop's product: y = float32(sum_k float64(x[col]) * val) of the context's own CSR within one float ulp per row (contraction and
    nothing else may differ); the fp64 product of the updates, launched on the walk laid out for the mixed kernel, equals the fp64
    loop's product bit for bit"""
    c, s = case, case.s
    fmt = s.matrix_format()
    if c.brick:
        assert fmt.brick_tiles > 0 and fmt.brick_pattern_rows >= 0.5 * c.n, "the brick form did not run"
        assert fmt.brick_value_codes == (1 if "varvisc" in c.name else 0)
    else:
        assert fmt.brick_tiles == 0
    want64 = _row_sums64(c.rp, c.col, c.val, c.xprobe)
    want = want64.astype(np.float32)
    for fused in (0, 1):
        got, dot = _product(s, c.xprobe, fused)
        assert np.array_equal(got, got.astype(np.float32).astype(np.float64))          # y is a float vector
        gf = got.astype(np.float32)
        ulps = np.abs(gf.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
        print(f"{c.name}: fused {fused}: rows that differ from the rounded fp64 row sum: {int((gf != want).sum())}, worst {float(ulps.max()):.2f} ulp")
        assert float(ulps.max()) <= 1.0, (c.name, fused, float(ulps.max()))
        if fused:
            terms = c.xprobe * want64
            assert abs(dot - float(terms.sum())) <= 1e-10 * max(1.0, float(np.abs(terms).sum()))
    got64, _ = _product(s, c.xprobe, 2)
    assert np.array_equal(got64.view(np.int64), c.y64.view(np.int64)), (c.name, int((got64 != c.y64).sum()))


def test_mixed_tight_tolerance(case):
    """tol = 1e-10 within twice the fp64 loop's iterations (a condition, not a target: the CPU model of the scheme needs <= 1.18 x): the
    fp64 residual the solve reports is the residual of the solution it returns

    Measured iteration ratios (mixed / fp64 loop, MI355X): see DESIGN.md 4.1a."""
    c, s = case, case.s
    it64, x64 = c.fresh[TIGHT]
    info = s.solve(TIGHT, 2 * it64)
    x = s.solution()
    fmt = s.matrix_format()
    res, bound = _residual_and_bound(c.rp, c.col, c.val, c.rhs, x)
    xo, io = c.oracle.solve(TIGHT, 20000)
    print(f"{c.name}: tol 1e-10: mixed {info.iterations} iterations, {fmt.reliable_updates} updates; fp64 loop {it64}; ratio {info.iterations / it64:.3f}; "
          f"info.error {info.error:.3e}, numpy residual {res:.3e} (bound on the difference {bound:.1e}); rel_l2 vs oracle {rel_l2(x, xo):.2e}, "
          f"vs the fp64 loop {rel_l2(x, x64):.2e}; {info.solve_ms:.2f} ms")
    assert info.converged == 1 and info.error < TIGHT
    assert fmt.float_vectors == 1 and info.resident == 0
    assert fmt.reliable_updates >= info.iterations // 32
    assert abs(res - info.error) <= bound, (res, info.error, bound)
    assert rel_l2(x, xo) < 1e-5


@pytest.mark.parametrize("tol", [1e-3, 1e-5])
def test_mixed_default_tolerances(case, tol):
    """iterations within max(3, 1 %) of the oracle's fp64 CG, the margin the fp64 loop is granted"""
    c, s = case, case.s
    info = s.solve(tol, 20000)
    xo, io = c.oracle.solve(tol, 20000)
    print(f"{c.name}: tol {tol:g}: mixed {info.iterations} iterations, oracle fp64 CG {io.iterations}; info.error {info.error:.3e}")
    assert info.converged == 1 and info.error < tol
    assert abs(info.iterations - io.iterations) <= max(3, io.iterations // 100), (info.iterations, io.iterations)


def test_mixed_exits(case):
    """max_iterations and avs_cancel leave the last iterate in x: the fp64 residual reported is the residual of what is returned"""
    c, s = case, case.s
    info = s.solve(TIGHT, 40)
    x = s.solution()
    fmt = s.matrix_format()
    res, bound = _residual_and_bound(c.rp, c.col, c.val, c.rhs, x)
    print(f"{c.name}: 40 iterations: info.error {info.error:.6e}, numpy residual {res:.6e} (bound {bound:.1e}), {fmt.reliable_updates} updates")
    assert info.converged == 0 and info.cancelled == 0 and info.iterations == 40 and fmt.reliable_updates == 2
    assert abs(res - info.error) <= bound, (res, info.error, bound)
    assert not np.array_equal(x, c.x0)
    capi.check(s.lib.avs_cancel(s.h))
    info = s.solve(TIGHT, 5000)
    assert info.cancelled == 1 and info.converged == 0 and info.iterations == 0
    assert np.array_equal(s.solution().view(np.int64), c.x0.view(np.int64))
    again = s.solve(1e-5, 5000)
    assert again.converged == 1 and again.cancelled == 0


def test_mixed_is_deterministic_and_switches_off_cleanly(case):
    """two mixed solves: same count, same updates, same bits.  Option 0 and a new assembly: the fp64 loop exactly as a context that never
    saw the option runs it"""
    c, s = case, case.s
    a = s.solve(1e-5, 20000)
    xa, fa = s.solution(), s.matrix_format()
    b = s.solve(1e-5, 20000)
    xb, fb = s.solution(), s.matrix_format()
    assert a.iterations == b.iterations and fa.reliable_updates == fb.reliable_updates > 0 and fa.float_vectors == 1
    assert np.array_equal(xa.view(np.int64), xb.view(np.int64))
    s.set_solver_option(capi.OPTION_GRAPH_REPLAY, 0)          # chunks enqueued launch by launch: same count, same bits
    g = s.solve(1e-5, 20000)
    assert g.iterations == a.iterations and np.array_equal(s.solution().view(np.int64), xa.view(np.int64))
    s.set_solver_option(capi.OPTION_GRAPH_REPLAY, 1)
    try:
        s.set_solver_option(capi.OPTION_MIXED_PRECISION, 0)
        off = s.solve(1e-5, 20000)                             # (takes effect at the next avs_assemble)
        assert s.matrix_format().float_vectors == 1 and off.iterations == a.iterations
        s.assemble()
        off = s.solve(1e-5, 20000)
        fmt = s.matrix_format()
        it, x = c.fresh[1e-5]
        assert fmt.float_vectors == 0 and fmt.reliable_updates == 0 and off.resident == 0
        assert off.iterations == it and np.array_equal(s.solution().view(np.int64), x.view(np.int64))
    finally:
        s.set_solver_option(capi.OPTION_MIXED_PRECISION, 1)
        s.assemble()


def test_mixed_environment_variable_equals_the_option(built_lib):
    make, brick = SCENES["beam64_L3_stream"]
    sc = make()
    pyr = build_pyramid(sc)
    s = _make(sc, pyr, brick, probe=False)
    s.set_solver_option(capi.OPTION_MIXED_PRECISION, 1)
    s.assemble()
    a = s.solve(1e-5, 20000)
    xa, fa = s.solution(), s.matrix_format()
    s.close()
    e = _make(sc, pyr, brick, probe=False, env={"AVS_MIXED_PRECISION": "1"})
    e.assemble()
    b = e.solve(1e-5, 20000)
    xb, fb = e.solution(), e.matrix_format()
    e.close()
    assert fa.float_vectors == 1 and fb.float_vectors == 1 and fa.reliable_updates == fb.reliable_updates > 0
    assert a.iterations == b.iterations and np.array_equal(xa.view(np.int64), xb.view(np.int64))


def test_mixed_leaves_the_resident_loop_its_systems(built_lib):
    """with the resident loop left on, a system it takes keeps it (fp64)"""
    sc = scenes.fat_beam(64, 3)
    pyr = build_pyramid(sc)
    s = _make(sc, pyr, False, probe=False)
    s.set_solver_option(capi.OPTION_RESIDENT_LOOP, 1)
    s.set_solver_option(capi.OPTION_MIXED_PRECISION, 1)
    s.assemble()
    info = s.solve(1e-5, 5000)
    fmt = s.matrix_format()
    assert info.converged == 1 and info.resident == 1 and fmt.float_vectors == 0 and fmt.reliable_updates == 0
    s.close()


def test_mixed_no_effect_on_float_contexts_and_plain_cg(built_lib):
    """an AVS_PRECISION_F32 context ignores the option; AVS_PRECONDITIONER_NONE runs mixed too"""
    sc = scenes.fat_beam(64, 3, wall=True)
    pyr = build_pyramid(sc)
    f = _make(sc, pyr, False, probe=False, precision=capi.PRECISION_F32)
    f.set_solver_option(capi.OPTION_F32_VECTORS, 1)
    f.assemble()
    ref = f.solve(1e-5, 8000)
    xr = f.solution()
    f.set_solver_option(capi.OPTION_MIXED_PRECISION, 1)
    f.assemble()
    got = f.solve(1e-5, 8000)
    assert got.iterations == ref.iterations and np.array_equal(f.solution(), xr) and f.matrix_format().reliable_updates == 0
    f.close()
    s = _make(sc, pyr, False, probe=False)
    s.set_solver_option(capi.OPTION_PRECONDITIONER, capi.PRECONDITIONER_NONE)
    s.assemble()
    plain = s.solve(1e-8, 20000)
    x64 = s.solution()
    s.set_solver_option(capi.OPTION_MIXED_PRECISION, 1)
    s.assemble()
    info = s.solve(1e-8, 2 * plain.iterations)
    fmt = s.matrix_format()
    print(f"plain CG at 1e-8: fp64 loop {plain.iterations}, mixed {info.iterations} iterations")
    assert info.converged == 1 and info.error < 1e-8 and fmt.float_vectors == 1 and fmt.reliable_updates > 0
    assert rel_l2(s.solution(), x64) < 1e-5
    s.close()


def test_what_plain_float_cannot_do(built_lib):
    """tol = 1e-10 on beam64_L3_stream: the float-vector loop of an AVS_PRECISION_F32 context stops far above it (its recurrence claims
    convergence, the true residual does not follow); the mixed loop's true residual is below the tolerance -- why the option exists"""
    make, brick = SCENES["beam64_L3_stream"]
    sc = make()
    pyr = build_pyramid(sc)
    s = _make(sc, pyr, brick, probe=False)
    s.set_solver_option(capi.OPTION_MIXED_PRECISION, 1)
    s.assemble()
    rp, col, val, rhs = s.csr()
    mi = s.solve(TIGHT, 5000)
    res_mixed, _ = _residual_and_bound(rp, col, val, rhs, s.solution())
    s.close()
    f = _make(sc, pyr, brick, probe=False, precision=capi.PRECISION_F32)
    f.set_solver_option(capi.OPTION_F32_VECTORS, 1)
    f.assemble()
    fi = f.solve(TIGHT, 5000)
    res_float, _ = _residual_and_bound(rp, col, val, rhs, f.solution())
    f.close()
    print(f"beam64_L3_stream at 1e-10: true residual |b - A x| / |b| against the fp64 system: mixed {res_mixed:.3e} ({mi.iterations} iterations), "
          f"float loop {res_float:.3e} ({fi.iterations} iterations, converged = {fi.converged})")
    assert res_mixed < TIGHT
    assert not res_float < TIGHT
