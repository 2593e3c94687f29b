"""The CU-resident PCG loop on small CSR systems at every edge of its plan (tests/resident_edges.py), iterate by iterate.

Seam A with max_iterations = k returns exactly x_k, `iterations` and error = sqrt(r_k.r_k / b.b) of the resident loop.  Every case is
solved through avs_pcg_csr_plan (libavs_probe.so: avs_pcg_csr + the plan the solve ran), under the case's AVS_* environment, and

  * the reported plan has the property the case is named for -- the instantiation (NG, STREAM, LT), the long-row lanes and their
    longest tail, the lane count, the fill trips, the remap passes, the tables per workgroup -- or, for a decline, used == 0 and the
    reason; a plan without streamed rows also has exactly the lanes, long-row lanes and tail of the restated lane rule;
  * x_k and error at k = 0, 1, 2, 3, 4, 7, 8 (few-row cases: every k up to their convergence) are within the rule of the long-double
    host model (tests/resident_model.py: 32 max(s_k, 2^-50), s_k measured from two fp64 summation orders -- never another GPU loop),
    iterations == k, k = 0 returns x0 bit for bit and a second call at the last k the same bits;
  * two loose tolerances stop at the model's `iterations` (one odd, one even) with the model's iterate, b = 0 gives x = 0, the model's
    converged solution as the initial guess is returned untouched after 0 iterations;
  * the solve to 1e-10 leaves a true residual (the oracle's product) <= 10 tol |b|.

A row dropped from one dot product, a stale column read for one iteration or a lost x += alpha p at an odd exit all still converge to
the same answer in about as many steps; tests/test_resident_model.py shows that each leaves this rule by a factor of 100 at least.

Unreachable on a small system: none of the edges resident_edges.py lists.  One is reached differently than first written: inside a
streamed plan a lane's stream takes any row of which it is owed half the quads, so an arrow row of 80 entries (16 quads) became a
streamed row, not a long-row lane; tier_ng3_stream carries an arrow row of 1,000 entries, which no stream is ever owed.  The measured
scales, the GPU's deviations (at most 0.10 of the bound) and the mutation ratios of the validating run are in profiles/resident_edges.md.
"""
import ctypes as C
import math

import numpy as np
import pytest

import resident_edges as R
import resident_model as M
from adaptiveviscositysolver_amd import capi
from oracle import oracle as O

pytestmark = pytest.mark.gpu


_gpu_error = []     # a call that came back with an error status: nothing more is started on the device by this module


def _solve(lib, c, b, x0, tol, max_iters):
    x = np.array(x0, np.float64, copy=True)
    b = np.ascontiguousarray(b, np.float64)
    info, plan = capi.SolveInfo(), capi.ResidentPlanInfo()
    try:
        capi.check(lib.avs_pcg_csr_plan(c.n, c.row_ptr.ctypes.data, c.col.ctypes.data, c.val.ctypes.data, b.ctypes.data, x.ctypes.data,
                                        float(tol), int(max_iters), capi.MEM_HOST, 0, None, C.byref(info), C.byref(plan)))
    except capi.AvsError as err:
        _gpu_error.append(f"{c.name}: {err}")
        raise
    return x, info, plan


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_plan(c, info, plan):
    e, why = c.expect, plan.why.decode()
    what = (c.name, {f: getattr(plan, f) for f, _ in plan._fields_ if f != "why"}, why)
    print(f"PLAN {c.name}: " + ", ".join(f"{k} {v}" for k, v in what[1].items() if k != "struct_size") + (f", why '{why}'" if why else ""))
    if "declined" in e:
        assert plan.used == 0 and info.resident == 0 and e["declined"] in why, what
        return
    assert plan.used == 1 and info.resident == 1 and why == "", what
    lens = R.row_lengths(c)
    assert 1 <= plan.max_lanes_per_workgroup <= R.LANES and plan.lanes <= plan.workgroups * R.LANES, what
    assert 0 <= plan.ng <= 3 and 0 < plan.lds_bytes <= 160 * 1024, what
    for key in ("workgroups", "ng", "local_tables", "tables_per_workgroup", "lanes", "longest_tail", "max_quads", "max_remote", "remap_passes"):
        if key in e:
            assert getattr(plan, key) == e[key], (key, e[key], what)
    if "long_row_lanes" in e:
        want = int((lens > 5).sum()) if e["long_row_lanes"] == "rows_over_5" else e["long_row_lanes"]
        assert plan.long_row_lanes == want, what
    if "stream" in e:
        assert (plan.streamed_rows > 0) == e["stream"], what
    if "fill_trips" in e:
        assert -(-plan.max_remote // R.FILL) == e["fill_trips"], what
    if plan.streamed_rows == 0:
        assert plan.streamed_words == 0 and plan.max_lane_streamed_rows == 0, what
        assert (plan.lanes, plan.long_row_lanes, plan.longest_tail) == R.lanes_in_registers(lens, plan.max_quads), what
        assert plan.max_remote <= R.SRC_LIST, what
    else:
        assert plan.streamed_words >= plan.streamed_rows and 1 <= plan.max_lane_streamed_rows <= 127, what
        # (streams start where the rows do not fit 93 % of the lanes' registers, and bring the lanes under 97 %)
        assert R.lanes_in_registers(lens, plan.max_quads)[0] > 0.93 * R.LANES * plan.workgroups >= 0.93 / 0.97 * plan.lanes, what
        assert plan.max_remote <= R.SRC_LIST_STREAM, what
    if plan.local_tables:
        assert 2 <= plan.largest_table <= (4096 if plan.tables_per_workgroup == 1 else 2048), what


@pytest.mark.parametrize("name", R.NAMES)
def test_resident_edge(name, built_lib, monkeypatch):
    assert not _gpu_error, f"not run: an earlier call failed on the device ({_gpu_error[0]})"
    lib = capi.load_probe()
    c = R.get(name)
    for k in R.RESIDENT_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    declined = "declined" in c.expect
    rp64 = c.row_ptr.astype(np.int64)
    bnorm = math.sqrt(math.fsum((c.b * c.b).tolist()))

    # ---- finish: the solve to 1e-10, and the plan it ran ----
    tol = 1e-10
    x, info, plan = _solve(lib, c, c.b, c.x0, tol, 2000)
    _check_plan(c, info, plan)
    assert info.converged == 1, (name, info.iterations, info.error)
    r = c.b - O.spmv_csr(rp64, c.col, c.val, x)
    assert math.sqrt(math.fsum((r * r).tolist())) <= 10 * tol * bnorm, name
    if declined:
        return

    # ---- iterates ----
    model = R.model_of(c)
    ks = R.checked_ks(c, model)
    last = None
    for k in ks:
        xk, info, plan = _solve(lib, c, c.b, c.x0, 0.0, k)
        dx, de = M.x_dev(xk, model.ld, k), M.error_dev(info.error, model.ld, k)
        sx, se = model.s[k]
        print(f"REC {name} k {k} s_x {sx:.3e} dev_x {dx:.3e} bound_x {model.bound_x(k):.3e} s_e {se:.3e} dev_e {de:.3e} "
              f"bound_e {model.bound_error(k):.3e} iterations {info.iterations}")
        what = (name, k)
        assert info.resident == 1 and plan.used == 1, what + (plan.why.decode(),)
        assert info.iterations == k and info.converged == 0, what + (info.iterations, info.converged)
        assert dx <= model.bound_x(k), what + (dx, model.bound_x(k))
        assert de <= model.bound_error(k), what + (de, model.bound_error(k))
        if k == 0:
            assert np.array_equal(_bits(xk), _bits(c.x0)), what
        last = (k, xk, info)
    k, xk, info = last
    x2, info2, _ = _solve(lib, c, c.b, c.x0, 0.0, k)
    assert np.array_equal(_bits(x2), _bits(xk)) and _bits([info2.error]) == _bits([info.error]) and info2.iterations == info.iterations, (name, k)

    # ---- exits ----
    for tol_e, iters, passes in model.exit_tolerances():
        xe, info, _ = _solve(lib, c, c.b, c.x0, tol_e, 100)
        dx = M.x_dev(xe, model.ld, passes)
        print(f"REC {name} exit tol {tol_e:.6e} iterations {info.iterations} (model {iters}) dev_x {dx:.3e} bound_x {model.bound_x(passes):.3e}")
        assert info.resident == 1 and info.iterations == iters and info.converged == 1, (name, tol_e, info.iterations, iters)
        assert dx <= model.bound_x(passes), (name, tol_e, dx, model.bound_x(passes))
    xz, info, _ = _solve(lib, c, np.zeros(c.n), c.x0, tol, 100)
    assert not xz.any() and info.error == 0.0 and info.converged == 1 and info.iterations == 0, (name, "b = 0")
    done = M.run(model.A, c.b, c.x0, 1e-13, 2000, "asc64")
    assert done.converged[-1]
    xs = done.x[-1]
    xd, info, _ = _solve(lib, c, c.b, xs, tol, 100)
    assert info.iterations == 0 and info.converged == 1 and np.array_equal(_bits(xd), _bits(xs)), (name, "converged x0", info.iterations)
