"""The launch-per-phase PCG loop (pcg_solve_phases, csrc/avs_pcg.hip) on small CSR systems at every edge of its host loop
(tests/phase_edges.py), iterate by iterate.

Seam A with max_iterations = k returns exactly x_k, `iterations` and error = sqrt(r_k.r_k / b.b) of the loop.  Every case is solved through
libavs_probe.so (avs_pcg_csr + avs_phase_loop_info: what the loop of that solve did) under the case's AVS_* environment -- always with
AVS_CG_RESIDENT=0 and AVS_PCG_FUSE_VECTORS=0: this loop, its two vector launches -- and

  * finish: the solve to 1e-10 converges with resident == 0 and a true residual (the oracle's product) <= 10 tol |b|, and the loop's
    report shows the property the case is named for: nb, g, coded, the alpha step folded or launched, fuse_beta, replayed chunks exactly
    where the graph is on and a second chunk was enqueued, no capture and no replay with the graph off;
  * iterates: x_k and error at the case's checked k are within the rule of the long-double host model (tests/phase_model.py:
    32 max(s_k, 2^-50), s_k measured from two fp64 summation orders -- never another GPU loop), iterations == k, converged == 0, the
    report shows exactly the chunks k iterations take (replayed and launched), k = 0 returns x0 bit for bit, a second call at the last k
    the same bits, and at every k the run with AVS_PCG_GRAPH flipped returns the same bits: it launches the same kernels;
  * exits (the n = 4,099 cases): six tolerances stop in iterations 3 or 4, 31, 32, 33, 34 and 70 -- odd and even positions, the last
    launch of a chunk and the first of the next, inside a replayed graph -- with the model's `iterations` and iterate, converged == 1,
    under max_iterations = 200 (a whole chunk of no-op launches follows) and under a cap equal to the converging iteration (done == 2
    is then what the host polls); b = 0 gives x = 0; a converged initial guess is returned untouched after 0 iterations;
  * one context (a scene with the brick form): the same rule at k = 0, 1, 2, 8, 33, 64, 96 on the context's own system, then the
    workspace's graph is reused by a second solve, dropped for another tolerance and captured again.

r.z taken from the wrong parity slot, a pending x update lost or applied twice, a replayed graph that reads a stale scalar, the odd last
row left out of a sum all still converge to the same answer in about as many steps; tests/test_phase_model.py shows that each leaves this
rule by a factor of 1e8 at least.  Not reached here: k_update_fused in the loop (tests/test_gpu_fused_vectors.py requires it bit-equal to
the pair checked here), k_reduce_mb (above 1 M rows), the partitioned loops, the float and mixed loops.  The measured scales, the GPU's
deviations (at most 0.05 of the bound) and the loop reports of the validating run are in profiles/phase_edges.md.
"""
import ctypes as C
import math

import numpy as np
import pytest

import phase_edges as R
import phase_model as P
from adaptiveviscositysolver_amd import capi
from oracle import oracle as O

pytestmark = pytest.mark.gpu

REPORT_FIELDS = ("chunks_launched", "chunks_replayed", "graphs_captured", "graph_broken", "alpha_folded", "alpha_launched", "coded", "keep",
                 "fuse_beta", "fuse_vectors", "g", "nb", "float_vectors")

_gpu_error = []     # a call that came back with an error status: nothing more is started on the device by this module


def _guard(what, fn, *args):
    assert not _gpu_error, f"not run: an earlier call failed on the device ({_gpu_error[0]})"
    try:
        return fn(*args)
    except capi.AvsError as err:
        _gpu_error.append(f"{what}: {err}")
        raise


def _report(lib, solves_before):
    rep = capi.PhaseLoopReport()
    capi.check(lib.avs_phase_loop_info(C.byref(rep)))
    assert rep.solves == solves_before + 1, "the solve did not run the launch-per-phase loop"
    return rep


def _solves(lib):
    rep = capi.PhaseLoopReport()
    capi.check(lib.avs_phase_loop_info(C.byref(rep)))
    return rep.solves


def _solve(lib, c, b, x0, tol, max_iters):
    """avs_pcg_csr of the probe library on host arrays -> (x, info, the loop's report of this solve)"""
    x = np.array(x0, np.float64, copy=True)
    b = np.ascontiguousarray(b, np.float64)
    info = capi.SolveInfo()
    before = _solves(lib)
    _guard(c.name, lambda: capi.check(lib.avs_pcg_csr(c.n, c.row_ptr.ctypes.data, c.col.ctypes.data, c.val.ctypes.data, b.ctypes.data,
                                                      x.ctypes.data, float(tol), int(max_iters), capi.MEM_HOST, 0, None, C.byref(info))))
    return x, info, _report(lib, before)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, ia, b, ib):
    return np.array_equal(_bits(a), _bits(b)) and _bits([ia.error]) == _bits([ib.error]) and ia.iterations == ib.iterations and \
        ia.converged == ib.converged


def _rep_str(rep):
    return ", ".join(f"{f} {getattr(rep, f)}" for f in REPORT_FIELDS)


def _check_report(what, rep, expect, enqueued, graph):
    """the loop's report of a solve that enqueued `enqueued` iterations (whole chunks, or max_iterations)"""
    assert rep.graph_broken == 0 and rep.float_vectors == expect["float_vectors"] and rep.fuse_vectors == 0, (what, _rep_str(rep))
    assert (rep.g, rep.coded, rep.fuse_beta) == (expect["g"], expect["coded"], expect["fuse_beta"]), (what, _rep_str(rep), expect)
    assert rep.nb == (expect["nb"] if enqueued else 0), (what, _rep_str(rep), expect)
    folded = enqueued if expect["alpha_folded"] else 0
    assert (rep.alpha_folded, rep.alpha_launched) == (folded, enqueued - folded), (what, _rep_str(rep), enqueued)
    replayed = R.replayed_chunks(enqueued, graph)
    assert (rep.chunks_replayed, rep.chunks_launched) == (replayed, R.launched_chunks(enqueued, graph)), (what, _rep_str(rep), enqueued)
    assert rep.graphs_captured == (1 if replayed else 0), (what, _rep_str(rep))     # (a fresh workspace per call: nothing to reuse)


def _set_env(monkeypatch, env):
    for k in R.PHASE_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _whole_chunks(iterations):
    return -(-iterations // R.K_CHUNK) * R.K_CHUNK


@pytest.mark.parametrize("name", R.NAMES)
def test_phase_edge(name, built_lib, monkeypatch):
    assert not _gpu_error, f"not run: an earlier call failed on the device ({_gpu_error[0]})"
    lib = capi.load_probe()
    c = R.get(name)
    expect = c.expect()
    flipped = {**c.env, "AVS_PCG_GRAPH": "0" if c.graph else "1"}
    _set_env(monkeypatch, c.env)
    rp64 = c.row_ptr.astype(np.int64)
    bnorm = math.sqrt(math.fsum((c.b * c.b).tolist()))

    # ---- finish: the solve to 1e-10, and what the loop did ----
    tol = 1e-10
    x_fin, info, rep = _solve(lib, c, c.b, c.x0, tol, 2000)
    print(f"LOOP {name} finish: iterations {info.iterations}, {_rep_str(rep)}")
    assert info.converged == 1 and info.resident == 0, (name, info.iterations, info.error, info.resident)
    r = c.b - O.spmv_csr(rp64, c.col, c.val, x_fin)
    assert math.sqrt(math.fsum((r * r).tolist())) <= 10 * tol * bnorm, name
    _check_report((name, "finish"), rep, expect, _whole_chunks(info.iterations + 1), c.graph)
    assert (rep.chunks_replayed > 0) == (c.graph and info.iterations + 1 > R.K_CHUNK), (name, _rep_str(rep))

    # ---- iterates ----
    model = R.model_of(c)
    ks = R.checked_ks(c, model)
    last = None
    for k in ks:
        xk, info, rep = _solve(lib, c, c.b, c.x0, 0.0, k)
        dx, de = P.x_dev(xk, model.ld, k), P.error_dev(info.error, model.ld, k)
        sx, se = model.s[k]
        print(f"REC {name} k {k} s_x {sx:.3e} dev_x {dx:.3e} bound_x {model.bound_x(k):.3e} s_e {se:.3e} dev_e {de:.3e} "
              f"bound_e {model.bound_error(k):.3e} iterations {info.iterations} replayed {rep.chunks_replayed} launched {rep.chunks_launched}")
        what = (name, k)
        assert info.resident == 0 and info.iterations == k and info.converged == 0, what + (info.iterations, info.converged, info.resident)
        assert dx <= model.bound_x(k), what + (dx, model.bound_x(k))
        assert de <= model.bound_error(k), what + (de, model.bound_error(k))
        _check_report(what, rep, expect, k, c.graph)
        if k == 0:
            assert np.array_equal(_bits(xk), _bits(c.x0)), what
        # the same launches replayed from a graph / enqueued one by one: the same bits
        _set_env(monkeypatch, flipped)
        xg, info_g, rep_g = _solve(lib, c, c.b, c.x0, 0.0, k)
        _set_env(monkeypatch, c.env)
        _check_report(what + ("graph flipped",), rep_g, expect, k, not c.graph)
        assert _same(xg, info_g, xk, info), what + ("AVS_PCG_GRAPH flipped", P._dev(xg, xk))
        last = (k, xk, info)
    k, xk, info = last
    x2, info2, _ = _solve(lib, c, c.b, c.x0, 0.0, k)
    assert _same(x2, info2, xk, info), (name, k, "second call")

    # ---- exits ----
    for tol_e, iters, it in R.exit_targets(c, model):
        xe, info, rep = _solve(lib, c, c.b, c.x0, tol_e, R.EXIT_MAX_ITERATIONS)
        dx, de = P.x_dev(xe, model.ld, it), P.error_dev(info.error, model.ld, it)
        print(f"REC {name} exit tol {tol_e:.6e} iterations {info.iterations} (model {iters}) dev_x {dx:.3e} bound_x {model.bound_x(it):.3e} "
              f"dev_e {de:.3e} bound_e {model.bound_error(it):.3e} replayed {rep.chunks_replayed} launched {rep.chunks_launched}")
        what = (name, "exit", it)
        assert info.resident == 0 and info.iterations == iters and info.converged == 1, what + (tol_e, info.iterations, info.converged)
        assert dx <= model.bound_x(it) and de <= model.bound_error(it), what + (dx, model.bound_x(it), de, model.bound_error(it))
        _check_report(what, rep, expect, _whole_chunks(it), c.graph)        # (the rest of the chunk: launches that exit at once)
        # a cap equal to the converging iteration: the host polls done == 2, no launch follows that would turn it into 1
        xc, info_c, rep_c = _solve(lib, c, c.b, c.x0, tol_e, it)
        assert info_c.iterations == iters and info_c.converged == 1, what + ("capped", info_c.iterations, info_c.converged)
        assert P.x_dev(xc, model.ld, it) <= model.bound_x(it) and P.error_dev(info_c.error, model.ld, it) <= model.bound_error(it), what + ("capped",)
        _check_report(what + ("capped",), rep_c, expect, it, c.graph)
        assert _same(xc, info_c, xe, info), what + ("capped: other bits than the uncapped solve",)
    xz, info, _ = _solve(lib, c, np.zeros(c.n), c.x0, tol, 100)
    assert not xz.any() and info.error == 0.0 and info.converged == 1 and info.iterations == 0, (name, "b = 0")
    if c.n <= 20000:        # the model's converged solution (a larger system: the solution verified above, against a looser tolerance)
        done = P.run(model.A, c.b, c.x0, 1e-13, 2000, "asc64")
        assert done.converged[-1]
        xs, tol_s = done.x[-1], tol
    else:
        xs, tol_s = x_fin, 1e-8
    xd, info, _ = _solve(lib, c, c.b, xs, tol_s, 100)
    assert info.iterations == 0 and info.converged == 1 and np.array_equal(_bits(xd), _bits(xs)), (name, "converged x0", info.iterations)


# ---------------------------------------------------------------------------------------------------------------------------------------
# one context: the loop over the brick product, with a workspace -- and its captured graph -- that outlives the solve
# ---------------------------------------------------------------------------------------------------------------------------------------
CONTEXT_KS = (0, 1, 2, 8, 33, 64, 96)


def _context_scene():
    """the smallest scene of the suite for which AVS_BRICK=1 builds the form: 17,304 rows, 32 tiles (fat_beam(64, 3, wall=True): 77,328)"""
    from adaptiveviscositysolver_amd import scenes
    return scenes.fat_beam(32, 2, wall=True)


def test_phase_context_workspace_reuse(built_lib, monkeypatch):
    assert not _gpu_error, f"not run: an earlier call failed on the device ({_gpu_error[0]})"
    import torch

    from adaptiveviscositysolver_amd import ViscositySolve, scenes
    from util import build_pyramid, feed
    _set_env(monkeypatch, {"AVS_BRICK": "1"})
    sc = _context_scene()
    pyr = build_pyramid(sc)
    s = ViscositySolve(sc.res, sc.dx, sc.dt, pyr.levels, device=0, probe=True)
    try:
        feed(s, pyr)
        s.set_scene_fields(scenes.to_device(sc, torch.device("cuda:0")))
        s.set_solver_option(capi.OPTION_RESIDENT_LOOP, 0)
        s.set_solver_option(capi.OPTION_FUSED_VECTOR_UPDATE, 0)
        _guard("context", s.assemble)
        fmt = s.matrix_format()
        assert fmt.brick_tiles > 0, "the brick form was not built"
        rp, col, val, b = s.csr()
        x0 = s.initial_guess()
        n = len(b)
        model = P.Model(P.Matrix(rp, col, val), b, x0, max(CONTEXT_KS))
        assert model.live_passes() >= max(CONTEXT_KS) and all(model.bound_x(k) <= 1e-9 for k in CONTEXT_KS)
        lib = s.lib

        def solve(tol, k):
            before = _solves(lib)
            info = _guard("context", s.solve, tol, k)
            return s.solution(), info, _report(lib, before)

        def within(x, info, k, what):
            dx, de = P.x_dev(x, model.ld, k), P.error_dev(info.error, model.ld, k)
            sx, se = model.s[k]
            print(f"REC context n {n} {what} k {k} s_x {sx:.3e} dev_x {dx:.3e} bound_x {model.bound_x(k):.3e} s_e {se:.3e} dev_e {de:.3e} "
                  f"bound_e {model.bound_error(k):.3e} iterations {info.iterations}")
            assert info.resident == 0 and info.iterations == k and info.converged == 0, (what, k, info.iterations, info.converged, info.resident)
            assert dx <= model.bound_x(k) and de <= model.bound_error(k), (what, k, dx, model.bound_x(k), de, model.bound_error(k))

        for k in CONTEXT_KS:
            xk, info, rep = solve(0.0, k)
            print(f"LOOP context k {k}: {_rep_str(rep)}")
            within(xk, info, k, "iterate")
            assert rep.float_vectors == 0 and rep.fuse_vectors == 0 and rep.graph_broken == 0 and rep.fuse_beta == 1, _rep_str(rep)
            assert rep.chunks_replayed == R.replayed_chunks(k) and rep.chunks_launched == R.launched_chunks(k), (k, _rep_str(rep))
            assert rep.alpha_folded + rep.alpha_launched == k
            if k == 0:
                assert np.array_equal(_bits(xk), _bits(x0))
        # (the solves at 64 and 96 above shared tol = 0: the second replayed the first one's graph)
        assert rep.graphs_captured == 0, _rep_str(rep)
        k = 96
        xa, ia, ra = solve(0.0, k)
        xb, ib, rb = solve(0.0, k)
        assert _same(xa, ia, xb, ib) and rb.graphs_captured == 0 and rb.chunks_replayed == 2, _rep_str(rb)
        xc, ic, rc = solve(1e-300, k)          # another tolerance (the threshold stays DBL_MIN: the same iterates): the key changes
        assert rc.graphs_captured == 1 and rc.chunks_replayed == 2, _rep_str(rc)
        xd, idd, rd = solve(0.0, k)            # the first tolerance again: one graph per workspace, so it is captured once more
        assert rd.graphs_captured == 1 and rd.chunks_replayed == 2, _rep_str(rd)
        for x, info, what in ((xa, ia, "first"), (xb, ib, "replay"), (xc, ic, "other tolerance"), (xd, idd, "first tolerance again")):
            within(x, info, k, what)
        assert _same(xc, ic, xa, ia) and _same(xd, idd, xa, ia)
    finally:
        s.close()
