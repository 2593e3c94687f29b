"""tests/pcg_scalar_model.py on the CPU: the model the scalar stages and the single-reduction vector kernels are compared with must not be a
transcription that only agrees with itself.

  * every summation order returns nb (nb + 1) / 2 EXACTLY on a[i] = i + 1 (all partial sums < 2^53 are exact whatever the order, so a
    skipped or twice-counted index shows), and stays within d 2^-53 sum |a_i| of math.fsum on random data, d the additions on the longest
    path of that order (derived per order below, not tuned);
  * the phase-loop ops (OP_INIT, OP_RHO0, OP_ALPHA / OP_ALPHA_ODD, OP_BETA) drive a plain PCG loop to the oracle's iteration count,
    verdict and x;
  * OP_SR_INIT / OP_SR_STEP drive dist_mixed_model.sr_pcg_f64's loop to its iterates bit for bit, the _F32 ops a float loop to an x
    whose fp64 residual passes the float threshold;
  * k_mixed_finish and k_sr_mixed_begin / k_sr_mixed_step take dist_mixed_model.sr_pcg_mixed's decisions on its own system.
"""
import math

import numpy as np
import pytest

import pcg_scalar_model as M
from adaptiveviscositysolver_amd import scenes
from dist_mixed_model import sr_pcg_f64, sr_pcg_mixed
from pcg_scalar_model import SCALARS, f32, f64
from util import oracle_for_scene

U = 2.0 ** -53


def scalars():
    return np.zeros(1, SCALARS)[0]


# ---------------------------------------------------------------------------------------------------------------------------------------
# sums
# ---------------------------------------------------------------------------------------------------------------------------------------
def depth_block(n):
    """additions on the longest path of reduce_block(n): thread 0 has the most entries, ceil(n / 1024); K four-deep trips put one entry
    each into s0 .. s3, the tail goes into s0 -- s0's chain is K + (entries - 4 K) long (every += counted, the first onto 0. too); then
    (s0 + s1) + (s2 + s3): 2, wave_sum: 6, the 16 waves ascending from 0.: 16"""
    entries = -(-n // 1024)
    K = max(0, -(-(n - 3072) // 4096))
    assert entries - 4 * K >= 0
    return K + (entries - 4 * K) + 2 + 6 + 16


def depth_mb(n):
    """the longest block (a full share), then wave_sum over the 64 block sums: 6"""
    return depth_block(-(-n // 64)) + 6


def depth_finish(n):
    """one accumulator per thread: ceil(n / 1024), wave_sum: 6, 16 waves"""
    return -(-n // 1024) + 6 + 16


ORDERS = {"reduce": (M.reduce_block, depth_block), "reduce_mb": (M.reduce_mb, depth_mb), "finish": (M.finish_sum, depth_finish),
          "reduce_launch": (M.reduce_launch_sum, lambda n: depth_mb(n) if n >= M.MB_FROM else depth_block(n))}
SIZES = {"reduce": [0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 5119, 8192, 8193],
         "reduce_mb": [1, 63, 64, 65, 127, 16383, 16384, 16385, 65536, 65537, 262144, 262145, 64 * 4097],
         "finish": [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049],
         "reduce_launch": [16383, 16384]}


def sixteen_decades(rng, n):
    """mixed signs over sixteen decades: another order changes bits"""
    return rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)


@pytest.mark.parametrize("order", list(ORDERS))
def test_every_index_is_summed_exactly_once(order):
    fn, _ = ORDERS[order]
    for nb in SIZES[order]:
        assert fn(np.arange(1, nb + 1, dtype=f64)) == nb * (nb + 1) // 2, (order, nb)


def test_block_sums_of_the_vector_kernels_are_exact():
    for g in (1, 2, 3, 8):
        for n in (1, 255, 256, 257, 256 * g - 1, 256 * g, 256 * g + 1, 2 * 256 * g + 5, 3 * 256 * g):
            for acc in (f64, f32):          # (float: a thread's own sum of at most three rows stays below 2^24; the rest is double)
                s, = M.grid_sums(g, acc, np.arange(1, n + 1).astype(acc))
                assert s.sum() == n * (n + 1) // 2, (g, n, acc)
                # workgroup blk owns the rows i with (i // 256) % g == blk
                i = np.arange(n)
                for blk in range(g):
                    assert s[blk] == (i[(i // 256) % g == blk] + 1).sum(), (g, n, blk)


@pytest.mark.parametrize("order", list(ORDERS))
def test_sums_stay_within_the_bound_of_their_longest_path(order):
    fn, depth = ORDERS[order]
    rng = np.random.default_rng(7)
    worst = 0.
    for nb in SIZES[order]:
        for _ in range(3):
            a = sixteen_decades(rng, nb)
            bound = depth(nb) * U * float(np.abs(a).sum())
            err = abs(float(fn(a)) - math.fsum(a))
            assert err <= bound, (order, nb, err, bound)
            if bound:
                worst = max(worst, err / bound)
    print(f"{order}: largest |sum - fsum| / (d 2^-53 sum|a|) = {worst:.3f}")


def test_vector_block_sums_stay_within_their_bound():
    """trips additions per thread, wave_sum: 6, ((w0 + w1) + w2) + w3: 3"""
    rng = np.random.default_rng(8)
    worst = 0.
    for g in (1, 3, 8):
        for n in (257, 2 * 256 * g + 5, 3 * 256 * g):
            a = sixteen_decades(rng, n)
            s, = M.grid_sums(g, f64, a)
            i = np.arange(n)
            for blk in range(g):
                mine = a[(i // 256) % g == blk]
                bound = (-(-n // (256 * g)) + 6 + 3) * U * float(np.abs(mine).sum())
                err = abs(float(s[blk]) - math.fsum(mine))
                assert err <= bound, (g, n, blk, err, bound)
                if bound:                  # (a workgroup without rows: 0 <= 0)
                    worst = max(worst, err / bound)
    print(f"block_sum: largest ratio to the bound {worst:.3f}")


def test_the_orders_differ_on_the_test_data():
    """the data the GPU tests use tells the orders apart on most arrays: a kernel that summed in another order would not match bit for bit
    over the cases of a test"""
    rng = np.random.default_rng(9)
    differ = np.zeros(3, int)
    for _ in range(40):
        a = sixteen_decades(rng, 8193)
        v = [float(M.reduce_block(a)), float(M.reduce_mb(a)), float(M.finish_sum(a))]
        differ += [v[0] != v[1], v[0] != v[2], v[1] != v[2]]
    assert (differ > 20).all(), differ


# ---------------------------------------------------------------------------------------------------------------------------------------
# phase-loop ops against the oracle
# ---------------------------------------------------------------------------------------------------------------------------------------
def csr_of(dense):
    n = len(dense)
    rows, cols = np.nonzero(dense)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return rp, cols.astype(np.int32), dense[rows, cols]


def spd_systems():
    """small SPD systems with a non-constant diagonal (Jacobi matters)"""
    out = {}
    n = 120                                    # 1-D diffusion, variable coefficient
    k = 1.0 + 0.9 * np.sin(0.37 * np.arange(n + 1))
    A = np.diag(k[:-1] + k[1:] + 0.05) - np.diag(k[1:-1], 1) - np.diag(k[1:-1], -1)
    out["diffusion_1d"] = A
    m = 11                                     # 2-D five-point stencil, a different weight per row
    L = np.kron(np.eye(m), 2 * np.eye(m) - np.eye(m, k=1) - np.eye(m, k=-1))
    L = L + np.kron(2 * np.eye(m) - np.eye(m, k=1) - np.eye(m, k=-1), np.eye(m))
    d = 1.0 + np.arange(m * m) % 7
    out["poisson_2d_scaled"] = np.sqrt(d)[:, None] * L * np.sqrt(d)[None, :] + 0.1 * np.eye(m * m)
    rng = np.random.default_rng(5)             # a random sparse SPD matrix, diagonal entries over a decade
    B = rng.standard_normal((90, 90)) * (rng.random((90, 90)) < 0.08)
    S = B @ B.T + np.diag(10.0 ** rng.uniform(0, 1, 90))
    out["random_spd"] = S
    return out


def phase_pcg(rp, col, val, b, x0, tol, max_iters, fused_parity):
    """Jacobi-PCG (Eigen's ConjugateGradient) with every scalar decision taken by the model's ops on a PcgScalars record.
    fused_parity: r.z alternates between rho and rho_alt as in the loops with the beta step folded into update_xp (OP_ALPHA_ODD on odd
    positions); else OP_ALPHA / OP_BETA.  Returns x, the record and r.r / threshold of every iteration."""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    spmv = lambda v: np.bincount(rows, val * v[col], minlength=len(b))
    diag = np.zeros(len(b))
    diag[rows[rows == col]] = val[rows == col]
    invd = np.where(diag != 0., 1. / np.where(diag != 0., diag, 1.), 1.)
    sc = scalars()
    x = x0.copy()
    r = b - spmv(x)
    sc["red"][:2] = float(b @ b), float(r @ r)
    M.apply_scalar_op(sc, M.OP_INIT, tol)
    if sc["done"] == 3:
        x[:] = 0.
    hist = []
    if sc["done"]:
        return x, sc, hist
    p = invd * r
    sc["red"][0] = float(r @ p)
    M.apply_scalar_op(sc, M.OP_RHO0, tol)
    c = 0
    while True:
        if sc["done"] == 0 and sc["iter"] >= max_iters:
            break
        odd = fused_parity and (c & 1)
        t = spmv(p)
        sc["red"][0] = float(p @ t)
        was = int(sc["done"])
        M.apply_scalar_op(sc, M.OP_ALPHA_ODD if odd else M.OP_ALPHA, tol)
        if was == 2:
            assert sc["done"] == 1
            break
        r = r - sc["alpha"] * t
        z = invd * r
        if fused_parity:                       # what update_xp's folded step does: OP_BETA on the slot of this parity
            sc["red"][:2] = float(r @ r), float(r @ z)
            old = sc["rho_alt"] if odd else sc["rho"]
            keep = sc["rho"].copy()
            sc["rho"] = old
            M.apply_scalar_op(sc, M.OP_BETA, tol)
            new = sc["rho"].copy()
            sc["rho"] = keep
            if sc["done"] == 0:
                sc["rho" if odd else "rho_alt"] = new
        else:
            sc["red"][:2] = float(r @ r), float(r @ z)
            M.apply_scalar_op(sc, M.OP_BETA, tol)
        hist.append(float(sc["rr"] / sc["threshold"]))
        x = x + sc["alpha"] * p               # (done == 2: the pending update of the converged iteration)
        if sc["done"] == 0:
            p = z + sc["beta"] * p
        c += 1
    return x, sc, hist


@pytest.mark.parametrize("fused_parity", [False, True])
@pytest.mark.parametrize("tol", [1e-3, 1e-10])
@pytest.mark.parametrize("name", list(spd_systems()))
def test_phase_loop_ops_reproduce_the_oracle(name, tol, fused_parity):
    import oracle.oracle as orc
    A = spd_systems()[name]
    n = len(A)
    rp, col, val = csr_of(A)
    rng = np.random.default_rng(n)
    b, x0 = rng.standard_normal(n), 0.1 * rng.standard_normal(n)
    xo, info = orc.pcg_csr(rp, col, val, b, x0, tol, 2500)
    x, sc, hist = phase_pcg(rp, col, val, b, x0, tol, 2500, fused_parity)
    # the count is not marginal: the last iteration's r.r is well below the threshold and the one before well above, and the count is
    # well below n (beyond it the recurrence has lost its orthogonality and r.r follows the rounding errors)
    assert hist[-1] < 0.9 and (len(hist) < 2 or hist[-2] > 1.1), (name, tol, hist[-2:])
    assert int(sc["iter"]) == info.iterations, (name, tol, int(sc["iter"]), info.iterations)
    assert (sc["done"] == 1) == (info.error < tol) and sc["done"] == 1
    assert info.iterations < 0.7 * n
    # x: the two runs differ in the order of their dot products and row sums only.  Each of the k iterations commits relative errors of at
    # most n 2^-53 per dot product / row sum (n terms) in a handful of vector operations; a perturbation of that size in the residual
    # moves x = A^-1 (b - r) by at most cond(A) times as much, relative to |x|.  First order, one such term per iteration:
    k = max(1, info.iterations)
    bound = k * n * U * np.linalg.cond(A)
    rel = float(np.linalg.norm(x - xo) / np.linalg.norm(xo))
    print(f"{name} tol {tol:g} parity {fused_parity}: {k} iterations, |x - x_oracle| / |x| = {rel:.3e}, bound {bound:.3e}, ratio {rel / bound:.3e}")
    assert rel <= bound, (name, tol, rel, bound)


def test_phase_loop_ops_at_a_zero_right_hand_side_and_a_converged_start():
    A = spd_systems()["diffusion_1d"]
    rp, col, val = csr_of(A)
    n = len(A)
    x, sc, _ = phase_pcg(rp, col, val, np.zeros(n), np.ones(n), 1e-3, 10, False)
    assert sc["done"] == 3 and not x.any() and sc["rr"] == 0.
    xs = np.linalg.solve(A, np.ones(n))
    x, sc, _ = phase_pcg(rp, col, val, np.ones(n), xs, 1e-3, 10, False)
    assert sc["done"] == 1 and sc["iter"] == 0 and np.array_equal(x, xs)


# ---------------------------------------------------------------------------------------------------------------------------------------
# single-reduction ops against dist_mixed_model
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def beam():
    o = oracle_for_scene(scenes.fat_beam(32, 2, wall=True, variable_viscosity=True))
    o.prepass()
    o.hot_path()
    A = o.csr()
    return np.asarray(A.row_ptr, np.int64), np.asarray(A.col), np.asarray(A.val), np.asarray(A.rhs), np.asarray(o.initial_guess(), np.float64)


def _diag(rp, col, val):
    rows = np.repeat(np.arange(len(rp) - 1), rp[1:] - rp[:-1])
    diag = np.zeros(len(rp) - 1)
    diag[rows[rows == col]] = val[rows == col]
    return diag


def sr_ops_pcg(T, rp, col, val, b, x0, tol, max_iters):
    """the loop of dist_mixed_model.sr_pcg_f64 in the vector type T, every scalar from OP_SR_INIT / OP_SR_STEP (T float: the _F32 ops)"""
    init, step = (M.OP_SR_INIT, M.OP_SR_STEP) if T is f64 else (M.OP_SR_INIT_F32, M.OP_SR_STEP_F32)
    val = val.astype(T)
    spmv = lambda v: np.add.reduceat(val * v[col], rp[:-1])
    diag = _diag(rp, col, val)
    invd = np.where(diag != 0, T(1) / np.where(diag != 0, diag, T(1)), T(1)).astype(T)
    dot = lambda a, c: float(a.astype(f64) @ c.astype(f64)) if T is f32 else float(a @ c)
    x = x0.astype(T)
    bt = b.astype(T)
    r = bt - spmv(x)
    u = invd * r
    w = spmv(u)
    sc = scalars()
    sc["red"][:] = dot(bt, bt), dot(r, u), dot(r, r), dot(w, u)
    M.apply_scalar_op(sc, init, tol)
    p, s = np.zeros_like(x), np.zeros_like(x)
    while not sc["done"] and sc["iter"] < max_iters:
        a, be = T(sc["alpha"]), T(sc["beta"])
        p = u + be * p
        s = w + be * s
        x += a * p
        r -= a * s
        u = invd * r
        w = spmv(u)
        sc["red"][:3] = dot(r, u), dot(r, r), dot(w, u)
        M.apply_scalar_op(sc, step, tol)
        assert x.dtype == T and r.dtype == T
    return x, sc


@pytest.mark.parametrize("tol,cap", [(1e-5, 5000), (1e-10, 5000), (1e-10, 40)])
def test_sr_ops_give_the_fp64_models_iterates_bit_for_bit(beam, tol, cap):
    rp, col, val, b, x0 = beam
    want, it, ok = sr_pcg_f64(rp, col, val, b, x0, tol, cap)
    x, sc = sr_ops_pcg(f64, rp, col, val, b, x0, tol, cap)
    assert (int(sc["iter"]), bool(sc["done"] == 1)) == (it, ok) and sc["done"] in (0, 1)
    assert x.tobytes() == want.tobytes()
    assert ok == (cap == 5000)


def test_sr_f32_ops_reach_the_float_threshold(beam):
    rp, col, val, b, x0 = beam
    tol = 1e-3
    bf = b.astype(f32).astype(f64)
    x, sc = sr_ops_pcg(f32, rp, col, val.astype(f32).astype(f64), bf, x0, tol, 5000)
    assert sc["done"] == 1 and 0 < sc["iter"] < 5000
    thr = f32(tol) * f32(tol) * f32(sc["rhs_norm2"])
    assert sc["threshold"] == f64(thr) and f32(sc["rr"]) < thr
    r = bf - np.add.reduceat(val.astype(f32).astype(f64) * x.astype(f64)[col], rp[:-1])
    print(f"float single-reduction ops: {int(sc['iter'])} iterations, fp64 |r|^2 / threshold = {float(r @ r) / float(thr):.3f}")
    assert float(r @ r) < float(thr)
    for name in ("rho", "alpha", "beta", "rr", "threshold", "rhs_norm2"):      # the float ops keep doubles that hold floats
        assert f64(f32(sc[name])) == sc[name], name


def sr_mixed_ops(rp, col, val, b, x0, tol, max_iters, period=32):
    """dist_mixed_model.sr_pcg_mixed's schedule -- chunks of `period` iterations of the float recurrence, a reliable update behind each --
    with OP_SR_INIT, the step folded into k_sr_update (OP_SR_STEP's arithmetic), k_sr_mixed_begin and k_sr_mixed_step deciding"""
    spmv64 = lambda v: np.add.reduceat(val * v[col], rp[:-1])
    spmv_mixed = lambda v: np.add.reduceat(val * v[col].astype(f64), rp[:-1]).astype(f32)
    dot = lambda a, c: float(a.astype(f64) @ c.astype(f64))
    d32 = _diag(rp, col, val).astype(f32)
    invd = np.where(d32 != 0, f32(1) / np.where(d32 != 0, d32, f32(1)), f32(1)).astype(f32)
    x = x0.astype(f64).copy()
    r64 = b - spmv64(x)
    r = r64.astype(f32)
    u = invd * r
    w = spmv_mixed(u)
    sc = scalars()
    sc["red"][:] = float(b @ b), dot(r, u), float(r64 @ r64), dot(w, u)
    M.apply_scalar_op(sc, M.OP_SR_INIT, tol)
    xf, p, s = np.zeros_like(r), np.zeros_like(r), np.zeros_like(r)
    updates, decisions = 0, []
    while not sc["done"] and sc["iter"] < max_iters:
        chunk = min(period, max_iters - int(sc["iter"]))
        for k in range(chunk):
            if k > 0:
                M.apply_scalar_op(sc, M.OP_SR_STEP, tol)          # (the step k_sr_update takes first: sr_step<double>)
            if sc["done"]:
                break                                             # frozen: the rest of the chunk returns at once
            a, bt = f32(sc["alpha"]), f32(sc["beta"])
            p = u + bt * p
            s = w + bt * s
            xf = xf + a * p
            r = r - a * s
            u = invd * r
            w = spmv_mixed(u)
            sc["red"][:3] = dot(r, u), dot(r, r), dot(w, u)
        frozen = bool(sc["done"])
        M.sr_mixed_begin(sc)
        assert sc["done"] == 0
        x += xf.astype(f64)
        xf[:] = 0
        r64 = b - spmv64(x)
        r = r64.astype(f32)
        u = invd * r
        w = spmv_mixed(u)
        sc["red"][:3] = dot(r, u), float(r64 @ r64), dot(w, u)
        before = int(sc["iter"])
        M.sr_mixed_step(sc)
        updates += 1
        decisions.append((frozen, int(sc["done"]), int(sc["iter"]) - before))
    return x, sc, updates, decisions


@pytest.mark.parametrize("tol,cap", [(1e-5, 5000), (1e-10, 5000), (1e-10, 40)])
def test_sr_mixed_ops_take_the_mixed_models_decisions(beam, tol, cap):
    rp, col, val, b, x0 = beam
    want, it, ok, updates, err = sr_pcg_mixed(rp, col, val, b, x0, tol, cap)
    x, sc, n_upd, decisions = sr_mixed_ops(rp, col, val, b, x0, tol, cap)
    assert (int(sc["iter"]), bool(sc["done"] == 1), n_upd) == (it, ok, updates)
    assert x.tobytes() == want.tobytes()
    assert math.sqrt(float(sc["rr"] / sc["rhs_norm2"])) == err
    # every update but a converging one counts its iteration, frozen chunk or not
    assert all(step == (0 if done else 1) for _, done, step in decisions)
    assert [d for _, d, _ in decisions[:-1]] == [0] * (len(decisions) - 1) and decisions[-1][1] == (1 if ok else 0)


def phase_mixed_ops(rp, col, val, b, x0, tol, max_iters, period=32):
    """the launch-per-phase mixed loop (csrc/avs_pcg_mixed.inl) on sr_pcg_mixed's update schedule: float recurrence of the standard CG,
    scalars by OP_ALPHA and update_xp's folded beta step, k_mixed_finish<true> at the start and k_mixed_finish<false> behind every chunk"""
    spmv64 = lambda v: np.add.reduceat(val * v[col], rp[:-1])
    spmv_mixed = lambda v: np.add.reduceat(val * v[col].astype(f64), rp[:-1]).astype(f32)
    dot = lambda a, c: float(a.astype(f64) @ c.astype(f64))
    d32 = _diag(rp, col, val).astype(f32)
    invd = np.where(d32 != 0, f32(1) / np.where(d32 != 0, d32, f32(1)), f32(1)).astype(f32)
    x = x0.astype(f64).copy()
    sc = scalars()

    def residual(init):
        r64 = b - spmv64(x)
        r = r64.astype(f32)
        part = [float(r64 @ r64), dot(r, invd * r)] + ([float(b @ b)] if init else [])
        M.mixed_finish(sc, np.array(part), 1, tol, init)
        return r, part[0]

    r, _ = residual(True)
    p = invd * r
    xf = np.zeros_like(r)
    updates, decisions = 0, []
    while not sc["done"] and sc["iter"] < max_iters:
        for k in range(min(period, max_iters - int(sc["iter"]))):
            t = spmv_mixed(p)
            sc["red"][0] = dot(p, t)
            M.apply_scalar_op(sc, M.OP_ALPHA, tol)
            if sc["done"]:
                break
            a = f32(sc["alpha"])
            r = r - a * t
            z = invd * r
            sc["red"][:2] = dot(r, r), dot(r, z)
            M.apply_scalar_op(sc, M.OP_BETA, tol)
            xf = xf + a * p
            if sc["done"] == 2:                # frozen: p keeps owing its beta step, rho is the r.z the iteration started from
                continue                       # (the next OP_ALPHA steps 2 -> 1)
            p = z + f32(sc["beta"]) * p
        entered = int(sc["done"])
        x += xf.astype(f64)
        xf[:] = 0
        before = int(sc["iter"])
        r, rr = residual(False)
        updates += 1
        decisions.append((entered, rr < sc["threshold"], int(sc["done"]), int(sc["iter"]) - before, float(sc["red"][3])))
        if sc["red"][3] == 1. and not sc["done"]:
            p = invd * r + f32(sc["beta"]) * p
    return x, sc, updates, decisions


@pytest.mark.parametrize("tol", [1e-5, 1e-10])
def test_mixed_finish_takes_the_mixed_models_decisions(beam, tol):
    rp, col, val, b, x0 = beam
    _, it, ok, updates, err = sr_pcg_mixed(rp, col, val, b, x0, tol, 5000)
    x, sc, n_upd, decisions = phase_mixed_ops(rp, col, val, b, x0, tol, 5000)
    print(f"tol {tol:g}: mixed model {it} iterations / {updates} updates, k_mixed_finish loop {int(sc['iter'])} / {n_upd}; decisions {decisions}")
    assert ok and sc["done"] == 1
    # the two recurrences are the same Krylov method in exact arithmetic: the margin tests/test_dist_mixed_model.py grants them
    assert abs(int(sc["iter"]) - it) <= max(3, int(0.01 * it))
    assert n_upd >= int(sc["iter"]) // 32
    true = float(np.linalg.norm(b - np.add.reduceat(val * x[col], rp[:-1])) / np.linalg.norm(b))
    assert true < tol and math.sqrt(float(sc["rr"] / sc["rhs_norm2"])) < tol
    for entered, below, done, counted, owes in decisions:
        assert done == (1 if below else 0)                              # the fp64 sum decides, whatever the recurrence claimed
        assert counted == (1 if (entered and not below) else 0)         # a rejected claim: that iteration counts, here
        assert owes == float(counted)
    assert [d[2] for d in decisions[:-1]] == [0] * (len(decisions) - 1)


def test_mixed_finish_counts_the_step_of_a_rejected_claim(beam):
    """tol 1e-13 on chunks of 64: the float recurrence claims convergence mid-chunk, the fp64 residual does not confirm it -- the frozen
    iteration counts at the update, p takes its beta step there, and the solve goes on to converge as the mixed model does"""
    rp, col, val, b, x0 = beam
    tol = 1e-13
    _, it, ok, updates, err = sr_pcg_mixed(rp, col, val, b, x0, tol, 3000, period=64)
    x, sc, n_upd, decisions = phase_mixed_ops(rp, col, val, b, x0, tol, 3000, period=64)
    assert ok and sc["done"] == 1 and err < tol
    true = float(np.linalg.norm(b - np.add.reduceat(val * x[col], rp[:-1])) / np.linalg.norm(b))
    assert true < tol
    rejected = [d for d in decisions if d[0] and not d[1]]
    assert rejected and all(d[2:] == (0, 1, 1.0) for d in rejected), decisions
    for entered, below, done, counted, owes in decisions:
        assert done == (1 if below else 0) and counted == (1 if (entered and not below) else 0) and owes == float(counted)
