"""numpy model of the partitioned mixed-precision loops (AVS_OPTION_DIST_MIXED_PRECISION; csrc/avs_pcg.hip, k_sr_mixed_residual): the
specification the kernels are compared with.

Chronopoulos-Gear single-reduction PCG (Jacobi) on float vectors r, u, w, p, s and a correction xf; x, b, the matrix values, every row sum
(rounded to float once), every dot product (terms widened) and alpha, beta, rho, the threshold stay fp64.  Behind every `period`
iterations, and whenever the recurrence's r.r claims convergence, the reliable update folds xf into x, recomputes r = (float)(b - A x) in
fp64, u = D^-1 r, w = A u, and the step of that iteration is taken on the sums of the TRUE residual (p and s are kept).
One rank: the partition changes the order of the sums, not the scheme."""
import numpy as np

f32, f64 = np.float32, np.float64


def _system(rp, col, val):
    rp = np.asarray(rp, dtype=np.int64)
    rows = np.repeat(np.arange(len(rp) - 1), rp[1:] - rp[:-1])
    diag = np.zeros(len(rp) - 1)
    d = rows == col
    diag[rows[d]] = val[d]
    return rp, diag


def sr_pcg_f64(rp, col, val, b, x0, tol, max_iters):
    """the fp64 single-reduction loop (OP_SR_INIT / OP_SR_STEP): (x, iterations, converged)"""
    rp, diag = _system(rp, col, val)
    spmv = lambda v: np.add.reduceat(val * v[col], rp[:-1])
    invd = np.where(diag != 0., 1. / np.where(diag != 0., diag, 1.), 1.)
    x = x0.astype(f64).copy()
    r = b - spmv(x)
    u = invd * r
    w = spmv(u)
    thr = max(tol * tol * float(b @ b), 2.2250738585072014e-308)
    if float(r @ r) < thr:
        return x, 0, True
    rho = float(r @ u)
    alpha, beta = rho / float(w @ u), 0.
    p, s = np.zeros_like(x), np.zeros_like(x)
    it = 0
    while it < max_iters:
        p = u + beta * p
        s = w + beta * s
        x += alpha * p
        r -= alpha * s
        u = invd * r
        w = spmv(u)
        gamma, rr, delta = float(r @ u), float(r @ r), float(w @ u)
        if rr < thr:
            return x, it, True
        beta = gamma / rho
        alpha = gamma / (delta - beta * gamma / alpha)
        rho = gamma
        it += 1
    return x, it, False


def sr_pcg_mixed(rp, col, val, b, x0, tol, max_iters, period=32):
    """the mixed-precision form: (x, iterations, converged, reliable updates, |b - A x| / |b| of the last update)"""
    rp, diag = _system(rp, col, val)
    spmv64 = lambda v: np.add.reduceat(val * v[col], rp[:-1])
    spmv_mixed = lambda v: np.add.reduceat(val * v[col].astype(f64), rp[:-1]).astype(f32)   # fp64 values and row sums, rounded once
    dot = lambda a, c: float(a.astype(f64) @ c.astype(f64))
    d32 = diag.astype(f32)
    invd = np.where(d32 != 0, f32(1) / np.where(d32 != 0, d32, f32(1)), f32(1)).astype(f32)
    x = x0.astype(f64).copy()
    bb = float(b @ b)
    thr = max(tol * tol * bb, 2.2250738585072014e-308)
    r64 = b - spmv64(x)
    r = r64.astype(f32)
    u = invd * r
    w = spmv_mixed(u)
    rr = float(r64 @ r64)
    err = lambda: float(np.sqrt(rr / bb)) if bb else 0.
    if rr < thr:
        return x, 0, True, 0, err()
    rho = dot(r, u)
    alpha, beta = rho / dot(w, u), 0.
    xf, p, s = np.zeros_like(r), np.zeros_like(r), np.zeros_like(r)
    it = updates = 0
    while it < max_iters:
        chunk = min(period, max_iters - it)
        for k in range(chunk):
            a, bt = f32(alpha), f32(beta)
            p = u + bt * p
            s = w + bt * s
            xf = xf + a * p
            r = r - a * s
            u = invd * r
            w = spmv_mixed(u)
            gamma, rr_rec, delta = dot(r, u), dot(r, r), dot(w, u)
            if k == chunk - 1 or rr_rec < thr:
                break                       # the step of this iteration is the update's
            beta = gamma / rho
            alpha = gamma / (delta - beta * gamma / alpha)
            rho = gamma
            it += 1
        x += xf.astype(f64)
        xf[:] = 0
        r64 = b - spmv64(x)
        r = r64.astype(f32)
        u = invd * r
        w = spmv_mixed(u)
        rr = float(r64 @ r64)
        updates += 1
        if rr < thr:
            return x, it, True, updates, err()
        gamma, delta = dot(r, u), dot(w, u)
        beta = gamma / rho
        alpha = gamma / (delta - beta * gamma / alpha)
        rho = gamma
        it += 1
    return x, it, False, updates, err()
