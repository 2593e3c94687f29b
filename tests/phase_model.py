"""Host model of the launch-per-phase PCG loop (pcg_solve_phases, csrc/avs_pcg.hip): the iterates x_k of seam A under max_iterations = k.

The recurrence is the standard one of Eigen's ConjugateGradient, as apply_scalar_op (OP_INIT, OP_RHO0, OP_ALPHA, OP_BETA: csrc/avs_halo.hpp)
and the kernels k_init_residual, k_init_p, k_update_r, k_update_xp implement it:

    set-up     r = b - A x0 ; b.b == 0: x = 0, done ; threshold = max(tol^2 b.b, DBL_MIN) ; r.r < threshold: done, x0 kept
               p = D^-1 r ; rho = r.p
    iteration  t = A p ; alpha = rho / p.t ; r -= alpha t ; rr = r.r ; rz = r.(D^-1 r) ; x += alpha p
               rr < threshold: converged, `iterations` stays (Eigen breaks before i++)
               else beta = rz / rho ; p = D^-1 r + beta p ; rho = rz ; iterations += 1

Row sums run left to right in the stored order, multiply then add (the library is built with -ffp-contract=off), D^-1 is a multiplication
with the rounded inverse of the diagonal, rz sums r_i * (dinv_i * r_i), error = sqrt(rr / b.b).  What a GPU loop may do differently is the
ORDER of the additions inside the dot products; Matrix, the three summation modes ("ld", "asc64", "desc"), the scales s_k and the rule
32 max(s_k, 2^-50) are those of tests/resident_model.py and are imported from there, not restated.

`Mutation` plants the errors of this loop's moving parts that a converged solve cannot see -- r.z read from the wrong parity slot, the
pending x update of the converging iteration lost or applied twice, a row (by default the lone last row of an odd n) left out of one sum,
an alpha left over from the chunk before -- and tests/test_phase_model.py shows that the rule sees each by a factor of 100 at least.
"""
from __future__ import annotations

import math

import numpy as np

import resident_model as M
from resident_model import DBL_MIN, FACTOR, FLOOR, MODES, Matrix, Run, _dev, _sum, bound, error_dev, scales, x_dev  # noqa: F401

K_CHUNK = 32            # kChunk: iterations per chunk
MUTATIONS = ("swap_rho", "skip_x", "double_x", "drop_row", "stale_alpha")
DOTS = ("pt", "rr", "rz")


class Mutation:
    """One planted error of the loop.  kind:
         "swap_rho"     beta of iteration `at` (>= 2) divides by the r.z of two iterations earlier: the other parity slot, read before it is
                        overwritten
         "skip_x"       the converging iteration's x += alpha p is lost (a run that does not converge is not changed)
         "double_x"     ... is applied twice
         "drop_row"     row `row` (None: the last row) is missing from the sum `dot` ("pt", "rr" or "rz") of iteration `at`
         "stale_alpha"  iteration `at` (default kChunk + 1: the first launch of the second chunk) uses the alpha of the iteration before"""

    def __init__(self, kind, at=None, row=None, dot="rz"):
        assert kind in MUTATIONS and dot in DOTS, (kind, dot)
        self.kind, self.row, self.dot = kind, row, dot
        self.at = at if at is not None else (K_CHUNK + 1 if kind == "stale_alpha" else 5)


def run(A, b, x0, tol, max_iters, mode="ld", mutation=None):
    """The loop on Matrix A for at most max_iters iterations.  Returns a Run holding the state after every iteration (index 0: the set-up)."""
    dt = np.longdouble if mode == "ld" else np.float64
    b = np.asarray(b, dtype=dt)
    x = np.asarray(x0, dtype=dt).copy()
    dinv = dt(1) / A.diag.astype(dt)
    out = Run()
    mut = mutation.kind if mutation is not None else None

    def dot(a, c, name, k):
        t = a * c
        if mut == "drop_row" and mutation.at == k and mutation.dot == name:
            t[A.n - 1 if mutation.row is None else mutation.row] = 0
        return _sum(t, mode)

    def keep(iters, conv, rr):
        out.x.append(x.copy())
        out.rr.append(rr)
        out.error.append(dt(0) if out.bb == 0 else np.sqrt(rr / out.bb))
        out.iterations.append(iters)
        out.converged.append(conv)

    out.bb = bb = dot(b, b, "bb", 0)
    if bb == 0:
        x[:] = 0
        keep(0, True, dt(0))
        return out
    out.threshold = thr = max(dt(tol) * dt(tol) * bb, dt(DBL_MIN))
    r = b - A.row_sums(x, dt)
    rr = dot(r, r, "rr", 0)
    if rr < thr:
        keep(0, True, rr)
        return out
    keep(0, False, rr)
    p = dinv * r
    rho = dot(r, p, "rz", 0)
    rz_of = [rho]               # r.z as iteration k left it (k = 0: the set-up)
    alpha = dt(0)
    iters = 0
    for k in range(1, max_iters + 1):
        t = A.row_sums(p, dt)
        alpha_before, alpha = alpha, rho / dot(p, t, "pt", k)
        if mut == "stale_alpha" and mutation.at == k and k > 1:
            alpha = alpha_before
        r = r - alpha * t
        rr = dot(r, r, "rr", k)
        z = dinv * r
        rz = dot(r, z, "rz", k)
        if rr < thr:
            if mut != "skip_x":
                x = x + alpha * p
            if mut == "double_x":
                x = x + alpha * p
            keep(iters, True, rr)
            break
        x = x + alpha * p
        beta = rz / (rz_of[k - 2] if mut == "swap_rho" and mutation.at == k and k >= 2 else rho)
        p = z + beta * p
        rho = rz
        rz_of.append(rz)
        iters += 1
        keep(iters, False, rr)
    return out


class Model(M.Model):
    """The three runs of one system at tol = 0 for `passes` iterations, the rule (bound_x, bound_error, live_passes: resident_model.Model)
    and the loose tolerances of the exit checks."""

    def __init__(self, A, b, x0, passes):
        self.A, self.b, self.x0 = A, np.asarray(b, np.float64), np.asarray(x0, np.float64)
        self.ld = run(A, b, x0, 0.0, passes, "ld")
        self.f64 = [run(A, b, x0, 0.0, passes, m) for m in ("asc64", "desc")]
        self.passes = min(q.passes for q in [self.ld] + self.f64)
        self.s = [scales(self.ld, self.f64, k) for k in range(self.passes + 1)]

    def exit_tolerance(self, iteration, margin=1e-6):
        """(tol, iterations, iteration) for a solve that converges in iteration `iteration` (1-based; `iterations` = iteration - 1 then), or
        None where no tolerance does that clearly: the threshold tol^2 b.b lies at the geometric mean of r.r of that iteration (below) and
        the smallest earlier r.r (above), `margin` away from both, relatively, in all three runs.  (The summation orders move r.r by about
        1e-13 of itself: the margin is ample, and the resident model's lo < 0.25 hi is not needed.)"""
        m = iteration - 1
        if not 0 <= m < self.live_passes():
            return None
        rr = [float(v) for v in self.ld.rr]
        lo, hi = rr[m + 1], min(rr[:m + 1])
        if not lo < hi:
            return None
        tol = math.sqrt(math.sqrt(lo * hi) / float(self.ld.bb))
        return (tol, m, m + 1) if self.exits_are_clear(tol, m, margin) else None

    def exit_tolerances(self, iterations=(4, 3), margin=1e-6):
        """[(tol, iterations, iteration)]: the admissible ones among the converging iterations asked for"""
        return [e for e in (self.exit_tolerance(i, margin) for i in iterations) if e is not None]
