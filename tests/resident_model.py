"""Host model of the CU-resident PCG loop (csrc/avs_pcg_resident.inl): the iterates x_k of seam A under max_iterations = k.

The recurrence is the single-reduction (Chronopoulos-Gear) one of OP_SR_INIT / sr_step_sums<double> (csrc/avs_halo.hpp):

    set-up   r = b - A x0 ; u = D^-1 r ; w = A u ; rho = gamma = r.u ; alpha = gamma / (w.u) ; beta = 0
             threshold = max(tol^2 b.b, DBL_MIN) ; b.b == 0: x = 0, done ; r.r < threshold: done, x0 kept
    pass     p = u + beta p ; s = w + beta s ; x += alpha p ; r -= alpha s ; u = D^-1 r ; w = A u
             r.r < threshold: converged, `iterations` stays
             else beta = gamma / rho ; alpha = gamma / (delta - beta gamma / alpha) ; rho = gamma ; iterations += 1

with gamma = r.u, delta = w.u taken after the pass.  Row sums run left to right inside the row, multiply then add (no FMA), D^-1 is a
multiplication with the rounded inverse of the diagonal -- what the kernels do.  Everything else that a GPU loop may do differently is
the ORDER of the additions inside the three dot products; the model therefore runs in three modes:

    "ld"     np.longdouble throughout: the reference
    "asc64"  fp64, dot products ascending in blocks of 64 (block sums left to right, then the blocks left to right)
    "desc"   fp64, dot products from the last entry to the first

The two fp64 runs are two samples of what a summation order does to x_k; their distance from the long-double run is the scale s_k of
the tolerance rule (`scales`, `bound`): a loop under test may deviate by 32 max(s_k, 2^-50) -- the factor because its own fold (shuffle
tree, 16 waves, workgroup slots) is a third order of which two samples only give the scale.  `Mutation` plants the errors a converged
solve cannot see (tests/test_resident_model.py shows that the rule sees each of them by a factor of 100 at least).
"""
from __future__ import annotations

import math

import numpy as np

DBL_MIN = 2.2250738585072014e-308
MODES = ("ld", "asc64", "desc")
FACTOR = 32.0
FLOOR = 2.0 ** -50


class Matrix:
    """CSR with the gather lists of a position-by-position (left to right) row sum over all rows at once"""

    def __init__(self, row_ptr, col, val):
        self.rp = np.asarray(row_ptr, dtype=np.int64)
        self.col = np.asarray(col, dtype=np.int64)
        self.val = np.ascontiguousarray(val, dtype=np.float64)
        self.n = n = len(self.rp) - 1
        lens = np.diff(self.rp)
        order = np.argsort(-lens, kind="stable")             # rows by length, longest first: position j is held by a prefix of them
        maxlen = int(lens.max()) if n else 0
        cnt = np.searchsorted(-lens[order], -np.arange(maxlen), side="left")   # rows longer than j
        self.off = np.zeros(maxlen + 1, dtype=np.int64)
        self.off[1:] = np.cumsum(cnt)
        self.rows = np.concatenate([order[:c] for c in cnt]) if maxlen else np.zeros(0, np.int64)
        pos = np.repeat(np.arange(maxlen, dtype=np.int64), cnt)
        self.k = self.rp[self.rows] + pos
        self.c = self.col[self.k]
        self._v = {}
        r = np.repeat(np.arange(n, dtype=np.int64), lens)
        d = np.nonzero(self.col == r)[0]
        assert len(d) == n and np.array_equal(r[d], np.arange(n)), "every row carries its diagonal once"
        self.diag = self.val[d]

    def values(self, dtype):
        if dtype not in self._v:
            self._v[dtype] = self.val[self.k].astype(dtype)
        return self._v[dtype]

    def row_sums(self, x, dtype=np.float64):
        """s_i = (((0 + v_0 x_c0) + v_1 x_c1) + ...) in the row's stored order, one rounding per multiply and per add"""
        x = np.asarray(x, dtype=dtype)
        v = self.values(dtype)
        s = np.zeros(self.n, dtype=dtype)
        for j in range(len(self.off) - 1):
            a, b = self.off[j], self.off[j + 1]
            rows = self.rows[a:b]
            s[rows] = s[rows] + v[a:b] * x[self.c[a:b]]
        return s

    def one_row_sum(self, i, x, dtype=np.float64):
        s = dtype(0)
        for k in range(self.rp[i], self.rp[i + 1]):
            s = s + dtype(self.val[k]) * x[self.col[k]]
        return s


def _sum(t, mode):
    if mode == "ld":
        return np.cumsum(t)[-1] if len(t) else np.longdouble(0)
    if mode == "desc":
        return np.cumsum(t[::-1])[-1] if len(t) else 0.0
    if mode == "asc64":
        pad = (-len(t)) % 64
        if pad:
            t = np.concatenate([t, np.zeros(pad)])
        return np.cumsum(np.cumsum(t.reshape(-1, 64), axis=1)[:, -1])[-1] if len(t) else 0.0
    raise ValueError(mode)


class Mutation:
    """One planted error of the loop.  kind:
         "drop_row"  row `row` is missing from the dot product `dot` ("ru", "rr" or "wu") of pass `at`
         "stale_u"   the row sum of `row` in pass `at` reads the previous pass's u at its first off-diagonal column
         "skip_x"    a run that ends after an odd number of passes returns x without the last x += alpha p"""

    def __init__(self, kind, at=2, row=0, dot="wu"):
        self.kind, self.at, self.row, self.dot = kind, at, row, dot


class Run:
    """x[k], error[k], iterations[k], converged[k], rr[k] for k = 0 .. passes: the state seam A returns when it stops after k passes
    (k = 0: the set-up).  x[k] etc. stop growing at convergence."""

    def __init__(self):
        self.x, self.error, self.iterations, self.converged, self.rr = [], [], [], [], []
        self.threshold = self.bb = None

    @property
    def passes(self):
        return len(self.x) - 1


def run(A, b, x0, tol, max_iters, mode="ld", mutation=None):
    """The loop on Matrix A for at most max_iters passes.  Returns a Run holding the state after every pass."""
    dt = np.longdouble if mode == "ld" else np.float64
    b = np.asarray(b, dtype=dt)
    x = np.asarray(x0, dtype=dt).copy()
    dinv = dt(1) / A.diag.astype(dt)
    out = Run()

    def dot(a, c, name, k):
        t = a * c
        if mutation is not None and mutation.kind == "drop_row" and mutation.at == k and mutation.dot == name:
            t[mutation.row] = 0
        return _sum(t, mode)

    def keep(k, iters, conv, rr):
        xk = x
        if mutation is not None and mutation.kind == "skip_x" and k % 2 == 1:
            xk = out.x[-1]
        out.x.append(xk.copy())
        out.rr.append(rr)
        out.error.append(dt(0) if out.bb == 0 else np.sqrt(rr / out.bb))
        out.iterations.append(iters)
        out.converged.append(conv)

    out.bb = bb = dot(b, b, "bb", 0)
    if bb == 0:
        x[:] = 0
        keep(0, 0, True, dt(0))
        return out
    out.threshold = thr = max(dt(tol) * dt(tol) * bb, dt(DBL_MIN))
    r = b - A.row_sums(x, dt)
    u = dinv * r
    w = A.row_sums(u, dt)
    gamma, rr, delta = dot(r, u, "ru", 0), dot(r, r, "rr", 0), dot(w, u, "wu", 0)
    if rr < thr:
        keep(0, 0, True, rr)
        return out
    keep(0, 0, False, rr)
    rho, alpha, beta = gamma, gamma / delta, dt(0)
    p = np.zeros(A.n, dtype=dt)
    s = np.zeros(A.n, dtype=dt)
    iters = 0
    for k in range(1, max_iters + 1):
        p = u + beta * p
        s = w + beta * s
        x = x + alpha * p
        r = r - alpha * s
        u_prev = u
        u = dinv * r
        w = A.row_sums(u, dt)
        if mutation is not None and mutation.kind == "stale_u" and mutation.at == k:
            i = mutation.row
            cols = A.col[A.rp[i]:A.rp[i + 1]]
            c = cols[cols != i][0]
            us = u.copy()
            us[c] = u_prev[c]
            w[i] = A.one_row_sum(i, us, dt)
        gamma, rr, delta = dot(r, u, "ru", k), dot(r, r, "rr", k), dot(w, u, "wu", k)
        if rr < thr:
            keep(k, iters, True, rr)
            break
        beta = gamma / rho
        alpha = gamma / (delta - beta * gamma / alpha)
        rho = gamma
        iters += 1
        keep(k, iters, False, rr)
    return out


def _dev(v, ref):
    """|v - ref|_inf / |ref|_inf in long double (0 / 0 = 0)"""
    v, ref = np.asarray(v, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    d = np.max(np.abs(v - ref)) if v.size else np.longdouble(0)
    m = np.max(np.abs(ref)) if ref.size else np.longdouble(0)
    if d == 0:
        return 0.0
    return float(d / m) if m > 0 else math.inf


def x_dev(x, ref_run, k):
    return _dev(x, ref_run.x[k])


def error_dev(err, ref_run, k):
    return _dev(np.array([err]), np.array([ref_run.error[k]]))


def scales(ref_run, runs, k):
    """(s_k of x, s_k of error): the larger deviation of the fp64 runs from the long-double run after k passes"""
    return (max(x_dev(q.x[k], ref_run, k) for q in runs), max(error_dev(q.error[k], ref_run, k) for q in runs))


def bound(s):
    """what a loop under test may deviate by, given the scale s"""
    return FACTOR * max(s, FLOOR)


class Model:
    """The three runs of one system at tol = 0 for `passes` passes (fewer when a run converges to DBL_MIN first), and the rule."""

    def __init__(self, A, b, x0, passes):
        self.A, self.b, self.x0 = A, np.asarray(b, np.float64), np.asarray(x0, np.float64)
        self.ld = run(A, b, x0, 0.0, passes, "ld")
        self.f64 = [run(A, b, x0, 0.0, passes, m) for m in ("asc64", "desc")]
        self.passes = min(q.passes for q in [self.ld] + self.f64)
        self.s = [scales(self.ld, self.f64, k) for k in range(self.passes + 1)]

    def bound_x(self, k):
        return bound(self.s[k][0])

    def bound_error(self, k):
        return bound(self.s[k][1])

    def live_passes(self, floor=1e-13):
        """the last k up to which every run's error stayed above `floor`: the iterates a few-row system has before it has converged
        as far as fp64 goes (past it r.r may underflow DBL_MIN in one summation order and not in another)"""
        k = 0
        while k < self.passes and all(float(q.error[k + 1]) > floor for q in [self.ld] + self.f64):
            k += 1
        return k

    def exit_tolerances(self, margin=1e-6):
        """[(tol, iterations, passes)] for one exit at an odd and one at an even `iterations`: the threshold tol^2 b.b lies between
        r.r of pass `passes` (below, where the loop stops) and every earlier r.r (above), at the geometric mean of the two nearest --
        `margin` away from both, relatively, in all three runs (checked by exits_are_clear)"""
        rr = [float(v) for v in self.ld.rr]
        out = {}
        live = self.live_passes()       # (past it r.r is rounding noise: no exit there)
        for m in [m for m in list(range(3, live)) + [1, 2] if m < live]:      # (a few passes in where there are that many)
            lo, hi = rr[m + 1], min(rr[:m + 1])
            if m % 2 in out or not lo < 0.25 * hi:
                continue
            tol = math.sqrt(math.sqrt(lo * hi) / float(self.ld.bb))
            if self.exits_are_clear(tol, m, margin):
                out[m % 2] = (tol, m, m + 1)
        return [out[q] for q in sorted(out)]

    def exits_are_clear(self, tol, iterations, margin=1e-6):
        for q in [self.ld] + self.f64:
            thr = max(tol * tol * float(q.bb), DBL_MIN)
            rr = [float(v) for v in q.rr]
            if not (rr[iterations + 1] < thr * (1 - margin) and all(v > thr * (1 + margin) for v in rr[:iterations + 1])):
                return False
        return True
