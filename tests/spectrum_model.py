"""avs_estimate_spectrum / avs_estimate_csr_spectrum restated in NumPy (include/avs.h states the conventions).

Everything is fp64 with one rounding per operation.  Row products use solution_check_model.row_products (the masked left-to-right loop),
so y, t, w and v are the bits the device forms from the same inputs.  A sum is not defined bit for bit across implementations -- the
device adds one partial sum per 256 rows in an order of its own -- so the model offers three orders: `forward` and `reverse` (one running
sum over the rows, from either end) and `fsum` (the exact sum, rounded once).  What differs between them is what a correct device may
differ by.  The host part (eigenvalues of the Lanczos tridiagonal) is numpy.linalg.eigh."""
import math

import numpy as np

import solution_check_model as SM

JACOBI, MATRIX = 0, 1
RESIDUAL, HASH, VECTOR = 0, 1, 2
MAX_STEPS = 512
BREAKDOWN = 2.0 ** -36
ORDERS = ("forward", "reverse", "fsum")
_M64 = (1 << 64) - 1


def splitmix64(i):
    z = (i + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def hash_vector(n):
    """v_i = (double)(splitmix64(i) >> 11) * 2^-53 - 0.5: exact in every operation"""
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = i + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 - 0.5


def total(terms, order):
    terms = np.asarray(terms, np.float64)
    if len(terms) == 0:
        return 0.0
    if order == "fsum":
        return math.fsum(terms) if np.isfinite(terms).all() else float(np.sum(terms))
    with np.errstate(all="ignore"):
        return float(np.add.accumulate(terms if order == "forward" else terms[::-1])[-1])


def diagonal(row_ptr, col, val):
    """d_i = the LAST entry of row i with col == i -> (d, have)"""
    rp = np.asarray(row_ptr, np.int64)
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    d, have = np.zeros(n), np.zeros(n, bool)
    on = np.asarray(col)[:len(rows)] == rows
    d[rows[on]] = np.asarray(val, np.float64)[:len(rows)][on]       # (ascending k: the last assignment stays)
    have[rows[on]] = True
    return d, have


def scale(row_ptr, col, val, op):
    """-> s, bad_diagonal (rows counted there have s_i = 0)"""
    n = len(row_ptr) - 1
    if op == MATRIX:
        return np.ones(n), 0
    d, have = diagonal(row_ptr, col, val)
    ok = have & (d > 0) & np.isfinite(d)
    s = np.zeros(n)
    s[ok] = 1.0 / np.sqrt(d[ok])
    return s, int((~ok).sum())


def gershgorin(row_ptr, col, val, s):
    """max_i g_i, g_i = g_i + |val[k]| * (s_i * s_col[k]) in stored order; a row sum that is not finite gives +Inf"""
    rp = np.asarray(row_ptr, np.int64)
    n = len(rp) - 1
    length = np.diff(rp)
    g = np.zeros(n)
    with np.errstate(all="ignore"):
        for k in range(int(length.max()) if n else 0):
            m = length > k
            e = rp[:-1][m] + k
            g[m] = g[m] + np.abs(val[e]) * (s[m] * s[col[e]])
    g[~(g < np.inf)] = np.inf
    return float(g.max()) if n else 0.0


def form_t(row_ptr, col, val, s, v, v_before, beta_j, j):
    """t_i = s_i * y_i - beta[j] * v_{j-1,i} with y = A (s o v_j): bit for bit"""
    with np.errstate(all="ignore"):
        t = s * SM.row_products(row_ptr, col, val, s * v)
        return t if j == 0 else t - beta_j * v_before


def start_vector(row_ptr, col, val, s, start, b=None, x0=None, given=None):
    n = len(row_ptr) - 1
    if start == HASH:
        return hash_vector(n)
    if start == VECTOR:
        return np.asarray(given, np.float64).copy()
    with np.errstate(all="ignore"):
        return s * (np.asarray(b, np.float64) - SM.row_products(row_ptr, col, val, np.asarray(x0, np.float64)))


def lanczos(row_ptr, col, val, b=None, x0=None, given=None, op=JACOBI, start=RESIDUAL, steps=8, order="fsum", seam_a=True):
    """the device part -> dict(evaluated, bad_diagonal, scale, gershgorin_max, start_norm, alpha [steps], beta [steps + 1], basis [columns
    formed], steps_taken, breakdown, nonfinite)"""
    n, nnz = len(row_ptr) - 1, len(col)
    out = dict(evaluated=0, bad_diagonal=0, scale=None, gershgorin_max=0.0, start_norm=0.0, alpha=np.zeros(steps), beta=np.zeros(steps + 1),
               basis=[], steps_taken=0, breakdown=0, nonfinite=0, n=n, nnz=nnz)
    if seam_a and not SM.rules_0_and_1_hold(row_ptr, col, n, nnz):
        return out
    col, val = np.asarray(col), np.asarray(val, np.float64)
    if n == 0:
        out["evaluated"] = 1
        return out
    s, bad = scale(row_ptr, col, val, op)
    out.update(scale=s, bad_diagonal=bad)
    if bad:
        return out
    out.update(evaluated=1, gershgorin_max=gershgorin(row_ptr, col, val, s))
    with np.errstate(all="ignore"):
        v = start_vector(row_ptr, col, val, s, start, b, x0, given)
        beta0 = math.sqrt(total(v * v, order)) if not math.isnan(total(v * v, order)) else math.nan
        out["beta"][0] = out["start_norm"] = beta0
        if not math.isfinite(beta0):
            out["nonfinite"] = 1
            return out
        if not beta0 > 0:
            return out
        v = v / beta0
        out["basis"].append(v)
        before = None
        for j in range(min(steps, n)):
            t = form_t(row_ptr, col, val, s, v, before, out["beta"][j], j)
            alpha = total(v * t, order)
            w = t - alpha * v
            sq = total(w * w, order)
            beta = math.sqrt(sq) if sq >= 0 else math.nan
            out["alpha"][j], out["beta"][j + 1], out["steps_taken"] = alpha, beta, j + 1
            if not (math.isfinite(alpha) and math.isfinite(beta)):
                out["nonfinite"] = 1
                break
            if not beta > BREAKDOWN * (abs(alpha) + out["beta"][j]):
                out["breakdown"] = 1
                break
            before, v = v, w / beta
            out["basis"].append(v)
    return out


def tridiagonal(alpha, beta, k):
    """T_k = tridiag(beta[1 .. k - 1]; alpha[0 .. k - 1])"""
    return np.diag(np.asarray(alpha[:k], np.float64)) + np.diag(np.asarray(beta[1:k], np.float64), 1) + np.diag(np.asarray(beta[1:k], np.float64), -1)


def iteration_bound(kappa, tolerance):
    if not (0 < tolerance < 1) or not (kappa >= 1) or not math.isfinite(kappa):
        return -1
    return int(math.ceil(0.5 * math.sqrt(kappa) * math.log(2.0 / tolerance)))


def host_part(alpha, beta, k, tolerance):
    """the host tridiagonal step -> dict(ritz [k], lambda_min, lambda_max, lambda_min_bound, lambda_max_bound, indefinite,
    condition_estimate, iteration_bound)"""
    out = dict(ritz=np.zeros(0), lambda_min=0.0, lambda_max=0.0, lambda_min_bound=0.0, lambda_max_bound=0.0, indefinite=0, condition_estimate=0.0,
               iteration_bound=-1)
    if k == 0:
        return out
    if not (np.isfinite(alpha[:k]).all() and np.isfinite(beta[1:k + 1]).all()):
        out.update(ritz=np.full(k, np.nan), lambda_min=math.nan, lambda_max=math.nan, lambda_min_bound=math.nan, lambda_max_bound=math.nan,
                   condition_estimate=math.nan)
        return out
    theta, z = np.linalg.eigh(tridiagonal(alpha, beta, k))
    out.update(ritz=theta, lambda_min=float(theta[0]), lambda_max=float(theta[-1]), lambda_min_bound=float(beta[k] * abs(z[-1, 0])),
               lambda_max_bound=float(beta[k] * abs(z[-1, -1])), indefinite=int(theta[0] <= 0))
    out["condition_estimate"] = math.inf if out["indefinite"] else out["lambda_max"] / out["lambda_min"]
    out["iteration_bound"] = iteration_bound(out["condition_estimate"], tolerance)
    return out


def estimate(row_ptr, col, val, b=None, x0=None, given=None, op=JACOBI, start=RESIDUAL, steps=8, tolerance=1e-3, order="fsum", seam_a=True):
    """every field of avs_spectrum, the arrays of `lanczos` and `ritz`"""
    out = lanczos(row_ptr, col, val, b, x0, given, op, start, steps, order, seam_a)
    host = host_part(out["alpha"], out["beta"], out["steps_taken"], tolerance) if out["evaluated"] else host_part(None, None, 0, tolerance)
    if not out["evaluated"]:
        host["iteration_bound"] = 0
    out.update(host)
    out.update(op=op, start=start, steps_asked=steps, tolerance=tolerance)
    return out


def dense_operator(row_ptr, col, val, op):
    """S A S as a dense matrix (entries of one place added up)"""
    n = len(row_ptr) - 1
    s, bad = scale(row_ptr, col, val, op)
    assert bad == 0
    a = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(np.asarray(row_ptr, np.int64)))
    np.add.at(a, (rows, np.asarray(col)), np.asarray(val, np.float64))
    return s[:, None] * a * s[None, :]


def lanczos_entry_by_entry(row_ptr, col, val, b, x0, op, steps):
    """the RESIDUAL-start recurrence in plain Python floats, one entry at a time, sums by math.fsum: what pins `lanczos`"""
    n = len(row_ptr) - 1
    s = []
    for i in range(n):
        if op == MATRIX:
            s.append(1.0)
            continue
        d = None
        for k in range(int(row_ptr[i]), int(row_ptr[i + 1])):
            if int(col[k]) == i:
                d = float(val[k])
        assert d is not None and d > 0 and math.isfinite(d)
        s.append(1.0 / math.sqrt(d))
    gersh = 0.0
    for i in range(n):
        g = 0.0
        for k in range(int(row_ptr[i]), int(row_ptr[i + 1])):
            g = g + abs(float(val[k])) * (s[i] * s[int(col[k])])
        gersh = max(gersh, g)

    def product(x):
        ys = []
        for i in range(n):
            y = 0.0
            for k in range(int(row_ptr[i]), int(row_ptr[i + 1])):
                y = y + float(val[k]) * x[int(col[k])]
            ys.append(y)
        return ys

    y = product([float(a) for a in x0])
    v = [s[i] * (float(b[i]) - y[i]) for i in range(n)]
    beta = [math.sqrt(math.fsum(a * a for a in v))]
    alpha, basis, before = [], [], None
    v = [a / beta[0] for a in v]
    basis.append(v)
    for j in range(min(steps, n)):
        y = product([s[i] * v[i] for i in range(n)])
        t = [s[i] * y[i] for i in range(n)]
        if j > 0:
            t = [t[i] - beta[j] * before[i] for i in range(n)]
        a = math.fsum(v[i] * t[i] for i in range(n))
        w = [t[i] - a * v[i] for i in range(n)]
        bt = math.sqrt(math.fsum(c * c for c in w))
        alpha.append(a)
        beta.append(bt)
        if not bt > BREAKDOWN * (abs(a) + beta[j]):
            break
        before, v = v, [c / bt for c in w]
        basis.append(v)
    return dict(scale=np.array(s), gershgorin_max=gersh, alpha=np.array(alpha), beta=np.array(beta), basis=[np.array(c) for c in basis])
