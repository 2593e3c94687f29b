"""avs_check_solution / avs_check_csr_solution restated in NumPy (include/avs.h states the conventions).

Rows: y_i = 0; y_i = y_i + val[k] * x[col[k]] for k = row_ptr[i] .. row_ptr[i + 1] - 1 in stored order, one rounding per operation;
r_i = b_i - y_i.  Formed with the masked left-to-right loop of strain_rate_model.stencil_rates, so y and r are the bits the device forms
(a generated NaN aside: IEEE 754 leaves its sign and payload to the implementation).  Counters and maxima are exact.  A sum is
math.fsum over its per-row terms -- the exact sum, rounded once -- and `abs_terms` gives the sum of their magnitudes, for the worst-case
bound of a sum in any order."""
import math

import numpy as np

SOLUTION, INITIAL_GUESS = 0, 1
COUNTERS = ("evaluated", "n", "nnz", "nonfinite_x", "nonfinite_b", "nonfinite_residual", "rows_summed", "max_residual_row")
MAXIMA = ("max_abs_residual", "max_abs_x", "max_abs_update")
SUMS = ("rhs_norm2", "residual_norm2", "x_dot_ax", "x_dot_b", "update_norm2")


def rules_0_and_1_hold(row_ptr, col, n, nnz):
    """rules 0 and 1 of avs_check_csr: the pointers start at 0, never run backwards and end at nnz; every column lies in [0, n)"""
    rp = np.asarray(row_ptr, np.int64)
    if len(rp) != n + 1 or rp[0] != 0 or rp[n] != nnz or (rp < 0).any() or (rp > nnz).any() or (np.diff(rp) < 0).any():
        return False
    c = np.asarray(col[:nnz], np.int64)
    return not ((c < 0) | (c >= n)).any()


def row_products(row_ptr, col, val, x):
    """y, by the masked left-to-right loop: trip k adds entry k of every row that has one"""
    rp = np.asarray(row_ptr, np.int64)
    n = len(rp) - 1
    length = np.diff(rp)
    y = np.zeros(n, np.float64)
    with np.errstate(all="ignore"):
        for k in range(int(length.max()) if n else 0):
            m = length > k
            e = rp[:-1][m] + k
            y[m] = y[m] + val[e] * x[col[e]]
    return y


def relative_residual(residual_norm2, rhs_norm2):
    if rhs_norm2 == 0.0:
        return 0.0 if residual_norm2 == 0.0 else math.inf
    return math.sqrt(residual_norm2 / rhs_norm2)


def evaluate(row_ptr, col, val, b, x, x0=None, which=SOLUTION, seam_a=True):
    """-> dict: every field of avs_solution_check but the claim, `residual` and `y` (None when not evaluated), and per sum S `S_abs` = the
    sum of the magnitudes of its terms.  seam_a: rules 0 and 1 of avs_check_csr decide `evaluated`."""
    n, nnz = len(row_ptr) - 1, len(col)
    out = {f: 0 for f in COUNTERS}
    out.update({f: 0.0 for f in MAXIMA + SUMS + ("relative_residual",)})
    out.update({f + "_abs": 0.0 for f in SUMS})
    out.update(which=which, n=n, nnz=nnz, evaluated=1, residual=None, y=None)
    if seam_a and not rules_0_and_1_hold(row_ptr, col, n, nnz):
        out["evaluated"] = 0
        return out
    b, x = np.asarray(b, np.float64), np.asarray(x, np.float64)
    y = row_products(row_ptr, np.asarray(col), np.asarray(val, np.float64), x)
    with np.errstate(all="ignore"):
        r = b - y
        fx, fb, fr = np.isfinite(x), np.isfinite(b), np.isfinite(r)
        summed = fx & fb & fr
        terms = {"rhs_norm2": b * b, "residual_norm2": r * r, "x_dot_ax": x * y, "x_dot_b": x * b}
        masks = dict.fromkeys(terms, summed)
        if x0 is not None:
            x0 = np.asarray(x0, np.float64)
            d = x - x0
            terms["update_norm2"] = d * d
            masks["update_norm2"] = summed & np.isfinite(x0)
            if masks["update_norm2"].any():
                out["max_abs_update"] = float(np.abs(d[masks["update_norm2"]]).max())
    out.update(residual=r, y=y, nonfinite_x=int((~fx).sum()), nonfinite_b=int((~fb).sum()), nonfinite_residual=int((~fr).sum()),
               rows_summed=int(summed.sum()), max_residual_row=-1)
    for name, t in terms.items():
        picked = t[masks[name]]
        out[name] = math.fsum(picked) if np.isfinite(picked).all() else float(np.sum(picked))
        out[name + "_abs"] = math.fsum(np.abs(picked)) if np.isfinite(picked).all() else math.inf
    if summed.any():
        a = np.where(summed, np.abs(r), -1.0)
        out["max_abs_residual"] = float(a.max())
        out["max_residual_row"] = int(np.argmax(a))          # (the first, hence the smallest, row that attains it)
        out["max_abs_x"] = float(np.abs(x[summed]).max())
    out["relative_residual"] = relative_residual(out["residual_norm2"], out["rhs_norm2"])
    return out


def evaluate_entry_by_entry(row_ptr, col, val, b, x, x0=None):
    """the same definitions in plain Python floats, one entry at a time (no masks, no vector operations): what pins `evaluate`"""
    n = len(row_ptr) - 1
    res, ys = [], []
    cnt = dict(nonfinite_x=0, nonfinite_b=0, nonfinite_residual=0, rows_summed=0)
    terms = {s: [] for s in SUMS}
    best, best_row, max_x, max_update = -1.0, -1, 0.0, 0.0
    for i in range(n):
        y = 0.0
        for k in range(int(row_ptr[i]), int(row_ptr[i + 1])):
            y = y + float(val[k]) * float(x[int(col[k])])
        r = float(b[i]) - y
        ys.append(y)
        res.append(r)
        xi, bi = float(x[i]), float(b[i])
        cnt["nonfinite_x"] += not math.isfinite(xi)
        cnt["nonfinite_b"] += not math.isfinite(bi)
        cnt["nonfinite_residual"] += not math.isfinite(r)
        if not (math.isfinite(xi) and math.isfinite(bi) and math.isfinite(r)):
            continue
        cnt["rows_summed"] += 1
        terms["rhs_norm2"].append(bi * bi)
        terms["residual_norm2"].append(r * r)
        terms["x_dot_ax"].append(xi * y)
        terms["x_dot_b"].append(xi * bi)
        max_x = max(max_x, abs(xi))
        if abs(r) > best:
            best, best_row = abs(r), i
        if x0 is not None and math.isfinite(float(x0[i])):
            d = xi - float(x0[i])
            terms["update_norm2"].append(d * d)
            max_update = max(max_update, abs(d))
    out = {s: math.fsum(t) for s, t in terms.items()}
    out.update(cnt)
    out.update(residual=np.array(res, np.float64), y=np.array(ys, np.float64), max_abs_residual=max(best, 0.0), max_residual_row=best_row,
               max_abs_x=max_x, max_abs_update=max_update, relative_residual=relative_residual(out["residual_norm2"], out["rhs_norm2"]))
    return out


def same_floats(a, b):
    """two float64 arrays hold the same bits, a NaN standing for any NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all()) and a[~na].tobytes() == b[~nb].tobytes()
