"""NumPy restatement of avs_apply_viscosity_model, written from the comment in include/avs.h (not from the kernels): the model viscosity
per centre id from the cells' shear rates (strain_rate_model.py), covered / fringe / untouched cells of the simulation grid, relaxation
against the current viscosity, and the summary.  np.power and np.expm1 stand for the device's pow and expm1: a few fp64 ulps apart at most,
which moves the value rounded to float32 by one ulp at most -- exact where the header's value involves neither (g == 0, a clamped value,
the Newtonian limits)."""
import numpy as np

import strain_rate_model as S

CARREAU_YASUDA, HERSCHEL_BULKLEY = 0, 1
PARAMETERS = ("mu_0", "mu_inf", "lambda", "a", "n", "consistency", "tau_y", "regularisation", "mu_min", "mu_max", "relaxation")


def carreau_yasuda(mu_0, mu_inf, lam, a, n, mu_min, mu_max, relaxation=1.0):
    return dict(dict.fromkeys(PARAMETERS, 0.0), kind=CARREAU_YASUDA, mu_0=mu_0, mu_inf=mu_inf, a=a, n=n, mu_min=mu_min, mu_max=mu_max,
                relaxation=relaxation, **{"lambda": lam})


def herschel_bulkley(consistency, n, tau_y, regularisation, mu_min, mu_max, relaxation=1.0):
    return dict(dict.fromkeys(PARAMETERS, 0.0), kind=HERSCHEL_BULKLEY, consistency=consistency, n=n, tau_y=tau_y, regularisation=regularisation,
                mu_min=mu_min, mu_max=mu_max, relaxation=relaxation)


# the models of the GPU tests (tests/test_gpu_viscosity_model.py); tests/test_viscosity_model.py shows on the CPU what they exercise there
CASES = {
    "carreau": carreau_yasuda(100.0, 1.0, 0.5, 2.0, 0.5, 50.0, 95.0),
    "carreau_relaxed": carreau_yasuda(100.0, 1.0, 0.5, 2.0, 0.5, 50.0, 95.0, relaxation=0.625),
    "bingham": herschel_bulkley(20.0, 0.75, 30.0, 4.0, 18.0, 50.0),
    "bingham_relaxed": herschel_bulkley(20.0, 0.75, 30.0, 4.0, 18.0, 50.0, relaxation=0.3),
    "newtonian_carreau": carreau_yasuda(70.0, 3.0, 0.5, 2.0, 1.0, 1.0, 1000.0),
    "newtonian_hb": herschel_bulkley(70.0, 1.0, 0.0, 0.0, 1.0, 1000.0),
}


def per_id(p, g):
    """m(g) per centre id: dict(P float32 (0: the id has no value), raw fp64 m before the clamp, low / high / novalue masks)"""
    g = np.asarray(g, np.float64)
    with np.errstate(all="ignore"):
        if p["kind"] == CARREAU_YASUDA:
            m = p["mu_inf"] + (p["mu_0"] - p["mu_inf"]) * np.power(1.0 + np.power(p["lambda"] * g, p["a"]), (p["n"] - 1.0) / p["a"])
        else:
            m = p["consistency"] * np.power(g, p["n"] - 1.0)
            if p["tau_y"] != 0.0:
                y = np.where(g == 0.0, p["tau_y"] * p["regularisation"],
                             (p["tau_y"] * (-np.expm1(-p["regularisation"] * g))) / np.where(g == 0.0, 1.0, g))
                m = m + y
    novalue = np.isnan(m) | ~np.isfinite(g)
    low, high = ~novalue & (m < p["mu_min"]), ~novalue & (m > p["mu_max"])
    clamped = np.where(low, p["mu_min"], np.where(high, p["mu_max"], m))
    with np.errstate(all="ignore"):
        P = np.where(novalue, 0.0, clamped).astype(np.float32)                    # one rounding, after the clamp
    return dict(P=P, m=m, low=low, high=high, novalue=novalue)


def neighbour_mean(painted):
    """per cell: (float)(S / count) over the covered (> 0) ones of its 27 - 1 neighbours inside the grid, S added in fp64 with z slowest and
    x fastest; and count"""
    nz, ny, nx = painted.shape
    pad = np.pad(painted.astype(np.float64), 1)                                   # outside the grid: not covered
    total, count = np.zeros(painted.shape), np.zeros(painted.shape, np.int64)
    for dz in (0, 1, 2):
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                v = pad[dz:dz + nz, dy:dy + ny, dx:dx + nx]
                hit = v > 0
                total = np.where(hit, total + v, total)
                count += hit
    with np.errstate(all="ignore"):
        mean = (total / np.maximum(count, 1)).astype(np.float32)
    return mean, count


def cells(P, g, ids, old, relaxation):
    """the simulation grid: ids (nz, ny, nx) from strain_rate_model.cell_ids, old (nz, ny, nx) float32 the current viscosity.  dict(field
    = new, M, covered / fringe / untouched masks, summary fields)"""
    has = (ids >= 0) & (ids < len(P))
    painted = np.zeros(ids.shape, np.float32)
    painted[has] = P[ids[has]]
    covered = painted > 0
    mean, count = neighbour_mean(painted)
    fringe, untouched = ~covered & (count > 0), ~covered & (count == 0)
    M = np.where(covered, painted, np.where(fringe, mean, np.float32(0))).astype(np.float32)
    old = np.ascontiguousarray(np.broadcast_to(np.asarray(old, np.float32), ids.shape))
    o64, m64 = old.astype(np.float64), M.astype(np.float64)
    new = M.copy() if relaxation == 1.0 else (o64 + relaxation * (m64 - o64)).astype(np.float32)
    new[untouched] = old[untouched]
    rel = covered & (old > 0)
    change = np.abs(new.astype(np.float64)[rel] - o64[rel]) / o64[rel]
    return dict(field=new, M=M, covered=covered, fringe=fringe, untouched=untouched,
                summary=dict(covered=int(covered.sum()), fringe=int(fringe.sum()), untouched=int(untouched.sum()),
                             min_viscosity=float(M[covered].min()) if covered.any() else 0.0,
                             max_viscosity=float(M[covered].max()) if covered.any() else 0.0,
                             max_shear_rate=float(np.asarray(g)[ids[covered]].max()) if covered.any() else 0.0,
                             max_relative_change=float(change.max()) if change.size else 0.0))


def evaluate(p, g, ids, old):
    """everything: per_id + cells, the summary complete"""
    v = per_id(p, g)
    r = cells(v["P"], g, ids, old, p["relaxation"])
    r["summary"].update(n_center=len(v["P"]), clamped_low=int(v["low"].sum()), clamped_high=int(v["high"].sum()), nonfinite=int(v["novalue"].sum()))
    r.update(per_id=v)
    return r


def replicate_onto(field, lattice_shape):
    """the border replication of avs_set_scalar_field: field (fz, fy, fx) onto the padded lattice (nz, ny, nx)"""
    fz, fy, fx = field.shape
    nz, ny, nx = lattice_shape
    return np.pad(field, ((0, nz - fz), (0, ny - fy), (0, nx - fx)), mode="edge")


def ulps_apart(a, b):
    """distance of two positive finite float32 arrays in units of the last place"""
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))
