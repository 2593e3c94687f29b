"""NumPy restatement of avs_get_strain_rates / avs_get_shear_rate_field (include/avs.h; kernels: csrc/avs_strain.hip).

Three definitions, each in the operation order the header states, so that fp64 results can be compared bit for bit:
  stencil_rates   the rate of every stencil of an SoA record set (edge stresses, centre lists)
  cell_shear      the shear rate of every centre id from the edge index pyramid, the edge rates and the centre rates
  paint           the shear-rate field on the simulation grid from the label and centre index pyramids
and summary(): the counters, dissipations (math.fsum: the exact sum, rounded once) and maxima.

Lattices are numpy arrays indexed [k][j][i] (x fastest), as the oracle and the device pre-pass hand them out."""
from __future__ import annotations

import math

import numpy as np

ACTIVE = 1
UNASSIGNED, OUTSIDE = -1, -3
OWN, CHILD, GRANDCHILD, SKIPPED = range(4)


def stencil_rates(st, u):
    """acc = 0; acc = acc + coef[k] * u[idx[k]] for k < cnt in stored order; acc = acc + bval[k] for k < bcnt.  Slots at or behind
    cnt / bcnt are never read."""
    cnt, idx, coef, bcnt, bval = st["cnt"], st["idx"], st["coef"], st["bcnt"], st["bval"]
    acc = np.zeros(len(cnt), np.float64)
    for k in range(int(cnt.max()) if len(cnt) else 0):
        m = cnt > k
        acc[m] = acc[m] + coef[k][m] * u[idx[k][m]]
    for k in range(int(bcnt.max()) if len(bcnt) else 0):
        m = bcnt > k
        acc[m] = acc[m] + bval[k][m]
    return acc


def center_table(cidx, n_center):
    """(n_center, 4) rows (level, i, j, k) of every centre id, from the centre index pyramid alone"""
    tab = np.full((n_center, 4), -1, np.int64)
    for l, lat in enumerate(cidx):
        k, j, i = np.nonzero(lat >= 0)
        ids = lat[k, j, i]
        tab[ids] = np.stack([np.full(len(ids), l), i, j, k], axis=1)
    assert (tab[:, 0] >= 0).all(), "a centre id does not occur"
    return tab


def _lookup(lat, e):
    """index of the edges e (N, 3: ijk) in one edge lattice; outside the lattice: UNASSIGNED"""
    nz, ny, nx = lat.shape
    ok = (e >= 0).all(axis=1) & (e[:, 0] < nx) & (e[:, 1] < ny) & (e[:, 2] < nz)
    v = np.full(len(e), UNASSIGNED, np.int64)
    v[ok] = lat[e[ok, 2], e[ok, 1], e[ok, 0]]
    return v


def cell_shear(eidx, table, n_edge, edge_rate, center_rate):
    """gamma (n_center,), lookups [OWN, CHILD, GRANDCHILD, SKIPPED], empty_pairs.  table: center_table() rows (level, i, j, k)."""
    n_center = len(table)
    gamma = np.zeros(n_center, np.float64)
    lookups = [0, 0, 0, 0]
    empty_pairs = 0
    m_all = np.zeros((3, n_center), np.float64)
    for l in sorted(set(int(v) for v in table[:, 0])):
        ids = np.nonzero(table[:, 0] == l)[0]
        C = table[ids, 1:4]
        N = len(ids)
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            total = np.zeros(N, np.float64)
            n = np.zeros(N, np.int64)
            for q in range(4):                                   # the b offset fastest
                e = C.copy()
                e[:, b] += q & 1
                e[:, c] += q >> 1
                v = _lookup(eidx[l][a], e)
                own = (v >= 0) & (v < n_edge)
                val = np.zeros(N, np.float64)
                val[own] = edge_rate[v[own]]
                has = own.copy()
                lookups[OWN] += int(own.sum())
                desc = (v == UNASSIGNED) & (l > 0)
                if l > 0 and desc.any():
                    csum = np.zeros(N, np.float64)
                    cn = np.zeros(N, np.int64)
                    for h in range(2):
                        child = 2 * e
                        child[:, a] += h
                        w = _lookup(eidx[l - 1][a], child)
                        good = desc & (w >= 0) & (w < n_edge)
                        csum[good] = csum[good] + edge_rate[w[good]]
                        cn[good] += 1
                        lookups[CHILD] += int(good.sum())
                        neg = desc & (w < 0)
                        if l >= 2 and neg.any():
                            gsum = np.zeros(N, np.float64)
                            gn = np.zeros(N, np.int64)
                            for g in range(2):
                                grand = 2 * child
                                grand[:, a] += g
                                x = _lookup(eidx[l - 2][a], grand)
                                gg = neg & (x >= 0) & (x < n_edge)
                                gsum[gg] = gsum[gg] + edge_rate[x[gg]]
                                gn[gg] += 1
                                lookups[GRANDCHILD] += int(gg.sum())
                            use = neg & (gn > 0)
                            csum[use] = csum[use] + gsum[use] / gn[use].astype(np.float64)
                            cn[use] += 1
                    dh = desc & (cn > 0)
                    val[dh] = csum[dh] / cn[dh].astype(np.float64)
                    has |= dh
                lookups[SKIPPED] += int((~has).sum())
                total[has] = total[has] + val[has]
                n[has] += 1
            some = n > 0
            m = np.zeros(N, np.float64)
            m[some] = total[some] / n[some].astype(np.float64)
            empty_pairs += int((~some).sum())
            m_all[a, ids] = m
    exx, eyy, ezz = center_rate[:n_center], center_rate[n_center:2 * n_center], center_rate[2 * n_center:]
    with np.errstate(invalid="ignore", over="ignore"):
        normal = (exx * exx + eyy * eyy) + ezz * ezz
        shear = (m_all[0] * m_all[0] + m_all[1] * m_all[1]) + m_all[2] * m_all[2]
        gamma = np.sqrt(2.0 * normal + 4.0 * shear)
    return gamma, lookups, empty_pairs


def cell_ids(labels, cidx, field_res):
    """centre id of the ACTIVE cell over every cell of the simulation grid (nz, ny, nx): the lowest level whose cell over it is ACTIVE;
    -1 where there is none or where its centre index is no id"""
    nx, ny, nz = field_res
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    out = np.full((nz, ny, nx), -1, np.int64)
    done = np.zeros((nz, ny, nx), bool)
    for l, lab in enumerate(labels):
        here = lab[z >> l, y >> l, x >> l]
        hit = ~done & (here == ACTIVE)
        cid = cidx[l][z >> l, y >> l, x >> l]
        out[hit & (cid >= 0)] = cid[hit & (cid >= 0)]
        done |= hit
    return out


def paint(labels, cidx, cell, field_res):
    """(float)gamma of the covering cell, 0 elsewhere"""
    ids = cell_ids(labels, cidx, field_res)
    ok = (ids >= 0) & (ids < len(cell))
    out = np.zeros(ids.shape, np.float32)
    with np.errstate(over="ignore"):
        out[ok] = cell[ids[ok]].astype(np.float32)
    return out


def summary(edge, center, n_center, edge_rate, center_rate, gamma, lookups, empty_pairs):
    """dict of the fields of avs_strain_summary; the dissipations are exact sums rounded once (math.fsum), with their numbers of terms"""
    fin_e, fin_c = np.isfinite(edge_rate), np.isfinite(center_rate)
    cell_ok = fin_c[:n_center] & fin_c[n_center:2 * n_center] & fin_c[2 * n_center:]
    exx, eyy, ezz = center_rate[:n_center], center_rate[n_center:2 * n_center], center_rate[2 * n_center:]
    e_terms = edge["weight"][fin_e] * (edge_rate[fin_e] * edge_rate[fin_e])
    c_terms = center["weight"][cell_ok] * ((exx[cell_ok] * exx[cell_ok] + eyy[cell_ok] * eyy[cell_ok]) + ezz[cell_ok] * ezz[cell_ok])
    fin_g = np.isfinite(gamma)
    return dict(n_edge=len(edge_rate), n_center=n_center,
                empty_edges=int((edge["cnt"] == 0).sum()), empty_centers=int((center["cnt"] == 0).sum()),
                boundary_edges=int((edge["bcnt"] > 0).sum()), boundary_centers=int((center["bcnt"] > 0).sum()),
                nonfinite=int((~fin_e).sum() + (~fin_c).sum()), edge_lookups=tuple(lookups), empty_pairs=empty_pairs,
                dissipation_edge=math.fsum(e_terms), dissipation_center=math.fsum(c_terms),
                edge_terms=int(fin_e.sum()), center_terms=int(cell_ok.sum()),
                max_abs_edge_rate=float(np.abs(edge_rate[fin_e]).max()) if fin_e.any() else 0.0,
                max_abs_center_rate=float(np.abs(center_rate[fin_c]).max()) if fin_c.any() else 0.0,
                max_shear_rate=float(gamma[fin_g].max()) if fin_g.any() else 0.0)


def evaluate(labels, eidx, cidx, n_edge, n_center, edge, center, u, field_res=None):
    """everything at once: dict(edge, center, cell, summary, field (None without field_res))"""
    er, cr = stencil_rates(edge, u), stencil_rates(center, u)
    gamma, lookups, empty_pairs = cell_shear(eidx, center_table(cidx, n_center), n_edge, er, cr)
    return dict(edge=er, center=cr, cell=gamma, summary=summary(edge, center, n_center, er, cr, gamma, lookups, empty_pairs),
                field=None if field_res is None else paint(labels, cidx, gamma, field_res))
