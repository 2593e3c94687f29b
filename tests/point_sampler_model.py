"""NumPy fp64 restatement of the octree velocity interpolant at arbitrary positions (interpSPGrid, HDK_OctreeVectorFieldInterpolator
.cpp:660-845), written from the algorithm and vectorised over the points -- the reference of avs_sample_velocity.

Inputs are what the interpolator holds after its node passes:
  labels[l]      int8  (nz, ny, nx) >> l         cell labels (1 = ACTIVE)
  vidx[l][a]     int32 face lattice a of level l  velocity index pyramid (>= 0 DOF, -1 UNASSIGNED, -2 SOLIDBOUNDARY, -3 OUTSIDE)
  vel[l][a]      fp32  face lattice a of level l  octree face velocities (face_velocities: rebuilt from a solution vector + dof table)
  nval[l][a]     fp32  (nz+1, ny+1, nx+1) >> l    node values
A position q is given in level-0 cells (positions_to_q: q = (p - origin) / dx in fp64).  Every index position is q scaled by a power of
two minus the lattice's half-cell offset.  Lattice reads next to the domain border are clamped, as in the library and the oracle.
"""
import numpy as np

ACTIVE, UNASSIGNED = 1, -1
OUTSIDE, TRILINEAR, NODE_BIG_FACE, NODE_CHILD_FACE = 0, 1, 2, 3
BRANCH_NAMES = {OUTSIDE: "outside", TRILINEAR: "trilinear", NODE_BIG_FACE: "node-based on the big face",
                NODE_CHILD_FACE: "node-based projected onto a child face"}


def positions_to_q(points, dx, origin=None):
    o = np.zeros(3) if origin is None else np.asarray(origin, np.float64)
    return (np.asarray(points).astype(np.float64) - o[None, :]) / np.float64(dx)


def face_velocities(x, dof_table, vidx):
    """vel[l][a]: zero fields with float32(x[id]) at the face of every velocity DOF (setOctreeVelocity, cpp:2779-2813)."""
    vel = [[np.zeros(vidx[l][a].shape, np.float32) for a in range(3)] for l in range(len(vidx))]
    t = np.asarray(dof_table)
    lev, ax = t[:, 0] & 0xff, t[:, 0] >> 8
    xf = np.asarray(x, np.float64).astype(np.float32)
    for l in range(len(vidx)):
        for a in range(3):
            m = (lev == l) & (ax == a)
            vel[l][a][t[m, 3], t[m, 2], t[m, 1]] = xf[m]
    return vel


def _at(arr, p):
    """arr[(z, y, x)] at integer positions p (M, 3) in x, y, z order, clamped to the lattice"""
    r = arr.shape
    i = np.clip(p[:, 0], 0, r[2] - 1)
    j = np.clip(p[:, 1], 0, r[1] - 1)
    k = np.clip(p[:, 2], 0, r[0] - 1)
    return arr[k, j, i]


def _unit(axis):
    e = np.zeros(3, np.int64)
    e[axis] = 1
    return e


def evaluate(q, labels, vidx, vel, nval):
    """Returns (v, branch, inside): v (N, 3) fp64 -- all three components per point; branch (N, 3) -- the branch taken per component
    (OUTSIDE / TRILINEAR / NODE_BIG_FACE / NODE_CHILD_FACE: the last when either of the two faces of the cell was replaced by a child
    face); inside (N,) uint8 -- 1 when an ACTIVE cell contains the point."""
    q = np.asarray(q, np.float64)
    N, L = q.shape[0], len(labels)
    n = np.array(labels[0].shape[::-1], np.int64)
    with np.errstate(invalid="ignore"):
        inbox = np.all((q >= 0.0) & (q <= n[None, :].astype(np.float64)), axis=1)   # (False for a NaN)
    c0 = np.zeros((N, 3), np.int64)
    c0[inbox] = np.floor(q[inbox]).astype(np.int64)
    found = np.full(N, -1, np.int64)
    for l in reversed(range(L)):                     # the lowest ACTIVE level over the level-0 cell
        found = np.where(_at(labels[l], c0 >> l) == ACTIVE, l, found)
    found[~inbox] = -1
    v = np.zeros((N, 3), np.float64)
    branch = np.zeros((N, 3), np.int64)
    for l in range(L):
        sel = np.nonzero(found == l)[0]
        if sel.size == 0:
            continue
        for axis in range(3):
            v[sel, axis], branch[sel, axis] = _at_level(q[sel], c0[sel] >> l, l, axis, vidx, vel, nval)
    return v, branch, (found >= 0).astype(np.uint8)


def _at_level(q, cell, l, axis, vidx, vel, nval):
    M = q.shape[0]
    s = 2.0 ** -l
    off = np.full(3, 0.5)
    off[axis] = 0.0
    ifp = q * s - off[None, :]                       # index position on the face lattice of level l
    face = np.floor(ifp).astype(np.int64)
    corners = [np.array([fi & 1, (fi >> 1) & 1, (fi >> 2) & 1], np.int64) for fi in range(8)]
    transition = np.zeros(M, bool)
    fv = []
    for d in corners:
        transition |= _at(vidx[l][axis], face + d) == UNASSIGNED
        fv.append(_at(vel[l][axis], face + d).astype(np.float64))
    out = np.zeros(M, np.float64)
    branch = np.full(M, TRILINEAR, np.int64)
    # trilinear over the eight faces around the sample
    iw = np.clip(ifp - face, 0.0, 1.0)
    tri = np.zeros(M, np.float64)
    for d, f in zip(corners, fv):
        wt = np.ones(M, np.float64)
        for a in range(3):
            wt = wt * (iw[:, a] if d[a] else 1.0 - iw[:, a])
        tri = tri + wt * f
    out[~transition] = tri[~transition]
    t = np.nonzero(transition)[0]
    if t.size == 0:
        return out, branch
    # node-based interpolation with the bubble correction, on the two faces of the cell
    q, cell = q[t], cell[t]
    a1, a2 = (axis + 1) % 3, (axis + 2) % 3
    ciw = np.clip(q[:, axis] * s - cell[:, axis], 0.0, 1.0)
    fiv = [None, None]
    projected = np.zeros(t.size, bool)
    for direction in range(2):
        af = cell + (_unit(axis)[None, :] if direction else 0)
        fl = np.full(t.size, l, np.int64)
        if l > 0:
            want = _at(vidx[l][axis], af) == UNASSIGNED
            cip1, cip2 = q[:, a1] * (2.0 * s), q[:, a2] * (2.0 * s)
            taken = np.zeros(t.size, bool)
            new_af = af.copy()
            for ci in range(4):                       # the first child face that contains the sample
                cf = 2 * af
                cf[:, a1] += ci & 1
                cf[:, a2] += (ci >> 1) & 1
                hit = want & ~taken & (cf[:, a1] <= cip1) & (cf[:, a2] <= cip2) & (cf[:, a1] + 1 >= cip1) & (cf[:, a2] + 1 >= cip2)
                new_af[hit] = cf[hit]
                taken |= hit
            af = new_af
            fl[taken] = l - 1
            projected |= taken
        res = np.zeros(t.size, np.float64)
        for lev in (l, l - 1):
            g = np.nonzero(fl == lev)[0]
            if g.size == 0:
                continue
            sf = 2.0 ** -lev
            inp1, inp2 = q[g, a1] * sf, q[g, a2] * sf
            fw0, fw1 = inp1 - np.floor(inp1), inp2 - np.floor(inp2)
            fvel = _at(vel[lev][axis], af[g]).astype(np.float64)
            avg = np.zeros(g.size, np.float64)
            acc = np.zeros(g.size, np.float64)
            for ni in range(4):
                nd = af[g].copy()
                nd[:, a1] += ni & 1
                nd[:, a2] += (ni >> 1) & 1
                wt = (fw0 if ni & 1 else 1.0 - fw0) * (fw1 if ni & 2 else 1.0 - fw1)
                nv = _at(nval[lev][axis], nd).astype(np.float64)
                avg = avg + nv
                acc = acc + nv * wt
            mm = np.minimum(np.minimum(1.0 - fw0, 1.0 - fw1), np.minimum(fw0, fw1))
            res[g] = acc + 2.0 * (fvel - 0.25 * avg) * mm
        fiv[direction] = res
    out[t] = (1.0 - ciw) * fiv[0] + ciw * fiv[1]
    branch[t] = np.where(projected, NODE_CHILD_FACE, NODE_BIG_FACE)
    return out, branch
