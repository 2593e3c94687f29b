"""A plain model of the partition plan (csrc/avs_partition.cpp documents it, csrc/avs_dist_plan.hip builds it on the device), written from
the definitions in numpy and plain Python.  Nothing here follows the kernels: no flags, scans or scatters.

The plan of rank r for a CSR matrix over n ids and an owner per id:
  own_global     the ids r owns, ascending
  halo_global    the ids other ranks own that r's rows read, grouped by owner (ascending rank), ascending inside a group
  send_idx       per peer q, ascending: the local indices of r's ids that rows of q read
  peers          every q != r that r sends to or receives from, ascending, with its send and receive counts
  local rows     r's rows in local order, columns relabelled [owned | halo], in-row order and values unchanged
  tile lists     tiles of T local rows: `bnd` when a row of the tile reads a halo column, `int` otherwise

The tail of the distributed assembly (TAIL) builds the same plan from the rank's own rows alone: the pattern is symmetric, so "q reads my
id i" is "my row i reads an id of q".  With a split the local row order is [rows that read no other rank | rows that do], each part in
ascending id order; own_global, send_idx and local_ref follow that order.  A `dom` list restricts and ORDERS the halo: inside a group the
ids come in the order `dom` lists them (the window's brick-major order in the product).
"""
import numpy as np

OUTSIDE = 0xFF   # owner byte of an id outside the rank's window (TAIL)


class OutsideWindow(Exception):
    """a row of the rank reads a column whose owner is OUTSIDE: the device core refuses with AVS_EINTERNAL"""


def plane_count(levels, extent):
    granule = 1 << (levels - 1)
    return -(-extent // granule)


def planes_of(dof, perm, levels, cut_axis, extent):
    """plane of every row: min(coord << level, extent - 1) >> (levels - 1) of the dof record behind it"""
    rec = np.asarray(dof, np.int64).reshape(-1, 4)
    if perm is not None:
        rec = rec[np.asarray(perm, np.int64)]
    level = rec[:, 0] & 0xFF
    pos = np.minimum(rec[:, 1 + cut_axis] << level, extent - 1)
    return pos >> (levels - 1)


def plane_weights(row_ptr, plane, nplanes):
    """non-zeros + 2 of every row, summed per plane"""
    w = np.zeros(nplanes, np.int64)
    np.add.at(w, plane, np.diff(np.asarray(row_ptr, np.int64)) + 2)
    return w


def plane_owners(weights, world):
    """the greedy cut rule: ranks take contiguous runs of planes; the next rank starts once the running weight has reached the current
    rank's share of the total (and is not zero), or when only as many planes are left as ranks that have none yet"""
    total = int(sum(int(w) for w in weights))
    owners, acc, r = [], 0, 0
    for p, w in enumerate(weights):
        share_reached = acc > 0 and acc >= (total * (r + 1)) // world
        planes_scarce = (len(weights) - p) < (world - r)
        if r < world - 1 and (share_reached or planes_scarce):
            r += 1
        owners.append(r)
        acc += int(w)
    return np.array(owners, np.int32)


def owners(row_ptr, dof, perm, levels, cut_axis, extent, world):
    """(weights, plane_owner, owner per row)"""
    plane = planes_of(dof, perm, levels, cut_axis, extent)
    w = plane_weights(row_ptr, plane, plane_count(levels, extent))
    po = plane_owners(w, world)
    return w, po, po[plane].astype(np.int32)


def _rows(row_ptr, col, ids):
    return [np.asarray(col[row_ptr[i]:row_ptr[i + 1]], np.int64) for i in ids]


def _finish(row_ptr, col, val, own, halo, sends, recv_counts, rank, world, T):
    """the parts both variants share: labels, peers, local rows, tile lists"""
    n = len(row_ptr) - 1
    n_own = len(own)
    label = np.full(n, -1, np.int64)
    label[own] = np.arange(n_own)
    label[halo] = n_own + np.arange(len(halo))
    peers = [q for q in range(world) if q != rank and (len(sends[q]) or recv_counts[q])]
    rows = _rows(row_ptr, col, own)
    row_ptr_local = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col_local = label[np.concatenate(rows)] if rows and row_ptr_local[-1] else np.zeros(0, np.int64)
    vals = [np.asarray(val[row_ptr[i]:row_ptr[i + 1]], np.float64) for i in own]
    val_local = np.concatenate(vals) if vals else np.zeros(0)
    tiles_int, tiles_bnd = [], []
    for t in range(-(-n_own // T)):
        seg = col_local[row_ptr_local[t * T]:row_ptr_local[min((t + 1) * T, n_own)]]
        (tiles_bnd if (seg >= n_own).any() else tiles_int).append(t)
    i32 = lambda a: np.asarray(a, np.int32).reshape(-1)
    return dict(own_global=i32(own), halo_global=i32(halo), row_ptr_local=row_ptr_local, col_local=i32(col_local),
                val_local=np.asarray(val_local, np.float64), send_idx=i32(np.concatenate([sends[q] for q in peers]) if peers else []),
                peers=i32(peers), send_counts=i32([len(sends[q]) for q in peers]), recv_counts=i32([recv_counts[q] for q in peers]),
                tiles_int=i32(tiles_int), tiles_bnd=i32(tiles_bnd))


def plan(row_ptr, col, val, owner, rank, world, T):
    """the plan of `rank` from the whole matrix (any pattern)"""
    row_ptr, col, owner = np.asarray(row_ptr, np.int64), np.asarray(col, np.int64), np.asarray(owner, np.int64)
    n = len(row_ptr) - 1
    own = np.flatnonzero(owner == rank)
    row_of = np.repeat(np.arange(n), np.diff(row_ptr))
    read_by_me = col[owner[row_of] == rank]
    halo_ids = np.unique(read_by_me[owner[read_by_me] != rank])
    halo = halo_ids[np.argsort(owner[halo_ids], kind="stable")]
    recv_counts = [int((owner[halo] == q).sum()) for q in range(world)]
    sends = {}
    for q in range(world):
        read_by_q = col[owner[row_of] == q] if q != rank else np.zeros(0, np.int64)
        mine = np.unique(read_by_q[owner[read_by_q] == rank])
        sends[q] = np.searchsorted(own, mine)          # own is ascending: the local index of an owned id
    return _finish(row_ptr, col, val, own, halo, sends, recv_counts, rank, world, T)


def tail_plan(row_ptr, col, val, owner, rank, world, split, dom, T):
    """the plan of `rank` from its own rows (symmetric pattern); + local_ref, rhs_local (the right-hand side of row i is i) and n_interior"""
    row_ptr, col, owner = np.asarray(row_ptr, np.int64), np.asarray(col, np.int64), np.asarray(owner, np.int64)
    own = np.flatnonzero(owner == rank)
    reads = []                                              # per own row: the other ranks whose ids it reads
    for r in _rows(row_ptr, col, own):
        if (owner[r] == OUTSIDE).any():
            raise OutsideWindow
        reads.append(set(int(q) for q in owner[r] if q != rank))
    n_interior = -1
    if split and len(own):
        interior = [k for k, s in enumerate(reads) if not s]
        boundary = [k for k, s in enumerate(reads) if s]
        order = interior + boundary
        own, reads, n_interior = own[order], [reads[k] for k in order], len(interior)
    rows = _rows(row_ptr, col, own)
    read_by_me = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    halo_set = set(int(c) for c in read_by_me[owner[read_by_me] != rank])
    candidates = np.arange(len(owner)) if dom is None else np.asarray(dom, np.int64)
    halo = np.array([g for g in candidates if int(g) in halo_set], np.int64)
    halo = halo[np.argsort(owner[halo], kind="stable")]
    recv_counts = [int((owner[halo] == q).sum()) for q in range(world)]
    sends = {q: np.array([k for k, s in enumerate(reads) if q in s], np.int64) for q in range(world)}
    p = _finish(row_ptr, col, val, own, halo, sends, recv_counts, rank, world, T)
    p["local_ref"] = np.concatenate([p["own_global"], p["halo_global"]]).astype(np.int32)
    p["rhs_local"] = p["own_global"].astype(np.float64)
    p["n_interior"] = n_interior
    p["unnumbered_halo"] = sorted(halo_set - set(int(g) for g in halo))   # halo columns `dom` does not list: the case is ill-posed
    return p


def spmv(row_ptr, col, val, x):
    """y = A x, one row at a time, products added left to right in fp64 (the order every kernel of the project keeps within a row)"""
    y = np.zeros(len(row_ptr) - 1)
    for i in range(len(y)):
        acc = 0.0
        for k in range(row_ptr[i], row_ptr[i + 1]):
            acc = acc + float(val[k]) * float(x[col[k]])
        y[i] = acc
    return y
