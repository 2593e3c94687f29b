"""The rule of the device builder of the brick-structured SpMV form (csrc/avs_brick_build.hip), restated in numpy: no torch, no device.

model(csr, dof, grid, limits) returns, per tile, what the builder must write into the first 16 words of the tile's descriptor block
(layout: csrc/avs_brick.hip), and the counts the form reports.  The rule, from the device code:

  * bricks -> tiles (k_bk_run_first .. k_bk_tile_finish): the rows of one 8^3 brick are consecutive; a brick of >= min_rows rows is a G tile,
    cut every max_rows rows (the pieces keep the brick's lattice origin); a run of smaller bricks is cut every etile_rows rows, counted from
    the run's first row, into E tiles.  A brick of >= 2048 rows stops the build (form not ready).
  * lattice slot of a face relative to the tile's brick (lattice_slot), extra slots (k_bk_rows pass A): the off-lattice columns that lie in
    the 27 neighbour bricks, over ALL rows of the tile; the smallest x_slots of them get the slots behind the lattice.  More than 512
    candidates do not fit the builder's hash set and which ones get in depends on the order of arrival: the tile is flagged `racy`.
  * a row may be a pattern (k_bk_rows pass B) when it has an own slot, 1 .. pat_len entries, level <= 3, every column has a slot and every
    delta (slot - the row's base on the column's lattice, base_slot) lies in -4096 .. 4095.
  * pattern identity: the word sequence in stored order -- delta, lattice level, value code (the value itself: one dictionary, a code per
    distinct bit pattern); in the value-code variant the words carry no code.
  * patterns kept per tile (k_bk_tile): in order of first use by row, the prefix that stays within pat_max patterns and the word cap
    (lengths padded to quads); the first pattern that does not fit ends the prefix, its rows and those of every later pattern are streamed.
  * fill runs: slot -> column over the entries of kept pattern rows whose column is not a row of the tile -- or is one that has no lattice
    slot of its own (level 4) and is read through an extra slot; natural runs are consecutive slots with consecutive columns, cut every
    run_len slots.
  * block limit: nruns <= max_runs and header_words + 2 nruns + npq + npat <= block_words, else the tile is redone as an E tile ("GE").
  * value-code variant: a G tile with more than tile_vals distinct values over ALL its rows is an E tile from the start ("GE"); ntv counts the
    values of the kept pattern rows; the code stream takes, per wave of 64 rows of the execution order (sorted by length), the quads of the
    wave's longest row x 64.
  * partitioned systems (n_cols > n_rows): a tile whose rows read a column >= n_rows carries the halo flag, and the flagged tiles move, in
    order, to the end of the tile list.
"""
from collections import namedtuple

import numpy as np

LEVEL_LATTICES = 4
XSET = 512            # slots of the builder's hash set of extra-slot candidates (k_bk_rows: xset)
TOO_BIG = 2048        # rows of one brick at which the build stops (k_bk_tile_counts)

Tile = namedtuple("Tile", "kind row0 nrows npat nruns npq nprow nsrows nsw halo ntv csize racy ncand npat_seen pat_words_seen nvals origin mixed_waves nprow_seen nruns_seen")
Model = namedtuple("Model", "ready tiles order headers patterns pattern_rows streamed_rows streamed_words halo_tiles racy")


def lattice_offsets():
    off = [0]
    for l in range(LEVEL_LATTICES):
        off.append(off[-1] + 3 * ((8 >> l) + 2) ** 3)
    return np.array(off, np.int64)      # 0, 3000, 3648, 3840, 3921


LOFF = lattice_offsets()


def geometry(dof, nx, ny, nz):
    """level, axis, i, j, k, brick of every dof record (k_bk_geo: the brick of the face's position, clamped into the grid)"""
    dof = np.asarray(dof, np.int64).reshape(-1, 4)
    level, axis = dof[:, 0] & 0xff, (dof[:, 0] >> 8) & 0xff
    i, j, k = dof[:, 1], dof[:, 2], dof[:, 3]
    px, py, pz = np.minimum(i << level, nx - 1), np.minimum(j << level, ny - 1), np.minimum(k << level, nz - 1)
    nbx, nby = (nx + 7) >> 3, (ny + 7) >> 3
    brick = ((pz >> 3) * nby + (py >> 3)) * nbx + (px >> 3)
    return level, axis, i, j, k, brick


def lattice_slot(level, axis, i, j, k, ob):
    """slot of faces on the lattices of the brick ob = (obx, oby, obz); -1 off the lattices"""
    lv = np.minimum(level, 3)
    w = 8 >> lv
    S = w + 2
    rx, ry, rz = i - w * ob[0] + 1, j - w * ob[1] + 1, k - w * ob[2] + 1
    on = (level <= 3) & (rx >= 0) & (rx < S) & (ry >= 0) & (ry < S) & (rz >= 0) & (rz < S)
    slot = LOFF[lv] + ((rz * S + ry) * S + rx) * 3 + axis
    return np.where(on, slot, -1)


def base_slot(lr, cx, cy, cz, lc):
    """base of a row (level lr, local cell c) on the lattice of level lc"""
    up, dn = np.maximum(lc - lr, 0), np.maximum(lr - lc, 0)
    S = (8 >> lc) + 2
    bx, by, bz = ((cx >> up) << dn) + 1, ((cy >> up) << dn) + 1, ((cz >> up) << dn) + 1
    return LOFF[lc] + ((bz * S + by) * S + bx) * 3


def tile_table(brick, L):
    """[(row0, nrows, is_g, brick id)] from the bricks of the rows, or None when a brick is too big for the form"""
    n = len(brick)
    starts = np.flatnonzero(np.r_[True, brick[1:] != brick[:-1]])
    ends = np.r_[starts[1:], n]
    if np.any(ends - starts >= TOO_BIG):
        return None
    tiles = []
    b = 0
    while b < len(starts):
        rows = ends[b] - starts[b]
        if rows >= L.min_rows:
            for r0 in range(starts[b], ends[b], L.max_rows):
                tiles.append((int(r0), 1, int(brick[starts[b]])))
            b += 1
            continue
        e = b
        while e < len(starts) and ends[e] - starts[e] < L.min_rows:
            e += 1
        for r0 in range(starts[b], ends[e - 1], L.etile_rows):   # (the brick a cut falls into: its id is not used for an E tile)
            tiles.append((int(r0), 0, int(brick[r0])))
        b = e
    out = []
    for t, (r0, g, bid) in enumerate(tiles):
        r1 = tiles[t + 1][0] if t + 1 < len(tiles) else n
        out.append((r0, r1 - r0, g, bid))
    return out


def fill_runs(smap_slots, smap_cols, run_len):
    """number of fill runs: natural runs (consecutive slots, consecutive columns) cut every run_len slots"""
    if len(smap_slots) == 0:
        return 0
    order = np.argsort(smap_slots)
    s, c = smap_slots[order], smap_cols[order]
    start = np.r_[True, (s[1:] != s[:-1] + 1) | (c[1:] != c[:-1] + 1)]
    first = np.maximum.accumulate(np.where(start, np.arange(len(s)), 0))
    return int(np.count_nonzero((np.arange(len(s)) - first) % run_len == 0))


def model(row_ptr, col, val, dof, n_rows, nx, ny, nz, L, vc=False):
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    vbits = np.ascontiguousarray(val, np.float64).view(np.int64)
    n_cols = len(np.asarray(dof).reshape(-1, 4))
    level, axis, gi, gj, gk, brick = geometry(dof, nx, ny, nz)
    nbx, nby = (nx + 7) >> 3, (ny + 7) >> 3
    bx, by, bz = brick % nbx, (brick // nbx) % nby, brick // (nbx * nby)
    table = tile_table(brick[:n_rows], L)
    if table is None:
        return Model(False, [], [], None, 0, 0, 0, 0, 0, False)
    lens = np.diff(row_ptr)
    cap = L.pat_words_vc if vc else L.pat_words
    slots_pad = L.emode_words
    tiles, global_patterns = [], set()
    for (row0, nrows, is_g, bid) in table:
        e0, e1 = row_ptr[row0], row_ptr[row0 + nrows]
        c = col[e0:e1]
        erow = np.repeat(np.arange(nrows), lens[row0:row0 + nrows])
        halo = bool(n_cols > n_rows and np.any(c >= n_rows))
        tl = lens[row0:row0 + nrows]
        nvals = len(np.unique(vbits[e0:e1]))
        ob = (bid % nbx, (bid // nbx) % nby, bid // (nbx * nby))
        stream_all = dict(npat=0, nruns=0, npq=0, nprow=0, nsrows=int(nrows), nsw=int(e1 - e0), ntv=0, csize=0)
        if not is_g:
            tiles.append(Tile("E", row0, nrows, halo=halo, racy=False, ncand=0, npat_seen=0, pat_words_seen=0, nvals=nvals, origin=ob, mixed_waves=0,
                              nprow_seen=0, nruns_seen=0, **stream_all))
            continue
        # ---- k_bk_rows: slots, extra slots, eligibility, words
        slot = lattice_slot(level[c], axis[c], gi[c], gj[c], gk[c], ob)
        near = (np.abs(bx[c] - ob[0]) <= 1) & (np.abs(by[c] - ob[1]) <= 1) & (np.abs(bz[c] - ob[2]) <= 1)
        cand = np.unique(c[(slot < 0) & near])
        racy = len(cand) > XSET
        extras = cand[:L.x_slots]
        pos = np.searchsorted(extras, c)
        is_x = np.zeros(len(c), bool)
        if len(extras):
            is_x = (slot < 0) & near & (pos < len(extras)) & (extras[np.minimum(pos, len(extras) - 1)] == c)
        slot = np.where(is_x, slots_pad + pos, slot)
        tag = np.where(is_x, 0, np.searchsorted(LOFF[1:LEVEL_LATTICES], np.maximum(slot, 0), side="right"))
        rows = np.arange(row0, row0 + nrows)
        own = lattice_slot(level[rows], axis[rows], gi[rows], gj[rows], gk[rows], ob)
        lr = np.minimum(level[rows], 3)
        w = 8 >> lr
        cx, cy, cz = gi[rows] - w * ob[0], gj[rows] - w * ob[1], gk[rows] - w * ob[2]
        ok = (own >= 0) & (tl >= 1) & (tl <= L.pat_len) & (level[rows] <= 3)
        for cc in (cx, cy, cz):
            ok &= (cc >= -1) & (cc < 15)
        delta = slot - base_slot(lr[erow], cx[erow], cy[erow], cz[erow], tag)
        bad = (slot < 0) | (delta < -4096) | (delta > 4095)
        ok &= np.bincount(erow, weights=bad, minlength=nrows) == 0
        word = np.stack([delta, tag, np.zeros_like(delta) if vc else vbits[e0:e1]], axis=1)
        rel = row_ptr[row0:row0 + nrows + 1] - e0
        keys = [word[rel[r]:rel[r + 1]].tobytes() if ok[r] else None for r in range(nrows)]
        global_patterns.update(k for k in keys if k is not None)
        force_e = vc and nvals > L.tile_vals
        # ---- k_bk_tile: the patterns kept, in order of first use
        seen, kept, acc, open_ = {}, {}, 0, True
        for r in range(nrows):
            k = keys[r]
            if k is None or k in seen:
                continue
            len4 = (int(tl[r]) + 3) & ~3
            seen[k] = len4
            if open_ and len(kept) < L.pat_max and acc + len4 <= cap:
                kept[k] = len(kept)
                acc += len4
            else:
                open_ = False
        prow = np.array([keys[r] in kept for r in range(nrows)], bool) if kept else np.zeros(nrows, bool)
        info = dict(racy=racy, ncand=len(cand), npat_seen=len(seen), pat_words_seen=sum(seen.values()), nvals=nvals, origin=ob, mixed_waves=0,
                    nprow_seen=int(prow.sum()), nruns_seen=0)
        if force_e:
            tiles.append(Tile("GE", row0, nrows, halo=halo, **info, **stream_all))
            continue
        pe = prow[erow] & ((c < row0) | (c >= row0 + nrows) | (slot >= slots_pad))   # (an own row without a lattice slot, read through an extra one)
        us, ui = np.unique(slot[pe], return_index=True)
        nruns = fill_runs(us, c[pe][ui], L.run_len)
        info["nruns_seen"] = nruns
        npat, npq = len(kept), acc >> 2
        nprow = int(prow.sum())
        if nruns > L.max_runs or L.header_words + 2 * nruns + npq + npat > L.block_words:
            tiles.append(Tile("GE", row0, nrows, halo=halo, **info, **stream_all))
            continue
        nprow = int(prow.sum())
        # execution order: pattern rows sorted by (length, kept pattern, row); a wave is 64 consecutive rows of it
        pr = np.flatnonzero(prow)
        li = np.array([kept[keys[r]] for r in pr], np.int64)
        xo = np.lexsort((pr, li, tl[pr]))
        simple = np.bincount(erow, weights=(tag != 0), minlength=nrows)[pr][xo] == 0
        mixed = sum(1 for lo in range(0, nprow, 64) if 0 < simple[lo:lo + 64].sum() < len(simple[lo:lo + 64]))
        info["mixed_waves"] = mixed
        ntv = csize = 0
        if vc and npat > 0:
            ntv = len(np.unique(vbits[e0:e1][prow[erow]]))
            plen = np.sort(tl[prow])
            for lo in range(0, nprow, 64):
                csize += int((plen[min(lo + 64, nprow) - 1] + 3) >> 2) * 64
        tiles.append(Tile("G", row0, nrows, npat, nruns, npq, nprow, int(nrows - nprow), int(tl[~prow].sum()), halo, ntv, csize, **info))
    # ---- headers in tile order, then the tile list (flagged tiles last)
    hdr = np.zeros((len(tiles), 16), np.int64)
    sword = cword = 0
    for t, T in enumerate(tiles):
        hdr[t, :12] = (T.row0, T.nrows, T.npat, T.nruns, T.npq, T.nprow, T.row0, T.nsrows, sword, T.nsw, T.row0, int(T.halo))
        hdr[t, 12] = cword if vc else 0
        hdr[t, 14] = T.ntv
        sword += T.nsw
        cword += T.csize
    order = [t for t, T in enumerate(tiles) if not T.halo] + [t for t, T in enumerate(tiles) if T.halo]
    nprow = sum(T.nprow for T in tiles)
    return Model(True, tiles, order, hdr, len(global_patterns), nprow, n_rows - nprow, sum(T.nsw for T in tiles),
                 sum(1 for T in tiles if T.halo), any(T.racy for T in tiles))


HEADER_WORDS_COMPARED = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 15)   # (13: the tile's place in the table array, t x the table stride)
