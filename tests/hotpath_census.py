"""Which branch every stencil slot and every row of the hot path takes, for a given pyramid: NumPy over coordinate lists, written from the
reference's rule (getEdgeStressFaces cpp:1717-1908, getCenterStressFaces cpp:1910-1963, faceOctreeVolumes cpp:1965-2002, applyToMatrix
cpp:2404-2457, buildOctreeSystemFromStencilsPartial cpp:2537-2773), not from the kernels and not from the oracle: it shares no code with
either, and it builds no coefficient -- only the LIST of face ids of every stencil, which is what the row sweep searches.

Input: the label and index pyramids plus the weight lattices (anything shaped like planted_pyramids.PlantedPyramid).  Output: Census with
counts per named branch (BRANCHES), and the reference asserts the pyramid would fire (ASSERTS) with the first site of each.  Arrays are
[z, y, x]; coordinates are (i, j, k) = (x, y, z).
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field

import numpy as np

INACTIVE, ACTIVE, UP, DOWN = 0, 1, 2, 3
UNASSIGNED, SOLIDBOUNDARY, OUTSIDE = -1, -2, -3
EDGE_CAP, CENTER_CAP = 32, 8

EDGE_SLOTS = ("edge_slot_out_of_lattice", "edge_slot_dof_plain", "edge_slot_dof_transition_pair", "edge_slot_dof_transition_face_outside",
              "edge_slot_outside", "edge_slot_solidboundary", "edge_slot_unassigned_odd_parent_id", "edge_slot_unassigned_odd_four_children",
              "edge_slot_unassigned_odd_parent_sentinel", "edge_slot_unassigned_even", "edge_slot_top_level_unassigned")
EDGE_WEIGHTS = ("edge_weight_l0_one", "edge_weight_l0_fractional", "edge_weight_coarse")
CENTER_SLOTS = ("center_slot_dof", "center_slot_four_children", "center_slot_solidboundary", "center_slot_sentinel_skipped")
ROWS = ("row_cell_active", "row_cell_parent_leaf", "row_cell_out_of_lattice", "row_inset_edge_applied", "row_edge_applied",
        "row_sibling_edge_applied", "row_child_edge_applied", "row_two_child_edges_applied", "mass_l0_weight_one", "mass_l0_fractional",
        "mass_coarse", "volume_side_out_of_lattice", "volume_side_active_or_inactive", "volume_side_parent_active")
LENGTHS = ("edge_stencil_len_le_6", "edge_stencil_len_7_8", "edge_stencil_len_gt_8", "self_before_dry_batch", "self_past_dry_batch",
           "self_before_emit_batch", "self_past_emit_batch", "raw_row_le_fast", "raw_row_gt_fast", "raw_row_le_wave", "raw_row_gt_wave")
# per-parity detail of the transition branches: edge[axis] parity picks the sibling, edge[fa] parity picks dangling / parent
PARITY = tuple(f"{b}_edge{e}_face{f}_{p}" for b in ("pair", "odd", "even") for e in "xyz" for f in "xyz" if e != f for p in ("p0", "p1"))
BRANCHES = EDGE_SLOTS + EDGE_WEIGHTS + CENTER_SLOTS + ROWS + LENGTHS
ASSERTS = ("cpp1820", "cpp1853_top_level", "cpp1878", "cpp1891", "center_level0", "center_child", "cpp1996", "cpp2436", "cpp2562_top_level",
           "cpp2680")
STENCIL_ASSERTS = ("cpp1820", "cpp1853_top_level", "cpp1878", "cpp1891", "center_level0", "center_child")      # build_stencils refuses
ROW_ASSERTS = ("cpp1996", "cpp2436", "cpp2562_top_level", "cpp2680")                                           # the row sweep refuses
DRY_BATCH, EMIT_BATCH = 6, 8          # kStencilBatch of k_rows<false> / k_rows<true>; batch_sizes() reads them from the source


def batch_sizes(source_text):
    m = re.search(r"kStencilBatch\s*=\s*EMIT\s*\?\s*(\d+)\s*:\s*(\d+)", source_text)
    return int(m.group(2)), int(m.group(1))


@dataclass
class Census:
    counts: dict = field(default_factory=dict)
    asserts: dict = field(default_factory=dict)        # name -> (count, first site (level, axis, i, j, k))
    edge_lists: object = None                          # (cnt [ne], idx [EDGE_CAP, ne]) in the reference's push order
    center_lists: object = None                        # (cnt [3 nc], idx [CENTER_CAP, 3 nc])
    raw_row_lengths: object = None

    def add(self, name, n):
        self.counts[name] = self.counts.get(name, 0) + int(n)

    def fire(self, name, mask, level, axis, xyz):
        n = int(mask.sum())
        if n:
            c, first = self.asserts.get(name, (0, None))
            if first is None:
                p = xyz[np.flatnonzero(mask)[0]]
                first = (level, axis, int(p[0]), int(p[1]), int(p[2]))
            self.asserts[name] = (c + n, first)

    def refused_by(self):
        return tuple(a for a in ASSERTS if a in self.asserts)


def _at(arr, p, fill):
    """arr[k, j, i] at coordinate rows p = (i, j, k); `fill` and False outside the lattice"""
    shape = np.asarray(arr.shape[::-1])
    ok = ((p >= 0) & (p < shape)).all(axis=1)
    q = np.where(ok[:, None], p, 0)
    return np.where(ok, arr[q[:, 2], q[:, 1], q[:, 0]], fill), ok


def _sites(lat):
    """(xyz [n, 3], ids [n]) of the entries of an index lattice that carry an id"""
    kji = np.argwhere(lat >= 0)
    return kji[:, ::-1].astype(np.int64), lat[lat >= 0].astype(np.int64)


def _unit(a):
    u = np.zeros(3, np.int64)
    u[a] = 1
    return u


class _Lists:
    def __init__(self, cap, n):
        self.cnt = np.zeros(n, np.int64)
        self.idx = np.full((cap, n), -1, np.int64)
        self.overflow = 0

    def push(self, sid, ids):
        """one entry for each stencil of `sid` (ids unique within a call)"""
        c = self.cnt[sid]
        fits = c < self.idx.shape[0]
        self.overflow += int((~fits).sum())
        self.idx[c[fits], sid[fits]] = ids[fits]
        self.cnt[sid[fits]] += 1


def census(pyr, enhanced=True, fast_limit=32, wave_limit=64):
    L = pyr.levels
    labels, vidx, eidx, cidx = pyr.labels, pyr.vidx, pyr.eidx, pyr.cidx
    C = Census()
    for b in BRANCHES + PARITY:
        C.counts[b] = 0
    cell_res = [np.asarray(labels[l].shape[::-1], np.int64) for l in range(L)]

    # ---- edge stencils (cpp:1717-1908) ---------------------------------------------------------------------------------------------------
    E = _Lists(EDGE_CAP, pyr.n_edge)
    for l in range(L):
        for axis in range(3):
            e, eid = _sites(eidx[l][axis])
            if not len(eid):
                continue
            others = [fa for fa in range(3) if fa != axis]
            slot = {}
            at_tr = {ga: np.zeros(len(eid), bool) for ga in others}
            f_out = {ga: np.zeros(len(eid), bool) for ga in others}
            for fa in others:                                   # first sweep: what the two slots across `ga` are (cpp:1740-1787)
                ga = 3 - fa - axis
                for d in (0, 1):
                    face = e - (_unit(ga) if d == 0 else 0)
                    inside = (face[:, ga] >= 0) & (face[:, ga] < cell_res[l][ga])
                    vi, ok = _at(vidx[l][fa], face, UNASSIGNED)
                    assert (ok | ~inside).all()
                    slot[fa, d] = (face, inside, vi)
                    f_out[ga] |= ~inside | (inside & ((vi == OUTSIDE) | (vi == SOLIDBOUNDARY)))
                    if enhanced:
                        at_tr[ga] |= inside & (vi == UNASSIGNED)
            for fa in others:                                   # second sweep, in the reference's push order (cpp:1789-1907)
                ga = 3 - fa - axis
                for d in (0, 1):
                    face, inside, vi = slot[fa, d]
                    C.add("edge_slot_out_of_lattice", (~inside).sum())
                    dof = inside & (vi >= 0)
                    pair = dof & at_tr[ga] & ~f_out[ga]
                    C.add("edge_slot_dof_transition_pair", pair.sum())
                    C.add("edge_slot_dof_transition_face_outside", (dof & at_tr[ga] & f_out[ga]).sum())
                    C.add("edge_slot_dof_plain", (dof & ~at_tr[ga]).sum())
                    if pair.any():
                        even = e[:, axis] % 2 == 0
                        sib = face + np.where(even, 1, -1)[:, None] * _unit(axis)
                        si, ok = _at(vidx[l][fa], sib, UNASSIGNED)
                        C.fire("cpp1820", pair & (si < 0), l, axis, e)
                        good = pair & (si >= 0)
                        E.push(eid[good], si[good])
                        for par in (0, 1):
                            C.add(f"pair_edge{'xyz'[axis]}_face{'xyz'[fa]}_p{par}", (pair & (e[:, axis] % 2 == par)).sum())
                    E.push(eid[dof], vi[dof])
                    C.add("edge_slot_outside", (inside & (vi == OUTSIDE)).sum())
                    C.add("edge_slot_solidboundary", (inside & (vi == SOLIDBOUNDARY)).sum())
                    un = inside & (vi == UNASSIGNED)
                    if l + 1 >= L:
                        C.add("edge_slot_top_level_unassigned", un.sum())
                        C.fire("cpp1853_top_level", un, l, axis, e)
                        continue
                    odd = un & (e[:, fa] % 2 != 0)
                    for par in (0, 1):
                        C.add(f"odd_edge{'xyz'[axis]}_face{'xyz'[fa]}_p{par}", (odd & (e[:, axis] % 2 == par)).sum())
                    for off in (-1, 1):                          # a dangling edge: the two coarse faces it hangs between (cpp:1835-1884)
                        pf = (face + off * _unit(fa)) // 2
                        pi, ok = _at(vidx[l + 1][fa], pf, OUTSIDE)
                        has = odd & ok & (pi >= 0)
                        C.add("edge_slot_unassigned_odd_parent_id", has.sum())
                        E.push(eid[has], pi[has])
                        four = odd & ok & (pi == UNASSIGNED)
                        C.add("edge_slot_unassigned_odd_four_children", four.sum())
                        C.add("edge_slot_unassigned_odd_parent_sentinel", (odd & ~has & ~four).sum())
                        for ci in range(4):
                            cf = 2 * pf + (ci & 1) * _unit((fa + 1) % 3) + ((ci >> 1) & 1) * _unit((fa + 2) % 3)
                            cvi, ok2 = _at(vidx[l][fa], cf, UNASSIGNED)
                            C.fire("cpp1878", four & (cvi < 0), l, axis, e)
                            g = four & (cvi >= 0)
                            E.push(eid[g], cvi[g])
                    ev = un & (e[:, fa] % 2 == 0)
                    C.add("edge_slot_unassigned_even", ev.sum())
                    for par in (0, 1):
                        C.add(f"even_edge{'xyz'[axis]}_face{'xyz'[fa]}_p{par}", (ev & (e[:, axis] % 2 == par)).sum())
                    pi, ok = _at(vidx[l + 1][fa], face // 2, UNASSIGNED)
                    C.fire("cpp1891", ev & (pi < 0), l, axis, e)
                    g = ev & (pi >= 0)
                    E.push(eid[g], pi[g])
            if l == 0:
                w, _ = _at(pyr.edge_weights[axis], e, 0.0)
                C.add("edge_weight_l0_one", (w == 1.0).sum())
                C.add("edge_weight_l0_fractional", (w != 1.0).sum())
            else:
                C.add("edge_weight_coarse", len(eid))
    C.edge_lists = (E.cnt, E.idx)
    C.add("edge_stencil_len_le_6", (E.cnt <= 6).sum())
    C.add("edge_stencil_len_7_8", ((E.cnt > 6) & (E.cnt <= 8)).sum())
    C.add("edge_stencil_len_gt_8", (E.cnt > 8).sum())

    # ---- centre stencils (cpp:1910-1963): list id = cell id + n_center * axis ------------------------------------------------------------
    nc = pyr.n_center
    Cn = _Lists(CENTER_CAP, 3 * nc)
    for l in range(L):
        c, cid = _sites(cidx[l])
        if not len(cid):
            continue
        for axis in range(3):
            for d in (0, 1):
                face = c + d * _unit(axis)
                vi, ok = _at(vidx[l][axis], face, OUTSIDE)
                dof = vi >= 0
                C.add("center_slot_dof", dof.sum())
                Cn.push(cid[dof] + nc * axis, vi[dof])
                un = vi == UNASSIGNED
                C.add("center_slot_four_children", un.sum())
                C.add("center_slot_solidboundary", (vi == SOLIDBOUNDARY).sum())
                C.add("center_slot_sentinel_skipped", (vi == OUTSIDE).sum())
                if l == 0:
                    C.fire("center_level0", un, l, axis, c)
                    continue
                for ci in range(4):
                    cf = 2 * face + (ci & 1) * _unit((axis + 1) % 3) + ((ci >> 1) & 1) * _unit((axis + 2) % 3)
                    cvi, ok2 = _at(vidx[l - 1][axis], cf, UNASSIGNED)
                    C.fire("center_child", un & (cvi < 0), l, axis, c)
                    g = un & (cvi >= 0)
                    Cn.push(cid[g] + nc * axis, cvi[g])
    C.center_lists = (Cn.cnt, Cn.idx)

    # ---- rows (cpp:2537-2773) ------------------------------------------------------------------------------------------------------------
    raw = np.ones(pyr.n_velocity, np.int64)                    # the row's own entry (cpp:2768)

    def apply(kind, vid, sid, level, axis, xyz):
        """the row `vid` applies stencil `sid`: find its own entry (cpp:2422-2436)"""
        cnt, idx = (E.cnt, E.idx) if kind == "edge" else (Cn.cnt, Cn.idx)
        hit = idx[:, sid] == vid[None, :]
        found = hit.any(axis=0)
        C.fire("cpp2436", ~found, level, axis, xyz)
        pos = hit.argmax(axis=0)[found]
        C.add("self_before_dry_batch", (pos < DRY_BATCH).sum())
        C.add("self_past_dry_batch", (pos >= DRY_BATCH).sum())
        C.add("self_before_emit_batch", (pos < EMIT_BATCH).sum())
        C.add("self_past_emit_batch", (pos >= EMIT_BATCH).sum())
        # every entry but those equal to the row's id makes a raw triplet (cpp:2440-2452)
        np.add.at(raw, vid, cnt[sid] - hit.sum(axis=0))

    for l in range(L):
        for axis in range(3):
            f, vid = _sites(vidx[l][axis])
            if not len(vid):
                continue
            for d in (0, 1):
                cell = f - (_unit(axis) if d == 0 else 0)
                lab, inside = _at(labels[l], cell, INACTIVE)
                C.add("row_cell_out_of_lattice", (~inside).sum())
                act = inside & (lab == ACTIVE)
                par = inside & ~act
                C.add("row_cell_active", act.sum())
                C.add("row_cell_parent_leaf", par.sum())
                if l + 1 >= L:
                    C.fire("cpp2562_top_level", par, l, axis, f)
                    par = par & False
                for m, sl, sc in ((act, l, cell), (par, l + 1, cell // 2)):
                    if not m.any():
                        continue
                    ci, ok = _at(cidx[sl], sc, UNASSIGNED)
                    g = m & (ci >= 0)
                    apply("center", vid[g], ci[g] + nc * axis, l, axis, f[g])
                    for fa in range(3):
                        if fa == axis:
                            continue
                        ea = 3 - fa - axis
                        for fd in (0, 1):
                            af = sc + fd * _unit(fa)
                            avi, ok = _at(vidx[sl][fa], af, OUTSIDE)
                            tj = m & (avi == UNASSIGNED)
                            if sl == 0 or not tj.any():
                                assert not (tj.any() and sl == 0)      # a level-0 cell with an UNASSIGNED face: the checkers' business
                                continue
                            for ii in (0, 1):                    # the two fine edges inset in the coarse face (cpp:2614-2649)
                                ce = 2 * af + ii * _unit(ea) + _unit(3 - fa - ea)
                                ei, ok = _at(eidx[sl - 1][ea], ce, UNASSIGNED)
                                g = tj & (ei >= 0)
                                C.add("row_inset_edge_applied", g.sum())
                                apply("edge", vid[g], ei[g], l, axis, f[g])
            for ea in range(3):
                if ea == axis:
                    continue
                ta = 3 - ea - axis
                for d in (0, 1):
                    e = f + d * _unit(ta)
                    ei, ok = _at(eidx[l][ea], e, OUTSIDE)
                    has = ei >= 0
                    if enhanced:                                 # cpp:2664-2697
                        af = f + (1 if d else -1) * _unit(ta)
                        avi, ok = _at(vidx[l][axis], af, OUTSIDE)
                        sb = has & ok & (avi == UNASSIGNED)
                        se = e + np.where(e[:, ea] % 2 == 0, 1, -1)[:, None] * _unit(ea)
                        sei, ok = _at(eidx[l][ea], se, OUTSIDE)
                        C.fire("cpp2680", sb & (sei < 0), l, axis, f)
                        g = sb & (sei >= 0)
                        C.add("row_sibling_edge_applied", g.sum())
                        apply("edge", vid[g], sei[g], l, axis, f[g])
                    C.add("row_edge_applied", has.sum())
                    apply("edge", vid[has], ei[has], l, axis, f[has])
                    un = ei == UNASSIGNED
                    if l == 0 or not un.any():
                        continue
                    n_child = np.zeros(len(vid), np.int64)
                    for ci in (0, 1):                            # cpp:2714-2742
                        ce = 2 * e + ci * _unit(ea)
                        cei, ok = _at(eidx[l - 1][ea], ce, OUTSIDE)
                        g = un & (cei >= 0)
                        n_child += g
                        C.add("row_child_edge_applied", g.sum())
                        apply("edge", vid[g], cei[g], l, axis, f[g])
                    C.add("row_two_child_edges_applied", (n_child == 2).sum())
            # the mass term (cpp:2748-2772) and the arms of faceOctreeVolumes (cpp:1965-2002)
            if l == 0:
                fw, _ = _at(pyr.face_weights[axis], f, 0.0)
                one = fw == 1.0
                C.add("mass_l0_weight_one", one.sum())
                C.add("mass_l0_fractional", (~one).sum())
            else:
                one = np.ones(len(vid), bool)
                C.add("mass_coarse", len(vid))
            for d in (0, 1):
                cell = f - (_unit(axis) if d == 0 else 0)
                lab, inside = _at(labels[l], cell, INACTIVE)
                C.add("volume_side_out_of_lattice", (one & ~inside).sum())
                flat = one & inside & ((lab == ACTIVE) | (lab == INACTIVE))
                C.add("volume_side_active_or_inactive", flat.sum())
                rest = one & inside & ~flat
                if l + 1 < L:
                    pl, ok = _at(labels[l + 1], cell // 2, INACTIVE)
                    good = rest & (pl == ACTIVE)
                else:
                    good = rest & False
                C.add("volume_side_parent_active", good.sum())
                C.fire("cpp1996", rest & ~good, l, axis, f)
    C.raw_row_lengths = raw
    C.add("raw_row_le_fast", (raw <= fast_limit).sum())
    C.add("raw_row_gt_fast", (raw > fast_limit).sum())
    C.add("raw_row_le_wave", (raw <= wave_limit).sum())
    C.add("raw_row_gt_wave", (raw > wave_limit).sum())
    return C


def table(rows):
    """text table: rows = {case name: Census}; one line per branch, one column per case, and the total"""
    names = list(rows)
    out = ["%-44s %10s  " % ("branch", "total") + " ".join("%2d" % i for i in range(len(names)))]
    for b in BRANCHES + PARITY:
        counts = [rows[n].counts.get(b, 0) for n in names]
        out.append("%-44s %10d  " % (b, sum(counts)) + " ".join(" x" if c else " ." for c in counts))
    out.append("cases: " + ", ".join(f"{i}={n}" for i, n in enumerate(names)))
    return "\n".join(out)
