"""NumPy model of the octree cell export (avs_get_octree_cells / avs_prepass_get_octree_cells; outputOctreeGeometry, oct.cpp:245-308).

labels per level -> the ACTIVE cells in the reference's sweep order: levels ascending; inside a level UT_VoxelArray tile order (16^3 tiles,
x fastest, then y, then z), inside a tile x fastest, then y, then z, partial tiles holding the voxels that exist.  Written in the pad /
reshape / permute form `_number` of tests/prepass_torch.py uses; tests/test_octree_cells_model.py pins it to a plain triple loop and to
the oracle's centre-stress numbering.  Lattices are (nz, ny, nx) arrays, x fastest."""
import numpy as np

TILE = 16
ACTIVE = 1
MAX_LEVELS = 8


def level_cells(lab):
    """(n, 3) int32 (i, j, k) of the ACTIVE cells of one lattice, in sweep order"""
    lab = np.asarray(lab)
    pad = [(-s) % TILE for s in lab.shape]
    f = np.pad(lab == ACTIVE, [(0, p) for p in pad])
    tz, ty, tx = (s // TILE for s in f.shape)
    flat = f.reshape(tz, TILE, ty, TILE, tx, TILE).transpose(0, 2, 4, 1, 3, 5).reshape(-1)
    bz, by, bx, lz, ly, lx = np.unravel_index(np.flatnonzero(flat), (tz, ty, tx, TILE, TILE, TILE))
    return np.stack([bx * TILE + lx, by * TILE + ly, bz * TILE + lz], axis=1).astype(np.int32)


def cells(labels, dx, origin=None):
    """position (n, 3) float32, pscale (n,) float32, level (n,) int32, ijk (n, 3) int32, per_level (MAX_LEVELS,) int64"""
    org = np.zeros(3) if origin is None else np.asarray(origin, np.float64).reshape(3)
    pos, ps, lev, ijk = [], [], [], []
    per_level = np.zeros(MAX_LEVELS, np.int64)
    for l, lab in enumerate(labels):
        c = level_cells(lab)
        h = float(dx) * float(1 << l)                      # exact: a power-of-two multiple
        ijk.append(c)
        lev.append(np.full(len(c), l, np.int32))
        ps.append(np.full(len(c), np.float32(h), np.float32))
        pos.append((org[None, :] + (c.astype(np.float64) + 0.5) * h).astype(np.float32))   # fp64, rounded once
        per_level[l] = len(c)
    if not ijk:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros((0, 3), np.int32), per_level
    return np.concatenate(pos), np.concatenate(ps), np.concatenate(lev), np.concatenate(ijk), per_level
