"""The NumPy model of the octree cell export (tests/octree_cells_model.py) against a plain serial sweep and against the oracle's fixtures;
and the two new entries in the built libraries.  No GPU."""
import ctypes
import glob
import os

import numpy as np
import pytest

import octree_cells_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "*.npz")))
PER_LEVEL = {"sphere16_L3": (2664, 8), "beam32_L2_wall_varvisc": (11392, 160), "sphere32_obstacle_rho_usolid": (8272, 26)}


def serial_sweep(lab):
    """for each 16^3 tile (x fastest), for each voxel of the tile that exists (x fastest): the ACTIVE ones"""
    nz, ny, nx = lab.shape
    T = M.TILE
    out = []
    for bz in range(0, nz, T):
        for by in range(0, ny, T):
            for bx in range(0, nx, T):
                for k in range(bz, min(bz + T, nz)):
                    for j in range(by, min(by + T, ny)):
                        for i in range(bx, min(bx + T, nx)):
                            if lab[k, j, i] == M.ACTIVE:
                                out.append((i, j, k))
    return np.array(out, np.int32).reshape(-1, 3)


@pytest.mark.parametrize("shape", [(16, 16, 16), (8, 8, 8), (4, 8, 32), (48, 16, 32)])
def test_model_equals_the_serial_sweep(shape):
    rng = np.random.default_rng(sum(shape))
    lab = rng.integers(0, 4, shape).astype(np.int8)
    want = serial_sweep(lab)
    assert len(want) > 0
    assert np.array_equal(M.level_cells(lab), want)
    pos, ps, lev, ijk, per_level = M.cells([lab], 0.25, origin=(0.1, -3.7, 12.3))
    assert np.array_equal(ijk, want) and per_level[0] == len(want) and not per_level[1:].any()
    assert (lev == 0).all() and (ps == np.float32(0.25)).all()
    assert np.array_equal(pos, (np.array([0.1, -3.7, 12.3]) + (want + 0.5) * 0.25).astype(np.float32))


def test_model_values_per_level():
    labs = [np.zeros((8 >> l, 16 >> l, 32 >> l), np.int8) for l in range(3)]
    labs[0][7, 15, 31] = labs[1][0, 0, 0] = labs[2][1, 3, 7] = M.ACTIVE
    pos, ps, lev, ijk, per_level = M.cells(labs, 0.5)
    assert ijk.tolist() == [[31, 15, 7], [0, 0, 0], [7, 3, 1]] and lev.tolist() == [0, 1, 2] and per_level[:3].tolist() == [1, 1, 1]
    assert ps.tolist() == [0.5, 1.0, 2.0]
    assert pos.tolist() == [[15.75, 7.75, 3.75], [0.5, 0.5, 0.5], [15.0, 7.0, 3.0]]


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p) for p in FIXTURES])
def test_model_is_anchored_to_the_oracle(path):
    """The reference numbers its centre stresses in the same sweep (cpp:1688-1714): along the model's order the ids are increasing."""
    g = np.load(path)
    L = int(g["levels"])
    labels = [g[f"labels{l}"] for l in range(L)]
    pos, ps, lev, ijk, per_level = M.cells(labels, float(g["dx"]))
    name = os.path.basename(path)[:-4]
    if name in PER_LEVEL:
        assert tuple(per_level[:L]) == PER_LEVEL[name]
    ids = np.concatenate([g[f"cidx{l}"][ijk[lev == l, 2], ijk[lev == l, 1], ijk[lev == l, 0]] for l in range(L)])
    ids = ids[ids >= 0]
    assert len(ids) == int(g["counts"][2])
    assert (np.diff(ids) > 0).all()
    for l in range(L):          # every centre-stress cell is ACTIVE
        assert (labels[l][g[f"cidx{l}"] >= 0] == M.ACTIVE).all()
    # the ACTIVE cells cover every level-0 cell at most once
    cover = np.zeros(labels[0].shape, np.int32)
    for l in range(L):
        a = (labels[l] == M.ACTIVE).astype(np.int32)
        for ax in range(3):
            a = np.repeat(a, 1 << l, axis=ax)
        cover += a
    assert cover.max() == 1
    assert sum(8 ** l * int(per_level[l]) for l in range(L)) == int(cover.sum())


def test_both_entries_are_exported(built_lib):
    """libavs_hip.so and the probe build of the same sources (whichever a plug-in links) carry the two entries."""
    from adaptiveviscositysolver_amd import capi
    for sym in ("avs_get_octree_cells", "avs_prepass_get_octree_cells"):
        assert sym in capi.EXPORTED_SYMBOLS
        for path in (capi.LIB_PATH, capi.PROBE_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), sym), (path, sym)
