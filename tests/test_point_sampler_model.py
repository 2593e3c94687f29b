"""The NumPy model of the general-position octree interpolant (tests/point_sampler_model.py) against the CPU oracle, before any GPU is
involved: at the face-lattice position of every regular face the transfer interpolates (regular DOF whose octree index is
AVS_UNASSIGNED) the model must give the oracle's transfer_to_regular_grid value.  The oracle rounds its fp64 result to float once and
reads float node values the model reads as well; the bound is two float roundings of the largest solution entry, 2^-23 * max|x| -- the
model's fp64 noise is far below it."""
import numpy as np
import pytest

from adaptiveviscositysolver_amd import scenes
from oracle import oracle as O
from util import oracle_for_scene

import point_sampler_model as M

CASES = {
    "sphere32_L3": lambda: scenes.sphere(32, 3, device="cpu"),
    "beam64_L3": lambda: scenes.fat_beam(64, 3, device="cpu"),
}


def oracle_interpolator(o, x):
    """(labels, vidx, vel, nval) of an oracle whose transfer has run on x"""
    L = o.levels
    labels = [o.labels(l) for l in range(L)]
    vidx = [[o.index(O.I_VELOCITY, l, a) for a in range(3)] for l in range(L)]
    vel = M.face_velocities(x, o.dof_table(O.I_VELOCITY), vidx)
    nval = [o.node_grid(l)[1] for l in range(L)]
    return labels, vidx, vel, nval


def lattice_face_points(ri, oi, axis):
    """(k, j, i) and q (level-0 cells) of the faces of lattice `axis` that are regular DOFs with an UNASSIGNED octree index"""
    kji = np.argwhere((ri >= 0) & (oi == M.UNASSIGNED))
    q = kji[:, ::-1].astype(np.float64) + 0.5
    q[:, axis] -= 0.5
    return kji, q


@pytest.mark.parametrize("name", list(CASES))
def test_model_matches_oracle_on_the_face_lattice(name):
    sc = CASES[name]()
    o = oracle_for_scene(sc)
    o.prepass()
    o.build_regular_indices()
    o.hot_path()
    x, _ = o.solve(1e-8, 5000, threads=O.max_threads())
    want = o.transfer_to_regular_grid(x)
    labels, vidx, vel, nval = oracle_interpolator(o, x)
    for l in range(o.levels):        # the dof table and the index pyramid name the same faces
        for a in range(3):
            m = vidx[l][a] >= 0
            assert np.array_equal(vel[l][a][m], x[vidx[l][a][m]].astype(np.float32)) and not vel[l][a][~m].any()
    bound = 2.0 ** -23 * np.abs(x).max()
    total = 0
    seen = set()
    for a in range(3):
        kji, q = lattice_face_points(o.regular_index(a), vidx[0][a], a)
        total += len(kji)
        v, branch, inside = M.evaluate(q, labels, vidx, vel, nval)
        assert inside.all()
        seen |= set(np.unique(branch[:, a]).tolist())
        ref = want[a][kji[:, 0], kji[:, 1], kji[:, 2]].astype(np.float64)
        err = np.abs(v[:, a] - ref)
        print(f"{name} axis {a}: {len(kji)} faces, max |model - oracle| = {err.max():.3e}, bound {bound:.3e}")
        assert err.max() <= bound
    assert total >= 1000
    # (an UNASSIGNED face is itself one of the eight faces around its position on a coarser level, or lies between faces of which one is:
    # these positions never take the trilinear branch; both node branches are anchored)
    assert {M.NODE_BIG_FACE, M.NODE_CHILD_FACE} <= seen, seen


def test_model_outside_points():
    sc = CASES["sphere32_L3"]()
    o = oracle_for_scene(sc)
    o.prepass()
    o.hot_path()
    x = o.initial_guess()
    o.build_regular_indices()
    o.transfer_to_regular_grid(x)
    labels, vidx, vel, nval = oracle_interpolator(o, x)
    n = sc.res[0]
    q = np.array([[0.5, 0.5, 0.5], [-0.25, 3.0, 3.0], [3.0, n + 0.5, 3.0], [np.nan, 1.0, 1.0], [n / 2, n / 2, n / 2]])
    v, branch, inside = M.evaluate(q, labels, vidx, vel, nval)
    assert inside.tolist() == [0, 0, 0, 0, 1]           # (the corner of the grid is air, the centre of the sphere liquid)
    assert not v[:4].any() and (branch[:4] == M.OUTSIDE).all() and (branch[4] != M.OUTSIDE).all()
