"""avs_sample_velocity: the solved octree velocity at arbitrary points on the device (k_sample_points, avs_post.hip).

Reference for arbitrary points: tests/point_sampler_model.py (NumPy fp64, anchored to the CPU oracle by test_point_sampler_model.py),
fed with the library's own pyramids, dof table, solution and node grids.  Bound: the library rounds an fp64 result to float once, and
its fp64 operations differ from the model's only in noise far below that; 2^-23 * max|x| is two float roundings of the largest
solution entry.  On the regular face lattice the sampler and the transfer run the same device function on the same values: bit-exact."""

import numpy as np
import pytest
import torch

from adaptiveviscositysolver_amd import DevicePrepass, ViscositySolve, capi, scenes

import point_sampler_model as M

pytestmark = pytest.mark.gpu

CASES = {
    "sphere32_L3": lambda dev: scenes.sphere(32, 3, device=dev),
    "beam64_L4": lambda dev: scenes.fat_beam(64, 4, device=dev),
    "beam64_wall_varvisc": lambda dev: scenes.fat_beam(64, 3, wall=True, variable_viscosity=True, device=dev),
}


class Frame:
    """one scene through pre-pass, assembly and solve; pyramids and solution on the host"""

    def __init__(self, name, precision=capi.PRECISION_F64, solve=True):
        dev = torch.device("cuda:0")
        self.sc = scenes.to_device(CASES[name]("cpu"), dev)
        self.pp = DevicePrepass(self.sc.res, self.sc.dx, self.sc.levels)
        self.info = self.pp.run(self.sc.liquid, self.sc.solid)
        self.L = int(self.info.levels)
        self.s = self.context(precision)
        self.labels = [self.pp.labels(l) for l in range(self.L)]
        self.vidx = [[self.pp.index(capi.INDEX_VELOCITY, l, a) for a in range(3)] for l in range(self.L)]
        self.x = None
        if solve:
            self.s.solve(1e-10, 5000)
            self.x = self.s.solution()
        self._model = None

    def context(self, precision=capi.PRECISION_F64):
        s = ViscositySolve(self.sc.res, self.sc.dx, self.sc.dt, self.L, device=0, precision=precision)
        self.pp.apply(s)
        s.set_scene_fields(self.sc)
        s.assemble()
        return s

    def covered(self):
        """level-0 cells under an ACTIVE cell of some level, (nz, ny, nx) bool -- from the label pyramid alone"""
        cov = np.zeros(self.labels[0].shape, bool)
        for l in range(self.L):
            a = self.labels[l] == M.ACTIVE
            for ax in range(3):
                a = np.repeat(a, 1 << l, axis=ax)
            cov |= a
        return cov

    def model(self, points, origin=None):
        if self._model is None:       # (the node grids are there once the library has built its interpolator: after any sample / transfer)
            vel = M.face_velocities(self.x, self.s.dof_table(), self.vidx)
            nval = [self.s.node_grid(l)[1] for l in range(self.L)]
            self._model = (vel, nval)
        return M.evaluate(M.positions_to_q(points, self.sc.dx, origin), self.labels, self.vidx, *self._model)

    def lattice_points(self, axis):
        """(k, j, i) and world positions (float32, exact: dx is a power of two) of the regular DOF faces with an UNASSIGNED octree index"""
        kji = np.argwhere((self.pp.regular_index(axis) >= 0) & (self.vidx[0][axis] == capi.UNASSIGNED))
        q = kji[:, ::-1].astype(np.float64) + 0.5
        q[:, axis] -= 0.5
        p = (q * self.sc.dx).astype(np.float32)
        assert np.array_equal(p.astype(np.float64) / self.sc.dx, q)
        return kji, p

    def close(self):
        self.s.close()
        self.pp.close()


_frames = {}


@pytest.fixture
def frame(request, built_lib):
    name = request.param
    if name not in _frames:
        _frames[name] = Frame(name)
    return _frames[name]


all_scenes = pytest.mark.parametrize("frame", list(CASES), indirect=True)
one_scene = pytest.mark.parametrize("frame", ["beam64_wall_varvisc"], indirect=True)


def check_lattice(f, s):
    out = s.transfer_to_regular_grid()
    total = 0
    for a in range(3):
        kji, p = f.lattice_points(a)
        total += len(kji)
        v, inside = s.sample_velocity(p)
        assert inside.all()
        assert np.array_equal(v[:, a], out[a][kji[:, 0], kji[:, 1], kji[:, 2]]), a      # bit for bit
    assert total >= 1000, total


@all_scenes
def test_lattice_points_equal_the_transfer_bit_for_bit(frame):
    check_lattice(frame, frame.s)


def test_lattice_points_on_a_float_precision_context(built_lib):
    f = Frame("sphere32_L3", precision=capi.PRECISION_F32)
    check_lattice(f, f.s)
    f.close()


def arbitrary_points(f, rng, n_random=20000, n_exact=500):
    """Points built from the pyramids: ACTIVE cells of every level, half of them cells with an UNASSIGNED face, a random offset inside the
    cell; then points exactly on cell corners, edges and faces (offsets 0 or 1 along three, two, one axes: coordinates that are multiples
    of dx * 2^l), kept where the label pyramid has an ACTIVE cell over the level-0 cell the position falls into (forward cell on a tie)."""
    cov = f.covered()
    n = np.array(f.sc.res)
    per_level, qs, exact = n_random // f.L, [], []
    for l in range(f.L):
        act = f.labels[l] == M.ACTIVE
        cells = np.argwhere(act)[:, ::-1]              # x, y, z
        if len(cells) == 0:
            continue
        tj = np.zeros(len(cells), bool)
        for a in range(3):
            e = np.zeros(3, np.int64)
            e[a] = 1
            for c in (cells, cells + e):
                tj |= f.vidx[l][a][c[:, 2], c[:, 1], c[:, 0]] == capi.UNASSIGNED
        want = per_level if l < f.L - 1 else n_random - per_level * (f.L - 1)
        pools = [cells[tj], cells] if tj.any() else [cells, cells]
        for pool, count in ((pools[0], want // 2), (pools[1], want - want // 2)):
            pick = pool[rng.integers(0, len(pool), count)]
            qs.append((pick + rng.random((count, 3))) * (1 << l))
        pick = cells[rng.integers(0, len(cells), 4 * n_exact)]
        u = rng.integers(1, 64, (len(pick), 3)) / 64.0   # (the free coordinates: 64ths of the cell, exact in float32 like the pinned ones)
        kind = rng.integers(1, 4, len(pick))            # number of axes with an offset of exactly 0 or 1
        for i in range(len(pick)):
            ax = rng.permutation(3)[:kind[i]]
            u[i, ax] = rng.integers(0, 2, kind[i])
        exact.append((pick + u) * (1 << l))
    q = np.concatenate(qs)
    p = (q * f.sc.dx).astype(np.float32)
    e = np.concatenate(exact)
    e = e[rng.permutation(len(e))]
    c = np.minimum(np.floor(e).astype(np.int64), n[None, :] - 1)
    e = e[cov[c[:, 2], c[:, 1], c[:, 0]]][:n_exact]
    assert len(p) == n_random and len(e) == n_exact
    pe = (e * f.sc.dx).astype(np.float32)
    assert np.array_equal(pe.astype(np.float64) / f.sc.dx, e)      # exactly on the lattice lines
    return np.concatenate([p, pe])


@all_scenes
def test_arbitrary_points_match_the_model(frame):
    f = frame
    p = arbitrary_points(f, np.random.default_rng(12345))
    v, inside = f.s.sample_velocity(p)
    assert inside.all()
    want, branch, m_inside = f.model(p)
    assert m_inside.all()
    for b in (M.TRILINEAR, M.NODE_BIG_FACE, M.NODE_CHILD_FACE):
        count = int((branch == b).any(axis=1).sum())
        print(f"{M.BRANCH_NAMES[b]}: {count} points")
        assert count >= 200, (M.BRANCH_NAMES[b], count)
    bound = 2.0 ** -23 * np.abs(f.x).max()
    err = np.abs(v.astype(np.float64) - want)
    print(f"max |gpu - model| = {err.max():.3e}, bound {bound:.3e}")
    assert err.max() <= bound


@all_scenes
def test_outside_points(frame):
    f = frame
    rng = np.random.default_rng(7)
    air = np.argwhere(~f.covered())[:, ::-1]
    assert len(air) >= 1000
    q = air[rng.integers(0, len(air), 1000)] + rng.random((1000, 3)) * 0.98 + 0.01
    n = np.array(f.sc.res, np.float64)
    beyond = np.array([[-0.5, 3, 3], [3, n[1] + 0.25, 3], [3, 3, n[2] + 4], [-1e30, 1, 1], [1, 1e30, 1], [np.inf, 1, 1], [1, -np.inf, 1],
                       [np.nan, 1, 1], [1, 1, np.nan]])
    p = (np.concatenate([q, beyond]) * f.sc.dx).astype(np.float32)
    v, inside = f.s.sample_velocity(p)
    assert not inside.any() and not v.any() and not np.isnan(v).any()
    # inside = NULL is accepted
    v2 = np.full(p.shape, 5.0, np.float32)
    capi.check(f.s.lib.avs_sample_velocity(f.s.h, len(p), p.ctypes.data, None, v2.ctypes.data, None, capi.MEM_HOST))
    assert not v2.any()


def test_rigid_translation_is_sampled_exactly(built_lib):
    dev = torch.device("cuda:0")
    sc = scenes.fat_beam(128, 4, device=dev)
    cv = (0.5, -2.0, 1.25)
    sc.velocity = scenes.constant_velocity(sc.res, cv, device=dev)
    pp = DevicePrepass(sc.res, sc.dx, sc.levels)
    info = pp.run(sc.liquid, sc.solid)
    s = ViscositySolve(sc.res, sc.dx, sc.dt, info.levels, device=0)
    pp.apply(s)
    s.set_scene_fields(sc)
    s.assemble()
    assert s.solve(1e-8, 50).iterations == 0
    shrink = 3 * (1 << (info.levels - 1)) * sc.dx                 # three coarsest cells
    half = np.array([0.45, 0.225, 0.225]) - shrink
    assert (half > 0).all()
    rng = np.random.default_rng(3)
    p = (0.5 + (rng.random((5000, 3)) * 2.0 - 1.0) * half).astype(np.float32)
    v, inside = s.sample_velocity(p)
    assert inside.all()
    for a in range(3):
        assert np.array_equal(v[:, a], np.full(len(p), cv[a], np.float32))    # interpolation weights sum to one, exactly
    s.close()
    pp.close()


@pytest.mark.parametrize("temporal", ["1", "0"])
def test_stale_state(temporal, monkeypatch, built_lib):
    """The node grids are kept between calls and rebuilt when the solution, the pyramids or the dof tables change."""
    monkeypatch.setenv("AVS_PREPASS_TEMPORAL", temporal)
    f = Frame("beam64_wall_varvisc")
    s, x = f.s, f.x
    p = arbitrary_points(f, np.random.default_rng(99), 4000, 100)
    # sampling twice: identical bits; a new solution: the node grids follow it (scaling by two is exact in every operation)
    v1, in1 = s.sample_velocity(p)
    v1b, in1b = s.sample_velocity(p)
    assert np.array_equal(v1, v1b) and np.array_equal(in1, in1b) and v1.any()
    s.set_solution(2.0 * x)
    v2, _ = s.sample_velocity(p)
    assert np.array_equal(v2, 2.0 * v1)
    s.set_solution(x)
    # transfer -> sample -> transfer: the sampler leaves the staging grids as a transfer does
    t1 = s.transfer_to_regular_grid()
    v3, _ = s.sample_velocity(p)
    t2 = s.transfer_to_regular_grid()
    fresh = f.context()
    fresh.set_solution(x)
    t3 = fresh.transfer_to_regular_grid()
    v4, _ = fresh.sample_velocity(p)
    for a in range(3):
        assert np.array_equal(t1[a], t2[a]) and np.array_equal(t1[a], t3[a]), a
    assert np.array_equal(v3, v1) and np.array_equal(v4, v1)
    # a new frame on the same context (another pyramid lent by the pre-pass): what a fresh context gives
    sc2 = scenes.to_device(scenes.fat_beam(64, 3, device="cpu"), torch.device("cuda:0"))
    assert f.pp.run(sc2.liquid, sc2.solid).levels == f.L
    f.sc = sc2
    f.pp.apply(s)
    s.set_scene_fields(sc2)
    s.assemble()
    s.solve(1e-10, 5000)
    x2 = s.solution()
    v5, in5 = s.sample_velocity(p)
    fresh2 = f.context()
    fresh2.set_solution(x2)
    v6, in6 = fresh2.sample_velocity(p)
    assert np.array_equal(v5, v6) and np.array_equal(in5, in6) and not np.array_equal(v5, v1)
    fresh.close()
    fresh2.close()
    f.close()


@one_scene
def test_host_and_device_memspace(frame):
    f = frame
    origin = (1.0, -2.0, 0.5)
    p0 = arbitrary_points(f, np.random.default_rng(5), 4000, 100)
    p = (p0.astype(np.float64) + np.array(origin)).astype(np.float32)
    vh, ih = f.s.sample_velocity(p, origin)
    want, _, m_inside = f.model(p, origin)
    assert np.array_equal(ih, m_inside) and ih.mean() > 0.99       # (adding the origin rounds the positions: a few may leave the band)
    assert np.abs(vh - want).max() <= 2.0 ** -23 * np.abs(f.x).max()
    pd = torch.from_numpy(p).cuda()
    vd, idv = f.s.sample_velocity(pd, origin)
    assert vd.is_cuda and idv.is_cuda and vd.dtype == torch.float32 and idv.dtype == torch.uint8
    assert np.array_equal(vd.cpu().numpy(), vh) and np.array_equal(idv.cpu().numpy(), ih)
    perm = np.random.default_rng(6).permutation(len(p))
    vp, ip = f.s.sample_velocity(np.ascontiguousarray(p[perm]), origin)
    assert np.array_equal(vp, vh[perm]) and np.array_equal(ip, ih[perm])
    vpd, _ = f.s.sample_velocity(pd[torch.from_numpy(perm).cuda()].contiguous(), origin)
    assert np.array_equal(vpd.cpu().numpy(), vh[perm])


def test_errors(built_lib):
    f = Frame("sphere32_L3", solve=False)
    s, lib = f.s, f.s.lib
    p = np.full((4, 3), 0.5, np.float32)
    v = np.zeros((4, 3), np.float32)
    ins = np.zeros(4, np.uint8)
    call = lambda h, n, pp_, vv: lib.avs_sample_velocity(h, n, pp_, None, vv, ins.ctypes.data, capi.MEM_HOST)
    assert call(s.h, 4, p.ctypes.data, v.ctypes.data) == capi.ESTATE              # before any solve
    s.solve(1e-6, 100)
    assert call(s.h, 4, None, v.ctypes.data) == capi.EINVAL
    assert call(s.h, 4, p.ctypes.data, None) == capi.EINVAL
    assert call(None, 4, p.ctypes.data, v.ctypes.data) == capi.EINVAL
    assert call(s.h, -1, p.ctypes.data, v.ctypes.data) == capi.EINVAL
    assert call(s.h, 0, None, None) == capi.OK                                     # nothing is touched
    assert call(s.h, 4, p.ctypes.data, v.ctypes.data) == capi.OK and ins.all()
    ve, ie = s.sample_velocity(np.zeros((0, 3), np.float32))
    assert ve.shape == (0, 3) and ie.shape == (0,)
    # a slab-local context (this rank's window of the lattices only)
    pp = DevicePrepass(f.sc.res, f.sc.dx, f.sc.levels)
    n = f.sc.res[0]
    pp.set_slab(0, [0, n // 2, n], 0, lambda ptr, count, stream: None)
    assert pp.run(f.sc.liquid, f.sc.solid).levels == f.L
    s2 = ViscositySolve(f.sc.res, f.sc.dx, f.sc.dt, f.L, device=0)
    pp.apply(s2)
    s2.set_solution(np.zeros(s2.counts[0], np.float64))
    assert call(s2.h, 4, p.ctypes.data, v.ctypes.data) == capi.ESTATE
    assert b"slab" in lib.avs_last_error()
    s2.close()
    pp.close()
    f.close()
