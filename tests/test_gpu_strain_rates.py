"""avs_get_strain_rates / avs_get_shear_rate_field: strain rates, dissipation and the shear-rate field on the device (avs_strain.hip).

Reference: tests/strain_rate_model.py (NumPy; anchored to the CPU oracle by test_strain_rate_model.py), fed with what the library itself
holds: its stencils, its index pyramids and its velocity vector.  Tolerances: edge and centre rates bit for bit (the same operations in
the same order, one rounding each); a cell's shear rate within 1 ulp (2^-52 relative: the margin is for the device's fp64 division and
square root alone); counters exact; a dissipation within n_terms * 2^-52 relative of the exact sum of its terms (math.fsum) -- the rigorous
bound for a sum of non-negative terms in any order."""
import ctypes as C

import numpy as np
import pytest
import torch

from adaptiveviscositysolver_amd import DevicePrepass, ViscositySolve, capi, scenes
from independent import face_positions

import strain_rate_model as M

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52
SHEAR = 3.0
TRANSLATION = (1.0, -2.0, 0.5)
SOLUTION, GUESS = capi.RATES_OF_SOLUTION, capi.RATES_OF_INITIAL_GUESS
SCENES = {
    "sphere32_L3": lambda: scenes.sphere(32, 3),
    "sphere64_L4": lambda: scenes.sphere(64, 4),
    "beam64_L3_wall_varvisc": lambda: scenes.fat_beam(64, 3, wall=True, variable_viscosity=True),
}
SUMMARY_COUNTERS = ("n_edge", "n_center", "empty_edges", "empty_centers", "boundary_edges", "boundary_centers", "nonfinite", "edge_lookups",
                    "empty_pairs")


class Frame:
    """one scene through DevicePrepass -> ViscositySolve; what the model needs is read back from the objects themselves"""

    def __init__(self, name, solve=True, precision=capi.PRECISION_F64):
        self.sc = sc = scenes.to_device(SCENES[name](), torch.device("cuda:0"))
        self.pp = pp = DevicePrepass(sc.res, sc.dx, sc.levels)
        info = pp.run(sc.liquid, sc.solid)
        self.L = L = int(info.levels)
        self.n_edge, self.n_center = int(info.n_edge), int(info.n_center)
        self.s = s = ViscositySolve(sc.res, sc.dx, sc.dt, L, device=0, precision=precision)
        pp.apply(s)
        s.set_scene_fields(sc)
        if solve:
            s.assemble()
            assert s.solve(1e-6, 3000).converged
        else:
            s.build_stencils()
            s.build_initial_guess()
        # before any stencil is read back: the slots behind cnt / bcnt still hold whatever the allocation held
        self.first = s.strain_rates(SOLUTION if solve else GUESS)
        self.labels = [pp.labels(l) for l in range(L)]
        self.eidx = [[pp.index(capi.INDEX_EDGE, l, a) for a in range(3)] for l in range(L)]
        self.cidx = [pp.index(capi.INDEX_CENTER, l) for l in range(L)]
        self.edge, self.center = s.edge_stencils(), s.center_stencils()

    def model(self, u):
        return M.evaluate(self.labels, self.eidx, self.cidx, self.n_edge, self.n_center, self.edge, self.center, u, self.s.field_res)

    def close(self):
        self.s.close()
        self.pp.close()


@pytest.fixture(scope="module")
def frames(built_lib):
    made = {}

    def get(name, solve=True, precision=capi.PRECISION_F64):
        key = (name, solve, precision)
        if key not in made:
            made[key] = Frame(name, solve, precision)
        return made[key]
    yield get
    for f in made.values():
        f.close()


def same_bytes(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in ((a.edge, b.edge), (a.center, b.center), (a.cell, b.cell))) and \
        a.summary == b.summary


def agree(got, want):
    """a StrainRates against the model's dict"""
    assert got.edge.tobytes() == want["edge"].tobytes()
    assert got.center.tobytes() == want["center"].tobytes()
    err = np.abs(got.cell - want["cell"])
    print("cell shear rate: worst error in ulps", float((err / np.maximum(np.abs(want["cell"]), 1e-300)).max() / ULP))
    assert (err <= ULP * np.abs(want["cell"])).all()
    ws, gs = want["summary"], got.summary
    for k in SUMMARY_COUNTERS:
        assert getattr(gs, k) == ws[k], (k, getattr(gs, k), ws[k])
    assert gs.max_abs_edge_rate == ws["max_abs_edge_rate"] and gs.max_abs_center_rate == ws["max_abs_center_rate"]
    assert gs.max_shear_rate == float(got.cell[np.isfinite(got.cell)].max()) and abs(gs.max_shear_rate - ws["max_shear_rate"]) <= ULP * ws["max_shear_rate"]
    for k, terms in (("dissipation_edge", ws["edge_terms"]), ("dissipation_center", ws["center_terms"])):
        print(k, getattr(gs, k), "exact", ws[k], "terms", terms)
        assert abs(getattr(gs, k) - ws[k]) <= terms * ULP * ws[k]


# ---- 1. parity against the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere32_L3", "beam64_L3_wall_varvisc"])
def test_parity_with_the_model(frames, name):
    f = frames(name)
    want = f.model(f.s.solution())
    got = f.s.strain_rates()
    agree(got, want)
    assert same_bytes(got, f.first)            # ... and the same bytes as before the stencils were padded for the read-back
    assert got.summary.which == SOLUTION and got.summary.dissipation_edge > 0 and got.summary.max_shear_rate > 0
    if name == "sphere32_L3":
        assert got.summary.edge_lookups == (33816, 1392, 96, 2904)       # every branch of the cell pass
    else:
        s = got.summary
        assert s.empty_edges > 0 and s.empty_centers > 0 and s.boundary_edges > 0 and s.boundary_centers > 0


@pytest.mark.parametrize("name", ["sphere32_L3", "beam64_L3_wall_varvisc"])
def test_field_is_the_cell_array_painted(frames, name):
    f = frames(name)
    cell = f.s.strain_rates().cell
    ids = M.cell_ids(f.labels, f.cidx, f.s.field_res)
    field = f.s.shear_rate_field()
    assert field.shape == ids.shape and field.dtype == np.float32
    assert (ids >= 0).any() and (ids < 0).any()
    assert np.array_equal(field[ids >= 0], cell[ids[ids >= 0]].astype(np.float32)) and (field[ids < 0] == 0).all()
    assert field.tobytes() == M.paint(f.labels, f.cidx, cell, f.s.field_res).tobytes()
    assert f.s.shear_rate_field(device_array=True).cpu().numpy().tobytes() == field.tobytes()
    # a device array that does not start on a 16-byte boundary is painted cell by cell
    buf = torch.full((field.size + 2,), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    capi.check(f.s.lib.avs_get_shear_rate_field(f.s.h, SOLUTION, buf.data_ptr() + 4, capi.MEM_DEVICE))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert got[0] == -7.0 and got[-1] == -7.0 and got[1:-1].tobytes() == field.tobytes()


@pytest.mark.parametrize("fres,center,half", [((48, 40, 24), (24, 20, 12), (17, 13, 6.5)),
                                              ((50, 33, 17), (25, 16.5, 8.5), (18, 10, 3.4))])      # rows of 50: no 16-byte stores
def test_field_on_a_padded_simulation_grid(built_lib, fres, center, half):
    """the 48 x 40 x 24 and 50 x 33 x 17 simulation grids of test_gpu_post.py::test_non_power_of_two_simulation_grid inside a 64^3 octree
    grid: only the field_n* window exists in the output"""
    n, levels = 64, 3
    dx = 1.0 / n
    liquid = scenes.box_sdf((n, n, n), dx, center=tuple(c * dx for c in center), half=tuple(h * dx for h in half))
    crop = lambda t, add=(0, 0, 0): t[:fres[2] + add[2], :fres[1] + add[1], :fres[0] + add[0]].contiguous()
    vel = scenes.smooth_velocity((n, n, n), dx, gravity_dt=0.1)
    pp = DevicePrepass((n, n, n), dx, levels, field_res=fres)
    info = pp.run(crop(liquid).cuda(), None)
    L = int(info.levels)
    s = ViscositySolve((n, n, n), dx, 1.0 / 60.0, L, device=0, field_res=fres)
    pp.apply(s)
    s.set_field(capi.FIELD_VISCOSITY, 0, None, 100.0)
    s.set_field(capi.FIELD_DENSITY, 0, None, 1000.0)
    for a in range(3):
        s.set_field(capi.FIELD_VELOCITY, a, crop(vel[a], tuple(1 if b == a else 0 for b in range(3))).cuda())
        s.set_field(capi.FIELD_SOLID_VELOCITY, a, None, 0.0)
    s.build_stencils()
    s.build_initial_guess()
    got = s.strain_rates(GUESS)
    labels, cidx = [pp.labels(l) for l in range(L)], [pp.index(capi.INDEX_CENTER, l) for l in range(L)]
    ids = M.cell_ids(labels, cidx, fres)
    guard = np.full(fres[0] * fres[1] * fres[2] + 64, np.float32(-7.0))       # nothing behind the window is written
    capi.check(s.lib.avs_get_shear_rate_field(s.h, GUESS, guard.ctypes.data, capi.MEM_HOST))
    field = s.shear_rate_field(GUESS)
    assert field.shape == (fres[2], fres[1], fres[0]) and guard[:field.size].tobytes() == field.tobytes() and (guard[field.size:] == -7.0).all()
    assert (ids >= 0).any() and got.cell.max() > 0
    assert np.array_equal(field[ids >= 0], got.cell[ids[ids >= 0]].astype(np.float32)) and (field[ids < 0] == 0).all()
    eidx = [[pp.index(capi.INDEX_EDGE, l, a) for a in range(3)] for l in range(L)]
    agree(got, M.evaluate(labels, eidx, cidx, int(info.n_edge), int(info.n_center), s.edge_stencils(), s.center_stencils(), s.initial_guess()))
    s.close()
    pp.close()


# ---- 2. known answers through set_solution ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere32_L3", "sphere64_L4"])
def test_known_answers(frames, name):
    f = frames(name, solve=False)
    s = f.s
    vel_table, edge_table = s.dof_table(capi.INDEX_VELOCITY), s.dof_table(capi.INDEX_EDGE)
    pos, ax, _ = face_positions(vel_table, f.sc.dx)
    a = SHEAR
    s.set_solution(np.where(ax == 0, a * pos[:, 1], 0.0))                       # u = (a y, 0, 0)
    got = s.strain_rates()
    e_ax = (edge_table[:, 0] >> 8) & 0xff
    want = np.where(e_ax == 2, a / 2, 0.0)
    print("edge", np.abs(got.edge - want).max(), "centre", np.abs(got.center).max(), "cell", np.abs(got.cell - a).max())
    assert (e_ax == 2).any() and np.abs(got.edge - want).max() <= 1e-9 * a
    assert np.abs(got.center).max() <= 1e-9 * a
    assert len(got.cell) == f.n_center > 0 and (np.abs(got.cell - a) <= 1e-9 * a).all()
    assert got.summary.empty_pairs == 0 and got.summary.nonfinite == 0
    ids = M.cell_ids(f.labels, f.cidx, s.field_res)
    field = s.shear_rate_field()
    assert np.array_equal(field == np.float32(a), ids >= 0) and (field[ids < 0] == 0).all()
    s.set_solution(np.asarray(TRANSLATION, np.float64)[ax])                     # a rigid translation
    got = s.strain_rates()
    bound = 1e-12 * max(abs(v) for v in TRANSLATION) / f.sc.dx
    worst = max(np.abs(got.edge).max(), np.abs(got.center).max(), np.abs(got.cell).max())
    print("translation: worst rate", worst, "bound", bound)
    assert worst <= bound and got.summary.max_shear_rate <= bound


# ---- 3. the initial-guess path ------------------------------------------------------------------------------------------------------------
def test_initial_guess_path_needs_no_system(frames):
    f = frames("sphere32_L3", solve=False)
    s = f.s
    with pytest.raises(capi.AvsError) as e:
        s.csr()
    assert e.value.status == capi.ESTATE                                         # nothing was assembled
    a, fa = s.strain_rates(GUESS), s.shear_rate_field(GUESS)
    assert a.summary.which == GUESS and a.summary.max_shear_rate > 0
    s.set_solution(s.initial_guess())
    b, fb = s.strain_rates(SOLUTION), s.shear_rate_field(SOLUTION)
    assert a.edge.tobytes() == b.edge.tobytes() and a.center.tobytes() == b.center.tobytes() and a.cell.tobytes() == b.cell.tobytes()
    assert fa.tobytes() == fb.tobytes()
    sa, sb = dict(vars(a.summary)), dict(vars(b.summary))
    sa.pop("which"), sb.pop("which")
    assert sa == sb
    agree(a, f.model(s.initial_guess()))


# ---- 4. capped grids, memory spaces, calling variants ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere32_L3", "beam64_L3_wall_varvisc"])
def test_capped_grid_gives_the_same_bytes(frames, monkeypatch, name):
    """AVS_CELLS_GRID_CAP=3: three workgroups walk every pass (13 trips over the edges of sphere32): a partial sum belongs to a chunk of
    256 stencils, not to a workgroup, so the dissipations are the same bytes too"""
    f = frames(name)
    want, wfield = f.s.strain_rates(), f.s.shear_rate_field()
    monkeypatch.setenv("AVS_CELLS_GRID_CAP", "3")
    try:
        f.s.set_solver_option(capi.OPTION_RELOAD_ENVIRONMENT, 1)                 # (the environment is read at avs_create)
        got, gfield = f.s.strain_rates(), f.s.shear_rate_field()
    finally:
        monkeypatch.delenv("AVS_CELLS_GRID_CAP")
        f.s.set_solver_option(capi.OPTION_RELOAD_ENVIRONMENT, 1)
    assert same_bytes(got, want) and gfield.tobytes() == wfield.tobytes()


def test_device_and_host_arrays_and_null_outputs(frames):
    f = frames("sphere32_L3")
    s = f.s
    host = s.strain_rates()
    dev = s.strain_rates(device_arrays=True)
    assert all(t.is_cuda for t in (dev.edge, dev.center, dev.cell))
    assert same_bytes(capi_host(dev), host)
    assert same_bytes(s.strain_rates(), host)                                    # a second call
    sizes = (f.n_edge, 3 * f.n_center, f.n_center)
    full = (host.edge, host.center, host.cell)
    for where in (capi.MEM_HOST, capi.MEM_DEVICE):
        for mask in range(16):                                                   # every subset of the four outputs
            if where == capi.MEM_HOST:
                bufs = [np.full(n, -7.0) if mask >> k & 1 else None for k, n in enumerate(sizes)]
                ptrs = [None if b is None else b.ctypes.data for b in bufs]
            else:
                bufs = [torch.full((n,), -7.0, dtype=torch.float64, device="cuda:0") if mask >> k & 1 else None for k, n in enumerate(sizes)]
                torch.cuda.synchronize()
                ptrs = [None if b is None else b.data_ptr() for b in bufs]
            summ = capi.StrainSummary() if mask & 8 else None
            capi.check(s.lib.avs_get_strain_rates(s.h, SOLUTION, *ptrs, None if summ is None else C.byref(summ), where))
            torch.cuda.synchronize()
            for b, want in zip(bufs, full):
                if b is not None:
                    assert (b if where == capi.MEM_HOST else b.cpu().numpy()).tobytes() == want.tobytes(), (where, mask)
            if summ is not None:
                assert summ.dissipation_edge == host.summary.dissipation_edge and summ.dissipation_center == host.summary.dissipation_center
                assert tuple(summ.edge_lookups) == host.summary.edge_lookups and summ.max_shear_rate == host.summary.max_shear_rate


def capi_host(r):
    """a StrainRates of device tensors as one of NumPy arrays"""
    from adaptiveviscositysolver_amd.solver import StrainRates
    return StrainRates(r.edge.cpu().numpy(), r.center.cpu().numpy(), r.cell.cpu().numpy(), r.summary)


def test_fresh_context_gives_the_same_bytes(frames):
    f = frames("sphere32_L3")
    want, wfield = f.s.strain_rates(), f.s.shear_rate_field()
    g = Frame("sphere32_L3", solve=False)                                        # its own pre-pass, stencils and scratch
    g.s.set_solution(f.s.solution())
    assert same_bytes(g.s.strain_rates(), want) and g.s.shear_rate_field().tobytes() == wfield.tobytes()
    g.close()


def test_float_precision_context(frames):
    """AVS_PRECISION_F32: the same evaluation on the values the context stores (float values in fp64 arrays)"""
    f = frames("sphere32_L3", precision=capi.PRECISION_F32)
    x = f.s.solution()
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64)) and np.abs(x).max() > 0
    agree(f.s.strain_rates(), f.model(x))


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------------------
def raw_rates(s, which, summary=None, where=capi.MEM_HOST):
    buf = np.zeros(max(3 * (s.counts[2] if s.counts else 0), s.counts[1] if s.counts else 0, 1))
    st = s.lib.avs_get_strain_rates(s.h, which, None, None, None if summary is not None else buf.ctypes.data,
                                    None if summary is None else C.byref(summary), where)
    return st, (s.lib.avs_last_error().decode() if st != capi.OK else "")


def raw_field(s, which, where=capi.MEM_HOST, null=False):
    nx, ny, nz = s.field_res
    buf = np.zeros(nx * ny * nz, np.float32)
    st = s.lib.avs_get_shear_rate_field(s.h, which, None if null else buf.ctypes.data, where)
    return st, (s.lib.avs_last_error().decode() if st != capi.OK else "")


def test_state_errors(built_lib):
    sc = scenes.to_device(SCENES["sphere32_L3"](), torch.device("cuda:0"))
    pp = DevicePrepass(sc.res, sc.dx, sc.levels)
    info = pp.run(sc.liquid, sc.solid)
    s = ViscositySolve(sc.res, sc.dx, sc.dt, info.levels, device=0)
    pp.apply(s)
    s.set_scene_fields(sc)
    for which in (SOLUTION, GUESS):                                              # before the stencils
        for st, err in (raw_rates(s, which), raw_field(s, which)):
            assert st == capi.ESTATE and "stencils" in err, err
    s.build_stencils()
    for st, err in (raw_rates(s, GUESS), raw_field(s, GUESS)):                   # before the initial guess
        assert st == capi.ESTATE and "initial guess" in err, err
    s.build_initial_guess()
    assert raw_rates(s, GUESS)[0] == capi.OK and raw_field(s, GUESS)[0] == capi.OK
    for st, err in (raw_rates(s, SOLUTION), raw_field(s, SOLUTION)):             # before a solution
        assert st == capi.ESTATE and "solution" in err, err
    s.assemble()
    assert raw_rates(s, SOLUTION)[0] == capi.ESTATE                              # assembled, still not solved
    assert s.solve(1e-6, 3000).converged
    assert raw_rates(s, SOLUTION)[0] == capi.OK and raw_field(s, SOLUTION)[0] == capi.OK
    s.close()
    pp.close()


def test_argument_errors(frames):
    f = frames("sphere32_L3")
    s = f.s
    for which in (-1, 2, 7):
        for st, err in (raw_rates(s, which), raw_field(s, which)):
            assert st == capi.EINVAL and err, which
    for where in (2, -1):
        for st, err in (raw_rates(s, SOLUTION, where=where), raw_field(s, SOLUTION, where=where)):
            assert st == capi.EINVAL and "memory space" in err
    st, err = raw_field(s, SOLUTION, null=True)
    assert st == capi.EINVAL and err
    assert s.lib.avs_get_strain_rates(None, SOLUTION, None, None, None, None, capi.MEM_HOST) == capi.EINVAL
    for size in (0, 4, 7, -8, 4097):
        summ = capi.StrainSummary()
        summ.struct_size = size
        st, err = raw_rates(s, SOLUTION, summ)
        assert st == capi.EINVAL and "struct_size" in err, size
    assert s.lib.avs_get_strain_rates(s.h, SOLUTION, None, None, None, None, capi.MEM_HOST) == capi.OK      # nothing asked for


def test_smaller_struct_size_writes_only_that_many_bytes(frames):
    f = frames("sphere32_L3")
    s = f.s
    full = capi.StrainSummary()
    capi.check(s.lib.avs_get_strain_rates(s.h, SOLUTION, None, None, None, C.byref(full), capi.MEM_HOST))
    assert C.sizeof(full) == 144 and full.struct_size == 144 and full.n_edge == f.n_edge and full.max_shear_rate > 0
    for size in (8, 24, 56, 100, 136, 144, 200):      # ... up to which, n_center, boundary_edges, inside edge_lookups, one field short, all, a larger future struct
        buf = (C.c_ubyte * 256)(*([0x5a] * 256))
        summ = capi.StrainSummary.from_buffer(buf)
        summ.struct_size = size
        capi.check(s.lib.avs_get_strain_rates(s.h, SOLUTION, None, None, None, C.byref(summ), capi.MEM_HOST))
        written = min(size, 144)
        assert bytes(buf)[4:written] == bytes(full)[4:written] and summ.struct_size == size
        assert all(b == 0x5a for b in bytes(buf)[written:])


# ---- 6. the round trip of a shear-dependent viscosity ---------------------------------------------------------------------------------------------
def test_shear_dependent_viscosity_round_trip(built_lib):
    """provisional fields -> stencils + initial guess -> shear-rate field -> mu = mu0 / (1 + gamma) -> viscosity field -> assemble ->
    the system passes its check -> the solve converges"""
    f = Frame("sphere32_L3", solve=False)
    s = f.s
    gamma = s.shear_rate_field(GUESS)
    assert gamma.max() > 0 and np.isfinite(gamma).all()
    mu0 = 100.0
    mu = (mu0 / (1.0 + gamma.astype(np.float64))).astype(np.float32)
    assert mu.min() < mu.max() <= mu0
    s.set_field(capi.FIELD_VISCOSITY, 0, mu)
    s.assemble()
    # bitwise symmetry is not what a variable viscosity gives (two roundings of one entry); the tolerance of test_gpu_csr_check.py
    exact = s.check_system()
    assert exact.violations[:7] == (0,) * 7, exact
    rep = s.check_system(symmetry_tolerance=1e-12 * exact.max_abs_value)
    print("asymmetric entries", exact.asymmetric_entries, "largest", exact.max_abs_asymmetry, "of", exact.max_abs_value)
    assert rep.passed, rep
    info = s.solve(1e-6, 3000)
    assert info.converged and info.iterations > 0
    got = s.strain_rates()
    assert got.summary.nonfinite == 0 and got.summary.dissipation_edge > 0
    f.close()
