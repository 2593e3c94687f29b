"""avs_apply_viscosity_model: a shear-dependent viscosity evaluated and installed on the device (avs_viscosity.hip), and the fixed-point
loop over it (ViscositySolve.solve_shear_dependent).

Reference: tests/viscosity_model.py (NumPy, written from include/avs.h; tests/test_viscosity_model.py shows on the CPU that these scenes
hold fringe cells, untouched cells, ids on both clamps and cells at rest), fed with the cell shear rates of tests/strain_rate_model.py.
Tolerances: counts and the covered / fringe / untouched partition exact; cells at rest, clamped values and the Newtonian limits bit for
bit; every other value within ONE float32 ulp -- both sides evaluate in fp64 and round once, and the few fp64 ulps np.power / np.expm1
may differ from the device's pow / expm1 by move the rounded float by one ulp at most.  Relaxation, border replication and the installed
lattice are exact operations on floats: bit for bit.  The contexts live in the probe build of the same sources, whose
avs_viscosity_lattice_probe reads the context's viscosity lattice back."""
import ctypes as C

import numpy as np
import pytest
import torch

from adaptiveviscositysolver_amd import DevicePrepass, ViscositySolve, capi, scenes

import strain_rate_model as S
import viscosity_model as V

pytestmark = pytest.mark.gpu

SOLUTION, GUESS = capi.RATES_OF_SOLUTION, capi.RATES_OF_INITIAL_GUESS
ULP64 = 2.0 ** -52
SCENES = ("sphere32_L3", "beam64_L3_wall_varvisc", "box48x40x24_in_64", "box47x40x24_in_64")    # rows of 47: no 16-byte stores
PADDED = {"box48x40x24_in_64": ((48, 40, 24), (24, 20, 12), (17, 13, 6.5)), "box47x40x24_in_64": ((47, 40, 24), (23.5, 20, 12), (17, 13, 6.5))}


def to_capi(p, **change):
    p = dict(p, **change)
    return capi.ViscosityModel(kind=p["kind"], mu_0=p["mu_0"], mu_inf=p["mu_inf"], lambda_=p["lambda"], a=p["a"], n=p["n"],
                               consistency=p["consistency"], tau_y=p["tau_y"], regularisation=p["regularisation"], mu_min=p["mu_min"],
                               mu_max=p["mu_max"], relaxation=p["relaxation"])


class Frame:
    """one scene through DevicePrepass -> ViscositySolve, both in the probe library; what the model needs is read back from the objects"""

    def __init__(self, name, solve=True):
        dev = torch.device("cuda:0")
        if name in PADDED:                      # the padded simulation grids of test_gpu_strain_rates.py inside a 64^3 octree grid
            fres, center, half = PADDED[name]
            n, levels = 64, 3
            dx, dt = 1.0 / n, 1.0 / 60.0
            liquid = scenes.box_sdf((n, n, n), dx, center=tuple(c * dx for c in center), half=tuple(h * dx for h in half))
            crop = lambda t, add=(0, 0, 0): t[:fres[2] + add[2], :fres[1] + add[1], :fres[0] + add[0]].contiguous()
            vel = scenes.smooth_velocity((n, n, n), dx, gravity_dt=0.1)
            self.pp = pp = DevicePrepass((n, n, n), dx, levels, field_res=fres, probe=True)
            info = pp.run(crop(liquid).cuda(), None)
            self.s = s = ViscositySolve((n, n, n), dx, dt, int(info.levels), device=0, field_res=fres, probe=True)
            pp.apply(s)
            s.set_field(capi.FIELD_VISCOSITY, 0, None, 100.0)
            s.set_field(capi.FIELD_DENSITY, 0, None, 1000.0)
            for a in range(3):
                s.set_field(capi.FIELD_VELOCITY, a, crop(vel[a], tuple(1 if b == a else 0 for b in range(3))).cuda())
                s.set_field(capi.FIELD_SOLID_VELOCITY, a, None, 0.0)
        else:
            sc = scenes.to_device({"sphere32_L3": lambda: scenes.sphere(32, 3),
                                   "beam64_L3_wall_varvisc": lambda: scenes.fat_beam(64, 3, wall=True, variable_viscosity=True)}[name](), dev)
            self.pp = pp = DevicePrepass(sc.res, sc.dx, sc.levels, probe=True)
            info = pp.run(sc.liquid, sc.solid)
            self.s = s = ViscositySolve(sc.res, sc.dx, sc.dt, int(info.levels), device=0, probe=True)
            pp.apply(s)
            s.set_scene_fields(sc)
        self.L = L = int(info.levels)
        self.n_edge, self.n_center = int(info.n_edge), int(info.n_center)
        if solve:
            s.assemble()
            assert s.solve(1e-6, 3000).converged
        else:
            s.build_stencils()
            s.build_initial_guess()
        self.labels = [pp.labels(l) for l in range(L)]
        self.cidx = [pp.index(capi.INDEX_CENTER, l) for l in range(L)]
        self.eidx = [[pp.index(capi.INDEX_EDGE, l, a) for a in range(3)] for l in range(L)]
        self.ids = S.cell_ids(self.labels, self.cidx, s.field_res)
        self.shear = {}

    def g(self, which):
        """the cells' shear rates of the NumPy strain model, from the stencils and the vector the context holds"""
        if which not in self.shear:
            s = self.s
            u = s.solution() if which == SOLUTION else s.initial_guess()
            self.shear[which] = S.evaluate(self.labels, self.eidx, self.cidx, self.n_edge, self.n_center, s.edge_stencils(), s.center_stencils(), u)["cell"]
        return self.shear[which]

    def close(self):
        self.s.close()
        self.pp.close()


def viscosity_lattice(s):
    """(padded lattice (nz, ny, nx), None) or (None, constant): the context's viscosity as the assembly reads it"""
    nx, ny, nz = s.res
    out, const, is_const = np.full((nz, ny, nx), np.float32(-7.0)), C.c_float(), C.c_int32()
    capi.check(s.lib.avs_viscosity_lattice_probe(s.h, out.ctypes.data, C.byref(const), C.byref(is_const), capi.MEM_HOST))
    return (None, np.float32(const.value)) if is_const.value else (out, None)


def old_viscosity(s):
    """the current viscosity on the simulation grid: an array, or the constant"""
    lat, const = viscosity_lattice(s)
    nx, ny, nz = s.field_res
    return const if lat is None else np.ascontiguousarray(lat[:nz, :ny, :nx])


@pytest.fixture(scope="module")
def frames(built_lib):
    made = {}

    def get(name, solve=True):
        if (name, solve) not in made:
            made[name, solve] = Frame(name, solve)
        return made[name, solve]
    yield get
    for f in made.values():
        f.close()


def summary_counts(s):
    return {k: getattr(s, k) for k in ("n_center", "covered", "fringe", "untouched", "clamped_low", "clamped_high", "nonfinite")}


def agree(f, p, which, field, summ, old):
    """a device result against the model's"""
    g = f.g(which)
    want = V.evaluate(p, g, f.ids, old)
    ws = want["summary"]
    print({k: ws[k] for k in ws}, "device", summ)
    assert summary_counts(summ) == {k: ws[k] for k in summary_counts(summ)}
    assert (summ.which, summ.kind, summ.installed) == (which, p["kind"], False)
    touched = want["covered"] | want["fringe"]
    assert field[want["untouched"]].tobytes() == want["field"][want["untouched"]].tobytes()      # they keep their viscosity, exactly
    assert (field[touched] > 0).all() and np.isfinite(field).all()
    ulps = V.ulps_apart(field[touched], want["field"][touched])
    print("cells off by one ulp:", int((ulps == 1).sum()), "of", int(touched.sum()), "worst", int(ulps.max()))
    if p["relaxation"] == 1.0:                                                   # (relaxed values: exact arithmetic on these, tested as such)
        assert ulps.max() <= 1
    # bit for bit: cells at rest, clamped values, the Newtonian limits
    v = want["per_id"]
    cid = f.ids[want["covered"]]
    exact_id = (g == 0) | v["low"] | v["high"] | (p["n"] == 1.0 and p["tau_y"] == 0.0)
    sel = np.zeros(f.ids.shape, bool)
    sel[want["covered"]] = exact_id[cid]
    if p["relaxation"] == 1.0:
        assert field[sel].tobytes() == want["field"][sel].tobytes()
    # the extrema are those of the device's own arrays (exact), and the model's within the same bounds
    o64 = np.broadcast_to(np.asarray(old, np.float32), field.shape).astype(np.float64)
    cov = want["covered"]
    assert summ.max_relative_change == float((np.abs(field.astype(np.float64)[cov] - o64[cov]) / o64[cov]).max())
    assert abs(summ.max_shear_rate - ws["max_shear_rate"]) <= ULP64 * ws["max_shear_rate"]
    if p["relaxation"] == 1.0:
        assert summ.min_viscosity == float(field[cov].min()) and summ.max_viscosity == float(field[cov].max())
        assert V.ulps_apart(np.float32(summ.min_viscosity), np.float32(ws["min_viscosity"])) <= 1
        assert V.ulps_apart(np.float32(summ.max_viscosity), np.float32(ws["max_viscosity"])) <= 1
    return want


# ---- 1. parity with the model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [SOLUTION, GUESS])
@pytest.mark.parametrize("name", SCENES)
def test_parity_with_the_model(frames, name, which):
    f = frames(name)
    old = old_viscosity(f.s)
    assert (np.ndim(old) == 3) == (name == "beam64_L3_wall_varvisc")            # a viscosity field and the constant are both read
    for case in ("carreau", "bingham", "newtonian_carreau", "newtonian_hb"):
        p = V.CASES[case]
        field, summ = f.s.apply_viscosity_model(to_capi(p), which)
        want = agree(f, p, which, field, summ, old)
        s = want["summary"]
        assert s["fringe"] > 0 and s["untouched"] > 0
        if case in ("carreau", "bingham") and name in ("sphere32_L3", "beam64_L3_wall_varvisc") and which == GUESS:
            assert s["clamped_low"] > 0 and s["clamped_high"] > 0               # (what test_viscosity_model.py shows for the oracle's pyramids)
        if case.startswith("newtonian"):
            assert (field[want["covered"] | want["fringe"]] == np.float32(70.0)).all() and summ.min_viscosity == summ.max_viscosity == 70.0


@pytest.mark.parametrize("name", ["sphere32_L3", "beam64_L3_wall_varvisc", "box47x40x24_in_64"])
def test_relaxation_is_exact_arithmetic_on_the_unrelaxed_field(frames, name):
    """new = (float)(old + omega (M - old)) in fp64 from the M the call with omega = 1 returns: bit for bit; untouched cells keep old"""
    f = frames(name)
    old = old_viscosity(f.s)
    for case in ("carreau_relaxed", "bingham_relaxed"):
        p = V.CASES[case]
        M, s1 = f.s.apply_viscosity_model(to_capi(p, relaxation=1.0), GUESS)
        new, sw = f.s.apply_viscosity_model(to_capi(p), GUESS)
        want = agree(f, p, GUESS, new, sw, old)
        o64 = np.broadcast_to(np.asarray(old, np.float32), M.shape).astype(np.float64)
        expect = (o64 + p["relaxation"] * (M.astype(np.float64) - o64)).astype(np.float32)
        expect[want["untouched"]] = M[want["untouched"]]
        assert new.tobytes() == expect.tobytes() and not np.array_equal(new, M)
        assert (sw.min_viscosity, sw.max_viscosity, sw.max_shear_rate) == (s1.min_viscosity, s1.max_viscosity, s1.max_shear_rate)   # of M
        assert 0 < sw.max_relative_change < s1.max_relative_change


# ---- 2. install ------------------------------------------------------------------------------------------------------------------------------
def system_bytes(s):
    return [np.asarray(a).tobytes() for a in s.csr()]


@pytest.mark.parametrize("name", ["sphere32_L3", "box48x40x24_in_64", "box47x40x24_in_64"])
def test_install_gives_the_bytes_of_set_field(built_lib, name):
    """install = 1, assemble against mu_out -> set_field -> assemble: the same viscosity lattice (borders replicated onto the padding), CSR
    and right-hand side; first over the scene's constant, then relaxed over the lattice the first round left"""
    a, b = Frame(name, solve=False), Frame(name, solve=False)
    for case in ("carreau", "bingham_relaxed"):
        m = to_capi(V.CASES[case])
        mu, sa = a.s.apply_viscosity_model(m, GUESS)
        a.s.set_field(capi.FIELD_VISCOSITY, 0, mu)
        a.s.assemble()
        mu_b, sb = b.s.apply_viscosity_model(m, GUESS, install=True)
        assert sb.installed and not sa.installed and summary_counts(sa) == summary_counts(sb) and mu_b.tobytes() == mu.tobytes()
        lat_a, lat_b = viscosity_lattice(a.s)[0], viscosity_lattice(b.s)[0]
        nx, ny, nz = b.s.res
        assert lat_b is not None and lat_b.tobytes() == lat_a.tobytes() == V.replicate_onto(mu, (nz, ny, nx)).tobytes()
        with pytest.raises(capi.AvsError) as e:                                  # the invalidation of avs_set_scalar_field
            b.s.csr()
        assert e.value.status == capi.ESTATE
        b.s.assemble()
        assert system_bytes(a.s) == system_bytes(b.s)
    # install alone: no array, no summary
    m = to_capi(V.CASES["carreau_relaxed"])
    mu, _ = a.s.apply_viscosity_model(m, GUESS)
    capi.check(b.s.lib.avs_apply_viscosity_model(b.s.h, GUESS, C.byref(m), None, 1, None, capi.MEM_HOST))
    nx, ny, nz = b.s.res
    assert viscosity_lattice(b.s)[0].tobytes() == V.replicate_onto(mu, (nz, ny, nx)).tobytes()
    a.close()
    b.close()


def test_after_install_the_solution_is_gone(built_lib):
    f = Frame("sphere32_L3")
    s = f.s
    m = to_capi(V.CASES["carreau"])
    rates = np.zeros(f.n_center)
    field = np.zeros(s.field_res[0] * s.field_res[1] * s.field_res[2], np.float32)
    _, summ = s.apply_viscosity_model(m, SOLUTION, install=True)
    assert summ.installed and summ.which == SOLUTION and summ.covered > 0
    for which in (SOLUTION, GUESS):
        for st in (s.lib.avs_get_strain_rates(s.h, which, None, None, rates.ctypes.data, None, capi.MEM_HOST),
                   s.lib.avs_get_shear_rate_field(s.h, which, field.ctypes.data, capi.MEM_HOST),
                   s.lib.avs_apply_viscosity_model(s.h, which, C.byref(m), field.ctypes.data, 0, None, capi.MEM_HOST)):
            assert st == capi.ESTATE and "stencils" in s.lib.avs_last_error().decode()
    with pytest.raises(capi.AvsError):
        s.solution()
    s.assemble()
    assert s.lib.avs_get_strain_rates(s.h, SOLUTION, None, None, rates.ctypes.data, None, capi.MEM_HOST) == capi.ESTATE      # not solved yet
    assert s.solve(1e-6, 3000).converged
    assert s.apply_viscosity_model(m, SOLUTION)[1].covered == summ.covered
    f.close()


# ---- 3. capped grids, fresh contexts, memory spaces, calling variants --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere32_L3", "beam64_L3_wall_varvisc", "box47x40x24_in_64"])
def test_capped_grid_gives_the_same_bytes(frames, monkeypatch, name):
    """AVS_CELLS_GRID_CAP=3: three workgroups walk every pass, tile after tile"""
    f = frames(name)
    m = to_capi(V.CASES["bingham_relaxed"])
    want, ws = f.s.apply_viscosity_model(m)
    monkeypatch.setenv("AVS_CELLS_GRID_CAP", "3")
    try:
        f.s.set_solver_option(capi.OPTION_RELOAD_ENVIRONMENT, 1)                 # (the environment is read at avs_create)
        got, gs = f.s.apply_viscosity_model(m)
    finally:
        monkeypatch.delenv("AVS_CELLS_GRID_CAP")
        f.s.set_solver_option(capi.OPTION_RELOAD_ENVIRONMENT, 1)
    assert got.tobytes() == want.tobytes() and gs == ws


def test_fresh_context_gives_the_same_bytes(frames):
    f = frames("sphere32_L3")
    m = to_capi(V.CASES["carreau"])
    want, ws = f.s.apply_viscosity_model(m)
    g = Frame("sphere32_L3", solve=False)                                        # its own pre-pass, stencils and scratch
    g.s.set_solution(f.s.solution())
    got, gs = g.s.apply_viscosity_model(m)
    assert got.tobytes() == want.tobytes() and gs == ws
    g.close()


def test_device_and_host_arrays_and_null_outputs(frames):
    f = frames("beam64_L3_wall_varvisc")
    s = f.s
    m = to_capi(V.CASES["carreau_relaxed"])
    host, hs = s.apply_viscosity_model(m)
    dev, ds = s.apply_viscosity_model(m, device_array=True)
    assert dev.is_cuda and dev.cpu().numpy().tobytes() == host.tobytes() and ds == hs
    for where in (capi.MEM_HOST, capi.MEM_DEVICE):
        for want_out in (False, True):
            for want_summary in (False, True):
                if where == capi.MEM_HOST:
                    buf = np.full(host.size + 8, np.float32(-7.0))
                    ptr = buf.ctypes.data
                else:
                    buf = torch.full((host.size + 8,), -7.0, dtype=torch.float32, device="cuda:0")
                    torch.cuda.synchronize()
                    ptr = buf.data_ptr()
                summ = capi.ViscositySummary() if want_summary else None
                capi.check(s.lib.avs_apply_viscosity_model(s.h, SOLUTION, C.byref(m), ptr if want_out else None, 0,
                                                           None if summ is None else C.byref(summ), where))
                torch.cuda.synchronize()
                got = buf if where == capi.MEM_HOST else buf.cpu().numpy()
                assert (got[host.size:] == -7.0).all()                          # nothing behind the window is written
                assert got[:host.size].tobytes() == host.tobytes() if want_out else (got == -7.0).all(), (where, want_out, want_summary)
                if summ is not None:
                    assert (summ.covered, summ.fringe, summ.max_relative_change, summ.max_viscosity) == \
                        (hs.covered, hs.fringe, hs.max_relative_change, hs.max_viscosity)
    # a device array that does not start on a 16-byte boundary is written cell by cell
    buf = torch.full((host.size + 2,), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    capi.check(s.lib.avs_apply_viscosity_model(s.h, SOLUTION, C.byref(m), buf.data_ptr() + 4, 0, None, capi.MEM_DEVICE))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert got[0] == -7.0 and got[-1] == -7.0 and got[1:-1].tobytes() == host.tobytes()


def test_smaller_struct_size_writes_only_that_many_bytes(frames):
    s = frames("sphere32_L3").s
    m = to_capi(V.CASES["carreau"])
    full = capi.ViscositySummary()
    capi.check(s.lib.avs_apply_viscosity_model(s.h, SOLUTION, C.byref(m), None, 0, C.byref(full), capi.MEM_HOST))
    assert C.sizeof(full) == 104 and full.struct_size == 104 and full.covered > 0 and full.max_relative_change > 0
    for size in (8, 16, 24, 52, 96, 104, 200):      # ... up to which, installed, n_center, inside untouched, one field short, all, a larger future struct
        buf = (C.c_ubyte * 256)(*([0x5a] * 256))
        summ = capi.ViscositySummary.from_buffer(buf)
        summ.struct_size = size
        capi.check(s.lib.avs_apply_viscosity_model(s.h, SOLUTION, C.byref(m), None, 0, C.byref(summ), capi.MEM_HOST))
        written = min(size, 104)
        assert bytes(buf)[4:written] == bytes(full)[4:written] and summ.struct_size == size
        assert all(b == 0x5a for b in bytes(buf)[written:])


# ---- 4. errors -------------------------------------------------------------------------------------------------------------------------------
def raw_apply(s, which, m, where=capi.MEM_HOST, summary=None, null_out=False):
    nx, ny, nz = s.field_res
    buf = np.zeros(nx * ny * nz, np.float32)
    st = s.lib.avs_apply_viscosity_model(s.h, which, None if m is None else C.byref(m), None if null_out else buf.ctypes.data, 0,
                                         None if summary is None else C.byref(summary), where)
    return st, (s.lib.avs_last_error().decode() if st != capi.OK else "")


def test_state_errors(built_lib):
    sc = scenes.to_device(scenes.sphere(32, 3), torch.device("cuda:0"))
    pp = DevicePrepass(sc.res, sc.dx, sc.levels)
    info = pp.run(sc.liquid, sc.solid)
    s = ViscositySolve(sc.res, sc.dx, sc.dt, info.levels, device=0)
    pp.apply(s)
    s.set_scene_fields(sc)
    m = to_capi(V.CASES["carreau"])
    for which in (SOLUTION, GUESS):                                              # before the stencils
        st, err = raw_apply(s, which, m)
        assert st == capi.ESTATE and "stencils" in err, err
    s.build_stencils()
    st, err = raw_apply(s, GUESS, m)                                             # before the initial guess
    assert st == capi.ESTATE and "initial guess" in err, err
    s.build_initial_guess()
    assert raw_apply(s, GUESS, m)[0] == capi.OK
    st, err = raw_apply(s, SOLUTION, m)                                          # before a solution
    assert st == capi.ESTATE and "solution" in err, err
    s.assemble()
    assert raw_apply(s, SOLUTION, m)[0] == capi.ESTATE                           # assembled, still not solved
    assert s.solve(1e-6, 3000).converged
    assert raw_apply(s, SOLUTION, m)[0] == capi.OK
    s.close()
    pp.close()


CARREAU_ERRORS = [("mu_0", -1.0), ("mu_0", np.nan), ("mu_0", np.inf), ("mu_inf", -1.0), ("mu_inf", np.nan), ("lambda", -0.5), ("lambda", np.inf),
                  ("lambda", np.nan), ("a", 0.0), ("a", -2.0), ("a", np.nan), ("a", np.inf), ("n", np.nan), ("n", np.inf)]
BINGHAM_ERRORS = [("consistency", -1.0), ("consistency", np.nan), ("consistency", np.inf), ("n", np.nan), ("n", -np.inf), ("tau_y", -1.0),
                  ("tau_y", np.nan), ("tau_y", np.inf), ("regularisation", -1.0), ("regularisation", np.nan), ("regularisation", np.inf),
                  ("regularisation", 0.0)]                                       # (a yield stress needs a regularisation)
COMMON_ERRORS = [("mu_min", 0.0), ("mu_min", -1.0), ("mu_min", 1e-50), ("mu_min", np.nan), ("mu_min", np.inf), ("mu_max", 1.0), ("mu_max", np.nan),
                 ("mu_max", np.inf), ("mu_max", 1e39), ("relaxation", 0.0), ("relaxation", -0.5), ("relaxation", 1.5), ("relaxation", np.nan),
                 ("relaxation", np.inf)]


def test_argument_errors(frames):
    s = frames("sphere32_L3").s
    good = to_capi(V.CASES["carreau"])
    for which in (-1, 2, 7):
        st, err = raw_apply(s, which, good)
        assert st == capi.EINVAL and err, which
    for where in (2, -1):
        st, err = raw_apply(s, SOLUTION, good, where=where)
        assert st == capi.EINVAL and "memory space" in err
    assert raw_apply(s, SOLUTION, None)[0] == capi.EINVAL
    assert s.lib.avs_apply_viscosity_model(None, SOLUTION, C.byref(good), None, 0, None, capi.MEM_HOST) == capi.EINVAL
    for size in (0, 4, 7, -8, 4097):
        summ = capi.ViscositySummary()
        summ.struct_size = size
        st, err = raw_apply(s, SOLUTION, good, summary=summ)
        assert st == capi.EINVAL and "avs_viscosity_summary.struct_size" in err, size
    for size in (0, 88, 95, 4097):
        m = to_capi(V.CASES["carreau"])
        m.struct_size = size
        st, err = raw_apply(s, SOLUTION, m)
        assert st == capi.EINVAL and "avs_viscosity_model.struct_size" in err, size
    for kind in (-1, 2):
        st, err = raw_apply(s, SOLUTION, to_capi(V.CASES["carreau"], kind=kind))
        assert st == capi.EINVAL and "kind" in err
    for case, errors in (("carreau", CARREAU_ERRORS + COMMON_ERRORS), ("bingham", BINGHAM_ERRORS + COMMON_ERRORS)):
        for name, value in errors:
            for null_out in (False, True):                                       # checked before "nothing asked for"
                st, err = raw_apply(s, SOLUTION, to_capi(V.CASES[case], **{name: value}), null_out=null_out)
                assert st == capi.EINVAL and "avs_viscosity_model." + name in err, (case, name, value, err)
    # the parameters of the other kind are not read
    assert raw_apply(s, SOLUTION, to_capi(V.CASES["carreau"], consistency=np.nan, tau_y=-1.0, regularisation=np.nan))[0] == capi.OK
    assert raw_apply(s, SOLUTION, to_capi(V.CASES["bingham"], mu_0=np.nan, mu_inf=-1.0, a=0.0, **{"lambda": np.nan}))[0] == capi.OK
    assert raw_apply(s, SOLUTION, to_capi(V.CASES["newtonian_hb"]))[0] == capi.OK                           # no yield stress: regularisation 0
    assert raw_apply(s, SOLUTION, good, null_out=True)[0] == capi.OK                                        # nothing asked for


# ---- 5. the fringe matters ---------------------------------------------------------------------------------------------------------------------
def test_the_fringe_continues_the_liquid_instead_of_mu_zero(frames):
    """a shear-thinning Carreau fluid (n < 1) on the sphere, whose liquid is sheared everywhere: the air cells next to the liquid -- the
    cells the viscosity samples of the level-0 surface edges interpolate from -- take the mean of their covered neighbours, below mu_0,
    where gamma -> mu(gamma) of the shear-rate field (0 in the air) puts mu_0, the largest value the material has"""
    f = frames("sphere32_L3", solve=False)
    p = V.carreau_yasuda(100.0, 1.0, 0.5, 2.0, 0.5, 1.0, 1000.0)
    field, summ = f.s.apply_viscosity_model(to_capi(p), GUESS)
    want = V.evaluate(p, f.g(GUESS), f.ids, old_viscosity(f.s))
    level0 = np.zeros(f.ids.shape, bool)                                         # cells covered by level-0 ACTIVE cells
    level0[:] = (f.labels[0] == S.ACTIVE) & (f.ids >= 0)
    pad = np.pad(level0, 1)
    near = np.zeros_like(level0)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                near |= pad[dz:dz + level0.shape[0], dy:dy + level0.shape[1], dx:dx + level0.shape[2]]
    sampled = near & want["fringe"]                                             # the air around the level-0 surface
    assert sampled.sum() > 1000 and summ.clamped_low == summ.clamped_high == 0 and f.g(GUESS).min() > 0
    print("fringe next to level 0:", int(sampled.sum()), "largest viscosity", float(field[sampled].max()), "mu_0", p["mu_0"], "liquid max", summ.max_viscosity)
    assert field[sampled].max() <= summ.max_viscosity < p["mu_0"]
    gamma = f.s.shear_rate_field(GUESS)
    recipe = V.per_id(p, gamma.astype(np.float64).ravel())["P"].reshape(gamma.shape)
    assert (gamma[sampled] == 0).all() and (recipe[sampled] == np.float32(p["mu_0"])).all()


# ---- 6. the fixed-point loop ---------------------------------------------------------------------------------------------------------------------
TOL, PICARD_TOL, MAX_PICARD = 1e-8, 1e-3, 20
# the solve's claim against the true residual of the system the context holds: single-digit factors on scenes of this kind (4.6 and 2.5 in
# test_gpu_solution_check.py); a context left with the system of ANOTHER viscosity would miss it by the size of the last change, ~1e-3 / 1e-8
CLAIM_FACTOR = 10.0


def test_solve_shear_dependent(built_lib):
    f = Frame("sphere32_L3", solve=False)
    s = f.s
    p = V.carreau_yasuda(100.0, 1.0, 0.5, 2.0, 0.5, 1.0, 1000.0)
    r = s.solve_shear_dependent(to_capi(p), tol=TOL, max_iters=3000, picard_tol=PICARD_TOL, max_picard=MAX_PICARD)
    print("solves", len(r.solves), "iterations", [i.iterations for i in r.solves], "changes", [q.max_relative_change for q in r.summaries])
    assert r.converged and 1 <= len(r.solves) == len(r.summaries) <= MAX_PICARD and all(i.converged for i in r.solves)
    assert r.summaries[-1].max_relative_change <= PICARD_TOL and r.initial.installed and not r.summaries[-1].installed
    assert len(r.solves) > 1 and r.summaries[0].max_relative_change > PICARD_TOL                  # the loop had something to do
    # still solved, by the system that produced the solution
    rep = s.check_solution()
    print("true residual", rep.relative_residual, "claimed", rep.claimed_error)
    assert rep.evaluated and rep.claimed_converged == 1 and rep.claimed_error == r.solves[-1].error and rep.claimed_iterations == r.solves[-1].iterations
    assert rep.relative_residual <= CLAIM_FACTOR * TOL
    x = s.solution()
    assert np.isfinite(x).all() and np.abs(x).max() > 0
    # the installed field is the model of the returned solution within the measure
    lattice = old_viscosity(s)
    assert np.ndim(lattice) == 3
    want = V.evaluate(p, f.g(SOLUTION), f.ids, lattice)
    cov = want["covered"]
    change = np.abs(want["field"].astype(np.float64)[cov] - lattice.astype(np.float64)[cov]) / lattice.astype(np.float64)[cov]
    print("model of the solution against the installed field: largest relative change", float(change.max()))
    assert change.max() <= PICARD_TOL * (1 + 2.0 ** -20)                          # (one float ulp of the model's value)
    f.close()


def test_solve_shear_dependent_newtonian_is_one_plain_solve(built_lib):
    """a Newtonian model: the first evaluation on the solution finds no change; the solution is that of the constant given as a field"""
    mu = 70.0
    f, g = Frame("sphere32_L3", solve=False), Frame("sphere32_L3", solve=False)
    f.s.set_field(capi.FIELD_VISCOSITY, 0, None, mu)                             # (untouched cells keep it)
    r = f.s.solve_shear_dependent(to_capi(V.CASES["newtonian_carreau"]), tol=TOL, max_iters=3000, picard_tol=PICARD_TOL, max_picard=MAX_PICARD)
    assert r.converged and len(r.solves) == 1 and r.summaries[0].max_relative_change == 0.0 and r.solves[0].converged
    nx, ny, nz = g.s.field_res
    g.s.set_field(capi.FIELD_VISCOSITY, 0, np.full((nz, ny, nx), np.float32(mu)))
    g.s.assemble()
    info = g.s.solve(TOL, 3000)
    assert system_bytes(f.s) == system_bytes(g.s)
    assert (info.iterations, info.error) == (r.solves[0].iterations, r.solves[0].error) and f.s.solution().tobytes() == g.s.solution().tobytes()
    f.close()
    g.close()
