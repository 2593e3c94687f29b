"""avs_check_csr / avs_check_system: the rules a CSR system has to keep for avs_pcg_csr, evaluated on the device (avs_csr_check.hip).

Reference: tests/csr_check_model.py (NumPy; pinned by test_csr_check_model.py).  The device report must equal the model's report exactly --
every count, `evaluated`, `passed`, `first_*` and the three measurements bit for bit: no tolerance anywhere in the comparison.  Corrupt
systems are only ever read by the checker: none is handed to a solver."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

from adaptiveviscositysolver_amd import DevicePrepass, ViscositySolve, capi, check_csr, pcg_csr, scenes

import csr_check_cases as cc
import csr_check_model as m

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def as_model(rep):
    """capi.CsrCheck -> the dict of csr_check_model"""
    d = {f: getattr(rep, f) for f in m.FIELDS}
    d["violations"] = tuple(int(v) for v in rep.violations)
    return d


def same(got, want):
    """equal field by field, the doubles by their bits"""
    bits = lambda v: struct.pack("<d", v)
    return all(got[f] == want[f] for f in m.FIELDS) and all(bits(got[f]) == bits(want[f]) for f in ("max_abs_value", "max_abs_asymmetry"))


def ptr(a):
    if a is None:
        return None
    return a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data


def call(n, nnz, rp, col, val, b, x, what, tol, where, rep=None, device=0):
    """-> status, report, message"""
    lib = capi.load()
    rep = capi.CsrCheck() if rep is None else rep
    st = lib.avs_check_csr(n, nnz, ptr(rp), ptr(col), ptr(val), ptr(b), ptr(x), what, tol, where, device, None, C.byref(rep))
    return st, rep, (lib.avs_last_error().decode() if st != capi.OK else "")


def on_device(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


def agree(s, arrays, where, tol=None):
    """the device report equals the model's for every `what`, with b and x and (where the VALUES bit makes them count) without; a
    second call gives the same report"""
    tol = s.tol if tol is None else tol
    rp, col, val, b, x = arrays
    with_vectors = m.Analysis(s.row_ptr, s.col, s.val, s.b, s.x)
    without = m.Analysis(s.row_ptr, s.col, s.val)
    for what in m.WHATS:
        for analysis, bb, xx in ((with_vectors, b, x),) + (((without, None, None),) if what & m.VALUES else ()):
            want = analysis.report(what, tol)
            st, rep, err = call(s.n, s.nnz, rp, col, val, bb, xx, what, tol, where)
            assert st == capi.OK, err
            got = as_model(rep)
            assert same(got, want), (s.name, what, bb is not None, got, want)
            st, rep, err = call(s.n, s.nnz, rp, col, val, bb, xx, what, tol, where)
            assert st == capi.OK and same(as_model(rep), got), (s.name, what, "second call")
    return with_vectors.report(m.ALL, tol)


# ---- 1. every case, host and device arrays -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", cc.all_names())
def test_report_equals_the_model(built_lib, name, where):
    s = cc.system(name)
    arrays = (s.row_ptr, s.col, s.val, s.b, s.x)
    if where == "device":
        arrays = tuple(on_device(a) for a in arrays)
        torch.cuda.synchronize()
    r = agree(s, arrays, capi.MEM_DEVICE if where == "device" else capi.MEM_HOST)
    if name in cc.CLEAN_NAMES:
        assert r["passed"] == 1 and r["asymmetric_entries"] == 0 and r["max_abs_asymmetry"] == 0.0
    elif s.expect is not None:
        assert r["violations"] == cc.expected_violations(s)


# ---- 2. the caller's arrays: read in place, inside larger buffers whose other entries would all violate, and left as they are ------------
SLICED = ["tri_65", "blocks", "spd_n_513", "raw_unsorted_repeated", "raw_specials", "several", "tri_65_rp_over_nnz", "tri_65_rp_last_long",
          "blocks_rp_int32_max", "tri_65_col_int32_max_last", "tri_1_diag_removed_0", "n_0"]


@pytest.mark.parametrize("name", SLICED)
def test_device_arrays_are_interior_slices_and_stay_untouched(built_lib, name):
    s = cc.system(name)
    pad = {"rp": (3, 5), "col": (1, 7), "val": (1, 3), "b": (3, 1), "x": (1, 2)}   # entries before / behind: 4- and 8-byte starts only

    def framed(a, key, poison, dtype):
        if a is None:
            a = np.zeros(s.n, dtype)
        before, behind = pad[key]
        return torch.from_numpy(np.concatenate([np.full(before, poison, dtype), a, np.full(behind, poison, dtype)])).to(DEV), before

    bufs = {"rp": framed(s.row_ptr, "rp", -1, np.int32), "col": framed(s.col, "col", cc.INT32_MIN, np.int32), "val": framed(s.val, "val", np.nan, np.float64),
            "b": framed(s.b, "b", np.nan, np.float64), "x": framed(s.x, "x", np.nan, np.float64)}
    lens = {"rp": s.n + 1, "col": s.nnz, "val": s.nnz, "b": s.n, "x": s.n}
    views = {k: buf[off:off + lens[k]] for k, (buf, off) in bufs.items()}
    copies = {k: buf.clone() for k, (buf, _) in bufs.items()}
    torch.cuda.synchronize()
    arrays = (views["rp"], views["col"], views["val"], None if s.b is None else views["b"], None if s.x is None else views["x"])
    agree(s, arrays, capi.MEM_DEVICE)
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert buf.cpu().numpy().tobytes() == copies[k].cpu().numpy().tobytes(), k


def test_nothing_at_or_behind_the_stated_nnz_is_read(built_lib):
    """nnz is the caller's statement: with three entries fewer stated than row_ptr[n] names, rule 0 reports index n and nothing else runs;
    the entries behind the stated length are poison here"""
    s = cc.system("tri_65")
    nnz = s.nnz - 3
    col, val = s.col.copy(), s.val.copy()
    col[nnz:], val[nnz:] = cc.INT32_MAX, np.nan
    want = m.check(s.row_ptr, col, val, s.b, s.x, nnz=nnz)
    assert want["violations"] == (2, 0, 0, 0, 0, 0, 0, 0) and want["evaluated"] == 1   # row_ptr[n - 1] and row_ptr[n] exceed the stated nnz
    for where, arrays in ((capi.MEM_HOST, (s.row_ptr, col, val, s.b, s.x)), (capi.MEM_DEVICE, tuple(on_device(a) for a in (s.row_ptr, col, val, s.b, s.x)))):
        torch.cuda.synchronize()
        st, rep, err = call(s.n, nnz, *arrays, m.ALL, 0.0, where)
        assert st == capi.OK and same(as_model(rep), want), (err, as_model(rep), want)


# ---- 3. the report struct ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [8, 16, 32, 96, 120, 136])
def test_only_struct_size_bytes_are_written(built_lib, size):
    s = cc.system("several")
    full = capi.CsrCheck()
    assert call(s.n, s.nnz, s.row_ptr, s.col, s.val, s.b, s.x, m.ALL, 0.0, capi.MEM_HOST, full)[0] == capi.OK and full.passed == 0
    rep = capi.CsrCheck()
    C.memset(C.byref(rep), 0x5a, C.sizeof(rep))
    rep.struct_size = size
    st, _, err = call(s.n, s.nnz, s.row_ptr, s.col, s.val, s.b, s.x, m.ALL, 0.0, capi.MEM_HOST, rep)
    assert st == capi.OK, err
    got, want = bytes(rep), bytes(full)
    assert rep.struct_size == size and got[4:size] == want[4:size] and got[size:] == b"\x5a" * (C.sizeof(rep) - size)


def test_argument_errors_have_messages(built_lib):
    s = cc.system("tri_5")
    good = dict(n=s.n, nnz=s.nnz, rp=s.row_ptr, col=s.col, val=s.val, b=s.b, x=s.x, what=m.ALL, tol=0.0, where=capi.MEM_HOST)
    assert call(**good)[0] == capi.OK
    small, absurd = capi.CsrCheck(), capi.CsrCheck()
    small.struct_size, absurd.struct_size = 4, 5000
    bad = [dict(what=16), dict(what=0x80000000), dict(what=m.ALL | 32), dict(rep=small), dict(rep=absurd), dict(n=-1), dict(nnz=-1), dict(n=2**31),
           dict(nnz=2**31), dict(rp=None), dict(col=None), dict(val=None), dict(tol=-1e-300), dict(tol=float("nan")), dict(tol=float("inf")),
           dict(device=-1), dict(device=torch.cuda.device_count()), dict(where=7)]
    for change in bad:
        st, _, err = call(**{**good, **change})
        assert st == capi.EINVAL and err, (change, st, err)
    lib = capi.load()
    st = lib.avs_check_csr(s.n, s.nnz, ptr(s.row_ptr), ptr(s.col), ptr(s.val), None, None, m.ALL, 0.0, capi.MEM_HOST, 0, None, None)   # no report
    assert st == capi.EINVAL and lib.avs_last_error()
    # col and val may be missing when there is nothing to read
    st, rep, err = call(1, 0, np.zeros(2, np.int32), None, None, None, None, m.ALL, 0.0, capi.MEM_HOST)
    assert st == capi.OK and rep.passed == 0 and rep.violations[m.DIAGONAL_RULE] == 1 and rep.empty_rows == 1, err
    assert call(**good)[0] == capi.OK


# ---- 4. the system a context assembled -----------------------------------------------------------------------------------------------------
SCENES = {"sphere16_L2": lambda: scenes.sphere(16, 2), "beam32_L3": lambda: scenes.fat_beam(32, 3), "beam32_L3_wall": lambda: scenes.fat_beam(32, 3, wall=True),
          "beam32_L4_variable": lambda: scenes.fat_beam(32, 4, variable_viscosity=True)}


def assembled(name, before_assemble=None):
    sc = scenes.to_device(SCENES[name](), torch.device(DEV))
    pp = DevicePrepass(sc.res, sc.dx, sc.levels, device=0)
    info = pp.run(sc.liquid, sc.solid)
    s = ViscositySolve(sc.res, sc.dx, sc.dt, info.levels, device=0)
    pp.apply(s)
    s.set_scene_fields(sc)
    if before_assemble:
        before_assemble(s)
    s.assemble()
    return pp, s


@pytest.mark.parametrize("name", list(SCENES))
def test_check_system_on_assembled_scenes(built_lib, name):
    lib = capi.load()

    def not_yet(s):
        rep = capi.CsrCheck()
        assert lib.avs_check_system(s.h, m.ALL, 0.0, C.byref(rep)) == capi.ESTATE and lib.avs_last_error()

    pp, s = assembled(name, not_yet)
    rp, col, val, rhs = s.csr()
    a = m.Analysis(rp, col, val, rhs, s.initial_guess())
    for what in m.WHATS:
        for tol in (0.0, 1e-12 * a.max_abs_value):
            want = a.report(what, tol)
            rep = capi.CsrCheck()
            capi.check(lib.avs_check_system(s.h, what, tol, C.byref(rep)))
            assert same(as_model(rep), want), (what, tol, as_model(rep), want)
            capi.check(lib.avs_check_system(s.h, what, tol, C.byref(rep)))
            assert same(as_model(rep), want), (what, tol, "second call")
    r = s.check_system(symmetry_tolerance=1e-12 * a.max_abs_value)
    print(name, "n", len(rhs), "nnz", len(col), "asymmetric_entries", r.asymmetric_entries, "max_abs_asymmetry", r.max_abs_asymmetry, "max_abs_value",
          r.max_abs_value, "ratio", r.max_abs_asymmetry / r.max_abs_value)
    assert r.evaluated == 255 and r.violations[:7] == (0,) * 7
    assert r.max_abs_asymmetry <= 1e-12 * r.max_abs_value
    assert r.passed and r.violations[7] == 0 and r.first is None
    # the bad arguments of this entry
    rep = capi.CsrCheck()
    for what, tol in ((16, 0.0), (m.ALL, -1.0), (m.ALL, float("nan"))):
        assert lib.avs_check_system(s.h, what, tol, C.byref(rep)) == capi.EINVAL and lib.avs_last_error()
    assert lib.avs_check_system(s.h, m.ALL, 0.0, None) == capi.EINVAL and lib.avs_check_system(None, m.ALL, 0.0, C.byref(rep)) == capi.EINVAL
    s.close()
    pp.close()


def test_a_checked_context_solves_as_an_unchecked_one(built_lib):
    def frame(checked):
        pp, s = assembled("beam32_L3")
        if checked:
            assert s.check_system(symmetry_tolerance=1e-9).passed
            assert s.check_system(what=capi.CSR_CHECK_ORDER | capi.CSR_CHECK_DIAGONAL).passed
        sol = s.solve(1e-8, 3000)
        if checked:
            assert s.check_system(symmetry_tolerance=1e-9).passed
        out = [s.csr(), s.initial_guess(), s.solution(), (sol.iterations, sol.converged, sol.error)]
        s.close()
        pp.close()
        return out

    (csr_a, g_a, x_a, i_a), (csr_b, g_b, x_b, i_b) = frame(False), frame(True)
    assert i_a == i_b and i_a[1] == 1
    assert all(a.tobytes() == b.tobytes() for a, b in zip(csr_a, csr_b))
    assert g_a.tobytes() == g_b.tobytes() and x_a.tobytes() == x_b.tobytes() and np.abs(x_a).max() > 0


# ---- 5. what the checker accepts is what the solver is defined for -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tri_1", "tri_65", "blocks", "arrow", "spd_n_513", "spd_long_row"])
def test_a_system_that_passes_is_solved(built_lib, name):
    s = cc.system(name)
    r = check_csr(s.row_ptr, s.col, s.val, s.b, s.x)
    assert r.passed and r.evaluated == 255 and r.first is None and r.asymmetric_entries == 0
    x, info = pcg_csr(s.row_ptr, s.col, s.val, s.b, np.zeros(s.n), tol=1e-10, max_iters=500)
    assert info.converged == 1
    rows = np.repeat(np.arange(s.n), np.diff(s.row_ptr))
    res = s.b - np.bincount(rows, weights=s.val * x[s.col], minlength=s.n)
    assert np.linalg.norm(res) <= 1e-8 * np.linalg.norm(s.b)
