"""The lossless SpMV storage forms on arbitrary CSR, at the edges of their thresholds (tests/csr_edges.py).

Products: avs_spmv_csr_form (libavs_probe.so) builds the form avs_pcg_csr would build for a case under each AVS_* environment and
multiplies with the kernel the solve launches on it.  The form must be the one the restated rule predicts, y must equal the C oracle's
row sums bit for bit (NaN where the oracle gives NaN), the folded x.y of the fused-dot launch must be within a summation bound of the
exact sum and identical over two launches; the non-temporal (no cache hint) instantiation and the float kernel are run as well.
Solves: symmetric, diagonally dominant versions of the cases through seam A (avs_pcg_csr) against the oracle's PCG.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import csr_edges as E
from adaptiveviscositysolver_amd import capi, pcg_csr
from oracle import oracle as O
from util import float_row_sums, rel_l2

pytestmark = pytest.mark.gpu

AVS_KEYS = ("AVS_VALUE_INDEX", "AVS_VALUE_PACK", "AVS_COLUMN_WINDOWS", "AVS_TILE_TABLES", "AVS_CG_RESIDENT")


def _set_env(monkeypatch, env):
    for k in AVS_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


class _Edge:
    """a case, its x and the oracle's product, and the arrays on the device (built once per module)"""

    def __init__(self, case, dev):
        self.case = case
        rng = np.random.default_rng(len(case.name) * 7919 + case.n)
        self.x = rng.standard_normal(case.n) * 10.0 ** rng.integers(-2, 3, case.n)
        self.want = O.spmv_csr(case.row_ptr.astype(np.int64), case.col, case.val, self.x)
        t = lambda a: torch.from_numpy(a).to(dev)
        self.d = [t(case.row_ptr), t(case.col), t(case.val), t(self.x)]


@pytest.fixture(scope="module")
def edges(built_lib):
    dev = torch.device("cuda:0")
    cases = {c.name: c for c in E.cases()}
    made = {}

    def get(name):
        if name not in made:
            made.clear()          # one case on the device at a time
            made[name] = _Edge(cases[name], dev)
        return made[name]
    return get


def _form_product(lib, e, flags):
    n = e.case.n
    y = torch.full((n,), float("nan"), dtype=torch.float64, device=e.d[0].device)
    fmt = capi.MatrixFormat()
    dot = C.c_double(float("nan"))
    d_rp, d_col, d_val, d_x = e.d
    capi.check(lib.avs_spmv_csr_form(n, d_rp.data_ptr(), d_col.data_ptr(), d_val.data_ptr(), d_x.data_ptr(), y.data_ptr(), flags,
                                     C.byref(dot), C.byref(fmt), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return y.cpu().numpy(), dot.value, {f: getattr(fmt, f) for f in E.FMT_FIELDS}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_rows(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN rows differ", np.nonzero(np.isnan(got) != nan)[0][:8])
    bad = np.nonzero(_bits(got[~nan]) != _bits(want[~nan]))[0]
    assert len(bad) == 0, (what, f"{len(bad)} rows differ", np.nonzero(~nan)[0][bad[:8]], got[~nan][bad[:4]], want[~nan][bad[:4]])


def _assert_dot(dot, x, y, what):
    terms = x * y
    if not np.all(np.isfinite(terms)):
        return
    exact = math.fsum(terms.tolist())
    bound = (len(x) / 64 + 16) * 2.0 ** -53 * math.fsum(np.abs(terms).tolist())
    assert abs(dot - exact) <= bound, (what, dot, exact, bound)


@pytest.mark.parametrize("name", E.NAMES)
def test_products_in_every_form(name, edges, monkeypatch):
    e = edges(name)
    c = e.case
    lib = capi.load_probe()
    for env_name, env in E.ENVS.items():
        _set_env(monkeypatch, env)
        want_fmt = E.expected_format(c.row_ptr, c.col, c.val, env)
        what = (name, env_name, E.instantiation(want_fmt, c.row_ptr, c.val))
        y, _, fmt = _form_product(lib, e, 0)
        assert fmt == want_fmt, (what, fmt)
        _assert_rows(y, e.want, what + ("plain",))
        y1, dot1, fmt = _form_product(lib, e, capi.SPMV_FORM_FUSED_DOT)
        assert fmt == want_fmt, (what, fmt)
        _assert_rows(y1, e.want, what + ("fused",))
        _assert_dot(dot1, e.x, e.want, what)
        y2, dot2, _ = _form_product(lib, e, capi.SPMV_FORM_FUSED_DOT)
        assert np.array_equal(_bits(y2), _bits(y1)) and _bits([dot2]) == _bits([dot1]), (what, "second launch differs", dot1, dot2)
        if env_name == "default":
            # the instantiation with non-temporal matrix loads (KEEPW = false): same products, same fold
            y3, dot3, _ = _form_product(lib, e, capi.SPMV_FORM_FUSED_DOT | capi.SPMV_FORM_NO_CACHE_HINT)
            assert np.array_equal(_bits(y3), _bits(y1)) and _bits([dot3]) == _bits([dot1]), (what, "no cache hint", dot1, dot3)
            if c.f32:
                want32 = float_row_sums(c.row_ptr, c.col, c.val, e.x)
                for flags in (capi.SPMV_FORM_F32, capi.SPMV_FORM_F32 | capi.SPMV_FORM_FUSED_DOT):
                    yf, _, _ = _form_product(lib, e, flags)
                    assert np.array_equal(yf.astype(np.float32).view(np.int32), want32.view(np.int32)), (what, "float", flags)


# forms forced by the environment under the launch-per-phase loop: every value-indexed one leaves one partial of x.y per 64-row wave
# in the same slots (k_spmv_vi2), the vector kernels differ in where 1 / diag comes from only -- so iterates agree bit for bit
FORCED = [{}, {"AVS_VALUE_PACK": "0"}, {"AVS_COLUMN_WINDOWS": "0"}, {"AVS_VALUE_PACK": "0", "AVS_COLUMN_WINDOWS": "0"},
          {"AVS_TILE_TABLES": "0"}, {"AVS_TILE_TABLES": "0", "AVS_VALUE_PACK": "0"}]


@pytest.mark.parametrize("name", E.SPD_NAMES)
def test_seam_a_solves(name, edges, monkeypatch):
    c = edges(name).case
    rp, col, val, b = E.spd_version(c, seed=c.n)
    n = c.n
    tol, max_iters = 1e-10, 2000
    x0 = np.zeros(n)
    xo, io = O.pcg_csr(rp.astype(np.int64), col, val, b, x0, tol, max_iters)
    bnorm = math.sqrt(math.fsum((b * b).tolist()))
    runs = [("default", {})] + [("loop " + ",".join(f"{k}={v}" for k, v in f.items()), {**f, "AVS_CG_RESIDENT": "0"}) for f in FORCED]
    coded = {}
    for label, env in runs:
        _set_env(monkeypatch, env)
        x, info = pcg_csr(rp, col, val, b, x0, tol, max_iters)
        what = (name, label)
        assert info.converged == 1, what
        assert abs(info.iterations - io.iterations) <= 3, (what, info.iterations, io.iterations)
        assert rel_l2(x, xo) < 1e-8, (what, rel_l2(x, xo))
        r = b - O.spmv_csr(rp.astype(np.int64), col, val, x)
        assert math.sqrt(math.fsum((r * r).tolist())) <= 10 * tol * bnorm, what
        fmt = E.expected_format(rp, col, val, env)
        if label == "default":
            # the CU-resident loop takes the packed single dictionary of <= 1023 values (resident_prepare)
            resident_form = fmt["column_bits"] > 0 and fmt["value_table_size"] <= 1023
            assert info.resident == (1 if resident_form else 0), (what, E.instantiation(fmt), info.resident)
        else:
            assert info.resident == 0, what
            if fmt["value_table_size"] > 0:
                coded.setdefault(E.instantiation(fmt, rp, val), (label, info.iterations, _bits(x)))
    forms = list(coded.values())
    for label, iters, xb in forms[1:]:
        assert iters == forms[0][1] and np.array_equal(xb, forms[0][2]), (name, forms[0][0], label, iters, forms[0][1])
