"""The vector kernels of the single-reduction PCG loops -- k_sr_init<T, CODED>, k_sr_update<T, CODED, S>, k_sr_mixed_residual<CODED, INIT>
(csrc/avs_pcg.hip) -- launched on their own through avs_sr_vector_probe (libavs_probe.so) and compared bit for bit with
tests/pcg_scalar_model.py: element-wise results in T, a thread's own sums in grid-stride order in S, block_sum in double.

The loops launch one workgroup per 256 rows up to 2,048 workgroups: a second grid-stride trip takes more than 524,288 rows, and no
workgroup is ever without rows.  Here g = 1, 2, 3, 8 workgroups meet n = 1 .. 3 x 256 g rows: workgroups without rows, one, two and three
trips, ragged tails.  Every array of a launch lives in one arena with 0xA5 guard bytes between the arrays, and the whole arena is
compared: `done` on entry must leave every array and the partial sums as they are, and the step folded into k_sr_update (workgroup 0
stores state `out` while every workgroup computes from state `in`) must leave `in` untouched and make `out` the model's image.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import pcg_scalar_model as M
from adaptiveviscositysolver_amd import capi
from pcg_scalar_model import SCALARS, f32, f64

pytestmark = pytest.mark.gpu

# vector type, scalar type of k_sr_update, flags
TYPES = {"f64": (f64, f64, 0), "f32": (f32, f32, capi.VECTOR_PROBE_F32), "f32_ds": (f32, f64, capi.VECTOR_PROBE_DS)}


def sizes(g):
    T = 256 * g
    return sorted({1, 255, 256, 257, T - 1, T, T + 1, 2 * T + 5, 3 * T})


def image(**over):
    sc = np.zeros(1, SCALARS)[0]
    sc["rho"], sc["pAp"], sc["rr"], sc["alpha"], sc["beta"], sc["threshold"], sc["rhs_norm2"] = 1.7, 4.2, 0.5, 0.37, 0.61, 1e-3, 3.0
    sc["red"][:] = (2.25, 8.5, 7.75, 6.125)
    sc["iter"], sc["done"], sc["fault"], sc["cancelled"], sc["rho_alt"] = 6, 0, 0, 0, 2.3
    for k, v in over.items():
        sc[k] = v
    return sc


class Vectors:
    def __init__(self, lib, tname, g, n, seed):
        T, S, flags = TYPES[tname]
        self.lib, self.T, self.S, self.flags, self.g, self.n = lib, T, S, flags, g, n
        self.ar = ar = M.DeviceArena([("b", f64, n), ("t64", f64, n)] + [(name, T, n) for name in ("x", "r", "p", "s", "u", "w", "invd")] +
                                     [("table", T, 8), ("dcode", np.uint16, n), ("partial", f64, 3 * g), ("in", np.uint8, SCALARS.itemsize),
                                      ("out", np.uint8, SCALARS.itemsize)])
        rng = np.random.default_rng(seed)
        v = ar.views(ar.host)
        for name in ("b", "t64", "x", "r", "p", "s", "u", "w"):
            a = rng.standard_normal(n) * 10.0 ** rng.integers(-1, 2, n)
            a[rng.random(n) < 0.03] = 0.0
            v[name][:] = a.astype(T).astype(v[name].dtype) if name == "b" else a.astype(v[name].dtype)      # (float loops: b holds float values)
        v["invd"][:] = (0.25 + 2.0 * rng.random(n)).astype(T)
        v["table"][:] = np.array([1.0, 0.5, 0.37, 2.25, 1.0 / 3.0, 0.8, 1.7, 1.0], T)
        v["dcode"][:] = rng.integers(0, 8, n)
        v["partial"][:] = 12345.0

    def start(self, sc_in):
        buf = self.ar.host.copy()
        self.ar.views(buf)["in"][:] = np.frombuffer(sc_in.tobytes(), np.uint8)
        return buf

    def launch(self, start, kernel, coded, step=0, out="in", mixed=False):
        ar = self.ar
        flags = (0 if mixed else self.flags) | (capi.VECTOR_PROBE_CODED if coded else 0)
        return ar.run(start, lambda: capi.check(self.lib.avs_sr_vector_probe(
            kernel, flags, self.g, self.n, ar.ptr("b"), ar.ptr("x"), ar.ptr("r"), ar.ptr("p"), ar.ptr("s"), ar.ptr("u"),
            ar.ptr("t64" if mixed else "w"), ar.ptr("table" if coded else "invd"), ar.ptr("dcode"), ar.ptr("in"), ar.ptr(out), SCALARS.itemsize,
            step, ar.ptr("partial"), C.c_void_p(torch.cuda.current_stream().cuda_stream))))

    def same(self, got, want, what):
        if not np.array_equal(got, want):
            o = self.ar.off["out"][0]
            raise AssertionError((what, "differs in", self.ar.which(got, want), "out got", got[o:o + 112].view(SCALARS)[0], "want",
                                  want[o:o + 112].view(SCALARS)[0]))


@pytest.fixture(scope="module")
def lib(built_lib):
    return capi.load_probe()


def idiag(v, coded):
    return v["table"][v["dcode"]] if coded else v["invd"]


@pytest.mark.parametrize("g", [1, 2, 3, 8])
@pytest.mark.parametrize("tname", ["f64", "f32"])
def test_sr_init(lib, tname, g):
    for n in sizes(g):
        vec = Vectors(lib, tname, g, n, 100 * g + n)
        for coded in ((False, True) if tname == "f32" else (False,)):
            start = vec.start(image())
            want = start.copy()
            v = vec.ar.views(want)
            M.sr_init(vec.T, g, v["b"], v["w"], idiag(v, coded), v["r"], v["u"], v["partial"])
            vec.same(vec.launch(start, capi.SR_PROBE_INIT, coded), want, ("init", tname, g, n, coded))
            # the three sums are three different sums, in the order OP_SR_INIT reads them: b.b, r.u, r.r
            p = v["partial"]
            if n > 8:
                assert len({float(p[:g].sum()), float(p[g:2 * g].sum()), float(p[2 * g:].sum())}) == 3
            assert p[:g].sum() >= 0 and p[2 * g:].sum() >= 0


# states of `in` for k_sr_update: (name, step, image) -- with step the sums in `in` converge (r.r below the threshold), go on, or `in` is done
def update_states():
    go = dict(threshold=1e-3)
    return [("as_is", 0, image()), ("as_is_done1", 0, image(done=1)), ("as_is_done3", 0, image(done=3)),
            ("step_goes_on", 1, image(**go)), ("step_converges", 1, image(threshold=1e3)),
            ("step_at_threshold", 1, image(threshold=8.5)),                       # r.r == threshold: the test is <
            ("step_done1", 1, image(done=1, **go)), ("step_done2", 1, image(done=2, **go)), ("step_done3", 1, image(done=3, **go))]


@pytest.mark.parametrize("g", [1, 2, 3, 8])
@pytest.mark.parametrize("tname", list(TYPES))
def test_sr_update(lib, tname, g):
    for n in sizes(g):
        vec = Vectors(lib, tname, g, n, 200 * g + n)
        for coded in ((False, True) if tname != "f64" else (False,)):
            for name, step, sc_in in update_states():
                start = vec.start(sc_in)
                want = start.copy()
                v = vec.ar.views(want)
                rec_in = v["in"].view(SCALARS)[0]
                M.sr_update(vec.T, vec.S, g, v["x"], v["r"], v["p"], v["s"], v["u"], v["w"], idiag(v, coded), rec_in,
                            v["out"].view(SCALARS), step, v["partial"])
                what = ("update", tname, g, n, coded, name)
                vec.same(vec.launch(start, capi.SR_PROBE_UPDATE, coded, step, "out" if step else "in"), want, what)
                # the cases are what they are meant to be
                assert rec_in.tobytes() == sc_in.tobytes()
                out = v["out"].view(SCALARS)[0]
                moved = not np.array_equal(v["x"], vec.ar.views(start)["x"])
                if not step:
                    assert np.all(v["out"] == 0xA5) and moved == (sc_in["done"] == 0), what
                else:
                    goes_on = name in ("step_goes_on", "step_at_threshold")
                    assert out["done"] == (0 if goes_on else 1 if name == "step_converges" else sc_in["done"]), what
                    assert out["iter"] == (7 if goes_on else 6) and moved == goes_on, what
                    assert (out["rho"] == 2.25) == goes_on, what


@pytest.mark.parametrize("g", [1, 2, 3, 8])
def test_sr_mixed_residual(lib, g):
    for n in sizes(g):
        vec = Vectors(lib, "f32_ds", g, n, 300 * g + n)
        for coded in (False, True):
            for init in (False, True):
                for done in (0, 1, 2, 3):
                    start = vec.start(image(done=done))
                    want = start.copy()
                    v = vec.ar.views(want)
                    M.sr_mixed_residual(g, v["b"], v["t64"], idiag(v, coded), v["r"], v["u"], v["partial"], v["in"].view(SCALARS)[0], init)
                    kernel = capi.SR_PROBE_MIXED_RESIDUAL_INIT if init else capi.SR_PROBE_MIXED_RESIDUAL
                    what = ("mixed residual", g, n, coded, init, done)
                    vec.same(vec.launch(start, kernel, coded, mixed=True), want, what)
                    # the plain form under done != 0 leaves every array and the partial sums as they are; the INIT form does not read it
                    assert np.array_equal(want, start) == (not init and done != 0), what
