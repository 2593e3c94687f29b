"""The two vector kernels of the launch-per-phase PCG loops (k_update_r / k_update_xp<T, S, ...>: csrc/avs_pcg.hip) against a NumPy model of their arithmetic, bit for bit, through avs_vector_update_probe (libavs_probe.so).

The kernels start their first D grid-stride trips' loads before the scalar prologue (the fold of the partial sums, alpha / beta); the
shapes below put 0, 1, D, D + 1 and D + 2 trips into one launch, leave workgroups without work and end in odd tails.  The model was
written against, and passed on, the kernels as they were BEFORE that change (one load chain behind the other): it describes what the
loops computed all along, not how the new code is laid out.

Element-wise results: NumPy rounds once per operation, as the -ffp-contract=off build does.  Sums, in the kernels' order: a thread's own
terms in trip order and row order (float32 accumulators in the float kernels), the 64 lanes of a wave by the shuffle tree of wave_sum
(lane i += lane i + o for o = 32, 16, .. 1; lane 0 holds the sum -- the vector kernels' block_sum uses this tree, the DPP tree of
wave_sum_dpp belongs to the SpMV kernels), the four waves as ((w0 + w1) + w2) + w3, the partial sums of a previous launch by thread t
adding partial[t + 256 j] in ascending j and the same block sum behind it.

The product path (avs_pcg_csr on host arrays, CU-resident loop off) is run on two systems large enough for several trips per thread.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from adaptiveviscositysolver_amd import capi, pcg_csr
from pcg_scalar_model import SCALARS, block_sum        # (the record of PcgScalars, wave_sum and the 256-thread block_sum live there)
from util import rel_l2

pytestmark = pytest.mark.gpu

D = 1                      # kVecAhead of csrc/avs_pcg.hip: trips whose loads are issued before the prologue
BLOCK = 256
NB_MAX = 4096
TYPES = {"f64": (np.float64, 2, 0), "f32": (np.float32, 4, capi.VECTOR_PROBE_F32), "f32_ds": (np.float32, 4, capi.VECTOR_PROBE_DS)}
GUARD = 64                 # bytes of 0xA5 between two arrays of the arena: a store beyond an array's end shows up in the comparison


def shapes(R, g):
    T = BLOCK * g
    return [1, R - 1, R, R + 1, R * T - 1, R * T, R * T + 1, R * T * D + R * (T // 2) + 1, R * T * (D + 1) + 3, R * T * (D + 2)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------------
def fold(a, count):
    """what every workgroup makes of `count` partial sums of the launch before"""
    acc = np.zeros(BLOCK)
    for j in range(0, count, BLOCK):
        c = a[j:min(j + BLOCK, count)]
        acc[:len(c)] += c
    return block_sum(acc[None, :])[0]


class Case:
    def __init__(self, tname, g, n, coded, fused, parity, nb):
        self.tname, self.g, self.n, self.coded, self.fused, self.parity, self.nb = tname, g, n, coded, fused, parity, nb
        self.ft, self.R, self.tflag = TYPES[tname]
        self.ds = tname == "f32_ds"
        self.f32 = tname == "f32"


def thread_sums(c, rn_of, id_of):
    """per-thread sums of rn^2 and rn (id rn) over the grid-stride trips (R rows each, in row order), thread 0 then takes the tail rows"""
    T, R, n, ft = BLOCK * c.g, c.R, c.n, c.ft
    nR = n // R
    rr, rz = np.zeros(T, ft), np.zeros(T, ft)
    for j0 in range(0, nR, T):
        m = min(nR, j0 + T) - j0
        a = rn_of[R * j0:R * (j0 + m)].reshape(m, R)
        d = id_of[R * j0:R * (j0 + m)].reshape(m, R)
        for q in range(R):
            rr[:m] += a[:, q] * a[:, q]
            rz[:m] += a[:, q] * (d[:, q] * a[:, q])
    for i in range(nR * R, n):
        rr[0] += rn_of[i] * rn_of[i]
        rz[0] += rn_of[i] * (id_of[i] * rn_of[i])
    return rr, rz


def model_update_r(c, sc, A):
    if sc["done"] != 0:
        if c.fused and sc["done"] == 2:
            sc["done"] = 1
        return
    f32 = np.float32
    rho = sc["rho_alt"] if c.parity else sc["rho"]
    if c.fused:
        pap = fold(A["spart"], c.nb)
        sc["red"][0] = pap
        if c.f32:
            alpha = f32(rho) / f32(pap)
            sc["pAp"], sc["alpha"] = np.float64(f32(pap)), np.float64(alpha)
        else:
            alpha_d = rho / pap
            sc["pAp"], sc["alpha"] = pap, alpha_d
            alpha = f32(alpha_d) if c.ds else alpha_d
    elif c.f32:
        alpha = f32(rho) / f32(sc["pAp"])
        sc["alpha"] = np.float64(alpha)
    else:
        alpha = f32(sc["alpha"]) if c.ds else sc["alpha"]
    r, t = A["r"], A["t"]
    r[:] = r - alpha * t
    assert r.dtype == c.ft
    rr, rz = thread_sums(c, r, A["id"])
    g = c.g
    A["vpart"][:g] = block_sum(rr.astype(np.float64).reshape(g, BLOCK))
    A["vpart"][g:2 * g] = block_sum(rz.astype(np.float64).reshape(g, BLOCK))


def model_update_xp(c, sc, A):
    done = int(sc["done"])
    if done in (1, 3):
        return
    f32 = np.float32
    alpha = sc["alpha"] if c.ft is np.float64 else f32(sc["alpha"])
    fused = c.fused or c.ft is np.float32          # (the float loops have the fused form only)
    beta = c.ft(0) if fused else sc["beta"]
    if fused and done == 0:
        g = c.g
        rr, rz = fold(A["vpart"], g), fold(A["vpart"][g:], g)
        old = sc["rho_alt"] if c.parity else sc["rho"]
        if c.f32:
            rr, rz, old = f32(rr), f32(rz), f32(old)
            conv = rr < f32(sc["threshold"])
        else:
            conv = rr < sc["threshold"]
        if conv:
            done = 2
        else:
            beta = f32(rz / old) if c.ds else rz / old
        sc["red"][0], sc["red"][1], sc["rr"] = rr, rz, rr
        if conv:
            sc["done"] = 2
            if c.ds and c.parity:
                sc["rho"] = old
        else:
            sc["rho" if c.parity else "rho_alt"] = rz
            sc["beta"] = rz / old
            sc["iter"] += 1
    x, p = A["x"], A["p"]
    if done == 2:
        x[:] = x + alpha * p
        return
    xn = x + alpha * p
    p[:] = A["id"] * A["r"] + beta * p
    x[:] = xn
    assert x.dtype == c.ft and p.dtype == c.ft


# ---------------------------------------------------------------------------------------------------------------------------------------
# the arena: every array of a launch in one buffer (one copy in, one copy out per launch), guards between them
# ---------------------------------------------------------------------------------------------------------------------------------------
class Arena:
    def __init__(self, tname, g, n, seed):
        ft, R, _ = TYPES[tname]
        self.ft, self.n, self.g = ft, n, g
        rng = np.random.default_rng(seed)
        fields = [("x", ft, n), ("p", ft, n), ("r", ft, n), ("t", ft, n), ("invd", ft, n), ("table", ft, 8), ("dcode", np.uint16, n),
                  ("spart", np.float64, NB_MAX), ("vpart", np.float64, 2 * g), ("sc", np.uint8, SCALARS.itemsize)]
        self.off, pos = {}, GUARD
        for name, dt, cnt in fields:
            self.off[name] = (pos, np.dtype(dt), cnt)
            pos += -(-(cnt * np.dtype(dt).itemsize) // 64) * 64 + GUARD
        self.host = np.full(pos, 0xA5, np.uint8)
        v = self.views(self.host)
        for name in ("x", "p", "r", "t"):
            a = rng.standard_normal(n) * 10.0 ** rng.integers(-1, 2, n)
            a[rng.random(n) < 0.03] = 0.0
            v[name][:] = a.astype(ft)
        v["table"][:] = np.array([1.0, 0.5, 0.37, 2.25, 1.0 / 3.0, 0.8, 1.7, 1.0], ft)
        v["dcode"][:] = rng.integers(0, 8, n)
        v["invd"][:] = (0.25 + 2.0 * rng.random(n)).astype(ft)
        sp = 0.2 + rng.random(NB_MAX)                      # p.Ap > 0; a few negative and zero partial sums among them
        sp[rng.random(NB_MAX) < 0.05] *= -0.5
        sp[rng.random(NB_MAX) < 0.02] = 0.0
        sp[0] = 0.9
        v["spart"][:] = sp
        v["vpart"][:] = 12345.0
        self.dev = torch.empty(pos, dtype=torch.uint8, device="cuda:0")
        self.base = self.dev.data_ptr()

    def views(self, buf):
        return {name: buf[o:o + cnt * dt.itemsize].view(dt) for name, (o, dt, cnt) in self.off.items()}

    def ptr(self, name):
        return C.c_void_p(self.base + self.off[name][0])

    def which(self, got, want):
        bad = [name for name, (o, dt, cnt) in self.off.items() if not np.array_equal(got[o:o + cnt * dt.itemsize], want[o:o + cnt * dt.itemsize])]
        return bad or ["guard bytes"]


def scalars_image(done, converge):
    sc = np.zeros((), SCALARS)
    sc["rho"], sc["rho_alt"], sc["pAp"], sc["alpha"], sc["beta"] = 1.7, 2.3, 4.2, 0.37, 0.61
    sc["threshold"] = 1e30 if converge else 1e-30
    sc["rhs_norm2"], sc["rr"], sc["iter"], sc["done"] = 3.0, 0.5, 6, done
    sc["red"][:] = (9.0, 8.0, 7.0, 6.0)
    return sc


def run_case(lib, ar, c, done, converge):
    """the expected arena of a launch pair (model), then the launch pair itself with KEEP on and off"""
    start = ar.host.copy()
    o = ar.off["sc"][0]
    start[o:o + SCALARS.itemsize] = np.frombuffer(scalars_image(done, converge).tobytes(), np.uint8)
    want = start.copy()
    v = ar.views(want)
    sc = want[o:o + SCALARS.itemsize].view(SCALARS)[0]
    v["id"] = v["table"][v["dcode"]] if c.coded else v["invd"]
    model_update_r(c, sc, v)
    model_update_xp(c, sc, v)
    flags0 = c.tflag | (capi.VECTOR_PROBE_CODED if c.coded else 0) | (capi.VECTOR_PROBE_FUSED if c.fused else 0)
    for keep in (0, capi.VECTOR_PROBE_KEEP):
        ar.dev.copy_(torch.from_numpy(start))
        capi.check(lib.avs_vector_update_probe(flags0 | keep, c.g, c.n, c.nb, c.parity, ar.ptr("x"), ar.ptr("p"), ar.ptr("r"), ar.ptr("t"),
                                               ar.ptr("table" if c.coded else "invd"), ar.ptr("dcode"), ar.ptr("spart"), ar.ptr("vpart"),
                                               ar.ptr("sc"), SCALARS.itemsize, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        got = ar.dev.cpu().numpy()
        if not np.array_equal(got, want):
            what = (c.tname, "g", c.g, "n", c.n, "coded", c.coded, "fused", c.fused, "keep", bool(keep), "parity", c.parity, "nb", c.nb,
                    "done", done, "converge", converge)
            gs, ws = got[o:o + SCALARS.itemsize].view(SCALARS)[0], sc
            raise AssertionError((what, "differs in", ar.which(got, want), "scalars got", gs, "want", ws))
    return sc


DONE_CASES = [(0, False), (1, False), (3, False), (2, False), (0, True)]     # (done on entry, threshold above r.r)


@pytest.mark.parametrize("g", [1, 3])
@pytest.mark.parametrize("tname", list(TYPES))
def test_kernels_match_the_model_bit_for_bit(tname, g, built_lib):
    lib = capi.load_probe()
    R = TYPES[tname][1]
    launches = 0
    for n in shapes(R, g):
        ar = Arena(tname, g, n, seed=1000 * g + n)
        for coded in (False, True):
            for done, converge in DONE_CASES:
                for parity in (0, 1):
                    for nb in (1, 255, 256, 257, 768, 4096):
                        sc = run_case(lib, ar, Case(tname, g, n, coded, True, parity, nb), done, converge)
                        launches += 2
                        # the cases are what they are meant to be
                        if done == 0:
                            assert sc["done"] == (2 if converge else 0) and sc["iter"] == (6 if converge else 7)
                        else:
                            assert sc["done"] == (1 if done == 2 else done) and sc["iter"] == 6
                run_case(lib, ar, Case(tname, g, n, coded, False, 0, 0), done, converge)      # the unfused form (float: update_r's)
                launches += 2
    assert launches == 10 * 2 * 5 * (2 * 6 + 1) * 2


# ---------------------------------------------------------------------------------------------------------------------------------------
# through the product path
# ---------------------------------------------------------------------------------------------------------------------------------------
def banded_csr(n, diag, bands):
    """symmetric CSR of a main diagonal and the bands {offset: values of the entries (i, i + offset)}"""
    offs = sorted(bands)
    cols = [np.arange(n) - o for o in reversed(offs)] + [np.arange(n)] + [np.arange(n) + o for o in offs]
    vals = [np.concatenate([np.zeros(o), bands[o]]) for o in reversed(offs)] + [diag] + [np.concatenate([bands[o], np.zeros(o)]) for o in offs]
    col, val = np.stack(cols, 1), np.stack(vals, 1)
    ok = (col >= 0) & (col < n)
    rp = np.concatenate([[0], np.cumsum(ok.sum(1))])
    return rp.astype(np.int32), col[ok].astype(np.int32), val[ok], (diag, bands)


def banded_product(op, x):
    diag, bands = op
    y = diag * x
    for o, e in bands.items():
        y[:-o] += e * x[o:]
        y[o:] += e * x[:-o]
    return y


def numpy_pcg(op, b, tol, max_iters, keep_at):
    """Jacobi-PCG from x = 0 by the recurrence of the loop (Eigen's ConjugateGradient); also x after `keep_at` iterations"""
    invd = 1.0 / op[0]
    x, r = np.zeros_like(b), b.copy()
    thr = tol * tol * float(b @ b)
    p = invd * r
    rho, it, kept = float(r @ p), 0, None
    while it < max_iters:
        t = banded_product(op, p)
        alpha = rho / float(p @ t)
        x += alpha * p
        r -= alpha * t
        if it + 1 == keep_at:
            kept = x.copy()
        if float(r @ r) < thr:
            break
        z = invd * r
        rho_new = float(r @ z)
        p = z + (rho_new / rho) * p
        rho = rho_new
        it += 1
    return x, it, kept


def _system(which):
    if which == "A":      # tridiagonal, all values distinct (but for symmetry): no dictionary, 12 B per non-zero, several trips per thread
        n = 3 * 2 ** 20 + 5
        k = np.arange(n - 1, dtype=np.float64)
        e = -(0.25 + 0.5 * (k + 1.0) / n)
        d = 2.0 + (np.arange(n) + 0.5) / n
        d[:-1] -= e
        d[1:] -= e
        return banded_csr(n, d, {1: e})
    n = 2 ** 20 + 3       # four distinct values: a coded diagonal, matrix and vectors stay in the cache
    d = np.where(np.arange(n) % 2 == 0, 5.0, 5.5)
    return banded_csr(n, d, {1: np.full(n - 1, -1.0), 64: np.full(n - 64, -0.5)})


@pytest.mark.parametrize("which", ["A", "B"])
def test_product_path(which, built_lib, monkeypatch):
    monkeypatch.setenv("AVS_CG_RESIDENT", "0")
    rp, col, val, op = _system(which)
    n = len(rp) - 1
    if which == "A":
        assert len(np.unique(val)) == 2 * n - 1       # (symmetric: every off-diagonal value twice)
    else:
        assert len(np.unique(val)) == 4
    rng = np.random.default_rng(n)
    b = rng.standard_normal(n)
    x0 = np.zeros(n)
    tol = 1e-10
    xo, it_o, x7 = numpy_pcg(op, b, tol, 2000, 7)
    assert 7 < it_o < 32, it_o                      # met inside the first chunk of 32 iterations
    bnorm = math.sqrt(float(b @ b))
    for cap, want in ((7, x7), (2000, xo)):
        x, info = pcg_csr(rp, col, val, b, x0, tol, cap)
        x2, info2 = pcg_csr(rp, col, val, b, x0, tol, cap)
        what = (which, cap, info.iterations, it_o)
        assert info.resident == 0, what
        assert x.tobytes() == x2.tobytes() and info.iterations == info2.iterations and info.error == info2.error, what
        if cap == 7:
            assert info.iterations == 7 and info.converged == 0, what
        else:
            assert info.converged == 1 and abs(info.iterations - it_o) <= 3, what
            r = b - banded_product(op, x)
            assert math.sqrt(float(r @ r)) <= 10 * tol * bnorm, what
        assert rel_l2(x, want) < 1e-8, (what, rel_l2(x, want))
