"""The scalar stages of the PCG loops -- k_reduce, k_reduce_mb, k_reduce_pair, k_scalar (apply_scalar_op), k_mixed_finish<INIT>,
k_sr_mixed_begin, k_sr_mixed_step: csrc/avs_pcg.hip, avs_halo.hpp, avs_pcg_mixed.inl -- launched on their own through
avs_pcg_scalar_probe (libavs_probe.so) and compared bit for bit with tests/pcg_scalar_model.py (checked on the CPU by
tests/test_pcg_scalar_model.py); the sums also on arrays of integers, where the result is exact whatever the order.

The loops reach k_reduce_mb only from 16,384 partial sums (a million rows) upward, k_reduce beyond 1,024 partial sums only between 65 k
and 1 M rows, and the corners of the state machine over PcgScalars::done / fault / cancelled only where a solve happens to pass through
them; here every count at which the kernels take another path and every corner is a case.  Every launch is compared as the whole arena --
partial sums, a NaN guard behind them, the 112-byte scalars image -- so a field or a slot written that should not be is seen.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import pcg_scalar_model as M
from adaptiveviscositysolver_amd import capi
from pcg_scalar_model import SCALARS, f32, f64

pytestmark = pytest.mark.gpu

NB_REDUCE = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 5119, 8192, 8193]
NB_MB = [1, 63, 64, 65, 127, 16383, 16384, 16385, 65536, 65537, 262144, 262145, 64 * 4097]
NRED_OFF = [(1, 0), (2, 0), (3, 0), (4, 0), (1, 2), (1, 3)]
NAN_GUARD = 64             # NaNs behind the nred * nb partial sums: a read beyond the end poisons the sum
STAGE_NAN = np.arange(256, dtype=np.uint64) | np.uint64(capi.SCALAR_PROBE_STAGE_NAN)
SUMMER = {capi.SCALAR_PROBE_REDUCE: M.reduce_block, capi.SCALAR_PROBE_REDUCE_MB: M.reduce_mb, capi.SCALAR_PROBE_REDUCE_PAIR: M.reduce_block,
          capi.SCALAR_PROBE_REDUCE_LAUNCH: M.reduce_launch_sum}


def image(**over):
    """a PcgScalars image with every field set to a distinct value"""
    sc = np.zeros(1, SCALARS)[0]
    sc["rho"], sc["pAp"], sc["rr"], sc["alpha"], sc["beta"], sc["threshold"], sc["rhs_norm2"] = 1.7, 4.2, 0.5, 0.37, 0.61, 1e-3, 3.0
    sc["red"][:] = (9.25, 8.5, 7.75, 6.125)
    sc["iter"], sc["done"], sc["fault"], sc["cancelled"], sc["rho_alt"] = 6, 0, 0, 0, 2.3
    for k, v in over.items():
        if k == "red":
            sc["red"][:] = v
        else:
            sc[k] = v
    return sc


def data(rng, n):
    """mixed signs over sixteen decades: another summation order changes bits"""
    return rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)


class Stage:
    """the arena of a scalar-stage launch and the launch itself"""

    def __init__(self, lib, na, nb_=0):
        self.lib = lib
        self.ar = M.DeviceArena([("pa", f64, na + NAN_GUARD), ("pb", f64, nb_ + NAN_GUARD), ("sc", np.uint8, SCALARS.itemsize)])
        self.stage = np.zeros(256)
        self.ticket = C.c_uint32(77)

    def start(self, pa, sc, pb=()):
        buf = self.ar.host.copy()
        v = self.ar.views(buf)
        v["pa"][:], v["pb"][:] = np.nan, np.nan
        v["pa"][:len(pa)], v["pb"][:len(pb)] = pa, pb
        v["sc"][:] = np.frombuffer(sc.tobytes(), np.uint8)
        return buf

    def record(self, buf):
        return self.ar.views(buf)["sc"].view(SCALARS)[0]

    def launch(self, start, which, nb=0, nred=0, nb_b=0, nred_b=0, op=M.OP_NONE, tol=1e-3, skip=0, red_off=0, launches=1):
        ar = self.ar
        self.stage[:] = 0.
        self.ticket.value = 77
        return ar.run(start, lambda: capi.check(self.lib.avs_pcg_scalar_probe(
            which, ar.ptr("pa"), nb, nred, ar.ptr("pb"), nb_b, nred_b, op, tol, skip, red_off, launches, ar.ptr("sc"), SCALARS.itemsize,
            self.stage.ctypes.data_as(C.c_void_p), C.byref(self.ticket), C.c_void_p(torch.cuda.current_stream().cuda_stream))))

    def same(self, got, want, what):
        if not np.array_equal(got, want):
            raise AssertionError((what, "differs in", self.ar.which(got, want), "scalars got", self.record(got), "want", self.record(want)))


@pytest.fixture(scope="module")
def lib(built_lib):
    return capi.load_probe()


def check_stage(st, nred, blocks):
    """the staging array: the block sums of the nred arrays (None: not written), the NaN pattern everywhere else"""
    want = STAGE_NAN.copy()
    if blocks is not None:
        for q in range(nred):
            want[64 * q:64 * (q + 1)] = blocks[q].view(np.uint64)
    assert np.array_equal(st.stage.view(np.uint64), want), "staging array"


# ---------------------------------------------------------------------------------------------------------------------------------------
# reductions
# ---------------------------------------------------------------------------------------------------------------------------------------
REDUCTIONS = [(capi.SCALAR_PROBE_REDUCE, nb) for nb in NB_REDUCE] + [(capi.SCALAR_PROBE_REDUCE_MB, nb) for nb in NB_MB] + \
    [(capi.SCALAR_PROBE_REDUCE_LAUNCH, nb) for nb in (16383, 16384)]


@pytest.mark.parametrize("which,nb", REDUCTIONS, ids=[f"{('reduce_launch', 'k_reduce', 'k_reduce_mb')[w]}-{nb}" for w, nb in REDUCTIONS])
def test_reductions_match_the_model_and_the_exact_sums(lib, which, nb):
    rng = np.random.default_rng(11 + which + nb)
    st = Stage(lib, 4 * nb)
    multi = which == capi.SCALAR_PROBE_REDUCE_MB or (which == capi.SCALAR_PROBE_REDUCE_LAUNCH and nb >= M.MB_FROM)
    for nred, off in NRED_OFF:
        for exact in (False, True):
            pa = np.concatenate([(q + 1.) * np.arange(1, nb + 1) for q in range(nred)]) if exact else data(rng, nred * nb)
            start = st.start(pa, image())
            want = start.copy()
            M.reduce_into(st.record(want), pa, nb, nred, off, SUMMER[which])
            got = st.launch(start, which, nb, nred, red_off=off)
            st.same(got, want, (which, nb, nred, off, exact))
            red = st.record(got)["red"]
            if exact:      # independent of the model: below 2^53 every order gives the integer
                assert [red[off + q] for q in range(nred)] == [(q + 1) * nb * (nb + 1) // 2 for q in range(nred)], (which, nb, nred, off)
            assert all(red[k] == image()["red"][k] for k in range(4) if not off <= k < off + nred)    # the other slots survive
            assert st.ticket.value == 0, (which, nb, "ticket")
            if which != capi.SCALAR_PROBE_REDUCE:
                check_stage(st, nred, [M.reduce_mb_blocks(pa[q * nb:(q + 1) * nb]) for q in range(nred)] if multi else None)


def test_reduce_pair_with_unequal_counts(lib):
    rng = np.random.default_rng(12)
    sizes = NB_REDUCE
    for k, nba in enumerate(sizes):
        nbb = sizes[(k + 5) % len(sizes)]                    # every count in both halves, never the same in both
        assert nba != nbb
        st = Stage(lib, 3 * nba, 3 * nbb)
        for nreda, nredb in [(2, 1), (1, 1), (3, 1), (1, 3), (2, 2), (0, 2), (2, 0)]:
            for exact in (False, True):
                pa = np.concatenate([(q + 1.) * np.arange(1, nba + 1) for q in range(nreda)] + [[]]) if exact else data(rng, nreda * nba)
                pb = np.concatenate([(q + 5.) * np.arange(1, nbb + 1) for q in range(nredb)] + [[]]) if exact else data(rng, nredb * nbb)
                start = st.start(pa, image(), pb)
                want = start.copy()
                M.reduce_into(st.record(want), pa, nba, nreda, 0)
                M.reduce_into(st.record(want), pb, nbb, nredb, nreda)
                got = st.launch(start, capi.SCALAR_PROBE_REDUCE_PAIR, nba, nreda, nbb, nredb)
                st.same(got, want, ("pair", nba, nreda, nbb, nredb, exact))
                if exact:
                    red = st.record(got)["red"]
                    assert [red[q] for q in range(nreda + nredb)] == [(q + 1) * nba * (nba + 1) // 2 for q in range(nreda)] + \
                        [(q + 5) * nbb * (nbb + 1) // 2 for q in range(nredb)]


@pytest.mark.parametrize("which,nb", [(capi.SCALAR_PROBE_REDUCE, 4097), (capi.SCALAR_PROBE_REDUCE_MB, 65), (capi.SCALAR_PROBE_REDUCE_MB, 16385),
                                      (capi.SCALAR_PROBE_REDUCE_LAUNCH, 16384)])
def test_launches_back_to_back_on_one_ticket(lib, which, nb):
    """two and three launches, each followed by its scalar op: a ticket that is not 0 again leaves the later launches without a last block"""
    rng = np.random.default_rng(13)
    st = Stage(lib, 3 * nb)
    pa = np.abs(data(rng, 3 * nb)) + 1.0                     # r.u, r.r, w.u > 0: OP_SR_STEP goes on at every launch
    for launches in (1, 2, 3):
        for op, nred in ((M.OP_SR_STEP, 3), (M.OP_BETA, 2), (M.OP_NONE, 3)):
            start = st.start(pa, image(threshold=1e-30))
            want = start.copy()
            for _ in range(launches):
                M.reduce_into(st.record(want), pa, nb, nred, 0, SUMMER[which])
                M.apply_scalar_op(st.record(want), op, 1e-3)
            got = st.launch(start, which, nb, nred, op=op, launches=launches)
            st.same(got, want, (which, nb, launches, op))
            assert st.ticket.value == 0
            if op != M.OP_NONE:
                assert st.record(got)["iter"] == 6 + launches and st.record(got)["done"] == 0


@pytest.mark.parametrize("which,nb", [(capi.SCALAR_PROBE_REDUCE, 1025), (capi.SCALAR_PROBE_REDUCE_MB, 127), (capi.SCALAR_PROBE_REDUCE_MB, 16385),
                                      (capi.SCALAR_PROBE_REDUCE_LAUNCH, 16384)])
def test_skip_if_done_leaves_sums_ticket_and_staging_alone(lib, which, nb):
    rng = np.random.default_rng(14)
    st = Stage(lib, 2 * nb)
    pa = data(rng, 2 * nb)
    for done in (1, 2, 3):
        for op in (M.OP_NONE, M.OP_ALPHA, M.OP_ALPHA_ODD, M.OP_BETA, M.OP_SR_STEP):
            for launches in (1, 2):
                start = st.start(pa, image(done=done))
                want = start.copy()
                if done == 2 and op in (M.OP_ALPHA, M.OP_ALPHA_ODD):
                    st.record(want)["done"] = 1                # the pending x update of the converged iteration has run; nothing else
                got = st.launch(start, which, nb, 2, op=op, skip=1, launches=launches)
                st.same(got, want, (which, nb, done, op, launches))
                assert st.ticket.value == 0
                if which != capi.SCALAR_PROBE_REDUCE:
                    check_stage(st, 2, None)
    # without skip_if_done the sums are folded whatever `done` says, and the op sees the flag
    start = st.start(pa, image(done=2))
    want = start.copy()
    M.reduce_into(st.record(want), pa, nb, 2, 0, SUMMER[which])
    M.apply_scalar_op(st.record(want), M.OP_ALPHA, 1e-3)
    st.same(st.launch(start, which, nb, 2, op=M.OP_ALPHA), want, (which, nb, "no skip"))
    assert st.record(want)["done"] == 1


# ---------------------------------------------------------------------------------------------------------------------------------------
# scalar ops
# ---------------------------------------------------------------------------------------------------------------------------------------
def ulps(x, k, T=f64):
    x = T(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, T(np.inf if k > 0 else -np.inf))
    return f64(x)


ALL_OPS = list(range(1, 10))


def scalar_cases():
    """(name, op, tol, image)"""
    out = []
    for op in ALL_OPS:
        for done in (0, 1, 2, 3):                                            # every op from every state
            out.append((f"op{op}_done{done}", op, 1e-3, image(done=done)))
            out.append((f"op{op}_done{done}_converges", op, 1e-3, image(done=done, threshold=1e3, red=(9.25, 1e-9, 1e-9, 6.125))))
    for op in (M.OP_INIT, M.OP_SR_INIT, M.OP_SR_INIT_F32):
        out.append((f"op{op}_rhs_zero", op, 1e-3, image(red=(0., 8.5, 7.75, 6.125))))
        out.append((f"op{op}_rhs_minus_zero", op, 1e-3, image(red=(-0., 8.5, 7.75, 6.125))))
        for tol in (1e-3, 1e-200):                                           # the clamp of the threshold at the smallest normal number
            for bb in (1e-300, 1e-40, 3.0):
                for rr in (1e-310, 1e-39, 1e-38, 2e-308, 4e-308, 1.0):      # either side of both clamps
                    red = (bb, rr, 7.75, 6.125) if op == M.OP_INIT else (bb, 8.5, rr, 6.125)
                    out.append((f"op{op}_clamp_tol{tol:g}_bb{bb:g}_rr{rr:g}", op, tol, image(red=red, done=1)))
    thr = 0.0123456789
    for k in (-1, 0, 1):                                                     # r.r one ulp below the threshold, equal to it (the test is <), one above
        out.append((f"beta_rr{k:+d}ulp", M.OP_BETA, 1e-3, image(threshold=thr, red=(ulps(thr, k), 8.5, 7.75, 6.125))))
        out.append((f"sr_step_rr{k:+d}ulp", M.OP_SR_STEP, 1e-3, image(threshold=thr, red=(9.25, ulps(thr, k), 7.75, 6.125))))
        t32 = f64(f32(thr))                                                  # the float step compares floats: a float threshold, float ulps ...
        out.append((f"sr_step_f32_rr{k:+d}ulp", M.OP_SR_STEP_F32, 1e-3, image(threshold=t32, red=(9.25, ulps(t32, k, f32), 7.75, 6.125))))
        # ... and a double one ulp off a float threshold rounds onto it
        out.append((f"sr_step_f32_rr{k:+d}ulp64", M.OP_SR_STEP_F32, 1e-3, image(threshold=t32, red=(9.25, ulps(t32, k), 7.75, 6.125))))
    for op in (M.OP_ALPHA, M.OP_ALPHA_ODD):
        out.append((f"op{op}_rho_and_rho_alt", op, 1e-3, image(rho=1.7, rho_alt=2.3)))
    return out


def test_every_scalar_op_matches_the_model_on_the_whole_image(lib):
    st = Stage(lib, 0)
    cases = scalar_cases()
    seen = set()
    for name, op, tol, sc in cases:
        start = st.start((), sc)
        want = start.copy()
        M.apply_scalar_op(st.record(want), op, tol)
        got = st.launch(start, capi.SCALAR_PROBE_SCALAR, op=op, tol=tol)
        st.same(got, want, name)
        w = st.record(want)
        seen.add((op, int(sc["done"]), int(w["done"])))
        # the cases are what they are meant to be
        if name.endswith("_rhs_zero") or name.endswith("_rhs_minus_zero"):
            assert w["done"] == 3 and w["rr"] == 0.
        if "_clamp_" in name:          # tol^2 = 1e-400 is 0 in double and in float; float: 1e-300 is 0 and 1e-6 x 1e-40 is below the denormals
            if op == M.OP_SR_INIT_F32 and "bb1e-300" in name:
                assert w["done"] == 3, name
            elif op == M.OP_SR_INIT_F32:
                assert (w["threshold"] == f64(M.FLT_MIN)) == (tol == 1e-200 or "bb1e-40" in name), name
            else:
                assert (w["threshold"] == M.DBL_MIN) == (tol == 1e-200), name
        if "ulp" in name:
            below = name.split("rr")[1].startswith("-1") and not name.endswith("-1ulp64")
            assert w["done"] == ((2 if op == M.OP_BETA else 1) if below else 0) and w["iter"] == (6 if below else 7), name
    a, b = (st.record(st.launch(st.start((), image()), capi.SCALAR_PROBE_SCALAR, op=op))["alpha"] for op in (M.OP_ALPHA, M.OP_ALPHA_ODD))
    assert (a, b) == (1.7 / 9.25, 2.3 / 9.25)
    # done 2 -> 1 by the alpha ops only (the three INIT ops start a solve: they set `done` whatever it was); every op that can converge,
    # freeze or detect a zero right-hand side did
    starts = (M.OP_INIT, M.OP_SR_INIT, M.OP_SR_INIT_F32)
    assert {(op, 2, 1) for op in ALL_OPS if op not in starts} & seen == {(M.OP_ALPHA, 2, 1), (M.OP_ALPHA_ODD, 2, 1)}
    assert {(M.OP_INIT, 0, 1), (M.OP_INIT, 1, 0), (M.OP_INIT, 0, 3), (M.OP_BETA, 0, 2), (M.OP_SR_INIT, 1, 0), (M.OP_SR_INIT, 0, 1),
            (M.OP_SR_STEP, 0, 1), (M.OP_SR_INIT_F32, 1, 0), (M.OP_SR_INIT_F32, 1, 1), (M.OP_SR_INIT_F32, 0, 3), (M.OP_SR_INIT, 0, 3), (M.OP_SR_STEP_F32, 0, 1)} <= seen


def test_a_wrong_image_size_is_refused(lib):
    st = Stage(lib, 0)
    ar = st.ar
    for size in (SCALARS.itemsize - 8, SCALARS.itemsize + 8, 0):
        rc = lib.avs_pcg_scalar_probe(capi.SCALAR_PROBE_SCALAR, None, 0, 0, None, 0, 0, M.OP_ALPHA, 1e-3, 0, 0, 1, ar.ptr("sc"), size, None, None, None)
        assert rc == capi.EINVAL
        rc = lib.avs_sr_vector_probe(capi.SR_PROBE_INIT, 0, 1, 1, ar.ptr("pa"), None, ar.ptr("pa"), None, None, ar.ptr("pa"), ar.ptr("pa"),
                                     ar.ptr("pa"), None, None, None, size, 0, ar.ptr("pa"), None)
        assert rc == capi.EINVAL


@pytest.mark.parametrize("init", [True, False], ids=["init", "update"])
def test_mixed_finish(lib, init):
    rng = np.random.default_rng(15)
    which = capi.SCALAR_PROBE_MIXED_FINISH_INIT if init else capi.SCALAR_PROBE_MIXED_FINISH
    nq = 3 if init else 2

    def run(st, part, g, sc, tol, what):
        start = st.start(part, sc)
        want = start.copy()
        M.mixed_finish(st.record(want), part, g, tol, init)
        st.same(st.launch(start, which, nb=g, tol=tol), want, what)
        return st.record(want)

    # the sums: one accumulator per thread, every count around the block and twice the block (the vector grid has at most 2,048 workgroups)
    for g in (0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048):
        st = Stage(lib, nq * g)
        for done in (0, 1, 2, 3):
            w = run(st, np.abs(data(rng, nq * g)) + 1.0, g, image(done=done, threshold=1e-30), 1e-3, ("sums", g, done))
            exact = np.concatenate([(q + 1.) * np.arange(1, g + 1) for q in range(nq)] + [[]])
            e = run(st, exact, g, image(done=done, threshold=1e-30), 1e-3, ("exact", g, done))
            if g and (init or done != 3):      # independent of the model: r.r and, behind it in rho, r.z as exact integers
                assert (e["rr"], e["rho"]) == (g * (g + 1) // 2, g * (g + 1))
            if not init and g:     # entered with done 0: goes on; 1 or 2: the frozen chunk's beta step, counted; 3: untouched
                assert (w["done"], w["iter"], w["red"][3]) == {0: (0, 6, 0.), 1: (0, 7, 1.), 2: (0, 7, 1.), 3: (3, 6, 6.125)}[done]
                if done in (1, 2):
                    assert w["beta"] == w["rho"] / 1.7
    st = Stage(lib, 3)
    thr = 0.0123456789
    if init:
        for bb in (0., -0., 1e-300, 1e-40, 3.0):
            for tol in (1e-3, 1e-200):
                for rr in (1e-310, 2e-308, 4e-308, 1.0):
                    for done in (0, 1, 2, 3):
                        w = run(st, np.array([rr, 8.5, bb]), 1, image(done=done), tol, ("init", bb, tol, rr, done))
                        assert w["done"] == (3 if bb == 0. else 1 if rr < w["threshold"] else 0)
                        assert bb == 0. or (w["threshold"] == M.DBL_MIN) == (tol == 1e-200)
    else:
        for k in (-1, 0, 1):
            for done in (0, 1, 2, 3):
                w = run(st, np.array([ulps(thr, k), 8.5]), 1, image(done=done, threshold=thr), 1e-3, ("threshold", k, done))
                assert w["done"] == (3 if done == 3 else 1 if k < 0 else 0)
                assert w["iter"] == (7 if done in (1, 2) and k >= 0 else 6)


def test_sr_mixed_begin_and_step(lib):
    st = Stage(lib, 0)
    thr = 0.0123456789
    reached = set()
    for done in (0, 1, 2, 3):
        for fault in (0, 1, 2):
            for cancelled in (0, 1):
                for k in (-1, 0, 1):
                    sc = image(done=done, fault=fault, cancelled=cancelled, threshold=thr, red=(9.25, ulps(thr, k), 7.75, 6.125))
                    for which, fn in ((capi.SCALAR_PROBE_SR_MIXED_BEGIN, M.sr_mixed_begin), (capi.SCALAR_PROBE_SR_MIXED_STEP, M.sr_mixed_step)):
                        start = st.start((), sc)
                        want = start.copy()
                        fn(st.record(want))
                        st.same(st.launch(start, which), want, (which, done, fault, cancelled, k))
                        w = st.record(want)
                        if done == 3 or fault:
                            assert w.tobytes() == sc.tobytes()           # rhs == 0 and a transport fault keep everything
                        elif which == capi.SCALAR_PROBE_SR_MIXED_BEGIN:
                            assert w["done"] == 0 and w["cancelled"] == cancelled
                        else:
                            stop = cancelled or k < 0
                            assert (w["done"], w["iter"], w["rr"]) == (1 if stop else 0, 6 if stop else 7, ulps(thr, k))
                            reached.add((bool(cancelled), k < 0))
    assert len(reached) == 4
