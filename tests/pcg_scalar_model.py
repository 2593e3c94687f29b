"""NumPy model of the scalar stages of the PCG loops and of the vector kernels of the single-reduction loops (csrc/avs_pcg.hip,
csrc/avs_halo.hpp, csrc/avs_pcg_mixed.inl): the specification the kernels are compared with bit for bit (tests/test_gpu_pcg_scalars.py,
tests/test_gpu_sr_vectors.py), itself checked on the CPU against exact sums, math.fsum, the oracle's PCG and tests/dist_mixed_model.py
(tests/test_pcg_scalar_model.py).

Summation orders (the build is -ffp-contract=off: NumPy's one rounding per operation is the kernels').
  k_reduce, k_reduce_pair   thread t of 1,024 adds src[t + 1024 j] in ascending j: while four more fit (t + 1024 (j + 3) < nb) into the
                            accumulators s0 .. s3 in turn, the rest into s0; then (s0 + s1) + (s2 + s3), the shuffle tree of wave_sum
                            over the 64 lanes, the 16 waves ascending from 0.
  k_reduce_mb               that order in block b of 64 over [b share, min((b + 1) share, nb)), share = ceil(nb / 64); wave_sum over the
                            64 block sums
  k_mixed_finish            one accumulator per thread, ascending j; wave_sum; the 16 waves ascending from 0.
  vector kernels            a thread's own terms in grid-stride order (trip k: row 256 (blk + g k) + t) in the accumulator type, widened
                            to double, wave_sum, the four waves as ((w0 + w1) + w2) + w3 (block_sum)
An absent entry is modelled as + 0.0: it changes no bit of a sum that started from + 0.0.
"""
import numpy as np

f32, f64 = np.float32, np.float64

SCALARS = np.dtype([("rho", "f8"), ("pAp", "f8"), ("rr", "f8"), ("alpha", "f8"), ("beta", "f8"), ("threshold", "f8"), ("rhs_norm2", "f8"),
                    ("red", "f8", 4), ("iter", "i4"), ("done", "i4"), ("fault", "i4"), ("cancelled", "i4"), ("rho_alt", "f8")])
assert SCALARS.itemsize == 112

(OP_NONE, OP_INIT, OP_RHO0, OP_ALPHA, OP_BETA, OP_SR_INIT, OP_SR_STEP, OP_ALPHA_ODD, OP_SR_INIT_F32, OP_SR_STEP_F32) = range(10)
RED_BLOCK = 1024           # kRedBlock: threads of the reduction kernels
RED_BLOCKS = 64            # kRedBlocks: workgroups of k_reduce_mb
MB_FROM = 16384            # reduce_launch: k_reduce_mb from this many partial sums
BLOCK = 256                # kBlock: threads of the vector kernels
DBL_MIN = 2.2250738585072014e-308
FLT_MIN = f32(1.17549435e-38)


# ---------------------------------------------------------------------------------------------------------------------------------------
# sums
# ---------------------------------------------------------------------------------------------------------------------------------------
def wave_sum(v):
    """v[..., 64] -> lane 0 of wave_sum (csrc/avs_wave.hpp): lane i += lane i + o for o = 32, 16, .. 1"""
    for o in (32, 16, 8, 4, 2, 1):
        v = v[..., :o] + v[..., o:2 * o]
    return v[..., 0]


def block_sum(v):
    """v[nblocks, 256] doubles -> thread 0's block_sum of every workgroup"""
    w = wave_sum(v.reshape(-1, 4, 64))
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _waves_ascending(v):
    """v[1024] -> thread 0 of the reduction kernels: wave_sum per wave, then t = 0.; t += red[w] for w = 0 .. 15"""
    t = f64(0.)
    for s in wave_sum(v.reshape(RED_BLOCK // 64, 64)):
        t = t + s
    return t


def _rows_of(a):
    """a[n] -> [ceil(n / 1024), 1024]: row j holds a[1024 j + t], absent entries + 0.0"""
    nj = -(-len(a) // RED_BLOCK)
    rows = np.zeros(nj * RED_BLOCK)
    rows[:len(a)] = a
    return rows.reshape(nj, RED_BLOCK)


def reduce_blocks(a, lens):
    """workgroups of k_reduce / k_reduce_pair / k_reduce_mb: row b of a[nblocks, >= max(lens)] holds the lens[b] doubles of workgroup b
    (+ 0.0 behind them)"""
    nblocks = len(lens)
    nj = -(-a.shape[1] // RED_BLOCK) if a.size else 0
    rows = np.zeros((nblocks, nj * RED_BLOCK))
    rows[:, :a.shape[1]] = a
    rows = rows.reshape(nblocks, nj, RED_BLOCK)
    t = np.arange(RED_BLOCK)[None, :]
    n = np.asarray(lens)[:, None]
    unrolled = 4 * np.maximum(0, -(-(n - 3 * RED_BLOCK - t) // (4 * RED_BLOCK)))   # entries j < this went through the four-deep loop
    s = np.zeros((4, nblocks, RED_BLOCK))
    for j in range(nj):
        q = np.where(j < unrolled, j % 4, 0)
        for k in range(4):
            s[k] = s[k] + np.where(q == k, rows[:, j], 0.)
    v = (s[0] + s[1]) + (s[2] + s[3])
    waves = wave_sum(v.reshape(nblocks, RED_BLOCK // 64, 64))
    tot = np.zeros(nblocks)
    for w in range(RED_BLOCK // 64):       # thread 0: t = 0.; t += red[w] for w = 0 .. 15
        tot = tot + waves[:, w]
    return tot


def reduce_block(a):
    """one workgroup over the doubles a[0 .. n)"""
    return reduce_blocks(np.asarray(a, f64)[None, :], [len(a)])[0]


def reduce_mb_blocks(a):
    """the 64 block sums k_reduce_mb stages for a[0 .. nb): block b over [b share, min((b + 1) share, nb)), share = ceil(nb / 64)"""
    nb = len(a)
    share = -(-nb // RED_BLOCKS)
    lo = np.minimum(np.arange(RED_BLOCKS) * share, nb)
    lens = np.minimum(lo + share, nb) - lo
    padded = np.zeros(RED_BLOCKS * share)
    padded[:nb] = a
    return reduce_blocks(padded.reshape(RED_BLOCKS, share), lens)


def reduce_mb(a):
    return wave_sum(reduce_mb_blocks(a))


def reduce_launch_sum(a):
    """reduce_launch's choice"""
    return reduce_mb(a) if len(a) >= MB_FROM else reduce_block(a)


def finish_sum(a):
    """k_mixed_finish: one accumulator per thread"""
    s = np.zeros(RED_BLOCK)
    for row in _rows_of(a):
        s = s + row
    return _waves_ascending(s)


def reduce_into(sc, partial, nb, nred, red_off=0, summer=reduce_block):
    """red[red_off + q] = the sum of partial[q nb .. (q + 1) nb)"""
    for q in range(nred):
        sc["red"][red_off + q] = summer(partial[q * nb:(q + 1) * nb])


# ---------------------------------------------------------------------------------------------------------------------------------------
# scalar ops: plain Python on a record of SCALARS (np.void: writes go through to the image)
# ---------------------------------------------------------------------------------------------------------------------------------------
def sr_step_sums(S, red, threshold, st):
    """sr_step_sums<S> on st = dict(rr, rho, alpha, beta, iter, done)"""
    if st["done"]:
        return
    rrs = S(red[1])
    st["rr"] = f64(rrs)
    if rrs < S(threshold):
        st["done"] = 1
        return
    gamma, delta = S(red[0]), S(red[2])
    b2 = gamma / S(st["rho"])
    a = gamma / (delta - b2 * gamma / S(st["alpha"]))
    st["alpha"], st["beta"], st["rho"] = f64(a), f64(b2), f64(gamma)
    st["iter"] += 1


_STEP_FIELDS = ("rr", "rho", "alpha", "beta", "iter", "done")


def sr_step(S, sc_in):
    st = {k: sc_in[k].copy() for k in _STEP_FIELDS}
    with np.errstate(all="ignore"):
        sr_step_sums(S, sc_in["red"], sc_in["threshold"], st)
    return st


def apply_scalar_op(sc, op, tol):
    with np.errstate(all="ignore"):
        _apply(sc, op, f64(tol))


def _apply(sc, op, tol):
    red = sc["red"]
    if op == OP_INIT:
        sc["rhs_norm2"], sc["rr"], sc["iter"] = red[0], red[1], 0
        if red[0] == 0.:
            sc["done"], sc["rr"] = 3, 0.
            return
        thr = max(tol * tol * red[0], f64(DBL_MIN))
        sc["threshold"] = thr
        sc["done"] = 1 if red[1] < thr else 0
    elif op == OP_RHO0:
        if not sc["done"]:
            sc["rho"] = red[0]
    elif op in (OP_ALPHA, OP_ALPHA_ODD):
        if sc["done"] == 2:
            sc["done"] = 1
        elif not sc["done"]:
            sc["pAp"] = red[0]
            sc["alpha"] = (sc["rho_alt"] if op == OP_ALPHA_ODD else sc["rho"]) / red[0]
    elif op == OP_BETA:
        if not sc["done"]:
            sc["rr"] = red[0]
            if red[0] < sc["threshold"]:
                sc["done"] = 2
            else:
                old = sc["rho"].copy()
                sc["rho"] = red[1]
                sc["beta"] = red[1] / old
                sc["iter"] += 1
    elif op == OP_SR_INIT:
        sc["rhs_norm2"], sc["rr"], sc["iter"] = red[0], red[2], 0
        if red[0] == 0.:
            sc["done"], sc["rr"] = 3, 0.
            return
        thr = max(tol * tol * red[0], f64(DBL_MIN))
        sc["threshold"] = thr
        if red[2] < thr:
            sc["done"] = 1
            return
        sc["done"], sc["rho"], sc["alpha"], sc["beta"] = 0, red[1], red[1] / red[3], 0.
    elif op == OP_SR_STEP:
        if not sc["done"]:
            sc["rr"] = red[1]
            if red[1] < sc["threshold"]:
                sc["done"] = 1
            else:
                gamma_old, gamma, delta = sc["rho"].copy(), red[0], red[2]
                beta = gamma / gamma_old
                sc["alpha"] = gamma / (delta - beta * gamma / sc["alpha"])
                sc["beta"], sc["rho"] = beta, gamma
                sc["iter"] += 1
    elif op == OP_SR_INIT_F32:
        bb, ru, rr, wu = (f32(v) for v in red)
        sc["rhs_norm2"], sc["rr"], sc["iter"] = f64(bb), f64(rr), 0
        if bb == f32(0):
            sc["done"], sc["rr"] = 3, 0.
            return
        t = f32(tol)
        thr = t * t * bb
        if thr < FLT_MIN:
            thr = FLT_MIN
        sc["threshold"] = f64(thr)
        if rr < thr:
            sc["done"] = 1
            return
        sc["done"], sc["rho"], sc["alpha"], sc["beta"] = 0, f64(ru), f64(ru / wu), 0.
    elif op == OP_SR_STEP_F32:
        for k, v in sr_step(f32, sc).items():
            sc[k] = v


def mixed_finish(sc, partial, g, tol, init):
    """k_mixed_finish<init>: partial holds (rr, rz[, bb]) x g"""
    tot = [finish_sum(partial[q * g:(q + 1) * g]) for q in range(3 if init else 2)]
    rr, rz = tot[0], tot[1]
    tol = f64(tol)
    with np.errstate(all="ignore"):
        if init:
            bb = tot[2]
            sc["rhs_norm2"], sc["rr"], sc["iter"], sc["red"][3] = bb, rr, 0, 0.
            if bb == 0.:
                sc["done"], sc["rr"] = 3, 0.
                return
            thr = max(tol * tol * bb, f64(DBL_MIN))
            sc["threshold"] = thr
            sc["done"] = 1 if rr < thr else 0
            sc["rho"] = rz
            return
        if sc["done"] == 3:
            return
        frozen = sc["done"] != 0
        sc["rr"], sc["red"][0], sc["red"][1], sc["red"][3] = rr, rr, rz, 0.
        if rr < sc["threshold"]:
            sc["done"] = 1
            return
        if frozen:
            sc["beta"] = rz / sc["rho"]
            sc["iter"] += 1
            sc["red"][3] = 1.
        sc["rho"] = rz
        sc["done"] = 0


def sr_mixed_begin(sc):
    if sc["done"] == 3 or sc["fault"]:
        return
    sc["done"] = 0


def sr_mixed_step(sc):
    if sc["done"] == 3 or sc["fault"]:
        return
    red = sc["red"]
    sc["rr"] = red[1]
    if sc["cancelled"] or red[1] < sc["threshold"]:
        sc["done"] = 1
        return
    with np.errstate(all="ignore"):
        gamma_old, gamma, delta = sc["rho"].copy(), red[0], red[2]
        beta = gamma / gamma_old
        sc["alpha"] = gamma / (delta - beta * gamma / sc["alpha"])
    sc["beta"], sc["rho"] = beta, gamma
    sc["iter"] += 1
    sc["done"] = 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# the vector kernels of the single-reduction loops
# ---------------------------------------------------------------------------------------------------------------------------------------
def grid_sums(g, acc, *terms):
    """per-workgroup block sums of sum_i term[i] for every `terms` array (already of the accumulator type `acc`): thread (blk, t) adds its
    rows 256 (blk + g k) + t in ascending k"""
    T = BLOCK * g
    out = []
    for term in terms:
        assert term.dtype == acc
        trips = -(-len(term) // T)
        rows = np.zeros(trips * T, acc)
        rows[:len(term)] = term
        s = np.zeros(T, acc)
        for row in rows.reshape(trips, T):
            s = s + row
        assert s.dtype == acc
        out.append(block_sum(s.astype(f64).reshape(g, BLOCK)))
    return out


def sr_init(T, g, b, t, idiag, r, u, partial):
    """k_sr_init<T>: idiag is the inverse diagonal per row (the coded form's table[dcode])"""
    bi = b.astype(T)
    ri = bi - t
    ui = idiag * ri
    assert ri.dtype == T and ui.dtype == T
    r[:], u[:] = ri, ui
    partial[:g], partial[g:2 * g], partial[2 * g:3 * g] = grid_sums(g, T, bi * bi, ri * ui, ri * ri)


def sr_update(T, S, g, x, r, p, s, u, w, idiag, sc_in, sc_out, step, partial):
    """k_sr_update<T, ., S>; sc_out is written (whole image) when step is set"""
    done, alpha, beta = int(sc_in["done"]), sc_in["alpha"].copy(), sc_in["beta"].copy()
    if step:
        st = sr_step(S, sc_in)
        done, alpha, beta = int(st["done"]), st["alpha"], st["beta"]
        image = sc_in.copy()
        for k, v in st.items():
            image[k] = v
        sc_out[()] = image
    if done:
        return
    a, bt = T(alpha), T(beta)
    pi = u + bt * p
    si = w + bt * s
    xi = x + a * pi
    ri = r - a * si
    ui = idiag * ri
    for v in (pi, si, xi, ri, ui):
        assert v.dtype == T
    p[:], s[:], x[:], r[:], u[:] = pi, si, xi, ri, ui
    rs, us = ri.astype(S), ui.astype(S)
    partial[:g], partial[g:2 * g] = grid_sums(g, S, rs * us, rs * rs)


def sr_mixed_residual(g, b, t64, idiag, r, u, partial, sc, init):
    """k_sr_mixed_residual<., init>: a state with done != 0 leaves everything as it is (plain form only)"""
    if not init and sc["done"] != 0:
        return
    ri = b - t64
    rf = ri.astype(f32)
    ui = idiag * rf
    assert ui.dtype == f32
    r[:], u[:] = rf, ui
    rr, ru = grid_sums(g, f64, ri * ri, rf.astype(f64) * ui.astype(f64))
    if init:
        partial[:g] = grid_sums(g, f64, b * b)[0]
        partial[g:2 * g], partial[2 * g:3 * g] = ru, rr
    else:
        partial[:g], partial[g:2 * g] = ru, rr


# ---------------------------------------------------------------------------------------------------------------------------------------
# the GPU tests' arena: every array of a launch in one device buffer (one copy in, one copy out), 0xA5 guard bytes between them -- a store
# beyond an array's end, or into an array the launch must not touch, shows up in the comparison of the whole buffer
# ---------------------------------------------------------------------------------------------------------------------------------------
GUARD = 64


class DeviceArena:
    def __init__(self, fields):
        """fields: (name, dtype, count)"""
        import torch
        self.off, pos = {}, GUARD
        for name, dt, cnt in fields:
            self.off[name] = (pos, np.dtype(dt), cnt)
            pos += -(-(cnt * np.dtype(dt).itemsize) // 64) * 64 + GUARD
        self.host = np.full(pos, 0xA5, np.uint8)
        self.dev = torch.empty(pos, dtype=torch.uint8, device="cuda:0")
        self.base = self.dev.data_ptr()

    def views(self, buf):
        return {name: buf[o:o + cnt * dt.itemsize].view(dt) for name, (o, dt, cnt) in self.off.items()}

    def ptr(self, name):
        import ctypes
        return ctypes.c_void_p(self.base + self.off[name][0])

    def run(self, start, launch):
        """the arena after launch() on the image `start`"""
        import torch
        self.dev.copy_(torch.from_numpy(start))
        launch()
        return self.dev.cpu().numpy()

    def which(self, got, want):
        bad = [name for name, (o, dt, cnt) in self.off.items() if not np.array_equal(got[o:o + cnt * dt.itemsize], want[o:o + cnt * dt.itemsize])]
        return bad or ["guard bytes"]
