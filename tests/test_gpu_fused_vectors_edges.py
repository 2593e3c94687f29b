"""k_update_fused (csrc/avs_pcg.hip), the single launch with a grid barrier that AVS_OPTION_FUSED_VECTOR_UPDATE puts in place of
k_update_r + k_update_xp, at the edges of its row range: ONE probe launch of it (avs_vector_update_probe, AVS_VECTOR_PROBE_ONE_LAUNCH)
against the two-launch probe with AVS_VECTOR_PROBE_FUSED on the same inputs -- the pair that test_gpu_vector_prologue.py checks against
its NumPy model.  Equality is bit for bit over the whole arena: x, p, r, the 2 g partial sums, the scalars image, every array the
kernels only read and the guard bytes between them.

A thread of the fused launch plays thread (T & 255) of the 256-thread workgroups 4 B + (T >> 8) and 1024 + 4 B + (T >> 8) of the 2048
workgroups of the pair, with up to eight pairs of rows each.  The row counts put the last pair at every edge of that layout:
    524,288     the smallest n with 2048 workgroups: only the first half's emulated workgroups hold a pair
    524,290     the first pair of the second half
    1,048,576   exactly one pair per emulated thread;  1,048,577: the odd last row;  1,048,578: the first pair of a second trip
    8,388,607 / 8,388,608   all eight pairs, odd and even;  8,388,609: refused on the host
The inputs are random doubles over twenty binades, so that a sum formed in another order has other bits.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from adaptiveviscositysolver_amd import capi
from pcg_scalar_model import SCALARS

pytestmark = pytest.mark.gpu

G = 2048                   # kVecGrid: the emulated workgroups
NB_MAX = 4096              # kFuseAlphaMax
TABLE = 2049               # kViLdsTable + 1: the largest inverted dictionary (every thread stages up to three entries)
GUARD = 64
ROWS = [524_288, 524_290, 1_048_576, 1_048_577, 1_048_578, 8_388_607, 8_388_608]
F64 = torch.float64


class Arena:
    """every array of a launch in one device buffer, guard bytes between them; `start` is never written after __init__"""

    def __init__(self, n):
        self.n = n
        fields = [("x", 8, n), ("p", 8, n), ("r", 8, n), ("t", 8, n), ("invd", 8, n), ("table", 8, TABLE), ("dcode", 2, n),
                  ("spart", 8, NB_MAX), ("vpart", 8, 2 * G), ("sc", 1, SCALARS.itemsize)]
        self.off, pos = {}, GUARD
        for name, size, cnt in fields:
            self.off[name] = (pos, cnt * size)
            pos += -(-(cnt * size) // 64) * 64 + GUARD
        dev = torch.device("cuda:0")
        gen = torch.Generator(device=dev).manual_seed(n)
        self.start = torch.full((pos,), 0xA5, dtype=torch.uint8, device=dev)
        for name in ("x", "p", "r", "t"):
            a = torch.randn(n, dtype=F64, device=dev, generator=gen)
            a *= torch.pow(10.0, torch.randint(-3, 4, (n,), device=dev, generator=gen).to(F64))
            a[torch.rand(n, device=dev, generator=gen) < 0.03] = 0.0
            self.view(self.start, name, F64).copy_(a)
        self.view(self.start, "invd", F64).copy_(0.25 + 2.0 * torch.rand(n, dtype=F64, device=dev, generator=gen))
        self.view(self.start, "table", F64).copy_(0.25 + 2.0 * torch.rand(TABLE, dtype=F64, device=dev, generator=gen))
        code = torch.randint(0, TABLE, (n,), device=dev, generator=gen).to(torch.int16)
        code[n // 3] = TABLE - 1                      # (the largest code is there: the probe sizes the dictionary by it)
        self.view(self.start, "dcode", torch.int16).copy_(code)
        rng = np.random.default_rng(n)
        sp = (0.2 + rng.random(NB_MAX)) * 10.0 ** rng.integers(-3, 4, NB_MAX)      # p.Ap > 0; negative and zero partial sums among them
        sp[rng.random(NB_MAX) < 0.05] *= -0.5
        sp[rng.random(NB_MAX) < 0.02] = 0.0
        sp[0] = 900.0
        self.view(self.start, "spart", F64).copy_(torch.from_numpy(sp))
        self.view(self.start, "vpart", F64).fill_(12345.0)
        self.work = torch.empty_like(self.start)

    def view(self, buf, name, dtype):
        o, nbytes = self.off[name]
        return buf[o:o + nbytes].view(dtype)

    def ptr(self, name):
        return C.c_void_p(self.work.data_ptr() + self.off[name][0])

    def scalars(self, buf):
        return self.view(buf, "sc", torch.uint8).cpu().numpy().view(SCALARS)[0]

    def differing(self, a, b):
        return [name for name, (o, nbytes) in self.off.items() if not torch.equal(a[o:o + nbytes], b[o:o + nbytes])] or ["guard bytes"]


@functools.lru_cache(maxsize=1)
def arena(n):
    return Arena(n)


def scalars_image(done, converge):
    sc = np.zeros((), SCALARS)
    sc["rho"], sc["rho_alt"], sc["pAp"], sc["alpha"], sc["beta"] = 1.7, 2.3, 4.2, 0.37, 0.61
    sc["threshold"] = 1e300 if converge else 1e-300
    sc["rhs_norm2"], sc["rr"], sc["iter"], sc["done"] = 3.0, 0.5, 6, done
    sc["red"][:] = (9.0, 8.0, 7.0, 6.0)
    return sc


def launch(lib, ar, flags, n, nb, parity, image):
    """one probe call on a fresh copy of the inputs; returns the arena as the launches left it"""
    ar.work.copy_(ar.start)
    ar.view(ar.work, "sc", torch.uint8).copy_(torch.from_numpy(np.frombuffer(image.tobytes(), np.uint8).copy()))
    coded = bool(flags & capi.VECTOR_PROBE_CODED)
    st = lib.avs_vector_update_probe(flags, G, n, nb, parity, ar.ptr("x"), ar.ptr("p"), ar.ptr("r"), ar.ptr("t"),
                                     ar.ptr("table" if coded else "invd"), ar.ptr("dcode"), ar.ptr("spart"), ar.ptr("vpart"), ar.ptr("sc"),
                                     SCALARS.itemsize, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    capi.check(st)
    torch.cuda.synchronize()
    return ar.work.clone()


DONE_CASES = [(0, False), (0, True), (1, False), (2, False), (3, False)]     # (done on entry, threshold above r.r)


@pytest.mark.parametrize("n", ROWS)
def test_one_launch_equals_the_pair_bit_for_bit(n, built_lib):
    lib = capi.load_probe()
    ar = arena(n)
    cases = 0
    for coded in (0, capi.VECTOR_PROBE_CODED):
        for keep in (0, capi.VECTOR_PROBE_KEEP):
            for parity in (0, 1):
                for nb in (1, 768, 4096):
                    for done, converge in DONE_CASES:
                        image = scalars_image(done, converge)
                        flags = capi.VECTOR_PROBE_FUSED | coded | keep
                        want = launch(lib, ar, flags, n, nb, parity, image)
                        got = launch(lib, ar, flags | capi.VECTOR_PROBE_ONE_LAUNCH, n, nb, parity, image)
                        what = ("n", n, "coded", bool(coded), "keep", bool(keep), "parity", parity, "nb", nb, "done", done, "converge", converge)
                        if not torch.equal(got, want):
                            raise AssertionError((what, "differs in", ar.differing(got, want), "scalars got", ar.scalars(got), "want",
                                                  ar.scalars(want)))
                        # the cases are what they are meant to be (the pair itself is checked against its model elsewhere)
                        sc = ar.scalars(got)
                        assert sc["fault"] == 0, what
                        changed = set(ar.differing(got, ar.start)) - {"guard bytes"}
                        if done:            # nothing touched except done: 2 -> 1
                            assert sc["done"] == (1 if done == 2 else done) and sc["iter"] == 6, what
                            want_sc = image.copy()
                            want_sc["done"] = sc["done"]
                            assert sc.tobytes() == want_sc.tobytes() and changed <= {"sc"}, (what, changed)
                        elif converge:      # x updated, p untouched
                            assert sc["done"] == 2 and sc["iter"] == 6 and changed == {"x", "r", "vpart", "sc"}, (what, changed)
                        else:
                            assert sc["done"] == 0 and sc["iter"] == 7 and changed == {"x", "p", "r", "vpart", "sc"}, (what, changed)
                        cases += 1
    assert cases == 2 * 2 * 2 * 3 * 5


def test_more_rows_than_the_registers_hold_are_refused_on_the_host(built_lib):
    lib = capi.load_probe()
    ar = arena(ROWS[-1])
    ar.work.copy_(ar.start)
    torch.cuda.synchronize()
    flags = capi.VECTOR_PROBE_FUSED | capi.VECTOR_PROBE_ONE_LAUNCH
    args = (ar.ptr("x"), ar.ptr("p"), ar.ptr("r"), ar.ptr("t"), ar.ptr("invd"), ar.ptr("dcode"), ar.ptr("spart"), ar.ptr("vpart"), ar.ptr("sc"),
            SCALARS.itemsize, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert lib.avs_vector_update_probe(flags, G, 8_388_609, 768, 0, *args) == capi.EINVAL
    assert lib.avs_vector_update_probe(flags, G - 1, ROWS[-1], 768, 0, *args) == capi.EINVAL                 # another grid
    assert lib.avs_vector_update_probe(flags | capi.VECTOR_PROBE_F32, G, ROWS[-1], 768, 0, *args) == capi.EINVAL  # fp64 only
    assert lib.avs_vector_update_probe(capi.VECTOR_PROBE_ONE_LAUNCH, G, ROWS[-1], 768, 0, *args) == capi.EINVAL  # the fused scalar steps only
    torch.cuda.synchronize()
    assert torch.equal(ar.work, ar.start)              # before any launch
