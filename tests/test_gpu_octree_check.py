"""avs_check_octree / avs_prepass_check_octree: the octree invariants on the device (avs_check.hip).

Reference: tests/octree_check_model.py (NumPy; pinned by test_octree_check_model.py).  The device report must equal the model's report
exactly -- every count, `passed`, and the first violation: integer work on both sides, no tolerance anywhere in this module.  Corrupted
pyramids are only ever read by the checker: the hot path is never run on one."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

from adaptiveviscositysolver_amd import DevicePrepass, ViscositySolve, capi, scenes

import octree_check_cases as K
import octree_check_model as M

pytestmark = pytest.mark.gpu

BOTH = capi.CHECK_LABELS | capi.CHECK_VELOCITY_INDICES
WHATS = (BOTH, capi.CHECK_LABELS, capi.CHECK_VELOCITY_INDICES)


def as_model(rep):
    """solver.OctreeCheck -> octree_check_model.Report"""
    return M.Report(int(rep.passed), tuple(rep.violations), (-1,) * 6 if rep.first is None else tuple(rep.first))


def context_for(labels, dx=1.0):
    nz, ny, nx = labels[0].shape
    return ViscositySolve((nx, ny, nz), dx, 1.0 / 60.0, len(labels), device=0)


def upload(s, labels, vidx=None, n=None):
    for l, lab in enumerate(labels):
        s.set_labels(l, np.ascontiguousarray(lab, np.int8))
        if vidx is not None:
            for a in range(3):
                s.set_index_field(capi.INDEX_VELOCITY, l, a, np.ascontiguousarray(vidx[l][a], np.int32))
    if n is not None:
        s.set_dof_counts(n, 0, 0)


def agree(obj, labels, vidx, n, want_both=None):
    """the object's report equals the model's for the three values of `what`, and a second call gives the same report; returns the
    report for both bits"""
    both = None
    for what in WHATS:
        want = want_both if (what == BOTH and want_both is not None) else M.check(labels, vidx, n, what)
        got = as_model(obj.check_octree(what))
        print(what, got)
        assert got == want, (what, got, want)
        assert as_model(obj.check_octree(what)) == got
        both = got if what == BOTH else both
    return both


# ---- 1. clean pyramids -----------------------------------------------------------------------------------------------------------------
CLEAN = ("sphere16_L2", "sheet64_one_level", "sphere64_L4", "leaving_box")
PASSED = M.Report(1, (0,) * M.RULES, (-1,) * 6)


@pytest.mark.parametrize("name", CLEAN)
def test_clean_pyramid_through_the_setters(built_lib, name):
    labels, vidx, n = K.oracle_pyramid(name)
    s = context_for(labels)
    upload(s, labels, vidx, n)
    agree(s, labels, vidx, n, PASSED)
    s.close()


@pytest.mark.parametrize("name", CLEAN)
def test_clean_pyramid_through_the_prepass(built_lib, name):
    sc = scenes.to_device(K.scene(name), torch.device("cuda:0"))
    pp = DevicePrepass(sc.res, sc.dx, sc.levels)
    info = pp.run(sc.liquid, sc.solid)
    L = int(info.levels)
    want_n = int(info.n_velocity)
    assert L == len(K.oracle_pyramid(name)[0])
    labels = [pp.labels(l) for l in range(L)]                                     # the model reads what the object itself holds
    vidx = [[pp.index(capi.INDEX_VELOCITY, l, a) for a in range(3)] for l in range(L)]
    agree(pp, labels, vidx, want_n, PASSED)
    s = ViscositySolve(sc.res, sc.dx, sc.dt, L, device=0)
    pp.apply(s)                                                                   # lent lattices, checked in place
    agree(s, labels, vidx, want_n, PASSED)
    # an avs_set_* call replaces ONE lent lattice by the context's own copy: the check reads the mix
    bad = labels[0].copy()
    bad[K._pick(bad == M.ACTIVE)] = 7
    s.set_labels(0, bad)
    got = agree(s, [bad] + labels[1:], vidx, want_n)
    assert got.passed == 0 and as_model(pp.check_octree()) == PASSED              # the pre-pass still holds the clean one
    s.close()
    pp.close()


def test_no_liquid_passes(built_lib):
    liquid = torch.full((16, 16, 16), 10.0, dtype=torch.float32, device="cuda:0")
    pp = DevicePrepass((16, 16, 16), 1 / 16, 3)
    assert pp.run(liquid).levels == 0
    for what in WHATS:
        assert as_model(pp.check_octree(what)) == PASSED
    pp.close()


# ---- 2. mutations ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def contexts(built_lib):
    made = {}

    def get(name):
        if name not in made:
            made[name] = context_for(K.oracle_pyramid(name)[0])
        return made[name]
    yield get
    for s in made.values():
        s.close()


@pytest.mark.parametrize("mutation", list(K.MUTATIONS))
@pytest.mark.parametrize("name", K.MUTATED_SCENES)
def test_mutations(contexts, name, mutation):
    labels, vidx, n, must, want = K.mutated(name, mutation)
    assert want.passed == 0 and must <= want.fired()
    s = contexts(name)
    upload(s, labels, vidx, n)
    agree(s, labels, vidx, n, want)


def test_walks_that_wrap(built_lib, monkeypatch):
    """AVS_CELLS_GRID_CAP caps the check's persistent grids too: three workgroups walk the 64^3 lattices (86 trips at level 0)"""
    monkeypatch.setenv("AVS_CELLS_GRID_CAP", "3")       # read at avs_create
    for mutation in ("nephew_inactive", "id_duplicated"):
        labels, vidx, n, _, want = K.mutated("sphere64_L4", mutation)
        s = context_for(labels)
        upload(s, labels, vidx, n)
        agree(s, labels, vidx, n, want)
        s.close()


# ---- 3. every rule at once: random lattices ----------------------------------------------------------------------------------------------
# Shapes: rows of 2 and 1 cells (the bytewise path, sibling blocks that reach beyond the lattice at the top level), 4 / 2 / 1 (a level that
# switches from words to bytes), 16 / 8 / 4 (words on every level), and 64 x 32 x 16 (32 workgroups at level 0).  Labels are mostly valid
# with a few bytes that are no label at all; indices run from below AVS_OUTSIDE to beyond n_velocity.
RANDOM = {"2x8x4_L2": ((2, 8, 4), 2), "4x4x4_L3": ((4, 4, 4), 3), "16x4x8_L3": ((16, 4, 8), 3), "64x32x16_L3": ((64, 32, 16), 3),
          "8x8x8_L1": ((8, 8, 8), 1)}


def random_pyramid(res, L, seed, mostly=None):
    rng = np.random.default_rng(seed)
    labels, vidx = [], []
    n = 40 + int(np.prod(res)) // 4
    for l in range(L):
        shp = (res[2] >> l, res[1] >> l, res[0] >> l)
        lab = rng.integers(0, 4, shp).astype(np.int8)
        if mostly is not None:                                   # large uniform regions: the rules meet cells that satisfy them
            lab[rng.random(shp) < 0.8] = mostly[l]
        odd = rng.random(shp) < 0.05
        lab[odd] = rng.choice(np.array([7, -1, 4, -128], np.int8), int(odd.sum()))
        labels.append(lab)
        per_level = []
        for a in range(3):
            f = list(shp)
            f[2 - a] += 1
            v = rng.integers(-5, n + 3, f).astype(np.int32)
            v[rng.random(f) < 0.5] = M.UNASSIGNED
            low = rng.random(f) < 0.15
            v[low] = rng.integers(-5, 0, int(low.sum()))
            per_level.append(v)
        vidx.append(per_level)
    return labels, vidx, n


@pytest.mark.parametrize("case", list(RANDOM))
@pytest.mark.parametrize("flavour", ["uniform", "up_under_active"])
def test_random_lattices(built_lib, case, flavour):
    res, L = RANDOM[case]
    mostly = None if flavour == "uniform" else [M.UP] * (L - 1) + [M.ACTIVE]
    labels, vidx, n = random_pyramid(res, L, sum(res) + L, mostly)
    want = M.check(labels, vidx, n)
    assert want.fired() >= ({M.RULE_COLUMN, M.RULE_INDEX_VALUE, M.RULE_FACE, M.RULE_NUMBERING} | ({M.RULE_SENTINEL} if L > 1 else set()))
    s = context_for(labels)
    upload(s, labels, vidx, n)
    agree(s, labels, vidx, n, want)
    s.close()


# ---- 4. errors and edges ---------------------------------------------------------------------------------------------------------------
def raw(fn, handle, what, rep=None):
    rep = capi.OctreeCheck() if rep is None else rep
    st = fn(handle, what, C.byref(rep))
    return st, rep, (capi.load().avs_last_error().decode() if st != capi.OK else "")


def test_state_errors(built_lib):
    lib = capi.load()
    labels, vidx, n = K.oracle_pyramid("sphere16_L2")
    s = context_for(labels)
    s.set_labels(1, labels[1])                                        # level 0 missing
    for what in WHATS:
        st, _, err = raw(lib.avs_check_octree, s.h, what)
        assert st == capi.ESTATE and err
    s.set_labels(0, labels[0])
    assert raw(lib.avs_check_octree, s.h, capi.CHECK_LABELS)[0] == capi.OK          # labels alone are enough for the label rules
    for l in range(2):
        for a in range(3):
            st, _, err = raw(lib.avs_check_octree, s.h, BOTH)         # an index lattice is still missing
            assert st == capi.ESTATE and err
            s.set_index_field(capi.INDEX_VELOCITY, l, a, vidx[l][a])
    st, _, err = raw(lib.avs_check_octree, s.h, capi.CHECK_VELOCITY_INDICES)        # ... and now only the dof counts
    assert st == capi.ESTATE and "count" in err
    s.set_dof_counts(n, 0, 0)
    st, rep, _ = raw(lib.avs_check_octree, s.h, BOTH)
    assert st == capi.OK and rep.passed == 1
    s.close()
    pp = DevicePrepass((32, 32, 32), 1.0 / 32, 2)                     # has not run
    for what in WHATS:
        st, _, err = raw(lib.avs_prepass_check_octree, pp.h, what)
        assert st == capi.ESTATE and err
    pp.close()


def test_argument_errors_and_what_0(built_lib):
    lib = capi.load()
    labels, vidx, n = K.oracle_pyramid("sphere16_L2")
    s = context_for(labels)
    pp = DevicePrepass((16, 16, 16), 1.0 / 16, 2)
    for fn, h in ((lib.avs_check_octree, s.h), (lib.avs_prepass_check_octree, pp.h)):
        for what in (4, 7, 0x80000001, 0x100):
            st, _, err = raw(fn, h, what)
            assert st == capi.EINVAL and err, what
        assert fn(h, BOTH, None) == capi.EINVAL
        assert fn(None, BOTH, C.byref(capi.OctreeCheck())) == capi.EINVAL
        for size in (0, 4, -8, 5000):
            rep = capi.OctreeCheck()
            rep.struct_size = size
            st, _, err = raw(fn, h, BOTH, rep)
            assert st == capi.EINVAL and "struct_size" in err, size
    # what == 0: nothing is needed and nothing runs -- the context holds no lattice at all
    st, rep, _ = raw(lib.avs_check_octree, s.h, 0)
    assert st == capi.OK and rep.passed == 1 and not any(rep.violations) and rep.first_rule == -1 and list(rep.first_ijk) == [-1] * 3
    s.close()
    pp.close()


def test_smaller_struct_size_writes_only_that_many_bytes(contexts):
    labels, vidx, n, _, want = K.mutated("sphere16_L2", "label_7")
    s = contexts("sphere16_L2")
    upload(s, labels, vidx, n)
    full = capi.OctreeCheck()
    capi.check(s.lib.avs_check_octree(s.h, BOTH, C.byref(full)))
    assert C.sizeof(full) == 96 and full.struct_size == 96 and full.passed == 0 and full.first_rule == M.RULE_LABEL_VALUE
    for size in (8, 24, 72, 80, 96, 200):                           # ... up to passed, violations[1], the last count, first_level, all, a larger future struct
        buf = (C.c_ubyte * 256)(*([0x5a] * 256))
        rep = capi.OctreeCheck.from_buffer(buf)
        rep.struct_size = size
        capi.check(s.lib.avs_check_octree(s.h, BOTH, C.byref(rep)))
        written = min(size, 96)
        assert bytes(buf)[4:written] == bytes(full)[4:written] and rep.struct_size == size
        assert all(b == 0x5a for b in bytes(buf)[written:])


def test_hot_path_is_bit_identical_after_a_check(built_lib):
    dev = torch.device("cuda:0")
    sc = scenes.to_device(scenes.sphere(32, 3), dev)

    def frame(checked):
        pp = DevicePrepass(sc.res, sc.dx, sc.levels)
        info = pp.run(sc.liquid, sc.solid)
        if checked:
            assert pp.check_octree().passed
        s = ViscositySolve(sc.res, sc.dx, sc.dt, info.levels, device=0)
        pp.apply(s)
        s.set_scene_fields(sc)
        if checked:
            assert s.check_octree().passed
        s.assemble()
        if checked:
            assert s.check_octree(capi.CHECK_LABELS).passed
        sol = s.solve(1e-8, 3000)
        if checked:
            assert s.check_octree().passed
        out = [s.csr(), s.solution(), s.transfer_to_regular_grid(), (sol.iterations, sol.converged, sol.error)]
        s.close()
        pp.close()
        return out

    (csr_a, x_a, t_a, i_a), (csr_b, x_b, t_b, i_b) = frame(False), frame(True)
    assert i_a == i_b and i_a[1] == 1
    assert all(a.tobytes() == b.tobytes() for a, b in zip(csr_a, csr_b))
    assert x_a.tobytes() == x_b.tobytes() and np.abs(x_a).max() > 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(t_a, t_b))


def test_slab_local_objects_are_refused(built_lib):
    """Two virtual ranks of an in-process group, bound the way tests/test_gpu_slab.py binds them: the lattices of a slab-local pre-pass and
    of the context it was applied to are defined inside the rank's window only."""
    dev = torch.device("cuda:0")
    world, axis = 2, 0
    sc = scenes.to_device(scenes.fat_beam(32, 2), dev)
    lib = capi.load()
    pp0 = DevicePrepass(sc.res, sc.dx, sc.levels)
    lv = pp0.run(sc.liquid, sc.solid).levels
    pp0.close()
    grp = C.c_void_p()
    capi.check(lib.avs_local_group_create(world, C.byref(grp)))
    cuts = np.asarray([0, 16, 32], np.int32)
    results, errors, objs = [None] * world, [], []

    def rank_fn(r):
        try:
            pp = DevicePrepass(sc.res, sc.dx, sc.levels)
            s = ViscositySolve(sc.res, sc.dx, sc.dt, lv, device=0)
            objs.append((s, pp))
            s.dist_init_local(grp, r)
            s.dist_bind_prepass(pp, cuts, axis)
            a = raw(lib.avs_prepass_check_octree, pp.h, BOTH)        # refused at entry, before any run
            assert pp.run(sc.liquid, sc.solid).levels == lv
            pp.apply(s)
            b = raw(lib.avs_prepass_check_octree, pp.h, capi.CHECK_LABELS)
            c = raw(lib.avs_check_octree, s.h, BOTH)
            results[r] = (a, b, c)
        except Exception as e:  # pragma: no cover
            import traceback
            errors.append((r, e, traceback.format_exc()))

    th = [threading.Thread(target=rank_fn, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errors, errors
    for res in results:
        assert res is not None
        for st, _, err in res:
            assert st == capi.ESTATE and err
    for s, pp in objs:
        s.close()
        pp.close()
    lib.avs_local_group_destroy(grp)
