"""The host-only geometry of a pre-pass run (csrc/avs_prepass_plan.cpp) without a GPU: avs_prepass_plan_host (libavs_probe.so) plans the
level cap, the slab-local ranges of every rank and level, and the numbering's tile layout; they are checked against what the kernels rely
on -- stated as properties of the ranges, not as a second copy of their arithmetic."""
import numpy as np
import pytest

from adaptiveviscositysolver_amd import capi

TILE, MARGIN, MAX_LEVELS = 16, 12, capi.MAX_LEVELS

# extent on the cut axis / levels / cuts
SLAB_CASES = [
    (16, 1, [0, 8, 16]),
    (16, 4, [0, 8, 16]),
    (64, 3, [0, 32, 64]),
    (64, 3, [0, 20, 64]),
    (64, 3, [0, 0, 64]),            # an empty rank at either end
    (64, 3, [0, 64, 64]),
    (32, 3, [0, 8, 16, 24, 32]),
    (64, 4, [0, 21, 43, 64]),
    (128, 5, [0, 1, 127, 128]),
    (64, 6, [0, 13, 64]),
    (256, 4, [0, 100, 101, 256]),   # the window of ranks 0 and 2 is a proper part of level 0
]


def _res(extent, levels, axis):
    res = [max(1 << levels, 16)] * 3     # the other axes carry `levels` levels and no more than they must
    res[axis] = extent
    return res


def _clip(lo, hi, n):
    return max(lo, 0), min(hi, n)


def _contains(outer, lo, hi):
    return outer[0] <= lo and hi <= outer[1]


@pytest.mark.parametrize("case", range(len(SLAB_CASES)))
def test_slab_ranges_of_every_rank(built_lib, case):
    extent, levels, cuts = SLAB_CASES[case]
    axis = case % 3
    world = len(cuts) - 1
    for rank in range(world):
        plan = capi.prepass_plan_host(_res(extent, levels, axis), levels, axis, cuts, rank)
        L = plan["levels"]
        assert L == levels
        rng = {r: [(int(a), int(b)) for a, b in zip(*plan[r])] for r in ("win", "nl", "v", "p1")}
        win, nl, v, p1 = rng["win"], rng["nl"], rng["v"], rng["p1"]
        for l in range(L):
            n = extent >> l
            for r in rng.values():
                assert 0 <= r[l][0] <= r[l][1] <= n, (rank, l, r[l])
            assert win[l][0] % TILE == 0 and (win[l][1] % TILE == 0 or win[l][1] == n)
            assert _contains(win[l], *_clip((cuts[rank] >> l) - MARGIN, -(-cuts[rank + 1] // (1 << l)) + MARGIN, n)), (rank, l)
            assert nl[l] == _clip(win[l][0] - 2, win[l][1] + 2, n)
            assert _contains(v[l], *nl[l])
            if l >= 1:
                assert _contains(p1[l], *_clip(v[l][0] - 1, v[l][1] + 1, n)), (rank, l)
            if l >= 2:
                assert v[l - 1] == (2 * p1[l][0], 2 * p1[l][1])
        assert v[L - 1] == nl[L - 1]
        if L >= 2:
            assert _contains(v[0], 2 * p1[1][0], 2 * p1[1][1])
        assert v[0][0] % 4 == 0 and (v[0][1] % 4 == 0 or v[0][1] == extent)
    if case == len(SLAB_CASES) - 1:     # (what the small cases cannot show)
        for rank in (0, 2):
            lo, hi = capi.prepass_plan_host(_res(extent, levels, axis), levels, axis, cuts, rank)["win"]
            assert (lo[0], hi[0]) != (0, extent)


@pytest.mark.parametrize("case", range(len(SLAB_CASES)))
def test_without_slabs_every_range_is_the_whole_level(built_lib, case):
    extent, levels, _ = SLAB_CASES[case]
    plan = capi.prepass_plan_host(_res(extent, levels, 0), levels)     # (without cuts the ranges are those along axis 0)
    assert plan["levels"] == levels
    for r in ("win", "nl", "v", "p1"):
        assert list(plan[r][0]) == [0] * levels and list(plan[r][1]) == [extent >> l for l in range(levels)]


def _extents(res, kind, level, axis):
    """entries per axis of a lattice: kind 0 faces across `axis`, 1 edges along `axis`, 2 cells"""
    gr = [n >> level for n in res]
    for a in range(3):
        gr[a] += (kind == 0 and a == axis) or (kind == 1 and a != axis)
    return gr


def _tiles(gr):
    return int(np.prod([-(-g // TILE) for g in gr]))


@pytest.mark.parametrize("res,levels", [((16, 16, 16), 1), ((16, 16, 16), 4), ((64, 32, 16), 3), ((32, 32, 32), 3)])
def test_tile_layout(built_lib, res, levels):
    plan = capi.prepass_plan_host(res, levels)
    L = plan["levels"]
    assert L == levels
    tile0_of, level_tile0, seg = plan["tile0_of"], plan["level_tile0"], plan["seg"]
    assert seg[0] == 0
    for c in range(3):      # velocity faces, edges, centres: level-major, then axis; one lattice per level for centres
        run = 0
        for l in range(L):
            assert level_tile0[c][l] == run == tile0_of[c][l][0]
            for a in range(1 if c == 2 else 3):
                assert tile0_of[c][l][a] == run
                run += _tiles(_extents(res, c, l, a))
        assert level_tile0[c][L] == run == seg[c + 1] - seg[c] - 1
    run = 0
    for a in range(3):      # the regular grid: the level-0 face lattices again
        assert tile0_of[3][0][a] == run == tile0_of[0][0][a]
        run += _tiles(_extents(res, 0, 0, a))
    assert run == seg[4] - seg[3] - 1 == level_tile0[0][1]
    assert plan["n_exchange"] == seg[4] + MAX_LEVELS


def test_a_fraction_of_a_tile_is_a_tile(built_lib):
    """64 x 32 x 16 at level 2: 4 cells along z"""
    plan = capi.prepass_plan_host((64, 32, 16), 3)
    assert plan["level_tile0"][2][3] - plan["level_tile0"][2][2] == 1 == _tiles(_extents((64, 32, 16), 2, 2, 0))


@pytest.mark.parametrize("res,desired,capped", [((16, 16, 16), 6, 4), ((64, 32, 16), 6, 4)])
def test_level_cap(built_lib, res, desired, capped):
    assert capi.prepass_plan_host(res, desired)["levels"] == capped


def test_plan_under_asan_and_ubsan(tmp_path):
    """the same cases through a stand-alone program (tests/prepass_plan_main.cpp) built with the host sanitizers"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "prepass_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(root, "include"), "-I", os.path.join(root, "adaptiveviscositysolver_amd", "csrc"),
                           os.path.join(root, "tests", "prepass_plan_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


def test_plan_struct_matches_header(tmp_path):
    """capi.PrepassPlanInfo mirrors avs_prepass_plan_info of include/avs_probe.h: size and the offset of every field"""
    import ctypes
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f for f, _ in capi.PrepassPlanInfo._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "avs_probe.h"\nint main(void){printf("%zu", sizeof(avs_prepass_plan_info));'
                   + "".join(f'printf(" %zu", offsetof(avs_prepass_plan_info, {f}));' for f in fields) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(capi.PrepassPlanInfo)] + [getattr(capi.PrepassPlanInfo, f).offset for f in fields]
    assert fields[0] == "struct_size" and capi.MAX_LEVELS == 8
