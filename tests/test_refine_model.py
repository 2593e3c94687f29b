"""The model of the pre-pass's fine layer bandwidth and refinement flags (tests/refine_model.py), on the CPU: its defaults are the
existing mask rule, its dilation is the box dilation, and the pyramids it gives for widened or flagged masks -- interior fine islands,
thicker fine layers, two of them with a changed level cap -- have exactly the worked cell and DOF counts and pass through the oracle's hot
path into symmetric systems that PCG solves."""
import numpy as np
import pytest
import torch

import prepass_torch
import refine_model as RM
from adaptiveviscositysolver_amd import scenes
from util import oracle_from_pyramid

DEFAULT_SCENES = {   # the scenes of tests/test_gpu_prepass.py
    "beam32_L3": lambda: scenes.fat_beam(32, 3),
    "beam64_wall": lambda: scenes.fat_beam(64, 3, wall=True),
    "sphere64_L4": lambda: scenes.sphere(64, 4),
    "noncubic": lambda: scenes.fat_beam(64, 3, res=(64, 32, 32)),
    "sheet64": lambda: scenes.thin_sheet(64, 3, thickness_cells=12),
    "levels_capped": lambda: scenes.fat_beam(16, 6),
    "tank64_L3": lambda: scenes.tank(64, 3),
}

SCENES = {
    "beam32_L3": lambda: scenes.fat_beam(32, 3),
    "beam64_L4": lambda: scenes.fat_beam(64, 4),
    "beam64_wall": lambda: scenes.fat_beam(64, 3, wall=True),
    "sphere64_L4": lambda: scenes.sphere(64, 4),
}
# (scene, bandwidth, dilate of the two-seed indicator or None, ACTIVE cells per level, n_velocity)
WORKED = [
    ("beam32_L3", 2, None, [11136, 192], 19972),
    ("beam32_L3", 4, None, [12352, 40], 22960),
    ("beam32_L3", 6, None, [12672], 23668),                # the level cap drops to 1
    ("beam32_L3", 2, 0, [11152, 190], 20029),
    ("beam32_L3", 2, 3, [11936, 92], 21997),
    ("beam64_L4", 2, None, [43744, 2208, 192], 83740),
    ("beam64_L4", 3, None, [52896, 1064, 192], 107320),
    ("beam64_L4", 2, 3, [44768, 2624, 124], 88192),
    ("beam64_wall", 2, 1, [46176, 2176, 158], 78174),
    ("sphere64_L4", 2, None, [27360, 1040, 96, 8], 52044),
    ("sphere64_L4", 2, 0, [27376, 1070, 148, 1], 52332),
    ("sphere64_L4", 2, 1, [27456, 1092, 152], 52680),      # the level cap drops to 3
]


@pytest.mark.parametrize("name", list(DEFAULT_SCENES))
def test_defaults_are_the_existing_mask_rule(name):
    sc = DEFAULT_SCENES[name]()
    want = prepass_torch.build_mask(sc.liquid, sc.solid, sc.dx)
    assert torch.equal(RM.build_mask(sc.liquid, sc.solid, sc.dx), want)
    assert torch.equal(RM.build_mask(sc.liquid, sc.solid, sc.dx, bandwidth=1.0, flagged=np.zeros(tuple(sc.liquid.shape), np.int8)), want)
    # a flag outside the deep liquid changes nothing
    outside = (want != -1).numpy().astype(np.int8)
    assert torch.equal(RM.build_mask(sc.liquid, sc.solid, sc.dx, flagged=outside), want)


@pytest.mark.parametrize("d", [0, 1, 2, 5, 16])
def test_dilation_is_the_box_dilation(d):
    rng = np.random.default_rng(7 + d)
    seed = rng.random((9, 10, 12)) < 0.01
    seed[0, 0, 0] = seed[8, 9, 11] = seed[4, 0, 11] = True
    zs, ys, xs = np.nonzero(seed)
    z, y, x = np.meshgrid(np.arange(9), np.arange(10), np.arange(12), indexing="ij")
    want = np.zeros(seed.shape, bool)
    for k, j, i in zip(zs, ys, xs):
        want |= np.maximum(np.maximum(abs(z - k), abs(y - j)), abs(x - i)) <= d
    assert np.array_equal(RM.dilate(seed, d), want)


def test_seeds_are_a_float_compare_and_flags_stay_inside_the_simulation_grid():
    ind = np.zeros((3, 4, 5), np.float32)
    ind[0, 0, 0], ind[1, 1, 1], ind[2, 3, 4], ind[1, 2, 3] = np.nan, np.inf, 0.25, np.nextafter(np.float32(0.25), np.float32(1))
    fl, n_seeds, n_flagged = RM.flags(ind, 0.25, 0, (8, 4, 4))
    assert n_seeds == n_flagged == 2 and fl.shape == (4, 4, 8)
    assert fl[1, 1, 1] == 1 and fl[1, 2, 3] == 1 and fl.sum() == 2
    fl, n_seeds, n_flagged = RM.flags(ind, 0.25, 16, (8, 4, 4))
    assert n_seeds == 2 and n_flagged == 60 and fl[:3, :4, :5].all() and fl.sum() == 60


_PYRAMIDS = {}


def worked_pyramid(case):
    """(scene, pyramid, flags or None) of a WORKED case; computed once"""
    name, bw, dil, _, _ = case
    key = (name, bw, dil)
    if key not in _PYRAMIDS:
        sc = SCENES[name]()
        fl = None
        if dil is not None:
            fl, n_seeds, _ = RM.flags(RM.two_seed_indicator(sc.res), 0.5, dil, sc.res)
            assert n_seeds == 2
        _PYRAMIDS[key] = (sc, RM.build_pyramid(sc, bandwidth=bw, flagged=fl, weights_key=name), fl)
    return _PYRAMIDS[key]


@pytest.mark.parametrize("case", WORKED, ids=lambda c: f"{c[0]}-bw{c[1]}-d{c[2]}")
def test_worked_cases_have_the_worked_counts(case):
    sc, pyr, fl = worked_pyramid(case)
    assert pyr.levels == len(case[3])
    assert RM.active_per_level(pyr) == case[3]
    assert pyr.n_velocity == case[4]
    if case[:3] == ("beam32_L3", 2, 3):   # flags outside the deep liquid change nothing
        default = prepass_torch.build_mask(sc.liquid, sc.solid, sc.dx)
        assert int(fl.sum()) == 686 and int((pyr.mask != default).sum()) == 637
    if case[1] == 2 and case[2] is None:  # the default settings: the restatement's own pyramid
        ref = prepass_torch.build_pyramid(sc)
        assert torch.equal(pyr.mask, ref.mask) and all(torch.equal(a, b) for a, b in zip(pyr.labels, ref.labels))
        assert (pyr.n_velocity, pyr.n_edge, pyr.n_center) == (ref.n_velocity, ref.n_edge, ref.n_center)


@pytest.mark.parametrize("case", WORKED, ids=lambda c: f"{c[0]}-bw{c[1]}-d{c[2]}")
def test_worked_pyramids_assemble_and_solve_in_the_oracle(case):
    sc, pyr, _ = worked_pyramid(case)
    o = oracle_from_pyramid(sc, pyr)
    o.hot_path()
    A = o.csr().to_scipy()
    assert A.shape[0] == pyr.n_velocity
    assert abs(A - A.T).max() <= 1e-12 * abs(A).max()      # the bar of tests/test_oracle_known_answers.py
    x, info = o.solve(1e-8, 5000)
    assert info.iterations < 5000 and info.error <= 1e-8


def test_refinement_info_mirror_matches_the_header(tmp_path):
    """capi.RefinementInfo against avs_refinement_info as a C compiler lays it out (include/avs.h compiles as plain C)."""
    import ctypes
    import os
    import subprocess

    from adaptiveviscositysolver_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [name for name, _ in capi.RefinementInfo._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "avs.h"\nint main(void){printf("%zu", sizeof(avs_refinement_info));\n'
                   + "".join(f'printf(" %zu", offsetof(avs_refinement_info, {f}));\n' for f in fields)
                   + 'printf(" %d\\n", (int)AVS_PREPASS_OPTION_FINE_BANDWIDTH);return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [ctypes.sizeof(capi.RefinementInfo)] + [getattr(capi.RefinementInfo, f).offset for f in fields] + [capi.PREPASS_OPTION_FINE_BANDWIDTH]
    assert got == want
