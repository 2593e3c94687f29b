"""The model of the pre-pass's "Apply Solid Weights" option (tests/solid_weights_model.py), on the CPU: hand-derived answers at a planar
wall, the properties the rule promises (an open neighbourhood leaves the weight bit for bit, a positive scaled weight had a positive
weight), the brick-level statement against the per-sample one on a case planted to hold every brick class, the counts the option leaves
on three scenes, and the ctypes mirror of the new struct against the header."""
import numpy as np
import pytest
import torch

import solid_weights_model as SM
from adaptiveviscositysolver_amd import scenes

SCENES = {
    "beam_wall": lambda: scenes.fat_beam(32, 3, wall=True),
    "tank": lambda: scenes.tank(32, 3),
    "obstacle": lambda: scenes.sphere_with_obstacle(32, 3),
}


def _cases():
    out = {name: (sc.liquid, sc.solid, sc.dx) for name, sc in ((k, f()) for k, f in SCENES.items())}
    out["planted"] = SM.planted_case()
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


@pytest.fixture(scope="module")
def models(cases):
    return {name: SM.solid_weights(*c) for name, c in cases.items()}


@pytest.mark.parametrize("n", [2, 3, 4])
def test_known_answers_at_a_planar_wall(n):
    """Liquid everywhere (w = 1), extrapolation 0, solid x < (k0 + j / n) cells.  The sub-samples of the centre sample of cell k0 sit at
    (s + 1/2) / n across the cell: j of the n columns lie inside the solid, so W = (n - j) / n exactly and w' = 1 / W; cells behind the
    wall get 0, cells beyond it keep 1.  j = 0 is the wall ON the cell boundary (every centre sample is on one side, W is n / n); there
    the fraction shows on the lattices that have a sample ON the wall plane -- edge y and edge z, node-based in x -- whose n columns of
    sub-samples straddle it: the floor(n / 2) columns strictly beyond the wall count, the middle column of an odd n interpolates to
    exactly 0 and does not."""
    k0, n3 = 5, np.float32(n ** 3)
    for j in range(n):
        liquid, solid, dx = SM.wall_case(16, k0, j, n)
        m = SM.solid_weights(liquid, solid, dx, 0.0, n)
        cw = m.center.numpy()
        S = (n - j) * n * n
        want = np.float32(1.0) / (np.float32(S) / n3)
        assert (cw[:, :, :k0] == 0).all() and (cw[:, :, k0 + 1:] == 1).all(), (n, j)
        assert (cw[:, :, k0] == want).all(), (n, j, cw[0, 0, k0], want)
        assert m.info.zeroed[0] == k0 * 16 * 16 and m.info.above_one[0] == (16 * 16 if j else 0)
        assert m.info.modified[0] == (k0 + (1 if j else 0)) * 16 * 16
        assert m.info.max_weight[0] == float(want)
        for f in m.face:      # never touched
            assert (f == 1).all()
    liquid, solid, dx = SM.wall_case(16, k0, 0, n)
    m = SM.solid_weights(liquid, solid, dx, 0.0, n)
    want = np.float32(1.0) / (np.float32((n // 2) * n * n) / n3)
    for a in (1, 2):          # edge y, edge z: a node plane at x = k0
        e = m.edge[a].numpy()
        assert (e[:, :, :k0] == 0).all() and (e[:, :, k0] == want).all() and (e[:, :, k0 + 1:] == 1).all(), (n, a)
    ex = m.edge[0].numpy()    # edge x is centred in x: as the centre lattice
    assert (ex[:, :, :k0] == 0).all() and (ex[:, :, k0:] == 1).all()


def test_open_neighbourhood_leaves_the_weight_bitwise(cases, models):
    """S == n^3 gives W == 1.0f and w / 1.0f == w, bit for bit -- also for the 26 other values of w"""
    seen = 0
    for name, (liquid, solid, dx) in cases.items():
        g = SM.shifted_solid(solid, dx, 0.5)
        for k, c in enumerate(SM.SCALED):
            S = SM.sample_counts(g, c, 3)
            scaled = ([models[name].center] + models[name].edge)[k]
            full = S == 27
            assert np.array_equal(scaled[full].numpy().view(np.uint32), models[name].unscaled[k][full].numpy().view(np.uint32)), (name, k)
            seen += int((full & (models[name].unscaled[k] > 0) & (models[name].unscaled[k] < 1)).sum())
    assert seen > 0      # ... some of them fractional


def test_a_positive_scaled_weight_had_a_positive_weight(cases, models):
    """w' > 0 implies w > 0: tile occupancy and the classification's visit lists stay valid supersets"""
    for name, m in models.items():
        for k, scaled in enumerate([m.center] + m.edge):
            assert not bool(((scaled > 0) & ~(m.unscaled[k] > 0)).any()), (name, k)
            assert bool(torch.isfinite(scaled).all()) and bool((scaled >= 0).all())
            assert float(scaled.max()) <= 27.0


def test_off_is_the_liquid_rule(cases):
    import prepass_torch
    for name, (liquid, solid, dx) in cases.items():
        cw, ew, fw = prepass_torch.build_weights(liquid, 3)
        for m in (SM.solid_weights(liquid, solid, dx, enabled=False), SM.solid_weights(liquid, None, dx, enabled=True)):
            assert torch.equal(m.center, cw) and all(torch.equal(a, b) for a, b in zip(m.edge + m.face, ew + fw)), name
            assert m.info.applied == 0 and m.info.modified == [0] * 4 and m.info.max_weight == [0.0] * 4


def test_brick_model_equals_sample_model(cases, models):
    """far bricks from the signs of their windows alone, with the constants they get -- (liquid < 0, solid >= 0): centre and edges 0 but
    faces 1 -- against the per-sample rule, option on and off"""
    for name, (liquid, solid, dx) in cases.items():
        for enabled in (True, False):
            ref = models[name] if enabled else SM.solid_weights(liquid, solid, dx, enabled=False)
            c, e, f, classes, near = SM.brick_weights(liquid, solid, dx, enabled=enabled)
            for got, want in zip([c] + e + f, [ref.center] + ref.edge + ref.face):
                assert np.array_equal(got.numpy().view(np.uint32), want.numpy().view(np.uint32)), (name, enabled)
            assert ref.info.near_bricks == len(near) and 0 < len(near) < len(classes)


def test_planted_case_holds_every_brick_class(cases):
    liquid, solid, dx = cases["planted"]
    assert tuple(liquid.shape) == (32, 32, 64)
    box = liquid < 0
    ground = solid > 0
    rows = (box & ground).any(dim=2).any(dim=0)       # the y rows where box and ground plane overlap
    assert int(rows.sum()) >= 10
    classes, near = SM.brick_classes(liquid, SM.shifted_solid(solid, dx, 0.5))
    have = set(classes.values())
    for want in (("neg", "neg"), ("neg", "pos"), ("neg", "mixed"), ("mixed", "pos"), ("mixed", "mixed")):
        assert want in have, want
    assert any(ls == "pos" for ls, _ in have)
    # the three scenes reach only some of them: their 32-cell bricks span the whole x extent
    for name in SCENES:
        l, s, d = cases[name]
        assert not {("neg", "neg"), ("neg", "pos"), ("neg", "mixed")} <= set(SM.brick_classes(l, SM.shifted_solid(s, d, 0.5))[0].values()), name


def test_counts_on_the_scenes(models, capsys):
    """modified / zeroed / above-one on the centre lattice (n_super 3, extrapolation 0.5) as first worked out for the option:
    beam with wall 1204 / 952 / 196, tank 8296 / 6056 / 2240, obstacle 1084 / 658 / 390, the obstacle reaching weight 27; on the edge
    lattices some scaled weights land exactly on 1.0 (the assembly's `== 1.` replacement, cpp:2133, then meets them)."""
    with capsys.disabled():
        print()
        print(f"{'case':10s} {'lattice':7s} {'modified':>9s} {'zeroed':>8s} {'above-one':>9s} {'max':>8s} {'== 1.0 scaled':>13s}")
        for name, m in models.items():
            for k, lat in enumerate(("centre", "edge x", "edge y", "edge z")):
                scaled = ([m.center] + m.edge)[k]
                on_one = int(((scaled == 1) & (m.unscaled[k] != 1)).sum())
                print(f"{name:10s} {lat:7s} {m.info.modified[k]:9d} {m.info.zeroed[k]:8d} {m.info.above_one[k]:9d} {m.info.max_weight[k]:8.4f} {on_one:13d}")
    for name in SCENES:
        i = models[name].info
        for k in range(4):
            assert i.modified[k] > 0 and i.zeroed[k] > 0 and i.above_one[k] > 0, (name, k)
            assert i.modified[k] >= i.zeroed[k] + i.above_one[k]
    assert models["obstacle"].info.max_weight[0] == 27.0
    for name in SCENES:
        m = models[name]
        assert sum(int(((m.edge[a] == 1) & (m.unscaled[1 + a] != 1)).sum()) for a in range(3)) > 0, name


def test_solid_weights_info_mirror_matches_the_header(tmp_path):
    """capi.SolidWeightsInfo against avs_solid_weights_info as a C compiler lays it out, the option's value, and the entry in the list of
    exported symbols"""
    import ctypes
    import os
    import subprocess

    from adaptiveviscositysolver_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [name for name, _ in capi.SolidWeightsInfo._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "avs.h"\nint main(void){printf("%zu", sizeof(avs_solid_weights_info));\n'
                   + "".join(f'printf(" %zu", offsetof(avs_solid_weights_info, {f}));\n' for f in fields)
                   + 'printf(" %d\\n", (int)AVS_PREPASS_OPTION_APPLY_SOLID_WEIGHTS);return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [ctypes.sizeof(capi.SolidWeightsInfo)] + [getattr(capi.SolidWeightsInfo, f).offset for f in fields] + [capi.PREPASS_OPTION_APPLY_SOLID_WEIGHTS]
    assert got == want
    assert "avs_prepass_get_solid_weights_info" in capi.EXPORTED_SYMBOLS
    hdr = open(os.path.join(root, "include", "avs.h")).read()
    assert "avs_status avs_prepass_get_solid_weights_info(avs_prepass *pp, avs_solid_weights_info *info);" in hdr
    assert "#define AVS_ABI_VERSION 2" in hdr      # purely additive
