"""TEST INFRASTRUCTURE: the model of the pre-pass's non-default mask settings -- the fine layer bandwidth
(avs_prepass_set_option) and the indicator-driven refinement flags (avs_prepass_set_refinement): seeds, box dilation, the extended
mask rule, and a pyramid builder composed from the steps of the independent torch restatement (prepass_torch: build_weights,
build_octree, classify_*, _number), which are untouched -- the settings only change the mask.  The oracle's own pre-pass keeps the
default rule; parity for non-default settings is: device pre-pass == this model, and this model's pyramid through the oracle's hot
path (util.oracle_from_pyramid).

Arrays are (nz, ny, nx), x fastest, as everywhere in tests/.
"""
from __future__ import annotations

import numpy as np
import torch

import prepass_torch as PT

MAX_DILATE = 16


def seeds(indicator, threshold):
    """bool (sim grid): indicator > threshold as a FLOAT compare -- NaN never marks, +inf does."""
    ind = np.asarray(indicator, np.float32)
    with np.errstate(invalid="ignore"):
        return ind > np.float32(threshold)


def dilate(seed, d):
    """Box (Chebyshev) dilation by d cells, clipped at the array: one axis after the other, OR of the 2 d + 1 shifted copies."""
    out = np.asarray(seed, bool)
    for dim in range(3):
        src = out
        out = src.copy()
        n = src.shape[dim]
        for s in range(1, min(d, n - 1) + 1):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[dim] = slice(0, n - s)
            hi[dim] = slice(s, n)
            out[tuple(hi)] |= src[tuple(lo)]
            out[tuple(lo)] |= src[tuple(hi)]
    return out


def flags(indicator, threshold, d, res):
    """(flags int8 on the OCTREE lattice res = (nx, ny, nz), n_seeds, n_flagged): nothing outside the simulation grid is flagged."""
    assert 0 <= d <= MAX_DILATE
    sd = seeds(indicator, threshold)
    fl = dilate(sd, d)
    out = np.zeros((res[2], res[1], res[0]), np.int8)
    nz, ny, nx = fl.shape
    out[:nz, :ny, :nx] = fl
    return out, int(sd.sum()), int(fl.sum())


def build_mask(liquid, solid, dx, extrapolation_scale=0.5, bandwidth=2.0, flagged=None):
    """prepass_torch.build_mask with inner = dx * max(2, bandwidth) (cpp:259-261) and: a deep cell (sdf <= -inner) is fine where the solid
    rule passes OR it is flagged.  Defaults: prepass_torch.build_mask, bit for bit."""
    sdf = liquid.to(torch.float64)
    extrap = dx * extrapolation_scale
    inner = dx * max(2.0, float(bandwidth))
    outer = 3.0 * dx
    sol = torch.full_like(sdf, -1.0) if solid is None else solid.to(torch.float64)
    m = torch.ones_like(liquid, dtype=torch.int8)
    band_out = (sdf > 0) & (sdf < outer)
    neg = sdf <= 0
    near = neg & (sdf > -inner)
    deep = neg & ~near
    keep = deep & (sol > (-inner - extrap))
    if flagged is not None:
        keep = keep | (deep & torch.as_tensor(np.asarray(flagged) != 0, device=liquid.device))
    m[band_out | near | keep] = 0
    m[deep & ~keep] = -1
    return m


_WEIGHTS = {}


def build_pyramid(scene, bandwidth=2.0, flagged=None, n_super=3, extrapolation_scale=0.5, weights_key=None):
    """prepass_torch.build_pyramid with the mask of build_mask above.  weights_key: the weights depend on the liquid SDF only -- a caller
    that builds several pyramids of one scene names it and they are computed once."""
    liquid = scene.liquid
    if weights_key is not None and weights_key in _WEIGHTS:
        cw, ew, fw = _WEIGHTS[weights_key]
    else:
        cw, ew, fw = PT.build_weights(liquid, n_super)
        if weights_key is not None:
            _WEIGHTS[weights_key] = (cw, ew, fw)
    mask = build_mask(liquid, scene.solid, scene.dx, extrapolation_scale, bandwidth, flagged)
    labels = PT.build_octree(mask, scene.levels)
    vidx = PT.classify_velocity(labels, liquid, scene.solid, cw, ew, scene.dx, extrapolation_scale)
    eidx = PT.classify_edges(labels, ew)
    cidx = PT.classify_centers(labels, cw)
    nv = ne = nc = 0
    for l in range(len(labels)):
        for a in range(3):
            vidx[l][a], nv = PT._number(vidx[l][a], nv)
    for l in range(len(labels)):
        for a in range(3):
            eidx[l][a], ne = PT._number(eidx[l][a], ne)
    for l in range(len(labels)):
        cidx[l], nc = PT._number(cidx[l], nc)
    return PT.Pyramid(res=scene.res, dx=scene.dx, dt=scene.dt, levels=len(labels), labels=labels, vidx=vidx, eidx=eidx, cidx=cidx,
                      n_velocity=nv, n_edge=ne, n_center=nc, center_weights=cw, edge_weights=ew, face_weights=fw, mask=mask)


def two_seed_indicator(res):
    """The indicator of the worked cases: 1 in cell (nz/2, ny/2, nx/2) and in cell (nz/2 + 1, ny/2 - 3, nx/4), 0 elsewhere; threshold 0.5."""
    nx, ny, nz = res
    ind = np.zeros((nz, ny, nx), np.float32)
    ind[nz // 2, ny // 2, nx // 2] = 1.0
    ind[nz // 2 + 1, ny // 2 - 3, nx // 4] = 1.0
    return ind


def active_per_level(pyr):
    return [int((lab == PT.ACTIVE).sum()) for lab in pyr.labels]
