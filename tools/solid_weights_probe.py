#!/usr/bin/env python
"""Measurements behind profiles/solid_weights.md (needs an MI355X; prints one JSON line per record).

  --mode off       weights_ms of avs_prepass_get_info with no option set, through a minimal binding of the four entries it needs -- so
                   that AVS_LIB_PATH may name a library built from an earlier commit, which lacks the option.  Device arrays, one
                   warm frame, then --frames timed frames per workload.  Workloads: the 512^3 four-level fat beam and the 1024^3
                   five-level thin sheet of bench.py.
  --mode feature   this tree's library, "Apply Solid Weights" off and on in the same process, on scenes that have a solid SDF --
                   fat_beam(512, 4, wall=True) and tank(512, 4): weights_ms of steady frames (the far bricks are skipped by the
                   temporal reuse) and of fresh objects (every brick is stored), the near bricks and the DOF counts of both
                   settings, and the counts of avs_solid_weights_info.

Every list of times is the timed frames in order; the notes quote the median with its range.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adaptiveviscositysolver_amd import capi, scenes  # noqa: E402


def off_workloads(which):
    dev = torch.device("cuda:0")
    if "beam64" in which:    # (a rehearsal size)
        yield "beam64", scenes.fat_beam(64, 4, device=dev)
    if "beam512" in which:
        yield "beam512", scenes.fat_beam(512, 4, device=dev)
    if "sheet1024" in which:
        yield "sheet1024", scenes.thin_sheet(1024, 5, thickness_cells=32, device=dev)


def feature_workloads(which):
    dev = torch.device("cuda:0")
    if "wall64" in which:    # (a rehearsal size)
        yield "wall64", scenes.fat_beam(64, 4, wall=True, device=dev)
    if "wall512" in which:
        yield "wall512", scenes.fat_beam(512, 4, wall=True, device=dev)
    if "tank512" in which:
        yield "tank512", scenes.tank(512, 4, device=dev)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def mode_off(args):
    vp, i32 = C.c_void_p, C.c_int32
    L = C.CDLL(capi.LIB_PATH)
    L.avs_prepass_create.argtypes = [C.POINTER(capi.PrepassDesc), C.POINTER(vp)]
    L.avs_prepass_run.argtypes = [vp, vp, vp, i32]
    L.avs_prepass_get_info.argtypes = [vp, C.POINTER(capi.PrepassInfo)]
    L.avs_prepass_destroy.argtypes = [vp]
    L.avs_prepass_destroy.restype = None
    for name, sc in off_workloads(args.workloads):
        d = capi.PrepassDesc(sc.res[0], sc.res[1], sc.res[2], float(sc.dx), int(sc.levels), 3, 0.5, 0, vp(0), 0, 0, 0)
        h = vp()
        assert L.avs_prepass_create(C.byref(d), C.byref(h)) == 0
        torch.cuda.synchronize()
        times, info = [], capi.PrepassInfo()
        for frame in range(1 + args.frames):
            assert L.avs_prepass_run(h, sc.liquid.data_ptr(), None if sc.solid is None else sc.solid.data_ptr(), capi.MEM_DEVICE) == 0
            assert L.avs_prepass_get_info(h, C.byref(info)) == 0
            if frame > 0:
                times.append(info.weights_ms)
            else:
                first = info.weights_ms
        emit({"mode": "off", "label": args.label, "lib": capi.LIB_PATH, "workload": name, "n_velocity": info.n_velocity,
              "weights_ms": times, "weights_ms_first_frame": first, "octree_ms": info.octree_ms, "classify_ms": info.classify_ms,
              "number_ms": info.number_ms}, args.out)
        L.avs_prepass_destroy(h)
        del sc
        torch.cuda.empty_cache()


def mode_feature(args):
    from adaptiveviscositysolver_amd import DevicePrepass
    on = capi.PREPASS_OPTION_APPLY_SOLID_WEIGHTS
    for name, sc in feature_workloads(args.workloads):
        rec = {"mode": "feature", "workload": name}
        pp = DevicePrepass(sc.res, sc.dx, sc.levels)
        pp.run(sc.liquid, sc.solid)   # warm (first launches load code objects)
        for key, value in (("off", 0), ("on", 1), ("off_again", 0), ("on_again", 1)):
            pp.set_option(on, value)
            first = pp.run(sc.liquid, sc.solid)   # the frame of the change: bricks whose constant differs are stored
            steady = [pp.run(sc.liquid, sc.solid).weights_ms for _ in range(args.frames)]
            si = pp.solid_weights_info()
            rec[key] = {"weights_ms_first": first.weights_ms, "weights_ms": steady, "near_bricks": si.near_bricks,
                        "dofs": [pp.info.n_velocity, pp.info.n_edge, pp.info.n_center], "levels": pp.info.levels,
                        "octree_ms": pp.info.octree_ms, "classify_ms": pp.info.classify_ms, "number_ms": pp.info.number_ms,
                        "modified": list(si.modified), "zeroed": list(si.zeroed), "above_one": list(si.above_one),
                        "max_weight": list(si.max_weight), "applied": si.applied}
        pp.close()
        for key, value in (("fresh_off", 0), ("fresh_on", 1)):   # a fresh object stores every brick: the pass at its most expensive
            ms = []
            for _ in range(args.frames):
                fp = DevicePrepass(sc.res, sc.dx, sc.levels)
                fp.set_option(on, value)
                ms.append(fp.run(sc.liquid, sc.solid).weights_ms)
                fp.close()
            rec[key] = {"weights_ms": ms}
        emit(rec, args.out)
        del sc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("off", "feature"), required=True)
    ap.add_argument("--workloads", default=None, help="off: beam512,sheet1024; feature: wall512,tank512")
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    if a.workloads is None:
        a.workloads = "beam512,sheet1024" if a.mode == "off" else "wall512,tank512"
    assert torch.cuda.is_available(), "needs a GPU"
    (mode_off if a.mode == "off" else mode_feature)(a)
