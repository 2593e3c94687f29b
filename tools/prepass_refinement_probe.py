#!/usr/bin/env python
"""Measurements behind profiles/prepass_refinement.md (needs an MI355X; prints one JSON line per record).

  --mode off       octree_ms of avs_prepass_get_info with no option set and no indicator given, through a minimal binding of
                   the four entries it needs -- so that AVS_LIB_PATH may name a library built from an earlier commit, which
                   lacks the refinement entries.  One warm frame, then --frames timed frames per workload.
  --mode feature   this tree's library: set_ms of avs_prepass_set_refinement at dilate 0 and 4 and octree_ms with flags set,
                   each next to the time its bytes take at the achievable HBM rate (MI355X: 6.29 TB/s); then, on the 512^3
                   beam, what the resolution costs: DOF counts, assemble and solve time and iterations with the default
                   octree, with fine bandwidth 4, and with the solve's own shear rate above its 98 % quantile, dilated by 2.

Workloads: the 512^3 four-level fat beam and the 1024^3 five-level thin sheet of bench.py.
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

HBM_BYTES_PER_S = 6.29e12   # the achievable stream rate the project quotes (8 TB/s peak)


def workloads(which):
    dev = torch.device("cuda:0")
    if "beam64" in which:    # (a rehearsal size)
        yield "beam64", scenes.fat_beam(64, 4, device=dev)
    if "beam512" in which:
        yield "beam512", scenes.fat_beam(512, 4, device=dev)
    if "sheet1024" in which:
        yield "sheet1024", scenes.thin_sheet(1024, 5, thickness_cells=32, device=dev)


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
    for name, sc in workloads(args.workloads):
        d = capi.PrepassDesc(sc.res[0], sc.res[1], sc.res[2], float(sc.dx), int(sc.levels), 3, 0.5, 0, vp(0), 0, 0, 0)
        h = vp()
        assert L.avs_prepass_create(C.byref(d), C.byref(h)) == 0
        torch.cuda.synchronize()
        times, info = [], capi.PrepassInfo()
        for frame in range(1 + args.frames):
            assert L.avs_prepass_run(h, sc.liquid.data_ptr(), None if sc.solid is None else sc.solid.data_ptr(), capi.MEM_DEVICE) == 0
            assert L.avs_prepass_get_info(h, C.byref(info)) == 0
            if frame > 0:
                times.append(info.octree_ms)
        emit({"mode": "off", "label": args.label, "lib": capi.LIB_PATH, "workload": name, "n_velocity": info.n_velocity,
              "octree_ms": times, "weights_ms": info.weights_ms, "classify_ms": info.classify_ms, "number_ms": info.number_ms}, args.out)
        L.avs_prepass_destroy(h)
        del sc
        torch.cuda.empty_cache()


def floor_ms(nbytes):
    return 1e3 * nbytes / HBM_BYTES_PER_S


def mode_feature(args):
    from adaptiveviscositysolver_amd import DevicePrepass, ViscositySolve
    for name, sc in workloads(args.workloads):
        cells = sc.res[0] * sc.res[1] * sc.res[2]
        word_bytes = cells // 8
        pp = DevicePrepass(sc.res, sc.dx, sc.levels)

        def frames(n):
            pp.run(sc.liquid, sc.solid)   # warm
            return [pp.run(sc.liquid, sc.solid).octree_ms for _ in range(n)]

        base = frames(args.frames)
        solve_rows = []
        if name.startswith("beam"):   # the indicator: the shear rate of this frame's solve
            def solve_with(label):
                info = pp.run(sc.liquid, sc.solid)
                s = ViscositySolve(sc.res, sc.dx, sc.dt, info.levels, device=0)
                pp.apply(s)
                s.set_scene_fields(sc)
                ai = s.assemble()
                si = s.solve(args.tol, 2500)
                solve_rows.append({"setting": label, "levels": info.levels, "n_velocity": info.n_velocity, "n_edge": info.n_edge, "n_center": info.n_center,
                                   "nnz": ai.nnz, "assemble_ms": ai.stencil_ms + ai.guess_ms + ai.system_ms + ai.csr_ms, "solve_ms": si.solve_ms,
                                   "iterations": si.iterations, "converged": si.converged, "octree_ms": info.octree_ms,
                                   "refined": pp.refinement_info().refined})
                return s
            solve_with("warm-up").close()   # (first launches load code objects)
            solve_rows.clear()
            s = solve_with("default")
            indicator = s.shear_rate_field(device_array=True)
            s.close()
            vals = indicator[sc.liquid <= 0]
            thr = float(vals.kthvalue(int(0.98 * (vals.numel() - 1)) + 1).values)   # 98 % quantile, nearest rank
            del vals
        else:                   # a field with 2 % of its cells above the threshold, scattered
            g = torch.Generator(device="cuda").manual_seed(1)
            indicator = torch.rand((sc.res[2], sc.res[1], sc.res[0]), dtype=torch.float32, device="cuda", generator=g)
            thr = 0.98
        for dilate in (0, 4):
            pp.set_refinement(indicator, thr, dilate)   # warm (and the first call allocates)
            ms = []
            for _ in range(args.frames):
                pp.set_refinement(indicator, thr, dilate)
                ms.append(pp.refinement_info().set_ms)
            ri = pp.refinement_info()
            nbytes = 4 * cells + word_bytes + (6 * word_bytes if dilate else 0)   # field read, bits written; three passes read and write the words
            flagged_ms = frames(args.frames)
            emit({"mode": "feature", "workload": name, "dilate": dilate, "threshold": thr, "seeds": ri.seeds, "flagged": ri.flagged,
                  "refined": pp.refinement_info().refined, "set_ms": ms, "set_bytes": nbytes, "set_floor_ms": floor_ms(nbytes),
                  "octree_ms_flagged": flagged_ms, "octree_ms_off_same_process": base, "mask_extra_floor_ms": floor_ms(word_bytes)}, args.out)
        # what reading the flags costs the mask kernel, apart from the octree they make: every cell flagged against no flags and a fine
        # bandwidth beyond the liquid's depth -- the same mask, the same octree passes
        pp.set_refinement(torch.ones_like(indicator), 0.5, 0)
        all_flagged = frames(args.frames)
        nv_flagged = pp.info.n_velocity
        pp.set_refinement(None)
        pp.set_option(capi.PREPASS_OPTION_FINE_BANDWIDTH, 1e9)
        by_bandwidth = frames(args.frames)
        assert pp.info.n_velocity == nv_flagged
        pp.set_option(capi.PREPASS_OPTION_FINE_BANDWIDTH, 2.0)
        emit({"mode": "feature", "workload": name, "same_octree": "all liquid cells fine", "n_velocity": nv_flagged,
              "octree_ms_all_flagged": all_flagged, "octree_ms_by_bandwidth": by_bandwidth}, args.out)
        if name.startswith("beam"):
            pp.set_refinement(None)
            pp.set_option(capi.PREPASS_OPTION_FINE_BANDWIDTH, 4.0)
            solve_with("fine bandwidth 4").close()
            pp.set_option(capi.PREPASS_OPTION_FINE_BANDWIDTH, 2.0)
            pp.set_refinement(indicator, thr, 2)
            solve_with("shear rate > 98 % quantile, dilate 2").close()
            emit({"mode": "feature", "workload": name, "tol": args.tol, "solves": solve_rows}, args.out)
        pp.close()
        del indicator, sc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("off", "feature"), required=True)
    ap.add_argument("--workloads", default="beam512,sheet1024")
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    (mode_off if a.mode == "off" else mode_feature)(a)
