"""avs_prepass_get_octree_cells with device arrays on the 512^3 four-level fat beam and the 1024^3 thin sheet: HIP-event time of one call
(the pre-pass object runs on a stream torch knows, the events bracket the call on that stream), the host's wall time of the same call,
and the count query alone; next to the floor -- the bytes of all label lattices over the stream rate the project quotes (6.29 TB/s).
Median of 20 calls after two warm-ups.  `python tools/octree_cells_probe.py [beam512] [sheet1024]` prints one JSON line per scene."""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from adaptiveviscositysolver_amd import DevicePrepass, capi, scenes  # noqa: E402

STREAM_RATE = 6.29e12   # bytes/s, DESIGN.md section 4
SCENES = {
    "beam512": lambda dev: scenes.fat_beam(512, 4, device=dev),
    "sheet1024": lambda dev: scenes.thin_sheet(1024, 5, thickness_cells=32, device=dev),
}


def main():
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    for name in sys.argv[1:] or list(SCENES):
        sc = SCENES[name](dev)
        torch.cuda.synchronize()
        pp = DevicePrepass(sc.res, sc.dx, sc.levels, stream=stream.cuda_stream)
        info = pp.run(sc.liquid, sc.solid)
        L = int(info.levels)
        label_bytes = sum((sc.res[0] >> l) * (sc.res[1] >> l) * (sc.res[2] >> l) for l in range(L))
        pos, ps, lev, ijk, per_level = pp.octree_cells(device_arrays=True)
        n = int(per_level.sum())
        fn = pp.lib.avs_prepass_get_octree_cells
        got = C.c_int64()

        def fill():
            capi.check(fn(pp.h, None, n, pos.data_ptr(), ps.data_ptr(), lev.data_ptr(), ijk.data_ptr(), C.byref(got), None, capi.MEM_DEVICE))

        def count():
            capi.check(fn(pp.h, None, 0, None, None, None, None, C.byref(got), None, capi.MEM_DEVICE))

        out = {"scene": name, "levels": L, "cells": n, "per_level": [int(v) for v in per_level[:L]], "label_bytes": label_bytes,
               "record_bytes": 32 * n, "floor_ms": round(label_bytes / STREAM_RATE * 1e3, 4)}
        for what, call in (("fill", fill), ("count", count)):
            ev_ms, wall_ms = [], []
            for k in range(22):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a.record(stream)
                call()
                b.record(stream)
                b.synchronize()
                t1 = time.perf_counter()
                if k >= 2:
                    ev_ms.append(a.elapsed_time(b))
                    wall_ms.append((t1 - t0) * 1e3)
            out[what + "_event_ms"] = round(statistics.median(ev_ms), 4)
            out[what + "_event_ms_min_max"] = [round(min(ev_ms), 4), round(max(ev_ms), 4)]
            out[what + "_wall_ms"] = round(statistics.median(wall_ms), 4)
        print(json.dumps(out), flush=True)
        pp.close()
        del sc, pos, ps, lev, ijk
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
