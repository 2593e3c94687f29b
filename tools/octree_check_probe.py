"""avs_prepass_check_octree on the 512^3 four-level fat beam and the 1024^3 thin sheet: HIP-event time of one call with AVS_CHECK_LABELS and
of one with AVS_CHECK_LABELS | AVS_CHECK_VELOCITY_INDICES (the pre-pass object runs on a stream torch knows, the events bracket the call
on that stream), the host's wall time of the same calls, and next to them the count query of avs_prepass_get_octree_cells on the same
object, which reads the same label lattices.  Each with the bytes it has to read (labels: one byte per cell of every level; indices: four
bytes per face of every level and axis, and the occurrence counters once written and once read) and the fraction of the stream rate
the project quotes (6.29 TB/s) that follows.  Median of 20 calls after two warm-ups.
`python tools/octree_check_probe.py [beam512] [sheet1024]` prints one JSON line per scene."""
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
BOTH = capi.CHECK_LABELS | capi.CHECK_VELOCITY_INDICES


def main():
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    for name in sys.argv[1:] or list(SCENES):
        sc = SCENES[name](dev)
        torch.cuda.synchronize()
        pp = DevicePrepass(sc.res, sc.dx, sc.levels, stream=stream.cuda_stream)
        info = pp.run(sc.liquid, sc.solid)
        L, nvel = int(info.levels), int(info.n_velocity)
        n = [[sc.res[a] >> l for a in range(3)] for l in range(L)]
        label_bytes = sum(r[0] * r[1] * r[2] for r in n)
        index_bytes = 4 * sum((r[0] + (a == 0)) * (r[1] + (a == 1)) * (r[2] + (a == 2)) for r in n for a in range(3)) + 8 * nvel
        rep = capi.OctreeCheck()
        got = C.c_int64()

        def labels():
            capi.check(pp.lib.avs_prepass_check_octree(pp.h, capi.CHECK_LABELS, C.byref(rep)))

        def both():
            capi.check(pp.lib.avs_prepass_check_octree(pp.h, BOTH, C.byref(rep)))

        def count():
            capi.check(pp.lib.avs_prepass_get_octree_cells(pp.h, None, 0, None, None, None, None, C.byref(got), None, capi.MEM_DEVICE))

        both()
        out = {"scene": name, "levels": L, "n_velocity": nvel, "passed": int(rep.passed), "violations": [int(v) for v in rep.violations],
               "label_bytes": label_bytes, "index_bytes": index_bytes}
        for what, call, nbytes in (("labels", labels, label_bytes), ("both", both, label_bytes + index_bytes), ("count_query", count, label_bytes)):
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
            med = statistics.median(ev_ms)
            out[what + "_event_ms"] = round(med, 4)
            out[what + "_event_ms_min_max"] = [round(min(ev_ms), 4), round(max(ev_ms), 4)]
            out[what + "_wall_ms"] = round(statistics.median(wall_ms), 4)
            out[what + "_floor_ms"] = round(nbytes / STREAM_RATE * 1e3, 4)
            out[what + "_fraction_of_stream_rate"] = round(nbytes / STREAM_RATE * 1e3 / med, 3)
        print(json.dumps(out), flush=True)
        pp.close()
        del sc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
