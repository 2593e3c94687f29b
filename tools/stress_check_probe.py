"""avs_prepass_check_stress_indices on the 512^3 four-level fat beam and the 1024^3 thin sheet: HIP-event time of one call with
AVS_CHECK_EDGE_INDICES, with AVS_CHECK_CENTER_INDICES and with both (the pre-pass object runs on a stream torch knows, the events bracket
the call on that stream), the host's wall time of the same calls, and next to them avs_prepass_check_octree (labels, labels + velocity
indices) on the same object in the same run.  Each with the bytes of lattice it has to read -- edges: four bytes per entry of every level
and axis; centres: four bytes per cell of every level; both with their occurrence counters once written and once read; the neighbour
reads of the entries that carry an id are not counted -- and the fraction of the stream rate the project quotes (6.29 TB/s) that follows.
Median of 20 calls after two warm-ups.
`python tools/stress_check_probe.py [beam512] [sheet1024]` prints one JSON line per scene."""
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
        L, nvel, nedge, ncen = int(info.levels), int(info.n_velocity), int(info.n_edge), int(info.n_center)
        n = [[sc.res[a] >> l for a in range(3)] for l in range(L)]
        label_bytes = sum(r[0] * r[1] * r[2] for r in n)
        velocity_bytes = 4 * sum((r[0] + (a == 0)) * (r[1] + (a == 1)) * (r[2] + (a == 2)) for r in n for a in range(3)) + 8 * nvel
        edge_bytes = 4 * sum((r[0] + (a != 0)) * (r[1] + (a != 1)) * (r[2] + (a != 2)) for r in n for a in range(3)) + 8 * nedge
        center_bytes = 4 * label_bytes + 8 * ncen
        stress, octree = capi.StressCheck(), capi.OctreeCheck()

        def stress_call(what):
            return lambda: capi.check(pp.lib.avs_prepass_check_stress_indices(pp.h, what, C.byref(stress)))

        def octree_call(what):
            return lambda: capi.check(pp.lib.avs_prepass_check_octree(pp.h, what, C.byref(octree)))

        both = capi.CHECK_EDGE_INDICES | capi.CHECK_CENTER_INDICES
        stress_call(both)()
        out = {"scene": name, "levels": L, "n_velocity": nvel, "n_edge": nedge, "n_center": ncen, "passed": int(stress.passed),
               "violations": [int(v) for v in stress.violations], "active_edges": int(stress.active_edges), "active_centers": int(stress.active_centers),
               "edge_bytes": edge_bytes, "center_bytes": center_bytes, "label_bytes": label_bytes, "velocity_bytes": velocity_bytes}
        for what, call, nbytes in (("edges", stress_call(capi.CHECK_EDGE_INDICES), edge_bytes), ("centers", stress_call(capi.CHECK_CENTER_INDICES), center_bytes),
                                   ("edges_and_centers", stress_call(both), edge_bytes + center_bytes),
                                   ("octree_labels", octree_call(capi.CHECK_LABELS), label_bytes),
                                   ("octree_labels_and_indices", octree_call(capi.CHECK_LABELS | capi.CHECK_VELOCITY_INDICES), label_bytes + velocity_bytes)):
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
        out["octree_passed"] = int(octree.passed)
        print(json.dumps(out), flush=True)
        pp.close()
        del sc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
