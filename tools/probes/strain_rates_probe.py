"""avs_get_strain_rates and avs_get_shear_rate_field on the 512^3 four-level fat beam and the 1024^3 thin sheet: HIP-event time of one call
(the context runs on a stream torch knows, the events bracket the call on that stream) and the host's wall time of the same call, for
  rates + cells + summary   every output of avs_get_strain_rates, device arrays
  edge rates / centre rates one array each: the stencil pass alone
  field                     avs_get_shear_rate_field into a device array (both stencil passes, the cell pass and the painting)
next to avs_assembly_info.stencil_ms of the same run's second avs_assemble -- the pass that writes every word the stencil passes read.
The velocity is the initial guess (AVS_RATES_OF_INITIAL_GUESS): nothing is solved.  Median of 20 calls after two warm-ups.
`python tools/probes/strain_rates_probe.py [beam512] [sheet1024]` prints one JSON line per scene."""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from adaptiveviscositysolver_amd import DevicePrepass, ViscositySolve, capi, scenes  # noqa: E402

SCENES = {
    "beam512": lambda dev: scenes.fat_beam(512, 4, device=dev),
    "sheet1024": lambda dev: scenes.thin_sheet(1024, 5, thickness_cells=32, device=dev),
}


def main():
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    which = capi.RATES_OF_INITIAL_GUESS
    for name in sys.argv[1:] or list(SCENES):
        sc = SCENES[name](dev)
        torch.cuda.synchronize()
        pp = DevicePrepass(sc.res, sc.dx, sc.levels, stream=stream.cuda_stream)
        info = pp.run(sc.liquid, sc.solid)
        s = ViscositySolve(sc.res, sc.dx, sc.dt, info.levels, device=0, stream=stream.cuda_stream)
        pp.apply(s)
        s.set_scene_fields(sc)
        s.assemble()
        ainfo = s.assemble()                                     # the second one: allocations and code objects are there
        ne, nc = int(ainfo.n_edge), int(ainfo.n_center)
        edge = torch.empty(ne, dtype=torch.float64, device=dev)
        center = torch.empty(3 * nc, dtype=torch.float64, device=dev)
        cell = torch.empty(nc, dtype=torch.float64, device=dev)
        field = torch.empty(tuple(reversed(s.field_res)), dtype=torch.float32, device=dev)
        summary = capi.StrainSummary()
        torch.cuda.synchronize()
        lib, h = s.lib, s.h
        calls = {
            "all": lambda: capi.check(lib.avs_get_strain_rates(h, which, edge.data_ptr(), center.data_ptr(), cell.data_ptr(), C.byref(summary), capi.MEM_DEVICE)),
            "edge_rates": lambda: capi.check(lib.avs_get_strain_rates(h, which, edge.data_ptr(), None, None, None, capi.MEM_DEVICE)),
            "center_rates": lambda: capi.check(lib.avs_get_strain_rates(h, which, None, center.data_ptr(), None, None, capi.MEM_DEVICE)),
            "field": lambda: capi.check(lib.avs_get_shear_rate_field(h, which, field.data_ptr(), capi.MEM_DEVICE)),
        }
        out = {"scene": name, "levels": int(info.levels), "n_velocity": int(ainfo.n_velocity), "n_edge": ne, "n_center": nc,
               "field_cells": int(field.numel()), "stencil_ms": round(float(ainfo.stencil_ms), 4)}
        for what, call in calls.items():
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
        out.update(empty_edges=int(summary.empty_edges), empty_centers=int(summary.empty_centers), boundary_edges=int(summary.boundary_edges),
                   boundary_centers=int(summary.boundary_centers), nonfinite=int(summary.nonfinite), edge_lookups=[int(v) for v in summary.edge_lookups],
                   empty_pairs=int(summary.empty_pairs), dissipation_edge=summary.dissipation_edge, dissipation_center=summary.dissipation_center,
                   max_shear_rate=summary.max_shear_rate, field_nonzero=int((field != 0).sum().item()), field_max=float(field.max().item()))
        print(json.dumps(out), flush=True)
        s.close()
        pp.close()
        del sc, edge, center, cell, field
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
