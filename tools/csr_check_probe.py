"""avs_check_system on assembled systems: HIP-event time of one call with AVS_CSR_CHECK_ALL (the context runs on a stream torch knows, the
events bracket the call on that stream; the first call is reported on its own, then the median of 10 warm ones), the same for what = 0
(rules 0 and 1: the two passes every call makes) and for ALL without the SYMMETRY bit, next to the run's avs_assembly_info.system_ms and
the byte floor of the row pass (12 B per non-zero, col + val, at the stream rate the project quotes, 6.29 TB/s).  And what the check
measures: asymmetric_entries and max_abs_asymmetry / max_abs_value of the assembled matrix.
`python tools/csr_check_probe.py [beam64] [beam512] [sheet1024] [beam256var] [beam512var] [scene_beam] [scene_buckling]` prints one JSON
line per scene (default: beam512 sheet1024)."""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from adaptiveviscositysolver_amd import DevicePrepass, ViscositySolve, capi, scenes  # noqa: E402

STREAM_RATE = 6.29e12   # bytes/s, DESIGN.md section 4
SCENES = {
    "beam64": lambda dev: scenes.fat_beam(64, 3, device=dev),
    "beam512": lambda dev: scenes.fat_beam(512, 4, device=dev),
    "sheet1024": lambda dev: scenes.thin_sheet(1024, 5, thickness_cells=32, device=dev),
    "beam256var": lambda dev: scenes.fat_beam(256, 4, variable_viscosity=True, device=dev),
    "beam512var": lambda dev: scenes.fat_beam(512, 4, variable_viscosity=True, device=dev),
    "scene_beam": lambda dev: scenes.viscous_beam_scene(device=dev),
    "scene_buckling": lambda dev: scenes.viscous_buckling_scene(device=dev),
}
NO_SYMMETRY = capi.CSR_CHECK_ALL & ~capi.CSR_CHECK_SYMMETRY


def main():
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    for name in sys.argv[1:] or ["beam512", "sheet1024"]:
        sc = SCENES[name](dev)
        fsc = scenes.crop_to_field(sc)
        torch.cuda.synchronize()
        pp = DevicePrepass(sc.res, sc.dx, sc.levels, field_res=sc.field_res)
        pinfo = pp.run(fsc.liquid, fsc.solid)
        s = ViscositySolve(sc.res, sc.dx, sc.dt, pinfo.levels, stream=stream.cuda_stream, field_res=sc.field_res)
        pp.apply(s)
        pp.close()
        s.set_scene_fields(fsc)
        s.assemble()
        ai = s.assemble()   # the second, steady-state assembly is the one whose system_ms is quoted
        rep = capi.CsrCheck()

        def timed(what, tol):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record(stream)
            capi.check(s.lib.avs_check_system(s.h, what, tol, C.byref(rep)))
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b)

        first = timed(capi.CSR_CHECK_ALL, 0.0)
        out = {"scene": name, "levels": int(pinfo.levels), "n": int(ai.n_velocity), "nnz": int(ai.nnz), "system_ms": round(ai.system_ms, 4),
               "csr_ms": round(ai.csr_ms, 4), "passed_at_tolerance_0": int(rep.passed), "evaluated": int(rep.evaluated),
               "violations": [int(v) for v in rep.violations], "empty_rows": int(rep.empty_rows), "longest_row": int(rep.longest_row),
               "asymmetric_entries": int(rep.asymmetric_entries), "max_abs_value": rep.max_abs_value, "max_abs_asymmetry": rep.max_abs_asymmetry,
               "asymmetry_over_max_value": rep.max_abs_asymmetry / rep.max_abs_value if rep.max_abs_value else 0.0,
               "all_first_call_event_ms": round(first, 4)}
        floor = 12.0 * int(ai.nnz) / STREAM_RATE * 1e3
        out["row_pass_floor_ms"] = round(floor, 4)
        for tag, what in (("all", capi.CSR_CHECK_ALL), ("no_symmetry", NO_SYMMETRY), ("rules_0_1", 0)):
            ms = [timed(what, 1e-12 * out["max_abs_value"]) for _ in range(10)]
            out[tag + "_event_ms"] = round(statistics.median(ms), 4)
            out[tag + "_event_ms_min_max"] = [round(min(ms), 4), round(max(ms), 4)]
            if tag == "all":
                out["passed_at_1e-12_of_max_value"] = int(rep.passed)
        out["all_over_row_pass_floor"] = round(out["all_event_ms"] / floor, 2)
        print(json.dumps(out), flush=True)
        s.close()
        del sc, fsc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
