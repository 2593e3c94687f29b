"""avs_check_solution on the 512^3 four-level fat beam and the 1024^3 thin sheet: HIP-event time of one call (the context runs on a
stream torch knows, the events bracket the call on that stream) and the host's wall time of the same call, for
  report             the report alone (x = the solution)
  report_residual    the report and every r_i into a device array
  residual           the residual alone: no fold, no wait
  guess              the report of the initial guess (x = x0)
  check_system       avs_check_system(what = AVS_CSR_CHECK_VALUES) of the same context, for scale: rules 0, 1, 2 and 3 over the same matrix
with the algorithmic bytes 12 nnz + 4 (n + 1) + 24 n (+ 8 n for the residual) and the fraction of 8 TB/s they make at the measured time.
The solution is one avs_solve to 1e-3 (the benchmark's tolerance); the line also says what that solve claimed and what was true.
Median of 20 calls after two warm-ups.
`python tools/probes/solution_check_probe.py [beam512] [sheet1024]` prints one JSON line per scene."""
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
PEAK_BYTES_PER_MS = 8e12 / 1e3


def main():
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    for name in sys.argv[1:] or list(SCENES):
        sc = SCENES[name](dev)
        torch.cuda.synchronize()
        pp = DevicePrepass(sc.res, sc.dx, sc.levels, stream=stream.cuda_stream)
        info = pp.run(sc.liquid, sc.solid)
        s = ViscositySolve(sc.res, sc.dx, sc.dt, info.levels, device=0, stream=stream.cuda_stream)
        pp.apply(s)
        s.set_scene_fields(sc)
        ainfo = s.assemble()
        solve = s.solve(1e-3, 2500)
        n, nnz = int(ainfo.n_velocity), int(solve.nnz)
        res = torch.empty(n, dtype=torch.float64, device=dev)
        rep, csr = capi.SolutionCheck(), capi.CsrCheck()
        torch.cuda.synchronize()
        lib, h = s.lib, s.h
        calls = {
            "report": lambda: capi.check(lib.avs_check_solution(h, capi.CHECK_OF_SOLUTION, None, C.byref(rep), capi.MEM_DEVICE)),
            "report_residual": lambda: capi.check(lib.avs_check_solution(h, capi.CHECK_OF_SOLUTION, res.data_ptr(), C.byref(rep), capi.MEM_DEVICE)),
            "residual": lambda: capi.check(lib.avs_check_solution(h, capi.CHECK_OF_SOLUTION, res.data_ptr(), None, capi.MEM_DEVICE)),
            "guess": lambda: capi.check(lib.avs_check_solution(h, capi.CHECK_OF_INITIAL_GUESS, None, C.byref(rep), capi.MEM_DEVICE)),
            "check_system": lambda: capi.check(lib.avs_check_system(h, capi.CSR_CHECK_VALUES, 0.0, C.byref(csr))),
        }
        out = {"scene": name, "levels": int(info.levels), "n": n, "nnz": nnz, "solve_iterations": int(solve.iterations), "solve_converged": int(solve.converged),
               "solve_error": solve.error, "solve_resident": int(solve.resident)}
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
            if what == "report":
                out.update(true_relative_residual=rep.relative_residual, claimed_error=rep.claimed_error, claimed_iterations=int(rep.claimed_iterations),
                           rows_summed=int(rep.rows_summed), nonfinite_residual=int(rep.nonfinite_residual), max_abs_residual=rep.max_abs_residual,
                           max_residual_row=int(rep.max_residual_row), x_dot_ax=rep.x_dot_ax, x_dot_b=rep.x_dot_b, update_norm2=rep.update_norm2)
            if what == "guess":
                out.update(guess_relative_residual=rep.relative_residual)
        algorithmic = 12 * nnz + 4 * (n + 1) + 24 * n
        out.update(bytes_report=algorithmic, bytes_report_residual=algorithmic + 8 * n,
                   fraction_of_8TBs_report=round(algorithmic / out["report_event_ms"] / PEAK_BYTES_PER_MS, 4),
                   fraction_of_8TBs_report_residual=round((algorithmic + 8 * n) / out["report_residual_event_ms"] / PEAK_BYTES_PER_MS, 4),
                   check_system_passed=int(csr.passed))
        print(json.dumps(out), flush=True)
        s.close()
        pp.close()
        del sc, res
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
