"""The CU-resident loop with local value tables (AVS_OPTION_RESIDENT_LOCAL_TABLES) against what the same context does without the option.

    python tools/resident_local_tables_probe.py --case beam128_varvisc [--alternations 3] [--tol 1e-6] [--f32]

Cases: `beam128_varvisc` (fat_beam(128, 3, variable_viscosity=True)), `sphere_rho` (with_sampled_fields(sphere_with_obstacle(64, 4)))
and `beam256_varvisc` (fat_beam(256, 4, variable_viscosity=True), BASELINE configs[2]).  Option 0 and option 1 are interleaved
`--alternations` times on ONE context.  Per arm: it/s (iterations / solve_ms), iterations, solve_ms, new_matrix_solve_ms (wall time of
the first solve after a re-assembly: plan included), whether the resident loop ran, and the plan's verbose lines
(AVS_CG_RESIDENT_VERBOSE=1: table granularity, largest table, code and column bits, LDS tier -- or why it declined).  One JSON document on stdout."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--case", required=True, choices=["beam128_varvisc", "sphere_rho", "beam256_varvisc"])
ap.add_argument("--alternations", type=int, default=3)
ap.add_argument("--tol", type=float, default=1e-6)
ap.add_argument("--f32", action="store_true", help="an AVS_PRECISION_F32 context iterating on float vectors (RESIDENT_F32 = 1, F32_VECTORS = 1)")
a = ap.parse_args()

os.environ["AVS_CG_RESIDENT_VERBOSE"] = "1"          # (read at avs_create)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from adaptiveviscositysolver_amd import ViscositySolve, capi, scenes  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
from util import build_pyramid, feed  # noqa: E402

dev = torch.device("cuda:0")


class StderrCapture:
    """the library's verbose lines go to fd 2: redirect it to a file around one call"""
    def __enter__(self):
        sys.stderr.flush()
        self.f = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.f.fileno(), 2)
        return self

    def __exit__(self, *exc):
        sys.stderr.flush()
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.f.seek(0)
        self.text = self.f.read().decode(errors="replace")
        self.f.close()


def plan_of(text):
    keep = [l.strip() for l in text.splitlines()
            if re.search(r"local tables|not used:|\] plan: |streamed rows:|plan built in", l)]
    return keep[-6:]


sc = {"beam128_varvisc": lambda: scenes.fat_beam(128, 3, variable_viscosity=True, device=dev),
      "sphere_rho": lambda: scenes.with_sampled_fields(scenes.sphere_with_obstacle(64, 4, device=dev)),
      "beam256_varvisc": lambda: scenes.fat_beam(256, 4, variable_viscosity=True, device=dev)}[a.case]()
pyr = build_pyramid(sc)
s = ViscositySolve(sc.res, sc.dx, sc.dt, pyr.levels, device=0, **({"precision": capi.PRECISION_F32} if a.f32 else {}))
feed(s, pyr)
s.set_scene_fields(sc)
if a.f32:
    s.set_solver_option(capi.OPTION_RESIDENT_F32, 1)
    s.set_solver_option(capi.OPTION_F32_VECTORS, 1)


def run(option):
    """new-matrix solve (assembly: new plan), then a timed steady-state solve"""
    s.set_solver_option(capi.OPTION_RESIDENT_LOCAL_TABLES, option)
    s.assemble()
    torch.cuda.synchronize()
    with StderrCapture() as cap:
        t0 = time.perf_counter()
        first = s.solve(a.tol, 5000)
        torch.cuda.synchronize()
        new_ms = (time.perf_counter() - t0) * 1e3
    info = s.solve(a.tol, 5000)
    return {"it_per_s": info.iterations / (info.solve_ms * 1e-3) if info.solve_ms > 0 else None, "iterations": int(info.iterations),
            "solve_ms": info.solve_ms, "new_matrix_solve_ms": new_ms, "resident": int(info.resident), "converged": int(info.converged),
            "first_resident": int(first.resident), "plan": plan_of(cap.text)}


out = {"case": a.case, "tol": a.tol, "float_vectors": bool(a.f32), "rows": None, "alternations": []}
for k in range(a.alternations):
    out["alternations"].append({f"option_{o}": run(o) for o in (0, 1)})
    print(f"[resident_local_tables_probe] {a.case} alternation {k}: " +
          ", ".join(f"{l} {v['it_per_s']:.0f} it/s (resident {v['resident']})" for l, v in out["alternations"][-1].items()), file=sys.stderr)
out["rows"] = int(s.info().n_velocity)
out["nnz"] = int(s.info().nnz)
s.close()
summary = {}
for arm in ("option_0", "option_1"):
    rs = [alt[arm] for alt in out["alternations"]]
    its = sorted(r["it_per_s"] for r in rs)
    summary[arm] = {"it_per_s_median": its[len(its) // 2], "it_per_s_all": its, "iterations": rs[-1]["iterations"],
                    "solve_ms_median": sorted(r["solve_ms"] for r in rs)[len(rs) // 2],
                    "new_matrix_solve_ms_median": sorted(r["new_matrix_solve_ms"] for r in rs)[len(rs) // 2],
                    "resident": rs[-1]["resident"], "plan": rs[-1]["plan"]}
out["summary"] = summary
print(json.dumps(out, indent=1))
