"""The CU-resident loop on float vectors (AVS_OPTION_RESIDENT_F32) against the other loops of an AVS_PRECISION_F32 context.

    python tools/resident_f32_probe.py --case beam128 [--alternations 3] [--loops f64_resident,f32_resident,...]

Cases: `beam` (viscous_beam_scene), `buckling` (viscous_buckling_scene), `beam128` (fat_beam(128, 3)) -- single GPU -- and `slab8`:
rank --rank of the 8-way partition of the 512^3 headline alone on the GPU, its peers looped back onto itself (AVS_DIST_LOOPBACK=1),
measured as tools/loopback_scaling.py measures a slab (the system it solves is not the right one; the time per iteration is).
Loops, interleaved `--alternations` times in this order:
    f64_resident   the resident loop in fp64 (single GPU: F32_VECTORS = 0; slab: DIST_F32_VECTORS = 0)
    f32_resident   the resident loop on float vectors (RESIDENT_F32 = 1)
    f32_phase      float launch-per-phase loop (single GPU: F32_VECTORS = 1; slab: the float single-reduction loop, DIST_F32_VECTORS = 1)
    f64_phase      fp64 launch-per-phase loop (single GPU: resident loop off; slab: DIST_F32_VECTORS = 0, resident loop off)
Per loop: it/s (iterations / solve_ms), iterations, new_matrix_solve_ms (wall time of the first solve after a re-assembly: plan included)
and the resident plan (AVS_CG_RESIDENT_VERBOSE=1: tier NG, LDS bytes, streamed rows).  One JSON document on stdout."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--case", required=True, choices=["beam", "buckling", "beam128", "slab8"])
ap.add_argument("--alternations", type=int, default=3)
ap.add_argument("--loops", default="f64_resident,f32_resident,f32_phase,f64_phase")
ap.add_argument("--tol", type=float, default=1e-5)
ap.add_argument("--iters", type=int, default=320, help="slab8: iterations per timed solve (the looped-back system never converges)")
ap.add_argument("--rank", type=int, default=3)
a = ap.parse_args()

os.environ["AVS_CG_RESIDENT_VERBOSE"] = "1"          # (read at avs_create)
if a.case == "slab8":
    os.environ["AVS_DIST_LOOPBACK"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from adaptiveviscositysolver_amd import DevicePrepass, ViscositySolve, capi, scenes  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
from util import build_pyramid, feed  # noqa: E402

dev = torch.device("cuda:0")
LOOPS = a.loops.split(",")


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
    m = re.search(r"plan: n = (\d+), (\d+) lanes .*?, (\d+) workgroups, .*?(\d+) row-local vectors in global memory, LDS (\d+) B, (\w+) vectors", text)
    st = re.search(r"streamed rows: ([\d.]+) % of the words", text)
    no = re.search(r"not used: (.*?) \(", text)
    if not m:
        return {"resident_plan": None, "refused": no.group(1) if no else None}
    return {"NG": int(m.group(4)), "lds_bytes": int(m.group(5)), "workgroups": int(m.group(3)), "vectors": m.group(6),
            "streamed_words_pct": float(st.group(1)) if st else 0.0}


def configure(s, loop):
    single = a.case != "slab8"
    s.set_solver_option(capi.OPTION_RESIDENT_LOOP, 0 if loop == "f64_phase" else 1)
    s.set_solver_option(capi.OPTION_RESIDENT_F32, 1 if loop == "f32_resident" else 0)
    if single:
        s.set_solver_option(capi.OPTION_F32_VECTORS, {"f64_resident": 0, "f32_resident": -1, "f32_phase": 1, "f64_phase": 0}[loop])
    else:
        s.set_solver_option(capi.OPTION_DIST_F32_VECTORS, 0 if loop.startswith("f64") else 1)


if a.case == "slab8":
    sc = scenes.fat_beam(512, 4, device=dev)
    pp = DevicePrepass(sc.res, sc.dx, sc.levels)
    pi = pp.run(sc.liquid, sc.solid)

    def make():
        s = ViscositySolve(sc.res, sc.dx, sc.dt, pi.levels, precision=capi.PRECISION_F32)
        pp.apply(s)
        s.set_scene_fields(sc)
        capi.check(s.lib.avs_dist_init_hosted(s.h, a.rank, 8))
        return s
else:
    sc = {"beam": lambda: scenes.viscous_beam_scene(), "buckling": lambda: scenes.viscous_buckling_scene(),
          "beam128": lambda: scenes.fat_beam(128, 3)}[a.case]()
    dsc = scenes.to_device(sc, dev)
    pyr = build_pyramid(dsc)

    def make():
        s = ViscositySolve(sc.res, sc.dx, sc.dt, pyr.levels, device=0, field_res=sc.field_res, precision=capi.PRECISION_F32)
        feed(s, pyr)
        s.set_scene_fields(scenes.crop_to_field(dsc))
        return s


def run(s, loop):
    """new-matrix solve (assembly: new plan), then a timed steady-state solve"""
    configure(s, loop)
    if a.case == "slab8":
        s.dist_assemble()                          # (the loop's storage form and vector type are latched here)
        capi.check(s.lib.avs_dist_import_blobs(s.h, None))
        solve = lambda: s.dist_solve(1e-30, a.iters)      # never converges: exactly a.iters iterations
    else:
        s.assemble()
        solve = lambda: s.solve(a.tol, 5000)
    torch.cuda.synchronize()
    with StderrCapture() as cap:
        t0 = time.perf_counter()
        first = solve()
        torch.cuda.synchronize()
        new_ms = (time.perf_counter() - t0) * 1e3
    info = solve()
    fv = int(s.matrix_format().float_vectors)
    return {"it_per_s": info.iterations / (info.solve_ms * 1e-3) if info.solve_ms > 0 else None, "iterations": int(info.iterations),
            "solve_ms": info.solve_ms, "new_matrix_solve_ms": new_ms, "resident": int(info.resident), "float_vectors": fv,
            "converged": int(info.converged), "first_resident": int(first.resident), **plan_of(cap.text)}


s = make()
out = {"case": a.case, "tol": a.tol if a.case != "slab8" else None, "alternations": []}
if a.case == "slab8":
    out.update({"rank": a.rank, "world": 8, "rows_total": int(pi.n_velocity)})
for k in range(a.alternations):
    out["alternations"].append({loop: run(s, loop) for loop in LOOPS})
    print(f"[resident_f32_probe] {a.case} alternation {k}: " +
          ", ".join(f"{l} {v['it_per_s']:.0f} it/s" for l, v in out["alternations"][-1].items() if v["it_per_s"]), file=sys.stderr)
if a.case == "slab8":
    out["n_own"] = int(s.plan_sizes.n_own)
s.close()
summary = {}
for loop in LOOPS:
    rs = [alt[loop] for alt in out["alternations"]]
    its = sorted(r["it_per_s"] for r in rs if r["it_per_s"])
    summary[loop] = {"it_per_s_median": its[len(its) // 2] if its else None, "it_per_s_all": its, "iterations": rs[-1]["iterations"],
                     "new_matrix_solve_ms_median": sorted(r["new_matrix_solve_ms"] for r in rs)[len(rs) // 2],
                     "resident": rs[-1]["resident"], "float_vectors": rs[-1]["float_vectors"],
                     "plan": {k: rs[-1].get(k) for k in ("NG", "lds_bytes", "workgroups", "vectors", "streamed_words_pct", "refused")}}
out["summary"] = summary
print(json.dumps(out, indent=1))
