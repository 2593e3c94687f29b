"""avs_estimate_spectrum on the 512^3 four-level fat beam, the 1024^3 thin sheet and the two small scenes of tests/test_gpu_spectrum.py:
  * HIP-event time of one call of 32 and of 64 steps (the context runs on a stream torch knows, the events bracket the call on that
    stream; median of 5 calls after one warm-up), per step as (t64 - t32) / 32 and as t64 / 64, beside the estimated traffic per step
    12 nnz + 4 n + 80 n bytes and the floor that traffic has at the 6.29 TB/s this project measures as achievable;
  * the Ritz extremes of the Jacobi-scaled operator and of the matrix after 64 steps from the scaled initial residual, their bounds, the
    Gershgorin bound, the condition estimate and iteration_bound at 1e-3 and 1e-8, beside the iterations avs_solve really took to those
    tolerances (Eigen's residual rule, not the A-norm bound: they measure different things);
  * `spreads`: no GPU -- the spread of the extreme Ritz values of tests/spectrum_cases.py between forward and reverse sums
    (tests/spectrum_model.py), what the tolerances of tests/test_gpu_spectrum.py are measured against.
`python tools/probes/spectrum_probe.py [--out profiles/spectrum.md] [beam512] [sheet1024] [beam32_L3] [sphere32] [spreads]` prints one JSON line
per scene and writes the report."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ACHIEVABLE_BYTES_PER_MS = 6.29e12 / 1e3
SCENES = {
    "beam512": ("512³ fat beam, 4 levels", lambda sc, dev: sc.fat_beam(512, 4, device=dev)),
    "sheet1024": ("1024³ thin sheet", lambda sc, dev: sc.thin_sheet(1024, 5, thickness_cells=32, device=dev)),
    "beam32_L3": ("`beam32_L3`", lambda sc, dev: sc.to_device(sc.fat_beam(32, 3), dev)),
    "sphere32": ("`sphere32`", lambda sc, dev: sc.to_device(sc.sphere(32, 3), dev)),
}


def scene_figures(name):
    import torch

    from adaptiveviscositysolver_amd import DevicePrepass, ViscositySolve, capi, scenes

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    sc = SCENES[name][1](scenes, dev)
    torch.cuda.synchronize()
    pp = DevicePrepass(sc.res, sc.dx, sc.levels, stream=stream.cuda_stream)
    info = pp.run(sc.liquid, sc.solid)
    s = ViscositySolve(sc.res, sc.dx, sc.dt, info.levels, device=0, stream=stream.cuda_stream)
    pp.apply(s)
    s.set_scene_fields(sc)
    ainfo = s.assemble()
    out = {"scene": name, "levels": int(info.levels), "n": int(ainfo.n_velocity)}
    rep = capi.Spectrum()
    lib, h = s.lib, s.h

    def estimate(op, steps, tolerance, start=capi.SPECTRUM_START_RESIDUAL):
        capi.check(lib.avs_estimate_spectrum(h, op, start, steps, tolerance, None, None, None, None, None, capi.MEM_DEVICE, C.byref(rep)))

    for steps in (32, 64):
        ms = []
        for k in range(6):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record(stream)
            estimate(capi.SPECTRUM_OF_JACOBI, steps, 1e-3)
            b.record(stream)
            b.synchronize()
            if k >= 1:
                ms.append(a.elapsed_time(b))
        out[f"steps{steps}_event_ms"] = round(statistics.median(ms), 4)
        out[f"steps{steps}_event_ms_min_max"] = [round(min(ms), 4), round(max(ms), 4)]
        out[f"steps{steps}_taken"] = int(rep.steps_taken)
    out["nnz"] = int(rep.nnz)
    for op, label in ((capi.SPECTRUM_OF_JACOBI, "jacobi"), (capi.SPECTRUM_OF_MATRIX, "matrix")):
        for tolerance in (1e-3, 1e-8):
            estimate(op, 64, tolerance)
            out[f"{label}_iteration_bound_{tolerance:g}"] = int(rep.iteration_bound)
        out[label] = dict(steps_taken=int(rep.steps_taken), breakdown=int(rep.breakdown), indefinite=int(rep.indefinite), lambda_min=rep.lambda_min,
                          lambda_min_bound=rep.lambda_min_bound, lambda_max=rep.lambda_max, lambda_max_bound=rep.lambda_max_bound,
                          gershgorin_max=rep.gershgorin_max, condition_estimate=rep.condition_estimate)
    for tolerance in (1e-3, 1e-8):
        solve = s.solve(tolerance, 5000)
        out[f"solve_iterations_{tolerance:g}"] = int(solve.iterations)
        out[f"solve_converged_{tolerance:g}"] = int(solve.converged)
    per_step_bytes = 12 * out["nnz"] + 4 * out["n"] + 80 * out["n"]
    out.update(per_step_bytes=per_step_bytes, floor_ms_per_step=round(per_step_bytes / ACHIEVABLE_BYTES_PER_MS, 4),
               marginal_ms_per_step=round((out["steps64_event_ms"] - out["steps32_event_ms"]) / 32, 4),
               mean_ms_per_step=round(out["steps64_event_ms"] / 64, 4))
    s.close()
    pp.close()
    del sc
    torch.cuda.empty_cache()
    return out


def spreads():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import spectrum_cases as cases
    return [(name, op, cases.case(name).steps, cases.model(name, op)["steps_taken"]) + cases.spread(name, op) for name, op in cases.runs()]


def report(command, figures, spread_rows):
    g = lambda v: f"{v:.6g}"
    lines = ["# Spectrum estimate (`avs_estimate_spectrum`, `avs_estimate_csr_spectrum`; `csrc/avs_spectrum.hip`)", "",
             f"Written by `{command}`.  All device numbers: 1× MI355X; HIP events around the call on the context's stream, median of 5 calls after",
             "one warm-up, min–max in brackets.  No pass/fail bar on time: the figures are recorded.", ""]
    if figures:
        lines += ["## Time of a call (Jacobi-scaled operator, start = scaled initial residual, no array output)", "",
                  "| scene | n | nnz | 32 steps: event ms | 64 steps: event ms | ms per step, (t64 − t32) / 32 | ms per step, t64 / 64 | estimated bytes per step, "
                  "12·nnz + 84·n | floor at 6.29 TB/s: ms per step | marginal / floor |", "|---|---|---|---|---|---|---|---|---|---|"]
        for f in figures:
            lo32, hi32 = f["steps32_event_ms_min_max"]
            lo64, hi64 = f["steps64_event_ms_min_max"]
            lines.append(f"| {SCENES[f['scene']][0]} | {f['n']:,} | {f['nnz']:,} | {f['steps32_event_ms']} [{lo32}–{hi32}] | {f['steps64_event_ms']} [{lo64}–{hi64}] | "
                         f"{f['marginal_ms_per_step']} | {f['mean_ms_per_step']} | {f['per_step_bytes']:,} | {f['floor_ms_per_step']} | "
                         f"{f['marginal_ms_per_step'] / f['floor_ms_per_step']:.2f} |" if f["floor_ms_per_step"] else "")
        lines += ["", "The traffic per step is an estimate (the matrix once, about ten vector passes), not a counter reading; the small scenes fit the caches and",
                  "are bound by their five launches per step, not by bytes.", "",
                  "## Spectra after 64 steps, and the iterations the solve really took", "",
                  "| scene | operator | steps taken | λ_min (± bound) | λ_max (± bound) | Gershgorin | condition estimate (a lower bound) | iteration_bound 1e-3 | "
                  "`avs_solve` 1e-3 | iteration_bound 1e-8 | `avs_solve` 1e-8 |", "|---|---|---|---|---|---|---|---|---|---|---|"]
        for f in figures:
            for label, text in (("jacobi", "D^-1/2 A D^-1/2"), ("matrix", "A")):
                r = f[label]
                took = lambda t: f"{f[f'solve_iterations_{t:g}']:,}" + ("" if f[f"solve_converged_{t:g}"] else " (not converged)")
                lines.append(f"| {SCENES[f['scene']][0]} | {text} | {r['steps_taken']}{' (breakdown)' if r['breakdown'] else ''} | {g(r['lambda_min'])} (± {g(r['lambda_min_bound'])}) | "
                             f"{g(r['lambda_max'])} (± {g(r['lambda_max_bound'])}) | {g(r['gershgorin_max'])} | {g(r['condition_estimate'])} | "
                             f"{f[f'{label}_iteration_bound_0.001']:,} | {took(1e-3) if label == 'jacobi' else '–'} | {f[f'{label}_iteration_bound_1e-08']:,} | "
                             f"{took(1e-8) if label == 'jacobi' else '–'} |")
        lines += ["", "`avs_solve` is Jacobi-preconditioned and stops by Eigen's residual rule; iteration_bound is the A-norm bound from a LOWER bound of the",
                  "condition number after 64 steps (λ_min converges from above): the two columns are beside each other, not the same quantity.", ""]
    if spread_rows:
        lines += ["## Spread of the extreme Ritz values between summation orders (CPU, `tests/spectrum_model.py`)", "",
                  "Relative difference between the model run with forward and with reverse sums; `tests/test_gpu_spectrum.py` allows the device 8 × this,",
                  "at least 64 · 2^-52, against the model run with exact sums.  0: no step, or a stop before any difference could show.", "",
                  "| case | operator | steps asked | steps taken | λ_min | λ_max | Ritz values / largest |", "|---|---|---|---|---|---|---|"]
        for name, op, steps, taken, lo, hi, ritz in spread_rows:
            lines.append(f"| `{name}` | {'A' if op else 'D^-1/2 A D^-1/2'} | {steps} | {taken} | {lo:.2e} | {hi:.2e} | {ritz:.2e} |")
        lines.append("")
    return "\n".join(lines)


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "spectrum.md")
    if "--out" in args:
        at = args.index("--out")
        out_path = args[at + 1]
        del args[at:at + 2]
    names = args or list(SCENES) + ["spreads"]
    figures = []
    for name in names:
        if name != "spreads":
            figures.append(scene_figures(name))
            print(json.dumps(figures[-1]), flush=True)
    text = report("python tools/probes/spectrum_probe.py " + " ".join(sys.argv[1:]), figures, spreads() if "spreads" in names else [])
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
