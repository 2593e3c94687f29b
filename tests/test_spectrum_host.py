"""The host side of avs_estimate_spectrum that needs no HIP call (csrc/avs_spectrum_report.hpp: argument checks, the eigenvalues of the
Lanczos tridiagonal and the last components of its extreme eigenvectors, the bounds, the raw words turned into avs_spectrum, the
struct_size hand-over, iteration_bound at its edges) under the host sanitizers: a stand-alone program with its own main, no GPU, no
library.  The tridiagonals are the model's (tests/spectrum_model.py) and a random one of 512 steps; their eigenvalues are numpy's, written
into a small header of constants; the program compares within 4 k 2^-52 |T|_inf -- both methods are backward stable to O(k) eps |T|."""
import os
import subprocess

import numpy as np

import spectrum_cases as sc
import spectrum_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FROM_THE_MODEL = [("tri_12", M.JACOBI), ("tri_12", M.MATRIX), ("tri_257", M.MATRIX), ("blocks", M.JACOBI), ("laplace_1000", M.MATRIX), ("indefinite", M.MATRIX),
                  ("n_1", M.JACOBI), ("identity_600", M.JACOBI)]


def tridiagonals():
    out = []
    for name, op in FROM_THE_MODEL:
        m = sc.model(name, op)
        k = m["steps_taken"]
        out.append((k, m["alpha"][:k], m["beta"][:k + 1]))
    rng = np.random.default_rng(9400)
    out.append((512, rng.standard_normal(512), np.abs(rng.standard_normal(513)) + 0.01))
    out.append((3, np.array([1.0, 1.0, 1.0]), np.array([1.0, 1e-9, 1e-9, 0.5])))       # a near-triple eigenvalue
    return out


def constants():
    lines = ["struct TriCase { int k; const double *alpha, *beta, *ritz; double last_min, last_max, gap_min, gap_max; };"]
    array = lambda name, a: lines.append(f"static const double {name}[] = {{{', '.join(float(v).hex() for v in a)}}};")
    rows = []
    for t, (k, alpha, beta) in enumerate(tridiagonals()):
        theta, z = np.linalg.eigh(M.tridiagonal(alpha, beta, k))
        gap_min = theta[1] - theta[0] if k > 1 else 1.0
        gap_max = theta[-1] - theta[-2] if k > 1 else 1.0
        array(f"kAlpha{t}", alpha)
        array(f"kBeta{t}", beta)
        array(f"kRitz{t}", theta)
        rows.append(f"{{{k}, kAlpha{t}, kBeta{t}, kRitz{t}, {float(abs(z[-1, 0])).hex()}, {float(abs(z[-1, -1])).hex()}, {float(gap_min).hex()}, "
                    f"{float(gap_max).hex()}}}")
    lines.append(f"static const TriCase kTriCases[] = {{{', '.join(rows)}}};")
    lines.append(f"static const int kTriCaseCount = {len(rows)};")
    array("kHashEntry", M.hash_vector(65537)[[0, 1, 255, 65536]])
    return "\n".join(lines) + "\n"


def test_report_and_tridiagonal_step_under_asan_and_ubsan(tmp_path):
    (tmp_path / "spectrum_report_constants.hpp").write_text(constants())
    exe = str(tmp_path / "spectrum_report")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "adaptiveviscositysolver_amd", "csrc"), "-I", str(tmp_path),
                           os.path.join(ROOT, "tests", "spectrum_report_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
