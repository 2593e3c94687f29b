"""The host side of avs_check_solution that needs no HIP call (csrc/avs_solution_check_report.hpp: argument checks, the order of the arg-max
pairs, the raw report turned into avs_solution_check, the struct_size hand-over) under the host sanitizers: a stand-alone program with its
own main, no GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_report_packing_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "solution_check_report")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "adaptiveviscositysolver_amd", "csrc"),
                           os.path.join(ROOT, "tests", "solution_check_report_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
