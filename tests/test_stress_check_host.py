"""The host side of avs_check_stress_indices that needs no HIP call (csrc/avs_stress_check_report.hpp: argument checks, the key of the first
violation, report unpacking, the struct_size hand-over) under the host sanitizers: a stand-alone program with its own main, no GPU, no
library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_report_packing_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "stress_check_report")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "adaptiveviscositysolver_amd", "csrc"),
                           os.path.join(ROOT, "tests", "stress_check_report_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


def test_struct_layout_matches_the_binding(tmp_path):
    """sizeof and the offsets of avs_stress_check in C (gcc compiles include/avs.h as plain C) == the ctypes mirror"""
    import ctypes

    from adaptiveviscositysolver_amd import capi
    fields = ("passed", "violations", "first_rule", "first_level", "first_axis", "first_ijk", "active_edges", "active_centers")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "avs.h"\nint main(void){printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(avs_stress_check)'
                   + "".join(f", offsetof(avs_stress_check, {f})" for f in fields) + ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    T = capi.StressCheck
    assert got == [ctypes.sizeof(T)] + [getattr(T, f).offset for f in fields] == [120, 4, 8, 80, 84, 88, 92, 104, 112]
    assert (capi.CHECK_EDGE_INDICES, capi.CHECK_CENTER_INDICES, capi.STRESS_RULES) == (1, 2, 9)
    assert (capi.STRESS_RULE_EDGE_VALUE, capi.STRESS_RULE_EDGE_NUMBERING, capi.STRESS_RULE_CENTER_VALUE, capi.STRESS_RULE_CENTER_NUMBERING) == (0, 3, 4, 8)
    # the existing checker's constants are untouched
    assert (capi.CHECK_LABELS, capi.CHECK_VELOCITY_INDICES, capi.OCTREE_RULES, ctypes.sizeof(capi.OctreeCheck)) == (1, 2, 8, 96)
