"""The host side of avs_check_octree that needs no HIP call (csrc/avs_check_report.hpp: argument checks, the key of the first violation,
report packing, the struct_size hand-over) under the host sanitizers: a stand-alone program with its own main, no GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_report_packing_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "octree_check_report")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "adaptiveviscositysolver_amd", "csrc"),
                           os.path.join(ROOT, "tests", "octree_check_report_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


def test_struct_layout_matches_the_binding(tmp_path):
    """sizeof and the offsets of avs_octree_check in C (gcc compiles include/avs.h as plain C) == the ctypes mirror"""
    import ctypes

    from adaptiveviscositysolver_amd import capi
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "avs.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(avs_octree_check), '
                   'offsetof(avs_octree_check, passed), offsetof(avs_octree_check, violations), offsetof(avs_octree_check, first_rule), '
                   'offsetof(avs_octree_check, first_ijk));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    T = capi.OctreeCheck
    assert got == [ctypes.sizeof(T), T.passed.offset, T.violations.offset, T.first_rule.offset, T.first_ijk.offset] == [96, 4, 8, 72, 84]
    assert (capi.CHECK_LABELS, capi.CHECK_VELOCITY_INDICES, capi.OCTREE_RULES) == (1, 2, 8)
