"""The host side of avs_check_csr that needs no HIP call (csrc/avs_csr_check_report.hpp: argument checks, the key of the first violation,
the raw report turned into avs_csr_check, the struct_size hand-over) under the host sanitizers: a stand-alone program with its own main,
no GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_report_packing_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "csr_check_report")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "adaptiveviscositysolver_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csr_check_report_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


def test_struct_layout_matches_the_binding(tmp_path):
    """sizeof and the offsets of avs_csr_check in C (gcc compiles include/avs.h as plain C) == the ctypes mirror"""
    import ctypes

    from adaptiveviscositysolver_amd import capi
    fields = ["passed", "evaluated", "first_rule", "first_index", "first_row", "first_col", "violations", "empty_rows", "longest_row",
              "asymmetric_entries", "max_abs_value", "max_abs_asymmetry"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "avs.h"\nint main(void){printf("%zu", sizeof(avs_csr_check));\n'
                   + "".join(f'printf(" %zu", offsetof(avs_csr_check, {f}));\n' for f in fields)
                   + 'printf(" %d %d %d %d %d %d\\n", AVS_CSR_CHECK_VALUES, AVS_CSR_CHECK_ORDER, AVS_CSR_CHECK_DIAGONAL, AVS_CSR_CHECK_SYMMETRY, '
                     'AVS_CSR_CHECK_ALL, AVS_CSR_RULES);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    T = capi.CsrCheck
    assert got[:13] == [ctypes.sizeof(T)] + [getattr(T, f).offset for f in fields] == [136, 4, 8, 12, 16, 24, 28, 32, 96, 104, 112, 120, 128]
    assert got[13:] == [capi.CSR_CHECK_VALUES, capi.CSR_CHECK_ORDER, capi.CSR_CHECK_DIAGONAL, capi.CSR_CHECK_SYMMETRY, capi.CSR_CHECK_ALL,
                        capi.CSR_RULES] == [1, 2, 4, 8, 15, 8]
    assert (capi.CSR_RULE_ROW_PTR, capi.CSR_RULE_COLUMN, capi.CSR_RULE_VALUE, capi.CSR_RULE_VECTOR, capi.CSR_RULE_ORDER, capi.CSR_RULE_DIAGONAL,
            capi.CSR_RULE_PATTERN, capi.CSR_RULE_SYMMETRY) == tuple(range(8))
    assert capi.CsrCheck().struct_size == 136


def test_model_and_binding_name_the_same_bits():
    import csr_check_model as m
    from adaptiveviscositysolver_amd import capi
    assert (m.VALUES, m.ORDER, m.DIAGONAL, m.SYMMETRY, m.ALL) == (capi.CSR_CHECK_VALUES, capi.CSR_CHECK_ORDER, capi.CSR_CHECK_DIAGONAL,
                                                                  capi.CSR_CHECK_SYMMETRY, capi.CSR_CHECK_ALL)
    assert (m.ROW_PTR, m.COLUMN, m.VALUE, m.VECTOR, m.ORDER_RULE, m.DIAGONAL_RULE, m.PATTERN, m.SYMMETRY_RULE) == tuple(range(8)) and m.RULES == capi.CSR_RULES
