"""AVS_OPTION_MIXED_PRECISION: the header enumerator, the ctypes mirror, the environment variable the library reads and the new last field of
avs_matrix_format agree (CPU)."""
import os
import re

from adaptiveviscositysolver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_option_value_matches_the_header():
    hdr = _read("include", "avs.h")
    m = re.search(r"^\s*AVS_OPTION_MIXED_PRECISION\s*=\s*(\d+)", hdr, re.M)      # (the enumerator, not a mention in a comment)
    assert m and int(m.group(1)) == 14
    assert capi.OPTION_MIXED_PRECISION == 14
    assert not re.search(r"^\s*AVS_OPTION_\w+\s*=\s*11\b", hdr, re.M)           # 11 stays unassigned
    assert re.search(r"^#define AVS_ABI_VERSION 2$", hdr, re.M)              # the struct grew behind struct_size; no entry changed


def test_environment_variable_is_read_and_documented():
    api = _read("adaptiveviscositysolver_amd", "csrc", "avs_api.hip")
    assert re.search(r'o\.mixed_precision\s*=\s*env_int\("AVS_MIXED_PRECISION",\s*0\)', api)     # default 0: opt-in
    assert re.search(r"case AVS_OPTION_MIXED_PRECISION:\s*c->opt\.mixed_precision", api)
    readme = _read("README.md")
    assert re.search(r"^\|[^\n]*AVS_MIXED_PRECISION[^\n]*\|\s*$", readme, re.M)                  # a row of the switch table
    assert "AVS_OPTION_MIXED_PRECISION" in _read("INTEGRATION.md")
    assert "AVS_OPTION_MIXED_PRECISION" in _read("DESIGN.md")


def test_reliable_updates_is_the_last_field_of_the_matrix_format():
    names = [f[0] for f in capi.MatrixFormat._fields_]
    assert names[-1] == "reliable_updates" and names[-2] == "float_vectors"
    hdr = _read("include", "avs.h")
    body = re.search(r"typedef struct avs_matrix_format \{(.*?)\} avs_matrix_format;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(?:int32_t|int64_t)\s+(\w+)\s*;", body)
    assert fields[-1] == "reliable_updates" and fields[-2] == "float_vectors"
    assert fields == [n for n in names if n != "_pad"]                          # the ctypes mirror lists the header's fields in order


def test_the_value_type_is_a_template_parameter_of_the_kernels():
    """the mixed product is a further instantiation of the float kernels (fp64 values next to float vectors), not a copy"""
    brick = _read("adaptiveviscositysolver_amd", "csrc", "avs_brick.hip")
    assert re.search(r"template <bool DOT, bool VC = false, typename T = double, typename V = T>\s*\n__global__[^\n]*void k_spmv_brick", brick)
    f32 = _read("adaptiveviscositysolver_amd", "csrc", "avs_pcg_f32.inl")
    assert re.search(r"template <bool DOT, typename V = float>\s*\n__global__[^\n]*void k_f32_spmv_csr", f32)
    # the vector kernels: one body each, the vector type T and the scalar type S are template parameters (mixed: <float, double>)
    pcg = _read("adaptiveviscositysolver_amd", "csrc", "avs_pcg.hip")
    assert re.search(r"template <typename T, typename S, bool CODED, bool FUSED, bool KEEP>\s*\n__global__[^\n]*void k_update_r\(", pcg)
    assert re.search(r"template <typename T, typename S, bool CODED, bool FUSED, bool KEEP>\s*\n__global__[^\n]*void k_update_xp\(", pcg)
    assert len(re.findall(r"void k_update_r\(", pcg)) == 1 and len(re.findall(r"void k_update_xp\(", pcg)) == 1
    for name in sorted(os.listdir(os.path.join(ROOT, "adaptiveviscositysolver_amd", "csrc"))):   # (the sources: not what a build leaves there)
        if name.endswith((".hip", ".inl", ".hpp", ".cpp", ".h")):
            text = _read("adaptiveviscositysolver_amd", "csrc", name)
            assert "k_f32_update_r" not in text and "k_f32_update_xp" not in text, name
    mixed = _read("adaptiveviscositysolver_amd", "csrc", "avs_pcg_mixed.inl")
    assert "k_mixed_fold" in mixed and "k_mixed_residual" in mixed
    assert '#include "avs_pcg_mixed.inl"' in _read("adaptiveviscositysolver_amd", "csrc", "avs_pcg.hip")
