"""AVS_OPTION_RESIDENT_LOCAL_TABLES: the header enumerator, the ctypes mirror and the environment variable the library reads agree (CPU)."""
import os
import re

from adaptiveviscositysolver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_value_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "avs.h")).read()
    m = re.search(r"^\s*AVS_OPTION_RESIDENT_LOCAL_TABLES\s*=\s*(\d+)", hdr, re.M)   # (the enumerator, not a mention in a comment)
    assert m and int(m.group(1)) == 13
    assert capi.OPTION_RESIDENT_LOCAL_TABLES == 13
    assert capi.OPTION_RESIDENT_F32 == 12
    assert not re.search(r"^\s*AVS_OPTION_\w+\s*=\s*11\b", hdr, re.M)           # 11 stays unassigned
    assert re.search(r"^#define AVS_ABI_VERSION 2$", hdr, re.M)              # no struct or entry changed


def test_environment_variable_is_read_and_documented():
    api = open(os.path.join(ROOT, "adaptiveviscositysolver_amd", "csrc", "avs_api.hip")).read()
    assert re.search(r'o\.resident_local_tables\s*=\s*env_int\("AVS_RESIDENT_LOCAL_TABLES",\s*0\)', api)     # default 0: opt-in
    assert re.search(r"case AVS_OPTION_RESIDENT_LOCAL_TABLES:\s*c->opt\.resident_local_tables", api)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "AVS_RESIDENT_LOCAL_TABLES" in readme


def test_the_kernel_variant_is_a_template_parameter():
    """the local-table loop is a further instantiation of k_cg_resident, not a run-time branch in the existing ones"""
    src = open(os.path.join(ROOT, "adaptiveviscositysolver_amd", "csrc", "avs_pcg_resident.inl")).read()
    assert re.search(r"template <int NG, bool STREAM, typename T, bool LT = false>\s*\n__global__ __launch_bounds__\(kResThreads\) void k_cg_resident", src)
    assert "k_resident_local_tables" in src
