"""AVS_OPTION_RESIDENT_F32: the header enumerator, the ctypes mirror and the environment variable the library reads agree (CPU)."""
import os
import re

from adaptiveviscositysolver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_value_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "avs.h")).read()
    m = re.search(r"^\s*AVS_OPTION_RESIDENT_F32\s*=\s*(\d+)", hdr, re.M)   # (the enumerator, not a mention in a comment)
    assert m and int(m.group(1)) == 12
    assert capi.OPTION_RESIDENT_F32 == 12
    assert not re.search(r"^\s*AVS_OPTION_\w+\s*=\s*11\b", hdr, re.M)           # the value after DIST_F32_VECTORS stays unassigned
    assert re.search(r"^#define AVS_ABI_VERSION 2$", hdr, re.M)              # no struct or entry changed


def test_environment_variable_is_read_and_documented():
    api = open(os.path.join(ROOT, "adaptiveviscositysolver_amd", "csrc", "avs_api.hip")).read()
    assert re.search(r'o\.resident_f32\s*=\s*env_int\("AVS_RESIDENT_F32",\s*0\)', api)
    assert re.search(r"case AVS_OPTION_RESIDENT_F32:\s*c->opt\.resident_f32", api)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "AVS_RESIDENT_F32" in readme
