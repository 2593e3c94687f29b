"""AVS_OPTION_DIST_MIXED_PRECISION: the header enumerator, the ctypes mirror, the environment variable and the documents agree (CPU), and
the library accepts the option (every entry of the product needs a context, hence the GPU)."""
import os
import re

import pytest

from adaptiveviscositysolver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_option_value_matches_the_header():
    hdr = _read("include", "avs.h")
    m = re.search(r"^\s*AVS_OPTION_DIST_MIXED_PRECISION\s*=\s*(\d+)", hdr, re.M)   # (the enumerator, not a mention in a comment)
    assert m and int(m.group(1)) == 15
    assert capi.OPTION_DIST_MIXED_PRECISION == 15
    assert not re.search(r"^\s*AVS_OPTION_\w+\s*=\s*11\b", hdr, re.M)             # 11 stays unassigned
    assert re.search(r"^#define AVS_ABI_VERSION 2$", hdr, re.M)


def test_reliable_updates_is_still_the_last_field_of_the_matrix_format():
    names = [f[0] for f in capi.MatrixFormat._fields_]
    assert names[-1] == "reliable_updates" and names[-2] == "float_vectors"
    body = re.search(r"typedef struct avs_matrix_format \{(.*?)\} avs_matrix_format;", _read("include", "avs.h"), re.S).group(1)
    fields = re.findall(r"\b(?:int32_t|int64_t)\s+(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields[-1] == "reliable_updates" and fields == [n for n in names if n != "_pad"]


def test_environment_variable_is_read_and_documented():
    api = _read("adaptiveviscositysolver_amd", "csrc", "avs_api.hip")
    assert re.search(r'o\.dist_mixed_precision\s*=\s*env_int\("AVS_DIST_MIXED_PRECISION",\s*0\)', api)     # default 0: opt-in
    assert re.search(r"case AVS_OPTION_DIST_MIXED_PRECISION:\s*c->opt\.dist_mixed_precision", api)
    assert re.search(r"^\|[^\n]*AVS_DIST_MIXED_PRECISION[^\n]*\|\s*$", _read("README.md"), re.M)           # a row of the switch table
    assert "AVS_OPTION_DIST_MIXED_PRECISION" in _read("INTEGRATION.md")
    design = _read("DESIGN.md")
    assert "AVS_OPTION_DIST_MIXED_PRECISION" in design
    assert "the partitioned loops have no mixed-precision form" not in design


def test_the_scalar_type_is_a_parameter_of_the_update_kernels():
    """the mixed loops launch further instantiations of the single-reduction update kernels (scalar type double next to float vectors),
    not copies"""
    pcg = _read("adaptiveviscositysolver_amd", "csrc", "avs_pcg.hip")
    assert re.search(r"template <typename T, bool CODED, typename S = T>\s*\n__global__[^\n]*void k_sr_update\(", pcg)
    assert re.search(r"template <bool CODED, bool KEEP = true, typename T = double, typename S = T>\s*\n__global__[^\n]*void k_sr_update_push\(", pcg)
    # both loops name the scalar type once (double for MIXED) and hand it to the kernel they launch for every precision
    assert len(re.findall(r"typedef typename std::conditional<MIXED, double, T>::type SS;", pcg)) == 2
    assert re.search(r"\(k_sr_update<T, [^<>]*, SS>\)", pcg) and re.search(r"\(k_sr_update_push<[^<>]*, T, SS>\)", pcg)
    assert not re.search(r"void k_sr_mixed_update", pcg) and "k_sr_mixed_residual" in pcg


@pytest.mark.gpu
def test_set_solver_option_accepts_it(built_lib):
    from adaptiveviscositysolver_amd import ViscositySolve, scenes
    sc = scenes.fat_beam(16, 2)
    s = ViscositySolve(sc.res, sc.dx, sc.dt, sc.levels, device=0)
    try:
        for v in (1, 0):
            s.set_solver_option(capi.OPTION_DIST_MIXED_PRECISION, v)
        with pytest.raises(capi.AvsError):   # the next value is not an option (yet)
            s.set_solver_option(capi.OPTION_DIST_MIXED_PRECISION + 1, 1)
    finally:
        s.close()
