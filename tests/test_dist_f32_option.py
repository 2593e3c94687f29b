"""AVS_OPTION_DIST_F32_VECTORS: the ctypes mirror matches include/avs.h (CPU), and the library accepts the option (every entry of the
product needs a context, hence the GPU)."""
import os
import re

import pytest

from adaptiveviscositysolver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_value_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "avs.h")).read()
    m = re.search(r"^\s*AVS_OPTION_DIST_F32_VECTORS\s*=\s*(\d+)", hdr, re.M)   # (the enumerator, not a mention in a comment)
    assert m and int(m.group(1)) == 10
    assert capi.OPTION_DIST_F32_VECTORS == 10
    assert "float_vectors" in [f for f, _ in capi.MatrixFormat._fields_]
    assert re.search(r"int32_t\s+float_vectors;", hdr)


@pytest.mark.gpu
def test_set_solver_option_accepts_it(built_lib):
    from adaptiveviscositysolver_amd import ViscositySolve, scenes
    sc = scenes.fat_beam(16, 2)
    s = ViscositySolve(sc.res, sc.dx, sc.dt, sc.levels, device=0, precision=capi.PRECISION_F32)
    try:
        for v in (1, 0):
            s.set_solver_option(capi.OPTION_DIST_F32_VECTORS, v)
        with pytest.raises(capi.AvsError):   # the next value is not an option (yet)
            s.set_solver_option(capi.OPTION_DIST_F32_VECTORS + 1, 1)
    finally:
        s.close()
