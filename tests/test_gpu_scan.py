"""exclusive_scan_i32 (csrc/avs_assembly.hip) -- the scan behind the assembly, the renumbering, the brick build, the pre-pass, the octree cells
and the partition plan -- against np.cumsum in int64, through avs_exclusive_scan_probe (libavs_probe.so): around the wave, the workgroup and
the 2048-element tile, where the single-block top pass starts to loop (more than 256 tiles), and the report of a total above INT32_MAX."""
import ctypes as C

import numpy as np
import pytest
import torch

import triplet_edges as E
from adaptiveviscositysolver_amd import capi

pytestmark = pytest.mark.gpu

TOP = 256 * 2048          # elements one trip of the top pass covers
SIZES = (0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, TOP, TOP + 1, 2 * TOP + 5)
INT32_MAX = 2 ** 31 - 1


def _scan(values):
    lib = capi.load_probe()
    dev = torch.device("cuda:0")
    n = len(values)
    d_in = torch.from_numpy(np.ascontiguousarray(values, np.int32)).to(dev)
    d_out = torch.full((n + 1 + 8,), -77, dtype=torch.int32, device=dev)
    capi.check(lib.avs_exclusive_scan_probe(d_in.data_ptr() if n else None, d_out.data_ptr(), n,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(out[n + 1:] == -77)
    return out[:n + 1]


def _want(values):
    return np.concatenate([[0], np.cumsum(np.asarray(values, np.int64))])


def test_sizes_sit_at_the_compiled_tile(built_lib):
    assert E.limits().tile * E.TOP_TILES == TOP


@pytest.mark.parametrize("n", SIZES)
def test_scan_equals_cumsum(n, built_lib):
    rng = np.random.default_rng(1000 + n)
    for values in (rng.integers(0, 101, n), np.zeros(n, np.int64)):
        got = _scan(values)
        want = _want(values)
        assert got[n] == want[n]                              # out[n] is the total
        assert np.array_equal(got.astype(np.int64), want), np.nonzero(got != want)[0][:8]


def test_total_above_int32_is_reported(built_lib):
    """2^20 entries of 2048: every tile's own sum is 2^22, the total exactly 2^31 -> out[n] == -1 (only out[n] is defined then).  One entry
    lowered by one: INT32_MAX, reported exactly, every prefix right."""
    n = 2 ** 20
    values = np.full(n, 2048, np.int64)
    assert values.sum() == INT32_MAX + 1 and values[:2048].sum() < 2 ** 31
    assert _scan(values)[n] == -1
    values[n // 2 + 3] = 2047
    assert values.sum() == INT32_MAX
    got = _scan(values)
    assert got[n] == INT32_MAX
    assert np.array_equal(got.astype(np.int64), _want(values))
