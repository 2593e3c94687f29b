"""The device setFromTriplets (csrc/avs_assembly.hip) on the edge cases of tests/triplet_edges.py, through avs_merge_triplets_probe
(libavs_probe.so): the product's unique / scan / merge / merge-long steps on the caller's triplets, laid out the way the row sweep emits them.

The kernels perform the additions of tests/triplet_model.py in the same order, so row pointers, columns and the BITS of every value must
equal the model's -- no tolerance; the probe poisons the raw slots behind every row with quiet NaNs, so none may come out."""
import ctypes as C

import numpy as np
import pytest
import torch

import triplet_edges as E
import triplet_model as M
from adaptiveviscositysolver_amd import capi

pytestmark = pytest.mark.gpu

PAD = 64                  # entries behind the capacity that must stay as they were
COL_FILL, VAL_FILL = -7, -12345.0


def _run(c, f32, capacity):
    """-> status, nnz, info, row_ptr, col, val (nnz + PAD entries, or capacity + PAD of them)"""
    lib = capi.load_probe()
    dev = torch.device("cuda:0")
    ptr, col, val = c.arrays(f32)
    d_ptr, d_col, d_val = (torch.from_numpy(a).to(dev) for a in (ptr, col, val))
    o_rp = torch.full((c.n + 1,), -1, dtype=torch.int32, device=dev)
    o_col = torch.full((capacity + PAD,), COL_FILL, dtype=torch.int32, device=dev)
    o_val = torch.full((capacity + PAD,), VAL_FILL, dtype=torch.float64, device=dev)
    nnz = C.c_int64(-1)
    info = capi.TripletMergeInfo()
    status = lib.avs_merge_triplets_probe(c.n, d_ptr.data_ptr(), d_col.data_ptr(), d_val.data_ptr(), int(f32), o_rp.data_ptr(), o_col.data_ptr(),
                                          o_val.data_ptr(), capacity, C.byref(nnz), C.byref(info),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return status, nnz.value, info, o_rp.cpu().numpy(), o_col.cpu().numpy(), o_val.cpu().numpy()


@pytest.mark.parametrize("name,f32", E.RUNS, ids=[f"{n}-{'f32' if f else 'f64'}" for n, f in E.RUNS])
def test_merge_equals_the_model(name, f32, built_lib):
    c = E.by_name(name)
    L = E.limits()
    want_rp, want_col, want_val = c.model(f32)
    want_nnz = len(want_col)
    status, nnz, info, rp, col, val = _run(c, f32, want_nnz)
    capi.check(status)
    assert (info.fast_limit, info.wave_limit, info.merge_lds, info.scan_tile, info.long_grid_waves) == tuple(L)
    R = c.lengths()
    nw = (c.n + 63) // 64
    assert info.raw_slots == sum(64 * int(R[64 * w:64 * w + 64].max()) for w in range(nw))
    assert info.long_rows == c.long_rows
    assert nnz == want_nnz
    assert np.array_equal(rp, want_rp)
    assert np.array_equal(col[:nnz], want_col), np.nonzero(col[:nnz] != want_col)[0][:8]
    assert not np.isnan(val).any(), np.nonzero(np.isnan(val))[0][:8]
    bad = np.nonzero(M.bits(val[:nnz]) != M.bits(want_val))[0]
    assert len(bad) == 0, (len(bad), bad[:8], np.searchsorted(want_rp, bad[:8], side="right") - 1, val[bad[:4]], want_val[bad[:4]])
    assert np.all(col[nnz:] == COL_FILL) and np.all(val[nnz:] == VAL_FILL)


@pytest.mark.parametrize("name,f32", [("mix_all_paths", False), ("staged_plus_1", True), ("long_first", False)])
def test_small_capacity_is_refused(name, f32, built_lib):
    c = E.by_name(name)
    want_rp, want_col, _ = c.model(f32)
    for capacity in (len(want_col) - 1, 0):
        status, nnz, _, rp, col, val = _run(c, f32, capacity)
        assert status == capi.EINVAL
        assert nnz == len(want_col)                      # what the caller has to provide
        assert np.array_equal(rp, want_rp)
        assert np.all(col == COL_FILL) and np.all(val == VAL_FILL)
