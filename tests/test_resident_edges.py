"""The edge systems of tests/resident_edges.py are what their names say (host numpy, no GPU)."""
import numpy as np
import pytest

import csr_edges as E
import resident_edges as R


def _rows(c):
    return np.repeat(np.arange(c.n, dtype=np.int64), R.row_lengths(c))


@pytest.mark.parametrize("name", R.NAMES)
def test_case_is_what_its_name_says(name):
    c = R.get(name)
    assert c.name == name
    rp, col, val = c.row_ptr.astype(np.int64), c.col.astype(np.int64), c.val
    n, lens, rows = c.n, R.row_lengths(c), _rows(c)
    nnz = int(rp[-1])
    assert n <= 50000 and nnz <= 600000, (n, nnz)
    assert c.row_ptr.dtype == np.int32 and c.col.dtype == np.int32 and val.dtype == np.float64
    # columns sorted and distinct inside every row, every row with its diagonal
    inner = np.ones(nnz, dtype=bool)
    inner[rp[:-1]] = False
    assert np.all(np.diff(col)[inner[1:]] > 0)
    diag = rows == col
    assert np.array_equal(rows[diag], np.arange(n))
    # symmetric, off-diagonal entries in (-1, -0.25], diagonal = the row's length: strictly dominant
    key, back = rows * n + col, col * n + rows
    order, rorder = np.argsort(key), np.argsort(back)
    assert np.array_equal(key[order], back[rorder]) and np.array_equal(val[order], val[rorder])
    off = val[~diag]
    assert np.all(off > -1.0) and np.all(off <= -0.25)
    assert np.array_equal(val[diag], lens.astype(np.float64))
    offsum = np.bincount(rows[~diag], weights=np.abs(off), minlength=n)
    assert np.all(val[diag] > offsum)
    # the default plan takes it: the packed single dictionary of <= 1,023 values
    fmt = E.expected_format(c.row_ptr, c.col, val, {k: v for k, v in c.env.items() if k in ("AVS_VALUE_INDEX", "AVS_VALUE_PACK")})
    distinct = len(np.unique(val.view(np.uint64)))
    if c.props.get("many_values"):
        assert distinct > 2048 and c.env.get("AVS_RESIDENT_LOCAL_TABLES") == "1"
        assert not (fmt["column_bits"] > 0 and fmt["value_table_size"] <= 1023)
    else:
        assert distinct <= 1023 and fmt["column_bits"] > 0 and fmt["value_table_size"] == distinct and fmt["tile_local_tables"] == 0, fmt
    assert np.all(c.x0 != 0) and np.any(c.b != 0)
    # the facts of the name
    p = c.props
    if "n" in p:
        assert n == p["n"]
    if "row_lengths" in p:
        assert sorted(set(lens.tolist())) == sorted(p["row_lengths"])
    for r, L in p.get("arrows", {}).items():
        assert lens[r] == L, (r, lens[r], L)
    for r, cc in p.get("entries", []):
        assert cc in col[rp[r]:rp[r + 1]], (r, cc)
    if "all_parts_read_all" in p:
        assert R.parts_read(c, p["all_parts_read_all"]).all()
    if "permutation_of" in p:
        o = R.get(p["permutation_of"])
        assert np.array_equal(np.sort(R.row_lengths(o)), np.sort(lens)) and np.array_equal(np.sort(o.val), np.sort(val))
        assert not np.array_equal(R.row_lengths(o), lens)
    if "same_matrix_as" in p:
        o = R.get(p["same_matrix_as"])
        assert np.array_equal(o.row_ptr, c.row_ptr) and np.array_equal(o.col, c.col) and np.array_equal(o.val, c.val)


def test_lane_packing_cases_pack_as_claimed():
    """the lane counts the packing cases are named for, from the restated lane rule"""
    lens = lambda name: R.row_lengths(R.get(name))
    assert R.lanes_in_registers(lens("pack_rows6")) == (500, 0, 0)          # 6 one-quad rows per lane
    assert R.lanes_in_registers(lens("pack_25")) == (1000, 0, 0)            # 3 x 5 quads = 15
    assert R.lanes_in_registers(lens("pack_26")) == (1500, 0, 0)            # 2 x 6 quads, the third row does not fit
    la = lens("long_arrows")
    assert R.lanes_in_registers(la)[1:] == (5, 925)                          # tails 1, 2, 5, 75, 925
    assert sorted(int(v) - R.W for v in la[la > R.W]) == [1, 2, 5, 75, 925]
    assert R.lanes_in_registers(la, 1) == (3000, int((la > 5).sum()), 995)   # one quad: one row per lane, every longer row has a tail
    cyc = lens("pack_cycle")
    assert cyc[0] == 1 and cyc[80] == 4 and cyc[-1] == 75


def test_every_edge_of_the_issue_has_a_case():
    names = set(R.NAMES)
    for n in R.FEW_ROWS:
        assert {f"rows_{n}", f"rows_{n}_1cu"} <= names
    for ng in range(4):
        assert {f"tier_ng{ng}", f"tier_ng{ng}_stream"} <= names
    assert {"lt_workgroup", "lt_workgroup_stream", "lt_wave", "lt_wave_stream"} <= names
    assert len([x for x in names if x.startswith("decline_")]) == 4


def test_plan_struct_matches_header(tmp_path):
    """capi.ResidentPlanInfo mirrors avs_resident_plan_info of include/avs_probe.h: size and the offsets of the 64-bit fields and `why`"""
    import ctypes
    import os
    import subprocess

    from adaptiveviscositysolver_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = ("lanes", "streamed_rows", "streamed_words", "max_remote", "largest_table", "why")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "avs_probe.h"\nint main(void){printf("%zu", sizeof(avs_resident_plan_info));'
                   + "".join(f'printf(" %zu", offsetof(avs_resident_plan_info, {f}));' for f in fields) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(capi.ResidentPlanInfo)] + [getattr(capi.ResidentPlanInfo, f).offset for f in fields]
    assert [f for f, _ in capi.ResidentPlanInfo._fields_][0] == "struct_size"
