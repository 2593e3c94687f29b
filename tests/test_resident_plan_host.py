"""The host-only planner of the CU-resident PCG (csrc/avs_resident_plan.cpp) on the edge systems of tests/resident_edges.py, without a
GPU: avs_resident_plan_host (libavs_probe.so) forms the lanes of a case's row pointers and the plan's first workgroup split; the lanes
are checked against the lane rule restated in resident_edges.lanes_in_registers and against what the kernel relies on."""
import functools

import numpy as np
import pytest

import resident_edges as R
from adaptiveviscositysolver_amd import capi

STREAMED = [n for n in R.NAMES if n.endswith("_stream") and n.startswith(("tier_", "lt_"))]


@functools.lru_cache(maxsize=None)
def _planned(name):
    """(row lengths, workgroups, max_quads, info, lanes) of the case: built and planned once"""
    c = R.get(name)
    G = int(c.env.get("AVS_CG_RESIDENT_CUS", 256))
    max_quads = int(c.env.get("AVS_CG_RESIDENT_MAX_QUADS", R.QUADS))
    info, lanes = capi.resident_plan_host(c.row_ptr, G, max_quads, lane_fill=float(c.env.get("AVS_CG_RESIDENT_LANE_FILL", 0.90)),
                                          no_stream="AVS_CG_RESIDENT_NO_STREAM" in c.env,
                                          stream_cost=float(c.env.get("AVS_CG_RESIDENT_STREAM_COST", 1.5)))
    return R.row_lengths(c), G, max_quads, info, lanes


def test_streamed_cases_are_the_ones_named_so(built_lib):
    assert len(STREAMED) == 6 and {f"tier_ng{ng}_stream" for ng in range(4)} <= set(STREAMED)


@pytest.mark.parametrize("name", R.NAMES)
def test_host_plan_of_every_edge_case(built_lib, name):
    lens, G, max_quads, info, lanes = _planned(name)
    n, W = len(lens), max_quads * R.QUAD_WORDS
    if name == "decline_no_stream":
        assert info.refused and lanes is None
        assert R.get(name).expect["declined"] in info.why.decode()
        return
    assert not info.refused, info.why
    row0, meta = lanes["row0"].astype(np.int64), lanes["meta"]
    reg, m, tail = (meta & 7).astype(np.int64), ((meta >> 3) & 127).astype(np.int64), (meta >> 10).astype(np.int64)
    L = len(row0)
    assert L == info.lanes >= 1
    if info.streamed_rows == 0:     # the lane rule restated on the host
        assert (L, info.long_row_lanes, info.longest_tail) == R.lanes_in_registers(lens, max_quads)
        assert info.stream_T == 0.0 and info.streamed_words == 0
    # the lanes cover rows 0 .. n - 1 exactly once, in order
    assert row0[0] == 0 and np.array_equal(row0[1:], (row0 + reg + m)[:-1]) and row0[-1] + reg[-1] + m[-1] == n
    assert np.all(reg >= 1)
    # register rows <= 6 in <= max_quads quads; streamed rows <= 127; their quads and words as reported
    quads = -(-lens // R.QUAD_WORDS)
    cq, cw = np.concatenate([[0], np.cumsum(quads)]), np.concatenate([[0], np.cumsum(lens)])
    long_ = tail > 0
    assert np.all(reg <= R.ROWS_MAX) and np.all((cq[row0 + reg] - cq[row0])[~long_] <= max_quads)
    assert np.all(m <= 127) and m.max() == info.max_lane_streamed_rows and m.sum() == info.streamed_rows
    assert np.array_equal(cq[row0 + reg + m] - cq[row0 + reg], lanes["stream_quads"])
    assert (cw[row0 + reg + m] - cw[row0 + reg]).sum() == info.streamed_words
    # a long-row lane holds one row, and its tail is len - 5 max_quads; no other row is longer than the registers
    assert np.all(reg[long_] == 1) and np.all(m[long_] == 0) and np.array_equal(tail[long_], lens[row0[long_]] - W)
    assert long_.sum() == info.long_row_lanes == (lens > W).sum() - _streamed_long_rows(lens, row0, reg, m, W)
    assert info.longest_tail == (tail.max() if long_.any() else 0)
    # the first split: monotone, at most 1,024 lanes per workgroup, all lanes; wr[b] is the first row of lane wl[b]
    wl, wr = lanes["wl"].astype(np.int64), lanes["wr"].astype(np.int64)
    assert len(wl) == len(wr) == G + 1 and wl[0] == 0 and wl[-1] == L
    assert np.all(np.diff(wl) >= 0) and np.all(np.diff(wl) <= R.LANES)
    assert np.array_equal(wr, np.concatenate([row0, [n]])[wl])
    assert info.max_rows_per_workgroup == np.diff(wr).max()
    if name in STREAMED:
        assert L <= 0.97 * R.LANES * G and info.streamed_rows >= 1 and info.stream_T > 0.0


def _streamed_long_rows(lens, row0, reg, m, W):
    """rows longer than the registers that a lane streams (a stream takes any row of which it is owed half the quads)"""
    streamed = np.zeros(len(lens) + 1, dtype=np.int64)
    np.add.at(streamed, row0 + reg, 1)
    np.add.at(streamed, row0 + reg + m, -1)
    return int(((np.cumsum(streamed)[:-1] > 0) & (lens > W)).sum())


def test_host_plan_struct_matches_header(tmp_path):
    """capi.ResidentHostPlanInfo mirrors avs_resident_host_plan_info of include/avs_probe.h: size and the offset of every field"""
    import ctypes
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f for f, _ in capi.ResidentHostPlanInfo._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "avs_probe.h"\nint main(void){printf("%zu", sizeof(avs_resident_host_plan_info));'
                   + "".join(f'printf(" %zu", offsetof(avs_resident_host_plan_info, {f}));' for f in fields) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(capi.ResidentHostPlanInfo)] + [getattr(capi.ResidentHostPlanInfo, f).offset for f in fields]
    assert fields[0] == "struct_size"
