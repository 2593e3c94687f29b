"""The float instantiations of k_sr_update_push (the direct transport's float-vector loop, csrc/avs_pcg.hip) keep the
ordering the protocol depends on: the halo entries leave with system-scope write-through stores, and an `s_waitcnt vmcnt(0)` sits
between the last of them and the barrier / ticket / flag (tools/isa_check.py disassembles the shipped library; no GPU needed)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_check  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(isa_check.LIB) or not os.path.exists(isa_check.LLVM + "/llvm-objdump"),
                                reason="needs the built library and llvm-objdump")

FLOAT_PUSH = r"^(void )?avs::k_sr_update_push<.*, float>\("


def test_float_update_push_exists():
    found = isa_check.kernels_matching(FLOAT_PUSH)
    assert len(found) >= 3, sorted(found)   # coded + brick, coded, plain inverse diagonal
    for k in found:
        assert "float*" in k, k


def test_float_update_push_stores_write_through_at_system_scope():
    for k, ins in isa_check.kernels_matching(FLOAT_PUSH).items():
        assert any(isa_check.is_remote_store(s) for s in ins), k
        ok, msg = isa_check.check_store_wait_sync(ins, isa_check.is_remote_store, isa_check.SYNC)
        assert ok, (k, msg)


def test_float_update_push_passes_the_library_checks():
    rows = isa_check.run_checks()
    mine = [(k, ok, m) for k, ok, m in rows if "k_sr_update_push<" in k and ", float>" in k]
    assert len(mine) >= 3, [k for k, _, _ in rows if "k_sr_update_push" in k]
    assert all(ok for _, ok, _ in mine), mine
    bad = [(k, m) for k, ok, m in rows if not ok]
    assert not bad, bad
