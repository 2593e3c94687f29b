"""k_update_fused (csrc/avs_pcg.hip) keeps its non-temporal hints in the INSTRUCTION STREAM of the shipped library.

Beyond the Infinity Cache (KEEP == false) the fused launch reads r, t, x and the diagonal codes and writes r and x with the `nt` bit: none
of them is read again before it is overwritten, and r in particular must not push the matrix form and p out of the cache in front of the
SpMV.  p stays plain (the SpMV reads it next).  With KEEP everything is left to the cache.  The hint is a template parameter; this is the
check that notices when the optimiser drops it (tools/isa_check.py; no GPU needed).

Per lane the kernel moves 2 x 8 pairs of rows per stream: 16 16-B loads each of r, t (phase 1), p, x (phase 2), 16 16-B stores each of
r, x, p, and -- coded diagonal -- 16 4-B code loads per phase."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_check  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(isa_check.LIB) or not os.path.exists(isa_check.LLVM + "/llvm-objdump"),
                                reason="needs the built library and llvm-objdump")

PAIRS = 16     # 2 * kFusedPairs: pairs of rows per lane and stream


def _ops(coded, keep):
    found = isa_check.kernels_matching(rf"avs::k_update_fused<{coded}, {keep}>")
    assert len(found) == 1, (coded, keep, list(found))
    (name, ins), = found.items()
    mem = [i for i in ins if i.startswith("global_")]

    def count(prefix, nt):
        return sum(1 for i in mem if i.split()[0] == prefix and (i.split()[-1] == "nt") == nt)
    return name, mem, count


@pytest.mark.parametrize("coded", ["true", "false"])
def test_streams_are_non_temporal_beyond_the_cache(coded):
    name, mem, count = _ops(coded, "false")
    assert count("global_load_dwordx4", True) >= 3 * PAIRS, (name, mem)      # r, t and x
    assert count("global_store_dwordx4", True) >= 2 * PAIRS, (name, mem)     # r and x
    assert count("global_load_dwordx4", False) >= PAIRS, (name, mem)         # p stays plain: the SpMV reads it next
    assert count("global_store_dwordx4", False) >= PAIRS, (name, mem)
    if coded == "true":
        assert count("global_load_dword", True) >= 2 * PAIRS, (name, mem)    # the codes of both phases


@pytest.mark.parametrize("coded", ["true", "false"])
def test_nothing_is_hinted_when_the_system_fits_the_cache(coded):
    name, mem, _ = _ops(coded, "true")
    assert len(mem) >= 7 * PAIRS, (name, mem)
    assert not [i for i in mem if i.split()[-1] == "nt"], (name, mem)


@pytest.mark.parametrize("keep", ["true", "false"])
@pytest.mark.parametrize("coded", ["true", "false"])
def test_no_scratch_and_five_workgroup_barriers(coded, keep):
    found = isa_check.kernels_matching(rf"avs::k_update_fused<{coded}, {keep}>")
    (name, ins), = found.items()
    assert not [i for i in ins if i.startswith("scratch_")], name
    # the fold at entry, the four sums of phase 1, in front of the ticket, behind the last poll, the beta fold
    assert sum(1 for i in ins if i.startswith("s_barrier")) == 5, name
