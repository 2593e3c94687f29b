// avs_check_report.hpp -- host side of avs_check_octree / avs_prepass_check_octree that needs no HIP call: argument checks, the layout of
// the raw report, and the report that goes back to the caller (the key of the first violation and the hand-over: avs_report.hpp).  Plain
// C++ over include/avs.h, so that a stand-alone program can run it under the host sanitizers (tests/octree_check_report_main.cpp).
#pragma once

#include "avs_report.hpp"

namespace avs {

// What the kernels leave behind: one 64-bit count per rule, then the smallest lattice_key of a violating entry (kNoKey: none).
constexpr int kCheckRawKey = AVS_OCTREE_RULES, kCheckRawWords = AVS_OCTREE_RULES + 1;

// AVS_OK, or AVS_EINVAL with *why set
inline avs_status check_octree_args(uint32_t what, const avs_octree_check *report, const char **why)
{
    if (!report) {
        *why = "octree check: report must not be null";
        return AVS_EINVAL;
    }
    if ((what & ~(uint32_t)(AVS_CHECK_LABELS | AVS_CHECK_VELOCITY_INDICES)) != 0) {
        *why = "octree check: unknown bits in `what`";
        return AVS_EINVAL;
    }
    if (!report_size_ok(report, offsetof(avs_octree_check, passed) + sizeof(int32_t))) {
        *why = "avs_octree_check.struct_size must be set to sizeof(avs_octree_check) before the call";
        return AVS_EINVAL;
    }
    return AVS_OK;
}

inline avs_octree_check check_octree_passed()
{
    avs_octree_check r;
    memset(&r, 0, sizeof(r));
    r.struct_size = (int32_t)sizeof(r);
    r.passed = 1;
    r.first_rule = r.first_level = r.first_axis = -1;
    r.first_ijk[0] = r.first_ijk[1] = r.first_ijk[2] = -1;
    return r;
}

// raw[kCheckRawWords] as the kernels wrote it; n: level-0 cells per axis.  Rules that were not asked for report 0.
inline avs_octree_check check_octree_report(const unsigned long long *raw, uint32_t what, const int n[3])
{
    avs_octree_check r = check_octree_passed();
    bool any = false;
    for (int rule = 0; rule < AVS_OCTREE_RULES; ++rule) {
        const bool asked = rule < AVS_RULE_INDEX_VALUE ? (what & AVS_CHECK_LABELS) != 0 : (what & AVS_CHECK_VELOCITY_INDICES) != 0;
        r.violations[rule] = asked ? (int64_t)raw[rule] : 0;
        any = any || r.violations[rule] != 0;
    }
    const unsigned long long key = raw[kCheckRawKey];
    if (!any || key == kNoKey) return r;
    r.passed = 0;
    r.first_rule = lattice_key_rule(key);
    r.first_level = lattice_key_level(key);
    r.first_axis = lattice_key_axis(key);
    const unsigned long long lin = lattice_key_lin(key);
    if (r.first_rule == AVS_RULE_NUMBERING) { // the entry is an id
        r.first_ijk[0] = (int32_t)lin;
        r.first_ijk[1] = r.first_ijk[2] = 0;
        return r;
    }
    lattice_entry_ijk(lin, n, r.first_level, r.first_rule >= AVS_RULE_INDEX_VALUE ? 1u << r.first_axis : 0u, r.first_ijk); // face lattice
    return r;
}

} // namespace avs
