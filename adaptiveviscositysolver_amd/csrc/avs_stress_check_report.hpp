// avs_stress_check_report.hpp -- host side of avs_check_stress_indices / avs_prepass_check_stress_indices that needs no HIP call: argument
// checks, the layout of the raw report, and the report that goes back to the caller (the key of the first violation and the hand-over:
// avs_report.hpp).  Plain C++ over include/avs.h, so that a stand-alone program can run it under the host sanitizers
// (tests/stress_check_report_main.cpp).
#pragma once

#include "avs_report.hpp"

namespace avs {

// What the kernels leave behind: one 64-bit count per rule, the smallest lattice_key of a violating entry (kNoKey: none), then the number
// of edge and of centre entries that carry an id.
constexpr int kStressRawKey = AVS_STRESS_RULES, kStressRawEdges = AVS_STRESS_RULES + 1, kStressRawCenters = AVS_STRESS_RULES + 2;
constexpr int kStressRawWords = AVS_STRESS_RULES + 3;

// AVS_OK, or AVS_EINVAL with *why set
inline avs_status check_stress_args(uint32_t what, const avs_stress_check *report, const char **why)
{
    if (!report) {
        *why = "stress index check: report must not be null";
        return AVS_EINVAL;
    }
    if ((what & ~(uint32_t)(AVS_CHECK_EDGE_INDICES | AVS_CHECK_CENTER_INDICES)) != 0) {
        *why = "stress index check: unknown bits in `what`";
        return AVS_EINVAL;
    }
    if (!report_size_ok(report, offsetof(avs_stress_check, passed) + sizeof(int32_t))) {
        *why = "avs_stress_check.struct_size must be set to sizeof(avs_stress_check) before the call";
        return AVS_EINVAL;
    }
    return AVS_OK;
}

inline avs_stress_check check_stress_passed()
{
    avs_stress_check r;
    memset(&r, 0, sizeof(r));
    r.struct_size = (int32_t)sizeof(r);
    r.passed = 1;
    r.first_rule = r.first_level = r.first_axis = -1;
    r.first_ijk[0] = r.first_ijk[1] = r.first_ijk[2] = -1;
    return r;
}

inline bool stress_rule_is_edge(int rule) { return rule <= AVS_STRESS_RULE_EDGE_NUMBERING; }

// raw[kStressRawWords] as the kernels wrote it; n: level-0 cells per axis.  Rules and counts that were not asked for report 0.
inline avs_stress_check check_stress_report(const unsigned long long *raw, uint32_t what, const int n[3])
{
    avs_stress_check r = check_stress_passed();
    bool any = false;
    for (int rule = 0; rule < AVS_STRESS_RULES; ++rule) {
        const bool asked = (what & (stress_rule_is_edge(rule) ? AVS_CHECK_EDGE_INDICES : AVS_CHECK_CENTER_INDICES)) != 0;
        r.violations[rule] = asked ? (int64_t)raw[rule] : 0;
        any = any || r.violations[rule] != 0;
    }
    r.active_edges = (what & AVS_CHECK_EDGE_INDICES) ? (int64_t)raw[kStressRawEdges] : 0;
    r.active_centers = (what & AVS_CHECK_CENTER_INDICES) ? (int64_t)raw[kStressRawCenters] : 0;
    const unsigned long long key = raw[kStressRawKey];
    if (!any || key == kNoKey) return r;
    r.passed = 0;
    r.first_rule = lattice_key_rule(key);
    r.first_level = lattice_key_level(key);
    r.first_axis = lattice_key_axis(key);
    const unsigned long long lin = lattice_key_lin(key);
    if (r.first_rule == AVS_STRESS_RULE_EDGE_NUMBERING || r.first_rule == AVS_STRESS_RULE_CENTER_NUMBERING) { // the entry is an id
        r.first_ijk[0] = (int32_t)lin;
        r.first_ijk[1] = r.first_ijk[2] = 0;
        return r;
    }
    // edge lattice: one more on the two other axes
    lattice_entry_ijk(lin, n, r.first_level, stress_rule_is_edge(r.first_rule) ? 7u & ~(1u << r.first_axis) : 0u, r.first_ijk);
    return r;
}

} // namespace avs
