// avs_stress_check_report.hpp -- host side of avs_check_stress_indices / avs_prepass_check_stress_indices that needs no HIP call: argument
// checks, the packed key of the first violation, and the report that goes back to the caller.  Plain C++ over include/avs.h, so that a
// stand-alone program can run it under the host sanitizers (tests/stress_check_report_main.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "avs.h"

namespace avs {

// What the kernels leave behind: one 64-bit count per rule, the smallest key of a violating entry (all ones: none), then the number of
// edge and of centre entries that carry an id.
constexpr int kStressRawKey = AVS_STRESS_RULES, kStressRawEdges = AVS_STRESS_RULES + 1, kStressRawCenters = AVS_STRESS_RULES + 2;
constexpr int kStressRawWords = AVS_STRESS_RULES + 3;
constexpr unsigned long long kStressNoKey = ~0ull;
// key = rule | level | axis | linear index of the entry in its own lattice (rules 3 and 8: the id): ascending keys are the order of the header
constexpr int kStressLinBits = 40, kStressAxisShift = kStressLinBits, kStressLevelShift = kStressAxisShift + 2, kStressRuleShift = kStressLevelShift + 3;
static_assert(AVS_MAX_LEVELS <= 8 && AVS_STRESS_RULES <= 16, "three bits for the level and four for the rule in the key");

constexpr unsigned long long stress_key(int rule, int level, int axis, unsigned long long lin)
{
    return (unsigned long long)rule << kStressRuleShift | (unsigned long long)level << kStressLevelShift | (unsigned long long)axis << kStressAxisShift | lin;
}

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
    if (report->struct_size < (int32_t)(offsetof(avs_stress_check, passed) + sizeof(int32_t)) || report->struct_size > 4096) {
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
    if (!any || key == kStressNoKey) return r;
    r.passed = 0;
    r.first_rule = (int32_t)(key >> kStressRuleShift & 15u);
    r.first_level = (int32_t)(key >> kStressLevelShift & 7u);
    r.first_axis = (int32_t)(key >> kStressAxisShift & 3u);
    const unsigned long long lin = key & ((1ull << kStressLinBits) - 1ull);
    if (r.first_rule == AVS_STRESS_RULE_EDGE_NUMBERING || r.first_rule == AVS_STRESS_RULE_CENTER_NUMBERING) { // the entry is an id
        r.first_ijk[0] = (int32_t)lin;
        r.first_ijk[1] = r.first_ijk[2] = 0;
        return r;
    }
    unsigned long long e[3];
    for (int a = 0; a < 3; ++a) {
        e[a] = (unsigned long long)(n[a] >> r.first_level);
        if (stress_rule_is_edge(r.first_rule) && a != r.first_axis) e[a] += 1; // edge lattice: one more on the two other axes
        if (e[a] == 0) e[a] = 1;
    }
    r.first_ijk[0] = (int32_t)(lin % e[0]);
    r.first_ijk[1] = (int32_t)(lin / e[0] % e[1]);
    r.first_ijk[2] = (int32_t)(lin / (e[0] * e[1]));
    return r;
}

// only the bytes the caller's header knows are written (struct_size is IN, as in avs_octree_check)
inline void check_stress_hand_over(const avs_stress_check &full, avs_stress_check *out)
{
    const int32_t size = out->struct_size;
    memcpy(out, &full, (size_t)size < sizeof(full) ? (size_t)size : sizeof(full));
    out->struct_size = size;
}

} // namespace avs
