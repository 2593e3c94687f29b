// avs_check_report.hpp -- host side of avs_check_octree / avs_prepass_check_octree that needs no HIP call: argument checks, the packed
// key of the first violation, and the report that goes back to the caller.  Plain C++ over include/avs.h, so that a stand-alone program
// can run it under the host sanitizers (tests/octree_check_report_main.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "avs.h"

namespace avs {

// What the kernels leave behind: one 64-bit count per rule, then the smallest key of a violating entry (all ones: none).
constexpr int kCheckRawWords = AVS_OCTREE_RULES + 1;
constexpr unsigned long long kCheckNoKey = ~0ull;
// key = rule | level | axis | linear index of the entry in its lattice (rule 7: the id): ascending keys are the order of the header
constexpr int kCheckLinBits = 40, kCheckAxisShift = kCheckLinBits, kCheckLevelShift = kCheckAxisShift + 2, kCheckRuleShift = kCheckLevelShift + 3;
static_assert(AVS_MAX_LEVELS <= 8 && AVS_OCTREE_RULES <= 8, "three bits each in the key");

constexpr unsigned long long check_key(int rule, int level, int axis, unsigned long long lin)
{
    return (unsigned long long)rule << kCheckRuleShift | (unsigned long long)level << kCheckLevelShift | (unsigned long long)axis << kCheckAxisShift | lin;
}

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
    if (report->struct_size < (int32_t)(offsetof(avs_octree_check, passed) + sizeof(int32_t)) || report->struct_size > 4096) {
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
    const unsigned long long key = raw[AVS_OCTREE_RULES];
    if (!any || key == kCheckNoKey) return r;
    r.passed = 0;
    r.first_rule = (int32_t)(key >> kCheckRuleShift);
    r.first_level = (int32_t)(key >> kCheckLevelShift & 7u);
    r.first_axis = (int32_t)(key >> kCheckAxisShift & 3u);
    const unsigned long long lin = key & ((1ull << kCheckLinBits) - 1ull);
    if (r.first_rule == AVS_RULE_NUMBERING) { // the entry is an id
        r.first_ijk[0] = (int32_t)lin;
        r.first_ijk[1] = r.first_ijk[2] = 0;
        return r;
    }
    unsigned long long e[3];
    for (int a = 0; a < 3; ++a) {
        e[a] = (unsigned long long)(n[a] >> r.first_level);
        if (r.first_rule >= AVS_RULE_INDEX_VALUE && a == r.first_axis) e[a] += 1; // face lattice
        if (e[a] == 0) e[a] = 1;
    }
    r.first_ijk[0] = (int32_t)(lin % e[0]);
    r.first_ijk[1] = (int32_t)(lin / e[0] % e[1]);
    r.first_ijk[2] = (int32_t)(lin / (e[0] * e[1]));
    return r;
}

// only the bytes the caller's header knows are written (struct_size is IN, as in avs_matrix_format)
inline void check_octree_hand_over(const avs_octree_check &full, avs_octree_check *out)
{
    const int32_t size = out->struct_size;
    memcpy(out, &full, (size_t)size < sizeof(full) ? (size_t)size : sizeof(full));
    out->struct_size = size;
}

} // namespace avs
