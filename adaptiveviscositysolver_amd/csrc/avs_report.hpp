// avs_report.hpp -- what the host sides of the device diagnostics share (avs_check_report.hpp, avs_stress_check_report.hpp,
// avs_csr_check_report.hpp, avs_solution_check_report.hpp, avs_spectrum_report.hpp, avs_strain.hip): admission and hand-over of a
// size-prefixed report struct, the "no violation" key, and the packed key of the first violation of the two pyramid checks with the
// decode of its lattice entry.  Plain C++ over include/avs.h, so that the stand-alone programs under tests/ can run it under the host
// sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "avs.h"

namespace avs {

// struct_size is IN: it must cover the first member the call writes (first_out_end: the offset behind it) and be plausible
template <typename T>
inline bool report_size_ok(const T *report, size_t first_out_end)
{
    return report->struct_size >= (int32_t)first_out_end && report->struct_size <= 4096;
}
// only the bytes the caller's header knows are written, and struct_size stays the caller's
template <typename T>
inline void report_hand_over(const T &full, T *out)
{
    const int32_t size = out->struct_size;
    memcpy(out, &full, (size_t)size < sizeof(full) ? (size_t)size : sizeof(full));
    out->struct_size = size;
}

// the key word of a raw report before any wave has found a violation: above every key
constexpr unsigned long long kNoKey = ~0ull;

// key of an entry of an index or label pyramid = rule | level | axis | linear index of the entry in its own lattice (numbering rules:
// the id): ascending keys are the order (rule, level, axis, entry) of the header
constexpr int kLatticeLinBits = 40, kLatticeAxisShift = kLatticeLinBits, kLatticeLevelShift = kLatticeAxisShift + 2,
              kLatticeRuleShift = kLatticeLevelShift + 3;
static_assert(AVS_MAX_LEVELS <= 8 && AVS_OCTREE_RULES <= 16 && AVS_STRESS_RULES <= 16, "three bits for the level and four for the rule in the key");

constexpr unsigned long long lattice_key(int rule, int level, int axis, unsigned long long lin)
{
    return (unsigned long long)rule << kLatticeRuleShift | (unsigned long long)level << kLatticeLevelShift | (unsigned long long)axis << kLatticeAxisShift | lin;
}
constexpr int32_t lattice_key_rule(unsigned long long key) { return (int32_t)(key >> kLatticeRuleShift & 15u); }
constexpr int32_t lattice_key_level(unsigned long long key) { return (int32_t)(key >> kLatticeLevelShift & 7u); }
constexpr int32_t lattice_key_axis(unsigned long long key) { return (int32_t)(key >> kLatticeAxisShift & 3u); }
constexpr unsigned long long lattice_key_lin(unsigned long long key) { return key & ((1ull << kLatticeLinBits) - 1ull); }

// entry `lin` of a lattice of `level` as (i, j, k), x fastest; n: level-0 cells per axis; bit a of plus_one_mask: the lattice has one
// entry more than cells along axis a (a face lattice: its own axis, an edge lattice: the two others)
inline void lattice_entry_ijk(unsigned long long lin, const int n[3], int level, unsigned plus_one_mask, int32_t out[3])
{
    unsigned long long e[3];
    for (int a = 0; a < 3; ++a) {
        e[a] = (unsigned long long)(n[a] >> level) + (plus_one_mask >> a & 1u);
        if (e[a] == 0) e[a] = 1;
    }
    out[0] = (int32_t)(lin % e[0]);
    out[1] = (int32_t)(lin / e[0] % e[1]);
    out[2] = (int32_t)(lin / (e[0] * e[1]));
}

} // namespace avs
