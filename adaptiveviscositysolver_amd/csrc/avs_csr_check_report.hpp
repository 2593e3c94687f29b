// avs_csr_check_report.hpp -- host side of avs_check_csr / avs_check_system that needs no HIP call: argument checks, the packed key of the
// first violation, the layout of the raw report the kernels leave behind, and the report that goes back to the caller (the hand-over:
// avs_report.hpp).  Plain C++ over include/avs.h, so that a stand-alone program can run it under the host sanitizers
// (tests/csr_check_report_main.cpp).
#pragma once

#include <cmath>

#include "avs_report.hpp"

namespace avs {

// What the kernels leave behind, in 64-bit words: a count per rule, the smallest key of a violating position (kNoKey: none), the
// measurements (the two maxima as the bit patterns of non-negative doubles: their order is the order of the values), and -- written by
// k_csr_check_first once every pass has run -- the row and the stored column of the first violation (as signed 64-bit values).
enum {
    kCsrRawKey = AVS_CSR_RULES,
    kCsrRawEmptyRows,
    kCsrRawLongestRow,
    kCsrRawAsymmetric,
    kCsrRawMaxValue,
    kCsrRawMaxAsymmetry,
    kCsrRawFirstRow,
    kCsrRawFirstCol,
    kCsrRawWords
};
// key = rule | index (a row_ptr index, an entry or a row: below 2^32): ascending keys are the order (rule, index) of the header
constexpr int kCsrKeyIndexBits = 32;
static_assert(AVS_CSR_RULES <= 8, "the rule above a 32-bit index");

constexpr unsigned long long csr_check_key(int rule, unsigned long long index) { return (unsigned long long)rule << kCsrKeyIndexBits | index; }
constexpr int csr_check_key_rule(unsigned long long key) { return (int)(key >> kCsrKeyIndexBits); }
constexpr long long csr_check_key_index(unsigned long long key) { return (long long)(key & ((1ull << kCsrKeyIndexBits) - 1ull)); }

// the rules `what` asks for, given that rule 0 holds (bit r: rule r); vectors: b or x was passed
constexpr int32_t csr_check_rules_asked(uint32_t what, bool vectors)
{
    return (int32_t)(1u << AVS_CSR_RULE_ROW_PTR | 1u << AVS_CSR_RULE_COLUMN | ((what & AVS_CSR_CHECK_VALUES) ? 1u << AVS_CSR_RULE_VALUE : 0u) |
                     ((what & AVS_CSR_CHECK_VALUES) && vectors ? 1u << AVS_CSR_RULE_VECTOR : 0u) |
                     ((what & AVS_CSR_CHECK_ORDER) ? 1u << AVS_CSR_RULE_ORDER : 0u) | ((what & AVS_CSR_CHECK_DIAGONAL) ? 1u << AVS_CSR_RULE_DIAGONAL : 0u) |
                     ((what & AVS_CSR_CHECK_SYMMETRY) ? 1u << AVS_CSR_RULE_PATTERN | 1u << AVS_CSR_RULE_SYMMETRY : 0u));
}

// AVS_OK, or AVS_EINVAL with *why set (the pointer arguments and the device are the entry's own business)
inline avs_status check_csr_args(int64_t n, int64_t nnz, uint32_t what, double symmetry_tolerance, const avs_csr_check *report, const char **why)
{
    if (!report) {
        *why = "csr check: report must not be null";
        return AVS_EINVAL;
    }
    if ((what & ~(uint32_t)AVS_CSR_CHECK_ALL) != 0) {
        *why = "csr check: unknown bits in `what`";
        return AVS_EINVAL;
    }
    if (!report_size_ok(report, offsetof(avs_csr_check, passed) + sizeof(int32_t))) {
        *why = "avs_csr_check.struct_size must be set to sizeof(avs_csr_check) before the call";
        return AVS_EINVAL;
    }
    if (n < 0 || n > (int64_t)INT32_MAX || nnz < 0 || nnz > (int64_t)INT32_MAX) {
        *why = "csr check: n and nnz must lie in [0, 2^31)";
        return AVS_EINVAL;
    }
    if (!(symmetry_tolerance >= 0.) || !std::isfinite(symmetry_tolerance)) {
        *why = "csr check: symmetry_tolerance must be a finite number >= 0";
        return AVS_EINVAL;
    }
    return AVS_OK;
}

inline avs_csr_check check_csr_passed()
{
    avs_csr_check r;
    memset(&r, 0, sizeof(r));
    r.struct_size = (int32_t)sizeof(r);
    r.passed = 1;
    r.evaluated = 1 << AVS_CSR_RULE_ROW_PTR;
    r.first_rule = r.first_row = r.first_col = -1;
    r.first_index = -1;
    return r;
}

// raw[kCsrRawWords] as the kernels wrote it.  rest_ran: the passes behind the row_ptr pass were launched (rule 0 held and n > 0) and
// k_csr_check_first has filled in the row and column words; vectors: b or x was passed.
inline avs_csr_check check_csr_report(const unsigned long long *raw, uint32_t what, bool vectors, bool rest_ran)
{
    avs_csr_check r = check_csr_passed();
    if (raw[AVS_CSR_RULE_ROW_PTR] != 0) { // rule 0 alone: every other count and every measurement stays 0
        r.violations[AVS_CSR_RULE_ROW_PTR] = (int64_t)raw[AVS_CSR_RULE_ROW_PTR];
        r.passed = 0;
        r.first_rule = AVS_CSR_RULE_ROW_PTR;
        r.first_index = csr_check_key_index(raw[kCsrRawKey]);
        return r;
    }
    if (!rest_ran) return r; // n == 0
    r.evaluated = csr_check_rules_asked(what, vectors);
    bool any = false;
    for (int rule = 0; rule < AVS_CSR_RULES; ++rule) {
        r.violations[rule] = (r.evaluated >> rule & 1) ? (int64_t)raw[rule] : 0;
        any = any || r.violations[rule] != 0;
    }
    r.empty_rows = (int64_t)raw[kCsrRawEmptyRows];
    r.longest_row = (int64_t)raw[kCsrRawLongestRow];
    if (what & AVS_CSR_CHECK_SYMMETRY) {
        r.asymmetric_entries = (int64_t)raw[kCsrRawAsymmetric];
        memcpy(&r.max_abs_value, &raw[kCsrRawMaxValue], sizeof(double));
        memcpy(&r.max_abs_asymmetry, &raw[kCsrRawMaxAsymmetry], sizeof(double));
    }
    const unsigned long long key = raw[kCsrRawKey];
    if (!any || key == kNoKey) return r;
    r.passed = 0;
    r.first_rule = csr_check_key_rule(key);
    r.first_index = csr_check_key_index(key);
    r.first_row = (int32_t)(int64_t)raw[kCsrRawFirstRow];
    r.first_col = (int32_t)(int64_t)raw[kCsrRawFirstCol];
    return r;
}

} // namespace avs
