// Stand-alone driver of the host side of avs_check_csr that needs no HIP call (csrc/avs_csr_check_report.hpp: argument checks, the packed key
// of the first violation, the raw report turned into avs_csr_check, the struct_size hand-over).  tests/test_csr_check_host.py builds it with
// the host sanitizers (-fsanitize=address,undefined) and runs it; it prints "ok" and exits 0, or says which expectation failed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "avs_csr_check_report.hpp"

#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

using namespace avs;

static unsigned long long bits_of(double v)
{
    unsigned long long b;
    std::memcpy(&b, &v, sizeof(b));
    return b;
}

int main()
{
    const char *why = nullptr;
    avs_csr_check rep;
    std::memset(&rep, 0, sizeof(rep));
    rep.struct_size = (int32_t)sizeof(rep);
    static_assert(sizeof(avs_csr_check) == 136, "layout of avs_csr_check");
    const int64_t top = (int64_t)INT32_MAX;
    // argument checks
    EXPECT(check_csr_args(3, 7, AVS_CSR_CHECK_ALL, 0., nullptr, &why) == AVS_EINVAL && why);
    for (uint32_t what = 0; what <= (uint32_t)AVS_CSR_CHECK_ALL; ++what) EXPECT(check_csr_args(3, 7, what, 0., &rep, &why) == AVS_OK);
    for (uint32_t what : {16u, 31u, 0x100u, 0x80000001u, 0xffffffffu}) {
        why = nullptr;
        EXPECT(check_csr_args(3, 7, what, 0., &rep, &why) == AVS_EINVAL && why);
    }
    for (int32_t size : {0, 4, 7, -8, 4097, INT32_MIN, INT32_MAX}) {
        rep.struct_size = size;
        EXPECT(check_csr_args(3, 7, 1u, 0., &rep, &why) == AVS_EINVAL);
    }
    for (int32_t size : {8, 24, 96, 136, 4096}) {
        rep.struct_size = size;
        EXPECT(check_csr_args(3, 7, 1u, 0., &rep, &why) == AVS_OK);
    }
    rep.struct_size = (int32_t)sizeof(rep);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (double tol : {-1., -0.5e-300, nan, -nan, inf, -inf}) {
        why = nullptr;
        EXPECT(check_csr_args(3, 7, AVS_CSR_CHECK_SYMMETRY, tol, &rep, &why) == AVS_EINVAL && why);
    }
    for (double tol : {0., -0., 5e-324, 1e-12, 1e300}) EXPECT(check_csr_args(3, 7, AVS_CSR_CHECK_SYMMETRY, tol, &rep, &why) == AVS_OK);
    EXPECT(check_csr_args(0, 0, 0u, 0., &rep, &why) == AVS_OK);
    EXPECT(check_csr_args(top, top, 0u, 0., &rep, &why) == AVS_OK);
    EXPECT(check_csr_args(-1, 0, 0u, 0., &rep, &why) == AVS_EINVAL);
    EXPECT(check_csr_args(0, -1, 0u, 0., &rep, &why) == AVS_EINVAL);
    EXPECT(check_csr_args(top + 1, 0, 0u, 0., &rep, &why) == AVS_EINVAL);
    EXPECT(check_csr_args(0, top + 1, 0u, 0., &rep, &why) == AVS_EINVAL);
    EXPECT(check_csr_args(INT64_MIN, INT64_MAX, 0u, 0., &rep, &why) == AVS_EINVAL);
    // keys: round trips at both ends of the index range, ordered by (rule, index), and all below "no key"
    for (int rule = 0; rule < AVS_CSR_RULES; ++rule)
        for (unsigned long long index : {0ull, 1ull, 2147483646ull, 2147483647ull}) {
            const unsigned long long key = csr_check_key(rule, index);
            EXPECT(csr_check_key_rule(key) == rule && csr_check_key_index(key) == (long long)index && key < kNoKey);
        }
    EXPECT(csr_check_key(0, 2147483647ull) < csr_check_key(1, 0));
    EXPECT(csr_check_key(6, (1ull << kCsrKeyIndexBits) - 1ull) < csr_check_key(7, 0));
    EXPECT(csr_check_key(3, 5) < csr_check_key(3, 6));
    // which rules a call evaluates
    EXPECT(csr_check_rules_asked(0u, true) == 3 && csr_check_rules_asked(AVS_CSR_CHECK_ALL, true) == 255 && csr_check_rules_asked(AVS_CSR_CHECK_ALL, false) == 247);
    EXPECT(csr_check_rules_asked(AVS_CSR_CHECK_VALUES, false) == 7 && csr_check_rules_asked(AVS_CSR_CHECK_ORDER, true) == 19);
    EXPECT(csr_check_rules_asked(AVS_CSR_CHECK_DIAGONAL, true) == 35 && csr_check_rules_asked(AVS_CSR_CHECK_SYMMETRY, true) == 195);
    // a clean raw report
    unsigned long long raw[kCsrRawWords] = {};
    raw[kCsrRawKey] = kNoKey;
    raw[kCsrRawEmptyRows] = 2;
    raw[kCsrRawLongestRow] = 10000;
    raw[kCsrRawMaxValue] = bits_of(3.5);
    raw[kCsrRawFirstRow] = raw[kCsrRawFirstCol] = ~0ull; // -1, as k_csr_check_first leaves them without a violation
    avs_csr_check r = check_csr_report(raw, AVS_CSR_CHECK_ALL, true, true);
    EXPECT(r.struct_size == 136 && r.passed == 1 && r.evaluated == 255 && r.first_rule == -1 && r.first_index == -1 && r.first_row == -1 && r.first_col == -1);
    EXPECT(r.empty_rows == 2 && r.longest_row == 10000 && r.asymmetric_entries == 0 && r.max_abs_value == 3.5 && r.max_abs_asymmetry == 0.);
    r = check_csr_report(raw, AVS_CSR_CHECK_VALUES, false, true); // the measurements of the SYMMETRY bit are not asked for
    EXPECT(r.passed == 1 && r.evaluated == 7 && r.max_abs_value == 0. && r.empty_rows == 2 && r.longest_row == 10000);
    r = check_csr_report(raw, AVS_CSR_CHECK_ALL, true, false); // n == 0: rule 0 alone
    EXPECT(r.passed == 1 && r.evaluated == 1 && r.longest_row == 0 && r.max_abs_value == 0.);
    // violations: 64-bit counts, rules that were not asked for dropped, the first position with its row and its stored column
    raw[AVS_CSR_RULE_COLUMN] = 5000000000ull;
    raw[AVS_CSR_RULE_VALUE] = 3;
    raw[AVS_CSR_RULE_VECTOR] = 4;
    raw[AVS_CSR_RULE_SYMMETRY] = 6;
    raw[kCsrRawAsymmetric] = 8;
    raw[kCsrRawMaxAsymmetry] = bits_of(inf);
    raw[kCsrRawKey] = csr_check_key(AVS_CSR_RULE_COLUMN, 2147483646ull);
    raw[kCsrRawFirstRow] = 2147483646ull;
    raw[kCsrRawFirstCol] = (unsigned long long)(long long)INT32_MIN;
    r = check_csr_report(raw, AVS_CSR_CHECK_ALL, false, true);
    EXPECT(r.passed == 0 && r.evaluated == 247 && r.violations[AVS_CSR_RULE_COLUMN] == 5000000000ll && r.violations[AVS_CSR_RULE_VALUE] == 3);
    EXPECT(r.violations[AVS_CSR_RULE_VECTOR] == 0 && r.violations[AVS_CSR_RULE_SYMMETRY] == 6 && r.asymmetric_entries == 8 && r.max_abs_asymmetry == inf);
    EXPECT(r.first_rule == AVS_CSR_RULE_COLUMN && r.first_index == 2147483646ll && r.first_row == 2147483646 && r.first_col == INT32_MIN);
    r = check_csr_report(raw, 0u, true, true);
    EXPECT(r.passed == 0 && r.evaluated == 3 && r.violations[AVS_CSR_RULE_VALUE] == 0 && r.violations[AVS_CSR_RULE_SYMMETRY] == 0 && r.asymmetric_entries == 0 &&
           r.max_abs_asymmetry == 0.);
    // a violated rule 0 stands alone, whatever else the raw words hold
    raw[AVS_CSR_RULE_ROW_PTR] = 2;
    raw[kCsrRawKey] = csr_check_key(AVS_CSR_RULE_ROW_PTR, 2147483647ull);
    r = check_csr_report(raw, AVS_CSR_CHECK_ALL, true, false);
    EXPECT(r.passed == 0 && r.evaluated == 1 && r.violations[AVS_CSR_RULE_ROW_PTR] == 2 && r.first_rule == 0 && r.first_index == 2147483647ll);
    EXPECT(r.first_row == -1 && r.first_col == -1 && r.empty_rows == 0 && r.longest_row == 0 && r.max_abs_value == 0.);
    for (int rule = 1; rule < AVS_CSR_RULES; ++rule) EXPECT(r.violations[rule] == 0);
    // the hand-over writes struct_size bytes and not one more: the caller's struct sits at the very end of a heap block
    for (int32_t size : {8, 12, 16, 24, 32, 96, 120, 136}) {
        std::vector<unsigned char> block((size_t)size, 0x5a);
        avs_csr_check *out = reinterpret_cast<avs_csr_check *>(block.data());
        std::memcpy(block.data(), &size, sizeof(size));
        report_hand_over(r, out);
        int32_t back, passed;
        std::memcpy(&back, block.data(), 4);
        std::memcpy(&passed, block.data() + 4, 4);
        EXPECT(back == size && passed == 0);
        if (size >= 24) {
            int64_t index;
            std::memcpy(&index, block.data() + 16, 8);
            EXPECT(index == 2147483647ll);
        }
    }
    { // a caller built against a larger, future struct: the bytes behind today's struct stay
        std::vector<unsigned char> block(200, 0x5a);
        const int32_t size = 200;
        std::memcpy(block.data(), &size, sizeof(size));
        report_hand_over(r, reinterpret_cast<avs_csr_check *>(block.data()));
        for (size_t b = sizeof(avs_csr_check); b < block.size(); ++b) EXPECT(block[b] == 0x5a);
    }
    std::puts("ok");
    return 0;
}
