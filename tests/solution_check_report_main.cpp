// Stand-alone driver of the host side of avs_check_solution that needs no HIP call (csrc/avs_solution_check_report.hpp: argument checks,
// the order of the arg-max pairs, the raw report turned into avs_solution_check, the struct_size hand-over).
// tests/test_solution_check_host.py builds it with the host sanitizers (-fsanitize=address,undefined) and runs it; it prints "ok" and
// exits 0, or says which expectation failed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "avs_solution_check_report.hpp"

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
    static_assert(sizeof(avs_solution_check) == 160, "layout of avs_solution_check");
    static_assert((int)AVS_CHECK_OF_SOLUTION == (int)AVS_RATES_OF_SOLUTION && (int)AVS_CHECK_OF_INITIAL_GUESS == (int)AVS_RATES_OF_INITIAL_GUESS, "one `which`");
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const char *why = nullptr;
    avs_solution_check rep;
    std::memset(&rep, 0, sizeof(rep));
    rep.struct_size = (int32_t)sizeof(rep);
    double some = 0.;
    // argument checks
    EXPECT(check_solution_args(AVS_CHECK_OF_SOLUTION, AVS_MEM_HOST, nullptr, &rep, false, &why) == AVS_OK);
    EXPECT(check_solution_args(AVS_CHECK_OF_INITIAL_GUESS, AVS_MEM_DEVICE, &some, &rep, true, &why) == AVS_OK);
    EXPECT(check_solution_args(AVS_CHECK_OF_SOLUTION, AVS_MEM_HOST, &some, nullptr, false, &why) == AVS_OK); // the residual alone
    for (int32_t which : {-1, 2, 7, INT32_MIN, INT32_MAX}) {
        why = nullptr;
        EXPECT(check_solution_args(which, AVS_MEM_HOST, &some, &rep, false, &why) == AVS_EINVAL && why);
    }
    for (int where : {-1, 2, 7, INT32_MAX}) {
        why = nullptr;
        EXPECT(check_solution_args(AVS_CHECK_OF_SOLUTION, where, &some, &rep, false, &why) == AVS_EINVAL && why);
    }
    why = nullptr;
    EXPECT(check_solution_args(AVS_CHECK_OF_SOLUTION, AVS_MEM_HOST, nullptr, nullptr, false, &why) == AVS_EINVAL && why); // nothing to write
    why = nullptr;
    EXPECT(check_solution_args(AVS_CHECK_OF_SOLUTION, AVS_MEM_HOST, &some, nullptr, true, &why) == AVS_EINVAL && why); // seam A: evaluated must be seen
    for (int32_t size : {0, 4, 8, 11, -8, 4097, INT32_MIN, INT32_MAX}) {
        rep.struct_size = size;
        EXPECT(check_solution_args(AVS_CHECK_OF_SOLUTION, AVS_MEM_HOST, &some, &rep, false, &why) == AVS_EINVAL);
    }
    for (int32_t size : {12, 24, 96, 160, 4096}) {
        rep.struct_size = size;
        EXPECT(check_solution_args(AVS_CHECK_OF_SOLUTION, AVS_MEM_HOST, &some, &rep, false, &why) == AVS_OK);
    }
    const int64_t top = (int64_t)INT32_MAX;
    EXPECT(check_solution_sizes(0, 0, &why) == AVS_OK && check_solution_sizes(top, top, &why) == AVS_OK);
    EXPECT(check_solution_sizes(-1, 0, &why) == AVS_EINVAL && check_solution_sizes(0, -1, &why) == AVS_EINVAL);
    EXPECT(check_solution_sizes(top + 1, 0, &why) == AVS_EINVAL && check_solution_sizes(0, top + 1, &why) == AVS_EINVAL);
    EXPECT(check_solution_sizes(INT64_MIN, INT64_MAX, &why) == AVS_EINVAL);
    // the order of the arg-max pairs: larger value, then smaller row, any row before none -- and never both ways
    EXPECT(sol_check_better(bits_of(2.), 9u, bits_of(1.), 3u) && !sol_check_better(bits_of(1.), 3u, bits_of(2.), 9u));
    EXPECT(sol_check_better(bits_of(1.), 3u, bits_of(1.), 9u) && !sol_check_better(bits_of(1.), 9u, bits_of(1.), 3u));
    EXPECT(!sol_check_better(bits_of(1.), 3u, bits_of(1.), 3u));
    EXPECT(sol_check_better(0ull, 0u, 0ull, kSolNoRow) && sol_check_better(0ull, 2147483646u, bits_of(inf), kSolNoRow));
    EXPECT(!sol_check_better(bits_of(inf), kSolNoRow, 0ull, 5u) && !sol_check_better(0ull, kSolNoRow, 0ull, kSolNoRow));
    EXPECT(sol_check_better(bits_of(5e-324), 7u, 0ull, 0u) && sol_check_better(bits_of(inf), 7u, bits_of(1.7e308), 0u));
    { // a fold in any order picks the same pair
        const unsigned long long b[5] = {bits_of(1.), bits_of(3.), 0ull, bits_of(3.), bits_of(2.)};
        const unsigned r[5] = {4u, 9u, kSolNoRow, 6u, 1u};
        for (int start = 0; start < 5; ++start)
            for (int step : {1, 2, 3, 4}) {
                unsigned long long best = 0ull;
                unsigned row = kSolNoRow;
                for (int t = 0, i = start; t < 5; ++t, i = (i + step) % 5)
                    if (sol_check_better(b[i], r[i], best, row)) best = b[i], row = r[i];
                EXPECT(best == bits_of(3.) && row == 6u);
            }
    }
    // Eigen's error() from the two sums
    EXPECT(solution_relative_residual(0., 0.) == 0. && solution_relative_residual(1e-300, 0.) == inf && solution_relative_residual(0., 4.) == 0.);
    EXPECT(solution_relative_residual(1., 4.) == 0.5 && solution_relative_residual(inf, 4.) == inf && std::isnan(solution_relative_residual(nan, 4.)));
    // a raw report into the struct
    unsigned long long raw[kSolRawWords] = {};
    raw[kSolRawNonfiniteX] = 1;
    raw[kSolRawNonfiniteB] = 2;
    raw[kSolRawNonfiniteResidual] = 5000000000ull;
    raw[kSolRawRowsSummed] = 2147483000ull;
    raw[kSolRawMaxX] = bits_of(7.5);
    raw[kSolRawMaxUpdate] = bits_of(0.25);
    raw[kSolRawSums + kSolSumRhs] = bits_of(16.);
    raw[kSolRawSums + kSolSumResidual] = bits_of(4.);
    raw[kSolRawSums + kSolSumXAx] = bits_of(-3.);
    raw[kSolRawSums + kSolSumXB] = bits_of(1.5);
    raw[kSolRawSums + kSolSumUpdate] = bits_of(0.125);
    raw[kSolRawMaxResidual] = bits_of(1.75);
    raw[kSolRawMaxResidualRow] = 2147483646ull;
    SolutionClaim claim;
    avs_solution_check r = check_solution_report(raw, AVS_CHECK_OF_SOLUTION, 2147483647, 2147483647, true, claim);
    EXPECT(r.struct_size == 160 && r.which == 0 && r.evaluated == 1 && r.claimed_converged == -1 && r.claimed_iterations == -1 && std::isnan(r.claimed_error));
    EXPECT(r.reserved == 0 && r.n == 2147483647 && r.nnz == 2147483647 && r.nonfinite_x == 1 && r.nonfinite_b == 2 && r.nonfinite_residual == 5000000000ll);
    EXPECT(r.rows_summed == 2147483000ll && r.rhs_norm2 == 16. && r.residual_norm2 == 4. && r.relative_residual == 0.5 && r.x_dot_ax == -3. && r.x_dot_b == 1.5);
    EXPECT(r.update_norm2 == 0.125 && r.max_abs_update == 0.25 && r.max_abs_x == 7.5 && r.max_abs_residual == 1.75 && r.max_residual_row == 2147483646ll);
    claim.known = true;
    claim.converged = 1;
    claim.iterations = 212;
    claim.error = 3e-9;
    r = check_solution_report(raw, AVS_CHECK_OF_INITIAL_GUESS, 10, 30, true, claim);
    EXPECT(r.which == 1 && r.claimed_converged == 1 && r.claimed_iterations == 212 && r.claimed_error == 3e-9 && r.n == 10 && r.nnz == 30);
    // no row was summed: no arg-max, whatever the words hold
    raw[kSolRawRowsSummed] = 0;
    raw[kSolRawMaxResidualRow] = kSolNoRow;
    r = check_solution_report(raw, AVS_CHECK_OF_SOLUTION, 10, 30, true, SolutionClaim());
    EXPECT(r.rows_summed == 0 && r.max_residual_row == -1 && r.max_abs_residual == 0.);
    // b == 0
    raw[kSolRawSums + kSolSumRhs] = bits_of(0.);
    r = check_solution_report(raw, AVS_CHECK_OF_SOLUTION, 10, 30, true, SolutionClaim());
    EXPECT(r.relative_residual == inf);
    raw[kSolRawSums + kSolSumResidual] = bits_of(0.);
    r = check_solution_report(raw, AVS_CHECK_OF_SOLUTION, 10, 30, true, SolutionClaim());
    EXPECT(r.relative_residual == 0.);
    // n == 0 (no raw words): evaluated, everything zero, no arg-max
    r = check_solution_report(nullptr, AVS_CHECK_OF_SOLUTION, 0, 0, true, SolutionClaim());
    EXPECT(r.evaluated == 1 && r.n == 0 && r.rows_summed == 0 && r.relative_residual == 0. && r.max_residual_row == -1 && r.rhs_norm2 == 0.);
    // seam A refused: evaluated = 0 and every figure zero
    r = check_solution_report(nullptr, AVS_CHECK_OF_SOLUTION, 300, 898, false, SolutionClaim());
    EXPECT(r.evaluated == 0 && r.n == 300 && r.nnz == 898 && r.rows_summed == 0 && r.max_residual_row == 0 && r.residual_norm2 == 0. && r.relative_residual == 0.);
    EXPECT(r.claimed_converged == -1 && std::isnan(r.claimed_error));
    // the hand-over writes struct_size bytes and not one more: the caller's struct sits at the very end of a heap block
    r = check_solution_report(raw, AVS_CHECK_OF_INITIAL_GUESS, 10, 30, true, claim);
    for (int32_t size : {12, 16, 24, 32, 40, 96, 152, 160}) {
        std::vector<unsigned char> block((size_t)size, 0x5a);
        std::memcpy(block.data(), &size, sizeof(size));
        report_hand_over(r, reinterpret_cast<avs_solution_check *>(block.data()));
        int32_t back, which, evaluated;
        std::memcpy(&back, block.data(), 4);
        std::memcpy(&which, block.data() + 4, 4);
        std::memcpy(&evaluated, block.data() + 8, 4);
        EXPECT(back == size && which == 1 && evaluated == 1);
        if (size >= 32) {
            int64_t n;
            std::memcpy(&n, block.data() + 24, 8);
            EXPECT(n == 10);
        }
    }
    { // a caller built against a larger, future struct: the bytes behind today's struct stay
        std::vector<unsigned char> block(200, 0x5a);
        const int32_t size = 200;
        std::memcpy(block.data(), &size, sizeof(size));
        report_hand_over(r, reinterpret_cast<avs_solution_check *>(block.data()));
        for (size_t b = sizeof(avs_solution_check); b < block.size(); ++b) EXPECT(block[b] == 0x5a);
    }
    std::puts("ok");
    return 0;
}
