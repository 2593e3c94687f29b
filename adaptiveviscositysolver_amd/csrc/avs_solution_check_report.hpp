// avs_solution_check_report.hpp -- host side of avs_check_solution / avs_check_csr_solution that needs no HIP call: argument checks, the
// order of the arg-max pairs, the layout of the raw report the kernels leave behind, and the report that goes back to the caller (the
// hand-over: avs_report.hpp).  Plain C++ over include/avs.h, so that a stand-alone program can run it under the host sanitizers
// (tests/solution_check_report_main.cpp).
#pragma once

#include <cmath>
#include <limits>

#include "avs_report.hpp"

namespace avs {

// What the kernels leave behind, in 64-bit words: four counters, two maxima as the bit patterns of non-negative doubles (their order is
// the order of the values), and -- written by k_solution_fold -- the five sums as bit patterns, the largest |r_i| and the smallest row
// that attains it (kSolNoRow: no row was summed).
enum {
    kSolRawNonfiniteX = 0,
    kSolRawNonfiniteB,
    kSolRawNonfiniteResidual,
    kSolRawRowsSummed,
    kSolRawMaxX,
    kSolRawMaxUpdate,
    kSolRawSums, // five words, in the order of the partial sums: kSolSum*
    kSolRawMaxResidual = kSolRawSums + 5,
    kSolRawMaxResidualRow,
    kSolRawWords
};
enum { kSolSumRhs = 0, kSolSumResidual, kSolSumXAx, kSolSumXB, kSolSumUpdate, kSolSums };
static_assert(kSolSums == 5, "five sums behind kSolRawSums");
constexpr unsigned kSolNoRow = 0xffffffffu;

// arg-max of |r_i| as a pair (bit pattern of |r_i|, row): is (bits, row) a better answer than (best_bits, best_row)?  The larger value,
// among equal values the smaller row, any row before none: a total order, so the winner does not depend on who compares first.
constexpr bool sol_check_better(unsigned long long bits, unsigned row, unsigned long long best_bits, unsigned best_row)
{
    return row != kSolNoRow && (best_row == kSolNoRow || bits > best_bits || (bits == best_bits && row < best_row));
}

// the claim of the solve that left x (avs_check_solution), or none
struct SolutionClaim {
    bool known = false;
    int32_t converged = -1, iterations = -1;
    double error = std::numeric_limits<double>::quiet_NaN();
};

// AVS_OK, or AVS_EINVAL with *why set (the pointers of the arrays, the state and the device are the entry's own business)
inline avs_status check_solution_args(int32_t which, int where, const double *residual, const avs_solution_check *report, bool report_required,
                                      const char **why)
{
    if (which != AVS_CHECK_OF_SOLUTION && which != AVS_CHECK_OF_INITIAL_GUESS) {
        *why = "solution check: `which` must be AVS_CHECK_OF_SOLUTION or AVS_CHECK_OF_INITIAL_GUESS";
        return AVS_EINVAL;
    }
    if (where != (int)AVS_MEM_HOST && where != (int)AVS_MEM_DEVICE) {
        *why = "solution check: unknown memory space";
        return AVS_EINVAL;
    }
    if (!report && (report_required || !residual)) {
        *why = report_required ? "solution check: report must not be null" : "solution check: report and residual are both null";
        return AVS_EINVAL;
    }
    if (report && !report_size_ok(report, offsetof(avs_solution_check, evaluated) + sizeof(int32_t))) {
        *why = "avs_solution_check.struct_size must be set to sizeof(avs_solution_check) before the call";
        return AVS_EINVAL;
    }
    return AVS_OK;
}
inline avs_status check_solution_sizes(int64_t n, int64_t nnz, const char **why)
{
    if (n < 0 || n > (int64_t)INT32_MAX || nnz < 0 || nnz > (int64_t)INT32_MAX) {
        *why = "solution check: n and nnz must lie in [0, 2^31)";
        return AVS_EINVAL;
    }
    return AVS_OK;
}

// Eigen's error() (cpp:630) from the two sums
inline double solution_relative_residual(double residual_norm2, double rhs_norm2)
{
    if (rhs_norm2 == 0.) return residual_norm2 == 0. ? 0. : std::numeric_limits<double>::infinity();
    return std::sqrt(residual_norm2 / rhs_norm2);
}

// raw: kSolRawWords as the kernels wrote them, or null where no row was walked (n == 0, or evaluated == 0: seam A found rule 0 or 1 of
// avs_check_csr violated)
inline avs_solution_check check_solution_report(const unsigned long long *raw, int32_t which, int64_t n, int64_t nnz, bool evaluated,
                                                const SolutionClaim &claim)
{
    avs_solution_check r;
    memset(&r, 0, sizeof(r));
    r.struct_size = (int32_t)sizeof(r);
    r.which = which;
    r.evaluated = evaluated ? 1 : 0;
    r.claimed_converged = claim.known ? claim.converged : -1;
    r.claimed_iterations = claim.known ? claim.iterations : -1;
    r.claimed_error = claim.known ? claim.error : std::numeric_limits<double>::quiet_NaN();
    r.n = n;
    r.nnz = nnz;
    r.max_residual_row = -1;
    if (!evaluated) {
        r.max_residual_row = 0; // "everything else zero"
        return r;
    }
    if (!raw) return r;
    const auto as_double = [raw](int word) {
        double v;
        memcpy(&v, &raw[word], sizeof(v));
        return v;
    };
    r.nonfinite_x = (int64_t)raw[kSolRawNonfiniteX];
    r.nonfinite_b = (int64_t)raw[kSolRawNonfiniteB];
    r.nonfinite_residual = (int64_t)raw[kSolRawNonfiniteResidual];
    r.rows_summed = (int64_t)raw[kSolRawRowsSummed];
    r.rhs_norm2 = as_double(kSolRawSums + kSolSumRhs);
    r.residual_norm2 = as_double(kSolRawSums + kSolSumResidual);
    r.x_dot_ax = as_double(kSolRawSums + kSolSumXAx);
    r.x_dot_b = as_double(kSolRawSums + kSolSumXB);
    r.update_norm2 = as_double(kSolRawSums + kSolSumUpdate);
    r.relative_residual = solution_relative_residual(r.residual_norm2, r.rhs_norm2);
    r.max_abs_x = as_double(kSolRawMaxX);
    r.max_abs_update = as_double(kSolRawMaxUpdate);
    const unsigned row = (unsigned)raw[kSolRawMaxResidualRow];
    if (r.rows_summed > 0 && row != kSolNoRow) {
        r.max_abs_residual = as_double(kSolRawMaxResidual);
        r.max_residual_row = (int64_t)row;
    }
    return r;
}

} // namespace avs
