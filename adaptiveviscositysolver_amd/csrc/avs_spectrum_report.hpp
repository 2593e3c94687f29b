// avs_spectrum_report.hpp -- host side of avs_estimate_spectrum / avs_estimate_csr_spectrum that needs no HIP call: argument checks, the
// layout of the raw words the kernels leave behind, the eigenvalues of the Lanczos tridiagonal with the last components of its two
// extreme eigenvectors, and the report that goes back to the caller (the hand-over: avs_report.hpp).  Plain C++ over include/avs.h, so
// that a stand-alone program can run it under the host sanitizers (tests/spectrum_report_main.cpp).
#pragma once

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "avs_report.hpp"

namespace avs {

// What the kernels leave behind, in 64-bit words: the stop word every kernel of the recurrence reads at entry, the three figures the
// fold behind a step writes with it, the count of bad diagonals (non-zero: nothing behind the scale kernel runs), the Gershgorin bound
// as the bit pattern of a non-negative double, and alpha[0 .. MAX_STEPS) / beta[0 .. MAX_STEPS] as bit patterns.
enum {
    kSpecRawStop = 0,
    kSpecRawStepsTaken,
    kSpecRawBreakdown,
    kSpecRawNonfinite,
    kSpecRawBadDiagonal,
    kSpecRawGershgorin,
    kSpecRawAlpha,
    kSpecRawBeta = kSpecRawAlpha + AVS_SPECTRUM_MAX_STEPS,
    kSpecRawWords = kSpecRawBeta + AVS_SPECTRUM_MAX_STEPS + 1
};

// beta[j + 1] <= kSpecBreakdown * (|alpha[j]| + beta[j]): the Krylov space is invariant to working accuracy
constexpr double kSpecBreakdown = 1.0 / 68719476736.0; // 2^-36

// the start vector of AVS_SPECTRUM_START_HASH: splitmix64 of the row, its upper 53 bits as a fraction, centred
constexpr uint64_t spectrum_splitmix64(uint64_t i)
{
    uint64_t z = i + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline double spectrum_hash_entry(uint64_t i) { return (double)(spectrum_splitmix64(i) >> 11) * (1.0 / 9007199254740992.0) - 0.5; }

// AVS_OK, or AVS_EINVAL with *why set (the pointers of the arrays, the state and the device are the entry's own business)
inline avs_status spectrum_args(int32_t op, int32_t start, int32_t steps, int where, const avs_spectrum *report, bool context_form, const char **why)
{
    if (op != AVS_SPECTRUM_OF_JACOBI && op != AVS_SPECTRUM_OF_MATRIX) {
        *why = "spectrum: `op` must be AVS_SPECTRUM_OF_JACOBI or AVS_SPECTRUM_OF_MATRIX";
        return AVS_EINVAL;
    }
    if (start != AVS_SPECTRUM_START_RESIDUAL && start != AVS_SPECTRUM_START_HASH && start != AVS_SPECTRUM_START_VECTOR) {
        *why = "spectrum: `start` must be AVS_SPECTRUM_START_RESIDUAL, _HASH or _VECTOR";
        return AVS_EINVAL;
    }
    if (context_form && start == AVS_SPECTRUM_START_VECTOR) {
        *why = "avs_estimate_spectrum: AVS_SPECTRUM_START_VECTOR belongs to avs_estimate_csr_spectrum (a context holds no such vector)";
        return AVS_EINVAL;
    }
    if (steps < 1 || steps > AVS_SPECTRUM_MAX_STEPS) {
        *why = "spectrum: `steps` must lie in [1, AVS_SPECTRUM_MAX_STEPS]";
        return AVS_EINVAL;
    }
    if (where != (int)AVS_MEM_HOST && where != (int)AVS_MEM_DEVICE) {
        *why = "spectrum: unknown memory space";
        return AVS_EINVAL;
    }
    if (!report) {
        *why = "spectrum: report must not be null";
        return AVS_EINVAL;
    }
    if (!report_size_ok(report, offsetof(avs_spectrum, evaluated) + sizeof(int32_t))) {
        *why = "avs_spectrum.struct_size must be set to sizeof(avs_spectrum) before the call";
        return AVS_EINVAL;
    }
    return AVS_OK;
}
inline avs_status spectrum_sizes(int64_t n, int64_t nnz, const char **why)
{
    if (n < 0 || n > (int64_t)INT32_MAX || nnz < 0 || nnz > (int64_t)INT32_MAX) {
        *why = "spectrum: n and nnz must lie in [0, 2^31)";
        return AVS_EINVAL;
    }
    return AVS_OK;
}

// Eigenvalues of the symmetric tridiagonal T_k = tridiag(off[0 .. k - 2]; diag[0 .. k - 1]) in ascending order, and with each the last
// component of its normalised eigenvector: the implicit QL iteration (EISPACK tql2), the rotations applied to the last row of the
// eigenvector matrix only.  Backward stable: every eigenvalue within O(k) eps |T| of one of T_k.  All entries must be finite.  False if
// an eigenvalue did not converge in 120 sweeps (never seen).
inline bool spectrum_tridiagonal(int k, const double *diag, const double *off, double *ritz, double *last)
{
    if (k <= 0) return true;
    std::vector<double> d(diag, diag + k), e((size_t)k, 0.), z((size_t)k, 0.);
    for (int i = 0; i + 1 < k; ++i) e[(size_t)i] = off[i];
    z[(size_t)k - 1] = 1.;
    const double eps = std::numeric_limits<double>::epsilon();
    for (int l = 0; l < k; ++l) {
        int iter = 0, m;
        do {
            for (m = l; m < k - 1; ++m) {
                const double dd = std::fabs(d[(size_t)m]) + std::fabs(d[(size_t)m + 1]);
                if (std::fabs(e[(size_t)m]) <= eps * dd) break;
            }
            if (m == l) break;
            if (iter++ == 120) return false;
            double g = (d[(size_t)l + 1] - d[(size_t)l]) / (2. * e[(size_t)l]);
            double r = std::hypot(g, 1.);
            g = d[(size_t)m] - d[(size_t)l] + e[(size_t)l] / (g + std::copysign(r, g));
            double s = 1., c = 1., p = 0.;
            int i;
            for (i = m - 1; i >= l; --i) {
                double f = s * e[(size_t)i];
                const double b = c * e[(size_t)i];
                r = std::hypot(f, g);
                e[(size_t)i + 1] = r;
                if (r == 0.) {
                    d[(size_t)i + 1] -= p;
                    e[(size_t)m] = 0.;
                    break;
                }
                s = f / r;
                c = g / r;
                g = d[(size_t)i + 1] - p;
                r = (d[(size_t)i] - g) * s + 2. * c * b;
                p = s * r;
                d[(size_t)i + 1] = g + p;
                g = c * r - b;
                f = z[(size_t)i + 1];
                z[(size_t)i + 1] = s * z[(size_t)i] + c * f;
                z[(size_t)i] = c * z[(size_t)i] - s * f;
            }
            if (r == 0. && i >= l) continue;
            d[(size_t)l] -= p;
            e[(size_t)l] = g;
            e[(size_t)m] = 0.;
        } while (m != l);
    }
    std::vector<int> order((size_t)k);
    for (int i = 0; i < k; ++i) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&d](int a, int b) { return d[(size_t)a] < d[(size_t)b] || (d[(size_t)a] == d[(size_t)b] && a < b); });
    for (int i = 0; i < k; ++i) {
        ritz[i] = d[(size_t)order[(size_t)i]];
        if (last) last[i] = z[(size_t)order[(size_t)i]];
    }
    return true;
}

// ceil(0.5 sqrt(kappa) ln(2 / tolerance)): the iterations after which CG has reduced the A-norm of the error by `tolerance`, at the
// latest.  -1 without a tolerance in (0, 1) or without a finite kappa >= 1.
inline int64_t spectrum_iteration_bound(double kappa, double tolerance)
{
    if (!(tolerance > 0. && tolerance < 1.) || !(kappa >= 1.) || !std::isfinite(kappa)) return -1;
    const double it = std::ceil(0.5 * std::sqrt(kappa) * std::log(2. / tolerance));
    return it < 9.0e18 ? (int64_t)it : INT64_MAX;
}

struct SpectrumAsk { // what the caller asked for, echoed in the report
    int32_t op = 0, start = 0, steps = 0;
    int64_t n = 0, nnz = 0;
    double tolerance = 0.;
};

// raw: kSpecRawWords as the kernels wrote them, or null where no kernel ran (n == 0; evaluated == false: seam A found rule 0 or 1 of
// avs_check_csr violated).  ritz: ask.steps entries or null.  False if the tridiagonal eigenvalues did not converge.
inline bool spectrum_report(const unsigned long long *raw, const SpectrumAsk &ask, bool evaluated, double *ritz, avs_spectrum *out)
{
    avs_spectrum r;
    memset(&r, 0, sizeof(r));
    r.struct_size = (int32_t)sizeof(r);
    r.op = ask.op;
    r.start = ask.start;
    r.steps_asked = ask.steps;
    r.n = ask.n;
    r.nnz = ask.nnz;
    r.tolerance = ask.tolerance;
    if (ritz)
        for (int i = 0; i < ask.steps; ++i) ritz[i] = 0.;
    memcpy(out, &r, sizeof(r)); // (the padding behind `indefinite` too: the bytes go to the caller)
    if (!evaluated) return true;
    if (raw && raw[kSpecRawBadDiagonal] != 0ull) {
        out->bad_diagonal = (int64_t)raw[kSpecRawBadDiagonal];
        return true;
    }
    out->evaluated = 1;
    out->iteration_bound = -1;
    if (!raw) return true;
    const auto as_double = [raw](int word) {
        double v;
        memcpy(&v, &raw[word], sizeof(v));
        return v;
    };
    const int k = (int)raw[kSpecRawStepsTaken];
    out->steps_taken = k;
    out->breakdown = raw[kSpecRawBreakdown] ? 1 : 0;
    out->nonfinite = raw[kSpecRawNonfinite] ? 1 : 0;
    out->gershgorin_max = as_double(kSpecRawGershgorin);
    out->start_norm = as_double(kSpecRawBeta);
    if (k <= 0 || k > AVS_SPECTRUM_MAX_STEPS) return k == 0;
    std::vector<double> diag((size_t)k), off((size_t)k), theta((size_t)k), last((size_t)k);
    bool finite = true;
    for (int j = 0; j < k; ++j) {
        diag[(size_t)j] = as_double(kSpecRawAlpha + j);
        off[(size_t)j] = as_double(kSpecRawBeta + j + 1); // off[k - 1] = beta[k]: the residual norm behind the last step
        finite = finite && std::isfinite(diag[(size_t)j]) && std::isfinite(off[(size_t)j]);
    }
    if (!finite) { // a step left a NaN or an Inf: no spectrum
        const double nan = std::numeric_limits<double>::quiet_NaN();
        if (ritz)
            for (int j = 0; j < k; ++j) ritz[j] = nan;
        out->lambda_min = out->lambda_max = out->lambda_min_bound = out->lambda_max_bound = out->condition_estimate = nan;
        return true;
    }
    if (!spectrum_tridiagonal(k, diag.data(), off.data(), theta.data(), last.data())) return false;
    if (ritz)
        for (int j = 0; j < k; ++j) ritz[j] = theta[(size_t)j];
    out->lambda_min = theta[0];
    out->lambda_max = theta[(size_t)k - 1];
    out->lambda_min_bound = off[(size_t)k - 1] * std::fabs(last[0]);
    out->lambda_max_bound = off[(size_t)k - 1] * std::fabs(last[(size_t)k - 1]);
    out->indefinite = out->lambda_min <= 0. ? 1 : 0;
    out->condition_estimate = out->indefinite ? std::numeric_limits<double>::infinity() : out->lambda_max / out->lambda_min;
    out->iteration_bound = spectrum_iteration_bound(out->condition_estimate, ask.tolerance);
    return true;
}

// alpha (steps), beta (steps + 1): the device's values up to what the steps taken wrote, 0 behind; either may be null
inline void spectrum_scalars(const unsigned long long *raw, int32_t steps, double *alpha, double *beta)
{
    if (alpha) {
        if (raw) memcpy(alpha, raw + kSpecRawAlpha, (size_t)steps * sizeof(double));
        else memset(alpha, 0, (size_t)steps * sizeof(double));
    }
    if (beta) {
        if (raw) memcpy(beta, raw + kSpecRawBeta, ((size_t)steps + 1) * sizeof(double));
        else memset(beta, 0, ((size_t)steps + 1) * sizeof(double));
    }
}

} // namespace avs
