// Stand-alone driver of the host side of avs_estimate_spectrum that needs no HIP call (csrc/avs_spectrum_report.hpp: argument checks, the
// eigenvalues of the Lanczos tridiagonal with the last components of its extreme eigenvectors, the bounds, the raw words turned into
// avs_spectrum, the struct_size hand-over, iteration_bound at its edges).  tests/test_spectrum_host.py writes spectrum_report_constants.hpp
// (tridiagonals of the model's recurrences with numpy's eigenvalues), builds this file with the host sanitizers
// (-fsanitize=address,undefined) and runs it; it prints "ok" and exits 0, or says which expectation failed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "avs_spectrum_report.hpp"

// struct TriCase { int k; const double *alpha, *beta (k + 1, beta[0] the start norm), *ritz; double last_min, last_max, gap_min, gap_max; }
// kTriCases[], kTriCaseCount, kHashEntry[4] (rows 0, 1, 255, 65536)
#include "spectrum_report_constants.hpp"

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

static double norm_inf(int k, const double *alpha, const double *beta)
{
    double m = 0.;
    for (int i = 0; i < k; ++i) {
        const double row = std::fabs(alpha[i]) + (i > 0 ? std::fabs(beta[i]) : 0.) + (i + 1 < k ? std::fabs(beta[i + 1]) : 0.);
        m = row > m ? row : m;
    }
    return m;
}

static std::vector<unsigned long long> raw_of(const TriCase &c)
{
    std::vector<unsigned long long> raw(kSpecRawWords, 0ull);
    raw[kSpecRawStepsTaken] = (unsigned long long)c.k;
    for (int i = 0; i < c.k; ++i) raw[kSpecRawAlpha + i] = bits_of(c.alpha[i]);
    for (int i = 0; i <= c.k; ++i) raw[kSpecRawBeta + i] = bits_of(c.beta[i]);
    raw[kSpecRawGershgorin] = bits_of(7.5);
    return raw;
}

int main()
{
    static_assert(sizeof(avs_spectrum) == 136, "layout of avs_spectrum");
    static_assert(kSpecRawWords == 6 + 2 * AVS_SPECTRUM_MAX_STEPS + 1, "raw words");
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity(), eps = std::ldexp(1., -52);
    const char *why = nullptr;
    avs_spectrum rep;
    std::memset(&rep, 0, sizeof(rep));
    rep.struct_size = (int32_t)sizeof(rep);
    // argument checks
    EXPECT(spectrum_args(AVS_SPECTRUM_OF_JACOBI, AVS_SPECTRUM_START_RESIDUAL, 1, AVS_MEM_HOST, &rep, true, &why) == AVS_OK);
    EXPECT(spectrum_args(AVS_SPECTRUM_OF_MATRIX, AVS_SPECTRUM_START_HASH, AVS_SPECTRUM_MAX_STEPS, AVS_MEM_DEVICE, &rep, true, &why) == AVS_OK);
    EXPECT(spectrum_args(AVS_SPECTRUM_OF_MATRIX, AVS_SPECTRUM_START_VECTOR, 7, AVS_MEM_DEVICE, &rep, false, &why) == AVS_OK);
    why = nullptr;
    EXPECT(spectrum_args(AVS_SPECTRUM_OF_MATRIX, AVS_SPECTRUM_START_VECTOR, 7, AVS_MEM_DEVICE, &rep, true, &why) == AVS_EINVAL && why); // no such vector in a context
    for (int32_t op : {-1, 2, 7, INT32_MIN, INT32_MAX}) {
        why = nullptr;
        EXPECT(spectrum_args(op, AVS_SPECTRUM_START_HASH, 8, AVS_MEM_HOST, &rep, false, &why) == AVS_EINVAL && why);
    }
    for (int32_t start : {-1, 3, INT32_MIN, INT32_MAX}) {
        why = nullptr;
        EXPECT(spectrum_args(AVS_SPECTRUM_OF_JACOBI, start, 8, AVS_MEM_HOST, &rep, false, &why) == AVS_EINVAL && why);
    }
    for (int32_t steps : {0, -1, AVS_SPECTRUM_MAX_STEPS + 1, INT32_MIN, INT32_MAX}) {
        why = nullptr;
        EXPECT(spectrum_args(AVS_SPECTRUM_OF_JACOBI, AVS_SPECTRUM_START_HASH, steps, AVS_MEM_HOST, &rep, false, &why) == AVS_EINVAL && why);
    }
    for (int where : {-1, 2, 7, INT32_MAX}) {
        why = nullptr;
        EXPECT(spectrum_args(AVS_SPECTRUM_OF_JACOBI, AVS_SPECTRUM_START_HASH, 8, where, &rep, false, &why) == AVS_EINVAL && why);
    }
    why = nullptr;
    EXPECT(spectrum_args(AVS_SPECTRUM_OF_JACOBI, AVS_SPECTRUM_START_HASH, 8, AVS_MEM_HOST, nullptr, false, &why) == AVS_EINVAL && why);
    for (int32_t size : {0, 4, 7, -8, 4097, INT32_MIN, INT32_MAX}) {
        rep.struct_size = size;
        why = nullptr;
        EXPECT(spectrum_args(AVS_SPECTRUM_OF_JACOBI, AVS_SPECTRUM_START_HASH, 8, AVS_MEM_HOST, &rep, false, &why) == AVS_EINVAL && why);
    }
    for (int32_t size : {8, 40, 136, 4096}) {
        rep.struct_size = size;
        EXPECT(spectrum_args(AVS_SPECTRUM_OF_JACOBI, AVS_SPECTRUM_START_HASH, 8, AVS_MEM_HOST, &rep, false, &why) == AVS_OK);
    }
    EXPECT(spectrum_sizes(0, 0, &why) == AVS_OK && spectrum_sizes(INT32_MAX, INT32_MAX, &why) == AVS_OK);
    for (int64_t bad : {(int64_t)-1, (int64_t)INT32_MAX + 1, INT64_MIN, INT64_MAX}) {
        why = nullptr;
        EXPECT(spectrum_sizes(bad, 0, &why) == AVS_EINVAL && why);
        why = nullptr;
        EXPECT(spectrum_sizes(0, bad, &why) == AVS_EINVAL && why);
    }
    // the hash start vector
    EXPECT(spectrum_hash_entry(0) == kHashEntry[0] && spectrum_hash_entry(1) == kHashEntry[1] && spectrum_hash_entry(255) == kHashEntry[2] &&
           spectrum_hash_entry(65536) == kHashEntry[3]);
    EXPECT(spectrum_splitmix64(0) == 0xE220A8397B1DCDAFull);
    // the tridiagonal eigen step against numpy's, within 4 k eps |T|_inf (both methods are backward stable to O(k) eps |T|); the last
    // components of the extreme eigenvectors within that perturbation over the gap to the next eigenvalue
    for (int t = 0; t < kTriCaseCount; ++t) {
        const TriCase &c = kTriCases[t];
        std::vector<double> ritz((size_t)c.k), last((size_t)c.k);
        EXPECT(spectrum_tridiagonal(c.k, c.alpha, c.beta + 1, ritz.data(), last.data()));
        const double tnorm = norm_inf(c.k, c.alpha, c.beta), tol = 4. * c.k * eps * tnorm;
        double sum2 = 0.;
        for (int i = 0; i < c.k; ++i) {
            if (!(std::fabs(ritz[(size_t)i] - c.ritz[i]) <= tol)) std::fprintf(stderr, "case %d ritz %d: %.17g against %.17g, tolerance %.3g\n", t, i, ritz[(size_t)i], c.ritz[i], tol);
            EXPECT(std::fabs(ritz[(size_t)i] - c.ritz[i]) <= tol);
            EXPECT(i == 0 || ritz[(size_t)i - 1] <= ritz[(size_t)i]);
            sum2 += last[(size_t)i] * last[(size_t)i];
        }
        EXPECT(std::fabs(sum2 - 1.) <= 4. * c.k * eps); // the last ROW of an orthogonal matrix
        EXPECT(std::fabs(std::fabs(last[0]) - c.last_min) <= tol / c.gap_min + 4. * c.k * eps);
        EXPECT(std::fabs(std::fabs(last[(size_t)c.k - 1]) - c.last_max) <= tol / c.gap_max + 4. * c.k * eps);
        // ... and through the report
        const std::vector<unsigned long long> raw = raw_of(c);
        SpectrumAsk ask;
        ask.op = AVS_SPECTRUM_OF_MATRIX;
        ask.start = AVS_SPECTRUM_START_HASH;
        ask.steps = c.k < AVS_SPECTRUM_MAX_STEPS ? c.k + 1 : c.k;
        ask.n = 1000;
        ask.nnz = 2998;
        ask.tolerance = 1e-3;
        std::vector<double> out((size_t)ask.steps, -1.), a((size_t)ask.steps, -1.), b((size_t)ask.steps + 1, -1.);
        avs_spectrum full;
        EXPECT(spectrum_report(raw.data(), ask, true, out.data(), &full));
        spectrum_scalars(raw.data(), ask.steps, a.data(), b.data());
        EXPECT(full.struct_size == (int32_t)sizeof(full) && full.evaluated == 1 && full.op == ask.op && full.start == ask.start && full.steps_asked == ask.steps);
        EXPECT(full.steps_taken == c.k && full.breakdown == 0 && full.nonfinite == 0 && full.n == 1000 && full.nnz == 2998 && full.bad_diagonal == 0);
        EXPECT(full.start_norm == c.beta[0] && full.gershgorin_max == 7.5 && full.tolerance == 1e-3);
        EXPECT(full.lambda_min == ritz[0] && full.lambda_max == ritz[(size_t)c.k - 1]);
        EXPECT(full.lambda_min_bound == c.beta[c.k] * std::fabs(last[0]) && full.lambda_max_bound == c.beta[c.k] * std::fabs(last[(size_t)c.k - 1]));
        EXPECT(full.indefinite == (ritz[0] <= 0. ? 1 : 0));
        if (full.indefinite) {
            EXPECT(full.condition_estimate == inf && full.iteration_bound == -1);
        } else {
            EXPECT(full.condition_estimate == full.lambda_max / full.lambda_min);
            EXPECT(full.iteration_bound == (int64_t)std::ceil(0.5 * std::sqrt(full.condition_estimate) * std::log(2. / 1e-3)));
        }
        for (int i = 0; i < ask.steps; ++i) {
            EXPECT(out[(size_t)i] == (i < c.k ? ritz[(size_t)i] : 0.));
            EXPECT(bits_of(a[(size_t)i]) == (i < c.k ? bits_of(c.alpha[i]) : 0ull));
        }
        for (int i = 0; i <= ask.steps; ++i) EXPECT(bits_of(b[(size_t)i]) == (i <= c.k ? bits_of(c.beta[i]) : 0ull));
    }
    // small and split tridiagonals
    {
        double r[3], l[3];
        const double d1[1] = {-2.5}, none[1] = {0.};
        EXPECT(spectrum_tridiagonal(0, d1, none, r, l));
        EXPECT(spectrum_tridiagonal(1, d1, none, r, l) && r[0] == -2.5 && l[0] == 1.);
        const double d2[2] = {2., 2.}, e2[1] = {1.};
        EXPECT(spectrum_tridiagonal(2, d2, e2, r, l) && std::fabs(r[0] - 1.) <= 8 * eps && std::fabs(r[1] - 3.) <= 8 * eps);
        EXPECT(std::fabs(std::fabs(l[0]) - std::sqrt(0.5)) <= 8 * eps && std::fabs(std::fabs(l[1]) - std::sqrt(0.5)) <= 8 * eps);
        const double d3[3] = {5., 1., 3.}, e3[2] = {0., 0.}; // already diagonal: sorted, and the last component follows its eigenvalue
        EXPECT(spectrum_tridiagonal(3, d3, e3, r, l) && r[0] == 1. && r[1] == 3. && r[2] == 5. && l[0] == 0. && l[1] == 1. && l[2] == 0.);
        EXPECT(spectrum_tridiagonal(3, d3, e3, r, nullptr) && r[2] == 5.);
    }
    // the report where no step was taken, where nothing was evaluated, and behind a non-finite step
    {
        SpectrumAsk ask;
        ask.op = AVS_SPECTRUM_OF_JACOBI;
        ask.start = AVS_SPECTRUM_START_RESIDUAL;
        ask.steps = 4;
        ask.n = 10;
        ask.nnz = 28;
        ask.tolerance = 1e-8;
        double out[4] = {-1., -1., -1., -1.}, a[4], b[5];
        avs_spectrum full;
        EXPECT(spectrum_report(nullptr, ask, true, out, &full)); // n == 0
        EXPECT(full.evaluated == 1 && full.steps_taken == 0 && full.iteration_bound == -1 && full.lambda_min == 0. && full.condition_estimate == 0. && out[3] == 0.);
        EXPECT(spectrum_report(nullptr, ask, false, out, &full)); // seam A: rule 0 or 1
        avs_spectrum zero;
        std::memset(&zero, 0, sizeof(zero));
        zero.struct_size = (int32_t)sizeof(zero);
        zero.op = ask.op;
        zero.start = ask.start;
        zero.steps_asked = 4;
        zero.n = 10;
        zero.nnz = 28;
        zero.tolerance = 1e-8;
        EXPECT(std::memcmp(&full, &zero, sizeof(full)) == 0);
        spectrum_scalars(nullptr, 4, a, b);
        EXPECT(a[0] == 0. && a[3] == 0. && b[0] == 0. && b[4] == 0.);
        spectrum_scalars(nullptr, 4, nullptr, nullptr);
        std::vector<unsigned long long> raw(kSpecRawWords, 0ull);
        raw[kSpecRawBadDiagonal] = 3ull;
        EXPECT(spectrum_report(raw.data(), ask, true, out, &full));
        zero.bad_diagonal = 3;
        EXPECT(std::memcmp(&full, &zero, sizeof(full)) == 0);
        raw[kSpecRawBadDiagonal] = 0ull; // a zero start vector
        raw[kSpecRawStop] = 1ull;
        raw[kSpecRawGershgorin] = bits_of(2.25);
        EXPECT(spectrum_report(raw.data(), ask, true, out, &full));
        EXPECT(full.evaluated == 1 && full.steps_taken == 0 && full.start_norm == 0. && full.gershgorin_max == 2.25 && full.iteration_bound == -1 && full.indefinite == 0);
        raw[kSpecRawBeta] = bits_of(nan); // a start norm that is not finite
        raw[kSpecRawNonfinite] = 1ull;
        EXPECT(spectrum_report(raw.data(), ask, true, out, &full));
        EXPECT(full.nonfinite == 1 && full.steps_taken == 0 && std::isnan(full.start_norm) && full.lambda_max == 0.);
        raw[kSpecRawBeta] = bits_of(2.); // step 1 left alpha[1] = Inf
        raw[kSpecRawStepsTaken] = 2ull;
        raw[kSpecRawAlpha] = bits_of(1.);
        raw[kSpecRawAlpha + 1] = bits_of(inf);
        raw[kSpecRawBeta + 1] = bits_of(0.5);
        raw[kSpecRawBeta + 2] = bits_of(nan);
        EXPECT(spectrum_report(raw.data(), ask, true, out, &full));
        EXPECT(full.steps_taken == 2 && full.nonfinite == 1 && std::isnan(full.lambda_min) && std::isnan(full.lambda_max) && std::isnan(full.lambda_min_bound) &&
               std::isnan(full.condition_estimate) && full.iteration_bound == -1 && full.indefinite == 0);
        EXPECT(std::isnan(out[0]) && std::isnan(out[1]) && out[2] == 0. && out[3] == 0.);
        raw[kSpecRawAlpha + 1] = bits_of(-3.); // an indefinite tridiagonal, stopped by a breakdown
        raw[kSpecRawBeta + 2] = bits_of(0.);
        raw[kSpecRawNonfinite] = 0ull;
        raw[kSpecRawBreakdown] = 1ull;
        EXPECT(spectrum_report(raw.data(), ask, true, nullptr, &full));
        EXPECT(full.breakdown == 1 && full.indefinite == 1 && full.lambda_min < -3. && full.lambda_max > 1. && full.condition_estimate == inf &&
               full.iteration_bound == -1 && full.lambda_min_bound == 0. && full.lambda_max_bound == 0.);
        // only struct_size bytes change hands
        for (int32_t size : {8, 12, 40, 64, 128, 136, 200}) {
            unsigned char buf[256];
            std::memset(buf, 0x5a, sizeof(buf));
            avs_spectrum *o = reinterpret_cast<avs_spectrum *>(buf);
            o->struct_size = size;
            report_hand_over(full, o);
            const size_t n = (size_t)size < sizeof(full) ? (size_t)size : sizeof(full);
            EXPECT(o->struct_size == size && std::memcmp(buf + 4, reinterpret_cast<const unsigned char *>(&full) + 4, n - 4) == 0);
            for (size_t i = n; i < sizeof(buf); ++i) EXPECT(buf[i] == 0x5a);
        }
    }
    // iteration_bound at its edges
    EXPECT(spectrum_iteration_bound(1., 1e-3) == (int64_t)std::ceil(0.5 * std::log(2000.)));
    EXPECT(spectrum_iteration_bound(4., 0.5) == 2); // ceil(0.5 * 2 * ln 4) = ceil(1.386)
    EXPECT(spectrum_iteration_bound(1e300, 1e-300) > 0 && spectrum_iteration_bound(1.7e308, 5e-324) == INT64_MAX);
    for (double tol : {0., 1., 2., -1e-3, nan, inf, -inf}) EXPECT(spectrum_iteration_bound(100., tol) == -1);
    for (double kappa : {inf, nan, 0.5, 0., -4., -inf}) EXPECT(spectrum_iteration_bound(kappa, 1e-3) == -1);
    std::printf("ok\n");
    return 0;
}
