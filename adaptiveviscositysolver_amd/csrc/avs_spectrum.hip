// avs_spectrum.hip -- why does a solve take the iterations it takes?  m steps of the symmetric Lanczos recurrence on S A S (S = D^-1/2 of
// the Jacobi preconditioner, or I) in fp64 from the plain reference-numbered CSR: avs_estimate_spectrum (the system a context
// assembled) and avs_estimate_csr_spectrum (seam A) over one implementation.  Every convention is stated in include/avs.h
// (avs_estimate_spectrum); tests/spectrum_model.py restates them in NumPy.
//
//   k_spectrum_scale       one lane per row: the last diagonal entry d_i, s_i = 1 / sqrt(d_i), bad diagonals counted (s_i = 0)
//   k_spectrum_gershgorin  one lane per row: g_i = g_i + |val[k]| * (s_i * s_col[k]) in stored order; the maximum as a bit pattern
//   k_spectrum_start       the start vector into w and the partial sums of w_i^2: s o (b - A x0) by the stream product, the hash, or the
//                          caller's vector
//   k_spectrum_product     the stream product of k_solution_check on u = s o v_j (chunk_stream_product, avs_report_device.hpp): a
//                          256-thread workgroup owns a chunk of 256 consecutive rows, persistent workgroups walk the chunks.  Then
//                          t_i = s_i * y_i - beta[j] * v_{j-1,i} into w and the chunk's partial sum of v_{j,i} t_i (chunk_partial_sum).
//   k_spectrum_orthogonalise  w_i = t_i - alpha[j] * v_{j,i} in place and the chunk's partial sum of w_i^2
//   k_spectrum_fold        one workgroup folds the partial sums in a fixed order (thread t adds the chunks t, t + 256, ..., then the
//                          block sum of avs_wave.hpp) and writes beta[0], alpha[j] or beta[j + 1]; behind beta it decides the stop
//   k_spectrum_advance     v_{j+1} = w / beta[j + 1] over the memory of v_{j-1} (the two Lanczos vectors change roles on the host: no
//                          copy), u = s o v_{j+1}, and the caller's basis column
//
// Bytes per step: 12 nnz + 4 n for the matrix, and about 80 n for the vectors (product: s, v, v_{j-1} read, w written, u gathered out
// of L2; orthogonalise: w, v read, w written; advance: w, s read, v, u written).  The whole recurrence is enqueued without a host
// wait: the stop decision is a word in device memory that every kernel reads uniformly at entry.  A partial sum belongs to a chunk, not
// to a workgroup, so the sums do not depend on the grid (Options::cells_grid_cap caps it for the tests).  No floating atomics, no
// hipGraph, no cooperative launch.  No index is read from a caller's array before rules 0 and 1 of avs_check_csr have passed on it.
#include "avs_internal.hpp"
#include "avs_report_device.hpp"
#include "avs_spectrum_report.hpp"

namespace avs {

// nothing behind a bad diagonal, a useless start vector, a breakdown or a non-finite step: the same answer in every thread of the grid
__device__ __forceinline__ bool spec_halted(const unsigned long long *raw)
{
    return raw[kSpecRawStop] != 0ull || raw[kSpecRawBadDiagonal] != 0ull;
}
__device__ __forceinline__ double spec_word(const unsigned long long *raw, int word) { return __longlong_as_double((long long)raw[word]); }

template <bool JACOBI>
__global__ __launch_bounds__(kBlock) void k_spectrum_scale(const int32_t *__restrict__ rp, const int32_t *__restrict__ col, const double *__restrict__ val, int n,
                                                           double *__restrict__ s, unsigned long long *raw)
{
    unsigned long long bad = 0ull;
    for (long long row = (long long)blockIdx.x * kBlock + threadIdx.x; row < n; row += (long long)gridDim.x * kBlock) {
        double si = 1.;
        if (JACOBI) {
            double d = 0.;
            bool have = false;
            const int e = rp[row + 1];
            for (int k = rp[row]; k < e; ++k)
                if (col[k] == (int)row) {
                    d = val[k];
                    have = true;
                }
            const bool ok = have && d > 0. && finite_bits(d);
            si = ok ? 1.0 / sqrt(d) : 0.;
            bad += ok ? 0ull : 1ull;
        }
        s[row] = si;
    }
    raw_add(bad, kSpecRawBadDiagonal, raw);
}

__global__ __launch_bounds__(kBlock) void k_spectrum_gershgorin(const int32_t *__restrict__ rp, const int32_t *__restrict__ col, const double *__restrict__ val,
                                                                const double *__restrict__ s, int n, unsigned long long *raw)
{
    if (spec_halted(raw)) return;
    unsigned long long m = 0ull;
    for (long long row = (long long)blockIdx.x * kBlock + threadIdx.x; row < n; row += (long long)gridDim.x * kBlock) {
        const double si = s[row];
        double g = 0.;
        const int e = rp[row + 1];
        for (int k = rp[row]; k < e; ++k) g = g + fabs(val[k]) * (si * s[col[k]]);
        if (!(g < __longlong_as_double(0x7ff0000000000000ll))) g = __longlong_as_double(0x7ff0000000000000ll); // NaN or +Inf
        const unsigned long long bits = (unsigned long long)__double_as_longlong(g); // g >= 0: the bit patterns order as the values
        m = bits > m ? bits : m;
    }
    raw_max_bits(m, kSpecRawGershgorin, raw);
}

// START: AVS_SPECTRUM_START_*.  b, x0: RESIDUAL only; start_vector: VECTOR only.
template <int START>
__global__ __launch_bounds__(kBlock) void k_spectrum_start(const int32_t *__restrict__ rp, const int32_t *__restrict__ col, const double *__restrict__ val,
                                                           const double *__restrict__ b, const double *__restrict__ x0, const double *__restrict__ start_vector,
                                                           const double *__restrict__ s, int n, long long chunks, double *__restrict__ w,
                                                           double *__restrict__ partial, const unsigned long long *raw)
{
    __shared__ double prod[START == AVS_SPECTRUM_START_RESIDUAL ? kStreamCap : 1];
    __shared__ double red[2][4];
    if (spec_halted(raw)) return;
    int parity = 0;
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x, parity ^= 1) { // (the same trips for every thread of the workgroup)
        const long long row0 = chunk * kBlock, row = row0 + threadIdx.x;
        double y = 0.;
        if (START == AVS_SPECTRUM_START_RESIDUAL) y = chunk_stream_product(rp, col, val, x0, n, row0, prod);
        double term = 0.;
        if (row < n) {
            double v;
            if (START == AVS_SPECTRUM_START_RESIDUAL) {
                const double r = b[row] - y;
                v = s[row] * r;
            } else if (START == AVS_SPECTRUM_START_HASH) {
                v = (double)(spectrum_splitmix64((uint64_t)row) >> 11) * (1.0 / 9007199254740992.0) - 0.5;
            } else {
                v = start_vector[row];
            }
            w[row] = v;
            term = v * v;
        }
        chunk_partial_sum(term, red, parity, partial + chunk);
    }
}

// t = S A u - beta[j] v_{j-1} into w, and the partial sums of v_j . t
__global__ __launch_bounds__(kBlock) void k_spectrum_product(const int32_t *__restrict__ rp, const int32_t *__restrict__ col, const double *__restrict__ val,
                                                             const double *__restrict__ u, const double *__restrict__ s, const double *__restrict__ v,
                                                             const double *__restrict__ vprev, int j, int n, long long chunks, double *__restrict__ w,
                                                             double *__restrict__ partial, const unsigned long long *raw)
{
    __shared__ double prod[kStreamCap];
    __shared__ double red[2][4];
    if (spec_halted(raw)) return;
    const double beta = spec_word(raw, kSpecRawBeta + j);
    int parity = 0;
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x, parity ^= 1) {
        const long long row0 = chunk * kBlock, row = row0 + threadIdx.x;
        const double y = chunk_stream_product(rp, col, val, u, n, row0, prod);
        double term = 0.;
        if (row < n) {
            double t = s[row] * y;
            if (j > 0) t = t - beta * vprev[row];
            w[row] = t;
            term = v[row] * t;
        }
        chunk_partial_sum(term, red, parity, partial + chunk);
    }
}

// w = t - alpha[j] v_j in place, and the partial sums of w . w
__global__ __launch_bounds__(kBlock) void k_spectrum_orthogonalise(const double *__restrict__ v, int j, int n, long long chunks, double *__restrict__ w,
                                                                   double *__restrict__ partial, const unsigned long long *raw)
{
    __shared__ double red[2][4];
    if (spec_halted(raw)) return;
    const double alpha = spec_word(raw, kSpecRawAlpha + j);
    int parity = 0;
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x, parity ^= 1) {
        const long long row = chunk * kBlock + threadIdx.x;
        double term = 0.;
        if (row < n) {
            const double wi = w[row] - alpha * v[row];
            w[row] = wi;
            term = wi * wi;
        }
        chunk_partial_sum(term, red, parity, partial + chunk);
    }
}

enum { kSpecFoldStart = 0, kSpecFoldAlpha = 1, kSpecFoldBeta = 2 };

// one workgroup.  kSpecFoldStart: beta[0]; kSpecFoldAlpha: alpha[j]; kSpecFoldBeta: beta[j + 1] and the stop decision of step j
__global__ __launch_bounds__(kBlock) void k_spectrum_fold(const double *__restrict__ partial, long long chunks, int what, int j, unsigned long long *raw)
{
    __shared__ double lds4[4];
    if (spec_halted(raw)) return;
    double sum = 0.;
    for (long long i = threadIdx.x; i < chunks; i += kBlock) sum = sum + partial[i];
    sum = block_sum(sum, lds4);
    if (threadIdx.x != 0) return;
    if (what == kSpecFoldAlpha) {
        raw[kSpecRawAlpha + j] = (unsigned long long)__double_as_longlong(sum);
        return;
    }
    const double beta = sqrt(sum);
    if (what == kSpecFoldStart) {
        raw[kSpecRawBeta] = (unsigned long long)__double_as_longlong(beta);
        if (!finite_bits(beta)) raw[kSpecRawNonfinite] = 1ull;
        if (!finite_bits(beta) || !(beta > 0.)) raw[kSpecRawStop] = 1ull;
        return;
    }
    raw[kSpecRawBeta + j + 1] = (unsigned long long)__double_as_longlong(beta);
    raw[kSpecRawStepsTaken] = (unsigned long long)(j + 1);
    const double alpha = spec_word(raw, kSpecRawAlpha + j), before = spec_word(raw, kSpecRawBeta + j);
    if (!finite_bits(alpha) || !finite_bits(beta)) {
        raw[kSpecRawNonfinite] = 1ull;
        raw[kSpecRawStop] = 1ull;
    } else if (!(beta > kSpecBreakdown * (fabs(alpha) + before))) {
        raw[kSpecRawBreakdown] = 1ull;
        raw[kSpecRawStop] = 1ull;
    }
}

// v_next = w / beta[index], u = s o v_next; column: the caller's basis column on the device, or null
__global__ __launch_bounds__(kBlock) void k_spectrum_advance(const double *__restrict__ w, const double *__restrict__ s, int index, int n,
                                                             double *__restrict__ v_next, double *__restrict__ u, double *__restrict__ column,
                                                             const unsigned long long *raw)
{
    if (spec_halted(raw)) return;
    const double beta = spec_word(raw, kSpecRawBeta + index);
    for (long long row = (long long)blockIdx.x * kBlock + threadIdx.x; row < n; row += (long long)gridDim.x * kBlock) {
        const double vi = w[row] / beta;
        v_next[row] = vi;
        u[row] = s[row] * vi;
        if (column) column[row] = vi;
    }
}

struct SpectrumSource { // device pointers; b, x0, start_vector: as the start needs them
    int64_t n, nnz;
    const int32_t *row_ptr, *col;
    const double *val, *b, *x0, *start_vector;
};

struct SpectrumOutputs { // the caller's; any may be null.  alpha, beta, ritz: host
    double *alpha, *beta, *ritz, *scale, *basis;
};

// report and the small arrays where no kernel ran
static avs_status spectrum_without_rows(const SpectrumAsk &ask, bool evaluated, const SpectrumOutputs &out, avs_spectrum *report)
{
    avs_spectrum full;
    (void)spectrum_report(nullptr, ask, evaluated, out.ritz, &full);
    spectrum_scalars(nullptr, ask.steps, out.alpha, out.beta);
    report_hand_over(full, report);
    return AVS_OK;
}

// The shared implementation: the arguments are checked, the arrays of src lie on the device of st and its indices may be followed.
// Returns once the report and every output are complete.
static avs_status estimate_spectrum(SpectrumScratch &S, const SpectrumSource &src, hipStream_t st, const SpectrumAsk &ask, int grid_cap,
                                    const SpectrumOutputs &out, avs_memspace where, avs_spectrum *report)
{
    const int n = (int)src.n;
    if (n == 0) return spectrum_without_rows(ask, true, out, report);
    const int m = ask.steps < n ? ask.steps : n;
    const long long chunks = ((long long)n + kBlock - 1) / kBlock;
    const unsigned grid = report_grid(chunks, grid_cap);
    const bool direct = where == AVS_MEM_DEVICE;
    const size_t vec = (size_t)n * sizeof(double);
    AVS_TRY(S.s.reserve((size_t)n));
    AVS_TRY(S.u.reserve((size_t)n));
    AVS_TRY(S.va.reserve((size_t)n));
    AVS_TRY(S.vb.reserve((size_t)n));
    AVS_TRY(S.w.reserve((size_t)n));
    AVS_TRY(S.partial.reserve((size_t)chunks));
    AVS_TRY(S.raw.begin(kSpecRawWords, -1, st));
    unsigned long long *raw = S.raw.p;
    if (out.basis && !direct) { // the column copies behind a stop copy what the two vectors hold: never memory nobody wrote
        AVS_HIP(hipMemsetAsync(S.va.p, 0, vec, st));
        AVS_HIP(hipMemsetAsync(S.vb.p, 0, vec, st));
    }
    if (ask.op == AVS_SPECTRUM_OF_JACOBI)
        hipLaunchKernelGGL(k_spectrum_scale<true>, dim3(grid), dim3(kBlock), 0, st, src.row_ptr, src.col, src.val, n, S.s.p, raw);
    else
        hipLaunchKernelGGL(k_spectrum_scale<false>, dim3(grid), dim3(kBlock), 0, st, src.row_ptr, src.col, src.val, n, S.s.p, raw);
    if (out.scale) AVS_HIP(copy_out(out.scale, S.s.p, vec, where, st));
    hipLaunchKernelGGL(k_spectrum_gershgorin, dim3(grid), dim3(kBlock), 0, st, src.row_ptr, src.col, src.val, (const double *)S.s.p, n, raw);
    if (ask.start == AVS_SPECTRUM_START_RESIDUAL)
        hipLaunchKernelGGL(k_spectrum_start<AVS_SPECTRUM_START_RESIDUAL>, dim3(grid), dim3(kBlock), 0, st, src.row_ptr, src.col, src.val, src.b, src.x0,
                           src.start_vector, (const double *)S.s.p, n, chunks, S.w.p, S.partial.p, (const unsigned long long *)raw);
    else if (ask.start == AVS_SPECTRUM_START_HASH)
        hipLaunchKernelGGL(k_spectrum_start<AVS_SPECTRUM_START_HASH>, dim3(grid), dim3(kBlock), 0, st, src.row_ptr, src.col, src.val, src.b, src.x0,
                           src.start_vector, (const double *)S.s.p, n, chunks, S.w.p, S.partial.p, (const unsigned long long *)raw);
    else
        hipLaunchKernelGGL(k_spectrum_start<AVS_SPECTRUM_START_VECTOR>, dim3(grid), dim3(kBlock), 0, st, src.row_ptr, src.col, src.val, src.b, src.x0,
                           src.start_vector, (const double *)S.s.p, n, chunks, S.w.p, S.partial.p, (const unsigned long long *)raw);
    hipLaunchKernelGGL(k_spectrum_fold, dim3(1), dim3(kBlock), 0, st, (const double *)S.partial.p, chunks, (int)kSpecFoldStart, 0, raw);
    double *v = S.va.p, *vprev = S.vb.p;
    // column j of the caller's basis: written by the kernel on the device, copied behind it to the host (behind a stop the copies still
    // run and copy what the two vectors hold: zeros or earlier columns, the unspecified columns of include/avs.h)
    const auto column = [&](int j) { return out.basis && direct ? out.basis + (size_t)j * (size_t)n : nullptr; };
    hipLaunchKernelGGL(k_spectrum_advance, dim3(grid), dim3(kBlock), 0, st, (const double *)S.w.p, (const double *)S.s.p, 0, n, v, S.u.p, column(0),
                       (const unsigned long long *)raw);
    if (out.basis && !direct) AVS_HIP(copy_out(out.basis, v, vec, where, st));
    for (int j = 0; j < m; ++j) {
        hipLaunchKernelGGL(k_spectrum_product, dim3(grid), dim3(kBlock), 0, st, src.row_ptr, src.col, src.val, (const double *)S.u.p, (const double *)S.s.p,
                           (const double *)v, (const double *)vprev, j, n, chunks, S.w.p, S.partial.p, (const unsigned long long *)raw);
        hipLaunchKernelGGL(k_spectrum_fold, dim3(1), dim3(kBlock), 0, st, (const double *)S.partial.p, chunks, (int)kSpecFoldAlpha, j, raw);
        hipLaunchKernelGGL(k_spectrum_orthogonalise, dim3(grid), dim3(kBlock), 0, st, (const double *)v, j, n, chunks, S.w.p, S.partial.p,
                           (const unsigned long long *)raw);
        hipLaunchKernelGGL(k_spectrum_fold, dim3(1), dim3(kBlock), 0, st, (const double *)S.partial.p, chunks, (int)kSpecFoldBeta, j, raw);
        // v_{j+1} over the memory of v_{j-1}: the product of step j + 1 reads v_j as its v_{j-1}
        hipLaunchKernelGGL(k_spectrum_advance, dim3(grid), dim3(kBlock), 0, st, (const double *)S.w.p, (const double *)S.s.p, j + 1, n, vprev, S.u.p,
                           column(j + 1), (const unsigned long long *)raw);
        if (out.basis && !direct) AVS_HIP(copy_out(out.basis + (size_t)(j + 1) * (size_t)n, vprev, vec, where, st));
        double *const was = v;
        v = vprev;
        vprev = was;
    }
    std::vector<unsigned long long> words(kSpecRawWords);
    AVS_TRY(S.raw.read(words.data(), st));
    avs_spectrum full;
    const bool converged = spectrum_report(words.data(), ask, true, out.ritz, &full);
    spectrum_scalars(words.data(), ask.steps, out.alpha, out.beta);
    report_hand_over(full, report);
    AVS_REQUIRE(converged, AVS_EINTERNAL, "spectrum: the eigenvalues of the Lanczos tridiagonal did not converge");
    return AVS_OK;
}

} // namespace avs

using namespace avs;

extern "C" avs_status avs_estimate_spectrum(avs_ctx *c, int32_t op, int32_t start, int32_t steps, double tolerance, double *alpha, double *beta, double *ritz,
                                            double *scale, double *basis, avs_memspace where, avs_spectrum *report)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c, AVS_EINVAL, "null argument");
    const char *why = nullptr;
    if (spectrum_args(op, start, steps, (int)where, report, true, &why) != AVS_OK) {
        set_error("%s", why);
        return AVS_EINVAL;
    }
    AVS_REQUIRE(!c->slab.on, AVS_ESTATE, "avs_estimate_spectrum: the context holds a slab-local pre-pass (this rank's window only)");
    AVS_REQUIRE(c->system_ready, AVS_ESTATE, "avs_estimate_spectrum: no system (avs_assemble; after avs_dist_assemble no global matrix exists)");
    AVS_REQUIRE(c->guess_ready && !c->guess_partial && c->x0.p, AVS_ESTATE, "avs_estimate_spectrum: no initial guess: call avs_assemble first");
    if (spectrum_sizes(c->n_vel, c->nnz, &why) != AVS_OK) {
        set_error("%s", why);
        return AVS_ESTATE;
    }
    AVS_HIP(hipSetDevice(c->desc.device));
    const SpectrumSource src{c->n_vel, c->nnz, c->row_ptr.p, c->col.p, c->val.p, c->rhs.p, c->x0.p, nullptr};
    SpectrumAsk ask;
    ask.op = op;
    ask.start = start;
    ask.steps = steps;
    ask.n = c->n_vel;
    ask.nnz = c->nnz;
    ask.tolerance = tolerance;
    Scope scope("Spectrum Estimate");
    return estimate_spectrum(c->spectrum, src, c->stream, ask, c->opt.cells_grid_cap, SpectrumOutputs{alpha, beta, ritz, scale, basis}, where, report);
}

extern "C" avs_status avs_estimate_csr_spectrum(int64_t n, int64_t nnz, const int32_t *row_ptr, const int32_t *col, const double *val, const double *b,
                                                const double *x0, const double *start_vector, int32_t op, int32_t start, int32_t steps, double tolerance,
                                                double *alpha, double *beta, double *ritz, double *scale, double *basis, avs_memspace where, int32_t device,
                                                void *stream, avs_spectrum *report)
{
    avs::OptScope opt_scope_(nullptr); // context-free entry, like avs_check_csr
    const char *why = nullptr;
    if (spectrum_args(op, start, steps, (int)where, report, false, &why) != AVS_OK || spectrum_sizes(n, nnz, &why) != AVS_OK) {
        set_error("%s", why);
        return AVS_EINVAL;
    }
    AVS_REQUIRE(row_ptr && (nnz == 0 || (col && val)), AVS_EINVAL, "spectrum: null argument (row_ptr, or col / val with nnz > 0)");
    AVS_REQUIRE(n == 0 || start != AVS_SPECTRUM_START_RESIDUAL || (b && x0), AVS_EINVAL, "spectrum: null argument (b or x0 with AVS_SPECTRUM_START_RESIDUAL)");
    AVS_REQUIRE(n == 0 || start != AVS_SPECTRUM_START_VECTOR || start_vector, AVS_EINVAL, "spectrum: null argument (start_vector with AVS_SPECTRUM_START_VECTOR)");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    AVS_REQUIRE(e == hipSuccess && ndev > 0, AVS_EHIP, "no HIP device available (%s)", hipGetErrorString(e));
    AVS_REQUIRE(device >= 0 && device < ndev, AVS_EINVAL, "device %d out of range", device);
    AVS_HIP(hipSetDevice(device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    bool own = false;
    if (!s) {
        AVS_HIP(hipStreamCreate(&s));
        own = true;
    }
    const bool residual = start == AVS_SPECTRUM_START_RESIDUAL, given = start == AVS_SPECTRUM_START_VECTOR;
    SpectrumAsk ask;
    ask.op = op;
    ask.start = start;
    ask.steps = steps;
    ask.n = n;
    ask.nnz = nnz;
    ask.tolerance = tolerance;
    const SpectrumOutputs out{alpha, beta, ritz, scale, basis};
    avs_status rc = AVS_OK;
    {
        CsrCheckScratch rules;
        SpectrumScratch scratch;
        DevBuf<int32_t> d_rp, d_col;
        DevBuf<double> d_val, d_b, d_x0, d_start;
        SpectrumSource src{n, nnz, row_ptr, col, val, residual ? b : nullptr, residual ? x0 : nullptr, given ? start_vector : nullptr};
        do {
            if (where == AVS_MEM_HOST) { // staged: n + 1 pointers, nnz entries, n vector elements, as the caller states them
                if ((rc = d_rp.alloc((size_t)n + 1)) || (rc = d_col.alloc((size_t)nnz)) || (rc = d_val.alloc((size_t)nnz)) ||
                    (residual && ((rc = d_b.alloc((size_t)n)) || (rc = d_x0.alloc((size_t)n)))) || (given && (rc = d_start.alloc((size_t)n))))
                    break;
                if (hipMemcpyAsync(d_rp.p, row_ptr, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
                    (nnz > 0 && hipMemcpyAsync(d_col.p, col, (size_t)nnz * 4, hipMemcpyHostToDevice, s) != hipSuccess) ||
                    (nnz > 0 && hipMemcpyAsync(d_val.p, val, (size_t)nnz * 8, hipMemcpyHostToDevice, s) != hipSuccess) ||
                    (residual && n > 0 && hipMemcpyAsync(d_b.p, b, (size_t)n * 8, hipMemcpyHostToDevice, s) != hipSuccess) ||
                    (residual && n > 0 && hipMemcpyAsync(d_x0.p, x0, (size_t)n * 8, hipMemcpyHostToDevice, s) != hipSuccess) ||
                    (given && n > 0 && hipMemcpyAsync(d_start.p, start_vector, (size_t)n * 8, hipMemcpyHostToDevice, s) != hipSuccess)) {
                    set_error("host -> device copy failed");
                    rc = AVS_EHIP;
                    break;
                }
                src.row_ptr = d_rp.p;
                src.col = d_col.p;
                src.val = d_val.p;
                src.b = residual ? d_b.p : nullptr;
                src.x0 = residual ? d_x0.p : nullptr;
                src.start_vector = given ? d_start.p : nullptr;
            }
            // the caller's col is an address: rules 0 and 1 of avs_check_csr before any gather
            avs_csr_check rep01;
            memset(&rep01, 0, sizeof(rep01));
            rep01.struct_size = (int32_t)sizeof(rep01);
            const CsrCheckSource csr{n, nnz, src.row_ptr, src.col, src.val, nullptr, nullptr};
            if ((rc = check_csr(rules, csr, s, 0u, 0., &rep01)) != AVS_OK) break;
            if (rep01.violations[AVS_CSR_RULE_ROW_PTR] != 0 || rep01.violations[AVS_CSR_RULE_COLUMN] != 0) {
                rc = spectrum_without_rows(ask, false, out, report);
                break;
            }
            rc = estimate_spectrum(scratch, src, s, ask, cur_opt().cells_grid_cap, out, where, report);
        } while (0);
        (void)hipStreamSynchronize(s);
    }
    if (own) (void)hipStreamDestroy(s);
    return rc;
}
