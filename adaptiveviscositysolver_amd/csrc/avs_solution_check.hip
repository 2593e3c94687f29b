// avs_solution_check.hip -- did x solve A x = b?  The true residual r = b - A x in fp64 from the plain reference-numbered CSR, whatever
// storage form and loop produced x: avs_check_solution (the system a context assembled) and avs_check_csr_solution (seam A) over one
// implementation.  Every convention is stated in include/avs.h (avs_check_solution); tests/solution_check_model.py restates them in NumPy.
//
//   k_solution_check  the stream product of avs_spmv.hip with the report behind it.  A 256-thread workgroup owns a chunk of 256 consecutive
//                     rows, persistent workgroups walk the chunks: y_i = y_i + val[k] * x[col[k]] in stored order (chunk_stream_product,
//                     avs_report_device.hpp: the order of k_spmv_stream and of the oracle, r is defined bit for bit).  Then
//                     r_i = b_i - y_i, the row's five terms, and one partial sum per term and CHUNK: wave sums without the LDS crossbar,
//                     the four waves added in order by thread 0.
//   k_solution_fold   workgroups 0 .. 4 fold the partial sums of one term each in a fixed order (thread t adds the chunks t, t + 256, ...,
//                     then the block sum of avs_wave.hpp); workgroup 5 picks the largest |r_i| and the smallest row that attains it from
//                     the pairs the waves of the grid left behind.
//
// Bytes per call: 12 nnz + 4 (n + 1) + 24 n (b, x, x0; x is gathered out of L2) + 8 n for the residual: HBM-bound, the matrix stream is
// nine tenths of it.  A partial sum belongs to a chunk, not to a workgroup, so the sums do not depend on the grid (Options::cells_grid_cap
// caps it for the tests).  Counters are 64-bit integers and the maxima the bit patterns of non-negative doubles: a lane accumulates in
// registers over its chunks, a wave folds its lanes and issues one integer atomic per word it has something for (avs_report_device.hpp).  The arg-max is a pair
// (bits of |r_i|, row) under a total order (sol_check_better): lane, wave and fold keep the better pair, so the answer is the same
// whoever compares first.  No floating atomics: the same arrays give the same bytes.  No index is read from a caller's array before
// rules 0 and 1 of avs_check_csr have passed on it (check_csr, what = 0); the context's own arrays are the library's.
#include "avs_internal.hpp"
#include "avs_report_device.hpp"
#include "avs_solution_check_report.hpp"

namespace avs {

// the best pair of the wave, in every lane
__device__ __forceinline__ void sol_wave_best(unsigned long long &bits, unsigned &row)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long ob = (unsigned long long)__shfl_xor((long long)bits, o, 64);
        const unsigned orow = (unsigned)__shfl_xor((int)row, o, 64);
        if (sol_check_better(ob, orow, bits, row)) {
            bits = ob;
            row = orow;
        }
    }
}

// x0, residual: may be null.  partial: kSolSums x chunks; wave_bits / wave_row: one pair per wave of the grid.
__global__ __launch_bounds__(kBlock) void k_solution_check(const int32_t *__restrict__ rp, const int32_t *__restrict__ col, const double *__restrict__ val,
                                                           const double *__restrict__ b, const double *__restrict__ x, const double *__restrict__ x0, int n,
                                                           long long chunks, double *__restrict__ residual, double *__restrict__ partial,
                                                           unsigned long long *__restrict__ wave_bits, unsigned *__restrict__ wave_row,
                                                           unsigned long long *__restrict__ raw)
{
    __shared__ double prod[kStreamCap];
    __shared__ double red[2][kSolSums][4]; // by the parity of the workgroup's trip: thread 0 may still read one while the next is written
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned nonfinite_x = 0u, nonfinite_b = 0u, nonfinite_r = 0u, summed = 0u;
    double max_x = 0., max_update = 0.;
    unsigned long long best_bits = 0ull;
    unsigned best_row = kSolNoRow;
    int parity = 0;
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x, parity ^= 1) { // (the same trips for every thread of the workgroup)
        const long long row0 = chunk * kBlock, row = row0 + tid;
        const double y = chunk_stream_product(rp, col, val, x, n, row0, prod);
        double term[kSolSums] = {0., 0., 0., 0., 0.};
        if (row < n) {
            const double xi = x[row], bi = b[row];
            const double r = bi - y;
            if (residual) residual[row] = r;
            const bool fx = finite_bits(xi), fb = finite_bits(bi), fr = finite_bits(r);
            nonfinite_x += fx ? 0u : 1u;
            nonfinite_b += fb ? 0u : 1u;
            nonfinite_r += fr ? 0u : 1u;
            if (fx && fb && fr) { // (hence y is finite too)
                ++summed;
                term[kSolSumRhs] = bi * bi;
                term[kSolSumResidual] = r * r;
                term[kSolSumXAx] = xi * y;
                term[kSolSumXB] = xi * bi;
                max_x = fmax(max_x, fabs(xi));
                const unsigned long long bits = (unsigned long long)__double_as_longlong(fabs(r));
                if (sol_check_better(bits, (unsigned)row, best_bits, best_row)) {
                    best_bits = bits;
                    best_row = (unsigned)row;
                }
                if (x0) {
                    const double gi = x0[row];
                    if (finite_bits(gi)) {
                        const double d = xi - gi;
                        term[kSolSumUpdate] = d * d;
                        max_update = fmax(max_update, fabs(d));
                    }
                }
            }
        }
        // the chunk's five partial sums: wave sums (in lane 63), then ((w0 + w1) + w2) + w3 as block_sum of avs_wave.hpp adds them
#pragma unroll
        for (int q = 0; q < kSolSums; ++q) {
            const double w = wave_sum_dpp(term[q]);
            if (lane == 63) red[parity][q][wave] = w;
        }
        __syncthreads();
        if (tid < kSolSums)
            partial[(long long)tid * chunks + chunk] = ((red[parity][tid][0] + red[parity][tid][1]) + red[parity][tid][2]) + red[parity][tid][3];
    }
    raw_add(nonfinite_x, kSolRawNonfiniteX, raw);
    raw_add(nonfinite_b, kSolRawNonfiniteB, raw);
    raw_add(nonfinite_r, kSolRawNonfiniteResidual, raw);
    raw_add(summed, kSolRawRowsSummed, raw);
    raw_max_bits(max_x, kSolRawMaxX, raw);
    raw_max_bits(max_update, kSolRawMaxUpdate, raw);
    sol_wave_best(best_bits, best_row);
    if (lane == 0) {
        wave_bits[blockIdx.x * (kBlock / 64) + wave] = best_bits;
        wave_row[blockIdx.x * (kBlock / 64) + wave] = best_row;
    }
}

__global__ __launch_bounds__(kBlock) void k_solution_fold(const double *__restrict__ partial, long long chunks, const unsigned long long *__restrict__ wave_bits,
                                                          const unsigned *__restrict__ wave_row, int waves, unsigned long long *__restrict__ raw)
{
    __shared__ double lds4[4];
    __shared__ unsigned long long best_b[4];
    __shared__ unsigned best_r[4];
    if (blockIdx.x < kSolSums) {
        const double *p = partial + (long long)blockIdx.x * chunks;
        double s = 0.;
        for (long long i = threadIdx.x; i < chunks; i += kBlock) s = s + p[i];
        s = block_sum(s, lds4);
        if (threadIdx.x == 0) raw[kSolRawSums + blockIdx.x] = (unsigned long long)__double_as_longlong(s);
        return;
    }
    unsigned long long bits = 0ull;
    unsigned row = kSolNoRow;
    for (int i = threadIdx.x; i < waves; i += kBlock)
        if (sol_check_better(wave_bits[i], wave_row[i], bits, row)) {
            bits = wave_bits[i];
            row = wave_row[i];
        }
    sol_wave_best(bits, row);
    if ((threadIdx.x & 63) == 0) {
        best_b[threadIdx.x >> 6] = bits;
        best_r[threadIdx.x >> 6] = row;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (sol_check_better(best_b[w], best_r[w], bits, row)) {
                bits = best_b[w];
                row = best_r[w];
            }
        raw[kSolRawMaxResidual] = bits;
        raw[kSolRawMaxResidualRow] = (unsigned long long)row;
    }
}

struct SolutionCheckSource { // device pointers; x0: may be null
    int64_t n, nnz;
    const int32_t *row_ptr, *col;
    const double *val, *b, *x, *x0;
};

// The shared implementation: the arguments are checked, the arrays of src lie on the device of st and its indices may be followed.
// residual: the caller's (device: written in place; host: staged), or null.  Returns once the report (and a host residual) is complete.
static avs_status check_solution(SolutionCheckScratch &S, const SolutionCheckSource &src, hipStream_t st, int32_t which, int grid_cap,
                                 const SolutionClaim &claim, double *residual, avs_memspace where, avs_solution_check *report)
{
    const int n = (int)src.n;
    if (n == 0) {
        if (report) report_hand_over(check_solution_report(nullptr, which, src.n, src.nnz, true, claim), report);
        return AVS_OK;
    }
    const long long chunks = ((long long)n + kBlock - 1) / kBlock;
    const unsigned grid = report_grid(chunks, grid_cap);
    const int waves = (int)grid * (kBlock / 64);
    const bool direct = where == AVS_MEM_DEVICE;
    double *d_res = residual;
    if (residual && !direct) {
        AVS_TRY(S.residual.reserve((size_t)n));
        d_res = S.residual.p;
    }
    AVS_TRY(S.partial.reserve((size_t)(kSolSums * chunks)));
    AVS_TRY(S.wave_bits.reserve((size_t)waves));
    AVS_TRY(S.wave_row.reserve((size_t)waves));
    AVS_TRY(S.raw.begin(kSolRawWords, -1, st));
    hipLaunchKernelGGL(k_solution_check, dim3(grid), dim3(kBlock), 0, st, src.row_ptr, src.col, src.val, src.b, src.x, src.x0, n, chunks, d_res,
                       S.partial.p, S.wave_bits.p, S.wave_row.p, S.raw.p);
    if (report)
        hipLaunchKernelGGL(k_solution_fold, dim3(kSolSums + 1), dim3(kBlock), 0, st, (const double *)S.partial.p, chunks,
                           (const unsigned long long *)S.wave_bits.p, (const unsigned *)S.wave_row.p, waves, S.raw.p);
    AVS_HIP(hipGetLastError());
    if (residual && !direct) AVS_HIP(copy_out(residual, d_res, (size_t)n * sizeof(double), where, st));
    unsigned long long raw[kSolRawWords];
    if (report) AVS_TRY(S.raw.read(raw, st));
    else if (!direct) AVS_HIP(hipStreamSynchronize(st));
    if (report) report_hand_over(check_solution_report(raw, which, src.n, src.nnz, true, claim), report);
    return AVS_OK;
}

} // namespace avs

using namespace avs;

extern "C" avs_status avs_check_solution(avs_ctx *c, int32_t which, double *residual, avs_solution_check *report, avs_memspace where)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c, AVS_EINVAL, "null argument");
    const char *why = nullptr;
    if (check_solution_args(which, (int)where, residual, report, false, &why) != AVS_OK) {
        set_error("%s", why);
        return AVS_EINVAL;
    }
    AVS_REQUIRE(!c->slab.on, AVS_ESTATE, "avs_check_solution: the context holds a slab-local pre-pass (this rank's window only)");
    AVS_REQUIRE(c->system_ready, AVS_ESTATE, "avs_check_solution: no system (avs_assemble; after avs_dist_assemble no global matrix exists)");
    AVS_REQUIRE(c->guess_ready && !c->guess_partial && c->x0.p, AVS_ESTATE, "avs_check_solution: no initial guess: call avs_assemble first");
    if (which == AVS_CHECK_OF_SOLUTION)
        AVS_REQUIRE(c->solved && c->x.p, AVS_ESTATE, "avs_check_solution: no solution: call avs_solve / avs_set_solution first");
    if (check_solution_sizes(c->n_vel, c->nnz, &why) != AVS_OK) {
        set_error("%s", why);
        return AVS_ESTATE;
    }
    AVS_HIP(hipSetDevice(c->desc.device));
    SolutionClaim claim;
    if (which == AVS_CHECK_OF_SOLUTION && c->claim_gen != 0 && c->claim_gen == c->solution_gen) {
        claim.known = true;
        claim.converged = c->claim.converged;
        claim.iterations = c->claim.iterations;
        claim.error = c->claim.error;
    }
    const SolutionCheckSource src{c->n_vel, c->nnz, c->row_ptr.p, c->col.p, c->val.p, c->rhs.p, which == AVS_CHECK_OF_SOLUTION ? c->x.p : c->x0.p,
                                  c->x0.p};
    Scope scope("Solution Check");
    return check_solution(c->solution_check, src, c->stream, which, c->opt.cells_grid_cap, claim, residual, where, report);
}

extern "C" avs_status avs_check_csr_solution(int64_t n, int64_t nnz, const int32_t *row_ptr, const int32_t *col, const double *val, const double *b,
                                             const double *x, const double *x0, double *residual, avs_memspace where, int32_t device, void *stream,
                                             avs_solution_check *report)
{
    avs::OptScope opt_scope_(nullptr); // context-free entry, like avs_check_csr
    const char *why = nullptr;
    if (check_solution_args(AVS_CHECK_OF_SOLUTION, (int)where, residual, report, true, &why) != AVS_OK || check_solution_sizes(n, nnz, &why) != AVS_OK) {
        set_error("%s", why);
        return AVS_EINVAL;
    }
    AVS_REQUIRE(row_ptr && (nnz == 0 || (col && val)), AVS_EINVAL, "solution check: null argument (row_ptr, or col / val with nnz > 0)");
    AVS_REQUIRE(n == 0 || (b && x), AVS_EINVAL, "solution check: null argument (b or x with n > 0)");
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
    avs_status rc = AVS_OK;
    {
        CsrCheckScratch rules;
        SolutionCheckScratch scratch;
        DevBuf<int32_t> d_rp, d_col;
        DevBuf<double> d_val, d_b, d_x, d_x0;
        SolutionCheckSource src{n, nnz, row_ptr, col, val, b, x, x0};
        do {
            if (where == AVS_MEM_HOST) { // staged: n + 1 pointers, nnz entries, n vector elements, as the caller states them
                if ((rc = d_rp.alloc((size_t)n + 1)) || (rc = d_col.alloc((size_t)nnz)) || (rc = d_val.alloc((size_t)nnz)) || (rc = d_b.alloc((size_t)n)) ||
                    (rc = d_x.alloc((size_t)n)) || (x0 && (rc = d_x0.alloc((size_t)n))))
                    break;
                if (hipMemcpyAsync(d_rp.p, row_ptr, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
                    (nnz > 0 && hipMemcpyAsync(d_col.p, col, (size_t)nnz * 4, hipMemcpyHostToDevice, s) != hipSuccess) ||
                    (nnz > 0 && hipMemcpyAsync(d_val.p, val, (size_t)nnz * 8, hipMemcpyHostToDevice, s) != hipSuccess) ||
                    (n > 0 && hipMemcpyAsync(d_b.p, b, (size_t)n * 8, hipMemcpyHostToDevice, s) != hipSuccess) ||
                    (n > 0 && hipMemcpyAsync(d_x.p, x, (size_t)n * 8, hipMemcpyHostToDevice, s) != hipSuccess) ||
                    (x0 && n > 0 && hipMemcpyAsync(d_x0.p, x0, (size_t)n * 8, hipMemcpyHostToDevice, s) != hipSuccess)) {
                    set_error("host -> device copy failed");
                    rc = AVS_EHIP;
                    break;
                }
                src.row_ptr = d_rp.p;
                src.col = d_col.p;
                src.val = d_val.p;
                src.b = d_b.p;
                src.x = d_x.p;
                src.x0 = x0 ? d_x0.p : nullptr;
            }
            // the caller's col is an address: rules 0 and 1 of avs_check_csr before any gather
            avs_csr_check rep01;
            memset(&rep01, 0, sizeof(rep01));
            rep01.struct_size = (int32_t)sizeof(rep01);
            const CsrCheckSource csr{n, nnz, src.row_ptr, src.col, src.val, nullptr, nullptr};
            if ((rc = check_csr(rules, csr, s, 0u, 0., &rep01)) != AVS_OK) break;
            if (rep01.violations[AVS_CSR_RULE_ROW_PTR] != 0 || rep01.violations[AVS_CSR_RULE_COLUMN] != 0) {
                report_hand_over(check_solution_report(nullptr, AVS_CHECK_OF_SOLUTION, n, nnz, false, SolutionClaim()), report);
                break;
            }
            rc = check_solution(scratch, src, s, AVS_CHECK_OF_SOLUTION, cur_opt().cells_grid_cap, SolutionClaim(), residual, where, report);
        } while (0);
        (void)hipStreamSynchronize(s);
    }
    if (own) (void)hipStreamDestroy(s);
    return rc;
}
