// avs_pcg_f32.inl -- what only the float-vector PCG loops of AVS_PRECISION_F32 contexts have (included by avs_pcg.hip, inside namespace
// avs): narrowing and widening, Eigen's float threshold, the streaming float SpMV with its dispatcher, and the product probe.  The host
// loop is pcg_solve_phases<float>, and the vector and set-up kernels are k_update_r / k_update_xp<float, float, ...>, k_init_residual<float>,
// k_init_p<float, .>, k_inv_diag<float> and prepare_diagonal<float> (all avs_pcg.hip), shared with the fp64 and mixed solves.
//
// The reference built with USESINGLEPRECISION (HDK_Utilities.h:25-37: SolveType = fpreal32, Vector = Eigen::VectorXf) hands a
// SparseMatrix<float> to Eigen::ConjugateGradient (HDK_AdaptiveViscosity.cpp:613-630): matrix values, vectors AND scalars are floats.
// Until round 5 this library assembled that float system bit for bit and then iterated on it in fp64; here the iteration itself runs on
// float vectors:
//   * x, r, p, A p and the inverse diagonal are float arrays (4 B per row and stream instead of 8: the vector kernels of the fp64 loop
//     run at the HBM roofline, so this halves their time);
//   * alpha = absNew / p.Ap, beta = absNew / absOld and the threshold tol^2 |b|^2 are computed in float from float operands;
//   * every row sum is a float sum left to right in the stored column order (one multiply, one add per entry, no FMA), exactly
//     the oracle's SPMV_F (oracle/avs_oracle.c: orc_pcg_csr_f32);
//   * dot products: a thread's own terms are added in float, everything across threads, workgroups and launches in double, and the
//     total is rounded to float where Eigen would hold a float.  Eigen's own (vectorised, 4-accumulator) reduction order is not
//     reproduced -- neither is it by the oracle, whose float dots run left to right --, so iteration counts agree with the oracle's
//     to a few per cent and the solution to the accuracy float CG reaches, not bit for bit.
// The SpMV is the brick kernel instantiated for float vectors where the matrix has the form (k_spmv_brick<DOT, VC, float>: the lattice
// in LDS is half as large), else a plain streaming kernel over the CSR arrays (value index or 8-B values).
// Control flow: pcg_solve_phases -- three launches per iteration with the scalar steps fused into the vector kernels, chunks of kChunk
// iterations replayed from a captured hipGraph, avs_cancel polled between chunks.

__global__ __launch_bounds__(kBlock) void k_f32_narrow(int64_t n, const double *__restrict__ src, float *__restrict__ dst)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) dst[i] = (float)src[i];
}
__global__ __launch_bounds__(kBlock) void k_f32_widen(int64_t n, const float *__restrict__ src, double *__restrict__ dst)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) dst[i] = (double)src[i];
}

// Eigen's float threshold: tol^2 |b|^2 in float, at least the smallest normal float (ConjugateGradient.h: considerAsZero =
// (std::numeric_limits<RealScalar>::min)()); b.b and r.r arrive as double sums of float terms
__global__ void k_f32_threshold(PcgScalars *sc, double tol)
{
    if (threadIdx.x != 0 || blockIdx.x != 0 || sc->done == 3) return;
    const float rhs = (float)sc->rhs_norm2, t = (float)tol;
    float thr = t * t * rhs;
    if (thr < 1.17549435e-38f) thr = 1.17549435e-38f;
    sc->threshold = (double)thr;
    sc->rhs_norm2 = (double)rhs;
    sc->rr = (double)(float)sc->rr;
    sc->done = ((float)sc->rr < thr) ? 1 : 0;
}

// y = A x for any CsrView (8-B values, one dictionary, tile-local dictionaries): coalesced stream of (column, value) -> float products
// parked in LDS -> every row adds its segment left to right.  256 rows per workgroup (a workgroup lies inside one 512-row tile: its
// dictionary base is uniform).  The systems that land here are small (no brick form: < 2 M rows) and cache-resident.
// V = double (the mixed-precision loop of fp64 contexts, avs_pcg_mixed.inl): the values are not narrowed, every product is
// (double)x * val, the row sum is a double sum left to right and is rounded to float once, when y is stored.
template <bool DOT, typename V = float>
__global__ __launch_bounds__(kBlock) void k_f32_spmv_csr(CsrView A, const float *__restrict__ x, float *__restrict__ y,
                                                         double *__restrict__ partial, const PcgScalars *sc)
{
    if (DOT && sc && sc->done) return;
    __shared__ V prod[kStreamCap];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kBlock;
    const int64_t row = row0 + tid;
    const int64_t rlast = (row0 + kBlock < A.n) ? row0 + kBlock : A.n;
    const int s_blk = A.row_ptr[row0];
    const int e_blk = A.row_ptr[rlast];
    const int tbase = A.tab_ptr ? A.tab_ptr[row0 / kTileRows] : 0;
    int rs = 0, re = 0;
    if (row < A.n) {
        rs = A.row_ptr[row];
        re = A.row_ptr[row + 1];
    }
    V sum = 0;
    for (int ts = s_blk; ts < e_blk; ts += kStreamCap) {
        const int te = (ts + kStreamCap < e_blk) ? ts + kStreamCap : e_blk;
        for (int k0 = ts + tid; k0 < te; k0 += 4 * kBlock) {
            int c[4];
            V v[4];
            float xv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = k0 + u * kBlock < te ? k0 + u * kBlock : ts;
                c[u] = A.col[k];
                v[u] = A.val && !A.codes ? (V)A.val[k] : (V)A.table[tbase + A.codes[k]];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) xv[u] = x[c[u]];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (k0 + u * kBlock < te) prod[k0 + u * kBlock - ts] = v[u] * (V)xv[u];
        }
        __syncthreads();
        const int a = rs > ts ? rs : ts;
        const int b = re < te ? re : te;
        for (int j = a; j < b; ++j) sum += prod[j - ts];
        __syncthreads();
    }
    if (row < A.n) y[row] = (float)sum;
    if (DOT) {
        double d = (row < A.n) ? (double)(sum * (V)x[row]) : 0.;
        d = block_sum(d, red);
        if (tid == 0) partial[blockIdx.x] = d;
    }
}

template <bool DOT>
static avs_status spmv_f32_dispatch(const CsrView &A, const float *x, float *y, double *partial, const PcgScalars *sc, hipStream_t stream, int *nblocks)
{
    if (A.n <= 0) { if (nblocks) *nblocks = 0; return AVS_OK; }
    if (A.brick && A.brick->ntiles > 0 && A.brick->pwords32) {
        if (nblocks) *nblocks = brick_partial_count(*A.brick, 4);
        return spmv_brick_launch_f32(*A.brick, x, y, DOT ? partial : nullptr, (DOT && sc) ? &sc->done : nullptr, stream);
    }
    const int g = stream_grid(A.n);
    hipLaunchKernelGGL((k_f32_spmv_csr<DOT>), dim3(g), dim3(kBlock), 0, stream, A, x, y, partial, sc);
    if (nblocks) *nblocks = g;
    AVS_HIP(hipGetLastError());
    return AVS_OK;
}

#ifdef AVS_PROBES
// probe / test entry of a float loop's product: y = A x (x holds float values; y is widened), + the folded partial sums of the fused dot.
// product(DOT, x, y, partial): the loop's dispatcher; n_cols: the entries of x; brick_partials: what the brick form's fused dot writes
template <typename P>
static avs_status spmv_float_probe(const CsrView &A, const double *x, double *y, bool fused, double *dot_out, hipStream_t st, int64_t n_cols,
                                   size_t brick_partials, P &&product)
{
    const int64_t n = A.n;
    DevBuf<float> xf, yf;
    DevBuf<double> partial;
    AVS_TRY(xf.alloc((size_t)n_cols + 8));
    AVS_TRY(yf.alloc((size_t)n + 8));
    const int g = stream_grid(n) < kVecGrid ? stream_grid(n) : kVecGrid;
    hipLaunchKernelGGL(k_f32_narrow, dim3(g), dim3(kBlock), 0, st, n_cols, x, xf.p);
    if (!fused) {
        AVS_TRY(product(std::false_type{}, xf.p, yf.p, nullptr));
    } else {
        size_t np = (size_t)stream_grid(n) + 16;
        if (brick_partials > np) np = brick_partials;
        AVS_TRY(partial.alloc(np));
        AVS_HIP(hipMemsetAsync(partial.p, 0, np * sizeof(double), st));
        AVS_TRY(product(std::true_type{}, xf.p, yf.p, partial.p));
        if (dot_out) {
            std::vector<double> h(np);
            AVS_HIP(hipMemcpyAsync(h.data(), partial.p, np * sizeof(double), hipMemcpyDeviceToHost, st));
            AVS_HIP(hipStreamSynchronize(st));
            double s = 0.;
            for (double v : h) s += v;
            *dot_out = s;
        }
    }
    hipLaunchKernelGGL(k_f32_widen, dim3(g), dim3(kBlock), 0, st, n, (const float *)yf.p, y);
    AVS_HIP(hipGetLastError());
    AVS_HIP(hipStreamSynchronize(st));
    return AVS_OK;
}
avs_status spmv_f32_probe(const CsrView &A, const double *x, double *y, bool fused, double *dot_out, hipStream_t st)
{
    return spmv_float_probe(A, x, y, fused, dot_out, st, A.n, A.brick ? (size_t)brick_partial_count(*A.brick, 4) : 0,
                            [&](auto DOT, const float *xf, float *yf, double *partial) {
                                return spmv_f32_dispatch<DOT.value>(A, xf, yf, partial, nullptr, st, nullptr);
                            });
}
#endif // AVS_PROBES
