// avs_pcg_mixed.inl -- kernels and SpMV dispatcher of the mixed-precision PCG loop of AVS_PRECISION_F64 contexts
// (AVS_OPTION_MIXED_PRECISION; included by avs_pcg.hip behind avs_pcg_f32.inl, inside namespace avs).  The host loop is
// pcg_solve_phases<float, true> (avs_pcg.hip), shared with the fp64 and float solves; this is the scheme it runs.
//
// The fp64 launch-per-phase loop is bound by the bytes of its vectors.  The mixed loop iterates on 4-byte vectors and keeps the answer
// and the stopping test in fp64 ("reliable updates" / residual replacement):
//   fp64:  the solution x and the right-hand side b (the context's arrays), one scratch vector t64, the matrix values, every row sum of
//          A p (rounded to float once, when it is stored), every dot product across threads / workgroups / launches, alpha, beta, rho,
//          the threshold tol^2 |b|^2 and the residual norm the solve reports;
//   float: r, p, t = A p, the correction xf (x_true = x + xf) and the inverse diagonal; a thread's own dot terms.
// One chunk of kChunk iterations (captured and replayed like the other loops' chunks) runs the float recurrence
//   t = A p ; alpha = rho / p.t ; r -= alpha t ; xf += alpha p ; beta = rho' / rho ; p = D^-1 r + beta p
// and freezes, as the other loops do, when the recurrence's r.r falls below the threshold.  Behind EVERY chunk the update follows,
// outside the graph:  x += xf ; xf = 0  ->  t64 = A x (the fp64 product of the fp64 loop)  ->  r = (float)(b - t64), with |b - t64|^2 and
// rho = r.D^-1 r summed in fp64.  The fp64 sum decides: below the threshold the solve has converged; else `done` is cleared and the
// next chunk goes on from the true residual with the SAME search direction (restarting p = z at every update costs more than three
// times the iterations; replacing r only when the recurrence claims convergence stalls -- DESIGN.md 4.1a).  Where the recurrence froze
// the chunk mid-way, xf already holds that iteration's alpha p and p still owes its beta step: the update takes it with the true
// residual's z, p = z + (rho_new / rho_old) p, and the iteration counts.
// Nothing here imitates Eigen-in-float: the scalars are doubles (a float tol^2 |b|^2 underflows for small right-hand sides).

template <bool DOT>
static avs_status spmv_mixed_dispatch(const CsrView &A, const float *x, float *y, double *partial, const PcgScalars *sc, hipStream_t stream,
                                      int *nblocks)
{
    if (A.n <= 0) { if (nblocks) *nblocks = 0; return AVS_OK; }
    if (A.brick && A.brick->ntiles > 0 && A.brick->pwords32) {
        if (nblocks) *nblocks = brick_partial_count_mixed(*A.brick);
        return spmv_brick_launch_mixed(*A.brick, x, y, DOT ? partial : nullptr, (DOT && sc) ? &sc->done : nullptr, stream);
    }
    const int g = stream_grid(A.n);
    hipLaunchKernelGGL((k_f32_spmv_csr<DOT, double>), dim3(g), dim3(kBlock), 0, stream, A, x, y, partial, sc);
    if (nblocks) *nblocks = g;
    AVS_HIP(hipGetLastError());
    return AVS_OK;
}

// x += xf ; xf = 0 (16 B per row read, 12 written)
__global__ __launch_bounds__(kBlock) void k_mixed_fold(int64_t n, double *__restrict__ x, float *__restrict__ xf, const PcgScalars *sc)
{
    if (sc->done == 3) return;
    const int64_t n4 = n >> 2;
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < n4; j += (int64_t)gridDim.x * kBlock) {
        const int64_t i = 4 * j;
        const f4_t c = *reinterpret_cast<const f4_t *>(xf + i);
        d2_t a = *reinterpret_cast<const d2_t *>(x + i), b = *reinterpret_cast<const d2_t *>(x + i + 2);
        a.x += (double)c.x; a.y += (double)c.y; b.x += (double)c.z; b.y += (double)c.w;
        *reinterpret_cast<d2_t *>(x + i) = a;
        *reinterpret_cast<d2_t *>(x + i + 2) = b;
        *reinterpret_cast<f4_t *>(xf + i) = f4_t{0.f, 0.f, 0.f, 0.f};
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = n4 * 4; i < n; ++i) {
            x[i] += (double)xf[i];
            xf[i] = 0.f;
        }
}

// r64 = b - t64 ; r = (float) r64 ; partials: [0..g) |r64|^2, [g..2g) r.(D^-1 r) of the ROUNDED residual (z is not stored), INIT: [2g..3g) b.b.
// All three sums in double.
template <bool CODED, bool INIT>
__global__ __launch_bounds__(kBlock) void k_mixed_residual(int64_t n, const double *__restrict__ b, const double *__restrict__ t64,
                                                           float *__restrict__ r, const float *__restrict__ invd,
                                                           const uint16_t *__restrict__ dcode, double *__restrict__ partial,
                                                           const PcgScalars *sc)
{
    __shared__ double red[4];
    const bool skip = !INIT && sc->done == 3;
    double rr = 0., rz = 0., bb = 0.;
    if (!skip)
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
            const double bi = b[i];
            const double ri = bi - t64[i];
            const float rf = (float)ri;
            r[i] = rf;
            const float zi = (CODED ? invd[dcode[i]] : invd[i]) * rf;
            rr += ri * ri;
            rz += (double)rf * (double)zi;
            if (INIT) bb += bi * bi;
        }
    rr = block_sum(rr, red);
    rz = block_sum(rz, red);
    if (INIT) bb = block_sum(bb, red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = rr;
        partial[gridDim.x + blockIdx.x] = rz;
        if (INIT) partial[2 * gridDim.x + blockIdx.x] = bb;
    }
}

// The scalar step of an update (one workgroup): folds k_mixed_residual's partial sums in a fixed order and applies the fp64 test.
// INIT: the start of the solve (what OP_INIT + OP_RHO0 do for the fp64 loop).  Else: `done` on entry tells whether the recurrence froze
// the chunk (1 / 2); sc->rho holds the r.z the frozen iteration started from (beta_step<float, double> of k_update_xp leaves it there for both parities).
// red[3] = 1: p still owes its beta step (k_mixed_pstep, sc->beta), 0: not.  The next chunk starts at an even position: it reads sc->rho.
template <bool INIT>
__global__ __launch_bounds__(kRedBlock) void k_mixed_finish(const double *__restrict__ partial, int g, PcgScalars *sc, double tol)
{
    __shared__ double red[kRedBlock / 64];
    __shared__ double tot[3];
    for (int q = 0; q < (INIT ? 3 : 2); ++q) {
        double s = 0.;
        for (int i = threadIdx.x; i < g; i += kRedBlock) s += partial[(size_t)q * g + i];
        s = wave_sum(s);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.;
#pragma unroll
            for (int w = 0; w < kRedBlock / 64; ++w) t += red[w];
            tot[q] = t;
        }
    }
    if (threadIdx.x != 0) return;
    const double rr = tot[0], rz = tot[1];
    if (INIT) {
        const double bb = tot[2];
        sc->rhs_norm2 = bb;
        sc->rr = rr;
        sc->iter = 0;
        sc->red[3] = 0.;
        if (bb == 0.) { sc->done = 3; sc->rr = 0.; return; }
        double thr = tol * tol * bb;
        const double considerAsZero = 2.2250738585072014e-308;
        if (thr < considerAsZero) thr = considerAsZero;
        sc->threshold = thr;
        sc->done = (rr < thr) ? 1 : 0;
        sc->rho = rz;
        return;
    }
    if (sc->done == 3) return;
    const bool frozen = sc->done != 0;
    sc->rr = rr;
    sc->red[0] = rr;
    sc->red[1] = rz;
    sc->red[3] = 0.;
    if (rr < sc->threshold) { sc->done = 1; return; } // the fp64 residual has passed Eigen's test: converged
    if (frozen) { // the recurrence's claim is rejected: that iteration counts, and p takes its beta step from the true residual
        sc->beta = rz / sc->rho;
        sc->iter += 1;
        sc->red[3] = 1.;
    }
    sc->rho = rz;
    sc->done = 0;
}

// p = D^-1 r + beta p after an update that rejected the recurrence's convergence claim (rare: most launches return at once)
template <bool CODED>
__global__ __launch_bounds__(kBlock) void k_mixed_pstep(int64_t n, float *__restrict__ p, const float *__restrict__ r, const float *__restrict__ invd,
                                                        const uint16_t *__restrict__ dcode, const PcgScalars *sc)
{
    if (sc->red[3] == 0. || sc->done) return;
    const float beta = (float)sc->beta;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
        p[i] = (CODED ? invd[dcode[i]] : invd[i]) * r[i] + beta * p[i];
}

#ifdef AVS_PROBES
// probe / test entry: y = A x through the mixed-precision loop's product (spmv_float_probe)
// n_cols (0: A.n): the entries of x -- [owned | halo] for the local rows of a partitioned plan
avs_status spmv_mixed_probe(const CsrView &A, const double *x, double *y, bool fused, double *dot_out, hipStream_t st, int64_t n_cols)
{
    return spmv_float_probe(A, x, y, fused, dot_out, st, n_cols < A.n ? A.n : n_cols, A.brick ? (size_t)brick_partial_count_mixed(*A.brick) : 0,
                            [&](auto DOT, const float *xf, float *yf, double *partial) {
                                return spmv_mixed_dispatch<DOT.value>(A, xf, yf, partial, nullptr, st, nullptr);
                            });
}
#endif // AVS_PROBES
