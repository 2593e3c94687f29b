// avs_pcg_mixed.inl -- the mixed-precision PCG loop of AVS_PRECISION_F64 contexts (AVS_OPTION_MIXED_PRECISION; included by avs_pcg.hip
// behind avs_pcg_f32.inl, inside namespace avs).
//
// The fp64 launch-per-phase loop is bound by the bytes of its vectors.  This loop iterates on 4-byte vectors and keeps the answer and
// the stopping test in fp64 ("reliable updates" / residual replacement):
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
// the chunk (1 / 2); sc->rho holds the r.z the frozen iteration started from (k_f32_update_xp<.., DS> leaves it there for both parities).
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

// (KEEP is a template parameter of the vector kernels: see stream_load_k)
#define AVS_MIXED_LAUNCH_R(C, F, ...)                                                                                       \
    do {                                                                                                                    \
        if (keep) hipLaunchKernelGGL((k_f32_update_r<C, F, true, true>), dim3(g), dim3(kBlock), 0, stream, __VA_ARGS__);   \
        else hipLaunchKernelGGL((k_f32_update_r<C, F, false, true>), dim3(g), dim3(kBlock), 0, stream, __VA_ARGS__);       \
    } while (0)
#define AVS_MIXED_LAUNCH_XP(C, ...)                                                                                         \
    do {                                                                                                                    \
        if (keep) hipLaunchKernelGGL((k_f32_update_xp<C, true, true>), dim3(g), dim3(kBlock), 0, stream, __VA_ARGS__);     \
        else hipLaunchKernelGGL((k_f32_update_xp<C, false, true>), dim3(g), dim3(kBlock), 0, stream, __VA_ARGS__);         \
    } while (0)

// b, x: the context's fp64 arrays; x holds the initial guess and receives the solution
static avs_status pcg_solve_mixed(PcgWork *w, const CsrView &A, const double *b, double *x, double tol, int max_iters, hipStream_t stream,
                                  avs_solve_info *info)
{
    const int64_t n = A.n;
    const size_t na = (size_t)n + 8;
    w->float_vectors = 1;
    if (!w->f_x.p) { AVS_TRY(w->f_x.alloc(na)); AVS_TRY(w->f_r.alloc(na)); AVS_TRY(w->f_p.alloc(na)); AVS_TRY(w->f_t.alloc(na)); }
    const bool brick = A.brick && A.brick->ntiles > 0 && A.brick->pwords32;
    {
        size_t need = 2 * ((size_t)((n + kBlock - 1) / kBlock) + 16) + 4 * (size_t)kVecGrid + 16; // the streaming kernel: one partial per 256 rows
        if (brick) { const size_t nb = 2 * ((size_t)A.brick->ntiles * 8 + 16) + 4 * (size_t)kVecGrid + 16; need = nb > need ? nb : need; }
        const size_t upd = 6 * (size_t)kVecGrid + 64; // k_mixed_residual<.., INIT>: three sums of g partials in the upper half
        AVS_TRY(ensure_partials(w, need > upd ? need : upd));
    }
    const int g = vec_grid(n);
    float *xf = w->f_x.p, *p = w->f_p.p, *r = w->f_r.p, *t = w->f_t.p;
    double *t64 = w->t.p, *partial = w->partial.p;
    double *vpart = partial + (w->npartial / 2); // the vector kernels' partial sums (the SpMV's are still being read)
    PcgScalars *sc = w->sc.p;
    const int variant = spmv_default_variant(A);

    AVS_HIP(hipMemsetAsync(sc, 0, sizeof(PcgScalars), stream));
    AVS_HIP(hipMemsetAsync(xf, 0, na * sizeof(float), stream));
    const bool coded = A.codes && !A.tab_ptr && A.table_size <= kViLdsTable;
    float *invd = nullptr;
    AVS_TRY(prepare_diagonal(w, A, coded, nullptr, stream));
    if (coded) {
        if (!w->f_invtab.p) AVS_TRY(w->f_invtab.alloc((size_t)kViLdsTable + 1));
        hipLaunchKernelGGL(k_f32_invtab, dim3((A.table_size + kBlock) / kBlock), dim3(kBlock), 0, stream, A, w->f_invtab.p);
        invd = w->f_invtab.p;
    } else {
        if (!w->f_invd.p) AVS_TRY(w->f_invd.alloc(na));
        hipLaunchKernelGGL(k_f32_inv_diag, dim3(row_grid(n)), dim3(kBlock), 0, stream, A, w->f_invd.p);
        invd = w->f_invd.p;
    }
    const uint16_t *dcode = coded ? w->dcode.p : nullptr;
    AVS_HIP(hipEventRecord(w->ev0, stream));

    // r64 = b - A x in fp64; |b|^2, |r64|^2, rho; r = (float) r64; p = z = D^-1 r
    AVS_TRY(spmv_dispatch<false>(A, x, t64, nullptr, nullptr, variant, stream, nullptr));
    if (coded) hipLaunchKernelGGL((k_mixed_residual<true, true>), dim3(g), dim3(kBlock), 0, stream, n, b, (const double *)t64, r, (const float *)invd, dcode, vpart, (const PcgScalars *)sc);
    else hipLaunchKernelGGL((k_mixed_residual<false, true>), dim3(g), dim3(kBlock), 0, stream, n, b, (const double *)t64, r, (const float *)invd, dcode, vpart, (const PcgScalars *)sc);
    hipLaunchKernelGGL(k_mixed_finish<true>, dim3(1), dim3(kRedBlock), 0, stream, (const double *)vpart, g, sc, tol);
    // (k_f32_init_p's own r.z partials are not used: rho is the fp64 sum above)
    if (coded) hipLaunchKernelGGL(k_f32_init_p<true>, dim3(g), dim3(kBlock), 0, stream, n, r, invd, dcode, p, xf, partial, sc);
    else hipLaunchKernelGGL(k_f32_init_p<false>, dim3(g), dim3(kBlock), 0, stream, n, r, invd, dcode, p, xf, partial, sc);
    AVS_HIP(hipGetLastError());

    const bool use_graph = cur_opt().graph != 0;
    // the footprint is the float loop's (plus x, b, t64 touched once per kChunk iterations): the float loop's rule
    const int keep = A.keep_cached ? 1 : 0;
    auto enqueue_iteration = [&](int c, bool timed) -> avs_status {
        int nb = 0;
        if (timed) AVS_HIP(hipEventRecord(w->evA[c], stream));
        AVS_TRY(spmv_mixed_dispatch<true>(A, p, t, partial, sc, stream, &nb)); // t = A p ; p.t
        if (timed) AVS_HIP(hipEventRecord(w->evB[c], stream));
        const int parity = c & 1; // (the position in the chunk: the update leaves r.z where position 0 reads it)
        const bool fuse_alpha = nb <= kFuseAlphaMax;
        if (fuse_alpha) {
            if (coded) AVS_MIXED_LAUNCH_R(true, true, n, r, t, invd, dcode, sc, vpart, partial, nb, parity);
            else AVS_MIXED_LAUNCH_R(false, true, n, r, t, invd, dcode, sc, vpart, partial, nb, parity);
        } else {
            AVS_TRY(reduce_stage(w, nb, 1, parity ? OP_ALPHA_ODD : OP_ALPHA, tol, 1, stream, nullptr));
            if (coded) AVS_MIXED_LAUNCH_R(true, false, n, r, t, invd, dcode, sc, vpart, (const double *)nullptr, 0, parity);
            else AVS_MIXED_LAUNCH_R(false, false, n, r, t, invd, dcode, sc, vpart, (const double *)nullptr, 0, parity);
        }
        if (coded) AVS_MIXED_LAUNCH_XP(true, n, xf, p, r, invd, dcode, sc, vpart, g, parity);
        else AVS_MIXED_LAUNCH_XP(false, n, xf, p, r, invd, dcode, sc, vpart, g, parity);
        return AVS_OK;
    };
    // the reliable update, behind every chunk (plain launches: the fp64 product is not part of the captured chunk)
    auto enqueue_update = [&]() -> avs_status {
        hipLaunchKernelGGL(k_mixed_fold, dim3(g), dim3(kBlock), 0, stream, n, x, xf, (const PcgScalars *)sc);
        AVS_TRY(spmv_dispatch<false>(A, x, t64, nullptr, nullptr, variant, stream, nullptr));
        if (coded) hipLaunchKernelGGL((k_mixed_residual<true, false>), dim3(g), dim3(kBlock), 0, stream, n, b, (const double *)t64, r, (const float *)invd, dcode, vpart, (const PcgScalars *)sc);
        else hipLaunchKernelGGL((k_mixed_residual<false, false>), dim3(g), dim3(kBlock), 0, stream, n, b, (const double *)t64, r, (const float *)invd, dcode, vpart, (const PcgScalars *)sc);
        hipLaunchKernelGGL(k_mixed_finish<false>, dim3(1), dim3(kRedBlock), 0, stream, (const double *)vpart, g, sc, tol);
        if (coded) hipLaunchKernelGGL(k_mixed_pstep<true>, dim3(g), dim3(kBlock), 0, stream, n, p, (const float *)r, (const float *)invd, dcode, (const PcgScalars *)sc);
        else hipLaunchKernelGGL(k_mixed_pstep<false>, dim3(g), dim3(kBlock), 0, stream, n, p, (const float *)r, (const float *)invd, dcode, (const PcgScalars *)sc);
        AVS_HIP(hipGetLastError());
        w->reliable_updates++;
        return AVS_OK;
    };
    GraphKey key = matrix_key(kGraphMixed, A, xf, tol);
    key.val = A.val;
    key.coded = coded;
    key.fuse_beta = true;
    key.brick = brick;
    ChunkState cs;
    bool cancelled = false;
    for (;;) {
        AVS_TRY(poll_scalars(w, sc, stream));
        sample_spmv(w, info != nullptr, false, &cs);
        const PcgScalars &h = *w->host_sc;
        if (h.done == 0 && h.iter < cs.enqueued) cs.enqueued = h.iter; // a chunk the recurrence froze: its remaining iterations did not run
        if (h.done || cs.enqueued >= max_iters) break;
        if (cancel_consume()) { cancelled = true; break; }
        AVS_TRY(enqueue_chunk(w, stream, use_graph ? &key : nullptr, max_iters, info != nullptr, enqueue_iteration, &cs));
        AVS_TRY(enqueue_update()); // x += xf before the host looks: whatever ends the loop, x holds the last iterate
    }
    if (w->host_sc->done == 3) AVS_HIP(hipMemsetAsync(x, 0, (size_t)n * sizeof(double), stream)); // rhsNorm2 == 0 -> x.setZero()
    return finish_info(w, A, stream, info, &cs, cancelled, 0, false);
}
#undef AVS_MIXED_LAUNCH_R
#undef AVS_MIXED_LAUNCH_XP

#ifdef AVS_PROBES
// probe / test entry: y = A x through the mixed-precision loop's product (x holds float values; y is widened), + the folded partial sums
// n_cols (0: A.n): the entries of x -- [owned | halo] for the local rows of a partitioned plan
avs_status spmv_mixed_probe(const CsrView &A, const double *x, double *y, bool fused, double *dot_out, hipStream_t st, int64_t n_cols)
{
    const int64_t n = A.n;
    if (n_cols < n) n_cols = n;
    DevBuf<float> xf, yf;
    DevBuf<double> partial;
    AVS_TRY(xf.alloc((size_t)n_cols + 8));
    AVS_TRY(yf.alloc((size_t)n + 8));
    const int g = stream_grid(n) < kVecGrid ? stream_grid(n) : kVecGrid;
    hipLaunchKernelGGL(k_f32_narrow, dim3(g), dim3(kBlock), 0, st, n_cols, x, xf.p);
    if (!fused) {
        AVS_TRY(spmv_mixed_dispatch<false>(A, xf.p, yf.p, nullptr, nullptr, st, nullptr));
    } else {
        size_t np = (size_t)stream_grid(n) + 16;
        if (A.brick && A.brick->ntiles > 0 && (size_t)brick_partial_count_mixed(*A.brick) > np) np = (size_t)brick_partial_count_mixed(*A.brick);
        AVS_TRY(partial.alloc(np));
        AVS_HIP(hipMemsetAsync(partial.p, 0, np * sizeof(double), st));
        AVS_TRY(spmv_mixed_dispatch<true>(A, xf.p, yf.p, partial.p, nullptr, st, nullptr));
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
#endif // AVS_PROBES
