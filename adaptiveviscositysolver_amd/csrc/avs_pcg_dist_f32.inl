// avs_pcg_dist_f32.inl -- the float-vector iteration of partitioned AVS_PRECISION_F32 solves (AVS_OPTION_DIST_F32_VECTORS = 1; included by
// avs_pcg.hip behind avs_pcg_f32.inl, inside namespace avs).
//
// The single-GPU float loop (avs_pcg_f32.inl) iterates on float vectors with float scalars, as Eigen's float CG does.  This file gives the
// partitioned single-reduction loops (Chronopoulos-Gear, avs_pcg.hip) the same arithmetic, over both transports:
//   * x, r, p, s, w = A u, u = M^-1 r [owned | halo] and the inverse diagonal are float arrays;
//   * sums: a thread's own terms in float, everything across threads and workgroups in double, across ranks in double in rank order
//     (the finalizer of the direct transport / the all-reduce) -- every rank computes bit-identical scalars;
//   * the scalar step (OP_SR_INIT_F32, OP_SR_STEP_F32, sr_step_f32 in avs_halo.hpp) rounds the all-reduced sums to float and computes
//     alpha, beta and the threshold in float;
//   * the SpMV is the single-GPU float loop's: k_spmv_brick<..., float> on the brick form, else k_f32_spmv_csr; both read the float
//     extended vector [owned | halo];
//   * halo entries travel as doubles (widened floats: exact) -- the direct transport's comm block, 8-B slots, self-test and checksums,
//     and the RCCL / in-process exchange's buffers stay as they are.
// What stays fp64: AVS_DIST_CG=standard, paranoid mode and the CU-resident loop between ranks (this option skips it).  The direct
// transport runs each round as three launches (float halo gather, float SpMV into the stage slots, k_halo_finalize): the word-stream
// kernels' HALO instantiations -- interior tiles multiplied while the halo travels -- have no float version.

// r = b - t, u = M^-1 r ; partials [0..g) b.b, [g..2g) r.u, [2g..3g) r.r
template <bool CODED>
__global__ __launch_bounds__(kBlock) void k_sr_init_f32(int64_t n, const double *__restrict__ b, const float *__restrict__ t,
                                                        const float *__restrict__ invd, const uint16_t *__restrict__ dcode,
                                                        float *__restrict__ r, float *__restrict__ u, double *__restrict__ partial)
{
    __shared__ double red[4];
    float bb = 0.f, ru = 0.f, rr = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const float bi = (float)b[i]; // (b holds float values)
        const float ri = bi - t[i];
        const float ui = (CODED ? invd[dcode[i]] : invd[i]) * ri;
        r[i] = ri;
        u[i] = ui;
        bb += bi * bi;
        ru += ri * ui;
        rr += ri * ri;
    }
    const double sb = block_sum((double)bb, red);
    const double su = block_sum((double)ru, red);
    const double sr = block_sum((double)rr, red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = sb;
        partial[gridDim.x + blockIdx.x] = su;
        partial[2 * gridDim.x + blockIdx.x] = sr;
    }
}

// k_sr_update on float vectors (RCCL / in-process transport): the previous iteration's scalar step folded in when `step` is set (state
// `in` -> `out`, as in k_sr_update), then p = u + beta p, s = w + beta s, x += alpha p, r -= alpha s, u = M^-1 r ; partials r.u, r.r
template <bool CODED>
__global__ __launch_bounds__(kBlock) void k_sr_update_f32(int64_t n, float *__restrict__ x, float *__restrict__ r, float *__restrict__ p,
                                                          float *__restrict__ s, float *__restrict__ u, const float *__restrict__ w,
                                                          const float *__restrict__ invd, const uint16_t *__restrict__ dcode,
                                                          const PcgScalars *in, PcgScalars *out, int step, double *__restrict__ partial)
{
    int done = in->done;
    double alpha = in->alpha, beta = in->beta;
    if (step) {
        double rr = in->rr, rho = in->rho;
        int iter = in->iter;
        sr_step_f32(in, rr, rho, alpha, beta, iter, done);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            PcgScalars o = *in;
            o.rr = rr; o.rho = rho; o.alpha = alpha; o.beta = beta; o.iter = iter; o.done = done;
            *out = o;
        }
    }
    if (done) return; // (rhs == 0, done == 3: the host zeroes x)
    const float a = (float)alpha, bt = (float)beta;
    __shared__ double red[4];
    float ru = 0.f, rr = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const float pi = u[i] + bt * p[i];
        const float si = w[i] + bt * s[i];
        p[i] = pi;
        s[i] = si;
        x[i] += a * pi;
        const float ri = r[i] - a * si;
        r[i] = ri;
        const float ui = (CODED ? invd[dcode[i]] : invd[i]) * ri;
        u[i] = ui;
        ru += ri * ui;
        rr += ri * ri;
    }
    const double su = block_sum((double)ru, red);
    const double sr = block_sum((double)rr, red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = su;
        partial[gridDim.x + blockIdx.x] = sr;
    }
}

// Float vectors of the loops below (x, r, p, s, w, u [owned | halo]), zeroed recurrences, both scalar states, and the float inverse
// diagonal: the table of inverted values for a `coded` matrix (+ the rows' 2-B codes), else one entry per row -- as pcg_solve_f32 makes them.
static avs_status sr_f32_prepare(PcgWork *w, const CsrView &A, bool coded, const float **invd, hipStream_t stream)
{
    const int64_t n = A.n;
    const size_t na = (size_t)n + 8, ne = (size_t)w->n_ext + 8;
    AVS_TRY(w->f_x.alloc(na)); AVS_TRY(w->f_r.alloc(na)); AVS_TRY(w->f_p.alloc(na)); AVS_TRY(w->f_s.alloc(na)); AVS_TRY(w->f_t.alloc(na));
    AVS_TRY(w->f_u.alloc(ne));
    AVS_HIP(hipMemsetAsync(w->sc.p, 0, 2 * sizeof(PcgScalars), stream));
    AVS_HIP(hipMemsetAsync(w->f_p.p, 0, na * sizeof(float), stream));
    AVS_HIP(hipMemsetAsync(w->f_s.p, 0, na * sizeof(float), stream));
    AVS_TRY(prepare_diagonal(w, A, coded, nullptr, stream));
    if (coded) {
        if (!w->f_invtab.p) AVS_TRY(w->f_invtab.alloc((size_t)kViLdsTable + 1));
        hipLaunchKernelGGL(k_f32_invtab, dim3((A.table_size + kBlock) / kBlock), dim3(kBlock), 0, stream, A, w->f_invtab.p);
        *invd = w->f_invtab.p;
    } else {
        AVS_TRY(w->f_invd.alloc(na));
        hipLaunchKernelGGL(k_f32_inv_diag, dim3(row_grid(n)), dim3(kBlock), 0, stream, A, w->f_invd.p);
        *invd = w->f_invd.p;
    }
    AVS_HIP(hipGetLastError());
    w->float_vectors = 1;
    return AVS_OK;
}

// Host-mediated transports (RCCL, in-process virtual ranks): pcg_solve_single_reduction on float vectors.  b, x: the rank's fp64 arrays
// holding float values; x receives the solution (float values again).
static avs_status pcg_solve_sr_f32(PcgWork *w, const CsrView &A, const double *b, double *x, double tol, int max_iters, hipStream_t stream,
                                   avs_solve_info *info, PcgDist *dist)
{
    const int64_t n = A.n;
    const int g = vec_grid(n);
    const bool coded = A.codes && !A.tab_ptr && A.table_size <= kViLdsTable;
    const bool brick = A.brick && A.brick->ntiles > 0 && A.brick->pwords32;
    const size_t nb_max = brick ? (size_t)brick_partial_count(*A.brick, 4) : (size_t)stream_grid(n);
    AVS_TRY(ensure_partials(w, 4 * (size_t)kVecGrid + nb_max + 16));
    const float *invd = nullptr;
    AVS_TRY(sr_f32_prepare(w, A, coded, &invd, stream));
    const uint16_t *dcode = coded ? w->dcode.p : nullptr;
    float *xf = w->f_x.p, *r = w->f_r.p, *p = w->f_p.p, *sv = w->f_s.p, *wv = w->f_t.p, *u = w->f_u.p;
    double *pvec = w->partial.p, *pspmv = w->partial.p + 4 * (size_t)kVecGrid; // 3 * g vector-kernel partials, the SpMV's behind them
    PcgScalars *sc = w->sc.p;
    AVS_HIP(hipEventRecord(w->ev0, stream));

    // r = b - A x (x staged through u for the exchange), u = M^-1 r, w = A u, the sums |b|^2, r.u, |r|^2, w.u -> OP_SR_INIT_F32
    hipLaunchKernelGGL(k_f32_narrow, dim3(g), dim3(kBlock), 0, stream, n, (const double *)x, xf);
    hipLaunchKernelGGL(k_f32_narrow, dim3(g), dim3(kBlock), 0, stream, n, (const double *)x, u);
    AVS_TRY(dist_halo_exchange_f32(dist, u, stream));
    AVS_TRY(spmv_f32_dispatch<false>(A, u, wv, nullptr, nullptr, stream, nullptr));
    if (coded) hipLaunchKernelGGL(k_sr_init_f32<true>, dim3(g), dim3(kBlock), 0, stream, n, b, (const float *)wv, invd, dcode, r, u, pvec);
    else hipLaunchKernelGGL(k_sr_init_f32<false>, dim3(g), dim3(kBlock), 0, stream, n, b, (const float *)wv, invd, dcode, r, u, pvec);
    AVS_TRY(dist_halo_exchange_f32(dist, u, stream));
    int nb0 = 0;
    AVS_TRY(spmv_f32_dispatch<true>(A, u, wv, pspmv, nullptr, stream, &nb0));
    reduce_launch(w, pvec, g, 3, sc, (int)OP_NONE, tol, 0, 0, stream);
    reduce_launch(w, pspmv, nb0, 1, sc, (int)OP_NONE, tol, 0, 3, stream);
    AVS_TRY(dist_allreduce(dist, sc->red, 4, stream));
    hipLaunchKernelGGL(k_scalar, dim3(1), dim3(64), 0, stream, sc, (int)OP_SR_INIT_F32, tol);
    AVS_HIP(hipGetLastError());

    int cur = 0; // two scalar states, ping-pong, as in pcg_solve_single_reduction
    auto enqueue_iteration = [&](int c, bool timed) -> avs_status {
        const int step = c > 0 ? 1 : 0;
        if (coded)
            hipLaunchKernelGGL(k_sr_update_f32<true>, dim3(g), dim3(kBlock), 0, stream, n, xf, r, p, sv, u, (const float *)wv, invd, dcode,
                               (const PcgScalars *)(sc + cur), sc + (step ? (cur ^ 1) : cur), step, pvec);
        else
            hipLaunchKernelGGL(k_sr_update_f32<false>, dim3(g), dim3(kBlock), 0, stream, n, xf, r, p, sv, u, (const float *)wv, invd, dcode,
                               (const PcgScalars *)(sc + cur), sc + (step ? (cur ^ 1) : cur), step, pvec);
        if (step) cur ^= 1;
        int nb = 0;
        AVS_TRY(dist_halo_exchange_f32(dist, u, stream));
        if (timed) AVS_HIP(hipEventRecord(w->evA[c], stream));
        AVS_TRY(spmv_f32_dispatch<true>(A, u, wv, pspmv, sc + cur, stream, &nb));
        if (timed) AVS_HIP(hipEventRecord(w->evB[c], stream));
        if (nb < 16384) hipLaunchKernelGGL(k_reduce_pair, dim3(1), dim3(kRedBlock), 0, stream, pvec, g, 2, pspmv, nb, 1, sc + cur);
        else {
            reduce_launch(w, pvec, g, 2, sc + cur, (int)OP_NONE, tol, 0, 0, stream);
            reduce_launch(w, pspmv, nb, 1, sc + cur, (int)OP_NONE, tol, 0, 2, stream);
        }
        return dist_allreduce(dist, sc[cur].red, 3, stream);
    };
    ChunkState cs;
    bool cancelled = false;
    AVS_TRY(w->cancel_word.alloc(2));
    for (;;) {
        // avs_cancel: the all-reduced requests of every rank decide at the chunk boundary (as pcg_solve_single_reduction)
        double stop_h[2] = {cancel_requested() ? 1. : 0., 0.};
        AVS_HIP(hipMemcpyAsync(w->cancel_word.p, stop_h, sizeof(double), hipMemcpyHostToDevice, stream));
        AVS_TRY(dist_allreduce(dist, w->cancel_word.p, 1, stream));
        AVS_HIP(hipMemcpyAsync(stop_h + 1, w->cancel_word.p, sizeof(double), hipMemcpyDeviceToHost, stream));
        AVS_TRY(poll_scalars(w, sc + cur, stream));
        sample_spmv(w, info != nullptr, true, &cs);
        if (w->host_sc->done || cs.enqueued >= max_iters) break;
        if (stop_h[1] != 0.) { (void)cancel_consume(); cancelled = true; break; }
        AVS_TRY(enqueue_chunk(w, stream, nullptr, max_iters, info != nullptr, enqueue_iteration, &cs)); // (no graph: RCCL calls inside)
        hipLaunchKernelGGL(k_scalar, dim3(1), dim3(64), 0, stream, sc + cur, (int)OP_SR_STEP_F32, tol);
        AVS_HIP(hipGetLastError());
    }
    if (w->host_sc->done == 3) AVS_HIP(hipMemsetAsync(xf, 0, (size_t)n * sizeof(float), stream)); // rhs == 0: x := 0
    hipLaunchKernelGGL(k_f32_widen, dim3(g), dim3(kBlock), 0, stream, n, (const float *)xf, x);
    AVS_HIP(hipGetLastError());
    return finish_info(w, A, stream, info, &cs, cancelled, 0, true);
}

// Direct transport: pcg_solve_direct on float vectors.  A round = the float halo gather (waits for the peers' flags, narrows their entries
// into the vector's tail), the float SpMV writing its x.Ax partials into the stage slots, k_halo_finalize -- three launches for either
// storage form.  No CU-resident loop.
static avs_status pcg_solve_direct_f32(PcgWork *w, const CsrView &A, const double *b, double *x, double tol, int max_iters,
                                       hipStream_t stream, avs_solve_info *info, const DirectArgs &da)
{
    const int64_t n = A.n;
    int g = 1, chunk_rows = kBlock; // every vector kernel of this loop uses the fused kernel's geometry (same partial layout)
    sr_update_geometry((long long)n, &g, &chunk_rows);
    AVS_REQUIRE(g == da.push_grid && chunk_rows == da.push_chunk, AVS_EINTERNAL, "push segments were built for another geometry");
    const bool coded = A.codes && !A.tab_ptr && A.table_size <= kViLdsTable;
    const bool brick = A.brick && A.brick->ntiles > 0 && A.brick->pwords32;
    const float *invd = nullptr;
    AVS_TRY(sr_f32_prepare(w, A, coded, &invd, stream));
    const uint16_t *dcode = coded ? w->dcode.p : nullptr;
    float *xf = w->f_x.p, *r = w->f_r.p, *p = w->f_p.p, *sv = w->f_s.p, *wv = w->f_t.p, *u = w->f_u.p;
    double *pvec = w->partial.p; // up to 3 * g vector-kernel partials
    double *wide = w->t.p;       // the set-up rounds' k_push reads doubles: u widened (the fp64 loops' w, unused here)
    PcgScalars *sc = w->sc.p;
    // the SpMV's partials: one per persistent workgroup of the float brick kernel, else one per 256-row block of k_f32_spmv_csr
    const int slots = n <= 0 ? 0 : (brick ? brick_partial_count(*A.brick, 4) : stream_grid(n));
    const int nfin = slots > 0 ? (slots + kFinShare - 1) / kFinShare : 1;
    AVS_TRY(w->stage2.alloc((size_t)(slots > 0 ? slots : 1) + (size_t)nfin));
    AVS_HIP(hipMemsetAsync(w->stage2.p, 0xFF, (size_t)(slots > 0 ? slots : 1) * sizeof(double), stream)); // arm: kSentinel in every slot
    const int push_blocks = da.n_send > 0 ? (da.n_send + 255) / 256 : 0;
    const int n_halo_cols = (int)(w->n_ext - n);
    AVS_TRY(w->cancel_dev.alloc(1));
    AVS_HIP(hipMemsetAsync(w->cancel_dev.p, 0, sizeof(int), stream));
    AVS_HIP(hipEventRecord(w->ev0, stream));

    auto round = [&](float *vec, int nred_vec, int op, hipEvent_t ea, hipEvent_t eb, bool push) -> avs_status {
        if (push && push_blocks) {
            hipLaunchKernelGGL(k_f32_widen, dim3(g), dim3(kBlock), 0, stream, n, (const float *)vec, wide);
            hipLaunchKernelGGL(k_push, dim3(push_blocks), dim3(256), 0, stream, da.dd, (const double *)wide, (const unsigned long long *)da.epoch,
                               da.push_ticket, (const PcgScalars *)sc);
        }
        if (ea) AVS_HIP(hipEventRecord(ea, stream));
        HaloView hv;
        hv.dd = da.dd;
        hv.epoch = da.epoch;
        hv.epoch_w = da.epoch;
        hv.fin_ticket = da.fin_ticket;
        hv.sc = sc;
        hv.pvec = pvec;
        hv.stage = w->stage2.p;
        hv.stage2 = w->stage2.p + (slots > 0 ? slots : 1);
        hv.tile_bnd = da.tile_flags;
        hv.ntiles = slots;
        hv.ppt = 1;
        hv.nfin = nfin;
        hv.g = g;
        hv.nred_vec = nred_vec;
        hv.op = op;
        hv.tol = tol;
        hv.cancel = w->cancel_dev.p;
        if (da.npeers > 0) {
            const int hg = n_halo_cols > 0 ? (n_halo_cols + 255) / 256 : 1;
            hipLaunchKernelGGL(k_halo_gather<float>, dim3(hg < 64 ? hg : 64), dim3(256), 0, stream, hv, vec);
        }
        AVS_TRY(spmv_f32_dispatch<true>(A, vec, wv, w->stage2.p, sc, stream, nullptr));
        hipLaunchKernelGGL(k_halo_finalize, dim3(nfin), dim3(512), 0, stream, hv);
        if (eb) AVS_HIP(hipEventRecord(eb, stream));
        AVS_HIP(hipGetLastError());
        return AVS_OK;
    };
    // r = b - A x (x staged through u for the exchange), u = M^-1 r, w = A u
    hipLaunchKernelGGL(k_f32_narrow, dim3(g), dim3(kBlock), 0, stream, n, (const double *)x, xf);
    hipLaunchKernelGGL(k_f32_narrow, dim3(g), dim3(kBlock), 0, stream, n, (const double *)x, u);
    AVS_TRY(round(u, 0, (int)OP_NONE, nullptr, nullptr, true));
    if (coded) hipLaunchKernelGGL(k_sr_init_f32<true>, dim3(g), dim3(kBlock), 0, stream, n, b, (const float *)wv, invd, dcode, r, u, pvec);
    else hipLaunchKernelGGL(k_sr_init_f32<false>, dim3(g), dim3(kBlock), 0, stream, n, b, (const float *)wv, invd, dcode, r, u, pvec);
    AVS_TRY(round(u, 3, (int)OP_SR_INIT_F32, nullptr, nullptr, true));
    AVS_HIP(hipGetLastError());
    w->resident_used = 0;

    auto enqueue_iteration = [&](int c, bool timed) -> avs_status {
        // update and push in one launch (the float instantiations of the fp64 loop's kernel)
        if (coded && brick)
            hipLaunchKernelGGL((k_sr_update_push<true, false, float>), dim3(g), dim3(kBlock), 0, stream, n, xf, r, p, sv, u, (const float *)wv, invd,
                               dcode, (const PcgScalars *)sc, pvec, da.dd, (const unsigned long long *)da.epoch, da.push_ticket);
        else if (coded)
            hipLaunchKernelGGL((k_sr_update_push<true, true, float>), dim3(g), dim3(kBlock), 0, stream, n, xf, r, p, sv, u, (const float *)wv, invd,
                               dcode, (const PcgScalars *)sc, pvec, da.dd, (const unsigned long long *)da.epoch, da.push_ticket);
        else
            hipLaunchKernelGGL((k_sr_update_push<false, true, float>), dim3(g), dim3(kBlock), 0, stream, n, xf, r, p, sv, u, (const float *)wv, invd,
                               (const uint16_t *)nullptr, (const PcgScalars *)sc, pvec, da.dd, (const unsigned long long *)da.epoch, da.push_ticket);
        return round(u, 2, (int)OP_SR_STEP_F32, timed ? w->evA[c] : nullptr, timed ? w->evB[c] : nullptr, false);
    };
    GraphKey key = matrix_key(kGraphDirectF32, A, xf, tol);
    key.b = b;
    key.dd = da.dd;
    key.ntiles = slots;
    key.brick = brick;
    key.coded = coded;
    const GraphKey *gkey = cur_opt().graph != 0 ? &key : nullptr;
    ChunkState cs;
    bool cancel_sent = false;
    for (;;) {
        AVS_TRY(poll_scalars(w, sc, stream));
        if (w->host_sc->fault) {
            if (w->host_sc->fault == 4)
                set_error("direct transport (paranoid mode): a halo segment does not add up to the checksum its sender left ahead of the flag "
                          "-- stale or torn halo entries (iteration ~%d)", w->host_sc->iter);
            else
                set_error("direct transport: %s did not arrive within the time limit (rank stalled or dead?)",
                          w->host_sc->fault == 1 ? "a peer's halo entries" : (w->host_sc->fault == 2 ? "a peer's partial sums" : "a workgroup's partial sums"));
            return AVS_ERCCL;
        }
        sample_spmv(w, info != nullptr, true, &cs);
        if (w->host_sc->done || cs.enqueued >= max_iters) break;
        if (cancel_requested() && !cancel_sent) { // the request word the finalizer adds to the round's sums: every rank stops in the same round
            static const int one = 1;
            AVS_HIP(hipMemcpyAsync(w->cancel_dev.p, &one, sizeof(int), hipMemcpyHostToDevice, stream));
            cancel_sent = true;
        }
        AVS_TRY(enqueue_chunk(w, stream, gkey, max_iters, info != nullptr, enqueue_iteration, &cs));
    }
    if (w->host_sc->done == 3) AVS_HIP(hipMemsetAsync(xf, 0, (size_t)n * sizeof(float), stream)); // rhs == 0: x := 0
    hipLaunchKernelGGL(k_f32_widen, dim3(g), dim3(kBlock), 0, stream, n, (const float *)xf, x);
    AVS_HIP(hipGetLastError());
    AVS_TRY(finish_info(w, A, stream, info, &cs, w->host_sc->cancelled != 0, 0, true));
    if (w->host_sc->cancelled) (void)cancel_consume();
    return AVS_OK;
}
