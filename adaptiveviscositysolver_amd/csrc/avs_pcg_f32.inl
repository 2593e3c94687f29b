// avs_pcg_f32.inl -- kernels, SpMV dispatcher and diagonal set-up of the float-vector PCG loops of AVS_PRECISION_F32 contexts (included by
// avs_pcg.hip, inside namespace avs).  The host loop is pcg_solve_phases<float> (avs_pcg.hip), shared with the fp64 and mixed solves.
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

typedef float f4_t __attribute__((ext_vector_type(4)));
typedef unsigned u2_t __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(kBlock) void k_f32_narrow(int64_t n, const double *__restrict__ src, float *__restrict__ dst)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) dst[i] = (float)src[i];
}
__global__ __launch_bounds__(kBlock) void k_f32_widen(int64_t n, const float *__restrict__ src, double *__restrict__ dst)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) dst[i] = (double)src[i];
}

// DiagonalPreconditioner<float>::factorize: invdiag(j) = A(j,j) != 0 ? 1.f / A(j,j) : 1.f
__global__ __launch_bounds__(kBlock) void k_f32_inv_diag(CsrView A, float *__restrict__ invd)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= A.n) return;
    float d = 0.f;
    for (int k = A.row_ptr[i]; k < A.row_ptr[i + 1]; ++k)
        if (A.col[k] == (int32_t)i) d = (float)(A.val ? A.val[k] : A.table[(A.tab_ptr ? A.tab_ptr[i / kTileRows] : 0) + A.codes[k]]);
    invd[i] = (d != 0.f && !A.no_precond) ? 1.f / d : 1.f;
}
// one small dictionary: invd[i] == invtab[dcode[i]] (dcode: k_inv_diag_coded), the table inverted in float
__global__ __launch_bounds__(kBlock) void k_f32_invtab(CsrView A, float *__restrict__ invtab)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i > A.table_size) return;
    const float d = i < A.table_size ? (float)A.table[i] : 0.f;
    invtab[i] = (d != 0.f && !A.no_precond) ? 1.f / d : 1.f;
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

// r = b - t ; partials: [0..g) b.b, [g..2g) r.r
__global__ __launch_bounds__(kBlock) void k_f32_init_residual(int64_t n, const float *__restrict__ b, const float *__restrict__ t,
                                                              float *__restrict__ r, double *__restrict__ partial)
{
    __shared__ double red[4];
    float bb = 0.f, rr = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const float bi = b[i];
        const float ri = bi - t[i];
        r[i] = ri;
        bb += bi * bi;
        rr += ri * ri;
    }
    const double sb = block_sum((double)bb, red);
    const double sr = block_sum((double)rr, red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = sb;
        partial[gridDim.x + blockIdx.x] = sr;
    }
}

// p = invd * r ; partial r.p
template <bool CODED>
__global__ __launch_bounds__(kBlock) void k_f32_init_p(int64_t n, const float *__restrict__ r, const float *__restrict__ invd,
                                                       const uint16_t *__restrict__ dcode, float *__restrict__ p, float *__restrict__ x,
                                                       double *__restrict__ partial, const PcgScalars *sc)
{
    __shared__ double red[4];
    const int done = sc->done;
    float rz = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        if (done == 3) { x[i] = 0.f; continue; } // rhsNorm2 == 0 -> x.setZero()
        if (done) continue;
        const float ri = r[i];
        const float zi = (CODED ? invd[dcode[i]] : invd[i]) * ri;
        p[i] = zi;
        rz += ri * zi;
    }
    const double s = block_sum((double)rz, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// r -= alpha t ; partials r.r and r.(invd r).  Four rows per thread (16-B accesses).  FUSED: every workgroup folds the SpMV's `nb`
// partial sums itself (the alpha step, as in k_update_r); else OP_ALPHA has left p.Ap in sc->pAp.  Either way alpha is the FLOAT
// quotient of the float-rounded sums.  DS (the mixed-precision loop, avs_pcg_mixed.inl): the scalars are doubles -- alpha is the double
// quotient of the unrounded sums, rounded to float only where it multiplies the float vector.
template <bool CODED, bool FUSED, bool KEEP, bool DS = false>
__global__ __launch_bounds__(kBlock) void k_f32_update_r(int64_t n, float *__restrict__ r, const float *__restrict__ t,
                                                         const float *__restrict__ invd, const uint16_t *__restrict__ dcode, PcgScalars *sc,
                                                         double *__restrict__ partial, const double *__restrict__ spmv_partial, int nb, int parity)
{
    __shared__ double pro[8], red[8];
    // (the partial sums and the loads of the first kVecAhead trips are requested before anything is waited for: vec_request, avs_pcg.hip)
    const int64_t n4 = n >> 2;
    const int64_t j0 = (int64_t)blockIdx.x * kBlock + threadIdx.x, stride = (int64_t)gridDim.x * kBlock;
    struct Trip { f4_t rv, tv, iv; u2_t cc; };
    auto request = [&](int64_t j, bool live, Trip &q) {
        const int64_t i = 4 * j;
        q.rv = *vec_src<f4_t>(live, r + i, sc);
        q.tv = stream_load_k<KEEP>(vec_src<f4_t>(live, t + i, sc));
        if (CODED) q.cc = stream_load_k<KEEP>(vec_src<u2_t>(live, dcode + i, sc));
        else q.iv = *vec_src<f4_t>(live, invd + i, sc);
    };
    VecScalars s = vec_request<FUSED ? 1 : 0>(sc, parity, spmv_partial, nb, 0);
    Trip ahead[kVecAhead];
#pragma unroll
    for (int u = 0; u < kVecAhead; ++u) request(j0 + u * stride, j0 + u * stride < n4, ahead[u]);
    vec_fold<FUSED ? 1 : 0>(s, spmv_partial, nb, 0, pro);
    if (s.done) {
        if (FUSED && blockIdx.x == 0 && threadIdx.x == 0 && s.done == 2) sc->done = 1; // the pending x update has run (OP_ALPHA)
        return;
    }
    float alpha;
    if (FUSED) {
        const double pap = s.sum[0];
        const double alpha_d = s.rho_old / pap;
        alpha = DS ? (float)alpha_d : (float)s.rho_old / (float)pap;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            sc->red[0] = pap;
            sc->pAp = DS ? pap : (double)(float)pap;
            sc->alpha = DS ? alpha_d : (double)alpha;
        }
    } else if (DS) {
        alpha = (float)s.alpha; // (OP_ALPHA's double quotient)
    } else {
        alpha = (float)s.rho_old / (float)s.pAp;
        if (blockIdx.x == 0 && threadIdx.x == 0) sc->alpha = (double)alpha; // (OP_ALPHA divided in double: k_f32_update_xp reads this one)
    }
    float rr = 0.f, rz = 0.f;
    auto row_quad = [&](int64_t j, const Trip &q) {
        const int64_t i = 4 * j;
        const f4_t rv = q.rv, tv = q.tv;
        f4_t iv = q.iv;
        if (CODED) {
            iv.x = invd[q.cc.x & 0xffffu]; iv.y = invd[q.cc.x >> 16]; iv.z = invd[q.cc.y & 0xffffu]; iv.w = invd[q.cc.y >> 16];
        }
        f4_t rn;
        rn.x = rv.x - alpha * tv.x; rn.y = rv.y - alpha * tv.y; rn.z = rv.z - alpha * tv.z; rn.w = rv.w - alpha * tv.w;
        *reinterpret_cast<f4_t *>(r + i) = rn;
        rr += rn.x * rn.x; rz += rn.x * (iv.x * rn.x);
        rr += rn.y * rn.y; rz += rn.y * (iv.y * rn.y);
        rr += rn.z * rn.z; rz += rn.z * (iv.z * rn.z);
        rr += rn.w * rn.w; rz += rn.w * (iv.w * rn.w);
    };
#pragma unroll
    for (int u = 0; u < kVecAhead; ++u)
        if (j0 + u * stride < n4) row_quad(j0 + u * stride, ahead[u]);
    for (int64_t j = j0 + kVecAhead * stride; j < n4; j += stride) {
        Trip q;
        request(j, true, q);
        row_quad(j, q);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = n4 * 4; i < n; ++i) {
            const float ri = r[i] - alpha * t[i];
            r[i] = ri;
            rr += ri * ri;
            rz += ri * ((CODED ? invd[dcode[i]] : invd[i]) * ri);
        }
    double srr = (double)rr, srz = (double)rz;
    block_sum2(srr, srz, red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = srr;
        partial[gridDim.x + blockIdx.x] = srz;
    }
}

// x += alpha p (also in the iteration that converges: done == 2), then p = invd r + beta p.  The beta step -- fold of k_f32_update_r's
// 2 g partials, convergence test, beta = absNew / absOld in float -- is done here by every workgroup for itself (as k_update_xp<FUSED>).
// DS (the mixed-precision loop): sums, threshold test and beta in double; the iteration that claims convergence leaves the r.z it started
// from in sc->rho whatever its parity (the reliable update that follows reads it there).
template <bool CODED, bool KEEP, bool DS = false>
__global__ __launch_bounds__(kBlock) void k_f32_update_xp(int64_t n, float *__restrict__ x, float *__restrict__ p, const float *__restrict__ r,
                                                          const float *__restrict__ invd, const uint16_t *__restrict__ dcode, PcgScalars *sc,
                                                          const double *__restrict__ partial, int g, int parity)
{
    __shared__ double pro[8];
    const int64_t n4 = n >> 2;
    const int64_t j0 = (int64_t)blockIdx.x * kBlock + threadIdx.x, stride = (int64_t)gridDim.x * kBlock;
    struct Trip { f4_t pv, xv, rv, iv; u2_t cc; };
    auto request = [&](int64_t j, bool live, Trip &q) {
        const int64_t i = 4 * j;
        q.pv = *vec_src<f4_t>(live, p + i, sc);
        q.xv = stream_load_k<KEEP>(vec_src<f4_t>(live, x + i, sc));
        q.rv = stream_load_k<KEEP>(vec_src<f4_t>(live, r + i, sc));
        if (CODED) q.cc = stream_load_k<KEEP>(vec_src<u2_t>(live, dcode + i, sc));
        else q.iv = *vec_src<f4_t>(live, invd + i, sc);
    };
    VecScalars s = vec_request<2>(sc, parity, partial, g, g);
    Trip ahead[kVecAhead];
#pragma unroll
    for (int u = 0; u < kVecAhead; ++u) request(j0 + u * stride, j0 + u * stride < n4, ahead[u]);
    vec_fold<2>(s, partial, g, g, pro);
    int done = s.done;
    if (done == 1 || done == 3) return;
    const float alpha = (float)s.alpha;
    float beta = 0.f;
    if (done == 0) {
        if (DS) {
            const double rrd = s.sum[0], rzd = s.sum[1];
            const double absOld = s.rho_old;
            if (rrd < s.threshold) done = 2;
            else beta = (float)(rzd / absOld);
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                sc->red[0] = rrd;
                sc->red[1] = rzd;
                sc->rr = rrd;
                if (done == 2) {
                    sc->done = 2;
                    if (parity) sc->rho = absOld; // (nobody reads sc->rho in an odd iteration: the slot this iteration would have written)
                } else {
                    if (parity) sc->rho = rzd;
                    else sc->rho_alt = rzd;
                    sc->beta = rzd / absOld;
                    sc->iter += 1;
                }
            }
        } else {
            const float rrf = (float)s.sum[0], rzf = (float)s.sum[1];
            const float absOld = (float)s.rho_old;
            if (rrf < (float)s.threshold) done = 2; // Eigen: break before i++ (x += alpha p still pending)
            else beta = rzf / absOld;
            if (blockIdx.x == 0 && threadIdx.x == 0) { // what OP_BETA does
                sc->red[0] = (double)rrf;
                sc->red[1] = (double)rzf;
                sc->rr = (double)rrf;
                if (done == 2) sc->done = 2;
                else {
                    if (parity) sc->rho = (double)rzf;
                    else sc->rho_alt = (double)rzf;
                    sc->beta = (double)beta;
                    sc->iter += 1;
                }
            }
        }
    }
    if (done == 2) { // (the loads that went ahead are dropped)
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) x[i] += alpha * p[i];
        return;
    }
    auto row_quad = [&](int64_t j, const Trip &q) {
        const int64_t i = 4 * j;
        const f4_t pv = q.pv, xv = q.xv, rv = q.rv;
        f4_t iv = q.iv;
        if (CODED) {
            iv.x = invd[q.cc.x & 0xffffu]; iv.y = invd[q.cc.x >> 16]; iv.z = invd[q.cc.y & 0xffffu]; iv.w = invd[q.cc.y >> 16];
        }
        f4_t xn, pn;
        xn.x = xv.x + alpha * pv.x; xn.y = xv.y + alpha * pv.y; xn.z = xv.z + alpha * pv.z; xn.w = xv.w + alpha * pv.w;
        pn.x = iv.x * rv.x + beta * pv.x; pn.y = iv.y * rv.y + beta * pv.y; pn.z = iv.z * rv.z + beta * pv.z; pn.w = iv.w * rv.w + beta * pv.w;
        stream_store_k<KEEP>(xn, reinterpret_cast<f4_t *>(x + i));
        *reinterpret_cast<f4_t *>(p + i) = pn;
    };
#pragma unroll
    for (int u = 0; u < kVecAhead; ++u)
        if (j0 + u * stride < n4) row_quad(j0 + u * stride, ahead[u]);
    for (int64_t j = j0 + kVecAhead * stride; j < n4; j += stride) {
        Trip q;
        request(j, true, q);
        row_quad(j, q);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = n4 * 4; i < n; ++i) {
            const float pi = p[i];
            x[i] += alpha * pi;
            p[i] = (CODED ? invd[dcode[i]] : invd[i]) * r[i] + beta * pi;
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

// The float loops' diagonal (coded: diag_coded(A)): the rows' codes and the table inverted in float, else one float inverse per row.
// *inv: what the vector kernels index -- by dcode[i] (coded) or by i.
static avs_status prepare_diagonal_f32(PcgWork *w, const CsrView &A, bool coded, float **inv, const uint16_t **dcode, hipStream_t stream)
{
    AVS_TRY(prepare_diagonal(w, A, coded, nullptr, stream));
    if (coded) {
        AVS_TRY(w->f_invtab.alloc((size_t)kViLdsTable + 1));
        hipLaunchKernelGGL(k_f32_invtab, dim3((A.table_size + kBlock) / kBlock), dim3(kBlock), 0, stream, A, w->f_invtab.p);
    } else {
        AVS_TRY(w->f_invd.alloc((size_t)A.n + 8));
        hipLaunchKernelGGL(k_f32_inv_diag, dim3(row_grid(A.n)), dim3(kBlock), 0, stream, A, w->f_invd.p);
    }
    *inv = coded ? w->f_invtab.p : w->f_invd.p;
    *dcode = coded ? w->dcode.p : nullptr;
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
