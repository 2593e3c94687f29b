// avs_pcg.hip -- device-resident Jacobi-PCG for gfx950 (MI355X): the loops and their vector, reduction and transport kernels.
// (The matrix-vector products on the caller's CSR: avs_spmv.hip; the brick-structured form: avs_brick.hip.)
//
// Replaces cpp:611-643 of the reference (HDK_AdaptiveViscosity.cpp): Eigen's
// ConjugateGradient<SparseMatrix<double>, Lower|Upper> with DiagonalPreconditioner and
// solveWithGuess.  The iteration follows Eigen 3.3/3.4 ConjugateGradient.h operation by operation
// (SURVEY.md 8(c)); only the order of additions inside dot products differs (block-wise tree).
//
// Roofline: every kernel here is HBM-bound.
//
// CG scalars never leave the device.  The host enqueues iterations in chunks and polls a
// `done` flag once per chunk; kernels of iterations enqueued past convergence exit immediately, so
// the iteration count and the solution are exactly those of the sequential algorithm.
#include "avs_internal.hpp"
#include "avs_halo.hpp"
#include "avs_resident_plan.hpp"
#include "avs_wave.hpp"

namespace avs {

static constexpr int kChunk = 32;            // iterations enqueued between host polls
static constexpr int kTimedChunkEvery = 8; // hipGraph replay: 1 chunk in 8 is enqueued launch by launch with timing events
static constexpr int kFuseAlphaMax = 4096;   // single-GPU loop: SpMV partial sums that k_update_r's workgroups fold themselves (<= 262 k rows;
                                             // 5.9 k partials at 380 k rows: 27.1 -> 25.4 k it/s, so not beyond)
static constexpr int kSampleEvery = 4;       // SpMV launches bracketed by HIP events: every 4th (events are not free)

// What a captured chunk (PcgWork::graph) was recorded against: the loop, the buffers and sizes its launches read, its flags and the
// tolerance.  It is replayed only while every field matches.  Each loop sets what it depends on and leaves the rest zero; the loop tag
// keeps one loop from ever replaying another's graph on the same workspace.
enum GraphLoop { kGraphF64 = 1, kGraphF32, kGraphDirect, kGraphDirectF32, kGraphMixed, kGraphDirectMixed };
struct GraphKey {
    int loop = 0;
    const void *row_ptr = nullptr, *col = nullptr, *val = nullptr, *codes = nullptr, *packed = nullptr, *table = nullptr;
    const void *x = nullptr, *b = nullptr, *dd = nullptr;
    int64_t n = 0, table_size = 0, col_bits = 0, ntiles = 0;
    uint64_t epoch = 0;
    bool coded = false, fuse_beta = false, fuse_vec = false, brick = false;
    double tol = 0.;
};
static bool operator==(const GraphKey &a, const GraphKey &b)
{
    return a.loop == b.loop && a.row_ptr == b.row_ptr && a.col == b.col && a.val == b.val && a.codes == b.codes && a.packed == b.packed &&
           a.table == b.table && a.x == b.x && a.b == b.b && a.dd == b.dd && a.n == b.n && a.table_size == b.table_size &&
           a.col_bits == b.col_bits && a.ntiles == b.ntiles && a.epoch == b.epoch && a.coded == b.coded && a.fuse_beta == b.fuse_beta &&
           a.fuse_vec == b.fuse_vec && a.brick == b.brick && a.tol == b.tol;
}

struct PcgWork {
    int64_t n = 0, n_ext = 0;
    DevBuf<double> r, p, t, invd, partial;
    DevBuf<uint16_t> dcode;  // value-indexed matrix: code of every row's diagonal entry ...
    DevBuf<double> invtab;   // ... into the table of inverted values (2 B instead of 8 B per row and vector pass)
    DevBuf<float> f_x, f_r, f_p, f_t, f_b, f_invd, f_invtab; // float-vector loop of AVS_PRECISION_F32 contexts (avs_pcg_f32.inl)
    DevBuf<float> f_s, f_u;  // ... and s, u [owned | halo] of the partitioned single-reduction loops on float vectors
    int float_vectors = 0;   // the last solve iterated on float vectors
    int reliable_updates = 0; // ... and its fp64 residual updates (the mixed-precision loop, avs_pcg_mixed.inl)
    DevBuf<double> x_save;   // the initial guess while the CU-resident loop runs (restored if it faults)
    DevBuf<double> cancel_word; // partitioned solves: [0] this rank's avs_cancel request as the kernels / the all-reduce see it (0. / 1.)
    DevBuf<int> cancel_dev;     // ... and as an int for the finalizer of the direct transport
    int resident_faults = 0; // CU-resident launches of this workspace that ended in a timed-out wait
    DevBuf<unsigned long long> fused_bar; // k_update_fused: the grid barrier's ticket counter (monotonic)
    bool fused_off = false;  // ... a launch of it timed out at its barrier on this workspace: the two-launch form from then on
    int fused_faults = 0, fused_used = 0;
    float fused_void_ms = 0.f; // a solve whose fused launch timed out: the time of the voided attempt (added to the redo's solve_ms)
    DevBuf<double> s, u; // single-reduction variant (multi-GPU): s = A p recurrence, u = M^-1 r with halo tail
    DevBuf<PcgScalars> sc;
    DevBuf<double> stage2;         // direct transport: per-workgroup SpMV sums of the halo-touching launch
    DevBuf<double> stage;          // multi-block reduction: kRedBlocks x 4 block sums ...
    DevBuf<unsigned> ticket;       // ... and the arrival counter (reset by the last block)
    PcgScalars *host_sc = nullptr; // pinned
    // one chunk of kChunk iterations captured as a hipGraph (enqueue_chunk: the f64, f32 and direct loops): relaunched while the key matches
    hipGraphExec_t graph = nullptr;
    GraphKey graph_key;
    bool graph_broken = false; // a capture failed: plain launches for the rest of this workspace's life
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t evA[kChunk] = {}, evB[kChunk] = {}; // per-launch SpMV timing inside the solve
    size_t npartial = 0;
    struct ResidentPlan *resident = nullptr; // CU-resident loop (avs_pcg_resident.inl): lane plan of the current matrix
    int resident_used = 0;                   // the last solve ran it
};

#ifdef AVS_PROBES
// include/avs_probe.h, avs_phase_loop_info: what the launch-per-phase loop did in this thread's last solve (pcg_solve_phases resets it,
// enqueue_chunk and the loop's enqueue_iteration count).  Probe build only: the product library keeps no such record.
static thread_local avs_phase_loop_report tl_phase_report = {};
static thread_local bool tl_phase_capturing = false; // enqueue_iteration is recording a graph: nothing is enqueued
static thread_local bool tl_phase_folded = false;    // the last enqueue_iteration folded its alpha step into update_r
#endif

// ---------------------------------------------------------------------------------------------
// vector kernels
// ---------------------------------------------------------------------------------------------
// T: the type of the vectors (double; float in the float and mixed-precision loops -- there the diagonal is narrowed, then inverted in float)
// DiagonalPreconditioner<T>::factorize: invdiag(j) = A(j,j) != 0 ? 1/A(j,j) : 1
template <typename T> __device__ __forceinline__ T inv_or_one(const CsrView &A, T d)
{
    return (d != T(0) && !A.no_precond) ? T(1) / d : T(1); // (no_precond: plain CG, z = r)
}
// entry i of the inverted dictionary of a value-indexed matrix; the extra entry, i == table_size, is 1 and stands for "no diagonal entry"
template <typename T, typename I> __device__ __forceinline__ T inv_table_entry(const CsrView &A, I i)
{
    return inv_or_one<T>(A, i < A.table_size ? (T)A.table[i] : T(0));
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_inv_diag(CsrView A, T *__restrict__ invd)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= A.n) return;
    T d = 0;
    for (int k = A.row_ptr[i]; k < A.row_ptr[i + 1]; ++k)
        if (A.col[k] == (int32_t)i) d = (T)(A.val ? A.val[k] : A.table[(A.tab_ptr ? A.tab_ptr[i / kTileRows] : 0) + A.codes[k]]);
    invd[i] = inv_or_one<T>(A, d);
}

// r = b - t ; partials: [0..g) b.b, [g..2g) r.r (a thread's own terms are added in T, everything across threads in double)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_init_residual(int64_t n, const T *__restrict__ b, const T *__restrict__ t, T *__restrict__ r,
                                                          double *__restrict__ partial)
{
    __shared__ double red[4];
    T bb = 0, rr = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const T bi = b[i];
        const T ri = bi - t[i];
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

// p = invd * r ; partial r.p.  CODED: invd is the inverted dictionary, indexed by the rows' codes (the fp64 loop reads the per-row inverse)
template <typename T, bool CODED>
__global__ __launch_bounds__(kBlock) void k_init_p(int64_t n, const T *__restrict__ r, const T *__restrict__ invd,
                                                   const uint16_t *__restrict__ dcode, T *__restrict__ p, T *__restrict__ x,
                                                   double *__restrict__ partial, const PcgScalars *sc)
{
    __shared__ double red[4];
    const int done = sc->done;
    T rz = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        if (done == 3) { x[i] = 0; continue; } // rhsNorm2 == 0 -> x.setZero()
        if (done) continue;
        const T ri = r[i];
        const T zi = (CODED ? invd[dcode[i]] : invd[i]) * ri;
        p[i] = zi;
        rz += ri * zi;
    }
    const double s = block_sum((double)rz, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// value-indexed matrix: invd[i] == invtab[dcode[i]], where invtab[c] = 1 / table[c] (1 for a zero) and the extra
// entry invtab[table_size] = 1 stands for "no diagonal entry" -- the same doubles k_inv_diag writes
__global__ __launch_bounds__(kBlock) void k_inv_diag_coded(CsrView A, uint16_t *__restrict__ dcode, double *__restrict__ invtab)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i <= A.table_size) invtab[i] = inv_table_entry<double>(A, i);
    if (i >= A.n) return;
    unsigned code = (unsigned)A.table_size;
    for (int k = A.row_ptr[i]; k < A.row_ptr[i + 1]; ++k)
        if (A.col[k] == (int32_t)i) code = A.codes[k];
    dcode[i] = (uint16_t)code;
}
// the float loops' dictionary: the same table narrowed, then inverted in float (the codes are k_inv_diag_coded's)
__global__ __launch_bounds__(kBlock) void k_f32_invtab(CsrView A, float *__restrict__ invtab)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i > A.table_size) return;
    invtab[i] = inv_table_entry<float>(A, i);
}

// ---------------------------------------------------------------------------------------------
// The scalar prologue of the vector kernels of the launch-per-phase loops (k_update_r and k_update_xp, below).  None of a
// kernel's stream loads depends on alpha or beta, and the scalar loads do not depend on each other, so at kernel entry every thread
// requests, in this order and without waiting for anything:
//   1. vec_request: the scalars (uniform loads; a kernel uses the ones its form needs, the others are never loaded) and its share of
//      the partial sums of the launch before (up to kFoldBatch per array: all of them in the loops' own launches);
//   2. the stream loads of its first kVecAhead grid-stride trips (a lane without such a trip reads *sc and drops the value: with no
//      branch between the requests the compiler can wait for the partial sums alone -- loads return in order);
//   3. vec_fold: folds the partial sums behind a single barrier while the streams are still in flight.
// The chain this replaces ran, in every workgroup and before the first byte of a stream was requested: load done -> load the partials
// -> two barriers per block_sum -> tot through LDS and a third barrier -> load rho / threshold -> divide -> first stream load at
// cold-start latency.
// The fold's arithmetic is the old one: thread t adds partial[t + 256 j] in ascending j (absent entries add +0.0, which changes no bit
// of a sum that started from +0.0), wave_sum, ((w0 + w1) + w2) + w3 -- the same bits in every thread of every workgroup.
// ---------------------------------------------------------------------------------------------
static constexpr int kVecAhead = 1;  // trips whose loads leave before the fold (1 against 2: profiles/vector_prologue.md)
static constexpr int kFoldBatch = 8; // partial sums per thread and array requested at once (k_update_xp at kVecGrid: 8 + 8)
struct VecScalars {
    int done;
    double alpha, beta, pAp, rho_old, threshold; // sc as it was at kernel entry (rho_old: the slot of this iteration's parity)
    double sum[2];                               // vec_fold: the folded partial sums
    double va[kFoldBatch], vb[kFoldBatch];       // vec_request: the thread's first partial sums as loaded (entries beyond count: part[0])
};
// NS sums to fold: 0 (the scalar step was a launch of its own), 1 (part[0 .. count)), 2 (+ part[second .. second + count))
template <int NS>
__device__ __forceinline__ VecScalars vec_request(const PcgScalars *sc, int parity, const double *__restrict__ part, int count, int second)
{
    VecScalars s;
    s.done = sc->done;
    s.alpha = sc->alpha;
    s.beta = sc->beta;
    s.pAp = sc->pAp;
    s.rho_old = *(parity ? &sc->rho_alt : &sc->rho);
    s.threshold = sc->threshold;
    s.sum[0] = s.sum[1] = 0.;
#pragma unroll
    for (int u = 0; u < kFoldBatch; ++u) {
        const int k = u * kBlock + (int)threadIdx.x, kc = k < count ? k : 0;
        s.va[u] = NS > 0 ? part[kc] : 0.;
        s.vb[u] = NS > 1 ? part[second + kc] : 0.;
    }
    __builtin_amdgcn_sched_barrier(0); // (the streams' requests stay behind these: what returns first is what is needed first)
    return s;
}
template <int NS>
__device__ __forceinline__ void vec_fold(VecScalars &s, const double *__restrict__ part, int count, int second, double *lds8)
{
    if (NS == 0) return;
    __builtin_amdgcn_sched_barrier(0);
    double a = 0., b = 0.;
#pragma unroll
    for (int u = 0; u < kFoldBatch; ++u) {
        const bool in = u * kBlock + (int)threadIdx.x < count;
        a += in ? s.va[u] : 0.;
        if (NS > 1) b += in ? s.vb[u] : 0.;
    }
    for (int k = kFoldBatch * kBlock + (int)threadIdx.x; k < count; k += kBlock) { // (k_update_r beyond 2048 partial sums)
        a += part[k];
        if (NS > 1) b += part[second + k];
    }
    block_sum2(a, b, lds8);
    s.sum[0] = a;
    s.sum[1] = b;
}
// the address a lane's stream load goes to: its rows, or *sc for a lane whose trip lies beyond the last row (value never used)
template <typename V, typename E>
__device__ __forceinline__ const V *vec_src(bool live, const E *rows, const PcgScalars *sc)
{
    return live ? reinterpret_cast<const V *>(rows) : reinterpret_cast<const V *>(sc);
}

// ---------------------------------------------------------------------------------------------
// k_update_r and k_update_xp: T is the type of the vectors, S the type the scalar step is computed in.  The three loops:
//   <double, double>  the fp64 loop;
//   <float, float>    AVS_PRECISION_F32 -- alpha, beta and the threshold test are FLOAT operations on the float-rounded sums;
//   <float, double>   the mixed-precision loop (avs_pcg_mixed.inl) -- double quotients of the unrounded sums, published unrounded and
//                     rounded to float only where they multiply the float vectors.
// A thread takes Vec16<T>::rows rows per trip (16-B accesses; the arrays are 16-B aligned); the rows behind the last full 16 B go
// alone, to thread 0 of workgroup 0.  A thread's own sums are added in T, everything across threads, workgroups and launches in double.
// ---------------------------------------------------------------------------------------------
// f(k) for the rows k = 0 .. R - 1 of a 16-B access, as straight-line code
template <int R, typename F> __device__ __forceinline__ void for_rows(F &&f)
{
    f(0);
    f(1);
    if constexpr (R == 4) {
        f(2);
        f(3);
    }
}
// The rows behind a vector's last full 16 B go alone, to thread 0 of workgroup 0: rows [vec_tail_begin, n).  fp64 has one such row at
// most and says so -- taken if n is odd, first row n - 1 --, which the compiler turns into a test where it would otherwise keep a loop.
template <typename T> __device__ __forceinline__ bool vec_tail_mine(int64_t n)
{
    return (Vec16<T>::rows > 2 || (n & 1)) && blockIdx.x == 0 && threadIdx.x == 0;
}
template <typename T> __device__ __forceinline__ int64_t vec_tail_begin(int64_t n)
{
    return Vec16<T>::rows == 2 ? n - 1 : Vec16<T>::rows * (n >> Vec16<T>::log2_rows);
}
// KEEP of update_r's accesses to r.  The fp64 kernel hints them like its other read-once streams; the float kernels load and store r
// plainly whatever KEEP is (as they were measured; hinting them is a performance change of its own).
#ifndef AVS_EXP_NO_RNT
template <typename T, bool KEEP> constexpr bool kKeepR = KEEP || std::is_same<T, float>::value;
#else
template <typename T, bool KEEP> constexpr bool kKeepR = true;
#endif

// The alpha step, alpha = r.z / p.Ap, as every workgroup takes it for itself.  FUSED: p.Ap is the folded sum of the SpMV's partials and
// thread 0 of workgroup 0 publishes what OP_ALPHA would.  Else OP_ALPHA has run: its double quotient is read -- but S = float divides
// again, in float, and publishes that (OP_ALPHA divided in double: k_update_xp reads this one).
template <typename T, typename S, bool FUSED>
__device__ __forceinline__ T alpha_step(const VecScalars &s, PcgScalars *sc)
{
    if (FUSED) {
        const double pap = s.sum[0];
        const S alpha = (S)s.rho_old / (S)pap;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            sc->red[0] = pap;
            sc->pAp = (double)(S)pap;
            sc->alpha = (double)alpha;
        }
        return (T)alpha;
    }
    if (std::is_same<S, double>::value) return (T)s.alpha;
    const S alpha = (S)s.rho_old / (S)s.pAp;
    if (blockIdx.x == 0 && threadIdx.x == 0) sc->alpha = (double)alpha;
    return (T)alpha;
}

// The beta step of an iteration that is not done, as every workgroup takes it for itself: convergence test (Eigen: break before i++,
// x += alpha p still pending: done = 2), else beta = r.z / old r.z; thread 0 of workgroup 0 publishes what OP_BETA would.  The sums, the
// old r.z and the threshold are rounded to S first and the scalars published as S holds them.  Mixed loop (T = float, S = double): the
// iteration that claims convergence leaves the r.z it started from in sc->rho whatever its parity (the reliable update reads it there;
// nobody reads sc->rho in an odd iteration: it is the slot this iteration would have written).
template <typename T, typename S>
__device__ __forceinline__ T beta_step(const VecScalars &s, PcgScalars *sc, int parity, int &done)
{
    const S rr = (S)s.sum[0], rz = (S)s.sum[1];
    const S absOld = (S)s.rho_old;
    S beta = 0;
    if (rr < (S)s.threshold) done = 2;
    else beta = rz / absOld;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sc->red[0] = (double)rr;
        sc->red[1] = (double)rz;
        sc->rr = (double)rr;
        if (done == 2) {
            sc->done = 2;
            if (!std::is_same<T, S>::value && parity) sc->rho = (double)absOld;
        } else {
            if (parity) sc->rho = (double)rz;
            else sc->rho_alt = (double)rz;
            // (mixed loop: the quotient is formed again for the store, as that kernel always has -- keeps its code object as it was)
            sc->beta = std::is_same<T, S>::value ? (double)beta : (double)(rz / absOld);
            sc->iter += 1;
        }
    }
    return (T)beta;
}

// r -= alpha t ; partials: r.r and r.(invd r).  (x += alpha p rides along with the p update below:
// one vector pass less per iteration -- 10 n instead of 11 n doubles of traffic.)
// FUSED (single-GPU loop, small systems): the alpha step -- fold of the SpMV's `nb` partial sums, alpha = r.z / p.Ap -- is done
// here by every workgroup for itself, as k_update_xp does with the beta step; only worth it while the SpMV leaves few
// partials (one per wave of 64 rows): the loop uses it up to kFuseAlphaMax of them.  The kernel's own partial sums then go
// to a second array (`partial`), because other workgroups are still reading the SpMV's.
template <typename T, typename S, bool CODED, bool FUSED, bool KEEP>
__global__ __launch_bounds__(kBlock) void k_update_r(int64_t n, T *__restrict__ r, const T *__restrict__ t, const T *__restrict__ invd,
                                                     const uint16_t *__restrict__ dcode, PcgScalars *sc, double *__restrict__ partial,
                                                     const double *__restrict__ spmv_partial, int nb, int parity)
{
    typedef typename Vec16<T>::type V;
    typedef typename Vec16<T>::codes C;
    constexpr int R = Vec16<T>::rows;
    __shared__ double pro[8], red[8];
    // t = A p is read for the last time here and r is next read one kernel later: the streams that nobody reads again before they
    // are overwritten are loaded / stored NON-TEMPORALLY, so that they do not push the matrix out of the caches between two products
    // (`keep`: matrix and vectors together fit the Infinity Cache -- then everything is left to it)
    const int64_t nv = n >> Vec16<T>::log2_rows; // R rows per thread and trip, partial sums in the order of the rows
    const int64_t j0 = (int64_t)blockIdx.x * kBlock + threadIdx.x, stride = (int64_t)gridDim.x * kBlock;
    struct Trip { V rv, tv, iv; C cc; };
    auto request = [&](int64_t j, bool live, Trip &q) {
        const int64_t i = R * j;
        q.rv = stream_load_k<kKeepR<T, KEEP>>(vec_src<V>(live, r + i, sc));
        q.tv = stream_load_k<KEEP>(vec_src<V>(live, t + i, sc));
        if (CODED) q.cc = stream_load_k<KEEP>(vec_src<C>(live, dcode + i, sc));
        else q.iv = *vec_src<V>(live, invd + i, sc);
    };
    VecScalars s = vec_request<FUSED ? 1 : 0>(sc, parity, spmv_partial, nb, 0);
    Trip ahead[kVecAhead];
#pragma unroll
    for (int u = 0; u < kVecAhead; ++u) request(j0 + u * stride, j0 + u * stride < nv, ahead[u]);
    vec_fold<FUSED ? 1 : 0>(s, spmv_partial, nb, 0, pro);
    if (s.done) {
        if (FUSED && blockIdx.x == 0 && threadIdx.x == 0 && s.done == 2) sc->done = 1; // the pending x update has run (OP_ALPHA)
        return;
    }
    const T alpha = alpha_step<T, S, FUSED>(s, sc);
    T rr = 0, rz = 0;
    auto rows = [&](int64_t j, const Trip &q) {
        const int64_t i = R * j;
        V iv;
        if (CODED) for_rows<R>([&](int k) { iv[k] = invd[code_of(q.cc, k)]; });
        else iv = q.iv;
        V rn;
        for_rows<R>([&](int k) { rn[k] = q.rv[k] - alpha * q.tv[k]; });
        stream_store_k<kKeepR<T, KEEP>>(rn, reinterpret_cast<V *>(r + i));
        for_rows<R>([&](int k) {
            rr += rn[k] * rn[k];
            rz += rn[k] * (iv[k] * rn[k]);
        });
    };
#pragma unroll
    for (int u = 0; u < kVecAhead; ++u)
        if (j0 + u * stride < nv) rows(j0 + u * stride, ahead[u]);
    for (int64_t j = j0 + kVecAhead * stride; j < nv; j += stride) {
        Trip q;
        request(j, true, q);
        rows(j, q);
    }
    if (vec_tail_mine<T>(n))
        for (int64_t i = vec_tail_begin<T>(n); i < n; ++i) {
            const T ri = r[i] - alpha * t[i];
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

// x += alpha p (Eigen does this before the convergence test, so it also runs in the iteration that
// converges: done == 2 = "converged, x update pending"); then p = invd r + beta p unless converged.
//
// FUSED (single-GPU loop): the beta step -- sum of k_update_r's 2 g partial sums, convergence test, beta = r.z / old r.z --
// is done HERE, by every workgroup for itself (8 + 8 loads per thread from L2, the same fixed order everywhere => the same
// bits everywhere), instead of in a k_reduce launch of its own between the two vector kernels (4.9 us + a launch gap per
// iteration).  Workgroup 0 publishes the scalars; the old r.z is read from the slot of this iteration's parity and the new
// one written to the other slot, so a workgroup that starts late still reads what the early ones read.
// The float and mixed loops have only this form.
template <typename T, typename S, bool CODED, bool FUSED, bool KEEP>
__global__ __launch_bounds__(kBlock) void k_update_xp(int64_t n, T *__restrict__ x, T *__restrict__ p, const T *__restrict__ r,
                                                      const T *__restrict__ invd, const uint16_t *__restrict__ dcode, PcgScalars *sc,
                                                      const double *__restrict__ partial, int g, int parity)
{
    static_assert(FUSED || std::is_same<T, double>::value, "the loops on float vectors always take the beta step here");
    typedef typename Vec16<T>::type V;
    typedef typename Vec16<T>::codes C;
    constexpr int R = Vec16<T>::rows;
    __shared__ double pro[8];
    const int64_t nv = n >> Vec16<T>::log2_rows;
    const int64_t j0 = (int64_t)blockIdx.x * kBlock + threadIdx.x, stride = (int64_t)gridDim.x * kBlock;
    struct Trip { V pv, xv, rv, iv; C cc; };
    auto request = [&](int64_t j, bool live, Trip &q) {
        const int64_t i = R * j;
        q.pv = *vec_src<V>(live, p + i, sc);
        q.xv = stream_load_k<KEEP>(vec_src<V>(live, x + i, sc));
        q.rv = stream_load_k<KEEP>(vec_src<V>(live, r + i, sc));
        if (CODED) q.cc = stream_load_k<KEEP>(vec_src<C>(live, dcode + i, sc));
        else q.iv = *vec_src<V>(live, invd + i, sc);
    };
    VecScalars s = vec_request<FUSED ? 2 : 0>(sc, parity, partial, g, g);
    Trip ahead[kVecAhead];
#pragma unroll
    for (int u = 0; u < kVecAhead; ++u) request(j0 + u * stride, j0 + u * stride < nv, ahead[u]);
    vec_fold<FUSED ? 2 : 0>(s, partial, g, g, pro);
    int done = s.done;
    if (done == 1 || done == 3) return;
    const T alpha = (T)s.alpha;
    T beta = FUSED ? T(0) : (T)s.beta;
    if (FUSED && done == 0) beta = beta_step<T, S>(s, sc, parity, done);
    if (done == 2) { // (the loads that went ahead are dropped)
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
            x[i] += alpha * p[i];
        return;
    }
    auto rows = [&](int64_t j, const Trip &q) {
        const int64_t i = R * j;
        V iv;
        if (CODED) for_rows<R>([&](int k) { iv[k] = invd[code_of(q.cc, k)]; });
        else iv = q.iv;
        V xn, pn;
        for_rows<R>([&](int k) { xn[k] = q.xv[k] + alpha * q.pv[k]; });
        for_rows<R>([&](int k) { pn[k] = iv[k] * q.rv[k] + beta * q.pv[k]; });
        stream_store_k<KEEP>(xn, reinterpret_cast<V *>(x + i)); // (x is touched once per iteration)
        *reinterpret_cast<V *>(p + i) = pn;
    };
#pragma unroll
    for (int u = 0; u < kVecAhead; ++u)
        if (j0 + u * stride < nv) rows(j0 + u * stride, ahead[u]);
    for (int64_t j = j0 + kVecAhead * stride; j < nv; j += stride) {
        Trip q;
        request(j, true, q);
        rows(j, q);
    }
    if (vec_tail_mine<T>(n))
        for (int64_t i = vec_tail_begin<T>(n); i < n; ++i) {
            const T pi = p[i];
            x[i] += alpha * pi;
            p[i] = (CODED ? invd[dcode[i]] : invd[i]) * r[i] + beta * pi;
        }
}

// ---------------------------------------------------------------------------------------------
// k_update_r and k_update_xp as ONE launch for HBM-sized systems -- r -= alpha t with its two sums, a GRID BARRIER, then x += alpha p ;
// p = invd r + beta p with the new r still in REGISTERS and LDS: 7.25 n instead of 8.5 n doubles of traffic per iteration and one launch
// boundary less.  kVecGrid / 8 workgroups of 1024 threads, one per CU (128 registers per lane: 16 rows of r per lane x 2); every sum is
// formed in exactly the order of the two kernels it replaces -- thread T of workgroup B plays the threads (T & 255) of the 256-thread
// workgroups 4 B + (T >> 8) and 1024 + 4 B + (T >> 8) of the kVecGrid-workgroup launches (same rows, same order, the same wave /
// four-wave folds, the same partial-sum arrays, the same 256-lane folds of them, which every quarter forms for itself) -- so the
// iteration, its scalars and the solution are bit-identical with the option on or off.
// Order of the requests (profiles/fused_vectors.md; the order of vec_request / vec_fold above):
//   entry     done and the scalars, the thread's share of the SpMV's partial sums (branch-free), its share of the inverted dictionary,
//             the first batch of r, t and codes -- all before anything is waited for; the fold and the dictionary's way into LDS share
//             one workgroup barrier, with the streams in flight;
//   phase 1   r, t, the codes and the store of r are NON-TEMPORAL unless KEEP (r is not read again before it is overwritten, and must
//             not push the matrix and p out of the Infinity Cache in front of the SpMV); p stays plain, the SpMV reads it next;
//   barrier   the first batch of phase 2 (p, x, codes: nothing of it depends on phase 1) is requested before the four sums of the
//             workgroup's halves go through ONE workgroup barrier and are published; behind the last poll every thread requests its
//             8 + 8 partial sums at once, folds them through one more workgroup barrier, and phase 2 starts on loads that have landed.
// The barrier: the partial sums leave with write-through stores (agent scope), one monotonic 64-bit counter (a launch's target is the
// next multiple of the grid above its own ticket), relaxed polls with s_sleep, bounded by wall_clock64 -- a grid that is not co-resident
// in time (the GPU shared with other work) sets sc->fault instead of hanging.  No L2 write-back fence anywhere: what crosses the barrier
// is read with agent-scope loads.  Plain launch (a graph node like any other); needs every CU free, which holds behind the persistent SpMV.
// ---------------------------------------------------------------------------------------------
static constexpr size_t kFusedTabBytes = (size_t)(kViLdsTable + 1) * sizeof(double) + 8; // CODED: the inverted dictionary
static constexpr size_t kFusedLds = (size_t)8 * 1024 * 16; // the second emulated workgroup's new r: kFusedPairs x kFusedBlock pairs of doubles
static constexpr unsigned kFusedStride = (unsigned)kVecGrid * kBlock * 16u; // bytes between two pairs of an emulated thread
static constexpr int kFusedBlock = 1024, kFusedPairs = 8, kFusedBatch = 4; // (loads in flight per lane: kFusedBatch pairs of rows of each stream)
static constexpr int kFusedTabAhead = (kViLdsTable + 1 + kFusedBlock - 1) / kFusedBlock; // dictionary entries a thread requests at entry
// (kFusedPairs pairs of rows per emulated thread: n <= 2 * kFusedPairs * kVecGrid * kBlock rows)
static_assert(kVecGrid == kFoldBatch * kBlock, "the beta fold requests all of a thread's partial sums in one batch");
#ifndef AVS_EXP_FUSED_AHEAD // where phase 2's first batch is requested (the experiment of profiles/fused_vectors.md): 0 behind the beta fold,
#define AVS_EXP_FUSED_AHEAD 2 // 1 in front of the partial sums' publication, 2 behind the ticket
#endif
// element at a 32-bit BYTE offset from a uniform base (global_load ... saddr: no 64-bit address per lane and stream kept in registers)
template <class T> __device__ __forceinline__ T *at_off(T *base, unsigned byte_off)
{
    return reinterpret_cast<T *>(reinterpret_cast<char *>(base) + (size_t)byte_off);
}
template <class T> __device__ __forceinline__ const T *at_off(const T *base, unsigned byte_off)
{
    return reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + (size_t)byte_off);
}
// one batch of a phase's streams as loaded: u, v = (r, t) in phase 1 and (p, x) in phase 2; the codes or the inverse diagonal of the rows
struct FusedBatch {
    d2_t u[kFusedBatch], v[kFusedBatch], idv[kFusedBatch];
    unsigned cc[kFusedBatch];
};
template <bool CODED, bool KEEP>
__global__ __launch_bounds__(kFusedBlock) void k_update_fused(int64_t n, double *__restrict__ x, double *__restrict__ p, double *__restrict__ r,
                                                              const double *__restrict__ t, const double *__restrict__ invd,
                                                              const uint16_t *__restrict__ dcode, PcgScalars *sc, double *__restrict__ vpart,
                                                              const double *__restrict__ spmv_partial, int nb, int parity,
                                                              unsigned long long *__restrict__ bar, long long timeout_ticks, int tab_n)
{
    // (every array is written once per launch: no barrier guards a reuse)
    __shared__ double fold_a[4][4];   // alpha fold: [quarter][wave]
    __shared__ double sums[4][4][4];  // phase 1: [quarter][rr0, rz0, rr1, rz1][wave]
    __shared__ double fold_b[4][8];   // beta fold: [quarter][rr waves | rz waves]
    __shared__ int sh_fail;
    extern __shared__ __attribute__((aligned(16))) unsigned char fused_lds[];
    d2_t *rl = reinterpret_cast<d2_t *>(fused_lds);                  // the new r of the second emulated workgroup's rows: rl[m * kFusedBlock + T] (128 KiB)
    double *tab = reinterpret_cast<double *>(fused_lds + kFusedLds); // CODED: the inverted dictionary (tab_n entries)
    const int T = threadIdx.x, tq = T & 255, q = T >> 8, wv = tq >> 6;
    constexpr int g = kVecGrid;
    const int64_t n2 = n >> 1;
    const unsigned lim = (unsigned)n2 * 16u; // byte offset behind the last pair (n < 2^28 rows: checked by the host)
    // byte offset of pair m of the emulated thread of half h; the loads of a lane beyond the last pair are clamped to pair 0 and their
    // results dropped: no branches around the loads, one predicate per store and per sum
    // (opaque: an offset is formed again wherever it is used instead of being carried, spilled, through the kernel)
    auto pair_off = [&](int h, int m) {
        unsigned o = (unsigned)T;
        asm volatile("" : "+v"(o));
        return (((unsigned)blockIdx.x * 4u + (o >> 8) + (unsigned)(g / 2) * (unsigned)h) * kBlock + (o & 255u)) * 16u + (unsigned)m * kFusedStride;
    };
    auto request1 = [&](int h, int m0, FusedBatch &b) {
#pragma unroll
        for (int u = 0; u < kFusedBatch; ++u) {
            const unsigned oj = pair_off(h, m0 + u), o = oj < lim ? oj : 0u;
            b.u[u] = stream_load_k<KEEP>(reinterpret_cast<const d2_t *>(at_off(r, o)));
            b.v[u] = stream_load_k<KEEP>(reinterpret_cast<const d2_t *>(at_off(t, o)));
            if (CODED) b.cc[u] = stream_load_k<KEEP>(reinterpret_cast<const unsigned *>(at_off(dcode, o >> 2))); // (read again in phase 2: 0.25 n)
            else b.idv[u] = *reinterpret_cast<const d2_t *>(at_off(invd, o));
        }
    };
    auto request2 = [&](int h, int m0, FusedBatch &b, bool px, bool id) { // px: p and x; id: the codes / the inverse diagonal
#pragma unroll
        for (int u = 0; u < kFusedBatch; ++u) {
            const unsigned oj = pair_off(h, m0 + u), o = oj < lim ? oj : 0u;
            if (px) {
                b.u[u] = *reinterpret_cast<const d2_t *>(at_off(p, o));
                b.v[u] = stream_load_k<KEEP>(reinterpret_cast<const d2_t *>(at_off(x, o)));
            }
            if (id) {
                if (CODED) b.cc[u] = stream_load_k<KEEP>(reinterpret_cast<const unsigned *>(at_off(dcode, o >> 2)));
                else b.idv[u] = *reinterpret_cast<const d2_t *>(at_off(invd, o));
            }
        }
    };
    // ---- entry: every request that depends on nothing, in the order in which the results are needed (loads return in order)
    const int d = sc->done;
    const double rho_old = parity ? sc->rho_alt : sc->rho, threshold = sc->threshold, alpha_in = sc->alpha;
    double va[kFoldBatch], dv[kFusedTabAhead];
#pragma unroll
    for (int u = 0; u < kFoldBatch; ++u) {
        const int k = u * kBlock + tq;
        va[u] = spmv_partial[k < nb ? k : 0];
    }
    if (CODED) {
#pragma unroll
        for (int u = 0; u < kFusedTabAhead; ++u) {
            const int i = u * kFusedBlock + T;
            dv[u] = invd[i < tab_n ? i : 0];
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    FusedBatch cur;
    request1(0, 0, cur);
    __builtin_amdgcn_sched_barrier(0);
    // ---- alpha: the fold of the SpMV's partial sums as every workgroup of k_update_r<FUSED> does it, by every quarter for itself (the
    //      barrier in it publishes the table)
    double pap = 0.;
#pragma unroll
    for (int u = 0; u < kFoldBatch; ++u) pap += u * kBlock + tq < nb ? va[u] : 0.;
    for (int k = kFoldBatch * kBlock + tq; k < nb; k += kBlock) pap += spmv_partial[k]; // (beyond 2048 partial sums)
    pap = wave_sum(pap);
    if ((T & 63) == 0) fold_a[q][wv] = pap;
    if (CODED) {
#pragma unroll
        for (int u = 0; u < kFusedTabAhead; ++u) {
            const int i = u * kFusedBlock + T;
            if (i < tab_n) tab[i] = dv[u];
        }
    }
    if (T == 0) sh_fail = 0;
    __syncthreads();
    if (d) { // (the loads that went ahead are dropped)
        if (blockIdx.x == 0 && T == 0 && d == 2 && nb) sc->done = 1; // the pending x update has run (nb == 0: OP_ALPHA has said so)
        return;
    }
    pap = ((fold_a[q][0] + fold_a[q][1]) + fold_a[q][2]) + fold_a[q][3];
    const double alpha = nb ? rho_old / pap : alpha_in; // (nb == 0: the alpha step was a launch of its own, as in front of k_update_r<., ., ., false, .>)
    // ---- phase 1: r -= alpha t
    d2_t rn[kFusedPairs]; // the new r of the first emulated workgroup's rows: registers
    double rr[2] = {0., 0.}, rz[2] = {0., 0.};
    auto consume1 = [&](int h, int m0, const FusedBatch &b) {
#pragma unroll
        for (int u = 0; u < kFusedBatch; ++u) {
            const int m = m0 + u;
            const unsigned oj = pair_off(h, m);
            // (opaque: used here, in front of the predicate -- the optimiser otherwise sinks a batch's first code load into the predicated
            //  block, where it becomes a second, dependent round trip)
            unsigned c = CODED ? b.cc[u] : 0u;
            double id0 = CODED ? 0. : b.idv[u].x, id1 = CODED ? 0. : b.idv[u].y;
            if (CODED) {
                asm volatile("" : "+v"(c));
                id0 = tab[c & 0xffffu];
                id1 = tab[c >> 16];
            } else asm volatile("" : "+v"(id0), "+v"(id1));
            d2_t v;
            v.x = b.u[u].x - alpha * b.v[u].x;
            v.y = b.u[u].y - alpha * b.v[u].y;
            if (h == 0) rn[m] = v;
            else rl[m * kFusedBlock + T] = v;
            if (oj < lim) {
                stream_store_k<KEEP>(v, reinterpret_cast<d2_t *>(at_off(r, oj)));
                rr[h] += v.x * v.x;
                rz[h] += v.x * (id0 * v.x);
                rr[h] += v.y * v.y;
                rz[h] += v.y * (id1 * v.y);
            }
        }
    };
    constexpr int kBatches = 2 * kFusedPairs / kFusedBatch; // of a phase: the first half's, then the second half's
#pragma unroll
    for (int k = 0; k < kBatches; ++k) {
        consume1(k / (kBatches / 2), k % (kBatches / 2) * kFusedBatch, cur);
        __builtin_amdgcn_sched_barrier(0); // (the next batch's loads stay behind this batch: registers)
        if (k + 1 < kBatches) request1((k + 1) / (kBatches / 2), (k + 1) % (kBatches / 2) * kFusedBatch, cur);
        __builtin_amdgcn_sched_barrier(0);
    }
    double r_last = 0.;
    if ((n & 1) && blockIdx.x == 0 && T == 0) { // (the odd last row: thread 0 of workgroup 0 of k_update_r)
        const int64_t i = n - 1;
        r_last = r[i] - alpha * t[i];
        r[i] = r_last;
        rr[0] += r_last * r_last;
        rz[0] += r_last * ((CODED ? invd[dcode[i]] : invd[i]) * r_last);
    }
#if AVS_EXP_FUSED_AHEAD == 1
    request2(0, 0, cur, true, CODED);
    __builtin_amdgcn_sched_barrier(0);
#endif
    {
        const double s0 = wave_sum(rr[0]), s1 = wave_sum(rz[0]), s2 = wave_sum(rr[1]), s3 = wave_sum(rz[1]);
        if ((T & 63) == 0) {
            sums[q][0][wv] = s0;
            sums[q][1][wv] = s1;
            sums[q][2][wv] = s2;
            sums[q][3][wv] = s3;
        }
    }
    __syncthreads();
    if (tq == 0) { // write-through: the other workgroups read these behind the barrier
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int b = (int)blockIdx.x * 4 + q + (g / 2) * h;
            const double srr = ((sums[q][2 * h][0] + sums[q][2 * h][1]) + sums[q][2 * h][2]) + sums[q][2 * h][3];
            const double srz = ((sums[q][2 * h + 1][0] + sums[q][2 * h + 1][1]) + sums[q][2 * h + 1][2]) + sums[q][2 * h + 1][3];
            __hip_atomic_store(vpart + b, srr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(vpart + g + b, srz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // ---- grid barrier
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the partial sums are acknowledged before the ticket is drawn
    __syncthreads();
    unsigned long long ticket = 0;
    if (T == 0) ticket = __hip_atomic_fetch_add(bar, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#if AVS_EXP_FUSED_AHEAD == 2
    // phase 2's first batch leaves here, behind the ticket: it is under way while the grid meets and the sums are folded, and it does not
    // hold the ticket back (in front of it, it sat under the wait for the partial sums' acknowledgement: profiles/fused_vectors.md).
    // The 8-B inverse diagonal of its rows follows when the partial sums' registers are free again (128 registers per lane)
    __builtin_amdgcn_sched_barrier(0);
    request2(0, 0, cur, true, CODED);
    __builtin_amdgcn_sched_barrier(0);
#endif
    if (T == 0) {
        const unsigned long long target = (ticket / gridDim.x + 1ull) * gridDim.x;
        const long long t0 = wall_clock64();
        while (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            __builtin_amdgcn_s_sleep(2);
            if (wall_clock64() - t0 > timeout_ticks) { sh_fail = 1; break; }
        }
    }
    __syncthreads();
    // ---- beta: the fold of the 2 g partial sums as every workgroup of k_update_xp<FUSED> does it, by every quarter for itself; all
    //      of a thread's 8 + 8 are requested before the first is waited for
    double fa[kFoldBatch], fb[kFoldBatch];
#pragma unroll
    for (int u = 0; u < kFoldBatch; ++u) {
        fa[u] = __hip_atomic_load(vpart + u * kBlock + tq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        fb[u] = __hip_atomic_load(vpart + g + u * kBlock + tq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (sh_fail) { // not every workgroup arrived in time: the solve is void (the host reads sc->fault and redoes it with the two launches)
        if (T == 0) {
            __hip_atomic_store(&sc->fault, 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&sc->done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return;
    }
    double frr = 0., frz = 0.;
#pragma unroll
    for (int u = 0; u < kFoldBatch; ++u) {
        frr += fa[u];
        frz += fb[u];
    }
    __builtin_amdgcn_sched_barrier(0);
#if AVS_EXP_FUSED_AHEAD != 0
    if (!CODED) request2(0, 0, cur, false, true);
#else
    request2(0, 0, cur, true, true);
#endif
    __builtin_amdgcn_sched_barrier(0);
    frr = wave_sum(frr);
    frz = wave_sum(frz);
    if ((T & 63) == 0) {
        fold_b[q][wv] = frr;
        fold_b[q][4 + wv] = frz;
    }
    __syncthreads();
    frr = ((fold_b[q][0] + fold_b[q][1]) + fold_b[q][2]) + fold_b[q][3];
    frz = ((fold_b[q][4] + fold_b[q][5]) + fold_b[q][6]) + fold_b[q][7];
    int done = 0;
    double beta = 0.;
    if (frr < threshold) done = 2; // Eigen: break before i++ (x += alpha p still runs)
    else beta = frz / rho_old;
    if (blockIdx.x == 0 && T == 0) { // what OP_ALPHA and OP_BETA do
        if (nb) {
            sc->pAp = pap;
            sc->alpha = alpha;
        }
        sc->red[0] = frr;
        sc->red[1] = frz;
        sc->rr = frr;
        if (done == 2) sc->done = 2;
        else {
            if (parity) sc->rho = frz;
            else sc->rho_alt = frz;
            sc->beta = beta;
            sc->iter += 1;
        }
    }
    // ---- phase 2: x += alpha p ; p = invd r + beta p
    auto consume2 = [&](int h, int m0, const FusedBatch &b) {
#pragma unroll
        for (int u = 0; u < kFusedBatch; ++u) {
            const int m = m0 + u;
            const unsigned oj = pair_off(h, m);
            // (opaque: used here, in front of the predicate -- the optimiser otherwise sinks a batch's first code load into the predicated
            //  block, where it becomes a second, dependent round trip)
            unsigned c = CODED ? b.cc[u] : 0u;
            double id0 = CODED ? 0. : b.idv[u].x, id1 = CODED ? 0. : b.idv[u].y;
            if (CODED) {
                asm volatile("" : "+v"(c));
                id0 = tab[c & 0xffffu];
                id1 = tab[c >> 16];
            } else asm volatile("" : "+v"(id0), "+v"(id1));
            const d2_t rv = h == 0 ? rn[m] : rl[m * kFusedBlock + T];
            double p0 = b.u[u].x, p1 = b.u[u].y, x0 = b.v[u].x, x1 = b.v[u].y;
            asm volatile("" : "+v"(p0), "+v"(p1), "+v"(x0), "+v"(x1)); // (as the codes: everything below is used behind the predicate only)
            d2_t xn, pn;
            xn.x = x0 + alpha * p0;
            xn.y = x1 + alpha * p1;
            pn.x = id0 * rv.x + beta * p0;
            pn.y = id1 * rv.y + beta * p1;
            if (oj < lim) {
                stream_store_k<KEEP>(xn, reinterpret_cast<d2_t *>(at_off(x, oj)));
                if (done != 2) *reinterpret_cast<d2_t *>(at_off(p, oj)) = pn;
            }
        }
    };
#pragma unroll
    for (int k = 0; k < kBatches; ++k) {
        consume2(k / (kBatches / 2), k % (kBatches / 2) * kFusedBatch, cur);
        __builtin_amdgcn_sched_barrier(0);
        if (k + 1 < kBatches) request2((k + 1) / (kBatches / 2), (k + 1) % (kBatches / 2) * kFusedBatch, cur, true, true);
        __builtin_amdgcn_sched_barrier(0);
    }
    if ((n & 1) && blockIdx.x == 0 && T == 0) {
        const int64_t i = n - 1;
        const double pi = p[i];
        x[i] += alpha * pi;
        if (done != 2) p[i] = (CODED ? invd[dcode[i]] : invd[i]) * r_last + beta * pi;
    }
}

// ---------------------------------------------------------------------------------------------
// scalar stages.  One 256-thread block sums `nb` partials of `nred` interleaved arrays in a fixed
// order (deterministic), then (optionally) applies the scalar update.
// ---------------------------------------------------------------------------------------------
static constexpr int kRedBlock = 1024;
__global__ __launch_bounds__(kRedBlock) void k_reduce(const double *__restrict__ partial, int nb, int nred,
                                                      PcgScalars *sc, int op, double tol, int skip_if_done, int red_off = 0)
{
    if (skip_if_done && sc->done) {
        if (threadIdx.x == 0 && (op == OP_ALPHA || op == OP_ALPHA_ODD) && sc->done == 2) sc->done = 1;
        return;
    }
    __shared__ double red[kRedBlock / 64];
    for (int q = 0; q < nred; ++q) {
        const double *src = partial + (size_t)q * nb;
        double s0 = 0., s1 = 0., s2 = 0., s3 = 0.;
        int i = threadIdx.x;
        for (; i + 3 * kRedBlock < nb; i += 4 * kRedBlock) { // 4 independent loads in flight
            const double a = src[i], b = src[i + kRedBlock], c = src[i + 2 * kRedBlock], d = src[i + 3 * kRedBlock];
            s0 += a; s1 += b; s2 += c; s3 += d;
        }
        for (; i < nb; i += kRedBlock) s0 += src[i];
        double s = wave_sum((s0 + s1) + (s2 + s3));
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.;
#pragma unroll
            for (int w = 0; w < kRedBlock / 64; ++w) t += red[w];
            sc->red[red_off + q] = t;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && op != OP_NONE) apply_scalar_op(sc, op, tol);
}

// Same job with kRedBlocks workgroups for long partial arrays (the value-indexed SpMV leaves one partial per wave:
// 116 k at 512^3): block b sums a fixed contiguous share (two loads per thread, one round trip), the block that arrives last
// folds the kRedBlocks sums with a fixed tree and applies the scalar update -- the result does not depend on the arrival order.
static constexpr int kRedBlocks = 64; // <= 64: the last block folds them with one wave
__global__ __launch_bounds__(kRedBlock) void k_reduce_mb(const double *__restrict__ partial, int nb, int nred, PcgScalars *sc, int op,
                                                        double tol, int skip_if_done, int red_off, double *__restrict__ stage,
                                                        unsigned *__restrict__ ticket)
{
    if (skip_if_done && sc->done) { // every block sees a non-zero flag whether or not block 0 has already stepped it
        if (blockIdx.x == 0 && threadIdx.x == 0 && (op == OP_ALPHA || op == OP_ALPHA_ODD) && sc->done == 2) sc->done = 1;
        return;
    }
    __shared__ double red[kRedBlock / 64];
    __shared__ int last;
    const int share = (nb + kRedBlocks - 1) / kRedBlocks;
    const int lo = blockIdx.x * share, hi = (lo + share < nb) ? lo + share : nb;
    for (int q = 0; q < nred; ++q) {
        const double *src = partial + (size_t)q * nb;
        double s0 = 0., s1 = 0., s2 = 0., s3 = 0.;
        int i = lo + threadIdx.x;
        for (; i + 3 * kRedBlock < hi; i += 4 * kRedBlock) {
            const double a = src[i], b = src[i + kRedBlock], c = src[i + 2 * kRedBlock], d = src[i + 3 * kRedBlock];
            s0 += a; s1 += b; s2 += c; s3 += d;
        }
        for (; i < hi; i += kRedBlock) s0 += src[i];
        double s = wave_sum((s0 + s1) + (s2 + s3));
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.;
#pragma unroll
            for (int w = 0; w < kRedBlock / 64; ++w) t += red[w];
            __hip_atomic_store(stage + q * kRedBlocks + blockIdx.x, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (threadIdx.x == 0) {
        // the block sums went out as write-through (agent-scope) atomic stores: waiting for their acknowledgement orders them
        // before the ticket -- an agent-scope release fence would also write back the XCD's dirty L2 (the y just computed)
        wait_own_stores();
        last = atomicAdd(ticket, 1u) == (unsigned)(kRedBlocks - 1);
    }
    __syncthreads();
    if (!last || threadIdx.x >= 64) return;
    for (int q = 0; q < nred; ++q) { // the workgroups ran on different XCDs (L2s): agent-scope atomic loads bypass the caches
        const double v = threadIdx.x < kRedBlocks ? __hip_atomic_load(stage + q * kRedBlocks + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.;
        const double t = wave_sum(v); // one load per lane, fixed summation tree: independent of the arrival order
        if (threadIdx.x == 0) sc->red[red_off + q] = t;
    }
    if (threadIdx.x != 0) return;
    *ticket = 0u;
    if (op != OP_NONE) apply_scalar_op(sc, op, tol);
}

__global__ void k_scalar(PcgScalars *sc, int op, double tol)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) apply_scalar_op(sc, op, tol);
}

// two partial sets in one launch (multi-GPU loop: its iterations are launch-bound, every launch saved counts):
// red[0 .. nredA) from A, red[nredA .. nredA + nredB) from B
__global__ __launch_bounds__(kRedBlock) void k_reduce_pair(const double *__restrict__ pa, int nba, int nreda, const double *__restrict__ pb,
                                                          int nbb, int nredb, PcgScalars *sc)
{
    __shared__ double red[kRedBlock / 64];
    for (int q = 0; q < nreda + nredb; ++q) {
        const bool first = q < nreda;
        const int nb = first ? nba : nbb;
        const double *src = first ? pa + (size_t)q * nba : pb + (size_t)(q - nreda) * nbb;
        double s0 = 0., s1 = 0., s2 = 0., s3 = 0.;
        int i = threadIdx.x;
        for (; i + 3 * kRedBlock < nb; i += 4 * kRedBlock) {
            const double a = src[i], b = src[i + kRedBlock], c = src[i + 2 * kRedBlock], d = src[i + 3 * kRedBlock];
            s0 += a; s1 += b; s2 += c; s3 += d;
        }
        for (; i < nb; i += kRedBlock) s0 += src[i];
        double s = wave_sum((s0 + s1) + (s2 + s3));
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.;
#pragma unroll
            for (int w = 0; w < kRedBlock / 64; ++w) t += red[w];
            sc->red[q] = t;
        }
    }
}

static void reduce_launch(PcgWork *w, const double *partial, int nb, int nred, PcgScalars *sc, int op, double tol, int skip_if_done,
                          int red_off, hipStream_t stream)
{
    if (nb >= 16384 && w->stage.p && w->ticket.p)
        hipLaunchKernelGGL(k_reduce_mb, dim3(kRedBlocks), dim3(kRedBlock), 0, stream, partial, nb, nred, sc, op, tol, skip_if_done, red_off,
                           w->stage.p, w->ticket.p);
    else
        hipLaunchKernelGGL(k_reduce, dim3(1), dim3(kRedBlock), 0, stream, partial, nb, nred, sc, op, tol, skip_if_done, red_off);
}

static avs_status reduce_stage(PcgWork *w, int nb, int nred, int op, double tol, int skip_if_done,
                               hipStream_t stream, PcgDist *dist)
{
    if (!dist) {
        reduce_launch(w, w->partial.p, nb, nred, w->sc.p, op, tol, skip_if_done, 0, stream);
    } else {
        // local sums -> RCCL all-reduce of sc->red[0..nred) -> scalar update
        reduce_launch(w, w->partial.p, nb, nred, w->sc.p, (int)OP_NONE, tol, 0, 0, stream);
        AVS_TRY(dist_allreduce(dist, reinterpret_cast<double *>(reinterpret_cast<char *>(w->sc.p) + offsetof(PcgScalars, red)), nred, stream));
        hipLaunchKernelGGL(k_scalar, dim3(1), dim3(64), 0, stream, w->sc.p, op, tol);
    }
    AVS_HIP(hipGetLastError());
    return AVS_OK;
}

// ---------------------------------------------------------------------------------------------
// Host side shared by the solve loops.  Every chunked loop has the same shape:
//   for (;;) { poll_scalars; sample_spmv; done / max_iters / cancel -> break; enqueue_chunk; }   then finish_info
// One body per loop, the precisions as template arguments: pcg_solve_phases<T, MIXED> (single GPU and the RCCL standard-CG path; the
// table in front of it lists what differs between fp64, float and mixed), pcg_solve_single_reduction<T, MIXED>, pcg_solve_direct<T, MIXED>.
// ---------------------------------------------------------------------------------------------
// Run-time flags -> template arguments: with_flags(f, a, b, ..) calls f(std::bool_constant<a>{}, std::bool_constant<b>{}, ..), so that a
// generic lambda names the instantiation once -- k<C.value, K.value> -- instead of one launch per branch of an if-ladder.  Plain
// branches, inlined: nothing per launch.  A combination that must not exist is folded inside the lambda (k_sr_update<T, F32 && C.value>).
template <typename F> static auto with_flags(F &&f) { return f(); }
template <typename F, typename... Bs> static auto with_flags(F &&f, bool b, Bs... rest)
{
    if (b) return with_flags([&](auto... c) { return f(std::true_type{}, c...); }, rest...);
    return with_flags([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}

// one dictionary of few values: the vector kernels read the rows' 2-B diagonal codes and the table of inverted values instead of one
// inverse per row (tile-local codes are not indices into one table)
static bool diag_coded(const CsrView &A) { return A.codes && !A.tab_ptr && A.table_size <= kViLdsTable; }

// doubles of partial sums a launch-per-phase loop needs when its SpMV leaves up to `nb`: the SpMV's in the lower half, the vector
// kernels' in the upper one (they are written while the SpMV's are still being read)
static size_t phase_partials(size_t nb) { return 2 * (nb + 16) + 4 * (size_t)kVecGrid + 16; }

// partial sums of the float product (spmv_f32_dispatch; mixed: spmv_mixed_dispatch): one per persistent workgroup of the brick kernel,
// else one per 256 rows of the streaming kernel
static size_t f32_spmv_partials(const CsrView &A, bool mixed)
{
    if (!(A.brick && A.brick->ntiles > 0 && A.brick->pwords32)) return (size_t)stream_grid(A.n);
    return (size_t)(mixed ? brick_partial_count_mixed(*A.brick) : brick_partial_count(*A.brick, 4));
}

static int vec_grid(int64_t n) // grid-stride vector kernels
{
    const int64_t g = (n + kBlock - 1) / kBlock;
    return (int)(g < 1 ? 1 : (g < kVecGrid ? g : kVecGrid));
}
static int row_grid(int64_t n) // one thread per row
{
    const int64_t g = (n + kBlock - 1) / kBlock;
    return (int)(g < 1 ? 1 : g);
}

static void drop_graph(PcgWork *w)
{
    if (w->graph) (void)hipGraphExecDestroy(w->graph);
    w->graph = nullptr;
}

// the partial-sum buffer holds at least `need` doubles (a captured chunk holds the old buffer's address: it goes with it)
static avs_status ensure_partials(PcgWork *w, size_t need)
{
    if (need <= w->npartial) return AVS_OK;
    AVS_TRY(w->partial.alloc(need));
    w->npartial = need;
    drop_graph(w);
    return AVS_OK;
}

// The inverse of the diagonal as the loops on vectors of T read it.  For a `coded` matrix (diag_coded(A): one dictionary of few values;
// never with tile-local tables) the rows' 2-B diagonal codes and the table of inverted values, else one inverse per row.
// *inv: what the vector kernels index -- by dcode[i] (coded) or by i.  fp64: w->invd is filled either way (the set-ups read it per row).
template <typename T>
static avs_status prepare_diagonal(PcgWork *w, const CsrView &A, bool coded, T **inv, const uint16_t **dcode, hipStream_t stream)
{
    constexpr bool F32 = std::is_same<T, float>::value;
    const int64_t n = A.n;
    if constexpr (!F32) hipLaunchKernelGGL(k_inv_diag<double>, dim3(row_grid(n)), dim3(kBlock), 0, stream, A, w->invd.p);
    if (coded) {
        if (!w->dcode.p) AVS_TRY(w->dcode.alloc((size_t)n + 8)); // (+ 8: the float loop's vector loads)
        if (!w->invtab.p) AVS_TRY(w->invtab.alloc((size_t)kViLdsTable + 1));
        const int cg = (int)(((n > A.table_size + 1 ? n : A.table_size + 1) + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(k_inv_diag_coded, dim3(cg), dim3(kBlock), 0, stream, A, w->dcode.p, w->invtab.p);
    }
    if constexpr (F32) {
        if (coded) {
            AVS_TRY(w->f_invtab.alloc((size_t)kViLdsTable + 1));
            hipLaunchKernelGGL(k_f32_invtab, dim3((A.table_size + kBlock) / kBlock), dim3(kBlock), 0, stream, A, w->f_invtab.p);
        } else {
            AVS_TRY(w->f_invd.alloc((size_t)n + 8));
            hipLaunchKernelGGL(k_inv_diag<float>, dim3(row_grid(n)), dim3(kBlock), 0, stream, A, w->f_invd.p);
        }
        *inv = coded ? w->f_invtab.p : w->f_invd.p;
    } else {
        *inv = coded ? w->invtab.p : w->invd.p;
    }
    *dcode = coded ? w->dcode.p : nullptr;
    return AVS_OK;
}

// the key fields every graph-replaying loop shares; the loop adds its own
static GraphKey matrix_key(GraphLoop loop, const CsrView &A, const void *x, double tol)
{
    GraphKey k;
    k.loop = loop;
    k.row_ptr = A.row_ptr;
    k.col = A.col;
    k.codes = A.codes;
    k.packed = A.packed;
    k.table = A.table;
    k.x = x;
    k.n = A.n;
    k.table_size = A.table_size;
    k.col_bits = A.col_bits;
    k.epoch = A.epoch;
    k.tol = tol;
    return k;
}

struct ChunkState {
    int enqueued = 0, last = 0; // iterations enqueued so far / by the last chunk
    bool timed = true;          // the last chunk was enqueued launch by launch: its SpMV events were recorded
    double spmv_ms_sum = 0.;
    int spmv_samples = 0;
};

// host_sc := the scalar state `slot`, once everything enqueued so far has run
static avs_status poll_scalars(PcgWork *w, const PcgScalars *slot, hipStream_t stream)
{
    AVS_HIP(hipMemcpyAsync(w->host_sc, slot, sizeof(PcgScalars), hipMemcpyDeviceToHost, stream));
    AVS_HIP(hipStreamSynchronize(stream));
    return AVS_OK;
}

// Adds the SpMV timing samples of the last chunk's launches that really ran: iterations 0 .. iter, plus the one that stopped the loop
// when it ran too -- done == 1 or 2 in the standard loops, any done != 0 in the single-reduction ones (`any_done`).
static void sample_spmv(PcgWork *w, bool sample, bool any_done, ChunkState *cs)
{
    if (!sample || cs->last == 0 || !cs->timed) return;
    const int done = w->host_sc->done;
    const int ran = w->host_sc->iter + ((any_done ? done != 0 : (done == 1 || done == 2)) ? 1 : 0);
    const int first = cs->enqueued - cs->last;
    for (int c = 0; c < cs->last && first + c < ran; c += kSampleEvery) {
        float ems = 0.f;
        if (hipEventElapsedTime(&ems, w->evA[c], w->evB[c]) == hipSuccess) {
            cs->spmv_ms_sum += ems;
            ++cs->spmv_samples;
        }
    }
}

// Enqueues the next chunk: kChunk iterations (fewer only at max_iters), iteration c by enqueue_iteration(c, timed).  With a `key`
// (nullptr: never a graph), full chunks replay one captured hipGraph -- recaptured when the key changes -- except every
// kTimedChunkEvery-th, which is enqueued launch by launch with the SpMV timing events so that the samples cover the whole solve.
// No per-launch host work in a replay: smaller gaps between the short kernels of small systems.  Kernels past convergence exit at
// once, so enqueueing a whole chunk is always safe.
template <typename F>
static avs_status enqueue_chunk(PcgWork *w, hipStream_t stream, const GraphKey *key, int max_iters, bool sample, F &&enqueue_iteration,
                                ChunkState *cs)
{
    const int chunk = (max_iters - cs->enqueued) < kChunk ? (max_iters - cs->enqueued) : kChunk;
    const bool replay = key && (cs->enqueued / kChunk) % kTimedChunkEvery != 0 && chunk == kChunk && !w->graph_broken;
    if (replay && w->graph && !(w->graph_key == *key)) drop_graph(w);
    if (replay && !w->graph) {
        hipGraph_t gr = nullptr;
        bool ok = hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed) == hipSuccess;
        if (ok) {
#ifdef AVS_PROBES
            tl_phase_capturing = true;
#endif
            for (int c = 0; c < kChunk && ok; ++c) ok = enqueue_iteration(c, false) == AVS_OK;
#ifdef AVS_PROBES
            tl_phase_capturing = false;
#endif
            ok = (hipStreamEndCapture(stream, &gr) == hipSuccess) && ok && gr;
        }
        if (ok) ok = hipGraphInstantiate(&w->graph, gr, nullptr, nullptr, 0) == hipSuccess;
        if (gr) (void)hipGraphDestroy(gr);
        if (ok) {
            w->graph_key = *key;
#ifdef AVS_PROBES
            tl_phase_report.graphs_captured++;
#endif
        } else { // plain launches for the rest of this workspace's life
            (void)hipGetLastError();
            w->graph = nullptr;
            w->graph_broken = true;
        }
    }
    cs->timed = !(replay && w->graph);
    if (cs->timed) {
        for (int c = 0; c < chunk; ++c) AVS_TRY(enqueue_iteration(c, sample && (c % kSampleEvery == 0)));
    } else {
        AVS_HIP(hipGraphLaunch(w->graph, stream));
    }
    AVS_HIP(hipGetLastError());
#ifdef AVS_PROBES
    if (cs->timed) {
        tl_phase_report.chunks_launched++;
    } else { // (its iterations: as the launch-by-launch chunk before it counted its own)
        tl_phase_report.chunks_replayed++;
        if (tl_phase_folded) tl_phase_report.alpha_folded += kChunk;
        else tl_phase_report.alpha_launched += kChunk;
    }
    tl_phase_report.graph_broken = w->graph_broken ? 1 : 0;
#endif
    cs->enqueued += chunk;
    cs->last = chunk;
    return AVS_OK;
}

// The end of every loop: ev1 recorded and waited for (solve_ms: ev0 -> ev1), then *info from the polled state.  cs: the loop's SpMV
// samples (nullptr: spmv_ms = 0).  f32: the relative error as the float loop computes it.
static avs_status finish_info(PcgWork *w, const CsrView &A, hipStream_t stream, avs_solve_info *info, const ChunkState *cs, bool cancelled,
                              int resident, bool f32)
{
    AVS_HIP(hipEventRecord(w->ev1, stream));
    AVS_HIP(hipEventSynchronize(w->ev1));
    float ms = 0.f;
    AVS_HIP(hipEventElapsedTime(&ms, w->ev0, w->ev1));
    const float void_ms = w->fused_void_ms;
    w->fused_void_ms = 0.f;
    if (!info) return AVS_OK;
    const PcgScalars &h = *w->host_sc;
    info->iterations = h.iter;
    info->converged = (h.done != 0 && !cancelled) ? 1 : 0;
    info->rhs_norm2 = h.rhs_norm2;
    if (h.done == 3 || h.rhs_norm2 == 0.) info->error = 0.;
    else info->error = f32 ? (double)sqrtf((float)h.rr / (float)h.rhs_norm2) : sqrt(h.rr / h.rhs_norm2);
    info->n = A.n;
    info->nnz = A.nnz;
    info->solve_ms = ms + void_ms; // (a redo behind a timed-out fused launch: the voided attempt counts)
    info->spmv_ms = (cs && cs->spmv_samples) ? cs->spmv_ms_sum / cs->spmv_samples : 0.;
    info->resident = resident;
    info->cancelled = cancelled ? 1 : 0;
    return AVS_OK;
}


#include "avs_pcg_f32.inl"
#include "avs_pcg_mixed.inl"

// ---------------------------------------------------------------------------------------------
// Single-reduction PCG (Chronopoulos & Gear 1989) -- used when the solve is partitioned over several
// GPUs: the same Krylov iterates in exact arithmetic, but gamma = r.u, delta = w.u and |r|^2 are
// all-reduced together, so an iteration has ONE all-reduce and ONE halo exchange (of u = M^-1 r)
// instead of two all-reduces + one exchange.  Costs one more vector (s = A p by recurrence): 12 n
// doubles of vector traffic instead of 10 n -- irrelevant once the solve is latency-bound.
//   u = M^-1 r ; w = A u ; p = u + beta p ; s = w + beta s ; x += alpha p ; r -= alpha s
// T, the vector type: double, or float for partitioned AVS_PRECISION_F32 solves (AVS_OPTION_DIST_F32_VECTORS = 1), which get the
// arithmetic of the single-GPU float loop (avs_pcg_f32.inl) over both transports:
//   * x, r, p, s, w, u [owned | halo] and the inverse diagonal are float arrays;
//   * sums: a thread's own terms in T, everything across threads and workgroups in double, across ranks in double in rank order
//     (the finalizer of the direct transport / the all-reduce) -- every rank computes bit-identical scalars;
//   * the scalar step (OP_SR_INIT_F32, OP_SR_STEP_F32, sr_step<float>) rounds the all-reduced sums to float and computes alpha, beta
//     and the threshold in float;
//   * the SpMV is the single-GPU float loop's (spmv_f32_dispatch);
//   * halo entries travel as doubles (widened floats: exact) -- the direct transport's comm block, 8-B slots, self-test and checksums,
//     and the RCCL / in-process exchange's buffers stay as they are.
// What stays fp64: AVS_DIST_CG=standard and paranoid mode (the CU-resident loop between ranks: with AVS_OPTION_RESIDENT_F32 only).
// CODED (float vectors only): the rows' 2-B diagonal codes and the table of inverted values instead of one inverse per row.
// ---------------------------------------------------------------------------------------------
// r = b - t, u = M^-1 r ; partials [0..g) b.b, [g..2g) r.u, [2g..3g) r.r
template <typename T, bool CODED>
__global__ __launch_bounds__(kBlock) void k_sr_init(int64_t n, const double *__restrict__ b, const T *__restrict__ t,
                                                    const T *__restrict__ invd, const uint16_t *__restrict__ dcode, T *__restrict__ r,
                                                    T *__restrict__ u, double *__restrict__ partial)
{
    __shared__ double red[4];
    T bb = 0, ru = 0, rr = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const T bi = (T)b[i]; // (float: b holds float values)
        const T ri = bi - t[i];
        const T ui = (CODED ? invd[dcode[i]] : invd[i]) * ri;
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

// The scalar step of the previous iteration (OP_SR_STEP / OP_SR_STEP_F32 on the all-reduced sums) is folded into the start of this
// kernel when `step` is set: every workgroup computes the same new scalars from state `in`, workgroup 0 stores them as
// state `out` (a different PcgScalars: nobody reads what is being written) -- one launch less per iteration of a loop
// that is launch-bound at 8 GPUs.  in == out and step == 0: scalars are used as they are.
//   p = u + beta p, s = w + beta s, x += alpha p, r -= alpha s, u = M^-1 r ; partials r.u, r.r
// S, the scalar type: T, or double next to T = float (the mixed-precision loops, AVS_OPTION_DIST_MIXED_PRECISION): the step is
// sr_step<double>, every dot term is widened before it is multiplied, and x is the correction xf.
template <typename T, bool CODED, typename S = T>
__global__ __launch_bounds__(kBlock) void k_sr_update(int64_t n, T *__restrict__ x, T *__restrict__ r, T *__restrict__ p,
                                                      T *__restrict__ s, T *__restrict__ u, const T *__restrict__ w,
                                                      const T *__restrict__ invd, const uint16_t *__restrict__ dcode,
                                                      const PcgScalars *in, PcgScalars *out, int step, double *__restrict__ partial)
{
    int done = in->done;
    double alpha = in->alpha, beta = in->beta;
    if (step) {
        double rr = in->rr, rho = in->rho;
        int iter = in->iter;
        sr_step<S>(in, rr, rho, alpha, beta, iter, done);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            PcgScalars o = *in;
            o.rr = rr; o.rho = rho; o.alpha = alpha; o.beta = beta; o.iter = iter; o.done = done;
            *out = o;
        }
    }
    if (done) return; // (rhs == 0, done == 3: the host zeroes x)
    const T a = (T)alpha, bt = (T)beta;
    __shared__ double red[4];
    S ru = 0, rr = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const T pi = u[i] + bt * p[i];
        const T si = w[i] + bt * s[i];
        p[i] = pi;
        s[i] = si;
        x[i] += a * pi;
        const T ri = r[i] - a * si;
        r[i] = ri;
        const T ui = (CODED ? invd[dcode[i]] : invd[i]) * ri;
        u[i] = ui;
        ru += (S)ri * (S)ui;
        rr += (S)ri * (S)ri;
    }
    const double su = block_sum((double)ru, red);
    const double sr = block_sum((double)rr, red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = su;
        partial[gridDim.x + blockIdx.x] = sr;
    }
}

// The mixed-precision form of the two loops (AVS_OPTION_DIST_MIXED_PRECISION; the scheme of avs_pcg_mixed.inl on the single-reduction
// iteration): r, u, w, p, s and the correction xf are float, x, b, the matrix values, every row sum, every dot product and the scalars
// stay fp64.  The reliable update runs behind every chunk, outside the captured graph: x += xf (k_mixed_fold), x exchanged in fp64,
// t64 = A x with the rank's fp64 product, the kernel below, u exchanged, w = A u with w.u, and the Chronopoulos-Gear step on the TRUE
// residual's sums (k_sr_mixed_step) IN PLACE OF the step of the chunk's last iteration -- which is therefore never taken on the
// recurrence's sums: the RCCL loop drops its explicit k_scalar behind the chunk, the last round of a chunk of the direct loop folds its
// sums with OP_NONE.  A chunk the recurrence froze (its r.r passed the threshold) left rho and alpha of the step it did not take: the
// same update either confirms the claim on the fp64 residual or takes that step.
//
// r64 = b - t64 ; r = (float) r64 ; u = D^-1 r (stored: the next product's input).  partials: [0..g) r.u of the ROUNDED residual,
// [g..2g) |r64|^2; INIT: [0..g) b.b, [g..2g) r.u, [2g..3g) |r64|^2 -- the layouts OP_SR_STEP / OP_SR_INIT read.  All sums in double.
template <bool CODED, bool INIT>
__global__ __launch_bounds__(kBlock) void k_sr_mixed_residual(int64_t n, const double *__restrict__ b, const double *__restrict__ t64,
                                                              float *__restrict__ r, float *__restrict__ u, const float *__restrict__ invd,
                                                              const uint16_t *__restrict__ dcode, double *__restrict__ partial,
                                                              const PcgScalars *sc)
{
    __shared__ double red[4];
    // done == 3, a transport fault: k_sr_mixed_begin left it set, and k_sr_mixed_step will not read the sums -- as k_sr_update, the launch
    // leaves the vectors AND the partial sums as they are (it used to store zero sums)
    if (!INIT && sc->done != 0) return;
    double rr = 0., ru = 0., bb = 0.;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const double bi = b[i];
        const double ri = bi - t64[i];
        const float rf = (float)ri;
        const float ui = (CODED ? invd[dcode[i]] : invd[i]) * rf;
        r[i] = rf;
        u[i] = ui;
        rr += ri * ri;
        ru += (double)rf * (double)ui;
        if (INIT) bb += bi * bi;
    }
    rr = block_sum(rr, red);
    ru = block_sum(ru, red);
    if (INIT) bb = block_sum(bb, red);
    if (threadIdx.x == 0) {
        if (INIT) partial[blockIdx.x] = bb;
        partial[(INIT ? 1 : 0) * gridDim.x + blockIdx.x] = ru;
        partial[(INIT ? 2 : 1) * gridDim.x + blockIdx.x] = rr;
    }
}

// In front of a reliable update: the kernels of its two exchanges return while `done` is set, and a chunk the recurrence froze (or an
// avs_cancel the direct transport's finalizer saw: sc->cancelled stays) left it set.  rhs == 0 and a transport fault keep it.
__global__ void k_sr_mixed_begin(PcgScalars *sc)
{
    if (sc->done == 3 || sc->fault) return;
    sc->done = 0;
}

// The scalar step of a reliable update on red = [r.u, |r64|^2, w.u] of the true residual (all-reduced / all-gathered in rank order):
// the fp64 test, else OP_SR_STEP's arithmetic from rho and alpha of the last step taken; the iteration counts once, here.
__global__ void k_sr_mixed_step(PcgScalars *sc)
{
    if (sc->done == 3 || sc->fault) return;
    sc->rr = sc->red[1];
    if (sc->cancelled || sc->red[1] < sc->threshold) { sc->done = 1; return; }
    const double gamma_old = sc->rho, gamma = sc->red[0], delta = sc->red[2];
    const double beta = gamma / gamma_old;
    sc->alpha = gamma / (delta - beta * gamma / sc->alpha);
    sc->beta = beta;
    sc->rho = gamma;
    sc->iter += 1;
    sc->done = 0;
}

// (k_sr_init / k_sr_update read diagonal codes in the float loops only: they are launched as KERNEL<T, F32 && CODED>, which keeps
// KERNEL<double, true> from being instantiated)
// The vectors of a single-reduction loop: fp64 -- the workspace's own (x: the caller's), float -- the f_* arrays (x narrowed)
template <typename T> struct SrVecs {
    T *x, *r, *p, *s, *w, *u;  // w = A u; u [owned | halo]
    const T *invd;             // one inverse per row (float and coded: nullptr)
    const T *invtab;           // coded: the table of inverted values, indexed by dcode (else nullptr)
    const uint16_t *dcode;
};

// the SpMV of the set-up and of the RCCL loop: the fp64 launcher (avs_spmv.hip; !DOT: partial is nullptr), or the float loop's
template <bool DOT>
static avs_status sr_spmv(const CsrView &A, const double *x, double *y, double *partial, const PcgScalars *sc, int variant,
                          hipStream_t stream, int *nb)
{
    return spmv_dot_launch(A, x, y, DOT ? partial : nullptr, variant, stream, sc, nb);
}
template <bool DOT>
static avs_status sr_spmv(const CsrView &A, const float *x, float *y, double *partial, const PcgScalars *sc, int, hipStream_t stream, int *nb)
{
    return spmv_f32_dispatch<DOT>(A, x, y, partial, sc, stream, nb);
}

// Set-up of the single-reduction loops: the vectors, zeroed recurrences, both scalar states and the diagonal (a `coded` matrix also
// gets the rows' codes and the table of inverted values), then r = b - A x (x staged through u for the halo), u = M^-1 r, w = A u.
// product(k): the transport's exchange of u and w = A u -- k = 0 of x, k = 1 of u, which also folds the sums |b|^2, r.u, |r|^2, w.u
// (the first 3 * g vector partials) and applies OP_SR_INIT / OP_SR_INIT_F32 in sc[0].  g: the grid of the loop's vector kernels.
// MIXED (T = float): v->x is the correction xf = 0; product(0) stages x through w->p [owned | halo] and leaves the fp64 A x in w->t;
// the sums are |b|^2, r.u of the rounded residual and |b - A x|^2 of the fp64 one.
template <typename T, bool MIXED = false, typename F>
static avs_status sr_setup(PcgWork *w, const CsrView &A, const double *b, double *x, bool coded, int g, SrVecs<T> *v, hipStream_t stream,
                           F &&product)
{
    constexpr bool F32 = std::is_same<T, float>::value;
    static_assert(F32 || !MIXED, "the mixed-precision loops iterate on float vectors");
    const int64_t n = A.n;
    AVS_HIP(hipMemsetAsync(w->sc.p, 0, 2 * sizeof(PcgScalars), stream));
    if constexpr (F32) { // as pcg_solve_phases<float> makes them
        const size_t na = (size_t)n + 8, ne = (size_t)w->n_ext + 8;
        AVS_TRY(w->f_x.alloc(na)); AVS_TRY(w->f_r.alloc(na)); AVS_TRY(w->f_p.alloc(na)); AVS_TRY(w->f_s.alloc(na)); AVS_TRY(w->f_t.alloc(na));
        AVS_TRY(w->f_u.alloc(ne));
        AVS_HIP(hipMemsetAsync(w->f_p.p, 0, na * sizeof(float), stream));
        AVS_HIP(hipMemsetAsync(w->f_s.p, 0, na * sizeof(float), stream));
        *v = {w->f_x.p, w->f_r.p, w->f_p.p, w->f_s.p, w->f_t.p, w->f_u.p, nullptr, nullptr, nullptr};
        w->float_vectors = 1;
    } else {
        AVS_TRY(w->s.alloc((size_t)n));
        AVS_TRY(w->u.alloc((size_t)w->n_ext));
        AVS_HIP(hipMemsetAsync(w->p.p, 0, (size_t)w->n_ext * sizeof(double), stream));
        AVS_HIP(hipMemsetAsync(w->s.p, 0, (size_t)n * sizeof(double), stream));
        *v = {x, w->r.p, w->p.p, w->s.p, w->t.p, w->u.p, nullptr, nullptr, nullptr};
    }
    {
        T *inv = nullptr;
        AVS_TRY(prepare_diagonal<T>(w, A, coded, &inv, &v->dcode, stream));
        v->invtab = coded ? inv : nullptr;
        if constexpr (F32) v->invd = coded ? nullptr : inv;
        else v->invd = w->invd.p; // (the fp64 set-up reads the per-row inverse of a coded matrix too)
    }
    AVS_HIP(hipEventRecord(w->ev0, stream));
    if constexpr (MIXED) {
        AVS_HIP(hipMemsetAsync(v->x, 0, ((size_t)n + 8) * sizeof(float), stream));
        AVS_HIP(hipMemcpyAsync(w->p.p, x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream));
    } else if constexpr (F32) {
        hipLaunchKernelGGL(k_f32_narrow, dim3(g), dim3(kBlock), 0, stream, n, (const double *)x, v->x);
        hipLaunchKernelGGL(k_f32_narrow, dim3(g), dim3(kBlock), 0, stream, n, (const double *)x, v->u);
    } else {
        AVS_HIP(hipMemcpyAsync(v->u, x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream));
    }
    AVS_TRY(product(0));
    const bool kc = F32 && coded; // (the fp64 set-up reads the per-row inverse)
    with_flags([&](auto C) {
        if constexpr (MIXED)
            hipLaunchKernelGGL((k_sr_mixed_residual<C.value, true>), dim3(g), dim3(kBlock), 0, stream, n, b, (const double *)w->t.p, v->r, v->u,
                               kc ? v->invtab : v->invd, v->dcode, w->partial.p, (const PcgScalars *)w->sc.p);
        else
            hipLaunchKernelGGL((k_sr_init<T, F32 && C.value>), dim3(g), dim3(kBlock), 0, stream, n, b, (const T *)v->w, kc ? v->invtab : v->invd,
                               v->dcode, v->r, v->u, w->partial.p);
    }, kc);
    AVS_TRY(product(1));
    AVS_HIP(hipGetLastError());
    return AVS_OK;
}

// sr_setup over the RCCL / in-process exchange; dist == nullptr: one GPU, no exchange and no all-reduce
template <typename T, bool MIXED = false>
static avs_status sr_setup_exchange(PcgWork *w, const CsrView &A, const double *b, double *x, double tol, bool coded, PcgDist *dist,
                                    SrVecs<T> *v, hipStream_t stream)
{
    const int g = vec_grid(A.n);
    const int variant = spmv_default_variant(A);
    double *pvec = w->partial.p, *pspmv = w->partial.p + 4 * (size_t)kVecGrid; // 3 * g vector-kernel partials, the SpMV's behind them
    PcgScalars *sc = w->sc.p;
    return sr_setup<T, MIXED>(w, A, b, x, coded, g, v, stream, [&](int k) -> avs_status {
        if constexpr (MIXED) {
            if (k == 0) { // x exchanged in fp64, then the rank's fp64 product (as in the reliable updates)
                if (dist) AVS_TRY(dist_halo_exchange(dist, w->p.p, stream));
                return spmv_launch(A, w->p.p, w->t.p, variant, stream);
            }
        }
        if (dist) AVS_TRY(dist_halo_exchange(dist, v->u, stream));
        if (k == 0) return sr_spmv<false>(A, v->u, v->w, nullptr, nullptr, variant, stream, nullptr);
        int nb = 0;
        if constexpr (MIXED) AVS_TRY(spmv_mixed_dispatch<true>(A, v->u, v->w, pspmv, nullptr, stream, &nb));
        else AVS_TRY(sr_spmv<true>(A, v->u, v->w, pspmv, nullptr, variant, stream, &nb));
        reduce_launch(w, pvec, g, 3, sc, (int)OP_NONE, tol, 0, 0, stream);
        reduce_launch(w, pspmv, nb, 1, sc, (int)OP_NONE, tol, 0, 3, stream);
        if (dist) AVS_TRY(dist_allreduce(dist, sc->red, 4, stream));
        hipLaunchKernelGGL(k_scalar, dim3(1), dim3(64), 0, stream, sc, (std::is_same<T, float>::value && !MIXED) ? (int)OP_SR_INIT_F32 : (int)OP_SR_INIT, tol);
        return AVS_OK;
    });
}

// Host-mediated transports (RCCL, in-process virtual ranks).  b, x: the rank's fp64 arrays (float vectors: holding float values); x
// receives the solution.
// MIXED (T = float, AVS_OPTION_DIST_MIXED_PRECISION): x stays fp64 and receives the reliable updates (see k_sr_mixed_residual).
template <typename T, bool MIXED = false>
static avs_status pcg_solve_single_reduction(PcgWork *w, const CsrView &A, const double *b, double *x, double tol,
                                             int max_iters, hipStream_t stream, avs_solve_info *info, PcgDist *dist)
{
    constexpr bool F32 = std::is_same<T, float>::value;
    typedef typename std::conditional<MIXED, double, T>::type SS; // the scalar type of the update kernel
    const int64_t n = A.n;
    const int g = vec_grid(n);
    const int variant = spmv_default_variant(A);
    const bool coded = F32 && diag_coded(A); // (the fp64 loop reads the per-row inverse)
    if (F32) AVS_TRY(ensure_partials(w, 4 * (size_t)kVecGrid + f32_spmv_partials(A, MIXED) + 16)); // (the float SpMV's behind the vector kernels')
    SrVecs<T> v;
    AVS_TRY((sr_setup_exchange<T, MIXED>(w, A, b, x, tol, coded, dist, &v, stream)));
    double *pvec = w->partial.p;                        // 3 * g vector-kernel partials
    double *pspmv = w->partial.p + 4 * (size_t)kVecGrid; // SpMV partials behind them
    PcgScalars *sc = w->sc.p; // two states, ping-pong: sc[cur] is current, k_sr_update writes sc[cur ^ 1]
    int cur = 0;

    auto enqueue_iteration = [&](int c, bool timed) -> avs_status {
        // first iteration of a chunk: scalars are final (SR_INIT or the explicit step after the chunk); afterwards the step of
        // the previous iteration rides in k_sr_update, which moves the state to the other slot
        const int step = c > 0 ? 1 : 0;
        with_flags([&](auto C) {
            hipLaunchKernelGGL((k_sr_update<T, F32 && C.value, SS>), dim3(g), dim3(kBlock), 0, stream, n, v.x, v.r, v.p, v.s, v.u, (const T *)v.w,
                               coded ? v.invtab : v.invd, v.dcode, (const PcgScalars *)(sc + cur), sc + (step ? (cur ^ 1) : cur), step, pvec);
        }, coded);
        if (step) cur ^= 1;
        const PcgScalars *now = sc + cur;
        int nb = 0;
        bool overlapped = false;
        if constexpr (!F32) {
            const int32_t *t_int = nullptr, *t_bnd = nullptr;
            int n_int = 0, n_bnd = 0;
            if (variant == 24 && !(A.brick && A.brick->ntiles > 0) && dist_tile_lists(dist, &t_int, &n_int, &t_bnd, &n_bnd)) {
                // overlap: the exchange runs on the communication stream while the tiles that touch no halo
                // column are multiplied; the halo-touching tiles follow once the halo has landed
                AVS_TRY(dist_halo_begin(dist, v.u, stream));
                if (timed) AVS_HIP(hipEventRecord(w->evA[c], stream));
                AVS_TRY(spmv_dot_tiles(A, v.u, v.w, pspmv, now, t_int, n_int, stream));
                AVS_TRY(dist_halo_end(dist, stream));
                AVS_TRY(spmv_dot_tiles(A, v.u, v.w, pspmv + (size_t)n_int * (A.codes ? kTileRows / 64 : 1), now, t_bnd, n_bnd, stream));
                if (timed) AVS_HIP(hipEventRecord(w->evB[c], stream));
                nb = (n_int + n_bnd) * (A.codes ? kTileRows / 64 : 1); // value-indexed kernel: one partial per wave
                overlapped = true;
            }
        }
        if (!overlapped) {
            AVS_TRY(dist_halo_exchange(dist, v.u, stream));
            if (timed) AVS_HIP(hipEventRecord(w->evA[c], stream));
            if constexpr (MIXED) AVS_TRY(spmv_mixed_dispatch<true>(A, v.u, v.w, pspmv, now, stream, &nb));
            else AVS_TRY(sr_spmv<true>(A, v.u, v.w, pspmv, now, variant, stream, &nb));
            if (timed) AVS_HIP(hipEventRecord(w->evB[c], stream));
        }
        if (nb < 16384) hipLaunchKernelGGL(k_reduce_pair, dim3(1), dim3(kRedBlock), 0, stream, pvec, g, 2, pspmv, nb, 1, sc + cur);
        else {
            reduce_launch(w, pvec, g, 2, sc + cur, (int)OP_NONE, tol, 0, 0, stream);
            reduce_launch(w, pspmv, nb, 1, sc + cur, (int)OP_NONE, tol, 0, 2, stream);
        }
        return dist_allreduce(dist, sc[cur].red, 3, stream);
    };
    // MIXED: the reliable update behind every chunk, on sc[cur] (every rank enqueues it: the exchanges are collective)
    auto enqueue_update = [&]() -> avs_status {
        if constexpr (MIXED) {
            PcgScalars *now = sc + cur;
            hipLaunchKernelGGL(k_sr_mixed_begin, dim3(1), dim3(1), 0, stream, now);
            hipLaunchKernelGGL(k_mixed_fold, dim3(g), dim3(kBlock), 0, stream, n, x, v.x, (const PcgScalars *)now);
            AVS_HIP(hipMemcpyAsync(w->p.p, x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream));
            AVS_TRY(dist_halo_exchange(dist, w->p.p, stream));
            AVS_TRY(spmv_launch(A, w->p.p, w->t.p, variant, stream));
            with_flags([&](auto C) {
                hipLaunchKernelGGL((k_sr_mixed_residual<C.value, false>), dim3(g), dim3(kBlock), 0, stream, n, b, (const double *)w->t.p, v.r, v.u,
                                   coded ? v.invtab : v.invd, v.dcode, pvec, (const PcgScalars *)now);
            }, coded);
            AVS_TRY(dist_halo_exchange(dist, v.u, stream));
            int nb = 0;
            AVS_TRY(spmv_mixed_dispatch<true>(A, v.u, v.w, pspmv, now, stream, &nb));
            reduce_launch(w, pvec, g, 2, now, (int)OP_NONE, tol, 0, 0, stream);
            reduce_launch(w, pspmv, nb, 1, now, (int)OP_NONE, tol, 0, 2, stream);
            AVS_TRY(dist_allreduce(dist, now->red, 3, stream));
            hipLaunchKernelGGL(k_sr_mixed_step, dim3(1), dim3(1), 0, stream, now);
            AVS_HIP(hipGetLastError());
            w->reliable_updates++;
        }
        return AVS_OK;
    };
    ChunkState cs;
    bool cancelled = false;
    AVS_TRY(w->cancel_word.alloc(2));
    for (;;) {
        // avs_cancel: every rank contributes its request (0 / 1), the sum is the verdict of ALL ranks for this chunk boundary
        double stop_h[2] = {cancel_requested() ? 1. : 0., 0.};
        AVS_HIP(hipMemcpyAsync(w->cancel_word.p, stop_h, sizeof(double), hipMemcpyHostToDevice, stream));
        AVS_TRY(dist_allreduce(dist, w->cancel_word.p, 1, stream));
        AVS_HIP(hipMemcpyAsync(stop_h + 1, w->cancel_word.p, sizeof(double), hipMemcpyDeviceToHost, stream));
        AVS_TRY(poll_scalars(w, sc + cur, stream));
        sample_spmv(w, info != nullptr, true, &cs);
        if (MIXED && w->host_sc->done == 0 && w->host_sc->iter < cs.enqueued) cs.enqueued = w->host_sc->iter; // a chunk the recurrence froze
        if (w->host_sc->done || cs.enqueued >= max_iters) break;
        if (stop_h[1] != 0.) { (void)cancel_consume(); cancelled = true; break; }
        AVS_TRY(enqueue_chunk(w, stream, nullptr, max_iters, info != nullptr, enqueue_iteration, &cs)); // (no graph: RCCL calls inside)
        if constexpr (MIXED) {
            AVS_TRY(enqueue_update()); // x += xf and the step on the true residual before the host looks
        } else {
            // the last iteration's step, explicitly: the host polls a final state
            hipLaunchKernelGGL(k_scalar, dim3(1), dim3(64), 0, stream, sc + cur, F32 ? (int)OP_SR_STEP_F32 : (int)OP_SR_STEP, tol);
            AVS_HIP(hipGetLastError());
        }
    }
    if constexpr (MIXED) {
        if (w->host_sc->done == 3) AVS_HIP(hipMemsetAsync(x, 0, (size_t)n * sizeof(double), stream)); // rhs == 0: x := 0
        return finish_info(w, A, stream, info, &cs, cancelled, 0, false);
    }
    if (w->host_sc->done == 3) AVS_HIP(hipMemsetAsync(v.x, 0, (size_t)n * sizeof(T), stream)); // rhs == 0: x := 0
    if constexpr (F32) hipLaunchKernelGGL(k_f32_widen, dim3(g), dim3(kBlock), 0, stream, n, (const float *)v.x, x);
    AVS_HIP(hipGetLastError());
    return finish_info(w, A, stream, info, &cs, cancelled, 0, F32);
}

// ---------------------------------------------------------------------------------------------
// Direct-transport loop (world >= 1): the single-reduction iteration above with NO RCCL call and no host work inside:
//   k_sr_update_push  p, s, x, r, u + partials of r.u, |r|^2; then the boundary entries of u -> the peers' halo areas and the
//                     epoch flag (last pushing block).  (k_push does the same for the two set-up rounds.)
//   SpMV, all tiles   interior tiles run while the peers' entries travel; the tiles that read halo columns (the last ones) wait
//                     for the flags; every wave drops its x.Ax partial into a stage slot (fire and forget); the finalizer blocks
//                     (dispatched last) watch the slots, fold them, and the last one all-gathers the 3 sums with every rank and
//                     applies the scalar step
// = 2 launches per iteration, replayed from one hipGraph per chunk of kChunk iterations.
// ---------------------------------------------------------------------------------------------
void sr_update_geometry(long long n, int *grid, int *chunk)
{
    long long g = (n + kBlock - 1) / kBlock;
    if (g < 1) g = 1;
    if (g > kVecGrid) g = kVecGrid;
    long long c = (n + g - 1) / g;
    c = (c + kBlock - 1) / kBlock * kBlock;
    if (c < kBlock) c = kBlock;
    *chunk = (int)c;
    *grid = (int)((n + c - 1) / c > 0 ? (n + c - 1) / c : 1);
}

// One thread of every pushing workgroup, AFTER the workgroup's stores have been acknowledged (wait_own_stores + barrier): take a
// ticket; the last one raises this rank's flag in the blocks of the peers it feeds.  Paranoid mode: the round's checksums first,
// acknowledged, then the flags.
__device__ __forceinline__ void push_raise_flags(const DistDev *dd, const unsigned long long *epoch, unsigned *ticket, unsigned nblocks)
{
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t != nblocks - 1u) return;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int np = dd->npeers;
    const unsigned long long E = *epoch + 1ull;
    if (dd->paranoid) {
        for (int i = 0; i < np; ++i)
            if (dd->send_off[i + 1] > dd->send_off[i])
                st_sys(dd->peer_hsum_dst[i], __hip_atomic_exchange(dd->psum + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        wait_own_stores();
    }
    for (int i = 0; i < np; ++i)
        if (dd->send_off[i + 1] > dd->send_off[i]) st_sys(dd->peer_hflag_dst[i], E);
}

// k_sr_update + k_push in one launch: workgroup b owns a CONTIGUOUS range of rows, updates them, and then stores those of its
// new u entries that a peer reads straight into that peer's halo area; the last pushing workgroup raises the flags.
// CODED (round 3): the diagonal's 2-B value code + the table of inverted values instead of the 8-B inverse (11.25 n instead of
// 12 n doubles of vector traffic; the same doubles, so nothing changes numerically); u is recomputed from r instead of read (10.25 n).  Rows are taken two at a time with 16-B
// loads / stores (ranges start at multiples of the block size, so the pairs are aligned).
// KEEP == false (round 5: the brick-structured form is small enough to stay in the Infinity Cache between two products -- but only
// if the ~0.5 GB this kernel moves do not push it out): p, s, x, r -- read and written once per iteration, by this kernel only -- are
// loaded and stored non-temporally; u (the next product's input) and w (the product's output, read here) stay cacheable.
// T (round 7): the vector type -- double, or float for the float-vector loop of AVS_PRECISION_F32 partitioned solves (see the
// single-reduction section: a thread's own sums in float, everything across threads in double; the pushed entries are widened to double,
// which is exact, so the comm block, its 8-B slots and the checksums stay as they are).  Rows two at a time: 16-B (double) or 8-B (float) accesses.
template <typename T> struct Pair;
template <> struct Pair<double> { typedef d2_t type; };
template <> struct Pair<float> { typedef float type __attribute__((ext_vector_type(2))); };

// S = double next to T = float: the mixed-precision loop's instantiation, as k_sr_update<float, .., double> -- dot terms widened, x is
// the correction xf.
template <bool CODED, bool KEEP = true, typename T = double, typename S = T>
__global__ __launch_bounds__(kBlock) void k_sr_update_push(int64_t n, T *__restrict__ x, T *__restrict__ r, T *__restrict__ p,
                                                           T *__restrict__ s, T *__restrict__ u, const T *__restrict__ w,
                                                           const T *__restrict__ invd, const uint16_t *__restrict__ dcode,
                                                           const PcgScalars *sc, double *__restrict__ partial,
                                                           const DistDev *__restrict__ dd, const unsigned long long *__restrict__ epoch,
                                                           unsigned *__restrict__ ticket)
{
    const int done = sc->done;
    const int64_t lo = (int64_t)blockIdx.x * dd->push_chunk;
    const int64_t hi = (lo + dd->push_chunk < n) ? lo + dd->push_chunk : n;
    if (done == 3) {
        for (int64_t i = lo + threadIdx.x; i < hi; i += kBlock) x[i] = 0.;
        return;
    }
    if (done) return;
    typedef typename Pair<T>::type v2_t;
    const T alpha = (T)sc->alpha, beta = (T)sc->beta;
    __shared__ double red[4];
    S ru = 0, rr = 0;
    int64_t i = lo + 2 * (int64_t)threadIdx.x;
    for (; i + 1 < hi; i += 2 * kBlock) { // (lo is a multiple of kBlock: i is even, the 16-B accesses are aligned)
        const v2_t pv = stream_load_k<KEEP>(reinterpret_cast<const v2_t *>(p + i));
        const v2_t wv = *reinterpret_cast<const v2_t *>(w + i), sv = stream_load_k<KEEP>(reinterpret_cast<const v2_t *>(s + i));
        const v2_t xv = stream_load_k<KEEP>(reinterpret_cast<const v2_t *>(x + i)), rv = stream_load_k<KEEP>(reinterpret_cast<const v2_t *>(r + i));
        T id0, id1;
        if (CODED) {
            const unsigned cc = stream_load_k<KEEP>(reinterpret_cast<const unsigned *>(dcode + i));
            id0 = invd[cc & 0xffffu];
            id1 = invd[cc >> 16];
        } else {
            const v2_t iv = *reinterpret_cast<const v2_t *>(invd + i);
            id0 = iv.x;
            id1 = iv.y;
        }
        // u is not read: what memory holds is inv(d) * r of the r just loaded (this kernel, or the set-up round, wrote exactly that product)
        v2_t uv;
        uv.x = id0 * rv.x;
        uv.y = id1 * rv.y;
        v2_t pn, sn, xn, rn, un;
        pn.x = uv.x + beta * pv.x;  pn.y = uv.y + beta * pv.y;
        sn.x = wv.x + beta * sv.x;  sn.y = wv.y + beta * sv.y;
        xn.x = xv.x + alpha * pn.x; xn.y = xv.y + alpha * pn.y;
        rn.x = rv.x - alpha * sn.x; rn.y = rv.y - alpha * sn.y;
        un.x = id0 * rn.x;          un.y = id1 * rn.y;
        stream_store_k<KEEP>(pn, reinterpret_cast<v2_t *>(p + i));
        stream_store_k<KEEP>(sn, reinterpret_cast<v2_t *>(s + i));
        stream_store_k<KEEP>(xn, reinterpret_cast<v2_t *>(x + i));
        stream_store_k<KEEP>(rn, reinterpret_cast<v2_t *>(r + i));
        *reinterpret_cast<v2_t *>(u + i) = un;
        ru += (S)rn.x * (S)un.x;
        rr += (S)rn.x * (S)rn.x;
        ru += (S)rn.y * (S)un.y;
        rr += (S)rn.y * (S)rn.y;
    }
    if (i < hi) { // odd tail of the last range
        const T idi = CODED ? invd[dcode[i]] : invd[i];
        const T pi = idi * r[i] + beta * p[i]; // (u[i] == inv(d) r[i], see above)
        const T si = w[i] + beta * s[i];
        p[i] = pi;
        s[i] = si;
        x[i] += alpha * pi;
        const T ri = r[i] - alpha * si;
        r[i] = ri;
        const T ui = idi * ri;
        u[i] = ui;
        ru += (S)ri * (S)ui;
        rr += (S)ri * (S)ri;
    }
    const double sru = block_sum((double)ru, red); // (barriers inside: every u of this range is written before the push below reads it)
    const double srr = block_sum((double)rr, red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = sru;
        partial[gridDim.x + blockIdx.x] = srr;
    }
    const int np = dd->npeers, G = (int)gridDim.x, b = (int)blockIdx.x;
    const int paranoid = dd->paranoid;
    const bool inject = paranoid && dd->inject_stale_round == (long long)(*epoch + 1ull); // test hook: one entry is NOT stored
    bool any = false;
    for (int i = 0; i < np; ++i) {
        const int a = dd->push_seg[i * (G + 1) + b], e = dd->push_seg[i * (G + 1) + b + 1];
        double *dst = dd->peer_halo_dst[i] - dd->send_off[i];
        unsigned long long cs = 0ull;
        for (int j = a + (int)threadIdx.x; j < e; j += kBlock) {
            const double v = (double)u[dd->send_idx[j]];
            if (!(inject && j == 0)) __hip_atomic_store(dst + j, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            cs += (unsigned long long)__double_as_longlong(v);
        }
        if (paranoid && e > a) { // (block-uniform condition)
            cs = wave_sum_u64(cs);
            if ((threadIdx.x & 63) == 0 && cs) __hip_atomic_fetch_add(dd->psum + i, cs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        any = any || e > a;
    }
    if (!any) return; // block-uniform
    wait_own_stores();
    __syncthreads();
    if (threadIdx.x == 0) push_raise_flags(dd, epoch, ticket, (unsigned)dd->n_send_blocks);
}

__global__ __launch_bounds__(256) void k_push(const DistDev *__restrict__ dd, const double *__restrict__ v,
                                              const unsigned long long *__restrict__ epoch, unsigned *__restrict__ ticket,
                                              const PcgScalars *sc)
{
    if (sc->done) return;
    const int np = dd->npeers;
    const int n_send = dd->send_off[np];
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int paranoid = dd->paranoid;
    const unsigned long long E = *epoch + 1ull;
    int mine = -1;
    unsigned long long bits = 0ull;
    if (j < n_send) {
        int i = 0;
        while (j >= dd->send_off[i + 1]) ++i;
        mine = i;
        // v == nullptr: the transport self-test's pattern of this round instead of vector entries
        bits = v ? (unsigned long long)__double_as_longlong(v[dd->send_idx[j]]) : selftest_pattern(E, dd->rank, j - dd->send_off[i]);
        // a write-through store over xGMI / into the peer process's block
        if (!(paranoid && dd->inject_stale_round == (long long)E && j == 0)) // (test hook: one entry is NOT stored)
            st_sys(reinterpret_cast<unsigned long long *>(dd->peer_halo_dst[i] + (j - dd->send_off[i])), bits);
    }
    if (paranoid) {
        for (int i = 0; i < np; ++i) { // a wave's lanes may feed different peers: one pass per peer
            if (dd->send_off[i + 1] <= (int)blockIdx.x * 256 || dd->send_off[i] >= (int)(blockIdx.x + 1) * 256) continue; // block-uniform
            const unsigned long long cs = wave_sum_u64(mine == i ? bits : 0ull);
            if ((threadIdx.x & 63) == 0 && cs) __hip_atomic_fetch_add(dd->psum + i, cs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    wait_own_stores(); // acknowledged by the destination before this wave reaches the barrier
    __syncthreads();
    if (threadIdx.x == 0) push_raise_flags(dd, epoch, ticket, gridDim.x); // every block's stores are out: raise my flag in the blocks of the peers I feed
}

// One round of the transport self-test (direct_selftest): a single workgroup waits for the peers' flags, checks the checksums and
// that every halo entry IS this round's pattern (a stale entry holds the previous round's), then all-gathers the cumulative
// count of bad entries through the same finalisation the solve uses (which is also the barrier between rounds).
__global__ __launch_bounds__(256) void k_direct_selftest(HaloView hv, unsigned long long *bad_total)
{
    if (hv.sc->done) return; // a wait timed out in an earlier round: the peers find out through their own time limit
    const unsigned long long bad = paranoid_check<256>(hv, true);
    __shared__ double cum;
    if (threadIdx.x == 0) {
        *bad_total += (bad & 0xFFFFFFFFull) + (bad >> 32);
        cum = (double)*bad_total;
    }
    __syncthreads();
    double acc[4] = {0., 0., 0., 0.};
    if (threadIdx.x == 0) acc[0] = cum;
    dist_finalize<256>(hv, acc);
}

// The finalizer of the direct transport as a launch of its own, behind the brick-structured form's SpMV (whose persistent workgroups
// keep three per CU with the LDS they have: the finalizer's staging would cost the third): folds the round's stage slots and the
// vector kernel's partials, all-gathers the sums with the other ranks and applies the scalar step (halo_finalizer, avs_halo.hpp).
__global__ __launch_bounds__(512) void k_halo_finalize(HaloView hv)
{
    if (hv.sc->done) return;
    halo_finalizer<512>(hv, (int)blockIdx.x);
}
// ... and in FRONT of it: wait for the peers' entries of this round (their epoch flags), then copy the comm block's halo area behind the
// owned entries of the vector the product reads (system-scope loads: the entries were written by other GPUs), so that the brick kernel
// itself is the plain one -- [owned | halo] is one array, as with the RCCL transport.  T = float: the entries (floats widened by the
// sender) are narrowed back, exactly.
template <typename T>
__global__ __launch_bounds__(256) void k_halo_gather(HaloView hv, T *__restrict__ vec)
{
    if (hv.sc->done) return;
    halo_wait(hv);
    const DistDev *dd = hv.dd;
    int n_halo = 0;
    for (int i = 0; i < dd->npeers; ++i) n_halo += dd->recv_cnt[i];
    const long long n_own = dd->n_own;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n_halo; j += gridDim.x * 256) vec[n_own + j] = (T)ld_sys_f64(dd->my_halo + j);
}

#include "avs_pcg_resident.inl"

// Transport self-test, run once per plan right after the blocks are connected and before the direct transport is trusted with a
// solve (round-2 review: "never run on more than one GPU"): `rounds` full-size halo rounds over the real links with a
// round-dependent pattern, checksum + per-entry verification by the reader while the next flag is already being polled, and the
// bad-entry count all-gathered through the solve's own finalisation.  Every rank gets the same total => the same decision.
avs_status direct_selftest(const DirectArgs &da, int rounds, hipStream_t stream, long long *bad_entries, int *fault)
{
    DevBuf<PcgScalars> sc;
    DevBuf<unsigned long long> bad;
    AVS_TRY(sc.alloc(1));
    AVS_TRY(bad.alloc(1));
    AVS_HIP(hipMemsetAsync(sc.p, 0, sizeof(PcgScalars), stream));
    AVS_HIP(hipMemsetAsync(bad.p, 0, sizeof(unsigned long long), stream));
    const int push_blocks = da.n_send > 0 ? (da.n_send + 255) / 256 : 0;
    HaloView hv;
    hv.dd = da.dd;
    hv.epoch = da.epoch;
    hv.epoch_w = da.epoch;
    hv.fin_ticket = da.fin_ticket;
    hv.sc = sc.p;
    hv.nfin = 1;
    hv.nred_vec = 0;
    hv.op = 0;
    hv.selftest = 1;
    for (int r = 0; r < rounds; ++r) {
        if (push_blocks)
            hipLaunchKernelGGL(k_push, dim3(push_blocks), dim3(256), 0, stream, da.dd, (const double *)nullptr, (const unsigned long long *)da.epoch,
                               da.push_ticket, (const PcgScalars *)sc.p);
        hipLaunchKernelGGL(k_direct_selftest, dim3(1), dim3(256), 0, stream, hv, bad.p);
    }
    AVS_HIP(hipGetLastError());
    PcgScalars h;
    AVS_HIP(hipMemcpyAsync(&h, sc.p, sizeof(h), hipMemcpyDeviceToHost, stream));
    AVS_HIP(hipStreamSynchronize(stream));
    *fault = h.fault;
    *bad_entries = (long long)h.red[0]; // the LAST round's all-gathered cumulative count (all ranks hold the same number)
    return AVS_OK;
}

// the message of a fault the direct transport's kernels left in the scalar state
static avs_status direct_fault(const PcgScalars &h)
{
    if (h.fault == 4)
        set_error("direct transport (paranoid mode): a halo segment does not add up to the checksum its sender left ahead of the flag "
                  "-- stale or torn halo entries (iteration ~%d)", h.iter);
    else
        set_error("direct transport: %s did not arrive within the time limit (rank stalled or dead?)",
                  h.fault == 1 ? "a peer's halo entries" : (h.fault == 2 ? "a peer's partial sums" : "a workgroup's partial sums"));
    return AVS_ERCCL;
}

// MIXED (T = float, AVS_OPTION_DIST_MIXED_PRECISION): the float path's three-launch round with the double-scalar step ops; the last round
// of a chunk folds its sums without a step (OP_NONE), and the reliable update behind the chunk -- a k_push round of x, the fp64 product,
// k_sr_mixed_residual, a round of u -- takes it on the true residual's sums (k_sr_mixed_step).
template <typename T, bool MIXED = false>
static avs_status pcg_solve_direct(PcgWork *w, const CsrView &A, const double *b, double *x, double tol, int max_iters,
                                   hipStream_t stream, avs_solve_info *info, const DirectArgs &da)
{
    constexpr bool F32 = std::is_same<T, float>::value;
    typedef typename std::conditional<MIXED, double, T>::type SS; // the scalar type of the update kernel
    const int64_t n = A.n;
    int g = 1, chunk_rows = kBlock; // every vector kernel of this loop uses the fused kernel's geometry (same partial layout)
    sr_update_geometry((long long)n, &g, &chunk_rows);
    AVS_REQUIRE(g == da.push_grid && chunk_rows == da.push_chunk, AVS_EINTERNAL, "push segments were built for another geometry");
    // one dictionary of few values: the loop's vector kernel reads a 2-B diagonal code
    const bool coded = diag_coded(A);
    // brick-structured form of the local rows (float vectors: with its float walk): one partial per persistent workgroup
    const bool brick = A.brick && A.brick->ntiles > 0 && (!F32 || A.brick->pwords32);
    int ntiles = 0, ppt = 1; // the SpMV's partials: ntiles * ppt stage slots
    if (F32) ntiles = n <= 0 ? 0 : (int)f32_spmv_partials(A, MIXED);
    else {
        ntiles = brick ? brick_partial_count(*A.brick, 8) : da.n_tiles_int + da.n_tiles_bnd; // (word stream: == ceil(n / kTileRows))
        ppt = brick ? 1 : (A.codes ? kTileRows / 64 : 1); // value-indexed kernel: one partial per wave
    }
    const int slots = ntiles * ppt;
    const int nfin = slots > 0 ? (slots + kFinShare - 1) / kFinShare : 1;
    AVS_TRY(w->stage2.alloc((size_t)(slots > 0 ? slots : 1) + (size_t)nfin));
    AVS_HIP(hipMemsetAsync(w->stage2.p, 0xFF, (size_t)(slots > 0 ? slots : 1) * sizeof(double), stream)); // arm: kSentinel in every slot
    const int push_blocks = da.n_send > 0 ? (da.n_send + 255) / 256 : 0;
    const int n_halo_cols = (int)(w->n_ext - n);
    AVS_TRY(w->cancel_dev.alloc(1));
    AVS_HIP(hipMemsetAsync(w->cancel_dev.p, 0, sizeof(int), stream));
    double *pvec = w->partial.p; // up to 3 * g vector-kernel partials
    PcgScalars *sc = w->sc.p;
    SrVecs<T> v;
    const int variant = spmv_default_variant(A);
    ChunkState cs;

    // MIXED: x to the peers in fp64 and t64 = A x with the rank's fp64 product (the set-up and every reliable update): a round of its own
    // -- push, wait + gather into the tail of the staging vector w->p, the product, and a finalizer without stage slots or sums, whose
    // all-gather is the round's barrier (nobody pushes u into a halo area that is still being gathered) and advances the epoch
    auto product_x = [&]() -> avs_status {
        AVS_HIP(hipMemcpyAsync(w->p.p, x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream));
        if (push_blocks)
            hipLaunchKernelGGL(k_push, dim3(push_blocks), dim3(256), 0, stream, da.dd, (const double *)x, (const unsigned long long *)da.epoch,
                               da.push_ticket, (const PcgScalars *)sc);
        HaloView hv;
        hv.dd = da.dd;
        hv.epoch = da.epoch;
        hv.epoch_w = da.epoch;
        hv.fin_ticket = da.fin_ticket;
        hv.sc = sc;
        hv.pvec = pvec;
        hv.stage = w->stage2.p;
        hv.stage2 = w->stage2.p + (slots > 0 ? slots : 1);
        hv.g = g;
        hv.tol = tol; // (ntiles = 0, nfin = 1, nred_vec = 0, op = OP_NONE, no cancel word: a request waits for the round of u)
        if (da.npeers > 0) {
            const int hg = n_halo_cols > 0 ? (n_halo_cols + 255) / 256 : 1;
            hipLaunchKernelGGL(k_halo_gather<double>, dim3(hg < 64 ? hg : 64), dim3(256), 0, stream, hv, w->p.p);
        }
        AVS_TRY(spmv_launch(A, w->p.p, w->t.p, variant, stream));
        hipLaunchKernelGGL(k_halo_finalize, dim3(1), dim3(512), 0, stream, hv);
        AVS_HIP(hipGetLastError());
        return AVS_OK;
    };

    // one round: push `vec` to the peers, v.w = A vec (+ partials of vec.v.w), fold `nred_vec` vector partial arrays + those, step `op`
    auto round = [&](T *vec, int nred_vec, int op, hipEvent_t ea, hipEvent_t eb, bool push) -> avs_status {
        if (push && push_blocks) {
            const double *pv = nullptr;
            if constexpr (F32) { // k_push reads doubles: vec widened through w->t (the fp64 loop's w, unused here)
                hipLaunchKernelGGL(k_f32_widen, dim3(g), dim3(kBlock), 0, stream, n, (const float *)vec, w->t.p);
                pv = w->t.p;
            } else {
                pv = vec;
            }
            hipLaunchKernelGGL(k_push, dim3(push_blocks), dim3(256), 0, stream, da.dd, pv, (const unsigned long long *)da.epoch, da.push_ticket,
                               (const PcgScalars *)sc);
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
        hv.ntiles = ntiles;
        hv.ppt = ppt;
        hv.nfin = nfin;
        hv.g = g;
        hv.nred_vec = nred_vec;
        hv.op = op;
        hv.tol = tol;
        hv.cancel = w->cancel_dev.p;
        if (!F32 && !brick) {
            // fp64 word stream: ONE launch over all tiles + the finalizer block: tiles that read halo columns (flagged; the last ones of
            // the [interior | halo-reading] row order) wait for the peers' flags, everything else multiplies while the halo travels
            if constexpr (!F32) AVS_TRY(spmv_dot_tiles_halo(A, vec, v.w, nullptr, sc, nullptr, ntiles + nfin, hv, stream));
        } else { // halo into the vector's tail, the SpMV (partials into the stage slots), the finalizer: three launches
            if (da.npeers > 0) {
                const int hg = n_halo_cols > 0 ? (n_halo_cols + 255) / 256 : 1;
                hipLaunchKernelGGL(k_halo_gather<T>, dim3(hg < 64 ? hg : 64), dim3(256), 0, stream, hv, vec);
            }
            if constexpr (MIXED) AVS_TRY(spmv_mixed_dispatch<true>(A, vec, v.w, w->stage2.p, sc, stream, nullptr));
            else if constexpr (F32) AVS_TRY(spmv_f32_dispatch<true>(A, vec, v.w, w->stage2.p, sc, stream, nullptr));
            else AVS_TRY(spmv_brick_launch(*A.brick, vec, v.w, w->stage2.p, &sc->done, stream));
            hipLaunchKernelGGL(k_halo_finalize, dim3(nfin), dim3(512), 0, stream, hv);
        }
        if (eb) AVS_HIP(hipEventRecord(eb, stream));
        AVS_HIP(hipGetLastError());
        return AVS_OK;
    };
    AVS_TRY((sr_setup<T, MIXED>(w, A, b, x, coded, g, &v, stream, [&](int k) -> avs_status {
        if (MIXED && k == 0) return product_x();
        return k == 0 ? round(v.u, 0, (int)OP_NONE, nullptr, nullptr, true)
                      : round(v.u, 3, (F32 && !MIXED) ? (int)OP_SR_INIT_F32 : (int)OP_SR_INIT, nullptr, nullptr, true);
    })));

    // Systems that fit on the chip (<= ~1 M rows, packed single-dictionary form): the rest of the solve in ONE cooperative launch,
    // matrix words in the register files, vector slices in LDS (avs_pcg_resident.inl).  Needs the GPU for itself.  fp64, and float
    // vectors with AVS_OPTION_RESIDENT_F32 (k_cg_resident<.., float>: the same state, the same scalar step as this loop).
    w->resident_used = 0;
    if (!MIXED && (!F32 || A.resident_f32)) {
        // (AVS_OPTION_RESIDENT_LOCAL_TABLES: also a matrix without one small dictionary, with the per-row inverse this set-up made --
        // the float set-up of a coded matrix makes none: no resident loop then)
        const bool local = resident_local_tables_wanted(A);
        if ((local ? v.invd != nullptr : coded) && (da.exclusive_device || cur_opt().resident_cus > 0) && resident_wanted(true)) {
            if (!w->resident) w->resident = new (std::nothrow) ResidentPlan();
            if (w->resident && resident_prepare(w->resident, A, w->n_ext, &da, F32, stream)) {
                bool launched = false;
                AVS_TRY(resident_run<T>(w->resident, A, v.x, v.r, v.p, v.s, v.u, v.w, v.dcode, w->resident->local ? v.invd : v.invtab, sc, max_iters, &da,
                                        stream, &launched));
                w->resident_used = launched ? 1 : 0; // (refused: the loop below takes over from the same state)
            }
        }
    }

    auto enqueue_iteration = [&](int c, bool timed) -> avs_status {
        // update and push in one launch (3 launches per iteration)
        // (KEEP = false only with the brick form, which serves single-dictionary matrices: coded)
        with_flags([&](auto C, auto B) {
            hipLaunchKernelGGL((k_sr_update_push<C.value, !(C.value && B.value), T, SS>), dim3(g), dim3(kBlock), 0, stream, n, v.x, v.r, v.p, v.s,
                               v.u, (const T *)v.w, coded ? v.invtab : v.invd, v.dcode, (const PcgScalars *)sc, pvec, da.dd,
                               (const unsigned long long *)da.epoch, da.push_ticket);
        }, coded, brick);
        int op = F32 ? (int)OP_SR_STEP_F32 : (int)OP_SR_STEP;
        if constexpr (MIXED) { // the chunk's last round leaves its step to the reliable update (cs.enqueued: iterations before this chunk)
            const int len = (max_iters - cs.enqueued) < kChunk ? (max_iters - cs.enqueued) : kChunk;
            op = c == len - 1 ? (int)OP_NONE : (int)OP_SR_STEP;
        }
        return round(v.u, 2, op, timed ? w->evA[c] : nullptr, timed ? w->evB[c] : nullptr, false);
    };
    auto enqueue_update = [&]() -> avs_status {
        if constexpr (MIXED) {
            hipLaunchKernelGGL(k_sr_mixed_begin, dim3(1), dim3(1), 0, stream, sc);
            hipLaunchKernelGGL(k_mixed_fold, dim3(g), dim3(kBlock), 0, stream, n, x, v.x, (const PcgScalars *)sc);
            AVS_TRY(product_x());
            with_flags([&](auto C) {
                hipLaunchKernelGGL((k_sr_mixed_residual<C.value, false>), dim3(g), dim3(kBlock), 0, stream, n, b, (const double *)w->t.p, v.r, v.u,
                                   coded ? v.invtab : v.invd, v.dcode, pvec, (const PcgScalars *)sc);
            }, coded);
            AVS_TRY(round(v.u, 2, (int)OP_NONE, nullptr, nullptr, true));
            hipLaunchKernelGGL(k_sr_mixed_step, dim3(1), dim3(1), 0, stream, sc);
            AVS_HIP(hipGetLastError());
            w->reliable_updates++;
        }
        return AVS_OK;
    };
    GraphKey key = matrix_key(MIXED ? kGraphDirectMixed : F32 ? kGraphDirectF32 : kGraphDirect, A, v.x, tol);
    key.b = b;
    key.dd = da.dd;
    key.ntiles = ntiles;
    key.brick = brick;
    key.coded = coded;
    const GraphKey *gkey = cur_opt().graph != 0 ? &key : nullptr;
    bool cancel_sent = false;
    for (;;) {
        AVS_TRY(poll_scalars(w, sc, stream));
        if (w->host_sc->fault) {
            if (w->resident_used && w->resident) w->resident->ok = false; // the next distributed solve on this plan takes the launch-per-phase loop
            return direct_fault(*w->host_sc);
        }
        sample_spmv(w, info != nullptr, true, &cs);
        if (MIXED && w->host_sc->done == 0 && w->host_sc->iter < cs.enqueued) cs.enqueued = w->host_sc->iter; // a chunk the recurrence froze
        if (w->host_sc->done || cs.enqueued >= max_iters || w->resident_used) break;
        if (cancel_requested() && !cancel_sent) { // avs_cancel: the request word the finalizer adds to the round's sums -- every rank stops in the same round
            static const int one = 1;
            AVS_HIP(hipMemcpyAsync(w->cancel_dev.p, &one, sizeof(int), hipMemcpyHostToDevice, stream));
            cancel_sent = true;
        }
        AVS_TRY(enqueue_chunk(w, stream, gkey, max_iters, info != nullptr, enqueue_iteration, &cs));
        AVS_TRY(enqueue_update()); // (MIXED)
    }
    if constexpr (MIXED) {
        if (w->host_sc->done == 3) AVS_HIP(hipMemsetAsync(x, 0, (size_t)n * sizeof(double), stream)); // rhs == 0: x := 0
    } else {
        if (w->host_sc->done == 3) AVS_HIP(hipMemsetAsync(v.x, 0, (size_t)n * sizeof(T), stream)); // rhs == 0: x := 0
        if constexpr (F32) hipLaunchKernelGGL(k_f32_widen, dim3(g), dim3(kBlock), 0, stream, n, (const float *)v.x, x);
    }
    AVS_HIP(hipGetLastError());
    AVS_TRY(finish_info(w, A, stream, info, &cs, w->host_sc->cancelled != 0, w->resident_used, F32 && !MIXED));
    if (w->host_sc->cancelled) (void)cancel_consume();
    return AVS_OK;
}

// ---------------------------------------------------------------------------------------------
avs_status pcg_create(PcgWork **out, int64_t n, int64_t n_ext, hipStream_t)
{
    PcgWork *w = new (std::nothrow) PcgWork();
    AVS_REQUIRE(w, AVS_ENOMEM, "out of host memory");
    w->n = n;
    w->n_ext = n_ext;
    w->npartial = spmv_partial_elems(n);
    avs_status s;
    if ((s = w->r.alloc((size_t)n)) || (s = w->p.alloc((size_t)n_ext)) || (s = w->t.alloc((size_t)n)) ||
        (s = w->invd.alloc((size_t)n)) || (s = w->partial.alloc(w->npartial)) || (s = w->sc.alloc(2)) ||
        (s = w->stage.alloc((size_t)kRedBlocks * 4)) || (s = w->ticket.alloc(1))) {
        delete w;
        return s;
    }
    if (hipMemset(w->ticket.p, 0, sizeof(unsigned)) != hipSuccess) {
        set_error("hipMemset failed");
        pcg_destroy(w);
        return AVS_EHIP;
    }
    if (hipHostMalloc(reinterpret_cast<void **>(&w->host_sc), sizeof(PcgScalars)) != hipSuccess ||
        hipEventCreate(&w->ev0) != hipSuccess || hipEventCreate(&w->ev1) != hipSuccess) {
        set_error("pinned host / event allocation failed");
        pcg_destroy(w);
        return AVS_EHIP;
    }
    for (int i = 0; i < kChunk; ++i)
        if (hipEventCreate(&w->evA[i]) != hipSuccess || hipEventCreate(&w->evB[i]) != hipSuccess) {
            set_error("event allocation failed");
            pcg_destroy(w);
            return AVS_EHIP;
        }
    *out = w;
    return AVS_OK;
}

int64_t pcg_rows(const PcgWork *w) { return w ? w->n : -1; }
int pcg_float_vectors(const PcgWork *w) { return w ? w->float_vectors : 0; }
int pcg_reliable_updates(const PcgWork *w) { return w ? w->reliable_updates : 0; }
void pcg_fused_state(const PcgWork *w, int *used, int *faults)
{
    if (used) *used = w ? w->fused_used : 0;
    if (faults) *faults = w ? w->fused_faults : 0;
}

void pcg_destroy(PcgWork *w)
{
    if (!w) return;
    delete w->resident;
    drop_graph(w);
    if (w->host_sc) (void)hipHostFree(w->host_sc);
    if (w->ev0) (void)hipEventDestroy(w->ev0);
    if (w->ev1) (void)hipEventDestroy(w->ev1);
    for (int i = 0; i < kChunk; ++i) {
        if (w->evA[i]) (void)hipEventDestroy(w->evA[i]);
        if (w->evB[i]) (void)hipEventDestroy(w->evB[i]);
    }
    delete w;
}

// Single GPU, no partition: the single-reduction iteration on the chip when the system qualifies (*ran = false otherwise, nothing
// touched).  Set-up (r = b - A x, u = M^-1 r, w = A u, the three sums) with the launch-per-phase kernels, the loop resident.
// T = float (AVS_OPTION_RESIDENT_F32): set-up and loop on float vectors, the solution widened into x at the end; a fault hands the
// solve to the float launch-per-phase loop (pcg_solve_phases<float>) instead of the fp64 one.
template <typename T>
static avs_status pcg_solve_resident_single(PcgWork *w, const CsrView &A, const double *b, double *x, double tol, int max_iters,
                                            hipStream_t stream, avs_solve_info *info, bool *ran)
{
    constexpr bool F32 = std::is_same<T, float>::value;
    *ran = false;
    const int64_t n = A.n;
    const bool coded = diag_coded(A);
    // AVS_OPTION_RESIDENT_LOCAL_TABLES: a matrix without one small dictionary is planned with local value tables; its set-up is the
    // uncoded one (one inverse per row, which the loop then reads)
    const bool local = resident_local_tables_wanted(A);
    if (!coded && !local) return AVS_OK;
    if (!w->resident) w->resident = new (std::nothrow) ResidentPlan();
    if (cancel_requested()) return AVS_OK; // (the launch-per-phase loop consumes the request at its first poll: 0 iterations, cancelled = 1)
    if (!w->resident || !resident_prepare(w->resident, A, A.n, nullptr, F32, stream)) return AVS_OK;
    if (F32) AVS_TRY(ensure_partials(w, 4 * (size_t)kVecGrid + f32_spmv_partials(A, false) + 16)); // (as pcg_solve_single_reduction<float>)
    SrVecs<T> v;
    AVS_TRY(sr_setup_exchange(w, A, b, x, tol, !w->resident->local, nullptr, &v, stream));
    // the initial guess is kept: if a bounded wait inside the cooperative launch times out (the grid was not co-resident in time: a GPU
    // shared with a viewport or OpenCL work) the solve is redone from it by the launch-per-phase loop IN THIS CALL
    AVS_TRY(w->x_save.alloc((size_t)n));
    AVS_HIP(hipMemcpyAsync(w->x_save.p, x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream));
    bool launched = false;
    AVS_TRY(resident_run<T>(w->resident, A, v.x, v.r, v.p, v.s, v.u, v.w, v.dcode, w->resident->local ? v.invd : v.invtab, w->sc.p, max_iters, nullptr,
                            stream, &launched));
    if (!launched) return AVS_OK; // (x is untouched: the launch-per-phase loop starts over from it)
    AVS_TRY(poll_scalars(w, w->sc.p, stream));
    bool faulted = w->host_sc->fault != 0;
#ifdef AVS_PROBES
    if (getenv("AVS_CG_RESIDENT_FAKE_FAULT")) faulted = true; // test hook of exactly this path (probe build only)
#endif
    if (faulted) {
        w->resident->ok = false; // not again for this plan (until a new matrix or the other vector type re-plans)
        w->resident_faults++;
        AVS_HIP(hipMemcpyAsync(x, w->x_save.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream));
        return AVS_OK;           // *ran stays false: pcg_solve carries on with the launch-per-phase loop
    }
    *ran = true;
    w->resident_used = 1;
    if (w->host_sc->done == 3) AVS_HIP(hipMemsetAsync(v.x, 0, (size_t)n * sizeof(T), stream)); // rhs == 0: x := 0
    if constexpr (F32) hipLaunchKernelGGL(k_f32_widen, dim3(vec_grid(n)), dim3(kBlock), 0, stream, n, (const float *)v.x, x);
    AVS_HIP(hipGetLastError());
    AVS_TRY(finish_info(w, A, stream, info, nullptr, false, 1, F32)); // (spmv_ms = 0: no separate SpMV launch to time)
    // avs_cancel during the cooperative launch: the launch cannot be interrupted, but the request ends HERE -- consumed, and reported when the
    // loop stopped at max_iterations without converging (a converged solve is a converged solve; the request is consumed either way, so that
    // it cannot hit the next solve on this context)
    if (cancel_consume() && info && w->host_sc->done == 0) {
        info->cancelled = 1;
        info->converged = 0;
    }
    return AVS_OK;
}


#ifdef AVS_PROBES
// include/avs_probe.h, avs_pcg_csr_plan: what resident_prepare left on the plan of w's last solve, and whether the loop ran it
void pcg_resident_plan_info(const PcgWork *w, avs_resident_plan_info *out)
{
    avs_resident_plan_info o{};
    const size_t size = out->struct_size > 0 ? std::min((size_t)out->struct_size, sizeof(o)) : 0;
    o.struct_size = (int32_t)size;
    o.used = w->resident_used;
    const char *why = "";
    if (const ResidentPlan *pl = w->resident) {
        o.workgroups = pl->G;
        o.max_lanes_per_workgroup = pl->max_lanes;
        o.lanes = pl->n_lanes;
        o.max_rows_per_workgroup = pl->max_rows;
        o.lc_bits = pl->lc_bits;
        o.ng = pl->ng;
        o.lds_bytes = (int32_t)pl->lds;
        o.max_quads = pl->max_quads;
        o.long_row_lanes = pl->long_lanes;
        o.longest_tail = pl->longest_tail;
        o.max_lane_streamed_rows = pl->max_lane_streamed;
        o.streamed_rows = pl->streamed_rows;
        o.streamed_words = pl->streamed_words;
        o.max_remote = pl->max_remote;
        o.remap_passes = pl->remap_passes;
        o.local_tables = pl->local ? 1 : 0;
        o.tables_per_workgroup = pl->local ? pl->lt_gpw : 0;
        o.largest_table = pl->lt_max;
        if (!o.used) why = !pl->why.empty() ? pl->why.c_str() : w->resident_faults ? "a bounded wait of the loop timed out" : "not tried";
    } else if (!o.used)
        why = "not planned (no dictionary-coded form, or the loop is switched off)";
    snprintf(o.why, sizeof(o.why), "%s", why);
    memcpy(out, &o, size);
}
#endif

// One fused launch for the two vector kernels of the fp64 launch-per-phase loop (k_update_fused): HBM-sized single-GPU systems whose
// rows fit its registers, a device with one CU per workgroup of its grid.  *on: this solve uses it; then the initial guess is kept, so
// that a timed-out barrier costs a redo, not a wrong answer.  fuse_beta: the loop's (never with a partition).
static avs_status fused_raise_lds() // the kernel's dynamic LDS limit: once per device
{
    static std::atomic<unsigned long long> raised{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev >= 0 && dev < 64 && !((raised.load() >> dev) & 1ull)) {
        AVS_HIP(hipFuncSetAttribute((const void *)k_update_fused<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kFusedLds + kFusedTabBytes)));
        AVS_HIP(hipFuncSetAttribute((const void *)k_update_fused<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kFusedLds + kFusedTabBytes)));
        AVS_HIP(hipFuncSetAttribute((const void *)k_update_fused<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kFusedLds + kFusedTabBytes)));
        AVS_HIP(hipFuncSetAttribute((const void *)k_update_fused<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kFusedLds + kFusedTabBytes)));
        raised.fetch_or(1ull << dev);
    }
    return AVS_OK;
}
static bool fused_device_fits() // one CU per workgroup of the fused launch's grid
{
    int dev = 0, cus = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return cus >= kVecGrid / 8;
}
static avs_status fused_vectors_setup(PcgWork *w, const CsrView &A, const double *x, int g, bool fuse_beta, bool keep, hipStream_t stream, bool *on)
{
    const int64_t n = A.n;
    bool fuse_vec = false;
    if (fuse_beta && cur_opt().fuse_vectors != 0 && !w->fused_off && g == kVecGrid && n <= (int64_t)2 * kFusedPairs * kVecGrid * kBlock &&
        n < ((int64_t)1 << 28) && (cur_opt().fuse_vectors > 0 || !keep))
        fuse_vec = fused_device_fits();
    if (fuse_vec) {
        AVS_TRY(fused_raise_lds());
        if (!w->fused_bar.p) {
            AVS_TRY(w->fused_bar.alloc(2));
            AVS_HIP(hipMemsetAsync(w->fused_bar.p, 0, 2 * sizeof(unsigned long long), stream));
        }
        AVS_TRY(w->x_save.alloc((size_t)n));
        AVS_HIP(hipMemcpyAsync(w->x_save.p, x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream));
    }
    w->fused_used = 0; // (1 once a fused launch has been enqueued: the loop falls back to the two launches where the SpMV leaves many partial sums)
    *on = fuse_vec;
    return AVS_OK;
}

// ---------------------------------------------------------------------------------------------
// The launch-per-phase loop: single-GPU solves in fp64 (T = double), on float vectors (T = float: AVS_PRECISION_F32, avs_pcg_f32.inl)
// and in mixed precision (T = float, MIXED: AVS_OPTION_MIXED_PRECISION, avs_pcg_mixed.inl), and the RCCL standard-CG path (dist, fp64
// only).  One iteration: SpMV with the fused dot, update_r, update_xp; chunks of kChunk iterations, replayed from a captured graph.
//                 fp64                                   float                                  mixed
//   vectors       caller's x, w->p/r/t, fp64 diagonal    f_x = narrowed x, f_b = narrowed b,    f_x = the correction, zeroed; f_p/r/t;
//                                                        f_p/r/t, float diagonal                t64 = w->t; float diagonal
//   partials      grown only for a brick form            max(stream, brick)                     that, and >= 6 kVecGrid + 64
//   start         spmv_launch, k_init_residual,          float SpMV, k_init_residual,           fp64 SpMV into t64, k_mixed_residual<., true>
//                 OP_INIT, k_init_p, OP_RHO0             OP_INIT, k_f32_threshold,              into vpart, k_mixed_finish<true>,
//                                                        k_init_p<., coded>, OP_RHO0            k_init_p<., coded> (no reduction)
//   vpart         upper half only with fuse_alpha        always the upper half                  as float
//   unfused       update_r: parity 0                     the iteration's parity                 as float
//   beta step     fuse_beta option, off with dist        always in update_xp                    as float
//   graph         !dist; kGraphF64, key x, key.brick =   kGraphF32, key f_x, key.brick = the    kGraphMixed, else as float
//                 A.brick != nullptr, key.fuse_vec       form has its float walk
//   behind chunk  --                                     --                                     the reliable update (enqueue_update)
//   end           fused-barrier redo                     k_f32_widen, float error               done == 3: x := 0
// ---------------------------------------------------------------------------------------------
// b, x: the context's fp64 arrays (float: holding float values); x holds the initial guess and receives the solution
template <typename T, bool MIXED = false>
static avs_status pcg_solve_phases(PcgWork *w, const CsrView &A, const double *b, double *x, double tol, int max_iters, hipStream_t stream,
                                   avs_solve_info *info, PcgDist *dist)
{
    constexpr bool F32 = std::is_same<T, float>::value;
    static_assert(F32 || !MIXED, "the mixed-precision loop iterates on float vectors");
    typedef std::conditional_t<MIXED, double, T> S; // the type of the vector kernels' scalar steps
    static_assert(kChunk % 2 == 0, "the parity of an iteration is taken from its position in the chunk");
    const int64_t n = A.n;
    const size_t na = (size_t)n + 8;
    const int g = vec_grid(n);
    const int variant = spmv_default_variant(A);
    const bool coded = diag_coded(A);
    // the brick form of the matrix (float vectors: with its float walk) -- one partial per wave of every tile: tiles may be smaller than 512 rows
    const bool brick = A.brick && A.brick->ntiles > 0 && (!F32 || A.brick->pwords32);
    {
        size_t need = F32 ? phase_partials((size_t)stream_grid(n)) : 0; // the streaming kernel: one partial per 256 rows
        if (brick) need = std::max(need, phase_partials((size_t)A.brick->ntiles * 8));
        if (MIXED) need = std::max(need, 6 * (size_t)kVecGrid + 64); // k_mixed_residual<.., INIT>: three sums of g partials in the upper half
        AVS_TRY(ensure_partials(w, need));
    }
    T *xv = nullptr, *p = nullptr, *r = nullptr, *t = nullptr, *inv = nullptr; // inv: indexed by dcode[i] (coded) or by i
    const uint16_t *dcode = nullptr;
    if constexpr (F32) { // (the float set-up of the CU-resident loop allocates all but f_b)
        w->float_vectors = 1;
        AVS_TRY(w->f_x.alloc(na)); AVS_TRY(w->f_r.alloc(na)); AVS_TRY(w->f_p.alloc(na)); AVS_TRY(w->f_t.alloc(na));
        if (!MIXED) AVS_TRY(w->f_b.alloc(na));
        xv = w->f_x.p, p = w->f_p.p, r = w->f_r.p, t = w->f_t.p;
    } else {
        xv = x, p = w->p.p, r = w->r.p, t = w->t.p;
    }
    double *const partial = w->partial.p, *const t64 = w->t.p;
    double *const upper = partial + (w->npartial / 2); // the vector kernels' partial sums while the SpMV's are still being read
    PcgScalars *sc = w->sc.p;
    auto product = [&](auto DOT, const T *in, T *out, int *nb) -> avs_status { // out = A in (DOT: + the partials of in.out)
        if constexpr (MIXED) return spmv_mixed_dispatch<DOT.value>(A, in, out, DOT.value ? partial : nullptr, DOT.value ? sc : nullptr, stream, nb);
        else return sr_spmv<DOT.value>(A, in, out, DOT.value ? partial : nullptr, DOT.value ? sc : nullptr, variant, stream, nb);
    };

    AVS_HIP(hipMemsetAsync(sc, 0, sizeof(PcgScalars), stream));
    if constexpr (MIXED) {
        AVS_HIP(hipMemsetAsync(xv, 0, na * sizeof(float), stream));
    } else if constexpr (F32) {
        hipLaunchKernelGGL(k_f32_narrow, dim3(g), dim3(kBlock), 0, stream, n, b, w->f_b.p);
        hipLaunchKernelGGL(k_f32_narrow, dim3(g), dim3(kBlock), 0, stream, n, (const double *)x, xv);
    }
    AVS_TRY(prepare_diagonal<T>(w, A, coded, &inv, &dcode, stream));
    AVS_HIP(hipEventRecord(w->ev0, stream));

    // residual = rhs - mat * x ; p = z = D^-1 r ; |b|^2, |r|^2, rho
    if constexpr (MIXED) { // in fp64, r rounded to float; rho is the fp64 sum (k_init_p's own r.z partials are not used)
        AVS_TRY(spmv_launch(A, x, t64, variant, stream));
        with_flags([&](auto C) {
            hipLaunchKernelGGL((k_mixed_residual<C.value, true>), dim3(g), dim3(kBlock), 0, stream, n, b, (const double *)t64, r, (const float *)inv,
                               dcode, upper, (const PcgScalars *)sc);
        }, coded);
        hipLaunchKernelGGL(k_mixed_finish<true>, dim3(1), dim3(kRedBlock), 0, stream, (const double *)upper, g, sc, tol);
    } else if constexpr (F32) {
        AVS_TRY(product(std::false_type{}, xv, t, nullptr));
        hipLaunchKernelGGL(k_init_residual<float>, dim3(g), dim3(kBlock), 0, stream, n, (const float *)w->f_b.p, (const float *)t, r, partial);
        AVS_TRY(reduce_stage(w, g, 2, OP_INIT, tol, 0, stream, nullptr));
        hipLaunchKernelGGL(k_f32_threshold, dim3(1), dim3(1), 0, stream, sc, tol);
    } else {
        if (dist) { // x must be visible in its extended form for the product: stage it through p
            AVS_HIP(hipMemcpyAsync(p, x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream));
            AVS_TRY(dist_halo_exchange(dist, p, stream));
        }
        AVS_TRY(product(std::false_type{}, dist ? p : x, t, nullptr));
        hipLaunchKernelGGL(k_init_residual<double>, dim3(g), dim3(kBlock), 0, stream, n, b, (const double *)t, r, partial);
        AVS_TRY(reduce_stage(w, g, 2, OP_INIT, tol, 0, stream, dist));
    }
    // p = z: float vectors read the loop's diagonal, fp64 the per-row inverse, of a coded matrix too
    if constexpr (F32)
        with_flags([&](auto C) {
            hipLaunchKernelGGL((k_init_p<float, C.value>), dim3(g), dim3(kBlock), 0, stream, n, (const float *)r, (const float *)inv, dcode, p, xv,
                               partial, (const PcgScalars *)sc);
        }, coded);
    else
        hipLaunchKernelGGL((k_init_p<double, false>), dim3(g), dim3(kBlock), 0, stream, n, (const double *)r, (const double *)w->invd.p,
                           (const uint16_t *)nullptr, p, xv, partial, (const PcgScalars *)sc);
    if constexpr (!MIXED) AVS_TRY(reduce_stage(w, g, 1, OP_RHO0, tol, 0, stream, dist));
    AVS_HIP(hipGetLastError());

    const bool use_graph = !dist && cur_opt().graph != 0;
    // the beta step rides in update_xp.  fp64: an option, and not with the RCCL transport (the sums are all-reduced between the two kernels)
    const bool fuse_beta = F32 || (!dist && cur_opt().fuse_beta != 0);
    // matrix + vectors fit the Infinity Cache (float vectors, half as large, more often): no non-temporal hints in the vector kernels
    const bool keep = A.keep_cached != 0;
    bool fuse_vec = false; // fp64: one launch for the two vector kernels (k_update_fused)
    if constexpr (!F32) AVS_TRY(fused_vectors_setup(w, A, x, g, fuse_beta, keep, stream, &fuse_vec));
    const long long fused_timeout = (long long)cur_opt().fused_timeout_ms * 100000ll; // wall_clock64: 100 MHz
#ifdef AVS_PROBES
    {
        const int solves = tl_phase_report.solves;
        tl_phase_report = avs_phase_loop_report{};
        tl_phase_report.solves = solves + 1;
        tl_phase_report.coded = coded, tl_phase_report.keep = keep, tl_phase_report.fuse_beta = fuse_beta, tl_phase_report.fuse_vectors = fuse_vec;
        tl_phase_report.g = g, tl_phase_report.float_vectors = MIXED ? 2 : (F32 ? 1 : 0);
    }
#endif
    auto enqueue_iteration = [&](int c, bool timed) -> avs_status {
        int nb = 0;
        if constexpr (!F32)
            if (dist) AVS_TRY(dist_halo_exchange(dist, p, stream));
        if (timed) AVS_HIP(hipEventRecord(w->evA[c], stream));
        AVS_TRY(product(std::true_type{}, p, t, &nb)); // tmp = A p ; p.tmp
        if (timed) AVS_HIP(hipEventRecord(w->evB[c], stream));
        // r.z alternates between two slots by the parity of the iteration -- every chunk starts at a multiple of kChunk (even; the
        // reliable update leaves r.z where position 0 reads it), so c & 1 IS that parity
        const int parity = fuse_beta ? (c & 1) : 0;
        const bool fuse_alpha = fuse_beta && nb <= kFuseAlphaMax; // few SpMV partials: every workgroup of update_r folds them itself
#ifdef AVS_PROBES
        tl_phase_report.nb = nb;
        tl_phase_folded = fuse_alpha; // (what the iterations of a replayed chunk count as)
        if (!tl_phase_capturing) ++(fuse_alpha ? tl_phase_report.alpha_folded : tl_phase_report.alpha_launched);
#endif
        double *vpart = (F32 || fuse_alpha) ? upper : partial;
        // the fused launch.  Where the SpMV leaves more partial sums than a workgroup folds for itself the alpha step stays a launch of
        // its own in front of it (nb = 0): only when the option is 1 -- "auto" (-1) takes the form that was measured
        const bool fused_launch = !F32 && fuse_vec && (fuse_alpha || cur_opt().fuse_vectors > 0);
        if (!fuse_alpha) AVS_TRY(reduce_stage(w, nb, 1, parity ? OP_ALPHA_ODD : OP_ALPHA, tol, 1, stream, dist));
        if constexpr (!F32)
            if (fused_launch) {
                w->fused_used = 1; // (every solve enqueues its first chunk launch by launch, so this runs in each that iterates)
                with_flags([&](auto C, auto K) {
                    hipLaunchKernelGGL((k_update_fused<C.value, K.value>), dim3(kVecGrid / 8), dim3(kFusedBlock), kFusedLds + (C.value ? kFusedTabBytes : 0),
                                       stream, n, x, p, r, t, inv, dcode, sc, vpart, partial, fuse_alpha ? nb : 0, parity, w->fused_bar.p, fused_timeout,
                                       A.table_size + 1);
                }, coded, keep);
                return AVS_OK;
            }
        const int r_parity = (F32 || fuse_alpha) ? parity : 0; // (the unfused fp64 kernel reads what OP_ALPHA left: no parity)
        with_flags([&](auto C, auto FA, auto K) {
            hipLaunchKernelGGL((k_update_r<T, S, C.value, FA.value, K.value>), dim3(g), dim3(kBlock), 0, stream, n, r, (const T *)t, (const T *)inv,
                               dcode, sc, vpart, FA.value ? (const double *)partial : nullptr, FA.value ? nb : 0, r_parity);
        }, coded, fuse_alpha, keep);
        if (!fuse_beta) AVS_TRY(reduce_stage(w, g, 2, OP_BETA, tol, 1, stream, dist));
        with_flags([&](auto C, auto FB, auto K) {
            constexpr bool FBK = F32 || FB.value; // (float vectors: fuse_beta is always set, and there is no other kernel)
            hipLaunchKernelGGL((k_update_xp<T, S, C.value, FBK, K.value>), dim3(g), dim3(kBlock), 0, stream, n, xv, p, (const T *)r, (const T *)inv, dcode,
                               sc, FBK ? (const double *)vpart : nullptr, FBK ? g : 0, parity);
        }, coded, fuse_beta, keep);
        return AVS_OK;
    };
    // MIXED: the reliable update, behind every chunk (plain launches: the fp64 product is not part of the captured chunk)
    auto enqueue_update = [&]() -> avs_status {
        if constexpr (MIXED) {
            hipLaunchKernelGGL(k_mixed_fold, dim3(g), dim3(kBlock), 0, stream, n, x, xv, (const PcgScalars *)sc);
            AVS_TRY(spmv_launch(A, x, t64, variant, stream));
            with_flags([&](auto C) {
                hipLaunchKernelGGL((k_mixed_residual<C.value, false>), dim3(g), dim3(kBlock), 0, stream, n, b, (const double *)t64, r, (const float *)inv,
                                   dcode, upper, (const PcgScalars *)sc);
            }, coded);
            hipLaunchKernelGGL(k_mixed_finish<false>, dim3(1), dim3(kRedBlock), 0, stream, (const double *)upper, g, sc, tol);
            with_flags([&](auto C) {
                hipLaunchKernelGGL(k_mixed_pstep<C.value>, dim3(g), dim3(kBlock), 0, stream, n, p, (const float *)r, (const float *)inv, dcode,
                                   (const PcgScalars *)sc);
            }, coded);
            AVS_HIP(hipGetLastError());
            w->reliable_updates++;
        }
        return AVS_OK;
    };
    GraphKey key = matrix_key(MIXED ? kGraphMixed : F32 ? kGraphF32 : kGraphF64, A, xv, tol);
    key.val = A.val;
    key.coded = coded;
    key.fuse_beta = fuse_beta;
    key.fuse_vec = fuse_vec;
    key.brick = F32 ? brick : A.brick != nullptr;
    ChunkState cs;
    bool cancelled = false;
    for (;;) {
        AVS_TRY(poll_scalars(w, sc, stream));
        sample_spmv(w, info != nullptr, false, &cs);
        const PcgScalars &h = *w->host_sc;
        if (MIXED && h.done == 0 && h.iter < cs.enqueued) cs.enqueued = h.iter; // a chunk the recurrence froze: its remaining iterations did not run
        if (h.done || cs.enqueued >= max_iters) break;
        // avs_cancel (single GPU: the host's poll is the only party to agree with).  Known gap: the RCCL standard-CG path (dist)
        // ignores it -- there is no all-rank vote here, so the request is neither consumed nor acted on
        if (!dist && cancel_consume()) { cancelled = true; break; }
        AVS_TRY(enqueue_chunk(w, stream, use_graph ? &key : nullptr, max_iters, info != nullptr, enqueue_iteration, &cs));
        AVS_TRY(enqueue_update()); // (MIXED) x += xf before the host looks: whatever ends the loop, x holds the last iterate
    }
    if constexpr (MIXED) {
        if (w->host_sc->done == 3) AVS_HIP(hipMemsetAsync(x, 0, (size_t)n * sizeof(double), stream)); // rhsNorm2 == 0 -> x.setZero()
    } else if constexpr (F32) {
        hipLaunchKernelGGL(k_f32_widen, dim3(g), dim3(kBlock), 0, stream, n, (const float *)xv, x);
    } else {
#ifdef AVS_PROBES
        if (fuse_vec && getenv("AVS_PCG_FUSED_FAKE_FAULT")) w->host_sc->fault = 4; // test hook of exactly the path below (probe build only)
#endif
        if (fuse_vec && w->host_sc->fault == 4) { // the fused launch's grid barrier timed out (GPU shared with other work): the solve again, from
            w->fused_off = true;                    // the initial guess, with the two vector launches -- on this workspace from now on
            w->fused_faults++;
            w->fused_used = 0;
            drop_graph(w);
            AVS_HIP(hipEventRecord(w->ev1, stream));
            AVS_HIP(hipEventSynchronize(w->ev1));
            float void_ms = 0.f;
            AVS_HIP(hipEventElapsedTime(&void_ms, w->ev0, w->ev1));
            w->fused_void_ms += void_ms;
            // (workgroups that gave up have left the counter between two multiples of the grid)
            AVS_HIP(hipMemsetAsync(w->fused_bar.p, 0, 2 * sizeof(unsigned long long), stream));
            AVS_HIP(hipMemcpyAsync(x, w->x_save.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream));
            return pcg_solve(w, A, b, x, tol, max_iters, stream, info, dist);
        }
    }
    return finish_info(w, A, stream, info, &cs, cancelled, 0, F32 && !MIXED);
}

avs_status pcg_solve(PcgWork *w, const CsrView &A, const double *b, double *x, double tol, int max_iters,
                     hipStream_t stream, avs_solve_info *info, PcgDist *dist)
{
    const int64_t n = A.n;
    AVS_REQUIRE(w && w->n == n, AVS_EINVAL, "pcg workspace does not match the system size");
    w->float_vectors = 0; // (the float loops set it)
    w->reliable_updates = 0;
    if (dist) {
        DirectArgs da;
        const bool direct = dist_direct_args(dist, &da);
        // AVS_OPTION_DIST_F32_VECTORS: the single-reduction loops on float vectors; AVS_DIST_CG=standard and paranoid mode stay fp64
        const bool paranoid = direct ? da.paranoid : cur_opt().paranoid != 0;
        if (A.f32_vectors > 0 && !cur_opt().dist_standard_cg && !paranoid)
            return direct ? pcg_solve_direct<float>(w, A, b, x, tol, max_iters, stream, info, da)
                          : pcg_solve_single_reduction<float>(w, A, b, x, tol, max_iters, stream, info, dist);
        // AVS_OPTION_DIST_MIXED_PRECISION (fp64 contexts; A.mixed is set from the plan's latch by avs_dist_solve only): the same loops on
        // float vectors with fp64 scalars and reliable updates, under the same conditions
        if (A.mixed && !cur_opt().dist_standard_cg && !paranoid && (direct || dist_wants_single_reduction(dist)))
            return direct ? pcg_solve_direct<float, true>(w, A, b, x, tol, max_iters, stream, info, da)
                          : pcg_solve_single_reduction<float, true>(w, A, b, x, tol, max_iters, stream, info, dist);
        if (direct) return pcg_solve_direct<double>(w, A, b, x, tol, max_iters, stream, info, da);
    }
    if (dist && dist_wants_single_reduction(dist))
        return pcg_solve_single_reduction<double>(w, A, b, x, tol, max_iters, stream, info, dist);
    // AVS_OPTION_RESIDENT_F32: a float-vector solve (f32_vectors 1 or -1) tries the resident loop on float vectors first
    const bool resident_f32 = !dist && A.resident_f32 && A.f32_vectors != 0;
    if (!dist && A.f32_vectors > 0 && !resident_f32) return pcg_solve_phases<float>(w, A, b, x, tol, max_iters, stream, info, nullptr); // AVS_PRECISION_F32: float vectors and scalars
    if (!dist && resident_wanted(false)) { // systems that fit on the chip (<= ~1 M rows, packed form): one cooperative launch
        bool ran = false;
        const avs_status rs = resident_f32 ? pcg_solve_resident_single<float>(w, A, b, x, tol, max_iters, stream, info, &ran)
                                           : pcg_solve_resident_single<double>(w, A, b, x, tol, max_iters, stream, info, &ran);
        if (ran || rs != AVS_OK) return rs;
    }
    if (!dist && A.f32_vectors != 0) return pcg_solve_phases<float>(w, A, b, x, tol, max_iters, stream, info, nullptr); // (auto, or a float resident loop that did not take it / faulted)
    if (!dist && A.mixed) return pcg_solve_phases<float, true>(w, A, b, x, tol, max_iters, stream, info, nullptr); // AVS_OPTION_MIXED_PRECISION: what the fp64 loop would run
    return pcg_solve_phases<double>(w, A, b, x, tol, max_iters, stream, info, dist);
}

#ifdef AVS_PROBES
// probe / test entry: one update_r launch followed by one update_xp launch of the launch-per-phase loops, any instantiation, on a grid
// of `g` workgroups and a caller's PcgScalars image (the loops reach g < kVecGrid only with one trip per thread, and KEEP = false only
// beyond the Infinity Cache)
template <typename T, typename S, bool CODED, bool FUSED, bool KEEP>
static void vector_probe(int g, int64_t n, int nb, int parity, T *x, T *p, T *r, const T *t, const T *invd, const uint16_t *dcode,
                         const double *spmv_partial, double *vpart, PcgScalars *sc, hipStream_t stream)
{
    // the unfused forms as pcg_solve_phases launches them.  fp64: OP_ALPHA / OP_BETA have left the scalars, no parity.  Float vectors:
    // there is no unfused k_update_xp -- OP_ALPHA, then both kernels with the iteration's parity
    constexpr bool F32 = std::is_same<T, float>::value, FX = FUSED || F32;
    hipLaunchKernelGGL((k_update_r<T, S, CODED, FUSED, KEEP>), dim3(g), dim3(kBlock), 0, stream, n, r, t, invd, dcode, sc, vpart,
                       FUSED ? spmv_partial : nullptr, FUSED ? nb : 0, FX ? parity : 0);
    hipLaunchKernelGGL((k_update_xp<T, S, CODED, FX, KEEP>), dim3(g), dim3(kBlock), 0, stream, n, x, p, (const T *)r, invd, dcode, sc,
                       FX ? (const double *)vpart : nullptr, FX ? g : 0, FX ? parity : 0);
}
__global__ __launch_bounds__(kBlock) void k_probe_max_code(int64_t n, const uint16_t *__restrict__ dcode, unsigned long long *__restrict__ top)
{
    unsigned long long m = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) m = m > dcode[i] ? m : dcode[i];
    if (m) atomicMax(top, m);
}
size_t vector_update_probe_scalars_size() { return sizeof(PcgScalars); }
avs_status vector_update_probe(int flags, int g, int64_t n, int nb, int parity, void *x, void *p, void *r, const void *t, const void *invd,
                               const uint16_t *dcode, const double *spmv_partial, double *vpart, void *scalars, hipStream_t stream)
{
    PcgScalars *sc = static_cast<PcgScalars *>(scalars);
    const bool ds = (flags & AVS_VECTOR_PROBE_DS) != 0, f32 = ds || (flags & AVS_VECTOR_PROBE_F32) != 0;
    if (flags & AVS_VECTOR_PROBE_ONE_LAUNCH) { // k_update_fused in place of the pair, as the fp64 loop launches it (the entry has checked the shape)
        const bool coded = (flags & AVS_VECTOR_PROBE_CODED) != 0;
        AVS_REQUIRE(fused_device_fits(), AVS_EINVAL, "the fused launch needs a CU per workgroup");
        AVS_TRY(fused_raise_lds());
        DevBuf<unsigned long long> bar; // [0] the barrier's counter, [1] the largest code
        AVS_TRY(bar.alloc(2));
        AVS_HIP(hipMemsetAsync(bar.p, 0, 2 * sizeof(unsigned long long), stream));
        int tab_n = 1;
        if (coded) { // the table has as many entries as the codes reach
            hipLaunchKernelGGL(k_probe_max_code, dim3(kVecGrid), dim3(kBlock), 0, stream, n, dcode, bar.p + 1);
            unsigned long long top = 0;
            AVS_HIP(hipMemcpyAsync(&top, bar.p + 1, sizeof(top), hipMemcpyDeviceToHost, stream));
            AVS_HIP(hipStreamSynchronize(stream));
            AVS_REQUIRE(top <= (unsigned long long)kViLdsTable, AVS_EINVAL, "the fused launch keeps at most 2049 dictionary entries");
            tab_n = (int)top + 1;
        }
        const long long timeout = (long long)cur_opt().fused_timeout_ms * 100000ll;
        with_flags([&](auto C, auto K) {
            hipLaunchKernelGGL((k_update_fused<C.value, K.value>), dim3(kVecGrid / 8), dim3(kFusedBlock), kFusedLds + (C.value ? kFusedTabBytes : 0),
                               stream, n, (double *)x, (double *)p, (double *)r, (const double *)t, (const double *)invd, dcode, sc, vpart, spmv_partial,
                               nb, parity, bar.p, timeout, tab_n);
        }, coded, (flags & AVS_VECTOR_PROBE_KEEP) != 0);
        AVS_HIP(hipGetLastError());
        AVS_HIP(hipStreamSynchronize(stream)); // (the counter goes with this call)
        return AVS_OK;
    }
    with_flags([&](auto C, auto F, auto K) {
        auto launch = [&](auto tv, auto sv) {
            typedef decltype(tv) T;
            vector_probe<T, decltype(sv), C.value, F.value, K.value>(g, n, nb, parity, (T *)x, (T *)p, (T *)r, (const T *)t, (const T *)invd, dcode,
                                                                     spmv_partial, vpart, sc, stream);
        };
        if (!f32) launch(0., 0.);
        else if (ds) launch(0.f, 0.);
        else launch(0.f, 0.f);
    }, (flags & AVS_VECTOR_PROBE_CODED) != 0, (flags & AVS_VECTOR_PROBE_FUSED) != 0, (flags & AVS_VECTOR_PROBE_KEEP) != 0);
    AVS_HIP(hipGetLastError());
    return AVS_OK;
}

// probe / test entry: the scalar stages of the loops on a caller's partial sums and PcgScalars image.  The loops reach k_reduce_mb only
// from 16,384 partial sums upward and the corners of apply_scalar_op only where a solve passes through them; this entry launches the same
// kernels at any count and from any state.  k_reduce_mb gets a staging array and a ticket laid out as pcg_create lays them out.
avs_status scalar_stage_probe(int which, const double *pa, int nb, int nred, const double *pb, int nbb, int nredb, int op, double tol,
                              int skip_if_done, int red_off, int launches, void *scalars, double *stage_out, unsigned *ticket_out,
                              hipStream_t stream)
{
    PcgScalars *sc = static_cast<PcgScalars *>(scalars);
    PcgWork w; // (only what reduce_launch reads)
    const bool multi = which == AVS_SCALAR_PROBE_REDUCE_LAUNCH || which == AVS_SCALAR_PROBE_REDUCE_MB;
    if (multi) {
        AVS_TRY(w.stage.alloc((size_t)kRedBlocks * 4));
        AVS_TRY(w.ticket.alloc(1));
        unsigned long long pattern[kRedBlocks * 4];
        for (int i = 0; i < kRedBlocks * 4; ++i) pattern[i] = AVS_SCALAR_PROBE_STAGE_NAN | (unsigned long long)i;
        AVS_HIP(hipMemcpyAsync(w.stage.p, pattern, sizeof(pattern), hipMemcpyHostToDevice, stream));
        AVS_HIP(hipMemsetAsync(w.ticket.p, 0, sizeof(unsigned), stream));
        AVS_HIP(hipStreamSynchronize(stream)); // (pattern leaves the stack)
    }
    for (int l = 0; l < launches; ++l) switch (which) {
        case AVS_SCALAR_PROBE_REDUCE_LAUNCH: reduce_launch(&w, pa, nb, nred, sc, op, tol, skip_if_done, red_off, stream); break;
        case AVS_SCALAR_PROBE_REDUCE:
            hipLaunchKernelGGL(k_reduce, dim3(1), dim3(kRedBlock), 0, stream, pa, nb, nred, sc, op, tol, skip_if_done, red_off);
            break;
        case AVS_SCALAR_PROBE_REDUCE_MB:
            hipLaunchKernelGGL(k_reduce_mb, dim3(kRedBlocks), dim3(kRedBlock), 0, stream, pa, nb, nred, sc, op, tol, skip_if_done, red_off, w.stage.p,
                               w.ticket.p);
            break;
        case AVS_SCALAR_PROBE_REDUCE_PAIR:
            hipLaunchKernelGGL(k_reduce_pair, dim3(1), dim3(kRedBlock), 0, stream, pa, nb, nred, pb, nbb, nredb, sc);
            break;
        case AVS_SCALAR_PROBE_SCALAR: hipLaunchKernelGGL(k_scalar, dim3(1), dim3(64), 0, stream, sc, op, tol); break;
        case AVS_SCALAR_PROBE_MIXED_FINISH_INIT: hipLaunchKernelGGL(k_mixed_finish<true>, dim3(1), dim3(kRedBlock), 0, stream, pa, nb, sc, tol); break;
        case AVS_SCALAR_PROBE_MIXED_FINISH: hipLaunchKernelGGL(k_mixed_finish<false>, dim3(1), dim3(kRedBlock), 0, stream, pa, nb, sc, tol); break;
        case AVS_SCALAR_PROBE_SR_MIXED_BEGIN: hipLaunchKernelGGL(k_sr_mixed_begin, dim3(1), dim3(1), 0, stream, sc); break;
        default: hipLaunchKernelGGL(k_sr_mixed_step, dim3(1), dim3(1), 0, stream, sc); break;
        }
    AVS_HIP(hipGetLastError());
    if (ticket_out) *ticket_out = 0u;
    if (multi) { // (the workspace goes with this call: wait for the launches either way)
        if (stage_out) AVS_HIP(hipMemcpyAsync(stage_out, w.stage.p, (size_t)kRedBlocks * 4 * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (ticket_out) AVS_HIP(hipMemcpyAsync(ticket_out, w.ticket.p, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
        AVS_HIP(hipStreamSynchronize(stream));
    }
    return AVS_OK;
}

// probe / test entry: one launch of a vector kernel of the single-reduction loops, any instantiation the loops make, on `g` workgroups
// (the loops reach a second trip per thread only above 524,288 rows, and never a workgroup without rows)
template <typename T, bool CODED>
static void sr_vector_probe_t(int kernel, bool ds, int g, int64_t n, const double *b, T *x, T *r, T *p, T *s, T *u, const T *wv, const T *invd,
                              const uint16_t *dcode, const PcgScalars *in, PcgScalars *out, int step, double *partial, hipStream_t stream)
{
    constexpr bool F32 = std::is_same<T, float>::value;
    if (kernel == AVS_SR_PROBE_INIT)
        hipLaunchKernelGGL((k_sr_init<T, F32 && CODED>), dim3(g), dim3(kBlock), 0, stream, n, b, wv, invd, dcode, r, u, partial);
    else if constexpr (F32) {
        if (ds) hipLaunchKernelGGL((k_sr_update<float, CODED, double>), dim3(g), dim3(kBlock), 0, stream, n, x, r, p, s, u, wv, invd, dcode, in, out, step, partial);
        else hipLaunchKernelGGL((k_sr_update<float, CODED, float>), dim3(g), dim3(kBlock), 0, stream, n, x, r, p, s, u, wv, invd, dcode, in, out, step, partial);
    } else
        hipLaunchKernelGGL((k_sr_update<double, false, double>), dim3(g), dim3(kBlock), 0, stream, n, x, r, p, s, u, wv, invd, dcode, in, out, step, partial);
}
avs_status sr_vector_probe(int kernel, int flags, int g, int64_t n, const double *b, void *x, void *r, void *p, void *s, void *u, const void *wv,
                           const void *invd, const uint16_t *dcode, const void *scalars_in, void *scalars_out, int step, double *partial,
                           hipStream_t stream)
{
    const PcgScalars *in = static_cast<const PcgScalars *>(scalars_in);
    PcgScalars *out = static_cast<PcgScalars *>(scalars_out);
    const bool ds = (flags & AVS_VECTOR_PROBE_DS) != 0, f32 = ds || (flags & AVS_VECTOR_PROBE_F32) != 0;
    with_flags([&](auto C) {
        if (kernel == AVS_SR_PROBE_MIXED_RESIDUAL || kernel == AVS_SR_PROBE_MIXED_RESIDUAL_INIT)
            with_flags([&](auto I) {
                hipLaunchKernelGGL((k_sr_mixed_residual<C.value, I.value>), dim3(g), dim3(kBlock), 0, stream, n, b, (const double *)wv, (float *)r,
                                   (float *)u, (const float *)invd, dcode, partial, in);
            }, kernel == AVS_SR_PROBE_MIXED_RESIDUAL_INIT);
        else if (f32)
            sr_vector_probe_t<float, C.value>(kernel, ds, g, n, b, (float *)x, (float *)r, (float *)p, (float *)s, (float *)u, (const float *)wv,
                                              (const float *)invd, dcode, in, out, step, partial, stream);
        else
            sr_vector_probe_t<double, false>(kernel, false, g, n, b, (double *)x, (double *)r, (double *)p, (double *)s, (double *)u,
                                             (const double *)wv, (const double *)invd, dcode, in, out, step, partial, stream);
    }, (flags & AVS_VECTOR_PROBE_CODED) != 0);
    AVS_HIP(hipGetLastError());
    return AVS_OK;
}

#endif

} // namespace avs

#ifdef AVS_PROBES
extern "C" avs_status avs_phase_loop_info(avs_phase_loop_report *report)
{
    AVS_REQUIRE(report && report->struct_size >= 8, AVS_EINVAL, "report: struct_size not set");
    avs_phase_loop_report o = avs::tl_phase_report;
    const size_t nbytes = (size_t)report->struct_size < sizeof(o) ? (size_t)report->struct_size : sizeof(o);
    o.struct_size = (int32_t)nbytes;
    memcpy(report, &o, nbytes);
    return AVS_OK;
}

extern "C" avs_status avs_vector_update_probe(int32_t flags, int32_t g, int64_t n, int32_t nb, int32_t parity, void *x, void *p, void *r,
                                              const void *t, const void *invd, const uint16_t *dcode, const double *spmv_partial,
                                              double *vpart, void *scalars, int32_t scalars_bytes, void *stream)
{
    AVS_REQUIRE(x && p && r && t && invd && vpart && scalars && n > 0 && g >= 1 && g <= 2048 && nb >= 0, AVS_EINVAL, "bad argument");
    AVS_REQUIRE((parity == 0 || parity == 1) && (dcode || !(flags & AVS_VECTOR_PROBE_CODED)) && (spmv_partial || !(flags & AVS_VECTOR_PROBE_FUSED)),
                AVS_EINVAL, "bad argument");
    AVS_REQUIRE((size_t)scalars_bytes == avs::vector_update_probe_scalars_size(), AVS_EINVAL, "the scalars image has another size");
    if (flags & AVS_VECTOR_PROBE_ONE_LAUNCH) { // refused on the host, before any launch: what the loop's dispatch never hands the fused kernel
        AVS_REQUIRE((flags & AVS_VECTOR_PROBE_FUSED) && !(flags & (AVS_VECTOR_PROBE_F32 | AVS_VECTOR_PROBE_DS)), AVS_EINVAL,
                    "one launch: fp64 and the fused scalar steps only");
        AVS_REQUIRE(g == 2048 && n >= 2 && n <= (int64_t)8388608 && nb >= 1 && nb <= 4096, AVS_EINVAL,
                    "one launch: 2048 emulated workgroups, at most 8,388,608 rows, 1 .. 4096 partial sums");
    }
    return avs::vector_update_probe(flags, g, n, nb, parity, x, p, r, t, invd, dcode, spmv_partial, vpart, scalars,
                                    reinterpret_cast<hipStream_t>(stream));
}

extern "C" avs_status avs_pcg_scalar_probe(int32_t which, const double *partial, int32_t nb, int32_t nred, const double *partial_b, int32_t nb_b,
                                           int32_t nred_b, int32_t op, double tol, int32_t skip_if_done, int32_t red_off, int32_t launches,
                                           void *scalars, int32_t scalars_bytes, double *stage_out, uint32_t *ticket_out, void *stream)
{
    AVS_REQUIRE(which >= AVS_SCALAR_PROBE_REDUCE_LAUNCH && which <= AVS_SCALAR_PROBE_SR_MIXED_STEP && scalars && launches >= 1 && launches <= 16,
                AVS_EINVAL, "bad argument");
    AVS_REQUIRE((size_t)scalars_bytes == avs::vector_update_probe_scalars_size(), AVS_EINVAL, "the scalars image has another size");
    AVS_REQUIRE(op >= 0 && op <= 9, AVS_EINVAL, "no such scalar op");
    if (which <= AVS_SCALAR_PROBE_REDUCE_PAIR) {
        const bool pair = which == AVS_SCALAR_PROBE_REDUCE_PAIR;
        AVS_REQUIRE(partial && nb >= (which == AVS_SCALAR_PROBE_REDUCE_MB ? 1 : 0) && nred >= 0 && red_off >= 0, AVS_EINVAL, "bad partial sums");
        AVS_REQUIRE(!pair || (partial_b && nb_b >= 0 && nred_b >= 0 && red_off == 0), AVS_EINVAL, "bad second set of partial sums");
        AVS_REQUIRE(red_off + nred + (pair ? nred_b : 0) <= 4, AVS_EINVAL, "the sums do not fit red[4]");
    } else if (which == AVS_SCALAR_PROBE_MIXED_FINISH_INIT || which == AVS_SCALAR_PROBE_MIXED_FINISH) {
        AVS_REQUIRE(partial && nb >= 0, AVS_EINVAL, "bad partial sums");
    }
    return avs::scalar_stage_probe(which, partial, nb, nred, partial_b, nb_b, nred_b, op, tol, skip_if_done, red_off, launches, scalars, stage_out,
                                   ticket_out, reinterpret_cast<hipStream_t>(stream));
}

extern "C" avs_status avs_sr_vector_probe(int32_t kernel, int32_t flags, int32_t g, int64_t n, const double *b, void *x, void *r, void *p, void *s,
                                          void *u, const void *w, const void *invd, const uint16_t *dcode, const void *scalars_in,
                                          void *scalars_out, int32_t scalars_bytes, int32_t step, double *partial, void *stream)
{
    const bool update = kernel == AVS_SR_PROBE_UPDATE, mixed = kernel == AVS_SR_PROBE_MIXED_RESIDUAL || kernel == AVS_SR_PROBE_MIXED_RESIDUAL_INIT;
    const bool f32 = (flags & (AVS_VECTOR_PROBE_F32 | AVS_VECTOR_PROBE_DS)) != 0;
    AVS_REQUIRE(kernel >= AVS_SR_PROBE_INIT && kernel <= AVS_SR_PROBE_MIXED_RESIDUAL_INIT && n > 0 && g >= 1 && g <= 2048, AVS_EINVAL, "bad argument");
    AVS_REQUIRE((flags & ~(AVS_VECTOR_PROBE_F32 | AVS_VECTOR_PROBE_DS | AVS_VECTOR_PROBE_CODED)) == 0, AVS_EINVAL, "no such flag");
    AVS_REQUIRE(!(flags & AVS_VECTOR_PROBE_DS) || update, AVS_EINVAL, "float vectors with double scalars: k_sr_update only");
    AVS_REQUIRE(!(flags & AVS_VECTOR_PROBE_F32) || !mixed, AVS_EINVAL, "k_sr_mixed_residual has one type form");
    AVS_REQUIRE(!(flags & AVS_VECTOR_PROBE_CODED) || ((f32 || mixed) && dcode), AVS_EINVAL, "diagonal codes: the float forms only");
    AVS_REQUIRE(r && u && w && invd && partial && (update || b) && (!update || (x && p && s)), AVS_EINVAL, "bad argument");
    AVS_REQUIRE(kernel == AVS_SR_PROBE_INIT || scalars_in, AVS_EINVAL, "bad argument");
    AVS_REQUIRE(!update || (scalars_out && (step == 0 || (step == 1 && scalars_out != scalars_in))), AVS_EINVAL, "bad scalar states");
    AVS_REQUIRE((size_t)scalars_bytes == avs::vector_update_probe_scalars_size(), AVS_EINVAL, "the scalars image has another size");
    return avs::sr_vector_probe(kernel, flags, g, n, b, x, r, p, s, u, w, invd, dcode, scalars_in, scalars_out, step, partial,
                                reinterpret_cast<hipStream_t>(stream));
}
#endif // AVS_PROBES
