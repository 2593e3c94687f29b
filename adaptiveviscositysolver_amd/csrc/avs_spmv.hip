// avs_spmv.hip -- the fp64 matrix-vector products on the caller's CSR and its lossless compressed forms (value-indexed, packed, tile
// tables, windowed columns: avs_reorder.hip builds them) for gfx950 (MI355X), with the partial sums of x.Ax the PCG loops fold
// (avs_pcg.hip).  The brick-structured form has its own file (avs_brick.hip); spmv_dispatch hands over to it.
// Reference: Eigen's `mat * p` inside ConjugateGradient (cpp:618-630 of HDK_AdaptiveViscosity.cpp).
//
// Roofline: every kernel here is HBM-bound.  Algorithmic bytes per SpMV launch:
//   12*nnz + 4*(n+1) + 16*n      (fp64 values, int32 columns / row pointers)
//
// SpMV kernels
//   variant 1  "stream": a 256-thread workgroup owns 256 consecutive rows.  Phase 1 streams the
//              rows' (val, col) pairs with fully coalesced loads, gathers x[col] and parks the
//              products in LDS; phase 2: one thread per row adds its LDS segment left to right
//              (the same order as the CPU oracle => bit-identical y).  Row stride ~15 doubles is
//              bank-conflict-free for ds_read_b64 (30*t mod 64 distinct for t < 32).
//   variant 2-4 "vector": 4 / 8 / 16 lanes per row, shuffle reduction.
#include "avs_internal.hpp"
#include "avs_halo.hpp"
#include "avs_wave.hpp"

namespace avs {

// ---------------------------------------------------------------------------------------------
// SpMV: stream variant
// ---------------------------------------------------------------------------------------------
template <bool DOT>
__global__ __launch_bounds__(kBlock) void k_spmv_stream(CsrView A, const double *__restrict__ x,
                                                        double *__restrict__ y,
                                                        double *__restrict__ partial,
                                                        const PcgScalars *sc)
{
    if (DOT && sc && sc->done) return;
    __shared__ double prod[kStreamCap];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kBlock;
    const int64_t row = row0 + tid;
    const int64_t rlast = (row0 + kBlock < A.n) ? row0 + kBlock : A.n;
    const int s_blk = A.row_ptr[row0];
    const int e_blk = A.row_ptr[rlast];
    int rs = 0, re = 0;
    if (row < A.n) {
        rs = A.row_ptr[row];
        re = A.row_ptr[row + 1];
    }
    double sum = 0.;
    for (int ts = s_blk; ts < e_blk; ts += kStreamCap) {
        const int te = (ts + kStreamCap < e_blk) ? ts + kStreamCap : e_blk;
        // phase 1: coalesced stream of (val, col), gather x, products to LDS.  4 independent
        // loads per thread in flight per trip.
        int k = ts + tid;
        for (; k + 3 * kBlock < te; k += 4 * kBlock) {
            const double v0 = A.val[k], v1 = A.val[k + kBlock], v2 = A.val[k + 2 * kBlock], v3 = A.val[k + 3 * kBlock];
            const int c0 = A.col[k], c1 = A.col[k + kBlock], c2 = A.col[k + 2 * kBlock], c3 = A.col[k + 3 * kBlock];
            const double x0 = x[c0], x1 = x[c1], x2 = x[c2], x3 = x[c3];
            prod[k - ts] = v0 * x0;
            prod[k - ts + kBlock] = v1 * x1;
            prod[k - ts + 2 * kBlock] = v2 * x2;
            prod[k - ts + 3 * kBlock] = v3 * x3;
        }
        for (; k < te; k += kBlock) prod[k - ts] = A.val[k] * x[A.col[k]];
        __syncthreads();
        // phase 2: each row adds its part of the tile, left to right
        const int a = rs > ts ? rs : ts;
        const int b = re < te ? re : te;
        for (int j = a; j < b; ++j) sum += prod[j - ts];
        __syncthreads();
    }
    if (row < A.n) y[row] = sum;
    if (DOT) {
        double d = (row < A.n) ? sum * x[row] : 0.;
        d = block_sum(d, red);
        if (tid == 0) partial[blockIdx.x] = d;
    }
}


// ---------------------------------------------------------------------------------------------
// SpMV: generic tile kernel for tuning.  One block = BLK rows; knobs: LDS capacity CAP, 16-B/8-B
// vector streaming (VEC), XCD-contiguous tile ownership (XCD: block b -> XCD b % 8 by the observed
// dispatch rule; each XCD then owns a contiguous eighth of the rows so x gathers of neighbouring
// tiles share one L2 -- used for speed only, never for correctness).
// ---------------------------------------------------------------------------------------------
template <int BLK, int CAP, bool DOT, bool VEC, bool XCD, bool NT, bool HALO = false>
__global__ __launch_bounds__(BLK) void k_spmv_tile(CsrView A, const double *__restrict__ xin,
                                                   double *__restrict__ y, double *__restrict__ partial,
                                                   const PcgScalars *sc, int chunk, const int32_t *__restrict__ tiles = nullptr,
                                                   HaloView hv = HaloView())
{
    if (DOT && sc && sc->done) return;
    __shared__ double prod[CAP + 2];
    __shared__ double red[BLK / 64];
    const int tid = threadIdx.x;
    // halo-touching launch of the direct transport: columns >= n_own live in the comm block's halo area
    struct Gather {
        const double *x, *hx;
        int n_own;
        __device__ __forceinline__ double operator[](int c) const { return (HALO && c >= n_own) ? ld_sys_f64(hx + (c - n_own)) : x[c]; }
    };
    const Gather x{xin, HALO ? hv.dd->my_halo : nullptr, HALO ? (int)hv.dd->n_own : 0};
    if (HALO) {
        if ((int)blockIdx.x >= hv.ntiles) { halo_finalizer<BLK>(hv, (int)blockIdx.x - hv.ntiles); return; }
        if (hv.tile_bnd[blockIdx.x]) halo_wait(hv); // block-uniform
    }
    int64_t tile = tiles ? (int64_t)tiles[blockIdx.x] : (int64_t)blockIdx.x; // tile lists: interior / halo-touching subsets
    if (XCD) {
        const int64_t ntiles = gridDim.x;
        if (chunk <= 0) { // each XCD owns one contiguous eighth
            const int64_t per = ntiles >> 3, rem = ntiles & 7;
            const int q = blockIdx.x & 7;
            const int64_t slot = blockIdx.x >> 3;
            tile = (int64_t)q * per + (q < rem ? q : rem) + slot;
        } else { // XCDs take turns on chunks of `chunk` consecutive tiles (one moving window)
            const int64_t super = (int64_t)chunk * 8;
            const int64_t full = (ntiles / super) * super; // tail keeps the identity mapping
            if (tile < full) {
                const int64_t sb = tile / super, r = tile % super;
                const int q = (int)(r & 7);
                const int64_t slot = r >> 3;
                tile = sb * super + (int64_t)q * chunk + slot;
            }
        }
    }
    const int64_t row0 = tile * BLK;
    const int64_t row = row0 + tid;
    const int64_t rlast = (row0 + BLK < A.n) ? row0 + BLK : A.n;
    const int s_blk = A.row_ptr[row0];
    const int e_blk = A.row_ptr[rlast];
    int rs = 0, re = 0;
    if (row < A.n) {
        rs = A.row_ptr[row];
        re = A.row_ptr[row + 1];
    }
    double sum = 0.;
    for (int ts = s_blk; ts < e_blk; ts += CAP) {
        const int te = (ts + CAP < e_blk) ? ts + CAP : e_blk;
        int base;
        if (VEC) {
            base = ts & ~1;          // even => 16-B aligned doubles, 8-B aligned ints
            const int te2 = te & ~1; // pairs fully below te
            int k = base + 2 * tid;
            for (; k + 2 * BLK < te2; k += 4 * BLK) {
                const d2_t v0 = stream_load<NT>(reinterpret_cast<const d2_t *>(A.val + k));
                const d2_t v1 = stream_load<NT>(reinterpret_cast<const d2_t *>(A.val + k + 2 * BLK));
                const i2_t c0 = stream_load<NT>(reinterpret_cast<const i2_t *>(A.col + k));
                const i2_t c1 = stream_load<NT>(reinterpret_cast<const i2_t *>(A.col + k + 2 * BLK));
                const double x00 = x[c0.x], x01 = x[c0.y], x10 = x[c1.x], x11 = x[c1.y];
                prod[k - base] = v0.x * x00;
                prod[k - base + 1] = v0.y * x01;
                prod[k - base + 2 * BLK] = v1.x * x10;
                prod[k - base + 2 * BLK + 1] = v1.y * x11;
            }
            for (; k < te2; k += 2 * BLK) {
                const d2_t v0 = stream_load<NT>(reinterpret_cast<const d2_t *>(A.val + k));
                const i2_t c0 = stream_load<NT>(reinterpret_cast<const i2_t *>(A.col + k));
                prod[k - base] = v0.x * x[c0.x];
                prod[k - base + 1] = v0.y * x[c0.y];
            }
            if (tid == 0 && (te & 1)) prod[te - 1 - base] = A.val[te - 1] * x[A.col[te - 1]];
        } else {
            base = ts;
            int k = ts + tid;
            for (; k + 3 * BLK < te; k += 4 * BLK) {
                const double v0 = stream_load<NT>(A.val + k), v1 = stream_load<NT>(A.val + k + BLK),
                             v2 = stream_load<NT>(A.val + k + 2 * BLK), v3 = stream_load<NT>(A.val + k + 3 * BLK);
                const int c0 = stream_load<NT>(A.col + k), c1 = stream_load<NT>(A.col + k + BLK),
                          c2 = stream_load<NT>(A.col + k + 2 * BLK), c3 = stream_load<NT>(A.col + k + 3 * BLK);
                const double x0 = x[c0], x1 = x[c1], x2 = x[c2], x3 = x[c3];
                prod[k - ts] = v0 * x0;
                prod[k - ts + BLK] = v1 * x1;
                prod[k - ts + 2 * BLK] = v2 * x2;
                prod[k - ts + 3 * BLK] = v3 * x3;
            }
            for (; k < te; k += BLK) prod[k - ts] = stream_load<NT>(A.val + k) * x[stream_load<NT>(A.col + k)];
        }
        __syncthreads();
        const int a = rs > ts ? rs : ts;
        const int b = re < te ? re : te;
        for (int j = a; j < b; ++j) sum += prod[j - base];
        __syncthreads();
    }
    if (row < A.n) {
        if (NT) __builtin_nontemporal_store(sum, y + row);
        else y[row] = sum;
    }
    if (DOT) {
        double d = (row < A.n) ? sum * xin[row] : 0.;
        d = wave_sum(d);
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = d;
        __syncthreads();
        if (tid == 0) {
            double t = 0.;
            for (int w = 0; w < BLK / 64; ++w) t += red[w];
            if (!HALO) partial[blockIdx.x] = t; // slot = position in the launch (== tile without a tile list)
            else __hip_atomic_store(hv.stage + tile, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // fire and forget, see halo_finalizer
        }
    }
}

// ---------------------------------------------------------------------------------------------
// SpMV: vector variants (LPR lanes per row)
// ---------------------------------------------------------------------------------------------
template <int LPR, bool DOT>
__global__ __launch_bounds__(kBlock) void k_spmv_vec(CsrView A, const double *__restrict__ x,
                                                     double *__restrict__ y,
                                                     double *__restrict__ partial,
                                                     const PcgScalars *sc)
{
    if (DOT && sc && sc->done) return;
    __shared__ double red[4];
    const int sub = threadIdx.x % LPR;
    const int64_t group = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LPR;
    const int64_t ngroups = (int64_t)gridDim.x * kBlock / LPR;
    double dot = 0.;
    for (int64_t row = group; row < A.n; row += ngroups) {
        const int s = A.row_ptr[row], e = A.row_ptr[row + 1];
        double sum = 0.;
        for (int k = s + sub; k < e; k += LPR) sum += A.val[k] * x[A.col[k]];
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) sum += __shfl_down(sum, o, LPR);
        if (sub == 0) {
            y[row] = sum;
            if (DOT) dot += sum * x[row];
        }
    }
    if (DOT) {
        dot = block_sum(dot, red);
        if (threadIdx.x == 0) partial[blockIdx.x] = dot;
    }
}

// ---------------------------------------------------------------------------------------------
// SpMV on the value-indexed matrix (CsrView::codes / table): same tile structure as k_spmv_tile, but the
// stream is (uint16 code, int32 col) = 6 B per non-zero instead of 12 B, and the value comes from the
// dictionary -- staged in LDS when it has at most TBL entries (the uniform-coefficient case: ~100
// entries), read through L1/L2 otherwise.  val == table[code] bit for bit, so products, their order and
// the row sums are those of the plain kernel.
// ---------------------------------------------------------------------------------------------
// Every lane issues ALL of its quad loads for the pass (8-B code quad + 16-B column quad, or one 16-B quad of
// packed words), then ALL 4*U gathers of x, before the first product is formed; products are parked with 16-B LDS
// stores.  Row sums stay left-to-right (oracle order).  U = CAP / (4 BLK) = 2 with 32 waves per CU is the measured
// optimum (profiles/r01_spmv_variants.md): U = 4 needs 70 VGPRs and twice the LDS, which halves the resident waves.
// TLT > 0: tile-local dictionaries (CsrView::tab_ptr): the tile's own table is staged in LDS (its first TLT entries; a tile with
// more distinct values takes a separate path that reads the rest through L1), codes are tile-local.
// CWIN: windowed columns (CsrView::cbase): one 32-bit word per non-zero = code << 20 | window slot << 14 | offset.
template <int BLK, int CAP, bool DOT, bool LTAB, bool PACK, int WIN = 0, int TLT = 0, bool HALO = false, bool CWIN = false, bool KEEPW = false>
__global__ __launch_bounds__(BLK) void k_spmv_vi2(CsrView A, const double *__restrict__ x, double *__restrict__ y,
                                                  double *__restrict__ partial, const PcgScalars *sc,
                                                  const int32_t *__restrict__ tiles, HaloView hv = HaloView())
{
    if (DOT && sc && sc->done) return;
    if (HALO) {
        if ((int)blockIdx.x >= hv.ntiles) { halo_finalizer<BLK>(hv, (int)blockIdx.x - hv.ntiles); return; }
        if (hv.tile_bnd[blockIdx.x]) halo_wait(hv); // block-uniform
    }
    const double *__restrict__ hx = HALO ? hv.dd->my_halo : nullptr;
    const int n_own_cols = HALO ? (int)hv.dd->n_own : 0;
    constexpr int U = CAP / (4 * BLK); // quads per lane per pass
    static_assert(U >= 1 && U * 4 * BLK == CAP, "CAP must be a multiple of 4*BLK");
    static_assert(TLT == 0 || (!LTAB && !PACK && BLK == 512), "tile tables: 512-row tiles, no plain packing");
    static_assert(!CWIN || (!PACK && BLK == 512), "windowed columns: 512-row tiles");
    constexpr bool WORDS = PACK || CWIN; // the stream is one 32-bit word per non-zero
    constexpr bool PREF = WORDS;         // prefetch the next pass's words during this one (4 dwords per quad; the 6-B form would need 6)
    extern __shared__ __attribute__((aligned(16))) double smem[];
    static_assert(WIN == 0 || (WIN >= BLK && WIN % BLK == 0), "window = a whole number of tiles");
    double *prod = smem;                 // CAP + 4
    double *xs = smem + CAP + 4;                           // WIN entries of x around the tile's rows
    int *cb = reinterpret_cast<int *>(smem + CAP + 4 + WIN); // CWIN: the tile's 64 window bases
    double *tbl = smem + CAP + 4 + WIN + (CWIN ? kCwinSlots / 2 : 0); // table_size (LTAB) / TLT entries (tile tables)
    const int tid = threadIdx.x;
    const int64_t tile = tiles ? (int64_t)tiles[blockIdx.x] : (int64_t)blockIdx.x;
    if (CWIN && tid < kCwinSlots) cb[tid] = A.cbase[tile * kCwinSlots + tid];
    const double *__restrict__ gtab = A.table;
    int tlen = A.table_size;
    if (TLT > 0) {
        const int t0 = A.tab_ptr[tile];
        gtab = A.table + t0;
        tlen = A.tab_ptr[tile + 1] - t0;
        if (tlen > TLT) tlen = TLT;
    }
    // Tile tables: the first TLT entries are in LDS.  The rare tile with more distinct values reads the rest through L1 -- on a
    // path of its own (`big`, wave-uniform), so that the common tile carries no global load (and no s_waitcnt on it) per product.
    bool big = false;
    if (TLT > 0) big = (A.tab_ptr[tile + 1] - A.tab_ptr[tile]) > TLT;
    auto value = [&](unsigned code) -> double { return (LTAB || TLT > 0) ? tbl[code] : gtab[code]; };
    auto value_big = [&](unsigned code) -> double { return code < (unsigned)TLT ? tbl[code] : gtab[code]; };
    const int64_t row0 = tile * BLK;
    const int64_t row = row0 + tid;
    const int64_t rlast = (row0 + BLK < A.n) ? row0 + BLK : A.n;
    // x window: 43 % (WIN = 256) / 58 % (512) of a tile's columns lie within WIN entries of its rows in the brick-major
    // numbering; those gathers are served from LDS instead of one L1 access each
    int w0 = 0;
    unsigned wlen = 0;
    if (WIN > 0) {
        const int64_t lo = row0 - (WIN - BLK) / 2;
        w0 = (int)(lo > 0 ? lo : 0);
        const int64_t left = A.n - w0;
        wlen = (unsigned)(left < WIN ? left : WIN);
#pragma unroll
        for (int i = 0; i < WIN / BLK; ++i) {
            const unsigned o = (unsigned)(tid + i * BLK);
            if (o < wlen) xs[o] = x[(int64_t)w0 + o];
        }
    }
    auto gather = [&](int col) -> double {
        if (WIN > 0 && !HALO) {
            // Both reads are issued for every lane, from a clamped address, and the value is selected afterwards.  As two exec-masked
            // branches writing ONE register the compiler put an `s_waitcnt lgkmcnt(0)` between the LDS read and the global load of every
            // gather (write-after-write on the destination): the eight global gathers of a pass went out one LDS round trip apart.
            const unsigned off = (unsigned)(col - w0);
            const bool in = off < wlen;
            const double a = xs[in ? off : 0u];
            const double b = x[in ? w0 : col];
            return in ? a : b;
        }
        if (WIN > 0) {
            const unsigned off = (unsigned)(col - w0);
            if (off < wlen) return xs[off];
        }
        if (HALO && col >= n_own_cols) return ld_sys_f64(hx + (col - n_own_cols)); // the comm block's halo area, written by the peers
        return x[col];
    };
    // the matrix stream of a pass: every lane's quads are requested in one go ...
    u4_t qn[U]; // value codes (WORDS: whole words, split at use)
    i4_t cn[U];
    auto request = [&](int ts, int e_blk) {
        const int te = (ts + CAP < e_blk) ? ts + CAP : e_blk;
        const int base = ts & ~3, te4 = te & ~3;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kk = base + 4 * (tid + u * BLK);
            qn[u] = u4_t{0, 0, 0, 0};
            cn[u] = i4_t{0, 0, 0, 0};
            if (kk < te4) {
                if (WORDS) {
                    qn[u] = stream_load_k<KEEPW>(reinterpret_cast<const u4_t *>(A.packed + kk));
                } else {
                    const us4_t h = stream_load_k<KEEPW>(reinterpret_cast<const us4_t *>(A.codes + kk));
                    qn[u] = u4_t{h.x, h.y, h.z, h.w};
                    cn[u] = stream_load_k<KEEPW>(reinterpret_cast<const i4_t *>(A.col + kk));
                }
            }
        }
    };
    const int s_blk = A.row_ptr[row0];
    const int e_blk = A.row_ptr[rlast];
    // ... and the FIRST pass is requested before the tile's tables / x window are staged: their latency (two dependent global
    // round trips for a tile-local dictionary) hides behind the stream instead of delaying it
    request(s_blk, e_blk);
    if (LTAB || TLT > 0)
        for (int i = tid; i < tlen; i += BLK) tbl[i] = gtab[i];
    int rs = 0, re = 0;
    double xr = 0.;
    if (row < A.n) {
        rs = A.row_ptr[row];
        re = A.row_ptr[row + 1];
        if (DOT && WIN == 0) xr = x[row]; // early: its latency hides behind the passes
    }
    if (LTAB || WIN > 0 || TLT > 0 || CWIN) __syncthreads();
    if (DOT && WIN > 0 && row < A.n) xr = xs[(int)(row - w0)]; // the tile's own rows are always inside the window
    double sum = 0.;
    for (int ts = s_blk; ts < e_blk; ts += CAP) {
        const int te = (ts + CAP < e_blk) ? ts + CAP : e_blk;
        const int base = ts & ~3; // 8-B aligned code quads, 16-B aligned column quads
        const int te4 = te & ~3;  // quads fully below te
        u4_t q[U];
        i4_t c[U];
        double xv[U][4];
        const unsigned cmask = PACK ? ((1u << A.col_bits) - 1u) : 0u;
        const int cbits = PACK ? A.col_bits : 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            q[u] = qn[u];
            c[u] = cn[u];
        }
        if (PREF && te < e_blk) request(te, e_blk); // software pipeline: the next pass travels while this one is multiplied
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kk = base + 4 * (tid + u * BLK);
            if (kk < te4) {
                if (PACK) {
                    c[u] = i4_t{(int)(q[u].x & cmask), (int)(q[u].y & cmask), (int)(q[u].z & cmask), (int)(q[u].w & cmask)};
                    q[u] = u4_t{q[u].x >> cbits, q[u].y >> cbits, q[u].z >> cbits, q[u].w >> cbits};
                }
                if (CWIN) {
                    constexpr unsigned om = (1u << kCwinOffBits) - 1u, sm = kCwinSlots - 1u;
                    c[u] = i4_t{cb[(q[u].x >> kCwinOffBits) & sm] + (int)(q[u].x & om), cb[(q[u].y >> kCwinOffBits) & sm] + (int)(q[u].y & om),
                                cb[(q[u].z >> kCwinOffBits) & sm] + (int)(q[u].z & om), cb[(q[u].w >> kCwinOffBits) & sm] + (int)(q[u].w & om)};
                    constexpr int sh = kCwinOffBits + kCwinSlotBits;
                    q[u] = u4_t{q[u].x >> sh, q[u].y >> sh, q[u].z >> sh, q[u].w >> sh};
                }
                if ((CWIN || TLT > 0) && kk < ts) {
                    // Head of the first pass: the aligned quad starts up to 3 entries BEFORE the tile's first non-zero.  Those
                    // entries belong to the previous tile -- they are never summed, but their words are relative to THAT tile's
                    // column windows / dictionary: decoded against this tile's they point anywhere (a gather up to 16 K entries
                    // past the end of x: found as a GPU memory fault on a 3-rank distributed solve by tools/stress_parity.py).
                    const int safe = (int)row0;
                    if (kk + 0 < ts) { c[u].x = safe; q[u].x = 0u; }
                    if (kk + 1 < ts) { c[u].y = safe; q[u].y = 0u; }
                    if (kk + 2 < ts) { c[u].z = safe; q[u].z = 0u; }
                }
                xv[u][0] = gather(c[u].x);
                xv[u][1] = gather(c[u].y);
                xv[u][2] = gather(c[u].z);
                xv[u][3] = gather(c[u].w);
            }
        }
        auto products = [&](auto val) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int kk = base + 4 * (tid + u * BLK);
                if (kk < te4) {
                    d2_t lo, hi;
                    lo.x = val(q[u].x) * xv[u][0];
                    lo.y = val(q[u].y) * xv[u][1];
                    hi.x = val(q[u].z) * xv[u][2];
                    hi.y = val(q[u].w) * xv[u][3];
                    *reinterpret_cast<d2_t *>(prod + (kk - base)) = lo;
                    *reinterpret_cast<d2_t *>(prod + (kk - base) + 2) = hi;
                }
            }
            if (tid < te - te4) { // ragged end of the pass (at most 3 entries; entries below ts are never summed)
                const int kk = te4 + tid;
                if (kk >= ts) prod[kk - base] = val(A.codes[kk]) * gather(A.col[kk]); // the unpacked arrays stay resident (an entry
                                                                                       // below ts is the previous tile's: see above)
            }
        };
        if (TLT > 0 && big) products(value_big);
        else products(value);
        if (!PREF && te < e_blk) request(te, e_blk);
        __syncthreads();
        const int a = rs > ts ? rs : ts;
        const int b = re < te ? re : te;
        for (int j = a; j < b; ++j) sum += prod[j - base];
        __syncthreads();
    }
    if (DOT) {
        // x.y: one partial per WAVE, reduced with DPP row shifts / broadcasts -- no LDS traffic, no barrier, no atomic.
        // (Measured: parking the terms in LDS and letting the last-arriving wave fold them cost 9-10 us per launch, two
        // dependent LDS round trips at the end of every wave's life while the LDS pipe is busy; a block barrier 15 us.)
        const double d = wave_sum_dpp((row < A.n) ? sum * xr : 0.);
        if ((tid & 63) == 63) {
            if (!HALO) partial[(int64_t)blockIdx.x * (BLK / 64) + (tid >> 6)] = d; // slot = position in the launch
            else // direct transport: write-through, fire and forget -- a finalizer block watches the slot (halo_finalizer)
                __hip_atomic_store(hv.stage + tile * (BLK / 64) + (tid >> 6), d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (row < A.n) __builtin_nontemporal_store(sum, y + row);
}

static constexpr int kTileCap = 4096;    // products parked per pass (U = 2 quads per lane)
static constexpr int kTileWin = 512;     // x entries staged in LDS (the tile's own rows): 38 KiB per workgroup => 32 waves per CU
static constexpr int kTltLds = 1024;     // tile-table entries staged in LDS (8 KiB; tiles rarely hold more distinct values)

template <int BLK, int CAP, bool DOT, bool LTAB, bool PACK, int WIN = 0, int TLT = 0, bool HALO = false, bool CWIN = false>
static avs_status spmv_vi2_launch_t(const CsrView &A, const double *x, double *y, double *partial, const PcgScalars *sc,
                                    const int32_t *tiles, int ntiles, size_t lds, hipStream_t stream, const HaloView &hv)
{
    // the words may stay in the Infinity Cache between two products: plain loads
    const auto kernel = (A.keep_cached && !HALO) ? k_spmv_vi2<BLK, CAP, DOT, LTAB, PACK, WIN, TLT, HALO, CWIN, !HALO>
                                                 : k_spmv_vi2<BLK, CAP, DOT, LTAB, PACK, WIN, TLT, HALO, CWIN>;
    // > 48 KiB of dynamic LDS (value table of ~1.5 k+ entries) needs the opt-in; it is a per-device function attribute, so it
    // is set on every such launch (cheap, rare path) rather than cached in a process-wide flag
    if (lds > 48 * 1024) AVS_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096));
    hipLaunchKernelGGL(kernel, dim3(ntiles), dim3(BLK), lds, stream, A, x, y, partial, sc, tiles, hv);
    AVS_HIP(hipGetLastError());
    return AVS_OK;
}

// tile-local dictionaries: 512-row tiles, CAP products per pass, the tile's table next to the x window
template <int CAP, bool DOT, int TCAP, bool HALO = false>
static avs_status spmv_tlt_launch(const CsrView &A, const double *x, double *y, double *partial, const PcgScalars *sc,
                                  const int32_t *tiles, int ntiles, hipStream_t stream, const HaloView &hv = HaloView())
{
    if (ntiles <= 0) return AVS_OK;
    const size_t lds = (size_t)(CAP + 4 + kTileWin + TCAP + (A.cbase ? kCwinSlots / 2 : 0)) * sizeof(double);
    if (A.cbase) return spmv_vi2_launch_t<kTileRows, CAP, DOT, false, false, kTileWin, TCAP, HALO, true>(A, x, y, partial, sc, tiles, ntiles, lds, stream, hv);
    return spmv_vi2_launch_t<kTileRows, CAP, DOT, false, false, kTileWin, TCAP, HALO>(A, x, y, partial, sc, tiles, ntiles, lds, stream, hv);
}

// the storage form of A picks the kernel.  HALO: the launch of the direct transport (ntiles = all tiles + the finalizer blocks, hv)
template <int BLK, int CAP, bool DOT, int WIN = 0, bool HALO = false>
static avs_status spmv_vi2_launch(const CsrView &A, const double *x, double *y, double *partial, const PcgScalars *sc,
                                  const int32_t *tiles, int ntiles, hipStream_t stream, const HaloView &hv = HaloView())
{
    if (ntiles <= 0) return AVS_OK;
    if (A.tab_ptr) { // tile-local codes: only the tile-table kernel can decode them
        if (BLK != kTileRows) { set_error("tile-local dictionaries need %d-row tiles", kTileRows); return AVS_EINVAL; }
        return spmv_tlt_launch<kTileCap, DOT, kTltLds, HALO>(A, x, y, partial, sc, tiles, ntiles, stream, hv);
    }
    const bool ltab = A.table_size <= kViLdsTable;
    if (A.cbase) { // windowed columns with ONE dictionary (it has at most 2048 entries, see build_matrix_index)
        if (BLK != kTileRows || WIN != kTileWin || !ltab) { set_error("windowed columns need the default tile geometry"); return AVS_EINVAL; }
        const size_t ldsw = (size_t)(kTileCap + 4 + kTileWin + kCwinSlots / 2 + ((A.table_size + 1) & ~1)) * sizeof(double);
        return spmv_vi2_launch_t<kTileRows, kTileCap, DOT, true, false, kTileWin, 0, HALO, true>(A, x, y, partial, sc, tiles, ntiles, ldsw, stream, hv);
    }
    const bool pack = A.packed != nullptr;
    const size_t lds = (size_t)(CAP + 4 + WIN + (ltab ? ((A.table_size + 1) & ~1) : 0)) * sizeof(double);
    if (ltab && pack) return spmv_vi2_launch_t<BLK, CAP, DOT, true, true, WIN, 0, HALO>(A, x, y, partial, sc, tiles, ntiles, lds, stream, hv);
    if (ltab) return spmv_vi2_launch_t<BLK, CAP, DOT, true, false, WIN, 0, HALO>(A, x, y, partial, sc, tiles, ntiles, lds, stream, hv);
    if (pack) return spmv_vi2_launch_t<BLK, CAP, DOT, false, true, WIN, 0, HALO>(A, x, y, partial, sc, tiles, ntiles, lds, stream, hv);
    return spmv_vi2_launch_t<BLK, CAP, DOT, false, false, WIN, 0, HALO>(A, x, y, partial, sc, tiles, ntiles, lds, stream, hv);
}

#ifdef AVS_PROBES
// ---------------------------------------------------------------------------------------------
// stream ceilings of this chip for the access widths the SpMV uses (measurement helpers)
// ---------------------------------------------------------------------------------------------
template <bool NT, int MODE>
__global__ __launch_bounds__(kBlock) void k_stream_probe(const d2_t *__restrict__ a, d2_t *__restrict__ b, int64_t n2,
                                                         double *__restrict__ sink)
{
    double acc = 0.;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (; i + 3 * stride < n2; i += 4 * stride) {
        const d2_t v0 = stream_load<NT>(a + i), v1 = stream_load<NT>(a + i + stride), v2 = stream_load<NT>(a + i + 2 * stride),
                   v3 = stream_load<NT>(a + i + 3 * stride);
        if (MODE == 1) { b[i] = v0; b[i + stride] = v1; b[i + 2 * stride] = v2; b[i + 3 * stride] = v3; }
        else acc += (v0.x + v0.y) + (v1.x + v1.y) + (v2.x + v2.y) + (v3.x + v3.y);
    }
    for (; i < n2; i += stride) {
        const d2_t v0 = stream_load<NT>(a + i);
        if (MODE == 1) b[i] = v0; else acc += v0.x + v0.y;
    }
    if (MODE == 0 && acc == 1.2345e300) sink[0] = acc; // keep the loads alive
}

avs_status stream_probe(int mode, const double *a, double *b, int64_t n, double *sink, int grid, hipStream_t st)
{
    const int64_t n2 = n / 2;
    switch (mode) {
    case 0: hipLaunchKernelGGL((k_stream_probe<false, 0>), dim3(grid), dim3(kBlock), 0, st, (const d2_t *)a, (d2_t *)b, n2, sink); break;
    case 1: hipLaunchKernelGGL((k_stream_probe<true, 0>), dim3(grid), dim3(kBlock), 0, st, (const d2_t *)a, (d2_t *)b, n2, sink); break;
    case 2: hipLaunchKernelGGL((k_stream_probe<false, 1>), dim3(grid), dim3(kBlock), 0, st, (const d2_t *)a, (d2_t *)b, n2, sink); break;
    default: set_error("unknown stream probe mode %d", mode); return AVS_EINVAL;
    }
    AVS_HIP(hipGetLastError());
    return AVS_OK;
}

// ---------------------------------------------------------------------------------------------
// SELL-C-sigma (C = 64 = one wavefront per slice) -- measurement only (BASELINE configs[4] asks for a blocked-ELL / SELL
// experiment; tools/sell_experiment.py builds the layout and reports padding + time, profiles/r02_sell_experiment.md).
// Slice s holds rows [64 s, 64 s + 64) of the sigma-sorted matrix, column-major: entry j of lane l at slice_ptr[s] + 64 j + l,
// padded to the slice's longest row with (col 0, val 0.0).  Every load is a full coalesced 512-B / 256-B wave access.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_spmv_sell(int64_t nslices, const int64_t *__restrict__ slice_ptr, const int32_t *__restrict__ col,
                                                   const double *__restrict__ val, const double *__restrict__ x, double *__restrict__ y)
{
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= nslices) return;
    const int64_t b = slice_ptr[s], e = slice_ptr[s + 1];
    double sum = 0.;
    int64_t k = b + lane;
    for (; k + 192 < e; k += 256) { // 4 entries per lane in flight
        const double v0 = __builtin_nontemporal_load(val + k), v1 = __builtin_nontemporal_load(val + k + 64),
                     v2 = __builtin_nontemporal_load(val + k + 128), v3 = __builtin_nontemporal_load(val + k + 192);
        const int c0 = __builtin_nontemporal_load(col + k), c1 = __builtin_nontemporal_load(col + k + 64),
                  c2 = __builtin_nontemporal_load(col + k + 128), c3 = __builtin_nontemporal_load(col + k + 192);
        const double x0 = x[c0], x1 = x[c1], x2 = x[c2], x3 = x[c3];
        sum += v0 * x0;
        sum += v1 * x1;
        sum += v2 * x2;
        sum += v3 * x3;
    }
    for (; k < e; k += 64) sum += __builtin_nontemporal_load(val + k) * x[__builtin_nontemporal_load(col + k)];
    y[s * 64 + lane] = sum;
}

#endif // AVS_PROBES


int spmv_default_variant(const CsrView &) { return 24; } // 512 rows/WG, 32 KiB LDS, 16-B vector + non-temporal stream (profiles/r01_spmv_variants.md)

template <bool DOT>
static avs_status spmv_dispatch(const CsrView &A, const double *x, double *y, double *partial,
                                const PcgScalars *sc, int variant, hipStream_t stream, int *nblocks)
{
    if (A.n <= 0) { if (nblocks) *nblocks = 0; return AVS_OK; }
    if (A.brick && A.brick->ntiles > 0 && (variant == 0 || variant == spmv_default_variant(A))) { // brick-structured form (avs_brick.hip)
        if (nblocks) *nblocks = brick_partial_count(*A.brick, 8);
        return spmv_brick_launch(*A.brick, x, y, DOT ? partial : nullptr, (DOT && sc) ? &sc->done : nullptr, stream);
    }
    if (A.codes && (variant == 0 || variant == spmv_default_variant(A))) { // value-indexed matrix: 6 or 4 B per non-zero
        const int nt = (int)((A.n + kTileRows - 1) / kTileRows);
        if (nblocks) *nblocks = nt * (kTileRows / 64);
        return spmv_vi2_launch<kTileRows, kTileCap, DOT, kTileWin>(A, x, y, partial, sc, nullptr, nt, stream);
    }
#ifdef AVS_PROBES // geometry sweeps of the value-indexed kernels (profiles/r01_spmv_variants.md, r02_varvisc.md)
    if (A.tab_ptr && variant >= 51 && variant <= 54) { // geometry sweep of the tile-table kernel (profiles/r02_varvisc.md)
        const int nt = (int)((A.n + kTileRows - 1) / kTileRows);
        if (nblocks) *nblocks = nt * (kTileRows / 64);
        switch (variant) {
        case 51: return spmv_tlt_launch<4096, DOT, 1024>(A, x, y, partial, sc, nullptr, nt, stream);
        case 52: return spmv_tlt_launch<2048, DOT, 2048>(A, x, y, partial, sc, nullptr, nt, stream);
        case 53: return spmv_tlt_launch<4096, DOT, 2048>(A, x, y, partial, sc, nullptr, nt, stream);
        case 54: return spmv_tlt_launch<2048, DOT, 1024>(A, x, y, partial, sc, nullptr, nt, stream);
        }
    }
    if (A.codes && !A.tab_ptr && !A.cbase && variant >= 31 && variant <= 46) {
#define AVS_VI2_CASE(ID, BLK, CAP, ...)                                                                         \
    case ID: {                                                                                                  \
        const int nt = (int)((A.n + BLK - 1) / BLK);                                                            \
        if (nblocks) *nblocks = nt * (BLK / 64);                                                                \
        return spmv_vi2_launch<BLK, CAP, DOT, ##__VA_ARGS__>(A, x, y, partial, sc, nullptr, nt, stream);        \
    }
        switch (variant) { // geometry sweep of the value-indexed kernel (profiles/r01_spmv_variants.md)
            AVS_VI2_CASE(31, 256, 4096)
            AVS_VI2_CASE(32, 512, 8192)
            AVS_VI2_CASE(33, 512, 4096)
            AVS_VI2_CASE(34, 128, 2048)
            AVS_VI2_CASE(36, 1024, 8192)
            AVS_VI2_CASE(37, 256, 2048)
            AVS_VI2_CASE(38, 512, 2048)
            AVS_VI2_CASE(39, 256, 1024)
            AVS_VI2_CASE(40, 128, 1024)
            AVS_VI2_CASE(41, 256, 2048, 256)
            AVS_VI2_CASE(42, 512, 4096, 512)
            AVS_VI2_CASE(43, 256, 2048, 512)
            AVS_VI2_CASE(44, 128, 1024, 128)
            AVS_VI2_CASE(45, 128, 1024, 256)
            AVS_VI2_CASE(46, 512, 4096, 1024)
        }
#undef AVS_VI2_CASE
    }
#endif
    if (variant == 0) variant = spmv_default_variant(A);
    int g;
    switch (variant) { // the plain kernels below read A.val / A.col only
#define AVS_TILE_CASE(ID, BLK, CAP, VEC, XCD, CHUNK, NT)                                                                  \
    case ID:                                                                                                   \
        g = (int)((A.n + BLK - 1) / BLK);                                                                      \
        hipLaunchKernelGGL((k_spmv_tile<BLK, CAP, DOT, VEC, XCD, NT>), dim3(g), dim3(BLK), 0, stream, A, x, y, partial, sc, CHUNK); \
        break;
#ifdef AVS_PROBES // the round-1 kernel sweep (14 = the plain reference kernel avs_bench_spmv compares against)
    case 1:
        g = stream_grid(A.n);
        hipLaunchKernelGGL((k_spmv_stream<DOT>), dim3(g), dim3(kBlock), 0, stream, A, x, y, partial, sc);
        break;
    case 2:
        g = kVecGrid * 4;
        hipLaunchKernelGGL((k_spmv_vec<4, DOT>), dim3(g), dim3(kBlock), 0, stream, A, x, y, partial, sc);
        break;
    case 3:
        g = kVecGrid * 4;
        hipLaunchKernelGGL((k_spmv_vec<8, DOT>), dim3(g), dim3(kBlock), 0, stream, A, x, y, partial, sc);
        break;
    case 4:
        g = kVecGrid * 4;
        hipLaunchKernelGGL((k_spmv_vec<16, DOT>), dim3(g), dim3(kBlock), 0, stream, A, x, y, partial, sc);
        break;
        AVS_TILE_CASE(5, 256, 4096, false, true, 0, false)
        AVS_TILE_CASE(6, 256, 4096, true, false, 0, false)
        AVS_TILE_CASE(7, 256, 2048, false, false, 0, false)
        AVS_TILE_CASE(8, 128, 2048, false, false, 0, false)
        AVS_TILE_CASE(9, 512, 8192, false, false, 0, false)
        AVS_TILE_CASE(10, 256, 2048, true, false, 0, false)
        AVS_TILE_CASE(11, 256, 2048, true, true, 2, false)
        AVS_TILE_CASE(12, 256, 2048, true, true, 4, false)
        AVS_TILE_CASE(13, 256, 2048, true, true, 16, false)
        AVS_TILE_CASE(14, 256, 2048, true, false, 0, true)
        AVS_TILE_CASE(15, 256, 2048, true, true, 4, true)
        AVS_TILE_CASE(16, 256, 2048, true, true, 16, true)
        AVS_TILE_CASE(17, 256, 2048, true, true, 64, true)
        AVS_TILE_CASE(18, 256, 4096, true, true, 4, true)
        AVS_TILE_CASE(19, 256, 2048, false, false, 0, true)
        AVS_TILE_CASE(20, 256, 2048, true, true, 2, true)
        AVS_TILE_CASE(21, 256, 2048, true, true, 8, true)
        AVS_TILE_CASE(22, 128, 1024, true, false, 0, true)
        AVS_TILE_CASE(23, 128, 2048, true, false, 0, true)
#endif
        AVS_TILE_CASE(24, 512, 4096, true, false, 0, true)
#undef AVS_TILE_CASE
    default:
        set_error("unknown SpMV variant %d", variant);
        return AVS_EINVAL;
    }
    if (nblocks) *nblocks = g;
    AVS_HIP(hipGetLastError());
    return AVS_OK;
}

size_t spmv_partial_elems(int64_t n)
{
    size_t a = (size_t)((n + 63) / 64) + 16, b = (size_t)kVecGrid * 4; // up to one partial per wave of rows
    return 2 * (a > b ? a : b) + 4 * (size_t)kVecGrid + 16;
}

avs_status spmv_launch(const CsrView &A, const double *x, double *y, int variant, hipStream_t stream)
{
    return spmv_dispatch<false>(A, x, y, nullptr, nullptr, variant, stream, nullptr);
}

// default kernel restricted to a list of kTileRows-row tiles (multi-GPU overlap: interior tiles run while the halo
// travels); partial[tile] receives the tile's share of x.y, so several launches fill one partial array
int spmv_tile_rows() { return kTileRows; }
avs_status spmv_dot_tiles(const CsrView &A, const double *x, double *y, double *partial, const PcgScalars *sc,
                          const int32_t *tiles, int ntiles, hipStream_t stream)
{
    if (ntiles <= 0) return AVS_OK;
    if (A.codes) return spmv_vi2_launch<kTileRows, kTileCap, true, kTileWin>(A, x, y, partial, sc, tiles, ntiles, stream);
    hipLaunchKernelGGL((k_spmv_tile<kTileRows, 4096, true, true, false, true>), dim3(ntiles), dim3(kTileRows), 0, stream, A, x, y,
                       partial, sc, 0, tiles);
    AVS_HIP(hipGetLastError());
    return AVS_OK;
}

// the SpMV launch of the direct transport: all tiles (those flagged in hv.tile_bnd wait for the peers' entries and gather halo
// columns from the comm block) + the finalizer block; launch_blocks = ntiles + 1
avs_status spmv_dot_tiles_halo(const CsrView &A, const double *x, double *y, double *partial, const PcgScalars *sc,
                               const int32_t *tiles, int launch_blocks, const HaloView &hv, hipStream_t stream)
{
    if (A.codes) return spmv_vi2_launch<kTileRows, kTileCap, true, kTileWin, true>(A, x, y, partial, sc, tiles, launch_blocks, stream, hv);
    hipLaunchKernelGGL((k_spmv_tile<kTileRows, 4096, true, true, false, true, true>), dim3(launch_blocks), dim3(kTileRows), 0, stream, A, x, y,
                       partial, sc, 0, tiles, hv);
    AVS_HIP(hipGetLastError());
    return AVS_OK;
}

// the form used inside the PCG loops: y = A x and per-block partials of x.y (partial == nullptr: the plain product)
avs_status spmv_dot_launch(const CsrView &A, const double *x, double *y, double *partial, int variant, hipStream_t stream,
                           const PcgScalars *sc, int *nblocks)
{
    return partial ? spmv_dispatch<true>(A, x, y, partial, sc, variant, stream, nblocks)
                   : spmv_dispatch<false>(A, x, y, nullptr, sc, variant, stream, nblocks);
}

#ifdef AVS_PROBES
avs_status spmv_sell_launch(int64_t nslices, const int64_t *slice_ptr, const int32_t *col, const double *val, const double *x, double *y,
                            hipStream_t stream)
{
    if (nslices <= 0) return AVS_OK;
    hipLaunchKernelGGL(k_spmv_sell, dim3((unsigned)((nslices + 3) / 4)), dim3(256), 0, stream, nslices, slice_ptr, col, val, x, y);
    AVS_HIP(hipGetLastError());
    return AVS_OK;
}
#endif

} // namespace avs

#ifdef AVS_PROBES
extern "C" avs_status avs_spmv_sell(int64_t nslices, const int64_t *slice_ptr, const int32_t *col, const double *val, const double *x,
                                    double *y, int32_t repeats, void *stream, double *ms_per_launch)
{
    AVS_REQUIRE(slice_ptr && col && val && x && y && repeats > 0, AVS_EINVAL, "bad argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    AVS_TRY(avs::spmv_sell_launch(nslices, slice_ptr, col, val, x, y, st)); // warm-up
    avs::Timer t(st);
    t.start();
    for (int i = 0; i < repeats; ++i) AVS_TRY(avs::spmv_sell_launch(nslices, slice_ptr, col, val, x, y, st));
    const double ms = t.stop() / repeats;
    if (ms_per_launch) *ms_per_launch = ms;
    return AVS_OK;
}
#endif // AVS_PROBES
