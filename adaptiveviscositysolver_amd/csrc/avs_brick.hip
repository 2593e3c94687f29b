// avs_brick.hip -- brick-structured SpMV for the brick-major system (round 4).
//
// The matrix of this problem is translation invariant along the liquid surface: the level-0 shell (80 % of the rows of the 512^3 beam) and
// the transitions below it repeat a few hundred row PATTERNS -- but only when a column is named by WHERE its face lies relative to the
// row's face, not by its index.  This form does that:
//
//   * tile = the rows of one 8^3 brick of fine cells (consecutive ids in the brick-major numbering, avs_reorder.hip; at most 1024 rows, a
//     fuller brick is cut in two); runs of small bricks (coarse interior: 3 .. 24 rows each) are cut into "E" tiles of 128 rows that keep
//     today's packed words;
//   * every face a tile may read has a tile-LOCAL slot on four padded lattices -- level l, brick-relative level-l cell (-1 .. 8>>l)^3,
//     axis a -> kBrickLoff[l] + ((z S + y) S + x) 3 + a with S = (8>>l) + 2: 3000 + 648 + 192 + 81 = 3921 slots of x in LDS (31 KB),
//     filled from <= 16-entry runs of consecutive (slot, column) pairs (quarter-wave loads; a run names its column as an offset into one
//     of the 27 neighbour bricks, whose first rows are in the tile header: 4 B per run);
//   * a row of a G tile whose columns all have a slot is stored as ONE 32-bit descriptor (tile-local pattern id, level, axis, cell) + its
//     16-bit position in the tile; its pattern -- the sequence of (slot delta relative to the row's base on the column's lattice,
//     lattice level, value code) in the STORED column order -- comes from a global table (a few thousand words, L2 resident), the tile's
//     patterns staged in LDS quad by quad.  The rows are EXECUTED sorted by (pattern length, pattern): a wave's 64 rows then have
//     the same trip count (one lane per row; unsorted, every wave pays for its longest row: 40 entries against 15 on average);
//   * any other row is "streamed": today's packed words (code << col_bits | column) in CSR order; the workgroup gathers x for them
//     from global memory (requested together with the fill, so the latencies overlap), parks the products in LDS and one lane per
//     row adds its segment -- the round-3 kernel's scheme, for the few rows that need it.  E tiles and G tiles without any pattern row use
//     the lattice's LDS for the products (3936 per pass instead of 1024).
//
// PERSISTENT workgroups (three per CU) walk the tiles: a workgroup launch per tile cost more than the tile (17 k launches of 8 waves with
// 53 KB of LDS: 68 us of a 170 us kernel with the arithmetic switched off).  Inside the walk the next tile's header (scalar) and ALL its
// descriptors are requested before the current tile is multiplied, so a tile waits for one global round trip (x and pattern words).
// One lane sums one row left to right with a multiply and an add per entry (no FMA, -ffp-contract=off): y is bit-identical to the
// plain CSR kernel.
// Round 5 -- partitioned systems: a fill run names its column as (one of <= 32 windows of 2^11 columns in the tile header, offset), so
// the local system of a rank ([owned | halo] columns) is just another matrix; with the halo in the tail of the vector (RCCL transport)
// the kernel is unchanged.  Direct transport: the halo lives in the rank's comm block, written by the peers; a small launch in front of
// this kernel (k_halo_gather, avs_pcg.hip) waits for the peers' flags and copies it behind the owned entries of the vector, and the
// persistent workgroups' x.y partials go to the stage slots the finalizer launch behind it folds (k_halo_finalize).  (A HALO
// instantiation of this kernel -- flag wait per flagged tile, comm-block loads in the fill -- was built first: 4-23 spilled registers
// and 139-167 us against 118 for the plain kernel; the two small launches cost ~5 us.)  Reference: Eigen's `mat * p` inside ConjugateGradient (cpp:618-630 of HDK_AdaptiveViscosity.cpp); the row
// structure is that of cpp:2537-2745.
#include <mutex>

#include "avs_internal.hpp"
#include "avs_wave.hpp" // wave_sum_dpp: lane 63 holds the sum (fixed order)

namespace avs {

constexpr int kBrickBlk = 512;
#ifndef AVS_BRICK_TAIL
#define AVS_BRICK_TAIL 4      // chunks of the execution order that count as a tile's tail (in-loop A/B with four-lane fill runs: 2 -> 94.0 us, 4 -> 91.9 us)
#endif
#ifndef AVS_BRICK_TAIL_PRIO
#define AVS_BRICK_TAIL_PRIO 1
#endif
#ifndef AVS_BRICK_LOAD_PRIO
#define AVS_BRICK_LOAD_PRIO 2
#endif
#ifndef AVS_BRICK_PRIO
#define AVS_BRICK_PRIO 3 // s_setprio placements (see the load phase below): 0 none, 1 load phase, 2 + waves 6 and 7 in the walk, 3 + the waves of the tile's last two chunks
#endif

#ifdef AVS_PROBES
// measurement only (AVS_BRICK_DEBUG & 16): wall_clock64 stamps of workgroup phases, 8 per tile, first kStampTiles tiles of every workgroup
constexpr int kStampTiles = 40, kStampWgs = 1024;
__device__ long long g_brick_stamps[kStampWgs * kStampTiles * 8];
#define BRICK_DBG(bit) (B.debug & (bit))
#define BRICK_STAMP(slot)                                                                                            \
    do {                                                                                                             \
        if (BRICK_DBG(16) && threadIdx.x == 0 && iter < kStampTiles && blockIdx.x < kStampWgs) {                             \
            g_brick_stamps[((int)blockIdx.x * kStampTiles + iter) * 8 + (slot)] = wall_clock64();                    \
        }                                                                                                            \
    } while (0)

#else
#define BRICK_DBG(bit) 0
#define BRICK_STAMP(slot) do { } while (0)
#endif

// i-th streamed row of a tile -> thread: consecutive rows go to different waves (a handful of rows per tile: every wave gets a few lanes)
__device__ __forceinline__ int brick_srow_of_thread(int tid, int k) { return k * kBrickBlk + ((tid & 63) << 3) + (tid >> 6); }

// The kernel has no static LDS: the dynamic segment starts at LDS address 0, and a read from a BYTE ADDRESS spares the "+ base" the
// compiler otherwise leaves in the instruction stream per access (v_add_u32 v, 0, v: one of six VALU instructions per matrix entry).
template <typename T>
__device__ __forceinline__ T lds_abs(unsigned byte_addr) { return *(const T __attribute__((address_space(3))) *)(uintptr_t)byte_addr; }
// LDS layout in BYTES for vectors of T (double: the PCG loops; float: the float-vector loop of AVS_PRECISION_F32, avs_pcg_f32.inl):
//   [0, kBrickSlotsPad T) the lattice | kBrickXSlots T extra x slots | kBrickBlockBytes: the tile's descriptor block, then the products of
//   its streamed rows | vals (value table, T) | pattern words | pinfo | row-base table.  With T = float the lattice is 15.4 KB instead of
//   31 KB: the LDS would hold FOUR workgroups per CU instead of three -- but only at 64 registers per lane, where the fused-dot
//   instantiation spills 13 of them (113 MB of scratch traffic per launch at 512^3): measured equal on the 512^3 beam (99 against 100.5 us),
//   8 % slower on the 1024^3 sheet (317 against 288 us).  The kernel keeps the 80-register budget of the double instantiation: three
//   workgroups per CU, no spills.
constexpr unsigned kBrickBlockBytes = (unsigned)((kBrickPark - kBrickXSlots) * sizeof(double));
template <typename T> constexpr unsigned brick_vals_byte() { return (unsigned)((kBrickSlotsPad + kBrickXSlots) * sizeof(T)) + kBrickBlockBytes; } // `vals` behind the lattice and `park`
template <typename T> constexpr unsigned brick_vals_elems(int table_size) { return (unsigned)((table_size + 4) & ~3); } // keeps the pattern image 16-B aligned for both T
// V, the type of the matrix values and of the row sums (default: T).  <float, double> is the mixed-precision loop's product
// (avs_pcg_mixed.inl): lattice and x slots stay 4-byte, the value table in LDS holds doubles, every entry is (double)x * val added in
// double left to right, and the row sum is rounded to float once, where y is stored (the fused dot uses the unrounded sum).  The
// streamed rows' parked products are V as well -- the park area is sized in bytes of doubles for every T -- so that every row of y is
// the correctly rounded double sum up to contraction.

// element `idx` of an array whose base is workgroup-uniform: a 32-bit byte offset in a VGPR + the base in SGPRs (global_load ... saddr)
// instead of 64-bit address arithmetic per lane
template <class T>
__device__ __forceinline__ T ld_u32(const T *base, unsigned idx)
{
    return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + (size_t)(unsigned)(idx * (unsigned)sizeof(T)));
}


// A tile's descriptors are ONE contiguous block of 32-bit words (<= 8 KB), fetched with one 16-B load per thread and parked in LDS:
//   [0] row0 [1] nrows [2] npat [3] nruns [4] npq (pattern quads) [5] nprow (pattern rows) [6] srow0 [7] nsrows [8] sword0 [9] nsw
//   [16 .. 48) first rows of the 27 neighbour bricks
//   [10] rd0 (first pattern-row descriptor of the tile in rdesc)
//   runs[nruns] (8 B each: absolute first column | slot << 4 | length - 1) | pquads[npq] | pinfo[npat]
//   [11] the tile's rows read halo columns (partitioned systems)
// The per-row arrays (rdesc: descriptor + position of every pattern row in execution order; ownslot) stay in global memory.
constexpr int kBlkHdr = kBlkHdrWords;

template <bool DOT, bool VC = false, typename T = double, typename V = T>
__global__ __launch_bounds__(kBrickBlk) __attribute__((amdgpu_waves_per_eu(6, 8))) void k_spmv_brick(BrickView B, const T *__restrict__ x, T *__restrict__ y,
                                                         double *__restrict__ partial, const int *__restrict__ done_flag)
{
    if (DOT && done_flag && *done_flag) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr unsigned ES = (unsigned)sizeof(T);                         // bytes per vector element: every LDS byte offset below scales with it
    constexpr unsigned kValsByte = brick_vals_byte<T>();
    T *xs = reinterpret_cast<T *>(smem_raw);                             // kBrickSlotsPad
    T *park = xs + kBrickSlotsPad;                                       // right behind the lattice: [0, kBrickXSlots) extra x slots (off-lattice
                                                                        // columns), behind them kBrickBlockBytes: first the tile's descriptor
                                                                        // block, then the products of its streamed rows
    constexpr bool MIX = sizeof(V) != sizeof(T);                         // 8-B values next to 4-B vector elements
    static_assert(sizeof(V) >= sizeof(T) && kValsByte % sizeof(V) == 0, "values at least as wide as the vectors, aligned behind the park area");
    V *vals = reinterpret_cast<V *>(smem_raw + kValsByte);               // table_size + 1 (the last entry is 0.0: padding words), padded to 16 B
    uint32_t *pw = reinterpret_cast<uint32_t *>(vals + brick_vals_elems<V>(B.table_size)); // kBrickPatWords (VC: kBrickPatWordsVc) + 8
    uint32_t *pinfo = pw + (VC ? kBrickPatWordsVc : kBrickPatWords) + 8; // kBrickPatMax: local start | quads << 16
    uint2 *rbt = reinterpret_cast<uint2 *>(pinfo + kBrickPatMax);       // kBrickRowBase entries: a row's bases on the four lattices, per axis
    const uint32_t *bw = reinterpret_cast<const uint32_t *>(park + kBrickXSlots);
    const int tid = threadIdx.x;
    constexpr int RL = kBrickRunLen;                                    // lanes per fill run
    const int lane = tid & 63, l16 = tid & (RL - 1), qw = tid / RL;
    const int wave_id = __builtin_amdgcn_readfirstlane(tid >> 6);          // (scalar)
    const bool wide = VC || B.col_bits == 0;                             // 64-bit streamed words: column | code << 32 (VC: 96 bits, column | value)
    const unsigned cmask = wide ? 0xffffffffu : (1u << B.col_bits) - 1u;
    const int cbits = B.col_bits;
    constexpr int QW = kBrickBlk / RL;
    static_assert((kBrickPark - kBrickXSlots) * 2 <= kBrickBlk * 4, "one 16-B load per thread fetches a whole descriptor block");

    if (!VC)
        for (int i = tid; i <= B.table_size; i += kBrickBlk) vals[i] = (i < B.table_size) ? (V)B.table[i] : (V)0; // once per workgroup (VC: a table per tile; float: the values ARE floats, AVS_PRECISION_F32)
    // A row of level lr at local cell (cx, cy, cz) has the byte offset 8 (kBrickLoff[lc] + 3 ((bz S + by) S + bx)) on lattice lc, with
    // b = ((c >> up) << down) + 1 per axis: the sum of one term per axis.  Table entry (axis d, lr, c + 1) = the four lattices' terms as
    // 16-bit fields {lattice 0 | lattice 1 << 16, lattice 2 | lattice 3 << 16} (the sums stay below 2^15: no carries between the fields);
    // the x entries carry the lattice offsets.  Three 8-B LDS reads and four adds per row instead of ~60 VALU instructions.
    if (tid < kBrickRowBase) {
        const int d = tid / 40, lr = (tid / 10) & 3, cc = tid % 10 - 1;
        unsigned f[4];
#pragma unroll
        for (int lc = 0; lc < 4; ++lc) {
            const int up = lc > lr ? lc - lr : 0, dn2 = lr > lc ? lr - lc : 0;
            const int S = (8 >> lc) + 2;
            const int b = ((cc >> up) << dn2) + 1;
            f[lc] = (unsigned)(3 * (int)ES * b * (d == 0 ? 1 : d == 1 ? S : S * S) + (d == 0 ? (int)ES * kBrickLoff[lc] : 0));
        }
        rbt[tid] = uint2{f[0] | (f[1] << 16), f[2] | (f[3] << 16)};
    }

    // Tile -> workgroup.  Workgroup b runs on XCD b mod 8 (round-robin dispatch); consecutive tiles are neighbouring bricks and read
    // each other's rows as halo, so what an XCD works on at any time is one contiguous run of gridDim / 8 tiles, its workgroups side by
    // side (a halo value is fetched by one L2; tile = b + k gridDim: by up to eight).  Two walks, chosen per matrix (BrickView::walk,
    // measured at the first assembly of a matrix size, avs_reorder.hip):
    //   0  one contiguous EIGHTH of the tiles per XCD -- best where tiles cost the same everywhere (512^3 beam: 2 % over walk 1 in the loop);
    //   1  chunks of gridDim / 8 tiles dealt to the XCDs in turn -- every XCD sees the same mix of tiles.  A thin sheet's eighths are its z
    //      layers (full surface bricks here, coarse interior there) and the kernel waits for the slowest XCD: 133 (walk 0) against 94 us.
    //   2  (round 5) a PLANNED walk: every workgroup's tile sequence is laid out by the host from a cost model of the tiles (BrickForm::plan_walk:
    //      cost-equal contiguous ranges per XCD, then the tiles of a range dealt, in order, to whichever of the XCD's workgroups has
    //      the least work so far) -- the static walks end 15-20 % after their average workgroup (E tiles cost two G tiles, G tiles
    //      differ by their rows); deterministic: the plan is a function of the matrix and the grid.
    const uint2 *seq;                                                    // this workgroup's tiles: seq[0], seq[step], ... (cnt of them)
    int step, cnt;
    if (B.wlist && (int)gridDim.x == B.wgrid && !BRICK_DBG(32)) {
        const int w0 = B.wptr[blockIdx.x];
        seq = B.wlist + w0;
        step = 1;
        cnt = B.wptr[blockIdx.x + 1] - w0;
    } else {
        int tile = blockIdx.x, tstep = (int)gridDim.x, tend = B.ntiles;
        if ((gridDim.x & 7u) == 0u && B.ntiles >= (int)gridDim.x && !BRICK_DBG(32)) {
            const int c = (int)(blockIdx.x & 7u), gx = (int)(gridDim.x >> 3);
            tile = c * gx + (int)(blockIdx.x >> 3);
            if (B.walk == 0) { // one contiguous eighth of the tiles per XCD
                tstep = gx;
                tile = (int)(((int64_t)B.ntiles * c) >> 3) + (int)(blockIdx.x >> 3);
                tend = (int)(((int64_t)B.ntiles * (c + 1)) >> 3);
            }
        }
        seq = B.tile_blk + tile;
        step = tstep;
        cnt = tile < tend ? (tend - tile + tstep - 1) / tstep : 0;
    }
    if (cnt <= 0) {                                                      // (a workgroup without tiles: only when the grid exceeds what the plan could fill)
        if (DOT && tid == 0) partial[blockIdx.x] = 0.;
        return;
    }
    const uint4 *blocks16 = reinterpret_cast<const uint4 *>(B.blocks);
    uint2 tb = seq[0];                                                   // first 16-B unit, units
    uint4 blk = blocks16[(int64_t)tb.x + (tid < (int)tb.y ? tid : 0)];
    int nsw_prev = 0;

    int iter = 0;
    V dot = 0;                                                           // x.y of this lane's rows, all tiles of the workgroup
    for (;;) {
        BRICK_STAMP(0);
        if (nsw_prev > 0) __syncthreads();                               // the previous tile's streamed sums have read `park`
        if (tid < (int)tb.y) reinterpret_cast<uint4 *>(park + kBrickXSlots)[tid] = blk;
        __syncthreads();                                                 // every wave is done with the previous tile; the block is visible
        const int row0 = __builtin_amdgcn_readfirstlane((int)bw[0]), nrows = __builtin_amdgcn_readfirstlane((int)bw[1]);
        const int npat = __builtin_amdgcn_readfirstlane((int)bw[2]), nruns = __builtin_amdgcn_readfirstlane((int)bw[3]);
        const int npq = __builtin_amdgcn_readfirstlane((int)bw[4]), nprow = __builtin_amdgcn_readfirstlane((int)bw[5]);
        const int srow0 = __builtin_amdgcn_readfirstlane((int)bw[6]), nsrows = __builtin_amdgcn_readfirstlane((int)bw[7]);
        const int sword0 = __builtin_amdgcn_readfirstlane((int)bw[8]), nsw = __builtin_amdgcn_readfirstlane((int)bw[9]);
        const int rd0 = __builtin_amdgcn_readfirstlane((int)bw[10]);
        // VC (variable viscosity: the patterns carry the geometry only): the tile's value codes start at vcodes[cw0] (one 8-B quad of four
        // 16-bit byte offsets into the tile's value table per row quad, wave-interleaved in execution order), its ntv values at ttab[tt0]
        const int cw0 = VC ? __builtin_amdgcn_readfirstlane((int)bw[12]) : 0, tt0 = VC ? __builtin_amdgcn_readfirstlane((int)bw[13]) : 0;
        const int ntv = VC ? __builtin_amdgcn_readfirstlane((int)bw[14]) : 0;
        const int o_runs = kBlkHdr, o_pq = o_runs + 2 * nruns, o_pi = o_pq + npq; // (runs are 8 B)
        const bool emode = npat == 0;                 // no pattern rows: the products of the streamed rows may use the x lattice's LDS
        V *prod = reinterpret_cast<V *>(emode ? xs : park + kBrickXSlots);
        const int cap = emode ? (int)(kBrickSlotsPad * sizeof(T) / sizeof(V)) : kBrickPark - kBrickXSlots; // (the park block holds kBrickPark - kBrickXSlots DOUBLES for every T)
        BRICK_STAMP(1);
        // Round 6: a CU runs three workgroups on the same SIMDs and the kernel is bound by instruction ISSUE (38 M VALU wave-instructions per
        // launch at 512^3, 80 % of them outside the row walk).  A wave in this phase -- descriptors, the tile's ONE round trip of loads, LDS
        // writes, with the whole workgroup waiting at the barrier behind it -- goes ahead of the other workgroups' row walks (s_setprio 2
        // until the barrier), and so do, in the walk, the two waves with the tile's LONGEST rows (the execution order is sorted by pattern
        // length: the slowest wave walks 8.9 quads per tile against a mean of 4.3 on the 512^3 beam, 5.5 against 2.7 on the 1024^3 sheet,
        // and the next tile cannot start before it is done).  Measured (profiles/r06_notes.md): 512^3 beam 111.5 -> 104.2 us stand-alone,
        // 1024^3 sheet 324 -> 305 us.
        if (AVS_BRICK_PRIO >= 1) __builtin_amdgcn_s_setprio(AVS_BRICK_LOAD_PRIO);
#ifdef AVS_PROBES
        if (BRICK_DBG(16) && threadIdx.x == 0 && iter < kStampTiles && blockIdx.x < kStampWgs) // tile kind: 1 E tile, 2 G tile with streamed rows, 0 G tile
        {
            long long *sp = &g_brick_stamps[((int)blockIdx.x * kStampTiles + iter) * 8];
            sp[5] = emode ? 1 : (nsw > 0 ? 2 : 0);
            sp[6] = (long long)nprow | ((long long)nruns << 16) | ((long long)npq << 32) | ((long long)nrows << 48);   // what a cost model can see
            sp[7] = (long long)nsw | ((long long)nsrows << 32);
        }
#endif
        // ---- this tile's loads, ONE round trip: x of the halo runs, x of the tile's own rows, the pattern quads, the row descriptors.
        // Round 5: (i) a fill run is 8 B -- absolute first column | slot << 4 | length - 1 -- so a batch costs ONE LDS read (it was two
        // dependent ones: run word, then the base of its neighbour brick); (ii) every LDS read the loads depend on (run words, pattern
        // quad offsets) is issued before the first global load -- one wait instead of one or two per batch; (iii) nothing is SELECTED
        // right behind a load (`valid ? loaded : default` made the compiler wait for that load on the spot: the round-4 binary stalled
        // for the own-slot load, the row descriptors and the streamed descriptors one after the other, three serialised round trips);
        // validity is a predicate recomputed where the value is used.
        constexpr int RPT = kBrickMaxRows / kBrickBlk;
        constexpr int PQ = (kBrickPatWords / 4 + kBrickBlk - 1) / kBrickBlk;
#ifndef AVS_BRICK_RUFAST
#define AVS_BRICK_RUFAST (RL == 16 ? 6 : (RL == 8 ? 4 : (RL == 4 ? 3 : 2)))
#endif
        constexpr int kRuFast = AVS_BRICK_RUFAST; // fill batches held in registers (192 / 256 / 384 / 512 runs: nearly every tile); the rest, rare, go run by run
        const uint2 *runs2 = reinterpret_cast<const uint2 *>(bw + o_runs);
        T fv[kRuFast];
        uint32_t rdsc[kRuFast];
        uint32_t pqo[PQ];
#pragma unroll
        for (int u = 0; u < PQ; ++u) {
            pqo[u] = 0u;
            if (u * kBrickBlk < npq) {
                const int q = tid + u * kBrickBlk;
                pqo[u] = bw[o_pq + (q < npq ? q : 0)];
            }
        }
        const uint32_t pinf = bw[o_pi + (tid < npat ? tid : 0)];
        {
            uint2 rw[kRuFast];
#pragma unroll
            for (int u = 0; u < kRuFast; ++u) {
                rw[u] = uint2{0u, 0u};
                if (u * QW < nruns) {                  // block-uniform: a batch nobody needs is not requested
                    const int q = u * QW + qw;
                    rw[u] = runs2[q < nruns ? q : 0];
                }
            }
#pragma unroll
            for (int u = 0; u < kRuFast; ++u) {
                fv[u] = 0;
                rdsc[u] = 0xffffffffu;
                if (u * QW < nruns) {
                    const int q = u * QW + qw;
                    const bool on = q < nruns && l16 <= (int)(rw[u].y & 15u) && !BRICK_DBG(1);
                    rdsc[u] = on ? rw[u].y : 0xffffffffu;
                    fv[u] = ld_u32(x, on ? rw[u].x + (unsigned)l16 : (unsigned)row0);
                }
            }
        }
        T xo[RPT];
        uint32_t os[RPT];
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            xo[k] = 0;
            os[k] = 0xffffu;
            if (!emode && k * kBrickBlk < nrows) {
                const int r = tid + k * kBrickBlk;
                xo[k] = ld_u32(x + row0, (unsigned)(r < nrows ? r : 0));
                os[k] = ld_u32(B.ownslot + row0, (unsigned)(r < nrows ? r : 0));   // (a clamped lane re-reads row 0's slot: it is not written, see below)
            }
        }
        uint4 pqv[PQ];
#pragma unroll
        for (int u = 0; u < PQ; ++u) {
            pqv[u] = uint4{0u, 0u, 0u, 0u};
            if (u * kBrickBlk < npq) pqv[u] = *reinterpret_cast<const uint4 *>(B.pwords + pqo[u]);
        }
        V tval = 0;
        if (VC && ntv > 0) tval = (V)ld_u32(B.ttab + tt0, (unsigned)(tid < ntv ? tid : 0));   // the tile's value table (<= kBrickTileVals entries)
        int cbo[RPT];                                  // VC: first quad of this wave's blocks of the code stream (read NOW: the streamed rows'
                                                       // products overwrite the block image while slower waves still walk their rows)
#pragma unroll
        for (int k = 0; k < RPT; ++k) cbo[k] = VC ? __builtin_amdgcn_readfirstlane((int)bw[16 + k * (kBrickBlk / 64) + (tid >> 6)]) : 0;
        uint2 rdv[RPT]; // descriptor, position in the tile (valid for tid + k * kBrickBlk < nprow)
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            rdv[k] = uint2{0u, 0u};
            if (k * kBrickBlk < nprow) {
                const int i = tid + k * kBrickBlk;
#ifdef AVS_EXP_MNT
                {
                    typedef unsigned u2v __attribute__((ext_vector_type(2)));
                    const u2v v = __builtin_nontemporal_load(reinterpret_cast<const u2v *>(reinterpret_cast<const char *>(B.rdesc + rd0) + (size_t)((unsigned)(i < nprow ? i : 0) * 8u)));
                    rdv[k] = uint2{v.x, v.y};
                }
#else
                rdv[k] = ld_u32(B.rdesc + rd0, (unsigned)(i < nprow ? i : 0));
#endif
            }
        }
        // streamed rows (few tiles): descriptors (valid for brick_srow_of_thread(tid, k) < nsrows), and for a G tile the first pass of words with their x
        uint2 sd[kBrickMaxRows / kBrickBlk];
#pragma unroll
        for (int k = 0; k < kBrickMaxRows / kBrickBlk; ++k) sd[k] = uint2{0u, 0u};
        uint32_t w0[2] = {0u, 0u};
        T xv0[2] = {0, 0};
        constexpr bool LATE_SD = MIX && VC; // (8-B values: the descriptors of the streamed rows are fetched behind the row walk instead of living across it)
        if (nsrows > 0) {
            if (!LATE_SD) {
#pragma unroll
            for (int k = 0; k < kBrickMaxRows / kBrickBlk; ++k) {
                if (k * kBrickBlk >= nsrows) break;
                const int i = brick_srow_of_thread(tid, k);
                sd[k] = B.sdesc[srow0 + (i < nsrows ? i : 0)];
            }
            }
            if (!emode && !wide) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int e = tid + u * kBrickBlk;
                    w0[u] = B.swords[(int64_t)sword0 + (e < nsw ? e : 0)];
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) xv0[u] = x[w0[u] & cmask];
            }
        }
        // the next tile's block address: a scalar load, in flight while this tile's data arrives
        const bool more = iter + 1 < cnt;
        const uint2 tbn = seq[(int64_t)(more ? iter + 1 : iter) * step];
        // ---- LDS writes
        if (VC && tid <= ntv) vals[tid] = tid < ntv ? tval : (V)0;          // (entry ntv = 0.0: the code of the padding words)
        if (tid < npat) pinfo[tid] = pinf;
#pragma unroll
        for (int u = 0; u < PQ; ++u) {
            const int q = tid + u * kBrickBlk;
            if (q < npq) reinterpret_cast<uint4 *>(pw)[q] = pqv[u];
        }
#pragma unroll
        for (int u = 0; u < kRuFast; ++u)
            if (rdsc[u] != 0xffffffffu) xs[((rdsc[u] >> 4) & 0xfffu) + l16] = fv[u]; // (extra slots: xs runs on into `park`)
        if (nruns > kRuFast * QW && !BRICK_DBG(1)) {   // (block-uniform, rare) the runs beyond the register batches: straight into LDS
#pragma unroll 1
            for (int q = kRuFast * QW + qw; q < nruns; q += QW) {
                const uint2 r = runs2[q];
                if (l16 <= (int)(r.y & 15u)) xs[((r.y >> 4) & 0xfffu) + l16] = ld_u32(x, r.x + (unsigned)l16);
            }
        }
#pragma unroll
        for (int k = 0; k < RPT; ++k)
            if (!emode && tid + k * kBrickBlk < nrows && os[k] != 0xffffu) xs[os[k]] = xo[k];
        __syncthreads();
        BRICK_STAMP(2);

        if (AVS_BRICK_PRIO >= 1) __builtin_amdgcn_s_setprio(0);
        // ---- the next tile's block travels while this tile is multiplied (16 B per thread)
        blk = blocks16[(int64_t)tbn.x + (tid < (int)tbn.y ? tid : 0)];

        if (!emode) {
            // products of the first streamed pass (the block in `park` is dead now)
            if (nsw > 0 && !wide) {
                if (tid < nsw && tid < cap) prod[tid] = vals[w0[0] >> cbits] * (V)xv0[0];
                if (tid + kBrickBlk < nsw && tid + kBrickBlk < cap) prod[tid + kBrickBlk] = vals[w0[1] >> cbits] * (V)xv0[1];
            }
            // pattern rows: one lane per row, everything from LDS
#pragma unroll
            for (int k = 0; k < RPT; ++k) {
            if (k * kBrickBlk >= nprow) break;
            if (tid + k * kBrickBlk < nprow && !BRICK_DBG(2)) {
                const uint32_t rd = rdv[k].x, ro = rdv[k].y;
                const unsigned pid = rd >> 20;
                const int lr = (int)((rd >> 18) & 3u), ax = (int)((rd >> 16) & 3u);
                const uint2 *rb = rbt + lr * 10;
                const uint2 tx = rb[rd & 15u], ty = rb[40 + ((rd >> 4) & 15u)], tz = rb[80 + ((rd >> 8) & 15u)];
                const unsigned P01 = tx.x + ty.x + tz.x, P23 = tx.y + ty.y + tz.y; // byte offsets of the row's base on the four lattices
                const unsigned own8 = __builtin_amdgcn_perm(P23, P01, (unsigned)lr * 0x0202u + 0x0c0c0100u) + ES * (unsigned)ax;
                const unsigned pi = pinfo[pid];
                const uint4 *wq = reinterpret_cast<const uint4 *>(pw + (pi & 0xffffu));
                const int nq = (int)((pi >> 16) & 0x7fffu);
                // (the wave's chunk of the execution order is one of the tile's last two: a scalar test -- as a per-lane test on the row index it
                //  cost two more spilled registers and made the kernel 4 % SLOWER than no priority at all)
#ifdef AVS_BRICK_GRADED
                {
                    const int back = ((nprow + 63) >> 6) - (k * (kBrickBlk / 64) + wave_id); // 1 = the last chunk
                    if (back <= 2) __builtin_amdgcn_s_setprio(2);
                    else if (back <= 4) __builtin_amdgcn_s_setprio(1);
                }
#else
                if (AVS_BRICK_PRIO == 2 ? wave_id >= 6 : (AVS_BRICK_PRIO >= 3 && k * (kBrickBlk / 64) + wave_id + AVS_BRICK_TAIL >= ((nprow + 63) >> 6))) __builtin_amdgcn_s_setprio(AVS_BRICK_TAIL_PRIO);
#endif
                // word: delta << 19 (signed 13) | 000 | lattice level << 14 | code << 3 -- byte offsets for 8-B elements; T = float reads
                // the 4-B image of the table (BrickView::pwords32: delta << 18 | level << 14 | code << 2).  A pattern is padded to whole
                // quads with words that repeat its first entry's slot with the code of 0.0: +-0.0 added to a sum that is never -0.0.
                constexpr unsigned CM = ES == 8 ? 0x3ff8u : 0x1ffcu;       // the code field as a byte offset into `vals`
                constexpr int VS = sizeof(V) == 8 ? 0 : 1;                // VC: the code stream holds byte offsets for 8-B values
                constexpr int CS = MIX ? 1 : 0;                           // 4-B pattern image, 8-B values: code << 2 -> code << 3
                auto addr = [&](uint32_t w) -> unsigned {
                    const unsigned sel = ((w >> 14) & 3u) * 0x0202u + 0x0c0c0100u;
                    return (unsigned)((int)w >> 16) + __builtin_amdgcn_perm(P23, P01, sel); // + 16-bit field number `level` of P23:P01
                };
                V sum = 0;
                // software pipeline: the words of quad q + 1 and the value / x reads of quad q are in flight while quad q - 1 is added
                // (reading the words one quad past the pattern is harmless: the LDS image ends with spare quads; they are never decoded)
                auto walk = [&](auto adr) {
                    V v0, v1, v2, v3;
                    T x0, x1, x2, x3;
                    const uint4 w = wq[0];
                    uint4 wn = wq[1];
                    v0 = lds_abs<V>(kValsByte + ((w.x & CM) << CS)); x0 = lds_abs<T>(adr(w.x));
                    v1 = lds_abs<V>(kValsByte + ((w.y & CM) << CS)); x1 = lds_abs<T>(adr(w.y));
                    v2 = lds_abs<V>(kValsByte + ((w.z & CM) << CS)); x2 = lds_abs<T>(adr(w.z));
                    v3 = lds_abs<V>(kValsByte + ((w.w & CM) << CS)); x3 = lds_abs<T>(adr(w.w));
                    for (int q = 1; q < nq; ++q) {
                        const uint4 wnn = wq[q + 1];
                        const V a0 = lds_abs<V>(kValsByte + ((wn.x & CM) << CS)); const T c0 = lds_abs<T>(adr(wn.x));
                        const V a1 = lds_abs<V>(kValsByte + ((wn.y & CM) << CS)); const T c1 = lds_abs<T>(adr(wn.y));
                        const V a2 = lds_abs<V>(kValsByte + ((wn.z & CM) << CS)); const T c2 = lds_abs<T>(adr(wn.z));
                        const V a3 = lds_abs<V>(kValsByte + ((wn.w & CM) << CS)); const T c3 = lds_abs<T>(adr(wn.w));
                        sum += v0 * (V)x0;
                        sum += v1 * (V)x1;
                        sum += v2 * (V)x2;
                        sum += v3 * (V)x3;
                        v0 = a0; x0 = c0; v1 = a1; x1 = c1; v2 = a2; x2 = c2; v3 = a3; x3 = c3;
                        wn = wnn;
                    }
                    sum += v0 * (V)x0;
                    sum += v1 * (V)x1;
                    sum += v2 * (V)x2;
                    sum += v3 * (V)x3;
                };
                // VC: the value of an entry comes from the row's own code stream -- quad q of this lane at cp[64 q] (the wave's rows are
                // interleaved, so a wave load is one 512-B run) -- instead of from the pattern word; same pipeline, same order of additions
                auto walk_vc = [&](auto adr) {
                    const uint2 *cp = B.vcodes + (int64_t)cw0 + cbo[k] + lane;
                    V v0, v1, v2, v3;
                    T x0, x1, x2, x3;
                    const uint4 w = wq[0];
                    uint4 wn = wq[1];
                    uint2 c = cp[0];
                    uint2 cn = cp[nq > 1 ? 64 : 0];
                    v0 = lds_abs<V>(kValsByte + ((c.x & 0xffffu) >> VS)); x0 = lds_abs<T>(adr(w.x));
                    v1 = lds_abs<V>(kValsByte + ((c.x >> 16) >> VS)); x1 = lds_abs<T>(adr(w.y));
                    v2 = lds_abs<V>(kValsByte + ((c.y & 0xffffu) >> VS)); x2 = lds_abs<T>(adr(w.z));
                    v3 = lds_abs<V>(kValsByte + ((c.y >> 16) >> VS)); x3 = lds_abs<T>(adr(w.w));
                    for (int q = 1; q < nq; ++q) {
                        const uint4 wnn = wq[q + 1];
                        const uint2 cnn = cp[(q + 1 < nq ? q + 1 : q) * 64];
                        const V a0 = lds_abs<V>(kValsByte + ((cn.x & 0xffffu) >> VS)); const T c0 = lds_abs<T>(adr(wn.x));
                        const V a1 = lds_abs<V>(kValsByte + ((cn.x >> 16) >> VS)); const T c1 = lds_abs<T>(adr(wn.y));
                        const V a2 = lds_abs<V>(kValsByte + ((cn.y & 0xffffu) >> VS)); const T c2 = lds_abs<T>(adr(wn.z));
                        const V a3 = lds_abs<V>(kValsByte + ((cn.y >> 16) >> VS)); const T c3 = lds_abs<T>(adr(wn.w));
                        sum += v0 * (V)x0;
                        sum += v1 * (V)x1;
                        sum += v2 * (V)x2;
                        sum += v3 * (V)x3;
                        v0 = a0; x0 = c0; v1 = a1; x1 = c1; v2 = a2; x2 = c2; v3 = a3; x3 = c3;
                        wn = wnn;
                        cn = cnn;
                    }
                    sum += v0 * (V)x0;
                    sum += v1 * (V)x1;
                    sum += v2 * (V)x2;
                    sum += v3 * (V)x3;
                };
                // (a queue of four code quads per lane, the first four loaded with the tile's other loads, was measured: 20 spilled registers, 288 us)
                if (pi >> 31) { // every column of the pattern on the level-0 lattice (rows are executed sorted by pattern: waves rarely mix)
                    const unsigned b0 = P01 & 0xffffu;
                    if (VC) walk_vc([&](uint32_t w) -> unsigned { return (unsigned)((int)w >> 16) + b0; });
                    else walk([&](uint32_t w) -> unsigned { return (unsigned)((int)w >> 16) + b0; });
                } else {
                    if (VC) walk_vc(addr);
                    else walk(addr);
                }
#ifdef AVS_EXP_YNT
                __builtin_nontemporal_store((T)sum, reinterpret_cast<T *>(reinterpret_cast<char *>(y + row0) + (size_t)(unsigned)(ro * ES)));
#else
                *reinterpret_cast<T *>(reinterpret_cast<char *>(y + row0) + (size_t)(unsigned)(ro * ES)) = (T)sum;
#endif
                if (AVS_BRICK_PRIO >= 2) __builtin_amdgcn_s_setprio(0);
                if (DOT) dot += sum * (V)lds_abs<T>(own8);
            }
            }
        }
        BRICK_STAMP(3);
        // streamed rows: passes of `cap` products parked in LDS, then every row adds its segment left to right
        if (nsw > 0 && !BRICK_DBG(4)) {
#ifdef AVS_EXP_SPRIO
            __builtin_amdgcn_s_setprio(1);
#endif
            V ssum[kBrickMaxRows / kBrickBlk];
            if (LATE_SD) {
#pragma unroll
                for (int k = 0; k < kBrickMaxRows / kBrickBlk; ++k) {
                    if (k * kBrickBlk >= nsrows) break;
                    const int i = brick_srow_of_thread(tid, k);
                    sd[k] = B.sdesc[srow0 + (i < nsrows ? i : 0)];
                }
            }
#pragma unroll
            for (int k = 0; k < kBrickMaxRows / kBrickBlk; ++k) ssum[k] = 0;
            for (int ts = 0; ts < nsw; ts += cap) {
                const int te = (ts + cap < nsw) ? ts + cap : nsw;
                if (emode || wide || ts > 0) {
                    if (ts > 0) __syncthreads(); // the previous pass has been summed
                    constexpr int SU = 4; // (8 entries per thread -- a whole pass of an E tile in one round of loads -- was measured SLOWER: 7.1 -> 7.7 us per E tile)
                    for (int e0 = ts + tid; e0 < te; e0 += SU * kBrickBlk) {
                        uint32_t w4[SU], c4[SU];
                        T x4[SU];
                        V v4[SU];
#pragma unroll
                        for (int u = 0; u < SU; ++u) {
                            const int e = e0 + u * kBrickBlk;
                            const int64_t at = (int64_t)sword0 + (e < te ? e : ts);
                            v4[u] = 0;
                            if (VC) { // 12 B per entry: column, value
                                const uint32_t *w = B.swords + 3 * at;
                                w4[u] = w[0];
                                c4[u] = 0u;
                                v4[u] = (V)__hiloint2double((int)w[2], (int)w[1]);
                            } else if (wide) {
                                const uint2 w = reinterpret_cast<const uint2 *>(B.swords)[at];
                                w4[u] = w.x;
                                c4[u] = w.y;
                            } else {
                                const uint32_t w = B.swords[at];
                                w4[u] = w & cmask;
                                c4[u] = w >> cbits;
                            }
                        }
#pragma unroll
                        for (int u = 0; u < SU; ++u) x4[u] = x[w4[u]];
#pragma unroll
                        for (int u = 0; u < SU; ++u) {
                            const int e = e0 + u * kBrickBlk;
                            if (e < te) prod[e - ts] = (VC ? v4[u] : vals[c4[u]]) * (V)x4[u];
                        }
                    }
                }
                __syncthreads();
#pragma unroll
                for (int k = 0; k < kBrickMaxRows / kBrickBlk; ++k) {
                    const int len = brick_srow_of_thread(tid, k) < nsrows ? (int)(sd[k].x >> 16) : 0, st = (int)sd[k].y;
                    const int a = st > ts ? st : ts, b = (st + len < te) ? st + len : te;
                    for (int j = a; j < b; ++j) ssum[k] += prod[j - ts];
                }
            }
#pragma unroll
            for (int k = 0; k < kBrickMaxRows / kBrickBlk; ++k)
                if (brick_srow_of_thread(tid, k) < nsrows && (sd[k].x >> 16) > 0) {
                    const int64_t row = (int64_t)row0 + (int)(sd[k].x & 0xffffu);
                    y[row] = (T)ssum[k];
                    if (DOT) dot += ssum[k] * (V)x[row];
                }
        }
#ifdef AVS_EXP_SPRIO
        __builtin_amdgcn_s_setprio(0);
#endif
        BRICK_STAMP(4);
        if (!more) break;
        ++iter;
        tb = tbn;
        nsw_prev = (nsw > 0 && !BRICK_DBG(4)) ? 1 : 0;
    }
    if (DOT) { // ONE partial per workgroup (fixed order: the tile walk is static, the waves' sums are added in wave order): few enough
               // for the vector kernel that follows to fold them itself instead of a reduction launch in between
        const double dsum = wave_sum_dpp((double)dot);                  // (float: a lane's few rows in float, everything across lanes in double)
        double *wsum = reinterpret_cast<double *>(park + kBrickXSlots);
        __syncthreads();                                                 // (the last tile's streamed sums may still be reading `park`)
        if (lane == 63) wsum[tid >> 6] = dsum;
        __syncthreads();
        if (tid == 0) {
            double s = wsum[0];
#pragma unroll
            for (int k = 1; k < kBrickBlk / 64; ++k) s += wsum[k];
            partial[blockIdx.x] = s;
        }
    }
}

// elem_bytes: of a vector element; val_bytes: of a matrix value in LDS (0: as the vectors; 8 with 4-B vectors = the mixed-precision kernel)
size_t brick_lds_bytes(const BrickView &B, int elem_bytes, int val_bytes)
{
    const size_t es = (size_t)elem_bytes, vs = val_bytes > 0 ? (size_t)val_bytes : es;
    const size_t vals = elem_bytes == 4 ? brick_vals_elems<float>(B.table_size) : brick_vals_elems<double>(B.table_size);
    return (size_t)(kBrickSlotsPad + kBrickXSlots) * es + kBrickBlockBytes + vals * vs +
           (size_t)((B.vc ? kBrickPatWordsVc : kBrickPatWords) + 8 + kBrickPatMax + 2 * kBrickRowBase) * sizeof(uint32_t);
}
size_t brick_lds_bytes(const BrickView &B, int elem_bytes) { return brick_lds_bytes(B, elem_bytes, 0); }
size_t brick_lds_bytes(const BrickView &B) { return brick_lds_bytes(B, B.f32 ? 4 : 8, B.f32 == 2 ? 8 : 0); }

// LDS a workgroup may ask for on this device (the kernel opts in to more than the default 48 KiB, hipFuncSetAttribute below)
constexpr size_t kBrickLdsLimit = 64 * 1024;
bool brick_lds_fits(const BrickView &B) { return brick_lds_bytes(B, 8) <= kBrickLdsLimit; }

template <typename T, typename V = T>
static const void *brick_kernel(bool dot, bool vc)
{
    if (vc) return dot ? (const void *)k_spmv_brick<true, true, T, V> : (const void *)k_spmv_brick<false, true, T, V>;
    return dot ? (const void *)k_spmv_brick<true, false, T, V> : (const void *)k_spmv_brick<false, false, T, V>;
}

// persistent grid: as many workgroups as the device keeps resident for THIS LDS size (a larger value table costs a workgroup per CU;
// the float kernel's lattice is half as large: four per CU); queried once per (device, LDS size, variant), guarded: contexts of several
// host threads share the cache
#ifdef AVS_PROBES
static thread_local int tl_probe_grid = 0;
#endif
static int brick_grid(const BrickView &B, size_t lds, int elem_bytes, int val_bytes = 0)
{
    if (val_bytes == elem_bytes) val_bytes = 0;
    struct Entry { int dev; size_t lds; int vc, es, vs; int grid; };
    static std::mutex mu;
    static std::vector<Entry> cache;
    int dev = 0;
    (void)hipGetDevice(&dev);
    int g = 0;
    {
        std::lock_guard<std::mutex> lk(mu);
        for (const Entry &e : cache)
            if (e.dev == dev && e.lds == lds && e.vc == B.vc && e.es == elem_bytes && e.vs == val_bytes) g = e.grid;
        if (!g) {
            int per_cu = 0, cus = 0;
            const void *fn = elem_bytes == 4 ? (val_bytes == 8 ? brick_kernel<float, double>(true, B.vc != 0) : brick_kernel<float>(true, B.vc != 0))
                                             : brick_kernel<double>(true, B.vc != 0);
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kBrickBlk, lds);
            (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
            if (per_cu < 1) per_cu = 1;
            if (cus < 1) cus = 256;
            g = per_cu * cus;
            cache.push_back(Entry{dev, lds, B.vc, elem_bytes, val_bytes, g});
        }
    }
#ifdef AVS_PROBES
    if (const char *e = getenv("AVS_BRICK_GRID")) g = atoi(e) > 0 ? atoi(e) : g;
    if (tl_probe_grid > 0) g = tl_probe_grid; // avs_brick_form_probe: the persistent grid as an argument
#endif
    return g < B.ntiles ? g : B.ntiles;
}

// the kernel's dynamic LDS limit is a per-device attribute of the loaded code object: raised once per device
static avs_status brick_raise_lds_limit()
{
    static std::mutex mu;
    static bool done[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64) dev = 0;
    std::lock_guard<std::mutex> lk(mu);
    if (done[dev]) return AVS_OK;
    for (int dot = 0; dot < 2; ++dot)
        for (int vc = 0; vc < 2; ++vc) {
            AVS_HIP(hipFuncSetAttribute(brick_kernel<double>(dot, vc), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBrickLdsLimit));
            AVS_HIP(hipFuncSetAttribute(brick_kernel<float>(dot, vc), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBrickLdsLimit));
            AVS_HIP(hipFuncSetAttribute(brick_kernel<float, double>(dot, vc), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBrickLdsLimit));
        }
    done[dev] = true;
    return AVS_OK;
}

#ifdef AVS_PROBES
// phase times of the last launch with AVS_BRICK_DEBUG & 16, in 10-ns ticks: mean over workgroups and tiles
static void brick_print_stamps()
{
    std::vector<long long> hs((size_t)kStampWgs * kStampTiles * 8);
    if (hipMemcpyFromSymbol(hs.data(), HIP_SYMBOL(g_brick_stamps), hs.size() * sizeof(long long)) != hipSuccess) return;
    if (const char *path = getenv("AVS_BRICK_STAMP_FILE")) { // raw stamps [workgroup][tile of its walk][8] for tools/probes/brick_cost_fit.py
        if (FILE *f = fopen(path, "wb")) {
            const int hdr[4] = {kStampWgs, kStampTiles, 8, 0};
            fwrite(hdr, sizeof(hdr), 1, f);
            fwrite(hs.data(), sizeof(long long), hs.size(), f);
            fclose(f);
        }
    }
    static const char *kind[3] = {"G tiles", "E tiles", "G tiles with streamed rows"};
    for (int ty = 0; ty < 3; ++ty) {
        double acc[6] = {};
        long cnt = 0;
        for (int w = 0; w < kStampWgs; ++w)
            for (int i = 1; i + 1 < kStampTiles; ++i) {
                const long long *p = &hs[((size_t)w * kStampTiles + i) * 8], *pn = p + 8;
                if (!p[0] || !p[4] || !pn[0] || p[5] != ty) continue;
                acc[0] += (double)(p[1] - p[0]); acc[1] += (double)(p[2] - p[1]); acc[2] += (double)(p[3] - p[2]);
                acc[3] += (double)(p[4] - p[3]); acc[4] += (double)(pn[0] - p[4]); acc[5] += (double)(pn[0] - p[0]);
                ++cnt;
            }
        if (cnt)
            fprintf(stderr, "brick phases (us, mean of %ld %s): block to LDS + barrier %.2f | issue loads, LDS writes, barrier %.2f | pattern rows %.2f | streamed + dot %.2f | loop %.2f | tile %.2f\n",
                    cnt, kind[ty], acc[0] / cnt / 100, acc[1] / cnt / 100, acc[2] / cnt / 100, acc[3] / cnt / 100, acc[4] / cnt / 100, acc[5] / cnt / 100);
    }
}
#endif

// partial sums of x.y the fused-dot launch writes: one per workgroup of the persistent grid (of the kernel the view is laid out for:
// BrickView::f32 -- the planned walk and the partial arrays follow that grid)
int brick_partial_count_mixed(const BrickView &B);
int brick_partial_count(const BrickView &B)
{
    if (B.f32 == 2) return brick_partial_count_mixed(B);
    const int es = B.f32 ? 4 : 8;
    return B.ntiles > 0 ? brick_grid(B, brick_lds_bytes(B, es), es) : 0;
}
int brick_partial_count(const BrickView &B, int elem_bytes)
{
    return B.ntiles > 0 ? brick_grid(B, brick_lds_bytes(B, elem_bytes), elem_bytes) : 0;
}
int brick_partial_count_mixed(const BrickView &B) // of k_spmv_brick<.., float, double>
{
    return B.ntiles > 0 ? brick_grid(B, brick_lds_bytes(B, 4, 8), 4, 8) : 0;
}

template <typename T, typename V = T>
static avs_status spmv_brick_launch_t(const BrickView &B0, const T *x, T *y, double *partial, const int *done_flag, hipStream_t stream)
{
    if (B0.ntiles <= 0) return AVS_OK;
    constexpr int es = (int)sizeof(T), vs = (int)sizeof(V);
    const size_t lds = brick_lds_bytes(B0, es, vs);
    AVS_REQUIRE(lds <= kBrickLdsLimit, AVS_EINTERNAL, "brick form: %zu bytes of LDS per workgroup exceed the limit (value table of %d entries)", lds,
                B0.table_size);
    AVS_TRY(brick_raise_lds_limit());
    const int grid = brick_grid(B0, lds, es, vs);
    BrickView B = B0;
    if (es == 4) {
        AVS_REQUIRE(B.pwords32, AVS_EINTERNAL, "brick form: no 4-byte pattern image for the float kernel");
        B.pwords = B.pwords32;
    }
#ifdef AVS_PROBES
    const int dbg = getenv("AVS_BRICK_DEBUG") ? atoi(getenv("AVS_BRICK_DEBUG")) : 0; // phase switches / stamps (measurement builds only; read per launch: a probe script flips it)
    B.debug |= dbg;
#endif
    if (B.vc) {
        if (partial) hipLaunchKernelGGL((k_spmv_brick<true, true, T, V>), dim3(grid), dim3(kBrickBlk), lds, stream, B, x, y, partial, done_flag);
        else hipLaunchKernelGGL((k_spmv_brick<false, true, T, V>), dim3(grid), dim3(kBrickBlk), lds, stream, B, x, y, partial, done_flag);
    } else if (partial) hipLaunchKernelGGL((k_spmv_brick<true, false, T, V>), dim3(grid), dim3(kBrickBlk), lds, stream, B, x, y, partial, done_flag);
    else hipLaunchKernelGGL((k_spmv_brick<false, false, T, V>), dim3(grid), dim3(kBrickBlk), lds, stream, B, x, y, partial, done_flag);
    AVS_HIP(hipGetLastError());
#ifdef AVS_PROBES
    if (B.debug & 64) { // print the phase stamps of THIS launch (synchronises: not for timing loops)
        AVS_HIP(hipStreamSynchronize(stream));
        brick_print_stamps();
    }
#endif
    return AVS_OK;
}
avs_status spmv_brick_launch(const BrickView &B, const double *x, double *y, double *partial, const int *done_flag, hipStream_t stream)
{
    return spmv_brick_launch_t<double>(B, x, y, partial, done_flag, stream);
}
avs_status spmv_brick_launch_f32(const BrickView &B, const float *x, float *y, double *partial, const int *done_flag, hipStream_t stream)
{
    return spmv_brick_launch_t<float>(B, x, y, partial, done_flag, stream);
}
// the mixed-precision loop's product (avs_pcg_mixed.inl): float x and y, the fp64 value table
avs_status spmv_brick_launch_mixed(const BrickView &B, const float *x, float *y, double *partial, const int *done_flag, hipStream_t stream)
{
    return spmv_brick_launch_t<float, double>(B, x, y, partial, done_flag, stream);
}

} // namespace avs

#ifdef AVS_PROBES
// Measurement / test entry: SpMV on a brick form whose arrays the caller built (tools/brick_build.py: the torch reference builder the
// device builder is tested against).  Device pointers.
extern "C" avs_status avs_brick_spmv_probe(const avs_brick_arrays *a, const double *x, double *y, double *partial, int32_t repeats,
                                           void *stream, double *ms_per_launch)
{
    AVS_REQUIRE(a && x && y && repeats > 0, AVS_EINVAL, "bad argument");
    AVS_REQUIRE(a->table_size > 0 && a->table_size < avs::kBrickTableMax, AVS_EINVAL, "value table size %d out of range", a->table_size);
    avs::BrickView B;
    B.ntiles = a->ntiles;
    B.tile_blk = reinterpret_cast<const uint2 *>(a->tile_blk);
    B.blocks = a->blocks;
    B.rdesc = reinterpret_cast<const uint2 *>(a->rdesc);
    B.ownslot = a->ownslot;
    B.pwords = a->pwords;
    B.sdesc = reinterpret_cast<const uint2 *>(a->sdesc);
    B.swords = a->swords;
    B.table = a->table;
    B.table_size = a->table_size;
    B.col_bits = a->col_bits;
    if (const char *e = getenv("AVS_BRICK_DEBUG")) B.debug = atoi(e);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    AVS_TRY(avs::spmv_brick_launch(B, x, y, partial, nullptr, st));
    avs::Timer t(st);
    t.start();
    for (int i = 0; i < repeats; ++i) AVS_TRY(avs::spmv_brick_launch(B, x, y, partial, nullptr, st));
    const double ms = t.stop() / repeats;
    if (ms_per_launch) *ms_per_launch = ms;
    if (B.debug & 16) avs::brick_print_stamps();
    return AVS_OK;
}

namespace avs {
namespace {
__global__ void k_bfp_narrow(int64_t n, const double *__restrict__ src, float *__restrict__ dst)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (float)src[i];
}
__global__ void k_bfp_widen(int64_t n, const float *__restrict__ src, double *__restrict__ dst)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (double)src[i];
}
__global__ void k_bfp_iota(int64_t n, int32_t *__restrict__ dst)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (int32_t)i;
}
struct ProbeGridScope { // the persistent grid of avs_brick_form_probe, for the launches and counts of this call
    explicit ProbeGridScope(int g) { tl_probe_grid = g; }
    ~ProbeGridScope() { tl_probe_grid = 0; }
};
// most tiles a workgroup of the strided walks takes: the kernel's tile -> workgroup rule, on the host
int brick_probe_max_walk(int ntiles, int grid, int walk)
{
    int most = 0;
    for (int b = 0; b < grid; ++b) {
        int tile = b, tstep = grid, tend = ntiles;
        if ((grid & 7) == 0 && ntiles >= grid) {
            const int c = b & 7, gx = grid >> 3;
            tile = c * gx + (b >> 3);
            if (walk == 0) {
                tstep = gx;
                tile = (int)(((int64_t)ntiles * c) >> 3) + (b >> 3);
                tend = (int)(((int64_t)ntiles * (c + 1)) >> 3);
            }
        }
        const int cnt = tile < tend ? (tend - tile + tstep - 1) / tstep : 0;
        most = std::max(most, cnt);
    }
    return most;
}
} // namespace
} // namespace avs

extern "C" avs_status avs_brick_form_probe(int64_t n_rows, int64_t n_cols, const int32_t *row_ptr, const int32_t *col, const double *val,
                                           const int32_t *dof, int32_t nx, int32_t ny, int32_t nz, int32_t levels, const double *x, double *y,
                                           int32_t flags, int32_t grid, int32_t walk, double *dot_out, double *partials,
                                           int32_t partial_capacity, avs_brick_form_info *info, int32_t *headers, int32_t header_capacity,
                                           void *stream)
{
    using namespace avs;
    OptScope opt_scope_(nullptr); // context-free entry: the environment as it is now
    AVS_REQUIRE(info && info->struct_size >= (int32_t)sizeof(avs_brick_form_info), AVS_EINVAL,
                "avs_brick_form_info.struct_size must be set to sizeof(avs_brick_form_info) before the call");
    {
        constexpr int RL = kBrickRunLen;
        const int32_t size = info->struct_size;
        memset(info, 0, sizeof(*info));
        info->struct_size = size;
        info->run_len = kBrickRunLen;
        info->max_runs = kBrickMaxRuns;
        info->fast_runs = (AVS_BRICK_RUFAST) * (kBrickBlk / RL);
        info->pat_max = kBrickPatMax;
        info->pat_words = kBrickPatWords;
        info->pat_words_vc = kBrickPatWordsVc;
        info->pat_len = kBrickPatLen;
        info->x_slots = kBrickXSlots;
        info->park_words = kBrickPark - kBrickXSlots;
        info->emode_words = kBrickSlotsPad;
        info->emode_words_mixed = (int32_t)(kBrickSlotsPad * sizeof(float) / sizeof(double));
        info->min_rows = kBrickMinRows;
        info->max_rows = kBrickMaxRows;
        info->etile_rows = kBrickETileRows;
        info->tile_vals = kBrickTileVals;
        info->table_max = kBrickTableMax;
        info->block_words = kBrickBlockStride;
        info->header_words = kBlkHdrWords;
    }
    if (n_rows == 0 && !row_ptr) return AVS_OK; // the limits only: no device
    AVS_REQUIRE(n_rows > 0 && n_cols >= n_rows && n_cols < (1ll << 31) - 64 && row_ptr && col && val && dof && x && y, AVS_EINVAL, "bad argument");
    AVS_REQUIRE(nx > 0 && ny > 0 && nz > 0 && nx <= 1024 && ny <= 1024 && nz <= 1024 && levels >= 1 && levels <= 8, AVS_EINVAL, "bad grid");
    constexpr int kAll = AVS_BRICK_PROBE_FUSED_DOT | AVS_BRICK_PROBE_F32 | AVS_BRICK_PROBE_MIXED | AVS_BRICK_PROBE_VALUE_CODES | AVS_BRICK_PROBE_DONE;
    AVS_REQUIRE((flags & ~kAll) == 0, AVS_EINVAL, "unknown flags 0x%x", (unsigned)flags);
    AVS_REQUIRE(!((flags & AVS_BRICK_PROBE_F32) && (flags & AVS_BRICK_PROBE_MIXED)), AVS_EINVAL, "F32 and MIXED exclude each other");
    AVS_REQUIRE(!(flags & AVS_BRICK_PROBE_DONE) || (flags & AVS_BRICK_PROBE_FUSED_DOT), AVS_EINVAL, "DONE needs FUSED_DOT: only that instantiation reads the flag");
    AVS_REQUIRE(grid >= 0 && grid <= 4096 && walk >= 0 && walk <= 2, AVS_EINVAL, "grid %d or walk %d out of range", grid, walk);
    AVS_REQUIRE(!partials || partial_capacity > 0, AVS_EINVAL, "partials without a capacity");
    const bool fused = (flags & AVS_BRICK_PROBE_FUSED_DOT) != 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // ---- the input is checked on the host before anything is launched on it
    std::vector<int32_t> hrp((size_t)n_rows + 1), hdof((size_t)n_cols * 4);
    AVS_HIP(hipMemcpyAsync(hrp.data(), row_ptr, hrp.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    AVS_HIP(hipMemcpyAsync(hdof.data(), dof, hdof.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    AVS_HIP(hipStreamSynchronize(st));
    AVS_REQUIRE(hrp[0] == 0, AVS_EINVAL, "row_ptr[0] must be 0");
    for (int64_t r = 0; r < n_rows; ++r)
        AVS_REQUIRE(hrp[(size_t)r + 1] > hrp[(size_t)r], AVS_EINVAL, "row %lld is empty (or row_ptr decreases): the brick kernel does not write y for it", (long long)r);
    const int64_t nnz = hrp[(size_t)n_rows];
    {
        std::vector<int32_t> hcol((size_t)nnz);
        AVS_HIP(hipMemcpyAsync(hcol.data(), col, hcol.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        AVS_HIP(hipStreamSynchronize(st));
        for (int64_t k = 0; k < nnz; ++k)
            AVS_REQUIRE(hcol[(size_t)k] >= 0 && hcol[(size_t)k] < n_cols, AVS_EINVAL, "entry %lld: column %d outside [0, %lld)", (long long)k, hcol[(size_t)k], (long long)n_cols);
    }
    {
        const uint32_t nbx = (uint32_t)((nx + 7) >> 3), nby = (uint32_t)((ny + 7) >> 3);
        uint32_t prev = 0;
        for (int64_t c = 0; c < n_cols; ++c) {
            const int32_t *rec = &hdof[(size_t)c * 4];
            const int level = rec[0] & 0xff, axis = (rec[0] >> 8) & 0xff;
            AVS_REQUIRE((rec[0] >> 16) == 0 && level <= 7 && level < levels && axis <= 2 && rec[1] >= 0 && rec[1] < 2048 && rec[2] >= 0 && rec[2] < 2048 && rec[3] >= 0 && rec[3] < 2048,
                        AVS_EINVAL, "dof record %lld (level %d, axis %d, cell %d %d %d) does not fit the geometry key", (long long)c, level, axis, rec[1], rec[2], rec[3]);
            if (c >= n_rows) continue;
            int px = rec[1] << level, py = rec[2] << level, pz = rec[3] << level; // (the key of k_bk_geo)
            px = px < nx ? px : nx - 1;
            py = py < ny ? py : ny - 1;
            pz = pz < nz ? pz : nz - 1;
            const uint32_t brick = ((uint32_t)(pz >> 3) * nby + (uint32_t)(py >> 3)) * nbx + (uint32_t)(px >> 3);
            AVS_REQUIRE(c == 0 || brick >= prev, AVS_EINVAL, "row %lld (brick %u) follows a row of brick %u: the rows are not brick-major", (long long)c, brick, prev);
            prev = brick;
        }
    }
    // ---- value index, form
    ValueIndex vi, no_vi;
    AVS_TRY(build_matrix_index(row_ptr, col, val, n_rows, nnz, n_cols, vi, st));
    const ValueIndex &use_vi = (flags & AVS_BRICK_PROBE_VALUE_CODES) ? no_vi : vi; // no dictionary: the value-code variant
    DevBuf<int32_t> ref_id;
    AVS_TRY(ref_id.alloc((size_t)n_cols));
    hipLaunchKernelGGL(k_bfp_iota, dim3((unsigned)((n_cols + 255) / 256)), dim3(256), 0, st, n_cols, ref_id.p);
    BrickSource src;
    src.n_rows = n_rows;
    src.n_cols = n_cols;
    src.nnz = nnz;
    src.row_ptr = row_ptr;
    src.col = col;
    src.vi = &use_vi;
    src.val = val;
    src.vdof = dof;
    src.ref_id = ref_id.p;
    src.nx = nx; src.ny = ny; src.nz = nz;
    src.levels = levels;
    src.brick_shift = 3;
    BrickForm bf;
    const Options opt = cur_opt();
    AVS_TRY(build_brick_form(bf, src, opt, st));
    AVS_HIP(hipStreamSynchronize(st));
    info->ready = bf.ready ? 1 : 0;
    info->vc = bf.vc ? 1 : 0;
    info->wide = bf.wide ? 1 : 0;
    info->col_bits = use_vi.col_bits;
    info->table_size = use_vi.table_size;
    info->tiles = bf.ntiles;
    info->patterns = bf.patterns;
    info->halo_tiles = bf.halo_tiles;
    info->pattern_rows = bf.regular_rows;
    info->streamed_rows = bf.streamed_rows;
    info->streamed_words = bf.streamed_words;
    if (headers && bf.ntiles > 0 && bf.ntiles <= header_capacity) {
        std::vector<uint2> tb((size_t)bf.ntiles);
        AVS_HIP(hipMemcpy(tb.data(), bf.tile_blk.p, tb.size() * sizeof(uint2), hipMemcpyDeviceToHost));
        std::vector<uint32_t> hb((size_t)bf.ntiles * kBrickBlockStride);
        AVS_HIP(hipMemcpy(hb.data(), bf.blocks.p, hb.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (int t = 0; t < bf.ntiles; ++t)
            memcpy(headers + 16 * (size_t)t, &hb[(size_t)tb[(size_t)t].x * 4], 16 * sizeof(uint32_t));
    }
    if (dot_out) *dot_out = 0.;
    if (!bf.ready) { bf.release(); return AVS_OK; }
    // ---- the launch
    BrickView B;
    bf.view(B, use_vi);
    B.walk = walk == 0 ? 0 : 1;
    const int es = (flags & (AVS_BRICK_PROBE_F32 | AVS_BRICK_PROBE_MIXED)) ? 4 : 8;
    B.f32 = (flags & AVS_BRICK_PROBE_F32) ? 1 : ((flags & AVS_BRICK_PROBE_MIXED) ? 2 : 0);
    ProbeGridScope grid_scope(grid);
    const int g = brick_partial_count(B);
    info->grid = g;
    info->max_walk = brick_probe_max_walk(bf.ntiles, g, B.walk);
    if (walk == 2) {
        AVS_TRY(bf.plan_walk(g, 1, opt.brick_cost, st));
        if (bf.wgrid > 0) {
            bf.view(B, use_vi);
            B.walk = 1;
            B.f32 = (flags & AVS_BRICK_PROBE_F32) ? 1 : ((flags & AVS_BRICK_PROBE_MIXED) ? 2 : 0);
            info->planned = 1;
            std::vector<int32_t> hp((size_t)g + 1);
            AVS_HIP(hipMemcpy(hp.data(), bf.wptr.p, hp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            int most = 0;
            for (int b = 0; b < g; ++b) most = std::max(most, hp[(size_t)b + 1] - hp[(size_t)b]);
            info->max_walk = most;
        }
    }
    DevBuf<double> dpart;
    DevBuf<int> dflag;
    std::vector<double> hpart;
    if (fused) {
        const size_t np = std::max((size_t)g, (size_t)(partials ? partial_capacity : 0));
        AVS_REQUIRE(!partials || partial_capacity >= g, AVS_EINVAL, "%d partials do not fit a capacity of %d", g, partial_capacity);
        hpart.assign(np, 0.);
        if (partials) std::copy(partials, partials + partial_capacity, hpart.begin());
        AVS_TRY(dpart.alloc(np));
        AVS_HIP(hipMemcpyAsync(dpart.p, hpart.data(), np * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (flags & AVS_BRICK_PROBE_DONE) {
        AVS_TRY(dflag.alloc(1));
        const int one = 1;
        AVS_HIP(hipMemcpyAsync(dflag.p, &one, sizeof(int), hipMemcpyHostToDevice, st));
    }
    AVS_HIP(hipStreamSynchronize(st)); // (pageable sources)
    if (es == 8) {
        AVS_TRY(spmv_brick_launch(B, x, y, fused ? dpart.p : nullptr, dflag.p, st));
    } else {
        DevBuf<float> xf, yf;
        AVS_TRY(xf.alloc((size_t)n_cols));
        AVS_TRY(yf.alloc((size_t)n_rows));
        hipLaunchKernelGGL(k_bfp_narrow, dim3((unsigned)((n_cols + 255) / 256)), dim3(256), 0, st, n_cols, x, xf.p);
        hipLaunchKernelGGL(k_bfp_narrow, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, n_rows, (const double *)y, yf.p); // (DONE: y must come back as it went in)
        if (flags & AVS_BRICK_PROBE_MIXED) AVS_TRY(spmv_brick_launch_mixed(B, xf.p, yf.p, fused ? dpart.p : nullptr, dflag.p, st));
        else AVS_TRY(spmv_brick_launch_f32(B, xf.p, yf.p, fused ? dpart.p : nullptr, dflag.p, st));
        hipLaunchKernelGGL(k_bfp_widen, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, n_rows, (const float *)yf.p, y);
        AVS_HIP(hipGetLastError());
        AVS_HIP(hipStreamSynchronize(st)); // xf, yf die here
    }
    if (fused) {
        AVS_HIP(hipMemcpyAsync(hpart.data(), dpart.p, hpart.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        AVS_HIP(hipStreamSynchronize(st));
        double s = 0.;
        for (int b = 0; b < g; ++b) s += hpart[(size_t)b];
        if (dot_out && !(flags & AVS_BRICK_PROBE_DONE)) *dot_out = s;
        if (partials) std::copy(hpart.begin(), hpart.begin() + partial_capacity, partials);
    }
    AVS_HIP(hipStreamSynchronize(st)); // the form's arrays die here
    return AVS_OK;
}
#endif // AVS_PROBES
