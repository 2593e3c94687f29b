// avs_pcg_resident.inl -- CU-resident single-reduction PCG for systems that fit ON the chip (included by avs_pcg.hip).
//
// At 0.93 M rows per rank (the 8-way partition of the 512^3 headline system) an iteration of the launch-per-phase loop is two
// latency-bound kernels (k_sr_update_push 19 us + SpMV with its finalizer 42 us, profiles/r03_notes.md): neither the HBM nor the
// CUs are busy, the time goes into ramps, tails and dependent round trips.  MI355X has 512 KiB of VGPRs and 160 KiB of LDS per CU
// -- 168 MiB on the chip.  A rank's 14 M packed matrix words are 56 MB: they FIT IN THE REGISTER FILES.  So:
//
//   * ONE persistent workgroup of 1024 threads per CU (cooperative launch: all of them are resident), for the whole solve;
//   * every lane keeps the packed words (value code | column, 4 B) of its <= 6 consecutive rows in 64 VGPRs -- loaded once;
//   * the workgroup's slices of u, r, p, s live in LDS (4 x 8 B x <= 4.6 k rows); x and w = A u are touched by their owner lane
//     only and stay in global memory (L2-resident, 4 n doubles of traffic per iteration instead of 12 n + the matrix);
//   * an iteration = update (LDS) -> u to global (write-through) + boundary entries into the peers' halo areas -> grid barrier
//     (+ L1/L2 invalidate) -> SpMV from registers / LDS (columns of other workgroups: plain loads of the global u; of other
//     ranks: the comm block's halo area) -> ONE reduction: slot per workgroup, the last to arrive folds them in slot order,
//     all-gathers with the other ranks through the comm blocks (same sentinel-armed slots as dist_finalize), applies the scalar
//     step and publishes (alpha, beta, done, |r|^2) in sentinel-armed broadcast slots everybody polls.
//
// Same recurrences as k_sr_update_push + OP_SR_STEP (Chronopoulos-Gear), same left-to-right row sums (one lane per row), so the
// iterates agree with the launch-per-phase loop up to the order of additions inside the three dot products.
// T, the vector type: double, or float for AVS_PRECISION_F32 solves with AVS_OPTION_RESIDENT_F32 = 1 -- the partitioned float loop's
// arithmetic (k_sr_update_push<.., float>): x, w, u and the slices / remote columns / tables in LDS are floats (the value table staged
// as float: exact, the float system's values are floats; the inverse diagonal inverted in float, k_f32_invtab), float row sums, a
// thread's own terms of the dot products in T and everything across threads, workgroups and ranks in double, the scalar step
// sr_step_sums<float> on the float-rounded sums.  Halo entries travel widened to double (exact): the comm block is the same.
// LT, local value tables (AVS_OPTION_RESIDENT_LOCAL_TABLES, opt-in): a matrix without one dictionary of <= 1,023 values (a viscosity /
// density field; tile-local tables, column windows, 6-B or 12-B words at the assembly) gets a value table per workgroup -- per wave where
// a workgroup's code bits do not fit the 25-bit word -- built by the plan from the plain CSR values (k_resident_local_tables), and reads
// one inverse of the diagonal per row (the launch-per-phase loops' array) instead of a code and a second table.  Same row sums.
// Every wait is bounded (wall_clock64): a missing workgroup / peer ends the kernel with sc->fault set, never a hung GPU.
// Not used when two ranks share one physical GPU (two kernels that each need every CU cannot wait for each other).

#include <time.h>

// (kResThreads, kResQuads, kResQuadWords, kResRowsMax, kResWordBits and the lane_meta layout: avs_resident_plan.hpp, shared with the planner)
#ifndef AVS_RES_UPD
#define AVS_RES_UPD 4
#endif
#ifndef AVS_RES_FILL
#define AVS_RES_FILL 4
#endif
static constexpr int kResFill = AVS_RES_FILL; // remote columns per thread in flight in the cache fill
#ifndef AVS_RES_STREAM_DB
#define AVS_RES_STREAM_DB 0
#endif
#ifndef AVS_RES_STREAM
#define AVS_RES_STREAM 2
#endif
static constexpr int kResStream = AVS_RES_STREAM; // streamed quads per batch (AVS_RES_STREAM_DB: the next batch in flight while this one is multiplied --
                                                  // measured on the 4-way partition: 2 / 4 per batch, with and without: 73.8-76.2 us, all within noise)
static constexpr int kResUpd = AVS_RES_UPD; // rows per thread in flight in the vector update
                                                            // (update 10.3 -> 8.5 us, SpMV 12.1 -> 13.0 us: the live registers push matrix quads to scratch), off
static constexpr int kResTimers = 8;   // phase time stamps per iteration (AVS_CG_RESIDENT_TIMERS=n)
static constexpr int kResGens = 4;     // generations of the broadcast slots (a ring: re-armed two iterations ahead)

template <typename T> struct ResidentArgs {
    // the local system (row pointers of the packed CSR; the words come re-encoded, see rwords)
    const int32_t *row_ptr;
    const double *table;                  // (float system: float values, staged as T)
    int table_size;
    int n;     // own rows
    int G;     // workgroups (= CUs used)
    // lane plan
    const int32_t *lane_row0;
    const uint32_t *lane_meta;            // register rows (3 bits) | streamed rows (bits 3..9) | words of a long row left in memory (bits 10..31)
    const int32_t *wg_lane0, *wg_row0;    // G + 1 entries each
    // workgroup-local re-encoding of the words (k_resident_remap): code << lc_bits | local column; local column < rows of the
    // workgroup = one of its own rows (LDS slice of u), >= : slot of the workgroup's remote-column cache behind the slice
    const uint32_t *rwords;
    // STREAMED rows (a slab larger than the register files: the 4-way partition): after its register rows a lane owns `m` more
    // consecutive rows (lane_meta bits 3..9) whose quads stay in memory -- same 5 x 25-bit quads, a row = whole quads, bit 127 = the
    // row's last quad -- laid out per wave lane-interleaved (quad j of lane l at swords[16 B x (wave_soff[wave] + 64 j + l)]: one
    // 1-KiB run per wave load), padded to the wave's longest lane with quads of zero words
    const uint32_t *swords;
    const int32_t *wave_soff;             // G x 16 + 1, in quads
    int lc_bits;
    int max_quads;                        // quads a lane uses (kResQuads; tests lower it to send ordinary rows down the long-row path)
    const int32_t *rem_list;              // G x rem_stride: source of every remote slot (< n: global u, >= n: the halo area)
    int rem_stride;
    const int32_t *rem_count;             // G
    // vectors
    T *x, *r, *p, *s, *u, *w;
    const uint16_t *dcode;                // diagonal's value code per row; invtab[code] = 1 / table[code]
    const T *invtab;
    // synchronisation (device memory, agent scope)
    unsigned *bar_count;                  // [0]: pushing workgroups that have stored their boundary entries (the last raises the halo flags)
    unsigned long long *bar_flags;        // G: update phases workgroup g has completed (its u is in memory)
    const unsigned *dep_mask;             // G x 32: the workgroups whose u entries workgroup b reads
    int n_push_wgs;                       // workgroups with boundary entries to push
    double *slots;                        // G x 4 partial sums, sentinel-armed (the value is its own arrival flag)
    double *bcast;                        // kResGens x 4: (alpha, beta, rho, done), sentinel-armed ring
    PcgScalars *sc;
    int max_iters;
    long long timeout_ticks;
    // other ranks (direct transport); dd == nullptr: a single-GPU solve
    const DistDev *dd;
    unsigned long long *epoch;            // rounds completed on this comm block
    const uint8_t *wg_halo;               // per workgroup: reads halo columns
    const int32_t *push_seg;              // npeers x (G + 1): segments of send_idx per workgroup
    long long *timers;                    // optional: max_timed x kResTimers wall-clock stamps of workgroup 0
    int max_timed;
    int coherent_fill;                    // 1: the remote columns are read with agent / system scope loads and L2 is NOT invalidated (see phase B)
    long long *wg_times;                  // optional: G x 4 stamps of every workgroup in iteration 20 (start, update done, fill done, SpMV done)
    // LOCAL VALUE TABLES (the LT kernels, AVS_OPTION_RESIDENT_LOCAL_TABLES; appended: the offsets above are those of every other kernel):
    // a word's code indexes the table of the GROUP its row belongs to -- the whole workgroup (ltab_gpw = 1) or the wave that sums the
    // row (16) --, the distinct value bit patterns of the group's rows in ascending order, entry 0 = +0 (what the padding words
    // multiply with: table_size is 0 there).  `table` then holds the groups' tables back to back, and `invtab` ONE INVERSE
    // PER ROW (the launch-per-phase loops' k_inv_diag<T> array: no LDS at all; dcode is not read)
    const int32_t *ltab_cnt;              // G x ltab_gpw: entries of every group's table
    const int32_t *ltab_off;              // ... and where it starts in `table` (G x ltab_gpw + 1)
    int ltab_gpw;
};

// Loop-body reads of the kernel arguments go through these: one scalar load from the kernarg segment AT THE USE.  Left to itself the
// compiler loads all ~40 fields of ResidentArgs at entry, keeps the ~25 the loop touches live across it, runs out of SGPRs and spills
// them to VGPR lanes: 817 v_readlane restores in a 4,000-instruction iteration (20 % of the VALU issue slots of a VALU-bound loop).
// (the struct is the kernel's only parameter: it sits at offset 0 of the kernarg segment; the macros name the kernel's vector type T)
template <int OFF> __device__ __forceinline__ unsigned long long res_karg64()
{
    unsigned long long v;
    asm volatile("s_load_dwordx2 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(__builtin_amdgcn_kernarg_segment_ptr()), "n"(OFF));
    return v;
}
template <int OFF> __device__ __forceinline__ unsigned res_karg32()
{
    unsigned v;
    asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(__builtin_amdgcn_kernarg_segment_ptr()), "n"(OFF));
    return v;
}
#define RES_P(f) (reinterpret_cast<decltype(ResidentArgs<T>::f)>(res_karg64<(int)offsetof(ResidentArgs<T>, f)>()))
#define RES_I(f) ((int)res_karg32<(int)offsetof(ResidentArgs<T>, f)>())
// The same pointer, typed as GLOBAL memory.  The value comes out of an asm statement, so the compiler only knows a generic pointer and
// emits flat_load / flat_store -- which tick the LDS counter (lgkmcnt) as well as vmcnt: every LDS wait then also waits for the
// outstanding global loads, and nothing can be kept in flight across LDS work (the streamed quads, the update's x / w / s loads).
template <class T> using res_gptr = T __attribute__((address_space(1))) *;
#define RES_G(f) (reinterpret_cast<res_gptr<std::remove_pointer_t<decltype(ResidentArgs<T>::f)>>>(res_karg64<(int)offsetof(ResidentArgs<T>, f)>()))

__device__ __forceinline__ bool res_spin_u64(const unsigned long long *f, unsigned long long want, long long timeout)
{
    if (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= want) return true;
    const long long t0 = wall_clock64();
    while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
        if (wall_clock64() - t0 > timeout) return false;
        __builtin_amdgcn_s_sleep(1);
    }
    return true;
}
// 16-B write-through store at agent scope (global_store_dwordx4 ... sc1): what two agent-scope atomic double stores (four float ones)
// would do, in one fabric write.  The caller orders it with wait_own_stores() (s_waitcnt vmcnt(0)) like every other write-through store here.
template <typename V> __device__ __forceinline__ void res_store_wt16(void *p, V v)
{
    static_assert(sizeof(V) == 16, "one 16-B store");
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}
// the same at system scope (sc0 sc1): boundary entries into a peer's halo area
__device__ __forceinline__ void res_store_sys16(double *p, d2_t v)
{
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(p), "v"(v) : "memory");
}
// a sentinel-armed slot: spin until it holds a value (false: timed out)
__device__ __forceinline__ bool res_take_slot(const double *slot, long long timeout, double *out)
{
    const unsigned long long *src = reinterpret_cast<const unsigned long long *>(slot);
    unsigned long long v = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v == kSentinel) {
        const long long t0 = wall_clock64();
        while ((v = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == kSentinel) {
            if (wall_clock64() - t0 > timeout) { *out = 0.; return false; }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    *out = __longlong_as_double((long long)v);
    return true;
}

// three sums at once over the 1024 threads: one LDS round (fixed order: lanes by shuffle tree, then the 16 waves ascending);
// valid in thread 0
__device__ __forceinline__ void res_block_fold3(double &v0, double &v1, double &v2, double *lds48)
{
    const double a0 = wave_sum(v0), a1 = wave_sum(v1), a2 = wave_sum(v2);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        lds48[w] = a0;
        lds48[16 + w] = a1;
        lds48[32 + w] = a2;
    }
    __syncthreads();
    double t0 = 0., t1 = 0., t2 = 0.;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < kResThreads / 64; ++w) {
            t0 += lds48[w];
            t1 += lds48[16 + w];
            t2 += lds48[32 + w];
        }
    }
    v0 = t0; v1 = t1; v2 = t2;
}

// Plan kernel, once per matrix: workgroup b re-encodes the words of ITS rows with workgroup-local columns.  Columns outside its row
// range get slots of a remote cache, numbered in ASCENDING column order (a bitmap of all local columns in LDS: pass 1 sets the bits,
// pass 2 counts them per 512-column block, pass 3 rewrites the words -- the slot of a column is the number of set bits below it), so
// the per-iteration fill of the cache reads ascending addresses (runs of neighbouring entries coalesce; a hash order cost 10 us
// per iteration on the workgroups that read 8 k halo entries) and the numbering is deterministic.
static constexpr int kRemapBlock = 16; // bitmap words per prefix block
static constexpr int kRemapChunk = 1 << 20; // columns per bitmap pass (128 KiB of LDS + 8 KiB of block prefixes): larger slabs take several passes
// PLAIN (local value tables): the columns come from the plain CSR (`cols`; no packed words needed) and the code part is left 0 for
// k_resident_local_tables to fill in.
template <bool PLAIN>
__global__ __launch_bounds__(kResThreads) void k_resident_remap(const uint32_t *__restrict__ packed, const int32_t *__restrict__ cols,
                                                                const int32_t *__restrict__ row_ptr, int col_bits,
                                                                int lc_bits, const int32_t *__restrict__ wg_row0, int rem_cap, int n_ext,
                                                                uint32_t *__restrict__ rwords, int32_t *__restrict__ rem_list,
                                                                int32_t *__restrict__ rem_count, int *__restrict__ fail, int n_own,
                                                                unsigned *__restrict__ dep_mask, int chunk)
{
    extern __shared__ unsigned bm[]; // bitmap[nw], prefix[nb + 1] of ONE chunk of columns
    __shared__ unsigned deps[32];    // bit g: a remote column of this workgroup belongs to workgroup g (G <= 1024)
    const int b = blockIdx.x, tid = threadIdx.x;
    const int r0 = wg_row0[b], r1 = wg_row0[b + 1];
    const int k0 = row_ptr[r0], k1 = row_ptr[r1];
    const unsigned cmask = PLAIN ? 0u : (1u << col_bits) - 1u;
    const int wrows = r1 - r0;
    auto col_of = [&](int k, uint32_t *code) { // column of word k, its value code already at the local word's position
        if (PLAIN) { *code = 0u; return (int)cols[k]; }
        const uint32_t wd = packed[k];
        *code = (wd >> col_bits) << lc_bits;
        return (int)(wd & cmask);
    };
    if (tid < 32) deps[tid] = 0u;
    int base = 0; // remote slots handed out by the chunks below this one (ascending columns overall)
    for (int c0 = 0; c0 < n_ext; c0 += chunk) {
        const int c1 = (c0 + chunk < n_ext) ? c0 + chunk : n_ext;
        const int nw = (c1 - c0 + 31) >> 5, nb = (nw + kRemapBlock - 1) / kRemapBlock;
        unsigned *prefix = bm + nb * kRemapBlock;
        for (int i = tid; i < nb * kRemapBlock; i += kResThreads) bm[i] = 0u;
        __syncthreads();
        for (int k = k0 + tid; k < k1; k += kResThreads) {
            uint32_t code;
            const int col = col_of(k, &code);
            if ((col < r0 || col >= r1) && col >= c0 && col < c1) atomicOr(&bm[(col - c0) >> 5], 1u << ((col - c0) & 31));
        }
        __syncthreads();
        for (int i = tid; i < nb; i += kResThreads) {
            unsigned c = 0u;
#pragma unroll
            for (int w = 0; w < kRemapBlock; ++w) c += (unsigned)__popc(bm[i * kRemapBlock + w]);
            prefix[i + 1] = c;
        }
        __syncthreads();
        if (tid == 0) { // exclusive scan over a few thousand block counts
            unsigned run = 0u;
            prefix[0] = 0u;
            for (int i = 1; i <= nb; ++i) {
                run += prefix[i];
                prefix[i] = run;
            }
        }
        __syncthreads();
        const int total = (int)prefix[nb];
        auto slot_of = [&](int col) { // (col relative to c0)
            const int w = col >> 5, blk = w / kRemapBlock;
            unsigned sl = prefix[blk];
            for (int j = blk * kRemapBlock; j < w; ++j) sl += (unsigned)__popc(bm[j]);
            return (int)(sl + (unsigned)__popc(bm[w] & ((1u << (col & 31)) - 1u)));
        };
        // the list of sources, ascending: every set bit
        if (base + total <= rem_cap)
            for (int w = tid; w < nw; w += kResThreads) {
                unsigned bits = bm[w];
                if (!bits) continue;
                int sl = base + slot_of(w << 5);
                while (bits) {
                    const int bit = __ffs((int)bits) - 1;
                    const int col = c0 + (w << 5) + bit;
                    rem_list[(size_t)b * rem_cap + sl++] = col;
                    if (col < n_own) { // the workgroup that owns (writes) this entry of u: binary search in the row boundaries
                        int lo = 0, hi = (int)gridDim.x;
                        while (hi - lo > 1) {
                            const int mid = (lo + hi) >> 1;
                            if (wg_row0[mid] <= col) lo = mid;
                            else hi = mid;
                        }
                        atomicOr(&deps[lo >> 5], 1u << (lo & 31));
                    }
                    bits &= bits - 1u;
                }
            }
        for (int k = k0 + tid; k < k1; k += kResThreads) {
            uint32_t code;
            const int col = col_of(k, &code);
            if ((col < r0 || col >= r1) && col >= c0 && col < c1) rwords[k] = code | (uint32_t)(wrows + base + slot_of(col - c0));
        }
        base += total;
        __syncthreads(); // the bitmap is cleared for the next chunk
    }
    if (tid == 0) {
        rem_count[b] = (int32_t)base;
        if (base > rem_cap) atomicExch(fail, 1);
    }
    if (tid < 32) dep_mask[(size_t)b * 32 + tid] = deps[tid];
    for (int k = k0 + tid; k < k1; k += kResThreads) { // the workgroup's own rows (and anything past the local columns: never read)
        uint32_t code;
        const int col = col_of(k, &code);
        if (col >= r0 && col < r1) rwords[k] = code | (uint32_t)(col - r0);
        else if (col >= n_ext) rwords[k] = code;
    }
}

// Plan kernel of the local value tables, after k_resident_remap<true>: workgroup b collects, group by group (its whole row range, or
// the rows of each of its 16 waves: tg_row0), the distinct BIT PATTERNS of the group's values -- an LDS hash set, so what it holds does
// not depend on the order of arrival --, sorts them ascending as unsigned 64-bit integers (bitonic, in place: the empty slots, all
// ones, end up last; +0 is always a member and therefore entry 0), writes the table and gives every word of the group its code by
// binary search.  Deterministic: the same matrix and split give the same tables and words in every context.
// ltab_cnt[group] > tcap: the group has more distinct values than a table holds (its words are left without codes).
static constexpr unsigned long long kLtEmpty = ~0ull; // (a NaN: never a matrix value -- one that is counts as an overflow)
__global__ __launch_bounds__(kResThreads) void k_resident_local_tables(const double *__restrict__ val, const int32_t *__restrict__ row_ptr,
                                                                       const int32_t *__restrict__ tg_row0, int gpw, int tcap, int lc_bits,
                                                                       uint32_t *__restrict__ rwords, double *__restrict__ ltab,
                                                                       int32_t *__restrict__ ltab_cnt)
{
    extern __shared__ unsigned long long hs[]; // 2 * tcap slots (tcap >= 1024: the count may pass tcap by one insertion per thread)
    __shared__ int cnt;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int slots = 2 * tcap;
    const unsigned hmask = (unsigned)slots - 1u, cmask = (1u << lc_bits) - 1u;
    for (int g = 0; g < gpw; ++g) {
        const int grp = b * gpw + g;
        const int k0 = row_ptr[tg_row0[grp]], k1 = row_ptr[tg_row0[grp + 1]];
        for (int i = tid; i < slots; i += kResThreads) hs[i] = kLtEmpty;
        if (tid == 0) { hs[0] = 0ull; cnt = 1; } // +0 hashes to slot 0
        __syncthreads();
        for (int k = k0 + tid; k < k1; k += kResThreads) {
            if (*(volatile int *)&cnt > tcap) break; // overflow: reported below
            const unsigned long long bits = (unsigned long long)__double_as_longlong(val[k]);
            if (bits == kLtEmpty) { atomicAdd(&cnt, slots); break; }
            unsigned h = (unsigned)((bits * 0x9E3779B97F4A7C15ull) >> 40) & hmask;
            for (int probe = 0; probe < slots; ++probe) {
                const unsigned long long old = atomicCAS(&hs[h], kLtEmpty, bits);
                if (old == kLtEmpty) { atomicAdd(&cnt, 1); break; }
                if (old == bits) break;
                h = (h + 1u) & hmask;
            }
        }
        __syncthreads();
        const int nv = cnt;
        if (nv <= tcap) {
            for (int k = 2; k <= slots; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int i = tid; i < slots; i += kResThreads) {
                        const int o = i ^ j;
                        if (o > i) {
                            const unsigned long long x = hs[i], y = hs[o];
                            if ((x > y) == ((i & k) == 0)) { hs[i] = y; hs[o] = x; }
                        }
                    }
                    __syncthreads();
                }
            for (int i = tid; i < nv; i += kResThreads) ltab[(size_t)grp * tcap + i] = __longlong_as_double((long long)hs[i]);
            for (int k = k0 + tid; k < k1; k += kResThreads) {
                const unsigned long long bits = (unsigned long long)__double_as_longlong(val[k]);
                int lo = 0, hi = nv - 1; // hs[lo] <= bits <= hs[hi]
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (hs[mid] < bits) lo = mid + 1;
                    else hi = mid;
                }
                rwords[k] = (rwords[k] & cmask) | ((uint32_t)lo << lc_bits);
            }
        }
        if (tid == 0) ltab_cnt[grp] = nv;
        __syncthreads(); // the set is cleared for the next group
    }
}
// ... and of the accepted plan: the tables, tcap entries apart while their sizes were not known, back to back (block = group)
__global__ __launch_bounds__(256) void k_resident_pack_tables(const double *__restrict__ src, int tcap, const int32_t *__restrict__ off,
                                                              double *__restrict__ dst)
{
    const int grp = blockIdx.x, o = off[grp], c = off[grp + 1] - o;
    for (int i = threadIdx.x; i < c; i += 256) dst[(size_t)o + i] = src[(size_t)grp * tcap + i];
}

// Plan kernel for STREAMED rows: thread = lane; packs the re-encoded words of the lane's streamed rows into quads (five 25-bit words, a
// row = whole quads, bit 127 of its last one set) in the wave's lane-interleaved stream (see ResidentArgs::swords), padded to the wave's
// longest lane with quads of zero words.
__global__ __launch_bounds__(kResThreads) void k_resident_stream_layout(const int32_t *__restrict__ row_ptr, const uint32_t *__restrict__ rwords,
                                                                        const int32_t *__restrict__ lane_row0, const uint32_t *__restrict__ lane_meta,
                                                                        const int32_t *__restrict__ wg_lane0, const int32_t *__restrict__ wave_soff,
                                                                        uint32_t padword, u4_t *__restrict__ squads)
{
    const int b = blockIdx.x, tid = threadIdx.x, wv = b * (kResThreads / 64) + (tid >> 6);
    const int off0 = wave_soff[wv], wcnt = (wave_soff[wv + 1] - off0) >> 6;
    u4_t *dst = squads + off0 + (tid & 63);
    const int lane = wg_lane0[b] + tid;
    auto pack = [&](const unsigned long long *wv5, bool last) {
        const unsigned long long lo = wv5[0] | (wv5[1] << 25) | (wv5[2] << 50);
        unsigned long long hi = (wv5[2] >> 14) | (wv5[3] << 11) | (wv5[4] << 36);
        if (last) hi |= 1ull << 63;
        return u4_t{(unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32)};
    };
    int j = 0;
    if (lane < wg_lane0[b + 1]) {
        const uint32_t meta = lane_meta[lane];
        const int m = (int)((meta >> kLaneStreamedShift) & kLaneStreamedMask);
        const int r = lane_row0[lane] + (int)(meta & kLaneRowsMask);
        for (int rr = r; rr < r + m; ++rr) {
            const int ks = row_ptr[rr], ke = row_ptr[rr + 1];
            for (int k = ks; k < ke && j < wcnt; k += kResQuadWords, ++j) {
                unsigned long long w5[kResQuadWords];
                for (int t = 0; t < kResQuadWords; ++t) w5[t] = k + t < ke ? rwords[k + t] : padword;
                dst[(size_t)64 * (size_t)j] = pack(w5, k + kResQuadWords >= ke);
            }
        }
    }
    const unsigned long long p5[kResQuadWords] = {padword, padword, padword, padword, padword};
    for (; j < wcnt; ++j) dst[(size_t)64 * (size_t)j] = pack(p5, false);
}

// NG: how many of the row-local vectors (s, then p, then r) stay in global memory (owner-only accesses) instead of LDS -- what is
// left of the LDS then holds a larger remote-column cache (workgroups in coarse regions read 2-3x as many remote columns as rows).
// Matrix words: 25 bits (value code | local column), five per 128-bit register quad, 15 quads per lane (60 VGPRs).  A row takes
// ceil(len / 5) consecutive quads of one lane, padded with words that address a zero of the dictionary, so rows end at quad
// boundaries: the inner loop is decode, two LDS reads and one FMA per word, and one end-of-row test per quad.  (Measured on the
// 8-way partition of the 512^3 system, tools/probes/rowlen_local.py: rows of 2 / 12 / 15 / 17 / 18 / 20 / 26 words make up 97 %;
// quads + <= 6 rows per lane need 0.89-0.92 of the chip's 262,144 lanes; slots of 15 or 18 words would need 1.06.)
// LT: local value tables (ResidentArgs::ltab_cnt): every wave reads the table of its group, the inverse diagonal comes per row.
template <int NG, bool STREAM, typename T, bool LT = false>
__global__ __launch_bounds__(kResThreads) void k_cg_resident(ResidentArgs<T> a)
{
    extern __shared__ __attribute__((aligned(16))) double rlds[];
    // u: the workgroup's slice, then its remote-column cache (one index space: a word's local column addresses both)
    // (the split is per workgroup -- its own row and remote-column counts: workgroups of coarse regions have few rows and many remote
    // columns, those of fine regions the opposite, and the sum is what has to fit)
    // (even counts of T: the doubles behind the tables stay 8-B aligned)
    const int wrows_al = (a.wg_row0[blockIdx.x + 1] - a.wg_row0[blockIdx.x] + 1) & ~1, nrem_al = (a.rem_count[blockIdx.x] + 1) & ~1;
    T *u_l = reinterpret_cast<T *>(rlds);
    T *r_l = u_l + wrows_al + nrem_al;
    T *p_l = r_l + (NG < 3 ? wrows_al : 0);
    T *s_l = p_l + (NG < 2 ? wrows_al : 0);
    T *tbl = s_l + (NG < 1 ? wrows_al : 0); // table_size values + one zero (what the padding words multiply with)
    T *itab = tbl + a.table_size + 1;          // table_size + 1 inverted values
    int lt_off = 0, lt_total = 0;              // LT: the wave's table inside the workgroup's (in entries), all of them (even)
    if constexpr (LT) {
        const int gpw = a.ltab_gpw, myg = (int)((threadIdx.x >> 6) * (unsigned)gpw) >> 4;
        for (int g = 0; g < gpw; ++g) {
            const int c = a.ltab_cnt[blockIdx.x * gpw + g];
            if (g < myg) lt_off += c;
            lt_total += c;
        }
        lt_off = __builtin_amdgcn_readfirstlane(lt_off);
        lt_total = (lt_total + 1) & ~1;
    }
    double *fold = reinterpret_cast<double *>(LT ? tbl + lt_total : itab + a.table_size + 1); // 3 x 16 wave sums
    double *bc = fold + 48;                                              // 4 rank sums + 4 broadcast scalars
    __shared__ int sh_fail;
    __shared__ double rank_all[kMaxRanks * 4];
    const int tid = threadIdx.x, b = blockIdx.x, G = a.G;
    const DistDev *dd = a.dd;
    const long long timeout = a.timeout_ticks;
    const int wrow0 = a.wg_row0[b], wrows = a.wg_row0[b + 1] - wrow0;
    const int lane = a.wg_lane0[b] + tid;
    const bool have = lane < a.wg_lane0[b + 1];
    int row0_c = 0, nrows = 0, tail = 0;
    if (have) {
        row0_c = a.lane_row0[lane];
        const uint32_t meta = a.lane_meta[lane];
        nrows = (int)(meta & kLaneRowsMask);
        tail = (int)(meta >> kLaneTailShift);
    }
    // ---- one-time loads: matrix words -> registers, vectors -> LDS, tables -> LDS -------------------------------------------
    u4_t m[kResQuads];
    unsigned endmask = 0u; // bit q: quad q holds the last words of a row
    int nquads = 0;        // quads of the lane that hold words
    const unsigned padword = (unsigned)a.table_size << a.lc_bits; // code = table_size (the zero), column 0
    {
        const int row0 = row0_c;
        int rcur = row0, off = 0; // row being laid out, words of it already placed
        int len = (have && nrows > 0) ? a.row_ptr[row0 + 1] - a.row_ptr[row0] : 0;
#pragma unroll
        for (int q = 0; q < kResQuads; ++q) {
            int cnt = 0, src = 0;
            if (rcur < row0 + nrows && q < a.max_quads) {
                cnt = len - off < kResQuadWords ? len - off : kResQuadWords;
                src = a.row_ptr[rcur] + off;
                nquads = q + 1;
                off += kResQuadWords;
                if (off >= len && tail == 0) { // the row is complete (a lane with a tail closes its single row after the tail)
                    endmask |= 1u << q;
                    ++rcur;
                    off = 0;
                    len = rcur < row0 + nrows ? a.row_ptr[rcur + 1] - a.row_ptr[rcur] : 0;
                }
            }
            unsigned long long wv[kResQuadWords];
#pragma unroll
            for (int t = 0; t < kResQuadWords; ++t) wv[t] = t < cnt ? a.rwords[src + t] : padword;
            const unsigned long long lo = wv[0] | (wv[1] << 25) | (wv[2] << 50);         // five 25-bit words -> 125 bits
            const unsigned long long hi = (wv[2] >> 14) | (wv[3] << 11) | (wv[4] << 36);
            m[q] = u4_t{(unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32)};
        }
    }
    // quads the WAVE has to walk: the longest lane's (a scalar loop bound: shorter lanes multiply their padding words by the zero)
    int wave_nq = nquads;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(wave_nq, o, 64);
        wave_nq = other > wave_nq ? other : wave_nq;
    }
    wave_nq = __builtin_amdgcn_readfirstlane(wave_nq);
    for (int i = tid; i < wrows; i += kResThreads) {
        u_l[i] = a.u[wrow0 + i];
        if (NG < 3) r_l[i] = a.r[wrow0 + i];
        if (NG < 2) p_l[i] = a.p[wrow0 + i];
        if (NG < 1) s_l[i] = a.s[wrow0 + i];
    }
    if constexpr (LT) { // the groups' tables, back to back (entry 0 of each: the zero)
        int off = 0;
        for (int g = 0; g < a.ltab_gpw; ++g) {
            const int grp = b * a.ltab_gpw + g, c = a.ltab_cnt[grp];
            const double *src = a.table + a.ltab_off[grp];
            for (int i = tid; i < c; i += kResThreads) tbl[off + i] = (T)src[i];
            off += c;
        }
    } else
    for (int i = tid; i <= a.table_size; i += kResThreads) {
        tbl[i] = i < a.table_size ? (T)a.table[i] : (T)0;
        itab[i] = a.invtab[i];
    }
    const T *const tblw = LT ? tbl + lt_off : tbl; // the table this wave's words index
    if (tid == 0) sh_fail = 0;
    __syncthreads();
    const unsigned cmask = (1u << a.lc_bits) - 1u;
    const int cbits = a.lc_bits;
    const int nrem = a.rem_count[b];
    const int32_t *rem = a.rem_list + (size_t)b * a.rem_stride;
    const bool mydep = tid < G && tid != b && ((a.dep_mask[(size_t)b * 32 + (tid >> 5)] >> (tid & 31)) & 1u) != 0u; // producer of this workgroup
    bool pushes = false;
    if (dd)
        for (int i = 0; i < dd->npeers; ++i) pushes = pushes || a.push_seg[i * (G + 1) + b + 1] > a.push_seg[i * (G + 1) + b];
    const unsigned long long E0 = dd ? *a.epoch : 0ull; // every workgroup reads the same value: it is only written at the very end
    const double *halo = dd ? dd->my_halo : nullptr;
    double alpha = a.sc->alpha, beta = a.sc->beta;
    int done = a.sc->done, iter = a.sc->iter;
    double rho = a.sc->rho;
    const double threshold = a.sc->threshold;
    const int max_iters = a.max_iters, max_timed = a.max_timed;
    double alpha_pend = 0.;
    bool x_pending = false;
    const bool coherent = a.coherent_fill != 0;
    const int tsize = a.table_size;
    const bool timing = a.timers && b == 0 && tid == 0, stamps = a.wg_times && tid == 0;
    int it = 0;
    for (; it < max_iters && !done; ++it) {
        const bool timed = timing && it < max_timed;
        long long *ts = timed ? RES_P(timers) + (size_t)it * kResTimers : nullptr;
        if (timed) ts[0] = wall_clock64();
        if (stamps && it == 20) RES_P(wg_times)[4 * b + 0] = wall_clock64();
        const unsigned long long E = E0 + (unsigned long long)it + 1ull;
        // (opaque per iteration: otherwise the 64-bit addresses of x, w, s for all six rows -- 36 registers -- are hoisted out of the
        // loop and kept live through the SpMV walk, and the allocator parks the matrix quads in scratch instead)
        int row0 = row0_c;
        asm volatile("" : "+v"(row0));
        // ---- A: vector update of the workgroup's rows (k_sr_update_push's arithmetic), u to global, boundary entries to the peers.
        // Row i of the slice belongs to thread i mod 1024 HERE (not to the lane that sums it in the SpMV): the vectors in LDS do not
        // care, and the ones in global memory (x, w, and the tiers) are read and written as whole 512-B runs per wave instead of
        // 8 B every ~32 B (the lane-owned order cost the L1 four times the tag look-ups: the update was 11 us of a 40 us iteration) ----
        // x is touched every SECOND iteration: the update that computes p_new still holds p_old, which is all the skipped
        // x += alpha_prev p_old needs (16 of the 56-82 B per row of this phase, every other time)
        const bool skip_x = (it & 1) == 0;
        T ru = 0, rr = 0;
        {
            const T al = (T)alpha, bt = (T)beta, al_pend = (T)alpha_pend; // (float: the scalars are floats held in doubles)
            const res_gptr<T> gx = RES_G(x) + wrow0, gp = NG >= 2 ? RES_G(p) + wrow0 : nullptr, gr = NG >= 3 ? RES_G(r) + wrow0 : nullptr;
            const res_gptr<T> gs = NG >= 1 ? RES_G(s) + wrow0 : nullptr;
            const res_gptr<const T> gw = RES_G(w) + wrow0;
            const res_gptr<const uint16_t> gd = LT ? nullptr : RES_G(dcode) + wrow0;
            const res_gptr<const T> gi = LT ? RES_G(invtab) + wrow0 : nullptr; // (LT: one inverse per row)
            for (int i0 = tid; i0 < wrows; i0 += kResUpd * kResThreads) {
                T xv[kResUpd], wv[kResUpd], sv[kResUpd], pv[kResUpd], rv[kResUpd];
                unsigned dv[kResUpd];
                T iv[kResUpd];
#pragma unroll
                for (int j = 0; j < kResUpd; ++j) {
                    const int i = i0 + j * kResThreads;
                    if (i < wrows) {
                        if (!skip_x) xv[j] = gx[i];
                        wv[j] = gw[i];
                        if constexpr (LT) iv[j] = gi[i];
                        else dv[j] = gd[i];
                        if (NG >= 1) sv[j] = gs[i];
                        if (NG >= 2) pv[j] = gp[i];
                        if (NG >= 3) rv[j] = gr[i];
                    }
                }
#pragma unroll
                for (int j = 0; j < kResUpd; ++j) {
                    const int i = i0 + j * kResThreads;
                    if (i < wrows) {
                        const T p_old = NG >= 2 ? pv[j] : p_l[i];
                        const T pi = u_l[i] + bt * p_old;
                        const T si = wv[j] + bt * (NG >= 1 ? sv[j] : s_l[i]);
                        if (NG >= 2) gp[i] = pi;
                        else p_l[i] = pi;
                        if (NG >= 1) gs[i] = si;
                        else s_l[i] = si;
                        if (!skip_x) gx[i] = (xv[j] + al_pend * p_old) + al * pi; // = the two sequential updates, bit for bit
                        const T ri = (NG >= 3 ? rv[j] : r_l[i]) - al * si;
                        if (NG >= 3) gr[i] = ri;
                        else r_l[i] = ri;
                        T ui;
                        if constexpr (LT) ui = iv[j] * ri;
                        else ui = itab[dv[j]] * ri;
                        u_l[i] = ui;
                        ru += ri * ui;
                        rr += ri * ri;
                    }
                }
            }
        }
        x_pending = skip_x;
        if (skip_x) alpha_pend = alpha;
        __syncthreads(); // the workgroup's u is complete in LDS
        // u to global for the other workgroups: write-through (other XCDs read it), coalesced, 16 B per lane where the slice allows
        // (8-B sc1 stores cost 2.7x per byte, MI355X_MICROARCH.md); K entries per store, the unaligned head and tail one entry per thread.
        // Every store stays inside the workgroup's rows: the head is clamped to them (float: a workgroup of 1-2 rows can start 1-3 entries
        // before a 16-B boundary -- small systems, one-row lanes), so groups >= 0 and head + K groups <= wrows
        {
            constexpr int K = 16 / (int)sizeof(T);
            T *const gu = RES_P(u);
            const int align = (K - (wrow0 & (K - 1))) & (K - 1); // entries before the first 16-B boundary
            const int head = K == 2 ? ((wrow0 & 1) && wrows > 0 ? 1 : 0) : (align < wrows ? align : wrows);
            if (K == 2) { // (fp64: at most one entry each side, written out as before)
                if (tid == 0 && head) __hip_atomic_store(gu + wrow0, u_l[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else if (tid < head)
                __hip_atomic_store(gu + wrow0 + tid, u_l[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int groups = (wrows - head) >> (K == 2 ? 1 : 2);
            for (int i = tid; i < groups; i += kResThreads) {
                typename Vec16<T>::type v; // the unit of the write-through stores of u
#pragma unroll
                for (int k = 0; k < K; ++k) v[k] = u_l[head + K * i + k];
                res_store_wt16(gu + wrow0 + head + K * i, v);
            }
            const int rest = head + K * groups; // first entry of the tail (<= wrows)
            if (K == 2) {
                if (tid == 0 && ((wrows - head) & 1)) __hip_atomic_store(gu + wrow0 + wrows - 1, u_l[wrows - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else if (tid < wrows - rest)
                __hip_atomic_store(gu + wrow0 + rest + tid, u_l[rest + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (dd && dd->npeers) {
            const int32_t *const pseg = RES_P(push_seg);
            for (int i = 0; i < dd->npeers; ++i) {
                const int sa = pseg[i * (G + 1) + b], se = pseg[i * (G + 1) + b + 1];
                double *dst = dd->peer_halo_dst[i] - dd->send_off[i];
                const int32_t *const sidx = dd->send_idx;
                // consecutive entries of the peer's halo area: two per fabric write where the address allows (an 8-B write-through store
                // costs 2.7x per byte, MI355X_MICROARCH.md); the flag that orders them is raised after wait_own_stores()
                const int head = (sa < se && (reinterpret_cast<uintptr_t>(dst + sa) & 15u)) ? 1 : 0;
                if (tid == 0 && head) __hip_atomic_store(dst + sa, (double)u_l[sidx[sa] - wrow0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                const int pairs = (se - sa - head) >> 1;
                for (int q = tid; q < pairs; q += kResThreads) {
                    const int j = sa + head + 2 * q;
                    d2_t v;
                    v.x = (double)u_l[sidx[j] - wrow0]; // (float: widened, exact; the reader narrows it back)
                    v.y = (double)u_l[sidx[j + 1] - wrow0];
                    res_store_sys16(dst + j, v);
                }
                if (tid == 0 && ((se - sa - head) & 1)) __hip_atomic_store(dst + se - 1, (double)u_l[sidx[se - 1] - wrow0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        wait_own_stores(); // u (agent scope) and the peers' entries (system scope) acknowledged before this wave reaches the barrier
        if (timed) ts[1] = wall_clock64();
        if (stamps && it == 20) RES_P(wg_times)[4 * b + 1] = wall_clock64();
        // ---- B: no grid barrier here: a workgroup only needs the u entries of the workgroups it reads from (10-30 of 256: the
        // neighbours in the brick order).  It publishes "my update k is in memory" (one write-through flag, after its stores were
        // acknowledged) and polls the flags of its producers, one per thread.  The reduction at the end of the iteration is the
        // grid-wide synchronisation that keeps iteration k + 1 from overwriting what iteration k still reads.  The workgroups that
        // push boundary entries to other ranks take a ticket; the last one raises this rank's halo flags.  Then drop the stale lines
        // of u from L1 / L2 ----
        __syncthreads();
        if (tid == 0) {
            __hip_atomic_store(RES_P(bar_flags) + b, (unsigned long long)it + 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (dd && pushes) { // (a monotone ticket, zeroed by the host before the launch: no reset to order)
                const unsigned t = __hip_atomic_fetch_add(RES_P(bar_count), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((t + 1u) % (unsigned)RES_I(n_push_wgs) == 0u)
                    for (int i = 0; i < dd->npeers; ++i)
                        if (dd->send_off[i + 1] > dd->send_off[i]) st_sys(dd->peer_hflag_dst[i], E);
            }
        }
        if (mydep && !res_spin_u64(RES_P(bar_flags) + tid, (unsigned long long)it + 1ull, timeout)) sh_fail = 1;
        if (dd && RES_P(wg_halo)[b] && tid >= 960 && tid < 960 + dd->npeers && dd->recv_cnt[tid - 960] > 0)
            if (!wait_flag(&dd->mine->hflag[dd->peer_rank[tid - 960]], E, timeout, RES_P(sc), 1)) sh_fail = 1;
        __syncthreads(); // every producer's u and the peers' halo entries are in memory
        if (!coherent) {
            if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); // buffer_inv sc1: this CU's L1 and the XCD's L2 drop other writers' lines
            __syncthreads();
        }
        if (sh_fail) break; // (block-uniform)
        if (timed) ts[2] = wall_clock64();
        // ---- C: w = A u for the lane's rows.  First the workgroup's remote columns -> LDS, ONE round trip for all of them (plain loads
        // of the global u: this CU's L1 / the XCD's L2 were invalidated behind the barrier; other ranks' entries: the halo area of the
        // comm block, fine-grained memory first touched after the flag); then every gather is an LDS read.
        const res_gptr<const T> fu = RES_G(u);
        const int fn = RES_I(n);
        for (int k0 = tid; k0 < nrem; k0 += kResFill * kResThreads) { // kResFill loads in flight per lane: a halo-reading workgroup fills 8-10 k slots
            T v[kResFill];
#pragma unroll
            for (int j = 0; j < kResFill; ++j) {
                const int k = k0 + j * kResThreads;
                if (k < nrem) {
                    const int src = rem[k];
                    if (!coherent) v[j] = (src < fn) ? fu[src] : (T)halo[src - fn]; // (halo entries: doubles; float: narrowed back, exact)
                    else if (src < fn) v[j] = __hip_atomic_load(fu + src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    else v[j] = (T)__hip_atomic_load(halo + (src - fn), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
#pragma unroll
            for (int j = 0; j < kResFill; ++j) {
                const int k = k0 + j * kResThreads;
                if (k < nrem) u_l[wrows + k] = v[j];
            }
        }
        __syncthreads();
        if (timed) ts[3] = wall_clock64();
        if (stamps && it == 20) RES_P(wg_times)[4 * b + 2] = wall_clock64();
        T wu = 0;
        {
            const res_gptr<T> gw = RES_G(w);
            T acc = 0;
            int rk = 0; // row of the lane being summed
            unsigned em = endmask;
            int wnq = wave_nq;
            asm volatile("" : "+v"(em)); // (loop-invariant: keep the compiler from turning them into 15 masks held in spilled SGPRs)
            asm volatile("" : "+s"(wnq));
#pragma unroll
            for (int q = 0; q < kResQuads; ++q) {
                if (q < wnq) { // (scalar branch)
                    u4_t mm = m[q];
                    // the words are loop-invariant: without this the compiler hoists every decode (code, column, LDS addresses) out of
                    // the iteration loop and spills hundreds of registers
                    asm volatile("" : "+v"(mm));
                    // five 25-bit words at bit offsets 0, 25, 50, 75, 100 of the quad: column = low lc_bits, code = the bits above (bit-field
                    // extracts straight from the shifted dwords: no intermediate 25-bit mask)
                    const unsigned kb = (unsigned)(kResWordBits - cbits);
                    { // words 0, 1 (three groups with scheduling barriers between them: ten reads in flight at once need 20 more
                      // registers than the file has next to the 60 of the matrix, and the allocator then parks the MATRIX in scratch)
                        const unsigned t1 = __builtin_amdgcn_alignbit(mm.y, mm.x, 25);
                        const T v0 = tblw[__builtin_amdgcn_ubfe(mm.x, (unsigned)cbits, kb)], x0 = u_l[mm.x & cmask];
                        const T v1 = tblw[__builtin_amdgcn_ubfe(t1, (unsigned)cbits, kb)], x1 = u_l[t1 & cmask];
                        acc += v0 * x0; // left to right inside the row, multiply then add (no FMA): the oracle's order and rounding, the same
                                        // row sums as the launch-per-phase kernels bit for bit (padding words add +0)
                        acc += v1 * x1;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    { // words 2, 3
                        const unsigned t2 = __builtin_amdgcn_alignbit(mm.z, mm.y, 18);
                        const unsigned t3 = __builtin_amdgcn_alignbit(mm.w, mm.z, 11);
                        const T v2 = tblw[__builtin_amdgcn_ubfe(t2, (unsigned)cbits, kb)], x2 = u_l[t2 & cmask];
                        const T v3 = tblw[__builtin_amdgcn_ubfe(t3, (unsigned)cbits, kb)], x3 = u_l[t3 & cmask];
                        acc += v2 * x2;
                        acc += v3 * x3;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    { // word 4
                        const T v4 = tblw[__builtin_amdgcn_ubfe(mm.w, 4u + (unsigned)cbits, kb)], x4 = u_l[__builtin_amdgcn_ubfe(mm.w, 4u, (unsigned)cbits)];
                        acc += v4 * x4;
                    }
                    if ((em >> q) & 1u) {
                        gw[row0 + rk] = acc;
                        wu += acc * u_l[row0 + rk - wrow0];
                        acc = 0;
                        ++rk;
                    }
                }
                __builtin_amdgcn_sched_barrier(0); // keep the scheduler from hoisting later quads' reads: their live ranges push the matrix to scratch
            }
            if (tail > 0) { // a row of more words than the registers hold (a coarse face ringed by fine ones; a handful per scene)
                const int kt = RES_P(row_ptr)[row0] + RES_I(max_quads) * kResQuadWords;
                const res_gptr<const uint32_t> twords = RES_G(rwords);
                for (int k = kt; k < kt + tail; ++k) {
                    const uint32_t wd = twords[k];
                    acc += tblw[wd >> cbits] * u_l[wd & cmask];
                }
                gw[row0] = acc;
                wu += acc * u_l[row0 - wrow0];
            }
            if (STREAM) { // the lane's streamed rows: the same quads, from memory -- one 1-KiB run per wave load
                const int32_t *const so = RES_P(wave_soff) + b * (kResThreads / 64) + (tid >> 6);
                const int off0 = __builtin_amdgcn_readfirstlane(so[0]);
                const int wcnt = (__builtin_amdgcn_readfirstlane(so[1]) - off0) >> 6; // quads of the wave's longest lane
                const res_gptr<const u4_t> sq = reinterpret_cast<res_gptr<const u4_t>>(RES_G(swords)) + off0 + (tid & 63);
                const unsigned kb = (unsigned)(kResWordBits - cbits);
                const unsigned pw = (unsigned)tsize << cbits; // a word that multiplies the dictionary's zero
                const unsigned long long plo = (unsigned long long)pw | ((unsigned long long)pw << 25) | ((unsigned long long)pw << 50);
                const unsigned long long phi = ((unsigned long long)pw >> 14) | ((unsigned long long)pw << 11) | ((unsigned long long)pw << 36);
                const u4_t padq = u4_t{(unsigned)plo, (unsigned)(plo >> 32), (unsigned)phi, (unsigned)(phi >> 32)};
                int row = row0 + nrows;
                T sacc = 0;
#if AVS_RES_STREAM_DB
                u4_t qn[kResStream]; // the batch in flight while the previous one is multiplied
#pragma unroll
                for (int i = 0; i < kResStream; ++i) qn[i] = (i < wcnt) ? sq[(size_t)64 * (size_t)i] : padq;
#endif
                for (int j0 = 0; j0 < wcnt; j0 += kResStream) {
                    u4_t qv[kResStream];
#if AVS_RES_STREAM_DB
#pragma unroll
                    for (int i = 0; i < kResStream; ++i) qv[i] = qn[i];
#pragma unroll
                    for (int i = 0; i < kResStream; ++i) qn[i] = (j0 + kResStream + i < wcnt) ? sq[(size_t)64 * (size_t)(j0 + kResStream + i)] : padq;
#else
#pragma unroll
                    for (int i = 0; i < kResStream; ++i) qv[i] = (j0 + i < wcnt) ? sq[(size_t)64 * (size_t)(j0 + i)] : padq;
#endif
#pragma unroll
                    for (int i = 0; i < kResStream; ++i) {
                        const u4_t mm = qv[i];
                        const unsigned t1 = __builtin_amdgcn_alignbit(mm.y, mm.x, 25);
                        const unsigned t2 = __builtin_amdgcn_alignbit(mm.z, mm.y, 18);
                        const unsigned t3 = __builtin_amdgcn_alignbit(mm.w, mm.z, 11);
                        const T v0 = tblw[__builtin_amdgcn_ubfe(mm.x, (unsigned)cbits, kb)], x0 = u_l[mm.x & cmask];
                        const T v1 = tblw[__builtin_amdgcn_ubfe(t1, (unsigned)cbits, kb)], x1 = u_l[t1 & cmask];
                        const T v2 = tblw[__builtin_amdgcn_ubfe(t2, (unsigned)cbits, kb)], x2 = u_l[t2 & cmask];
                        const T v3 = tblw[__builtin_amdgcn_ubfe(t3, (unsigned)cbits, kb)], x3 = u_l[t3 & cmask];
                        const T v4 = tblw[__builtin_amdgcn_ubfe(mm.w, 4u + (unsigned)cbits, kb)], x4 = u_l[__builtin_amdgcn_ubfe(mm.w, 4u, (unsigned)cbits)];
                        sacc += v0 * x0;
                        sacc += v1 * x1;
                        sacc += v2 * x2;
                        sacc += v3 * x3;
                        sacc += v4 * x4;
                        if (mm.w >> 31) { // (bit 127) the row's last quad
                            gw[row] = sacc;
                            wu += sacc * u_l[row - wrow0];
                            sacc = 0;
                            ++row;
                        }
                    }
                }
            }
        }
        // ---- D: one reduction of (r.u, |r|^2, w.u): every workgroup drops its three sums into sentinel-armed slots (fire and forget:
        // the value is its own arrival); workgroup 0 takes them in slot order, exchanges with the other ranks, applies the scalar step
        // and publishes it in the broadcast ring everybody polls ----
        double s0 = (double)ru, s1 = (double)rr, s2 = (double)wu; // (across threads, workgroups and ranks: double)
        res_block_fold3(s0, s1, s2, fold);
        if (tid == 0) {
            double *const sl = RES_P(slots) + 4 * b;
            __hip_atomic_store(sl + 0, s0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(sl + 1, s1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(sl + 2, s2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (timed) ts[4] = wall_clock64();
        if (stamps && it == 20) { // every workgroup's own phase stamps of one iteration (imbalance diagnostics)
            RES_P(wg_times)[4 * b + 3] = wall_clock64();
        }
        const int gen = it & (kResGens - 1);
        if (b == 0) {
            double v0 = 0., v1 = 0., v2 = 0.;
            if (tid < G) {
                double *const sl = RES_P(slots) + 4 * tid;
                bool ok = res_take_slot(sl + 0, timeout, &v0);
                ok = res_take_slot(sl + 1, timeout, &v1) && ok;
                ok = res_take_slot(sl + 2, timeout, &v2) && ok;
                if (!ok) sh_fail = 1;
                // re-arm, and wait for the sentinel stores to be acknowledged: the broadcast below releases the workgroups into the next
                // iteration, whose partial sums land in these very slots -- a sentinel still in flight then would overwrite one (a
                // workgroup barrier does not wait for vmcnt)
                for (int k = 0; k < 3; ++k)
                    __hip_atomic_store(reinterpret_cast<unsigned long long *>(sl + k), kSentinel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                wait_own_stores();
            }
            res_block_fold3(v0, v1, v2, fold);
            if (tid == 0) { bc[0] = v0; bc[1] = v1; bc[2] = v2; bc[3] = 0.; }
            __syncthreads();
            if (dd && dd->world > 1) {
                // all-gather of the rank sums through the comm blocks: dist_finalize's sentinel-armed slots (value = its own arrival)
                const int epar = (int)(E & 1ull);
                if (tid < dd->world * 4) {
                    const int q = tid >> 2, k = tid & 3;
                    unsigned long long *dst = reinterpret_cast<unsigned long long *>(dd->all_red_dst[q] + (size_t)epar * kMaxRanks * 4 + k);
                    st_sys(dst, (unsigned long long)__double_as_longlong(bc[k]));
                    unsigned long long *src = reinterpret_cast<unsigned long long *>(&dd->mine->red[epar][q][k]);
                    unsigned long long v = ld_sys(src);
                    if (v == kSentinel) {
                        const long long tw = wall_clock64();
                        while ((v = ld_sys(src)) == kSentinel) {
                            if (wall_clock64() - tw > timeout) {
                                __hip_atomic_store(&RES_P(sc)->fault, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                sh_fail = 1;
                                v = 0ull;
                                break;
                            }
                            __builtin_amdgcn_s_sleep(2);
                        }
                    }
                    rank_all[tid] = __longlong_as_double((long long)v);
                    st_sys(src, kSentinel);
                }
                __syncthreads();
                if (tid == 0)
                    for (int k = 0; k < 3; ++k) {
                        double t = 0.;
                        for (int q = 0; q < dd->world; ++q) t += rank_all[q * 4 + k]; // rank order: identical on every rank
                        bc[k] = t;
                    }
                __syncthreads();
            }
            if (tid == 0) {
                // OP_SR_STEP (float: OP_SR_STEP_F32) on (gamma, |r|^2, delta)
                const double gamma = bc[0], rr_all = bc[1], delta = bc[2];
                const double sums[3] = {gamma, rr_all, delta};
                int nd = sh_fail ? 1 : 0;
                double na = alpha, nb = beta, nrho = rho, nrr = (double)(T)rr_all;
                int niter = iter;
                sr_step_sums<T>(sums, &threshold, nrr, nrho, na, nb, niter, nd);
                // the ring: re-arm the generation two iterations ahead, publish this one
                double *const ring = RES_P(bcast);
                double *ahead = ring + 4 * ((it + 2) & (kResGens - 1)), *me = ring + 4 * gen;
                for (int k = 0; k < 4; ++k)
                    __hip_atomic_store(reinterpret_cast<unsigned long long *>(ahead + k), kSentinel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(me + 0, na, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(me + 1, nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(me + 2, nrho, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(me + 3, (double)(nd * 1048576 + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // done | 1 (never the sentinel)
                if (timed) { // debug record (AVS_CG_RESIDENT_TIMERS): the sums this step was taken from
                    ts[6] = __double_as_longlong(rr_all);
                    ts[7] = __double_as_longlong(delta - (gamma / rho) * gamma / alpha);
                }
                // the host's copy of the state (always written by this one thread: plain stores)
                PcgScalars *const hs = RES_P(sc);
                hs->red[0] = gamma; hs->red[1] = rr_all; hs->red[2] = delta;
                hs->rr = nrr; hs->alpha = na; hs->beta = nb; hs->rho = nrho; hs->iter = niter; hs->done = nd;
                if (sh_fail && !hs->fault) hs->fault = 3;
            }
        }
        // everybody (the publisher included) picks the step up from the ring
        if (tid < 4)
            if (!res_take_slot(RES_P(bcast) + 4 * gen + tid, timeout, &bc[4 + tid])) sh_fail = 1;
        __syncthreads();
        if (sh_fail) break;
        const int nd = (int)bc[7] >> 20;
        if (!nd) {
            alpha = bc[4];
            beta = bc[5];
            rho = bc[6];
            iter += 1;
        }
        done = nd;
        if (timed) ts[5] = wall_clock64();
        __syncthreads(); // bc is rewritten next iteration
    }
    // ---- write the vectors back (a later solve / the host reads them), close the round counter -----------------------------------
    if (x_pending) // the last update skipped x: x += alpha p with the p it left behind
        for (int i = tid; i < wrows; i += kResThreads) a.x[wrow0 + i] += (T)alpha_pend * (NG >= 2 ? a.p[wrow0 + i] : p_l[i]);
    for (int i = tid; i < wrows; i += kResThreads) {
        if (NG < 3) a.r[wrow0 + i] = r_l[i];
        if (NG < 2) a.p[wrow0 + i] = p_l[i];
        if (NG < 1) a.s[wrow0 + i] = s_l[i];
    }
    if (sh_fail && tid == 0) {
        if (!__hip_atomic_load(&a.sc->fault, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_store(&a.sc->fault, 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&a.sc->done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (dd && b == 0 && tid == 0) *a.epoch = E0 + (unsigned long long)it;
}

// ---------------------------------------------------------------------------------------------
// host side: the lane plan (which rows / words every lane of every workgroup keeps), built once per matrix
// ---------------------------------------------------------------------------------------------
struct ResidentPlan {
    DevBuf<int32_t> lane_row0, wg_lane0, wg_row0, push_seg, rem_list, rem_count;
    DevBuf<uint32_t> lane_meta, rwords, swords;
    DevBuf<int32_t> wave_soff;
    // local value tables (AVS_OPTION_RESIDENT_LOCAL_TABLES): the plan of a matrix without one small dictionary
    bool local = false, key_local = false; // this plan uses them; the option it was built (or refused) under
    DevBuf<double> ltab;                  // G x lt_gpw tables, back to back
    DevBuf<int32_t> ltab_cnt, ltab_off, tg_row0; // entries per table, its offset in ltab; row boundaries of the groups (G x lt_gpw + 1)
    int lt_gpw = 1;                       // tables per workgroup: 1, or 16 (one per wave)
    bool streams = false;
    DevBuf<unsigned long long> bar_flags;
    DevBuf<unsigned> dep_mask;
    int n_push_wgs = 0;
    DevBuf<uint8_t> wg_halo;
    DevBuf<unsigned> bar_count;
    DevBuf<double> slots, bcast;
    DevBuf<long long> timers;
    int G = 0, max_timed = 0, lc_bits = 0, ng = 0, max_quads = kResQuads;
    size_t lds = 0;
    bool f32 = false;                     // laid out (LDS split, kernel) for float vectors: only resident_run<float> runs it
    const void *key[4] = {};
    int64_t key_n = -1;
    uint64_t key_epoch = 0;
    bool ok = false, tried = false;
    std::string why;
    // what the plan turned out to be (reported by avs_pcg_csr_plan, include/avs_probe.h: a test names the edge it reached); the counts of
    // a refused plan hold what was known when it stopped
    int64_t n_lanes = 0, streamed_rows = 0, streamed_words = 0;
    int max_lanes = 0, max_rows = 0, long_lanes = 0, longest_tail = 0, max_lane_streamed = 0, max_remote = 0, remap_passes = 0, lt_max = 0;
};

static bool resident_wanted(bool distributed)
{
    (void)distributed;
    return cur_opt().resident != 0; // default for every system that qualifies (plan: 1.5-2 ms per new matrix; AVS_CG_RESIDENT=0 keeps the launch-per-phase loops)
}

// the system is one the ordinary plan takes as far as its dictionary goes: the packed single-dictionary form, <= 1,023 values
static bool resident_single_dictionary(const CsrView &A)
{
    return A.packed && A.codes && !A.tab_ptr && !A.cbase && A.col_bits > 0 && A.table_size <= 1023;
}
// ... or one that AVS_OPTION_RESIDENT_LOCAL_TABLES sends through the plan with local value tables (from the plain CSR)
static bool resident_local_tables_wanted(const CsrView &A)
{
    return cur_opt().resident_local_tables != 0 && !resident_single_dictionary(A) && A.val && A.col;
}

template <typename T, bool LT> static const void *resident_kernel(int ng, bool streams)
{
    // (streamed rows are a template parameter: their code costs the plain kernels 15 more spilled registers otherwise)
    switch (ng) {
    case 0: return streams ? (const void *)k_cg_resident<0, true, T, LT> : (const void *)k_cg_resident<0, false, T, LT>;
    case 1: return streams ? (const void *)k_cg_resident<1, true, T, LT> : (const void *)k_cg_resident<1, false, T, LT>;
    case 2: return streams ? (const void *)k_cg_resident<2, true, T, LT> : (const void *)k_cg_resident<2, false, T, LT>;
    default: return streams ? (const void *)k_cg_resident<3, true, T, LT> : (const void *)k_cg_resident<3, false, T, LT>;
    }
}
template <typename T> static const void *resident_kernel(int ng, bool streams, bool local)
{
    return local ? resident_kernel<T, true>(ng, streams) : resident_kernel<T, false>(ng, streams);
}
static const void *resident_kernel(int ng, bool streams, bool f32, bool local)
{
    return f32 ? resident_kernel<float>(ng, streams, local) : resident_kernel<double>(ng, streams, local);
}

// ---- resident_prepare: the driver of the plan.  The integer planning is avs_resident_plan.cpp (host only); here are its device steps ----
static bool resident_refuse(ResidentPlan *pl, const char *why, int64_t n)
{
    pl->why = why;
    if (cur_opt().resident_verbose > 0) fprintf(stderr, "[avs resident] not used: %s (n = %lld)\n", why, (long long)n);
    return false;
}
// a failed HIP step of the plan: the error is cleared, the caller refuses the plan and the solve keeps the launch-per-phase loop
static bool plan_failed(bool failed)
{
    if (failed) (void)hipGetLastError();
    return failed;
}
struct PlanClock { // (verbose: where the plan's milliseconds go)
    bool verbose;
    timespec t0{}, last{};
    explicit PlanClock(bool v) : verbose(v)
    {
        clock_gettime(CLOCK_MONOTONIC, &t0);
        last = t0;
    }
    static double ms(const timespec &a, const timespec &b) { return (b.tv_sec - a.tv_sec) * 1e3 + (b.tv_nsec - a.tv_nsec) * 1e-6; }
    void stage(const char *what)
    {
        if (!verbose) return;
        timespec t{};
        clock_gettime(CLOCK_MONOTONIC, &t);
        fprintf(stderr, "[avs resident]   plan stage %-28s %.2f ms\n", what, ms(last, t));
        last = t;
    }
    double total() const
    {
        timespec t{};
        clock_gettime(CLOCK_MONOTONIC, &t);
        return ms(t0, t);
    }
};

// One split of the lanes into workgroups and what the device steps worked out for it: shared by the rounds and the accepted-plan work
struct ResidentSplitState {
    ResidentPlan *pl = nullptr;
    const CsrView *A = nullptr;
    const ResidentLanes *lanes = nullptr;
    hipStream_t stream = nullptr;
    bool lt = false, verbose = false;
    int G = 0, cap = 0;                         // workgroups; stride of the per-workgroup source lists
    int64_t n = 0, n_ext = 0, chunk_cols = 0;   // rows, columns, columns per bitmap pass of the re-encoding
    size_t remap_lds = 0;
    ResidentSplit split;
    std::vector<int32_t> rc, tabs, tcnt, tgr;   // per workgroup: remote columns, LDS entries of its tables (even); entries per group; group boundaries
    int lc_bits = 0, code_bits = 1;
    int lt_gpw = 1, lt_cap = 0, lt_max = 0, lt_max_grp = 0;
    std::string lt_why;                         // the quantity of a local-table plan that did not fit
    DevBuf<double> lt_strided;                  // the tables while the plan is being made: lt_cap entries apart
    DevBuf<int> fail;
    ResidentCounts counts() const { return ResidentCounts{split.wr, rc, tabs}; }
};

// Local tables, for the split and the columns just re-encoded: one table per workgroup where its code bits fit the word next to
// the REAL column bits (rows + remote columns of the largest workgroup, not the source lists' stride), else one per wave (the
// rows of the wave's 64 lanes: fewer values, 16 tables whose entries add up to more LDS).  0 ok, 2 declined (lt_why), -1 failure
static int resident_local_tables(ResidentSplitState &s)
{
    const int G = s.G;
    const int64_t L = s.lanes->size();
    const std::vector<int32_t> &wl = s.split.wl;
    const int cols = std::max(2, max_local_columns(s.counts()));
    s.lc_bits = 1;
    while ((1 << s.lc_bits) < cols) ++s.lc_bits;
    for (s.lt_gpw = 1; s.lt_gpw <= 16; s.lt_gpw *= 16) {
        const int gpw = s.lt_gpw;
        s.lt_cap = gpw == 1 ? 4096 : 2048;
        const size_t ngrp = (size_t)G * (size_t)gpw;
        s.tgr.assign(ngrp + 1, (int32_t)s.n);
        for (int b = 0; b < G; ++b)
            for (int g = 0; g < gpw; ++g) { // (a wave's rows: from its first lane's first row to the next wave's)
                const int64_t l = std::min<int64_t>((int64_t)wl[(size_t)b] + 64 * g * (16 / gpw), wl[(size_t)b + 1]);
                s.tgr[(size_t)b * gpw + g] = l < L ? s.lanes->row0[(size_t)l] : (int32_t)s.n;
            }
        s.tcnt.assign(ngrp, 0);
        if (s.lt_strided.alloc(ngrp * (size_t)s.lt_cap) != AVS_OK ||
            hipMemcpyAsync(s.pl->tg_row0.p, s.tgr.data(), s.tgr.size() * 4, hipMemcpyHostToDevice, s.stream) != hipSuccess)
            return -1;
        hipLaunchKernelGGL(k_resident_local_tables, dim3((unsigned)G), dim3(kResThreads), (size_t)2 * s.lt_cap * 8, s.stream, s.A->val, s.A->row_ptr,
                           (const int32_t *)s.pl->tg_row0.p, gpw, s.lt_cap, s.lc_bits, s.pl->rwords.p, s.lt_strided.p, s.pl->ltab_cnt.p);
        if (hipMemcpyAsync(s.tcnt.data(), s.pl->ltab_cnt.p, ngrp * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream) != hipSuccess ||
            hipStreamSynchronize(s.stream) != hipSuccess)
            return -1;
        s.lt_max = 0;
        for (size_t g = 0; g < ngrp; ++g)
            if (s.tcnt[g] > s.lt_max) { s.lt_max = s.tcnt[g]; s.lt_max_grp = (int)g; }
        s.code_bits = 1;
        while ((1 << s.code_bits) < s.lt_max) ++s.code_bits;
        char who[64];
        if (gpw == 1) snprintf(who, sizeof(who), "workgroup %d", s.lt_max_grp);
        else snprintf(who, sizeof(who), "wave %d of workgroup %d", s.lt_max_grp % 16, s.lt_max_grp / 16);
        char msg[256];
        if (s.lt_max > s.lt_cap)
            snprintf(msg, sizeof(msg), "local table of %s has more than %d distinct values", who, s.lt_cap);
        else if (s.code_bits + s.lc_bits > kResWordBits)
            snprintf(msg, sizeof(msg), "local table of %s (%d values) needs %d code bits, %d left by the %d column bits of the %d-bit word", who,
                     s.lt_max, s.code_bits, kResWordBits - s.lc_bits, s.lc_bits, kResWordBits);
        else {
            for (int b = 0; b < G; ++b) {
                int t = 0;
                for (int g = 0; g < gpw; ++g) t += s.tcnt[(size_t)b * gpw + g];
                s.tabs[(size_t)b] = (t + 1) & ~1;
            }
            return 0;
        }
        s.lt_why = msg;
        if (s.verbose) fprintf(stderr, "[avs resident] local tables per %s: %s\n", gpw == 1 ? "workgroup" : "wave", msg);
    }
    return 2;
}

// re-encodes the words for the split in s (the plan kernel) and fetches the remote-column counts; with local tables, builds them too.
// 0 ok, 1 a source list overflowed, 2 the local tables do not fit the word, -1 failure
static int resident_remap(ResidentSplitState &s)
{
    const CsrView &A = *s.A;
    ResidentPlan *pl = s.pl;
    if (s.lt)
        hipLaunchKernelGGL(k_resident_remap<true>, dim3((unsigned)s.G), dim3(kResThreads), s.remap_lds, s.stream, (const uint32_t *)nullptr, A.col,
                           A.row_ptr, 0, s.lc_bits, (const int32_t *)pl->wg_row0.p, s.cap, (int)s.n_ext, pl->rwords.p, pl->rem_list.p,
                           pl->rem_count.p, s.fail.p, (int)s.n, pl->dep_mask.p, (int)s.chunk_cols);
    else
        hipLaunchKernelGGL(k_resident_remap<false>, dim3((unsigned)s.G), dim3(kResThreads), s.remap_lds, s.stream, A.packed, (const int32_t *)nullptr,
                           A.row_ptr, A.col_bits, s.lc_bits, (const int32_t *)pl->wg_row0.p, s.cap, (int)s.n_ext, pl->rwords.p, pl->rem_list.p,
                           pl->rem_count.p, s.fail.p, (int)s.n, pl->dep_mask.p, (int)s.chunk_cols);
    int f = 0;
    if (plan_failed(hipMemcpyAsync(&f, s.fail.p, sizeof(int), hipMemcpyDeviceToHost, s.stream) != hipSuccess ||
                    hipMemcpyAsync(s.rc.data(), pl->rem_count.p, (size_t)s.G * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream) != hipSuccess ||
                    hipStreamSynchronize(s.stream) != hipSuccess))
        return -1;
    if (f) return 1;
    if (!s.lt) return 0;
    const int t = resident_local_tables(s);
    plan_failed(t < 0);
    return t;
}

// the sizes of the split's arrays and of the re-encoding passes, the plan's device buffers, the plan kernels' LDS opt-in
static const char *resident_split_setup(ResidentSplitState &s, int64_t n_cols, double stream_T)
{
    ResidentPlan *pl = s.pl;
    const CsrView &A = *s.A;
    const int G = s.G;
    const int64_t n = s.n, L = s.lanes->size();
    while (!s.lt && (1 << s.code_bits) < A.table_size + 1) ++s.code_bits; // + the zero the padding words address
    if (s.code_bits >= kResWordBits - 8) return "dictionary needs too many bits";
    s.cap = stream_T > 0. ? 32768 : 16384; // (a workgroup with more remote columns than its source list holds does not qualify)
    s.n_ext = n_cols > n ? n_cols : n;
    s.chunk_cols = std::min<int64_t>(s.n_ext, kRemapChunk);
    if (cur_opt().resident_remap_chunk >= 512) // tests: several bitmap passes on a small system
        s.chunk_cols = std::min<int64_t>(s.chunk_cols, (cur_opt().resident_remap_chunk + 511) / 512 * 512);
    pl->remap_passes = (int)((s.n_ext + s.chunk_cols - 1) / s.chunk_cols);
    s.remap_lds = ((size_t)(((s.chunk_cols + 31) / 32 + kRemapBlock - 1) / kRemapBlock) * (kRemapBlock + 1) + 2) * sizeof(unsigned);
    s.split.wl.resize((size_t)G + 1);
    s.split.wr.resize((size_t)G + 1);
    s.rc.resize((size_t)G);
    s.tabs.assign((size_t)G, 0);
    s.split.lane_w.assign((size_t)L, 1.0);
    s.split.cum.assign((size_t)L + 1, 0.);
    s.split.lane_extra.assign((size_t)L, 0.);
    if (plan_failed(pl->wg_row0.alloc((size_t)G + 1) != AVS_OK || pl->rwords.alloc((size_t)A.nnz) != AVS_OK || pl->rem_count.alloc((size_t)G) != AVS_OK ||
                    pl->rem_list.alloc((size_t)G * s.cap) != AVS_OK || s.fail.alloc(1) != AVS_OK || pl->dep_mask.alloc((size_t)G * 32) != AVS_OK || G > 1024 ||
                    hipFuncSetAttribute(s.lt ? (const void *)k_resident_remap<true> : (const void *)k_resident_remap<false>,
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.remap_lds) != hipSuccess ||
                    (s.lt && (pl->ltab_cnt.alloc((size_t)G * 16) != AVS_OK || pl->tg_row0.alloc((size_t)G * 16 + 1) != AVS_OK ||
                            hipFuncSetAttribute((const void *)k_resident_local_tables, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 4096 * 8) != hipSuccess))))
        return "plan allocation failed";
    return nullptr;
}

struct ResidentTier {
    int ng = -1, max_cols = 0; // row-local vectors in global memory (-1: no tier fits); most rows + remote columns of a workgroup
    size_t lds = 0;
    const char *last_reason = "the vector slices + remote columns of a workgroup do not fit the LDS";
};

// Tiers: the fewest row-local vectors in global memory that fit.  Tier 1 (s) is tried with re-balancing first; tiers 2 and 3 (p, r
// too) only when that fails -- larger slabs (streamed rows: the 2- and 4-way partitions) -- since their vector traffic is back in
// the update phase (coalesced since the second pass of round 3, which is what makes them worth it).
// Rounds of a tier: workgroup boundaries by estimated time (split_by_cost), then the words are re-encoded (k_resident_remap) and the
// LDS footprints checked: a workgroup whose slices + remote columns do not fit (the ones that read the halo: up to 10 k remote
// columns) gets its lanes re-weighted and the split is redone -- a few rounds.  Remote columns cost their workgroup a fill (the
// halo-reading workgroups fill 8-10 k and finished 5 us after the median one).  Known only after a first split: round 0 measures
// them, round 1 splits with them spread over the workgroup's lanes.  Per slot, in the units of c_lane / c_row: 0 / 1.1 / 2 / 3 / 4.5
// -> 8-way loop-back (ranks 0 / 3) 33.8 / 35.9, 32.6 / 35.0, 31.6 / 33.0, 30.0 / 32.1, 30.4 / 32.3 us per iteration.
// Returns the refusal of a step that ends the plan, else nullptr with tier->ng >= 0 (s holds the accepted split) or < 0 (none fits).
static const char *resident_split_rounds(ResidentSplitState &s, double stream_T, size_t esz, size_t lds_max, size_t lds_extra, ResidentTier *tier)
{
    const int G = s.G;
    const int64_t L = s.lanes->size();
    const int max_ng_limit = cur_opt().resident_max_global;
    const bool equal_lanes = cur_opt().resident_equal_lanes != 0;
    const double c_rem = cur_opt().resident_remote_cost;
    const double limit = (double)(lds_max - lds_extra) / (double)esz; // entries of the vector type a workgroup may hold
    ResidentSplit &sp = s.split;
    std::vector<int32_t> rc_round0;
    bool round0_done = false;
    for (int max_ng = std::min(1, max_ng_limit); max_ng <= max_ng_limit && tier->ng < 0; ++max_ng) {
        if ((size_t)(4 - max_ng) * (size_t)(s.n / G) * esz > lds_max) continue; // (even the average workgroup's slices would not fit)
        const int t_max = max_ng < 3 ? (max_ng < 0 ? 0 : max_ng) : 3;           // the largest tier allowed here: its footprints steer the split
        std::fill(sp.lane_w.begin(), sp.lane_w.end(), 1.0);
        std::fill(sp.lane_extra.begin(), sp.lane_extra.end(), 0.);
        bool reweighted = false, extras_active = false, extras_off = false;
        for (int round = 0; round < (stream_T > 0. ? 9 : 5) && tier->ng < 0; ++round) { // (large slabs: a lower tier is worth more rounds)
            bool whole = split_by_cost(*s.lanes, G, cur_opt().resident_stream_cost, &sp);
            if (!whole && extras_active && !reweighted) { // the remote-column term alone pushed a workgroup past 1024 lanes: split without it
                std::fill(sp.lane_extra.begin(), sp.lane_extra.end(), 0.);
                extras_active = false;
                extras_off = true;
                whole = split_by_cost(*s.lanes, G, cur_opt().resident_stream_cost, &sp);
            }
            if (!whole || equal_lanes) {
                if (reweighted) break; // (re-weighting pushed a workgroup past 1024 lanes: next tier)
                split_equal_lanes(L, G, &sp.wl);
            }
            sp.max_rows = workgroup_rows(sp.wl, *s.lanes, s.n, &sp.wr);
            s.lc_bits = 1;
            while ((1 << s.lc_bits) < sp.max_rows + s.cap + 2) ++s.lc_bits;
            if (s.lc_bits + s.code_bits > kResWordBits) s.lc_bits = kResWordBits - s.code_bits; // (checked against the real counts below)
            if (plan_failed(hipMemcpy(s.pl->wg_row0.p, sp.wr.data(), sp.wr.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
                            hipMemsetAsync(s.fail.p, 0, sizeof(int), s.stream) != hipSuccess))
                return "plan upload failed";
            // (round 0 of a later tier is the split of the first tier's round 0: its counts are re-used, the words re-encoded only if it is accepted)
            const bool reuse_round0 = round == 0 && round0_done && !equal_lanes && !s.lt; // (local tables belong to ONE split)
            if (reuse_round0) s.rc = rc_round0;
            else {
                const int rm = resident_remap(s);
                if (rm < 0) return "remap failed";
                if (rm == 2) return s.lt_why.c_str();
                if (rm > 0) {
                    tier->last_reason = "a workgroup reads more remote columns than its source list holds";
                    break;
                }
            }
            const ResidentCounts counts = s.counts();
            if (round == 0) {
                if (!reuse_round0) {
                    rc_round0 = s.rc;
                    round0_done = true;
                }
                // a tier whose TOTAL demand is close to the chip's LDS never fits (lanes, not LDS, bound the split; every further round is a
                // re-encoding pass: 10 ms of plan time on a 1.3 M-row system): next tier
                if (total_demand(counts, t_max) > 0.88 * limit * (double)G) break;
                // the remote columns are known now: one more split that counts them
                if (c_rem > 0. && !extras_off && spread_remote_cost(s.rc, c_rem, &sp)) {
                    extras_active = true;
                    continue;
                }
            }
            // LDS split: every workgroup holds its slice of u + its remote-column cache, and as many of r, p, s as still fit (tiers: NG =
            // 0 .. 3 of them in global memory instead).  Footprint of workgroup b: (4 - NG) rows_b + remote_b entries; the largest decides.
            tier->max_cols = max_local_columns(counts);
            for (int t = 0; t <= 3 && t <= max_ng && tier->ng < 0; ++t) {
                const size_t need = (size_t)largest_footprint(counts, t) * esz + lds_extra;
                if (s.verbose) fprintf(stderr, "[avs resident] round %d, LDS tier %d: largest workgroup footprint %zu B (limit %zu)\n", round, t, need, lds_max);
                if (need <= lds_max) {
                    tier->ng = t;
                    tier->lds = need;
                }
            }
            if (tier->ng >= 0) {
                if (reuse_round0) { // accepted on re-used counts: the words still hold another split's encoding
                    const int rm = resident_remap(s);
                    if (rm == 2) return s.lt_why.c_str();
                    if (rm != 0) return "remap failed";
                }
                continue;
            }
            // shrink the offenders (at the largest tier allowed) and split again ... unless the MEDIAN workgroup does not fit either:
            // no re-split helps, go to the next tier
            if (median_footprint(counts, t_max) > 0.98 * limit) break;
            if (reweight_offenders(counts, t_max, limit, &sp)) reweighted = true;
        }
    }
    return nullptr;
}

// the tables of the accepted split, back to back
static const char *resident_pack_tables(ResidentSplitState &s)
{
    ResidentPlan *pl = s.pl;
    std::vector<int32_t> toff(s.tcnt.size() + 1, 0);
    for (size_t g = 0; g < s.tcnt.size(); ++g) toff[g + 1] = toff[g] + s.tcnt[g];
    if (plan_failed(pl->ltab_off.alloc(toff.size()) != AVS_OK || pl->ltab.alloc((size_t)toff.back()) != AVS_OK ||
                    hipMemcpy(pl->ltab_off.p, toff.data(), toff.size() * 4, hipMemcpyHostToDevice) != hipSuccess))
        return "plan allocation failed";
    hipLaunchKernelGGL(k_resident_pack_tables, dim3((unsigned)s.tcnt.size()), dim3(256), 0, s.stream, (const double *)s.lt_strided.p, s.lt_cap,
                       (const int32_t *)pl->ltab_off.p, pl->ltab.p);
    if (plan_failed(hipGetLastError() != hipSuccess || hipStreamSynchronize(s.stream) != hipSuccess)) return "table layout failed";
    return nullptr;
}

// a partitioned plan: the push segments of every peer's send list and the workgroups that wait for the peers' flags (every workgroup
// overlapping a halo-reading 512-row tile of the plan)
static const char *resident_partition_arrays(ResidentPlan *pl, const DirectArgs *da, const std::vector<int32_t> &wr, int64_t n,
                                             std::vector<int32_t> *seg, std::vector<uint8_t> *whalo)
{
    DistDev h;
    if (plan_failed(hipMemcpy(&h, da->dd, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess)) return "DistDev download failed";
    if (h.paranoid) return "paranoid mode keeps the launch-per-phase loop";
    std::vector<int32_t> sidx((size_t)(da->n_send > 0 ? da->n_send : 1));
    if (plan_failed(da->n_send && hipMemcpy(sidx.data(), h.send_idx, (size_t)da->n_send * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess))
        return "send list download failed";
    pl->n_push_wgs = push_segments(h.send_off, h.npeers, sidx.data(), wr, seg);
    std::vector<int32_t> tb((size_t)(da->n_tiles_bnd > 0 ? da->n_tiles_bnd : 1));
    if (plan_failed(da->n_tiles_bnd &&
                    hipMemcpy(tb.data(), da->tiles_bnd, (size_t)da->n_tiles_bnd * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess))
        return "tile list download failed";
    halo_workgroups(tb.data(), da->n_tiles_bnd, kTileRows, n, wr, whalo);
    return nullptr;
}

static const char *resident_upload(ResidentPlan *pl, const ResidentLanes &lanes, const std::vector<int32_t> &wl, const std::vector<int32_t> &seg,
                                   const std::vector<uint8_t> &whalo)
{
    const size_t L = (size_t)lanes.size(), G = whalo.size();
    if (!(pl->lane_row0.alloc(L) == AVS_OK && pl->lane_meta.alloc(L) == AVS_OK && pl->wg_lane0.alloc(G + 1) == AVS_OK &&
          pl->push_seg.alloc(seg.size()) == AVS_OK && pl->wg_halo.alloc(G) == AVS_OK && pl->bar_count.alloc(2) == AVS_OK &&
          pl->bar_flags.alloc(G) == AVS_OK && pl->slots.alloc(G * 4) == AVS_OK && pl->bcast.alloc(4 * kResGens) == AVS_OK))
        return "plan allocation failed";
    if (plan_failed(!(hipMemcpy(pl->lane_row0.p, lanes.row0.data(), L * 4, hipMemcpyHostToDevice) == hipSuccess &&
                      hipMemcpy(pl->lane_meta.p, lanes.meta.data(), L * 4, hipMemcpyHostToDevice) == hipSuccess &&
                      hipMemcpy(pl->wg_lane0.p, wl.data(), wl.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
                      hipMemcpy(pl->push_seg.p, seg.data(), seg.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
                      hipMemcpy(pl->wg_halo.p, whalo.data(), whalo.size(), hipMemcpyHostToDevice) == hipSuccess)))
        return "plan upload failed";
    return nullptr;
}

// the waves' lane-interleaved streams of the rows that do not fit the registers; *run = their quads, padding included
static const char *resident_stream_layout(ResidentSplitState &s, uint32_t padword, int64_t *run)
{
    ResidentPlan *pl = s.pl;
    std::vector<int32_t> soff;
    *run = wave_stream_offsets(s.split.wl, *s.lanes, &soff);
    if (*run >= (1ll << 29)) return "streamed quads exceed 32-bit offsets";
    if (plan_failed(pl->swords.alloc((size_t)*run * 4) != AVS_OK || pl->wave_soff.alloc(soff.size()) != AVS_OK ||
                    hipMemcpy(pl->wave_soff.p, soff.data(), soff.size() * 4, hipMemcpyHostToDevice) != hipSuccess))
        return "stream allocation failed";
    hipLaunchKernelGGL(k_resident_stream_layout, dim3((unsigned)s.G), dim3(kResThreads), 0, s.stream, s.A->row_ptr, (const uint32_t *)pl->rwords.p,
                       (const int32_t *)pl->lane_row0.p, (const uint32_t *)pl->lane_meta.p, (const int32_t *)pl->wg_lane0.p,
                       (const int32_t *)pl->wave_soff.p, padword, reinterpret_cast<u4_t *>(pl->swords.p));
    if (plan_failed(hipGetLastError() != hipSuccess || hipStreamSynchronize(s.stream) != hipSuccess)) return "stream layout failed";
    return nullptr;
}

// The plan of this matrix, vector type and option is kept; otherwise the plan is reset for a new attempt under the new key.
static bool resident_plan_is_current(ResidentPlan *pl, const CsrView &A, const DirectArgs *da, bool f32)
{
    const void *key[4] = {A.row_ptr, A.packed, A.table, da ? (const void *)da->dd : nullptr};
    const bool opt_local = cur_opt().resident_local_tables != 0; // (part of the key, like the vector type: switching the option plans again)
    if (pl->tried && memcmp(key, pl->key, sizeof(key)) == 0 && pl->key_n == A.n && pl->key_epoch == A.epoch && pl->f32 == f32 &&
        pl->key_local == opt_local)
        return true;
    pl->key_local = opt_local;
    pl->local = false;
    pl->key_epoch = A.epoch; // (a re-assembly with the same DOF count rewrites the same buffers: the words of the plan would be stale)
    pl->tried = true;
    pl->ok = false;
    pl->f32 = f32;          // (part of the key: a plan laid out for one vector type never runs the other's kernel; switching the option
                            // re-plans, which also tries the resident loop again after a fault retired the other plan)
    memcpy(pl->key, key, sizeof(key));
    pl->key_n = A.n;
    pl->n_lanes = pl->streamed_rows = pl->streamed_words = 0;
    pl->max_lanes = pl->max_rows = pl->long_lanes = pl->longest_tail = pl->max_lane_streamed = pl->max_remote = pl->remap_passes = pl->lt_max = 0;
    return false;
}

// Builds (or re-uses) the plan for A; returns false (with plan->why) when the system does not qualify.  f32: for the float-vector
// kernel -- the LDS holds T = float slices, remote columns and tables, so the split and the tier are chosen for 4-B entries.
static bool resident_prepare(ResidentPlan *pl, const CsrView &A, int64_t n_cols, const DirectArgs *da, bool f32, hipStream_t stream)
{
    if (resident_plan_is_current(pl, A, da, f32)) return pl->ok; // 1. the key
    const size_t esz = f32 ? sizeof(float) : sizeof(double); // LDS entry of the vector slices, remote columns and tables
    const bool verbose = cur_opt().resident_verbose > 0;
    PlanClock clock(verbose);
    const int64_t n = A.n;
    auto no = [&](const char *why) { return resident_refuse(pl, why, n); };

    // ---- 2. cheap refusals (before the row pointers cross PCIe and the host walks them: 20-100 ms at 4-7 M rows, per new matrix) ----
    // lt: a matrix that fails only these two dictionary conditions is planned with local value tables when the option asks for it
    const bool lt = resident_local_tables_wanted(A);
    if (!lt && (!A.packed || !A.codes || A.tab_ptr || A.cbase || A.col_bits <= 0)) return no("needs the packed single-dictionary form");
    if ((!lt && A.table_size > 1023) || A.n < 1 || A.n >= (1ll << 31)) return no("dictionary too large");
    int dev = 0, cus = 0, coop = 0;
    if (plan_failed(hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
                    hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, dev) != hipSuccess || !coop || cus < 1))
        return no("no cooperative launch");
    int G = cus;
    if (cur_opt().resident_cus > 0 && cur_opt().resident_cus < cus) G = cur_opt().resident_cus; // tests: two ranks on ONE GPU, each on a share of the CUs
    // every workgroup keeps its slice of u in LDS next to its remote columns (never less than about half as much again)
    if ((size_t)(n / G) * esz > (size_t)(160 * 1024) * 65 / 100) return no("the workgroups' slices of u leave no room for their remote columns in the LDS");

    // ---- 3. the row pointers ----
    std::vector<int32_t> rp((size_t)n + 1);
    if (plan_failed(hipMemcpyAsync(rp.data(), A.row_ptr, rp.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
                    hipStreamSynchronize(stream) != hipSuccess))
        return no("row pointer download failed");
    clock.stage("row pointers to the host");

    // ---- 4. lanes (avs_resident_plan.cpp) ----
    int max_quads = kResQuads;
    if (cur_opt().resident_max_quads >= 1 && cur_opt().resident_max_quads <= kResQuads) max_quads = cur_opt().resident_max_quads; // tests: long-row path
    ResidentLanes lanes;
    int64_t q_total = 0;
    double stream_T = 0.;
    if (const char *why = lanes_in_registers(rp.data(), n, G, max_quads, &lanes, &q_total)) return no(why);
    clock.stage("lanes (registers only)");
    if (const char *why = lanes_with_streams(rp.data(), n, G, max_quads, cur_opt().resident_lane_fill, cur_opt().resident_no_stream != 0, q_total,
                                             &lanes, &stream_T))
        return no(why);
    clock.stage("lanes with streamed rows");
    const int64_t L = lanes.size();
    pl->n_lanes = L;
    pl->long_lanes = lanes.long_lanes;
    pl->longest_tail = lanes.longest_tail;
    pl->streamed_rows = lanes.streamed_rows;
    pl->max_lane_streamed = lanes.max_lane_streamed;
    pl->streamed_words = lanes.streamed_words;

    // ---- 5. the split: tiers and rounds ----
    ResidentSplitState s;
    s.pl = pl;
    s.A = &A;
    s.lanes = &lanes;
    s.stream = stream;
    s.lt = lt;
    s.verbose = verbose;
    s.G = G;
    s.n = n;
    const size_t lds_max = 160 * 1024 - 4096 - 1024;
    // the two tables (values + zero, inverted values) in T, then the fold space (3 x 16 wave sums) and 4 + 4 scalars in double
    // (local tables: their entries are counted per workgroup, tabs[b], next to the remote columns; no inverted values in LDS)
    const size_t lds_extra = (lt ? 0 : 2 * ((size_t)A.table_size + 1) * esz) + (48 + 8) * sizeof(double);
    if (const char *why = resident_split_setup(s, n_cols, stream_T)) return no(why);
    ResidentTier tier;
    if (const char *why = resident_split_rounds(s, stream_T, esz, lds_max, lds_extra, &tier)) return no(why);
    clock.stage("split + re-encoding rounds");
    const int ng = tier.ng, max_rows = s.split.max_rows;
    pl->max_rows = max_rows;
    pl->max_remote = *std::max_element(s.rc.begin(), s.rc.end());
    pl->lt_max = s.lt_max;
    if (verbose) {
        std::vector<int32_t> srt(s.rc);
        std::sort(srt.begin(), srt.end());
        fprintf(stderr, "[avs resident] remote columns per workgroup: min %d / median %d / 90 %% %d / max %d; rows per workgroup <= %d\n", srt[0],
                srt[(size_t)G / 2], srt[(size_t)G * 9 / 10], srt[(size_t)G - 1], max_rows);
    }
    if (ng < 0) {
        if (lt && s.lt_max > 0) { // the quantity that did not fit: the LDS, with the tables it would have had to hold
            char msg[256];
            snprintf(msg, sizeof(msg), "%s (local tables per %s, largest %d values, up to %d table entries per workgroup)", tier.last_reason,
                     s.lt_gpw == 1 ? "workgroup" : "wave", s.lt_max, *std::max_element(s.tabs.begin(), s.tabs.end()));
            return no(msg);
        }
        return no(tier.last_reason);
    }

    // ---- 6. the accepted plan: tables, kernel, partition arrays, uploads, streams ----
    if (lt && verbose)
        fprintf(stderr, "[avs resident] local tables: one per %s, largest %d values (%s %d%s), %d code bits + %d column bits of %d, LDS tier %d, "
                        "<= %d table entries per workgroup, inverse diagonal per row (no LDS)\n", s.lt_gpw == 1 ? "workgroup" : "wave", s.lt_max,
                s.lt_gpw == 1 ? "workgroup" : "wave", s.lt_gpw == 1 ? s.lt_max_grp : s.lt_max_grp % 16,
                s.lt_gpw == 1 ? "" : (" of workgroup " + std::to_string(s.lt_max_grp / 16)).c_str(), s.code_bits, s.lc_bits, kResWordBits, ng,
                *std::max_element(s.tabs.begin(), s.tabs.end()));
    if ((1 << s.lc_bits) < tier.max_cols) return no("rows + remote columns exceed the word's column bits");
    if (lt)
        if (const char *why = resident_pack_tables(s)) return no(why);
    const std::vector<int32_t> &wl = s.split.wl;
    int64_t lpw = 0;
    for (int b = 0; b < G; ++b) lpw = std::max<int64_t>(lpw, wl[(size_t)b + 1] - wl[(size_t)b]);
    const void *kern = resident_kernel(ng, lanes.streamed_words > 0, f32, lt);
    if (plan_failed(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096) != hipSuccess)) return no("LDS opt-in refused");
    int per_cu = 0;
    if (plan_failed(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kResThreads, tier.lds) != hipSuccess || per_cu < 1))
        return no("kernel does not fit a CU (registers / LDS)");
    std::vector<uint8_t> whalo((size_t)G, 0);
    std::vector<int32_t> seg(1, 0);
    if (da && da->dd)
        if (const char *why = resident_partition_arrays(pl, da, s.split.wr, n, &seg, &whalo)) return no(why);
    if (const char *why = resident_upload(pl, lanes, wl, seg, whalo)) return no(why);
    clock.stage("push segments, uploads");
    pl->streams = false;
    if (lanes.streamed_words > 0) {
        int64_t run = 0;
        if (const char *why = resident_stream_layout(s, lt ? 0u : (uint32_t)A.table_size << s.lc_bits, &run)) return no(why);
        pl->streams = true;
        if (verbose)
            fprintf(stderr, "[avs resident] streamed rows: %.1f %% of the words (%lld of %lld), %.1f MB per iteration incl. padding, %.1f streamed quads per lane\n",
                    100. * (double)lanes.streamed_words / (double)A.nnz, (long long)lanes.streamed_words, (long long)A.nnz, (double)run * 16e-6, stream_T);
    }
    if (verbose) {
        fprintf(stderr, "[avs resident] plan built in %.2f ms (host: lanes + split; device: re-encoding)\n", clock.total());
        fprintf(stderr, "[avs resident] plan: n = %lld, %lld lanes (%lld per workgroup), %d workgroups, <= %d rows per workgroup, %d-bit local columns, "
                        "%d row-local vectors in global memory, LDS %zu B, %s vectors\n", (long long)n, (long long)L, (long long)lpw, G, max_rows, s.lc_bits, ng,
                tier.lds, f32 ? "float" : "fp64");
    }

    // ---- 7. the plan ----
    pl->G = G;
    pl->max_lanes = (int)lpw;
    pl->lc_bits = s.lc_bits;
    pl->max_quads = max_quads;
    pl->ng = ng;
    pl->lds = tier.lds;
    pl->local = lt;
    pl->lt_gpw = s.lt_gpw;
    pl->ok = true;
    pl->why.clear();
    return true;
}

// per-phase averages of workgroup 0 (tuning aid, AVS_CG_RESIDENT_TIMERS) after a launch with a.timers set
static avs_status resident_report_timers(ResidentPlan *pl, int khz, hipStream_t stream)
{
    std::vector<long long> t((size_t)pl->max_timed * kResTimers + (size_t)pl->G * 4);
    AVS_HIP(hipMemcpyAsync(t.data(), pl->timers.p, t.size() * sizeof(long long), hipMemcpyDeviceToHost, stream));
    AVS_HIP(hipStreamSynchronize(stream));
    {
        const long long *wt = t.data() + (size_t)pl->max_timed * kResTimers;
        std::vector<double> ua, sp, tot;
        long long first = 0;
        for (int b = 0; b < pl->G; ++b)
            if (wt[4 * b + 3]) {
                if (!first || wt[4 * b] < first) first = wt[4 * b];
            }
        for (int b = 0; b < pl->G; ++b)
            if (wt[4 * b + 3]) {
                ua.push_back((double)(wt[4 * b + 1] - wt[4 * b]) * 1e3 / khz);
                sp.push_back((double)(wt[4 * b + 3] - wt[4 * b + 2]) * 1e3 / khz);
                tot.push_back((double)(wt[4 * b + 3] - first) * 1e3 / khz);
            }
        if (!tot.empty() && cur_opt().resident_verbose > 0) {
            std::vector<int32_t> wl2((size_t)pl->G + 1), wr2((size_t)pl->G + 1), rc2((size_t)pl->G);
            (void)hipMemcpy(wl2.data(), pl->wg_lane0.p, wl2.size() * 4, hipMemcpyDeviceToHost);
            (void)hipMemcpy(wr2.data(), pl->wg_row0.p, wr2.size() * 4, hipMemcpyDeviceToHost);
            (void)hipMemcpy(rc2.data(), pl->rem_count.p, rc2.size() * 4, hipMemcpyDeviceToHost);
            std::vector<int> order((size_t)pl->G);
            for (int b = 0; b < pl->G; ++b) order[(size_t)b] = b;
            std::sort(order.begin(), order.end(), [&](int x, int y) { return wt[4 * x + 3] > wt[4 * y + 3]; });
            for (int i = 0; i < 4; ++i) {
                const int b = order[(size_t)i];
                fprintf(stderr, "[avs resident]   slow workgroup %d: %d lanes, %d rows, %d remote; update %.2f, barrier+fill %.2f, spmv %.2f us\n", b,
                        wl2[(size_t)b + 1] - wl2[(size_t)b], wr2[(size_t)b + 1] - wr2[(size_t)b], rc2[(size_t)b], (double)(wt[4 * b + 1] - wt[4 * b]) * 1e3 / khz,
                        (double)(wt[4 * b + 2] - wt[4 * b + 1]) * 1e3 / khz, (double)(wt[4 * b + 3] - wt[4 * b + 2]) * 1e3 / khz);
            }
            const int b = order[(size_t)pl->G / 2];
            fprintf(stderr, "[avs resident]   median workgroup %d: %d lanes, %d rows, %d remote; update %.2f, barrier+fill %.2f, spmv %.2f us\n", b,
                    wl2[(size_t)b + 1] - wl2[(size_t)b], wr2[(size_t)b + 1] - wr2[(size_t)b], rc2[(size_t)b], (double)(wt[4 * b + 1] - wt[4 * b]) * 1e3 / khz,
                    (double)(wt[4 * b + 2] - wt[4 * b + 1]) * 1e3 / khz, (double)(wt[4 * b + 3] - wt[4 * b + 2]) * 1e3 / khz);
        }
        if (!ua.empty()) {
            auto q = [](std::vector<double> v, double f) { std::sort(v.begin(), v.end()); return v[(size_t)((v.size() - 1) * f)]; };
            fprintf(stderr, "[avs resident] iteration 20, all workgroups, us (min / median / max): update %.2f / %.2f / %.2f | spmv %.2f / %.2f / %.2f | "
                            "SpMV done after the first workgroup started %.2f / %.2f / %.2f\n", q(ua, 0), q(ua, .5), q(ua, 1), q(sp, 0), q(sp, .5), q(sp, 1),
                    q(tot, 0), q(tot, .5), q(tot, 1));
        }
    }
    double sum[5] = {0, 0, 0, 0, 0};
    int cnt = 0;
    for (int i = 0; i < pl->max_timed; ++i) {
        const long long *q = t.data() + (size_t)i * kResTimers;
        if (!q[5]) break;
        for (int k = 0; k < 5; ++k) sum[k] += (double)(q[k + 1] - q[k]);
        ++cnt;
    }
    if (cur_opt().resident_verbose >= 2)
        for (int i = 0; i < pl->max_timed && i < 80; ++i) {
            const long long *q = t.data() + (size_t)i * kResTimers;
            double rr, den;
            memcpy(&rr, q + 6, 8);
            memcpy(&den, q + 7, 8);
            fprintf(stderr, "[avs resident]   it %d: |r|^2 %.6e  alpha denominator %.6e\n", i, rr, den);
        }
    if (cnt)
        fprintf(stderr, "[avs resident] %d iterations of workgroup 0, us: update+push %.2f | barrier+inv+flags %.2f | remote fill %.2f | spmv+fold %.2f | "
                        "reduce+broadcast %.2f\n", cnt, sum[0] / cnt * 1e3 / khz, sum[1] / cnt * 1e3 / khz, sum[2] / cnt * 1e3 / khz,
                sum[3] / cnt * 1e3 / khz, sum[4] / cnt * 1e3 / khz);
    return AVS_OK;
}

// Runs the rest of the solve (state in sc / the vectors, as the set-up rounds left it) in ONE cooperative launch.
// *launched = false: the cooperative launch was refused (the grid is not co-resident on this device right now); nothing was
// touched, the plan is retired and the caller carries on with the launch-per-phase loop.
// T: the plan's vector type (resident_prepare's f32).  A plan with local value tables (pl->local) takes ONE INVERSE PER ROW in `invtab`
// (the launch-per-phase loops' array) and ignores dcode.
template <typename T>
static avs_status resident_run(ResidentPlan *pl, const CsrView &A, T *x, T *r, T *p, T *s, T *u, T *wv, const uint16_t *dcode,
                               const T *invtab, PcgScalars *sc, int max_iters, const DirectArgs *da, hipStream_t stream, bool *launched)
{
    *launched = false;
    constexpr bool F32 = std::is_same<T, float>::value;
    AVS_REQUIRE(pl->f32 == F32, AVS_EINTERNAL, "the resident plan was laid out for the other vector type");
    ResidentArgs<T> a{};
    a.row_ptr = A.row_ptr;
    a.table = pl->local ? pl->ltab.p : A.table;
    a.table_size = pl->local ? 0 : A.table_size; // (local tables: entry 0 of every table is the zero of the padding words)
    a.ltab_cnt = pl->local ? pl->ltab_cnt.p : nullptr;
    a.ltab_off = pl->local ? pl->ltab_off.p : nullptr;
    a.ltab_gpw = pl->lt_gpw;
    a.n = (int)A.n;
    a.G = pl->G;
    a.lane_row0 = pl->lane_row0.p;
    a.lane_meta = pl->lane_meta.p;
    a.wg_lane0 = pl->wg_lane0.p;
    a.wg_row0 = pl->wg_row0.p;
    a.rwords = pl->rwords.p;
    a.swords = pl->streams ? pl->swords.p : nullptr;
    a.wave_soff = pl->streams ? pl->wave_soff.p : nullptr;
    a.lc_bits = pl->lc_bits;
    a.max_quads = pl->max_quads;
    a.rem_list = pl->rem_list.p;
    a.rem_stride = (int)(pl->rem_list.n / (size_t)pl->G);
    a.rem_count = pl->rem_count.p;
    a.x = x; a.r = r; a.p = p; a.s = s; a.u = u; a.w = wv;
    a.dcode = dcode;
    a.invtab = invtab;
    a.bar_count = pl->bar_count.p;
    a.bar_flags = pl->bar_flags.p;
    a.dep_mask = pl->dep_mask.p;
    a.n_push_wgs = pl->n_push_wgs > 0 ? pl->n_push_wgs : 1;
    a.slots = pl->slots.p;
    a.bcast = pl->bcast.p;
    a.sc = sc;
    a.max_iters = max_iters;
    int dev = 0, khz = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) {
        (void)hipGetLastError();
        khz = 100000;
    }
    // a wait between workgroups of ONE device ends in microseconds unless the cooperative grid is not co-resident in time (a shared
    // GPU): 2 s, then the solve is redone by the launch-per-phase loop in the same call; waits on peers keep the transport's 20 s
    long long ms = da ? 20000 : 2000;
    if (cur_opt().dist_timeout_ms > 0) ms = cur_opt().dist_timeout_ms;
    a.timeout_ticks = (long long)khz * ms;
    a.dd = da ? da->dd : nullptr;
    a.epoch = da ? da->epoch : nullptr;
    a.wg_halo = pl->wg_halo.p;
    a.push_seg = pl->push_seg.p;
    a.timers = nullptr;
    a.max_timed = 0;
    a.coherent_fill = cur_opt().resident_coherent_fill;
    if (cur_opt().resident_timers > 0) {
            pl->max_timed = cur_opt().resident_timers > 4096 ? 4096 : cur_opt().resident_timers;
            AVS_TRY(pl->timers.alloc((size_t)pl->max_timed * kResTimers + (size_t)pl->G * 4));
            AVS_HIP(hipMemsetAsync(pl->timers.p, 0, ((size_t)pl->max_timed * kResTimers + (size_t)pl->G * 4) * sizeof(long long), stream));
            a.timers = pl->timers.p;
            a.max_timed = pl->max_timed;
            a.wg_times = pl->timers.p + (size_t)pl->max_timed * kResTimers;
        }
    AVS_HIP(hipMemsetAsync(pl->bar_count.p, 0, 2 * sizeof(unsigned), stream));
    AVS_HIP(hipMemsetAsync(pl->bar_flags.p, 0, (size_t)pl->G * sizeof(unsigned long long), stream));
    AVS_HIP(hipMemsetAsync(pl->slots.p, 0xFF, (size_t)pl->G * 4 * sizeof(double), stream));   // armed: kSentinel in every slot
    AVS_HIP(hipMemsetAsync(pl->bcast.p, 0xFF, 4 * kResGens * sizeof(double), stream));
    void *args[] = {&a};
    const hipError_t le = hipLaunchCooperativeKernel(resident_kernel<T>(pl->ng, pl->streams, pl->local), dim3((unsigned)pl->G), dim3(kResThreads), args, (unsigned)pl->lds, stream);
    if (le != hipSuccess) {
        (void)hipGetLastError();
        pl->ok = false;
        pl->why = std::string("cooperative launch refused: ") + hipGetErrorString(le);
        if (cur_opt().resident_verbose > 0) fprintf(stderr, "[avs resident] not used: %s\n", pl->why.c_str());
        return AVS_OK;
    }
    *launched = true;
    if (a.timers) AVS_TRY(resident_report_timers(pl, khz, stream));
    return AVS_OK;
}
