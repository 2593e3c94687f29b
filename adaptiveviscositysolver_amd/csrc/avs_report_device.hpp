// avs_report_device.hpp -- device code the diagnostics share (avs_check.hip, avs_stress_check.hip, avs_csr_check.hip, avs_strain.hip,
// avs_solution_check.hip, avs_spectrum.hip): wave folds of a 64-bit word into a raw report, the sizing of the persistent grids, the
// 256-row chunk stream product with its partial sum, and the numbering kernel of the two pyramid checks.  Integer atomics only: the same
// inputs give the same raw report whatever the order of the waves.
#pragma once

#include "avs_report.hpp"
#include "avs_wave.hpp"

namespace avs {

constexpr int kReportGrid = 2048; // persistent grids: eight workgroups per CU
// workgroups of kBlock threads for `workgroups` of work, at least one, at most cap (cap <= 0: kReportGrid)
inline unsigned report_grid(long long workgroups, int cap)
{
    const long long lim = cap > 0 ? cap : kReportGrid;
    return (unsigned)(workgroups < 1 ? 1 : (workgroups < lim ? workgroups : lim));
}
constexpr long long report_workgroups(long long threads) { return (threads + kBlock - 1) / kBlock; }

__device__ __forceinline__ bool finite_bits(double v)
{
    return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// the sum / smallest / largest of the wave's 64 values, in every lane
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long s)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += (unsigned long long)__shfl_xor((long long)s, o, 64);
    return s;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long m)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = (unsigned long long)__shfl_xor((long long)m, o, 64);
        m = other < m ? other : m;
    }
    return m;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long m)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = (unsigned long long)__shfl_xor((long long)m, o, 64);
        m = other > m ? other : m;
    }
    return m;
}

// What a lane found, folded into the raw report; every lane of the wave arrives here, and lane 0 issues one atomic if the wave has
// something for the word.  raw[word] += the wave's sum of v:
__device__ __forceinline__ void raw_add(unsigned long long v, int word, unsigned long long *raw)
{
    const unsigned long long s = wave_sum_u64(v);
    if (((int)threadIdx.x & 63) == 0 && s) atomicAdd(raw + word, s);
}
// raw[word] = min(raw[word], the wave's smallest key) (kNoKey: the lane has none)
__device__ __forceinline__ void raw_min(unsigned long long key, int word, unsigned long long *raw)
{
    const unsigned long long m = wave_min_u64(key);
    if (((int)threadIdx.x & 63) == 0 && m != kNoKey) atomicMin(raw + word, m);
}
// raw[word] = max(raw[word], the wave's largest v); a count, or the bit pattern of a double >= 0 that is no NaN: those order as the values
__device__ __forceinline__ void raw_max_bits(unsigned long long bits, int word, unsigned long long *raw)
{
    const unsigned long long m = wave_max_u64(bits);
    if (((int)threadIdx.x & 63) == 0 && m) atomicMax(raw + word, m);
}
__device__ __forceinline__ void raw_max_bits(double v, int word, unsigned long long *raw)
{
    raw_max_bits((unsigned long long)__double_as_longlong(v), word, raw);
}
// raw_add of N counts and raw_min of the key of the first violation.  The folds are written out here: through raw_add and raw_min the
// register allocation of k_check_labels (avs_check.hip) changes and its level-0 pass slows down (profiles/diagnostics_refactor.md).
template <int N>
__device__ __forceinline__ void raw_commit(const unsigned (&c)[N], const int (&word)[N], unsigned long long key, int key_word, unsigned long long *raw)
{
    const int lane = (int)threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < N; ++r) {
        unsigned long long s = c[r];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += (unsigned long long)__shfl_xor((long long)s, o, 64);
        if (lane == 0 && s) atomicAdd(raw + word[r], s);
    }
    unsigned long long m = key;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = (unsigned long long)__shfl_xor((long long)m, o, 64);
        m = other < m ? other : m;
    }
    if (lane == 0 && m != kNoKey) atomicMin(raw + key_word, m);
}

// The stream product of avs_spmv.hip for one chunk of 256 consecutive rows: y of row row0 + threadIdx.x (0 behind row n); every thread
// of the workgroup calls it.  Phase 1 streams the chunk's (val, col) pairs fully coalesced with non-temporal loads (the matrix is read
// once and must not evict x from L2), gathers x[col] with plain loads and parks the products in LDS tiles of kStreamCap (prod); phase 2:
// one lane per row adds its segment of the tile left to right, y = y + val[k] * x[col[k]] in stored order, across as many tiles as the
// row has (the order of k_spmv_stream and of the oracle).
__device__ __forceinline__ double chunk_stream_product(const int32_t *__restrict__ rp, const int32_t *__restrict__ col, const double *__restrict__ val,
                                                       const double *__restrict__ x, int n, long long row0, double *prod)
{
    const int tid = threadIdx.x;
    const long long row = row0 + tid;
    const long long rlast = row0 + kBlock < n ? row0 + kBlock : n;
    const long long s_blk = rp[row0], e_blk = rp[rlast];
    long long rs = 0, re = 0;
    if (row < n) {
        rs = rp[row];
        re = rp[row + 1];
    }
    double y = 0.;
    for (long long ts = s_blk; ts < e_blk; ts += kStreamCap) {
        const long long te = ts + kStreamCap < e_blk ? ts + kStreamCap : e_blk;
        // phase 1: coalesced stream of (val, col), gather x, products to LDS; four independent loads per lane in flight per trip
        long long k = ts + tid;
        for (; k + 3 * kBlock < te; k += 4 * kBlock) {
            const double v0 = stream_load<true>(val + k), v1 = stream_load<true>(val + k + kBlock), v2 = stream_load<true>(val + k + 2 * kBlock),
                         v3 = stream_load<true>(val + k + 3 * kBlock);
            const int c0 = stream_load<true>(col + k), c1 = stream_load<true>(col + k + kBlock), c2 = stream_load<true>(col + k + 2 * kBlock),
                      c3 = stream_load<true>(col + k + 3 * kBlock);
            const double x0v = x[c0], x1v = x[c1], x2v = x[c2], x3v = x[c3];
            const int o = (int)(k - ts);
            prod[o] = v0 * x0v;
            prod[o + kBlock] = v1 * x1v;
            prod[o + 2 * kBlock] = v2 * x2v;
            prod[o + 3 * kBlock] = v3 * x3v;
        }
        for (; k < te; k += kBlock) prod[(int)(k - ts)] = stream_load<true>(val + k) * x[stream_load<true>(col + k)];
        __syncthreads();
        // phase 2: each row adds its part of the tile, left to right
        const long long a = rs > ts ? rs : ts, e = re < te ? re : te;
        for (long long j = a; j < e; ++j) y = y + prod[(int)(j - ts)];
        __syncthreads();
    }
    return y;
}

// the chunk's partial sum: wave sums (in lane 63), then ((w0 + w1) + w2) + w3 as block_sum of avs_wave.hpp adds them.  red: by the parity
// of the workgroup's trip, thread 0 may still read one while the next is written.
__device__ __forceinline__ void chunk_partial_sum(double term, double (*red)[4], int parity, double *out)
{
    const double w = wave_sum_dpp(term);
    if (((int)threadIdx.x & 63) == 63) red[parity][(int)threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) *out = ((red[parity][0] + red[parity][1]) + red[parity][2]) + red[parity][3];
}

// the numbering rule of an index pyramid (AVS_RULE_NUMBERING, AVS_STRESS_RULE_EDGE_NUMBERING, AVS_STRESS_RULE_CENTER_NUMBERING) over the
// occurrence counters its lattice walk left: every id below n_ids exactly once.  raw[rule] counts, raw[key_word] takes the first id.
// Defined in avs_check.hip.
__global__ __launch_bounds__(kBlock) void k_index_numbering(const int32_t *__restrict__ occ, int n_ids, int rule, int key_word, unsigned long long *__restrict__ raw);

} // namespace avs
