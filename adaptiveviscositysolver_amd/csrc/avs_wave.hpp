// avs_wave.hpp -- device helpers shared by the SpMV kernels (avs_spmv.hip, avs_brick.hip) and the PCG loops' vector kernels (avs_pcg.hip
// and its .inl files): wave / block reductions in a fixed order, cache-hinted stream loads, the 8- and 16-byte vector types, and the
// geometry of the 256-thread kernels.  Nothing here crosses the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace avs {

constexpr int kBlock = 256;
constexpr int kVecGrid = 2048;        // grid-stride vector kernels: 8 blocks per CU
constexpr int kStreamCap = 4096;      // LDS products per tile (32 KiB)
inline int stream_grid(int64_t n) { return (int)((n + kBlock - 1) / kBlock); }

typedef double d2_t __attribute__((ext_vector_type(2)));
typedef int i2_t __attribute__((ext_vector_type(2)));
typedef unsigned short us4_t __attribute__((ext_vector_type(4)));
typedef int i4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u4_t __attribute__((ext_vector_type(4)));
typedef float f4_t __attribute__((ext_vector_type(4)));
typedef unsigned u2_t __attribute__((ext_vector_type(2)));

// 16 B of a vector of T -- the unit of the vector kernels' accesses and of the resident kernel's write-through stores: `rows` rows,
// and the rows' 2-B diagonal codes as `codes` (two codes per 32-bit word, the even row's in the low half)
template <typename T> struct Vec16;
template <> struct Vec16<double> { typedef d2_t type; typedef unsigned codes; static constexpr int rows = 2, log2_rows = 1; };
template <> struct Vec16<float> { typedef f4_t type; typedef u2_t codes; static constexpr int rows = 4, log2_rows = 2; };
__device__ __forceinline__ unsigned code_of(unsigned words, int k) { return k & 1 ? words >> 16 : words & 0xffffu; }
__device__ __forceinline__ unsigned code_of(u2_t words, int k) { return code_of(k < 2 ? words.x : words.y, k); }

// ---------------------------------------------------------------------------------------------
// block reduction helpers (wave64 shuffles, then LDS across the 4 waves of a 256-thread block)
// ---------------------------------------------------------------------------------------------
// wave64 sum by shuffles (fixed order)
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// wave64 sum without the LDS crossbar: inclusive scan inside every row of 16 lanes (row_shr 1, 2, 4, 8), then
// row_bcast15 / row_bcast31 carry the row totals forward; lane 63 ends up with the sum of all 64 lanes (fixed order)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
    return v + __hiloint2double(hi, lo); // lanes without a source (or masked rows) add +0.0
}

__device__ __forceinline__ double wave_sum_dpp(double v) // result in lane 63
{
    v = dpp_add<0x111, 0xf>(v); // row_shr:1
    v = dpp_add<0x112, 0xf>(v); // row_shr:2
    v = dpp_add<0x114, 0xf>(v); // row_shr:4
    v = dpp_add<0x118, 0xf>(v); // row_shr:8
    v = dpp_add<0x142, 0xa>(v); // row_bcast:15 into rows 1 and 3
    v = dpp_add<0x143, 0xc>(v); // row_bcast:31 into rows 2 and 3
    return v;
}

__device__ __forceinline__ double block_sum(double v, double *lds4)
{
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) lds4[wave] = v;
    __syncthreads();
    double s = 0.;
    if (threadIdx.x == 0) s = ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
    return s; // valid in thread 0
}

// two block sums through ONE barrier, each formed exactly as block_sum forms it (wave_sum, then ((w0 + w1) + w2) + w3); every thread adds
// the four wave sums itself, so both totals are valid in EVERY thread and no broadcast barrier follows.  lds8 must be an array that
// nothing else in the kernel touches: the barrier that block_sum takes before its stores only guards a reused array.
__device__ __forceinline__ void block_sum2(double &a, double &b, double *lds8)
{
    a = wave_sum(a);
    b = wave_sum(b);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        lds8[wave] = a;
        lds8[4 + wave] = b;
    }
    __syncthreads();
    a = ((lds8[0] + lds8[1]) + lds8[2]) + lds8[3];
    b = ((lds8[4] + lds8[5]) + lds8[6]) + lds8[7];
}

// matrix words of the value-indexed kernels: non-temporal when the matrix is larger than the caches can hold between two products (the
// read-once stream must not evict x from L2), plain when it may stay in the 256 MB Infinity Cache from one iteration to the next
template <bool KEEP, typename T>
__device__ __forceinline__ T stream_load_k(const T *p)
{
    if (KEEP) return *p;
    return __builtin_nontemporal_load(p);
}
template <bool KEEP, typename T>
__device__ __forceinline__ void stream_store_k(T v, T *p)
{
    if (KEEP) *p = v;
    else __builtin_nontemporal_store(v, p);
}
// (the choice is a TEMPLATE parameter: with a run-time flag the optimiser merges the plain and the hinted load of one address into one
// plain load and the hint is gone)
template <bool NT, typename T>
__device__ __forceinline__ T stream_load(const T *p)
{
    if (NT) return __builtin_nontemporal_load(p); // read once: do not let the stream evict x from L2
    return *p;
}

} // namespace avs
