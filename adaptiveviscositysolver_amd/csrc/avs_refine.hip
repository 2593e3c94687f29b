// avs_refine.hip -- the refinement flags of the pre-pass (avs_prepass_set_refinement / avs_prepass_get_refinement, include/avs.h):
//   k_refine_seeds    indicator > threshold on the simulation grid -> the bit lattice of the octree grid (avs_refine.hpp), one coalesced
//                     read of the field: a wave's 64 consecutive x cells give two words through the wave ballot
//   k_refine_dilate_x / k_refine_dilate_rows   box dilation on the words, one axis per pass: along x shifts with the carries of the two
//                     neighbouring words, along y and z the OR of the 2 d + 1 rows; every pass clips at the simulation grid, so the
//                     three passes give the box dilation clipped there exactly
//   k_refine_expand   bits -> 0 / 1 bytes (the getter)
// The mask kernel that reads the bits stays with the pre-pass (k_mask_labels, avs_prepass.hip).  All counts are integer sums: their order
// does not matter.
#include "avs_refine.hpp"

namespace avs {

static constexpr int kRefBlock = 256;
static constexpr int kRefWaves = kRefBlock / 64;
static constexpr int kSeedBatch = 8; // 64-cell segments a wave has in flight: eight 256-B loads issued before the first ballot

// (the octree grid is a power of two per axis -- avs_prepass_create -- so every index splits by shifts: a 64-bit division per cell made
// the seed kernel compute-bound at a third of the HBM rate)
struct RefineGrid {
    int sim[3], oct[3];
    int wx, lg_wx;     // words per x row
    int nseg, lg_nseg; // 64-cell segments per x row
    int lg_nx, lg_ny;
};

__device__ __forceinline__ int wave_sum_i32(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v; // lane 0
}

// One wave per 64 consecutive x cells of one (y, z) row of the OCTREE lattice; lanes past field_nx and rows outside the simulation grid
// contribute 0, so every word of the lattice is written (no memset) and a row shorter than a word (nx = 16) is one word with its upper
// bits clear.
__global__ __launch_bounds__(kRefBlock) void k_refine_seeds(const float *__restrict__ indicator, RefineGrid G, float threshold,
                                                            uint32_t *__restrict__ bits, unsigned long long *__restrict__ counters)
{
    const int lane = threadIdx.x & 63;
    const size_t tasks = (size_t)G.nseg << (G.lg_ny + __builtin_ctz(G.oct[2]));
    const size_t stride = (size_t)gridDim.x * kRefWaves * kSeedBatch;
    // the words of consecutive segments are consecutive in memory (wx == 2 nseg; one word per row below 64 cells): lane l of the first
    // 8 or 16 stores word l of the batch -- one 32- or 64-B store instead of eight of two lanes each
    const int per = G.wx == 2 * G.nseg ? 2 : 1;
    const int my_u = per == 2 ? lane >> 1 : lane, my_half = per == 2 ? lane & 1 : 0;
    int seeds = 0; // (wave-uniform; < 2^31: a wave meets tasks / waves segments of 64 cells)
    for (size_t t0 = ((size_t)blockIdx.x * kRefWaves + (threadIdx.x >> 6)) * kSeedBatch; t0 < tasks; t0 += stride) {
        float v[kSeedBatch];
#pragma unroll
        for (int u = 0; u < kSeedBatch; ++u) {
            const size_t t = t0 + u;
            const int seg = (int)(t & (size_t)(G.nseg - 1));
            const size_t row = t >> G.lg_nseg;
            const int j = (int)(row & (size_t)(G.oct[1] - 1)), k = (int)(row >> G.lg_ny), x = seg * 64 + lane;
            const bool in = t < tasks && x < G.sim[0] && j < G.sim[1] && k < G.sim[2];
            // (outside the simulation grid: NaN, never a seed whatever the threshold)
            v[u] = in ? indicator[(size_t)x + (size_t)G.sim[0] * ((size_t)j + (size_t)G.sim[1] * (size_t)k)] : __builtin_nanf("");
        }
        uint32_t word = 0u;
#pragma unroll
        for (int u = 0; u < kSeedBatch; ++u) {
            const unsigned long long b = __ballot(v[u] > threshold); // strict float compare: NaN never marks, +inf does
            seeds += __popcll(b);
            if (my_u == u) word = my_half ? (uint32_t)(b >> 32) : (uint32_t)b;
        }
        if (my_u < kSeedBatch && t0 + my_u < tasks) bits[(t0 + my_u) * per + my_half] = word;
    }
    if (lane == 0 && seeds) atomicAdd(&counters[0], (unsigned long long)seeds);
}

// bits of word w of an x row that lie inside the simulation grid
__device__ __forceinline__ uint32_t sim_word_mask(int w, int sim_nx)
{
    const int left = sim_nx - w * 32;
    return left >= 32 ? 0xffffffffu : (left <= 0 ? 0u : (1u << left) - 1u);
}

// x: bit i of the result = OR of the bits i - d .. i + d of the row (d <= 16 < 32: the two neighbouring words carry everything)
__global__ __launch_bounds__(kRefBlock) void k_refine_dilate_x(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, RefineGrid G, int d)
{
    const size_t words = (size_t)G.wx * G.oct[1] * G.oct[2];
    for (size_t t = (size_t)blockIdx.x * kRefBlock + threadIdx.x; t < words; t += (size_t)gridDim.x * kRefBlock) {
        const int w = (int)(t & (size_t)(G.wx - 1));
        const uint32_t cur = in[t], prev = w > 0 ? in[t - 1] : 0u, next = w + 1 < G.wx ? in[t + 1] : 0u;
        const unsigned long long up = ((unsigned long long)cur << 32) | prev, down = ((unsigned long long)next << 32) | cur;
        unsigned long long ru = up, rd = down;
        for (int s = 1; s <= d; ++s) {
            ru |= up << s;
            rd |= down >> s;
        }
        out[t] = ((uint32_t)(ru >> 32) | (uint32_t)rd) & sim_word_mask(w, G.sim[0]);
    }
}

// y (AXIS 1) or z (AXIS 2): word (w, j, k) = OR of the words of the rows within d along the axis, clipped at the simulation grid (rows
// outside it stay 0).  count: the set bits of the result go to counters[1] -- one atomic per wave.
template <int AXIS>
__global__ __launch_bounds__(kRefBlock) void k_refine_dilate_rows(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, RefineGrid G, int d, int count,
                                                                  unsigned long long *__restrict__ counters)
{
    const size_t words = (size_t)G.wx * G.oct[1] * G.oct[2];
    const size_t pitch = AXIS == 1 ? (size_t)G.wx : (size_t)G.wx * G.oct[1];
    int set = 0;
    for (size_t t0 = (size_t)blockIdx.x * kRefBlock; t0 < words; t0 += (size_t)gridDim.x * kRefBlock) { // (whole waves stay for the sum)
        const size_t t = t0 + threadIdx.x;
        if (t >= words) continue;
        const size_t row = t >> G.lg_wx;
        const int c = AXIS == 1 ? (int)(row & (size_t)(G.oct[1] - 1)) : (int)(row >> G.lg_ny);
        uint32_t r = 0u;
        if (c < G.sim[AXIS]) {
            const int lo = c - d < 0 ? 0 : c - d, hi = c + d > G.sim[AXIS] - 1 ? G.sim[AXIS] - 1 : c + d;
            const uint32_t *src = in + (t - (size_t)c * pitch);
            for (int q = lo; q <= hi; q += 4) { // four rows in flight (one load at a time left the pass waiting on latency)
                uint32_t a[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) a[u] = q + u <= hi ? src[(size_t)(q + u) * pitch] : 0u;
                r |= (a[0] | a[1]) | (a[2] | a[3]);
            }
        }
        out[t] = r;
        set += __popc(r);
    }
    if (count) {
        set = wave_sum_i32(set);
        if ((threadIdx.x & 63) == 0 && set) atomicAdd(&counters[1], (unsigned long long)set);
    }
}

__global__ __launch_bounds__(kRefBlock) void k_refine_expand(const uint32_t *__restrict__ bits, RefineGrid G, int8_t *__restrict__ flags)
{
    const size_t cells = (size_t)G.oct[0] * G.oct[1] * G.oct[2];
    for (size_t t = (size_t)blockIdx.x * kRefBlock + threadIdx.x; t < cells; t += (size_t)gridDim.x * kRefBlock) {
        const int i = (int)(t & (size_t)(G.oct[0] - 1));
        const size_t row = t >> G.lg_nx;
        flags[t] = (int8_t)((bits[row * G.wx + (i >> 5)] >> (i & 31)) & 1u);
    }
}

static RefineGrid refine_grid(const int sim[3], const int oct[3])
{
    RefineGrid G;
    for (int a = 0; a < 3; ++a) {
        G.sim[a] = sim[a];
        G.oct[a] = oct[a];
    }
    auto lg = [](int v) { int l = 0; while ((1 << (l + 1)) <= v) ++l; return l; };
    G.wx = refine_row_words(oct[0]);
    G.nseg = (oct[0] + 63) / 64;
    G.lg_wx = lg(G.wx);
    G.lg_nseg = lg(G.nseg);
    G.lg_nx = lg(oct[0]);
    G.lg_ny = lg(oct[1]);
    return G;
}

static unsigned refine_blocks(size_t threads, unsigned cap)
{
    size_t b = (threads + kRefBlock - 1) / kRefBlock;
    if (b < 1) b = 1;
    return (unsigned)(b > cap ? cap : b);
}

avs_status refine_set(RefineState &S, const float *indicator, const int sim[3], const int oct[3], float threshold, int dilate, hipStream_t st)
{
    const RefineGrid G = refine_grid(sim, oct);
    const size_t words = (size_t)G.wx * oct[1] * oct[2];
    const size_t tasks = (size_t)G.nseg * oct[1] * oct[2];
    AVS_TRY(S.bits.alloc(words));
    if (dilate > 0) AVS_TRY(S.tmp.alloc(words));
    AVS_TRY(S.counters.reserve(kRefineCounters));
    S.active = false; // (until the new flags are complete)
    S.wx = G.wx;
    hipEvent_t ev[2] = {nullptr, nullptr};
    AVS_HIP(hipEventCreate(&ev[0]));
    if (hipEventCreate(&ev[1]) != hipSuccess) {
        (void)hipEventDestroy(ev[0]);
        set_error("hipEventCreate failed");
        return AVS_EHIP;
    }
    auto run = [&]() -> avs_status {
        AVS_HIP(hipMemsetAsync(S.counters.p, 0, 2 * sizeof(unsigned long long), st));
        AVS_HIP(hipEventRecord(ev[0], st));
        // pure streaming (4 B read per cell, a bit written): eight workgroups per CU walk the lattice
        hipLaunchKernelGGL(k_refine_seeds, dim3(refine_blocks((tasks + kSeedBatch - 1) / kSeedBatch * 64, 2048)), dim3(kRefBlock), 0, st, indicator, G, threshold,
                           S.bits.p, S.counters.p);
        if (dilate > 0) {
            const unsigned gb = refine_blocks(words, 4096);
            hipLaunchKernelGGL(k_refine_dilate_x, dim3(gb), dim3(kRefBlock), 0, st, (const uint32_t *)S.bits.p, S.tmp.p, G, dilate);
            hipLaunchKernelGGL(k_refine_dilate_rows<1>, dim3(gb), dim3(kRefBlock), 0, st, (const uint32_t *)S.tmp.p, S.bits.p, G, dilate, 0, S.counters.p);
            hipLaunchKernelGGL(k_refine_dilate_rows<2>, dim3(gb), dim3(kRefBlock), 0, st, (const uint32_t *)S.bits.p, S.tmp.p, G, dilate, 1, S.counters.p);
        }
        AVS_HIP(hipGetLastError());
        AVS_HIP(hipEventRecord(ev[1], st));
        unsigned long long h[2] = {0, 0};
        AVS_HIP(hipMemcpyAsync(h, S.counters.p, sizeof(h), hipMemcpyDeviceToHost, st));
        AVS_HIP(hipStreamSynchronize(st));
        float ms = 0.f;
        AVS_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        if (dilate > 0) swap(S.bits, S.tmp); // the third pass wrote tmp
        S.seeds = (int64_t)h[0];
        S.flagged = dilate > 0 ? (int64_t)h[1] : (int64_t)h[0];
        S.set_ms = ms;
        return AVS_OK;
    };
    const avs_status rs = run();
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
    AVS_TRY(rs);
    S.threshold = threshold;
    S.dilate = dilate;
    S.active = true;
    return AVS_OK;
}

avs_status refine_expand(const RefineState &S, const int oct[3], int8_t *flags, hipStream_t st)
{
    const size_t cells = (size_t)oct[0] * oct[1] * oct[2];
    if (!S.active) {
        AVS_HIP(hipMemsetAsync(flags, 0, cells, st));
        return AVS_OK;
    }
    const int sim[3] = {0, 0, 0}; // (the bits are already clipped)
    hipLaunchKernelGGL(k_refine_expand, dim3(refine_blocks(cells, 1u << 16)), dim3(kRefBlock), 0, st, (const uint32_t *)S.bits.p, refine_grid(sim, oct), flags);
    AVS_HIP(hipGetLastError());
    return AVS_OK;
}

} // namespace avs
