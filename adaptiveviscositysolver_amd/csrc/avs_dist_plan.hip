// avs_dist_plan.hip -- the partition planners of the multi-GPU layer (avs_dist.hip is the transport): a rank's plan and local system, built
// on the device.  Entries: plan_on_device (avs_dist_partition; plan_on_host is its independent reference), dist_assemble_device and
// dist_assemble_window (avs_dist_assemble: replicated indices / a slab-local pre-pass).  Their cores, plan_from_source and
// dist_tail_from_rows, work on plain arrays and share every common step in one copy; avs_dist_plan_probe runs them on a caller's arrays.
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>

#include "avs_dist_internal.hpp"

namespace avs {

// ---------------------------------------------------------------------------------------------
// Device-side partition planner: the same plan avs_partition.cpp builds on the host (slabs on multiples of
// 2^(levels-1) fine cells balanced by non-zeros, local numbering [owned ascending | halo grouped by owner,
// ascending], ascending send lists), but from the CSR that already lives in HBM: flag + exclusive scan +
// scatter, one pass over the rows for the halo / "needed by" marks.  Only O(planes) + O(world) scalars visit
// the host.  AVS_DIST_PLAN=host selects the host planner (tests compare the two array for array).
// ---------------------------------------------------------------------------------------------
constexpr int kPlanLdsPlanes = 2048;

__device__ __forceinline__ int plane_of_dof(const int32_t *__restrict__ vdof, int64_t src, int axis, int extent, int shift)
{
    const int32_t *t = vdof + 4 * src;
    const int level = t[0] & 0xff;
    int64_t pos = (int64_t)t[1 + axis] << level;
    if (pos >= extent) pos = extent - 1;
    return (int)(pos >> shift);
}

// plane of every row + per-plane weights (non-zeros + 2 per row, as the host planner); row i stands for the DOF perm[i] (null: i).  `w` is
// the row pointer of the assembled rows, or (kRawCount: nothing is assembled yet) the raw triplet count of every DOF
template <bool kRawCount>
__global__ __launch_bounds__(256) void k_plan_planes(int64_t n, const int32_t *__restrict__ vdof, const int32_t *__restrict__ perm,
                                                     const int32_t *__restrict__ w, int axis, int extent, int shift,
                                                     int nplanes, uint16_t *__restrict__ plane, unsigned long long *__restrict__ weight)
{
    __shared__ unsigned long long h[kPlanLdsPlanes];
    const bool lds = nplanes <= kPlanLdsPlanes;
    if (lds) {
        for (int i = threadIdx.x; i < nplanes; i += 256) h[i] = 0ull;
        __syncthreads();
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t dof = perm ? perm[i] : i;
        const int pl = plane_of_dof(vdof, dof, axis, extent, shift);
        plane[i] = (uint16_t)pl;
        atomicAdd(lds ? &h[pl] : &weight[pl], (unsigned long long)(kRawCount ? w[dof] : w[i + 1] - w[i]) + 2ull);
    }
    if (lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < nplanes; i += 256)
            if (h[i]) atomicAdd(&weight[i], h[i]);
    }
}

__global__ __launch_bounds__(256) void k_plan_owner(int64_t n, const uint16_t *__restrict__ plane, const int32_t *__restrict__ plane_owner,
                                                    int rank, uint8_t *__restrict__ owner, int32_t *__restrict__ own_flag)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int q = plane_owner[plane[i]];
    owner[i] = (uint8_t)q;
    own_flag[i] = q == rank;
}

// one pass over all rows: my rows mark the foreign columns they read (halo), foreign rows mark which of my
// columns their owner needs (bit q)
__global__ __launch_bounds__(256) void k_plan_mark(int64_t n, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                   const uint8_t *__restrict__ owner, int rank, uint8_t *__restrict__ is_halo,
                                                   uint32_t *__restrict__ needed_by)
{
    const int sub = threadIdx.x & 15;
    const int64_t group = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int64_t ngroups = ((int64_t)gridDim.x * 256) >> 4;
    for (int64_t r = group; r < n; r += ngroups) {
        const int q = owner[r];
        const int s = row_ptr[r], e = row_ptr[r + 1];
        for (int k = s + sub; k < e; k += 16) {
            const int32_t c = col[k];
            const int oc = owner[c];
            if (q == rank) {
                if (oc != rank) is_halo[c] = 1; // same value from every writer
            } else if (oc == rank) {
                const uint32_t bit = 1u << q;
                if (!(needed_by[c] & bit)) atomicOr(&needed_by[c], bit);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_plan_flag_halo(int64_t n, const uint8_t *__restrict__ is_halo, const uint8_t *__restrict__ owner,
                                                        int q, int32_t *__restrict__ f, const int32_t *__restrict__ dom = nullptr)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t id = dom ? dom[i] : i;
    f[i] = is_halo[id] && owner[id] == q;
}

__global__ __launch_bounds__(256) void k_plan_flag_send(int64_t n, const uint8_t *__restrict__ owner, int rank,
                                                        const uint32_t *__restrict__ needed_by, int q, int32_t *__restrict__ f)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) f[i] = owner[i] == rank && ((needed_by[i] >> q) & 1u);
}

// flagged i -> out[pos[i]] = (map ? map[i] : i); g2l[i] = base + pos[i] when g2l is given
__global__ __launch_bounds__(256) void k_plan_scatter(int64_t n, const int32_t *__restrict__ f, const int32_t *__restrict__ pos,
                                                      const int32_t *__restrict__ map, int32_t *__restrict__ out,
                                                      int32_t *__restrict__ g2l, int32_t base, const int32_t *__restrict__ dom = nullptr)
{
    // dom (slab-local assembly): entry i stands for the id dom[i] (the window's DOFs in brick-major order) instead of for i itself
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !f[i]) return;
    const int32_t id = dom ? dom[i] : (int32_t)i;
    out[pos[i]] = map ? map[i] : id;
    if (g2l) g2l[id] = base + pos[i];
}

__global__ __launch_bounds__(256) void k_plan_local_len(int64_t n_own, const int32_t *__restrict__ own_global,
                                                        const int32_t *__restrict__ row_ptr, int32_t *__restrict__ len)
{
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l > n_own) return;
    len[l] = l < n_own ? row_ptr[own_global[l] + 1] - row_ptr[own_global[l]] : 0;
}

// local rows: columns through global -> local, values (and value codes) copied, in-row order unchanged;
// tile_bnd[tile] = 1 when a row of the tile reads a halo column
__global__ __launch_bounds__(256) void k_plan_local_rows(int64_t n_own, const int32_t *__restrict__ own_global,
                                                         const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                         const double *__restrict__ val, const uint16_t *__restrict__ codes,
                                                         const int32_t *__restrict__ g2l, const int32_t *__restrict__ row_ptr_l,
                                                         int32_t *__restrict__ col_l, double *__restrict__ val_l,
                                                         uint16_t *__restrict__ codes_l, int tile_rows, int32_t *__restrict__ tile_bnd)
{
    const int sub = threadIdx.x & 15;
    const int64_t group = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int64_t ngroups = ((int64_t)gridDim.x * 256) >> 4;
    for (int64_t l = group; l < n_own; l += ngroups) {
        const int src = row_ptr[own_global[l]], dst = row_ptr_l[l], len = row_ptr_l[l + 1] - dst;
        bool touches = false;
        for (int k = sub; k < len; k += 16) {
            const int32_t lc = g2l[col[src + k]];
            col_l[dst + k] = lc;
            val_l[dst + k] = val[src + k];
            if (codes) codes_l[dst + k] = codes[src + k];
            touches |= lc >= n_own;
        }
        if (touches) tile_bnd[l / tile_rows] = 1;
    }
}

__global__ __launch_bounds__(256) void k_plan_not(int64_t n, const int32_t *__restrict__ f, int32_t *__restrict__ g)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) g[i] = !f[i];
}

// exclusive scan of 0/1 flags + their total (one small read-back)
static avs_status scan_flags(const int32_t *f, int32_t *pos, int64_t n, DevBuf<int32_t> &tmp, int64_t *total, hipStream_t st)
{
    *total = 0;
    if (n == 0) return AVS_OK;
    AVS_TRY(exclusive_scan_i32(f, pos, n, tmp.p, tmp.n, st));
    int32_t last[2] = {0, 0};
    AVS_HIP(hipMemcpyAsync(&last[0], pos + (n - 1), 4, hipMemcpyDeviceToHost, st));
    AVS_HIP(hipMemcpyAsync(&last[1], f + (n - 1), 4, hipMemcpyDeviceToHost, st));
    AVS_HIP(hipStreamSynchronize(st));
    *total = (int64_t)last[0] + last[1];
    return AVS_OK;
}

// Guard words behind the arrays the planners fill.  The probe build (avs_dist_plan_probe) hands the planner cores a PlanGuards: plan_buf then
// allocates every array with kBytes of a known pattern behind its last entry, and the core counts the altered bytes before it returns.  The
// product passes null: plan_buf is DevBuf::alloc / DevBuf::reserve and nothing else, so what the product allocates does not change.
struct PlanGuards {
#ifdef AVS_PROBES
    static constexpr size_t kBytes = 64;
    static constexpr int kPattern = 0xA5;
    static constexpr int kMaxSpans = 96;
    const uint8_t *at[kMaxSpans];
    size_t bytes[kMaxSpans];
    int spans = 0;
    int64_t hit = 0;
#endif
};
#ifdef AVS_PROBES
static avs_status plan_guard_add(PlanGuards *g, const void *p, size_t bytes, hipStream_t st)
{
    AVS_REQUIRE(g->spans < PlanGuards::kMaxSpans, AVS_EINTERNAL, "too many guarded arrays");
    AVS_HIP(hipMemsetAsync(const_cast<void *>(p), PlanGuards::kPattern, bytes, st));
    g->at[g->spans] = static_cast<const uint8_t *>(p);
    g->bytes[g->spans++] = bytes;
    return AVS_OK;
}
// an array is about to be freed: its guard can no longer be read
static void plan_guard_drop(PlanGuards *g, const void *p, size_t bytes)
{
    const uint8_t *lo = static_cast<const uint8_t *>(p);
    int k = 0;
    for (int i = 0; i < g->spans; ++i)
        if (!p || g->at[i] < lo || g->at[i] >= lo + bytes) { g->at[k] = g->at[i]; g->bytes[k++] = g->bytes[i]; }
    g->spans = k;
}
// counts the guard bytes that no longer hold the pattern (the stream is idle afterwards) and forgets the spans
static avs_status plan_guard_check(PlanGuards *g, hipStream_t st)
{
    AVS_HIP(hipStreamSynchronize(st));
    uint8_t h[PlanGuards::kBytes + 16];
    for (int i = 0; i < g->spans; ++i) {
        AVS_HIP(hipMemcpy(h, g->at[i], g->bytes[i], hipMemcpyDeviceToHost));
        for (size_t b = 0; b < g->bytes[i]; ++b) g->hit += h[b] != (uint8_t)PlanGuards::kPattern;
    }
    g->spans = 0;
    return AVS_OK;
}
#endif
// `count` entries of `b`: DevBuf::reserve (`keep`: scratch kept across frames) or DevBuf::alloc; with guards, exactly count entries + the guard
template <typename T>
static avs_status plan_buf(PlanGuards *g, DevBuf<T> &b, size_t count, bool keep, hipStream_t st)
{
#ifdef AVS_PROBES
    if (g) {
        const size_t extra = (PlanGuards::kBytes + sizeof(T) - 1) / sizeof(T);
        if (b.p) plan_guard_drop(g, b.p, b.n * sizeof(T));
        b.release();
        AVS_TRY(b.alloc(count + extra));
        return plan_guard_add(g, b.p + count, extra * sizeof(T), st);
    }
#endif
    (void)g;
    (void)st;
    return keep ? b.reserve(count) : b.alloc(count);
}

// What the device planner reads, as plain arrays (device pointers): a CSR of n rows whose columns lie in [0, n), one dof record per DOF
// (level | axis << 8, i, j, k), perm (row i stands for the DOF perm[i]; null: identity) and the cut geometry.  Rank and world are d's.
struct PlanSource {
    int64_t n = 0;
    const int32_t *row_ptr = nullptr, *col = nullptr;
    const double *val = nullptr;
    const int32_t *vdof = nullptr, *perm = nullptr;
    int levels = 1, cut_axis = 0, extent = 1;
    hipStream_t stream = nullptr;
    struct PlanKeep *keep = nullptr; // null (the product): the intermediate results below are scratch
};
// intermediate results a caller may ask the cores to keep (avs_dist_plan_probe) + the guard words of that run
struct PlanKeep {
    std::vector<int64_t> weight;   // per plane
    std::vector<int> plane_owner;
    DevBuf<uint8_t> owner;         // per row
    DevBuf<int32_t> halo;          // the halo ids, grouped by owner, ascending inside a group (n_halo entries)
    int64_t n_interior = -1;       // the tail's row split: rows that read no other rank (-1: not split)
    PlanGuards guards;
};

// The steps the planner cores share, each in one copy: plan_from_source and dist_tail_from_rows are lists of these plus what is their own.

// the assembly's plane size (2^shift fine cells): levels - 1, capped at 2, AVS_DIST_PLANE_SHIFT overrides -- why: dist_assemble_device
static int plane_shift(int levels)
{
    const int top = levels - 1, asked = cur_opt().dist_plane_shift;
    return std::min(top, asked >= 0 ? asked : 2);
}

// host, O(planes): per-plane weights -> the rank that owns every plane (greedy cuts, as the host planner)
static std::vector<int> plane_owners(const std::vector<int64_t> &w, int world)
{
    std::vector<int> po(w.size());
    plane_owners_from_weights(w.data(), (int)w.size(), world, po.data());
    return po;
}

// slabs: per-plane weights -> host (h_w) -> the planes' owners (h_po) -> plane_owner -> owner of every row and its own flag
static avs_status owners_from_weights(const unsigned long long *weight, int nplanes, int world, int rank, int64_t n, const uint16_t *plane, int32_t *plane_owner,
                                      uint8_t *owner, int32_t *own_flag, std::vector<int64_t> &h_w, std::vector<int> &h_po, hipStream_t st)
{
    std::vector<unsigned long long> w((size_t)nplanes);
    AVS_HIP(hipMemcpyAsync(w.data(), weight, w.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    AVS_HIP(hipStreamSynchronize(st));
    h_w.assign(w.begin(), w.end());
    h_po = plane_owners(h_w, world);
    AVS_HIP(hipMemcpyAsync(plane_owner, h_po.data(), h_po.size() * sizeof(int), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_plan_owner, dim3(grid256(n)), dim3(256), 0, st, n, plane, (const int32_t *)plane_owner, rank, owner, own_flag);
    return AVS_OK;
}

// what a per-peer pass works with: 0/1 flags, their exclusive scan (as many entries as the longest pass + 1) and the scan's work array
struct PlanPass {
    int rank, world;
    int32_t *flag, *pos;
    DevBuf<int32_t> &scan_tmp;
    PlanGuards *G;
    hipStream_t st;
    // what the steps count, per rank and in all: finish_plan alone writes PcgDist's sizes and peer table, all of them at the end
    std::vector<int64_t> recv_cnt, send_cnt;
    int64_t n_halo = 0, n_send = 0;
    int n_tiles_int = 0, n_tiles_bnd = 0;
};

// Halo numbering: peer after peer of `mask`, the halo columns among the n candidates (dom[i]; null: i) that q owns get the next local ids
// behind the n_own owned rows, ascending: g2l, p.recv_cnt[q], p.n_halo.  The ids are only needed to number them: every peer's scatter starts
// at 0 of halo_ids unless the caller keeps the list.  One scan + host round trip per peer of the mask.
static avs_status number_halo(PlanPass &p, uint32_t mask, int64_t n, const int32_t *dom, const uint8_t *is_halo, const uint8_t *owner, int64_t n_own,
                              int32_t *g2l, int32_t *halo_ids, bool keep_ids)
{
    p.recv_cnt.assign((size_t)p.world, 0);
    for (int q = 0; q < p.world; ++q) {
        if (q == p.rank || !((mask >> q) & 1u)) continue;
        hipLaunchKernelGGL(k_plan_flag_halo, dim3(grid256(n)), dim3(256), 0, p.st, n, is_halo, owner, q, p.flag, dom);
        AVS_TRY(scan_flags(p.flag, p.pos, n, p.scan_tmp, &p.recv_cnt[(size_t)q], p.st));
        if (p.recv_cnt[(size_t)q]) hipLaunchKernelGGL(k_plan_scatter, dim3(grid256(n)), dim3(256), 0, p.st, n, p.flag, p.pos, (const int32_t *)nullptr,
                                                      halo_ids + (keep_ids ? p.n_halo : 0), g2l, (int32_t)(n_own + p.n_halo), dom);
        p.n_halo += p.recv_cnt[(size_t)q];
    }
    return AVS_OK;
}

// Send lists: per peer q of `mask`, the rows among n_rows that flag_send(q) flags (it launches the kernel that fills p.flag), ascending, as
// local DOF ids (map[row]; null: the row index is the id): p.send_cnt[q], p.n_send.  A counting pass (one scan + host round trip per peer),
// ONE allocation of send_idx / sendbuf (`keep`: kept across frames), a filling pass over the peers that get entries.
template <typename FlagSend>
static avs_status build_send_lists(PcgDist *d, PlanPass &p, uint32_t mask, int64_t n_rows, FlagSend flag_send, const int32_t *map, bool keep)
{
    p.send_cnt.assign((size_t)p.world, 0);
    for (int q = 0; q < p.world; ++q) {
        if (q == p.rank || !((mask >> q) & 1u)) continue;
        flag_send(q);
        AVS_TRY(scan_flags(p.flag, p.pos, n_rows, p.scan_tmp, &p.send_cnt[(size_t)q], p.st));
        p.n_send += p.send_cnt[(size_t)q];
    }
    AVS_TRY(plan_buf(p.G, d->send_idx, (size_t)p.n_send, keep, p.st));
    AVS_TRY(plan_buf(p.G, d->sendbuf, (size_t)p.n_send, keep, p.st));
    int64_t off = 0;
    for (int q = 0; q < p.world; ++q) {
        if (q == p.rank || !p.send_cnt[(size_t)q]) continue;
        flag_send(q);
        AVS_TRY(exclusive_scan_i32(p.flag, p.pos, n_rows, p.scan_tmp.p, p.scan_tmp.n, p.st));
        hipLaunchKernelGGL(k_plan_scatter, dim3(grid256(n_rows)), dim3(256), 0, p.st, n_rows, p.flag, p.pos, map, d->send_idx.p + off,
                           (int32_t *)nullptr, 0);
        off += p.send_cnt[(size_t)q];
    }
    return AVS_OK;
}

// Tile lists for the overlap of the exchange with the interior rows: the tiles with tile_bnd set (a row reads a halo column) and the others,
// both ascending.  tile_int and tile_pos are scratch of ntiles + 1 entries.
static avs_status build_tile_lists(PcgDist *d, PlanPass &p, int64_t ntiles, const int32_t *tile_bnd, int32_t *tile_int, int32_t *tile_pos, bool keep)
{
    auto list = [&](const int32_t *f, DevBuf<int32_t> &out, int *count) -> avs_status {
        int64_t m = 0;
        AVS_TRY(scan_flags(f, tile_pos, ntiles, p.scan_tmp, &m, p.st));
        AVS_TRY(plan_buf(p.G, out, (size_t)m, keep, p.st));
        if (m) hipLaunchKernelGGL(k_plan_scatter, dim3(grid256(ntiles)), dim3(256), 0, p.st, ntiles, f, tile_pos, (const int32_t *)nullptr, out.p, (int32_t *)nullptr, 0);
        *count = (int)m;
        return AVS_OK;
    };
    AVS_TRY(list(tile_bnd, d->tiles_bnd, &p.n_tiles_bnd));
    if (ntiles) hipLaunchKernelGGL(k_plan_not, dim3(grid256(ntiles)), dim3(256), 0, p.st, ntiles, tile_bnd, tile_int);
    return list(tile_int, d->tiles_int, &p.n_tiles_int);
}

// The cores' last step, the one closing block: the launches are checked, the stream is drained (temporaries die here), the guard bytes are
// counted; then the peer table (every other rank with a send or a receive count, ascending) and the six sizes are written, together.
static avs_status finish_plan(PcgDist *d, const PlanPass &p, int64_t n_own, int64_t nnz_local)
{
    AVS_HIP(hipGetLastError());
    AVS_HIP(hipStreamSynchronize(p.st));
#ifdef AVS_PROBES
    if (p.G) AVS_TRY(plan_guard_check(p.G, p.st));
#endif
    d->peers.clear();
    d->send_counts.clear();
    d->recv_counts.clear();
    for (int q = 0; q < p.world; ++q)
        if (q != p.rank && (p.send_cnt[(size_t)q] || p.recv_cnt[(size_t)q])) {
            d->peers.push_back(q);
            d->send_counts.push_back((int32_t)p.send_cnt[(size_t)q]);
            d->recv_counts.push_back((int32_t)p.recv_cnt[(size_t)q]);
        }
    d->n_tiles_int = p.n_tiles_int;
    d->n_tiles_bnd = p.n_tiles_bnd;
    d->n_own = n_own;
    d->n_halo = p.n_halo;
    d->n_send = p.n_send;
    d->nnz_local = nnz_local;
    return AVS_OK;
}

// fills the plan and the local system of `d` (its rank of its world) from the system in `s`
static avs_status plan_from_source(PcgDist *d, const PlanSource &s)
{
    hipStream_t st = s.stream;
    const int64_t n = s.n;
    const int rank = d->rank, world = d->world;
    AVS_REQUIRE(world <= 32, AVS_EINVAL, "at most 32 ranks");
    const int32_t *g_rp = s.row_ptr, *g_col = s.col;
    const double *g_val = s.val;
    const int cut_axis = s.cut_axis, extent = s.extent;
    const int shift = s.levels - 1;
    const int nplanes = (extent + (1 << shift) - 1) >> shift;
    AVS_REQUIRE(nplanes <= 65535, AVS_EINVAL, "too many cut planes");
    PlanGuards *G = s.keep ? &s.keep->guards : nullptr;

    DevBuf<uint16_t> plane;
    DevBuf<unsigned long long> weight;
    DevBuf<int32_t> plane_owner, flag, pos, g2l, scan_tmp, halo_scratch;
    DevBuf<uint8_t> owner_scratch, is_halo;
    DevBuf<uint32_t> needed_by;
    DevBuf<uint8_t> &owner = s.keep ? s.keep->owner : owner_scratch;
    DevBuf<int32_t> &halo_tmp = s.keep ? s.keep->halo : halo_scratch;
    AVS_TRY(plan_buf(G, plane, (size_t)n, false, st));
    AVS_TRY(plan_buf(G, weight, (size_t)nplanes, false, st));
    AVS_TRY(plan_buf(G, plane_owner, (size_t)nplanes, false, st));
    AVS_TRY(plan_buf(G, flag, (size_t)n + 1, false, st));
    AVS_TRY(plan_buf(G, pos, (size_t)n + 1, false, st));
    AVS_TRY(plan_buf(G, g2l, (size_t)n, false, st));
    AVS_TRY(plan_buf(G, scan_tmp, scan_tmp_elems(n + 1), false, st));
    AVS_TRY(plan_buf(G, owner, (size_t)n, false, st));
    AVS_TRY(plan_buf(G, is_halo, (size_t)n, false, st));
    AVS_TRY(plan_buf(G, needed_by, (size_t)n, false, st));
    AVS_HIP(hipMemsetAsync(weight.p, 0, (size_t)nplanes * sizeof(unsigned long long), st));
    AVS_HIP(hipMemsetAsync(is_halo.p, 0, (size_t)n, st));
    AVS_HIP(hipMemsetAsync(needed_by.p, 0, (size_t)n * sizeof(uint32_t), st));
    AVS_HIP(hipMemsetAsync(g2l.p, 0xFF, (size_t)n * sizeof(int32_t), st));

    // 1. slabs: per-plane weights -> (host, O(planes)) greedy cuts -> owner of every row
    hipLaunchKernelGGL(k_plan_planes<false>, dim3(2048), dim3(256), 0, st, n, s.vdof, s.perm, g_rp, cut_axis, extent,
                       shift, nplanes, plane.p, weight.p);
    std::vector<int64_t> w_scratch;
    std::vector<int> po_scratch;
    AVS_TRY(owners_from_weights(weight.p, nplanes, world, rank, n, plane.p, plane_owner.p, owner.p, flag.p, s.keep ? s.keep->weight : w_scratch,
                                s.keep ? s.keep->plane_owner : po_scratch, st));
    PlanPass pass{rank, world, flag.p, pos.p, scan_tmp, G, st};

    // 2. owned rows, ascending
    int64_t n_own = 0;
    AVS_TRY(scan_flags(flag.p, pos.p, n, scan_tmp, &n_own, st));
    AVS_TRY(plan_buf(G, d->own_global, (size_t)n_own, false, st));
    hipLaunchKernelGGL(k_plan_scatter, dim3(grid256(n)), dim3(256), 0, st, n, flag.p, pos.p, (const int32_t *)nullptr, d->own_global.p,
                       g2l.p, 0);

    // 3. halo / needed-by marks
    hipLaunchKernelGGL(k_plan_mark, dim3(8192), dim3(256), 0, st, n, g_rp, g_col, owner.p, rank, is_halo.p, needed_by.p);

    // 4. halo numbering (grouped by owner) and send lists (ascending owned entries each peer reads)
    AVS_TRY(plan_buf(G, halo_tmp, (size_t)n, false, st));
    const uint32_t every_rank = ~0u; // (the marks cover the rows of all ranks: no peer mask)
    AVS_TRY(number_halo(pass, every_rank, n, nullptr, is_halo.p, owner.p, n_own, g2l.p, halo_tmp.p, s.keep != nullptr));
    auto flag_send = [&](int q) { hipLaunchKernelGGL(k_plan_flag_send, dim3(grid256(n)), dim3(256), 0, st, n, owner.p, rank, needed_by.p, q, flag.p); };
    AVS_TRY(build_send_lists(d, pass, every_rank, n, flag_send, g2l.p, false));

    // 5. local CSR: k_plan_local_len leaves the n_own row lengths (and a 0 behind them); the scan of n_own inputs writes the n_own + 1 row
    // pointers (out[n_own] = total)
    AVS_TRY(plan_buf(G, d->row_ptr, (size_t)n_own + 1, false, st));
    hipLaunchKernelGGL(k_plan_local_len, dim3(grid256(n_own + 1)), dim3(256), 0, st, n_own, d->own_global.p, g_rp, flag.p);
    AVS_TRY(exclusive_scan_i32(flag.p, d->row_ptr.p, n_own, scan_tmp.p, scan_tmp.n, st));
    int32_t nnz_local = 0;
    AVS_HIP(hipMemcpyAsync(&nnz_local, d->row_ptr.p + n_own, 4, hipMemcpyDeviceToHost, st));
    AVS_HIP(hipStreamSynchronize(st));
    AVS_TRY(plan_buf(G, d->col, (size_t)nnz_local, false, st));
    AVS_TRY(plan_buf(G, d->val, (size_t)nnz_local, false, st));
    const int T = spmv_tile_rows();
    const int64_t ntiles = (n_own + T - 1) / T;
    DevBuf<int32_t> tile_bnd, tile_int, tile_pos;
    AVS_TRY(plan_buf(G, tile_bnd, (size_t)ntiles + 1, false, st));
    AVS_TRY(plan_buf(G, tile_int, (size_t)ntiles + 1, false, st));
    AVS_TRY(plan_buf(G, tile_pos, (size_t)ntiles + 1, false, st));
    AVS_HIP(hipMemsetAsync(tile_bnd.p, 0, ((size_t)ntiles + 1) * 4, st));
    if (n_own)
        hipLaunchKernelGGL(k_plan_local_rows, dim3(8192), dim3(256), 0, st, n_own, d->own_global.p, g_rp, g_col, g_val,
                           (const uint16_t *)nullptr, g2l.p, d->row_ptr.p, d->col.p, d->val.p, (uint16_t *)nullptr, T, tile_bnd.p);

    // 6. tile lists for the overlap of the exchange with the interior rows
    AVS_TRY(build_tile_lists(d, pass, ntiles, tile_bnd.p, tile_int.p, tile_pos.p, false));
    return finish_plan(d, pass, n_own, nnz_local);
}

// the plan of the context's (brick-major when `ro`) system
avs_status plan_on_device(avs_ctx *c, PcgDist *d, int cut_axis, int extent, bool ro)
{
    PlanSource s;
    s.n = c->n_vel;
    s.row_ptr = ro ? c->p_row_ptr.p : c->row_ptr.p;
    s.col = ro ? c->p_col.p : c->col.p;
    s.val = ro ? c->p_val.p : c->val.p; // (the local rows get their own dictionaries afterwards: build_matrix_index)
    s.vdof = c->vdof.p;
    s.perm = ro ? c->perm.p : nullptr;
    s.levels = c->desc.levels;
    s.cut_axis = cut_axis;
    s.extent = extent;
    s.stream = c->stream;
    return plan_from_source(d, s);
}

// ---------------------------------------------------------------------------------------------
// Distributed assembly ("each GPU assembles the rows it owns").  Nothing global is built except what
// is cheap and index-only: dof tables, stencils, restriction, the raw per-row triplet counts (slab weights) and the
// brick-major permutation.  Each rank then assembles ITS rows (assemble_rows), renumbers their columns
// reference id -> brick-major id -> local [owned | halo by owner], and derives its send lists from its own rows:
// the matrix pattern is symmetric (every stress contributes d d^T), so "rank q reads my DOF i" <=> "my row i reads
// a DOF of q".
// ---------------------------------------------------------------------------------------------
// owned rows: columns reference id -> brick-major id (in place); marks halo columns and, per local row, the ranks
// whose DOFs it reads (= the ranks that read this row's DOF)
__global__ __launch_bounds__(256) void k_da_mark(int64_t n_own, const int32_t *__restrict__ row_ptr, int32_t *__restrict__ col,
                                                 const int32_t *__restrict__ inv, const uint8_t *__restrict__ owner, int rank,
                                                 uint8_t *__restrict__ is_halo, uint32_t *__restrict__ needed_by, int *__restrict__ err = nullptr)
{
    // inv == null (slab-local assembly): ids stay the reference's; a column without an owner lies outside the rank's window (err)
    const int sub = threadIdx.x & 15;
    const int64_t group = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int64_t ngroups = ((int64_t)gridDim.x * 256) >> 4;
    for (int64_t l = group; l < n_own; l += ngroups) {
        uint32_t bits = 0u;
        for (int k = row_ptr[l] + sub; k < row_ptr[l + 1]; k += 16) {
            const int32_t cb = inv ? inv[col[k]] : col[k];
            col[k] = cb;
            const int q = owner[cb];
            if (q == 0xFF) {
                if (err) *err = 1;
            } else if (q != rank) {
                is_halo[cb] = 1; // same value from every writer
                bits |= 1u << q;
            }
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) bits |= __shfl_xor(bits, o, 16);
        if (sub == 0) needed_by[l] = bits;
    }
}

// brick-major column ids -> local ids; tile_bnd[tile] = 1 when a row of the tile reads a halo column
__global__ __launch_bounds__(256) void k_da_localize(int64_t n_own, const int32_t *__restrict__ row_ptr, int32_t *__restrict__ col,
                                                     const int32_t *__restrict__ g2l, int tile_rows, int32_t *__restrict__ tile_bnd)
{
    const int sub = threadIdx.x & 15;
    const int64_t group = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int64_t ngroups = ((int64_t)gridDim.x * 256) >> 4;
    for (int64_t l = group; l < n_own; l += ngroups) {
        bool touches = false;
        for (int k = row_ptr[l] + sub; k < row_ptr[l + 1]; k += 16) {
            const int32_t lc = g2l[col[k]];
            col[k] = lc;
            touches |= lc >= n_own;
        }
        if (touches) tile_bnd[l / tile_rows] = 1;
    }
}

// reference DOF id of every halo column: global brick-major id g with a local id >= n_own -> perm[g]
__global__ __launch_bounds__(256) void k_da_halo_ref(int64_t n, const int32_t *__restrict__ g2l, const int32_t *__restrict__ perm, int64_t n_own,
                                                     int32_t *__restrict__ local_ref, const int32_t *__restrict__ dom = nullptr)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t g = dom ? dom[i] : (int32_t)i;
    const int32_t l = g2l[g];
    if (l >= n_own) local_ref[l] = perm ? perm[g] : g;
}

// the ranks this rank exchanges with: the union of the rows' needed_by bits (the pattern is symmetric: whom I read from reads from me)
__global__ __launch_bounds__(256) void k_da_peer_mask(int64_t n_own, const uint32_t *__restrict__ needed_by, uint32_t *__restrict__ mask)
{
    uint32_t m = 0u;
    for (int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x; l < n_own; l += (int64_t)gridDim.x * 256) m |= needed_by[l];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m |= __shfl_xor(m, o, 64);
    if ((threadIdx.x & 63) == 0 && m) atomicOr(mask, m);
}

__global__ __launch_bounds__(256) void k_da_flag_send(int64_t n_own, const uint32_t *__restrict__ needed_by, int q, int32_t *__restrict__ f)
{
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l < n_own) f[l] = q < 0 ? (needed_by[l] == 0u) : ((needed_by[l] >> q) & 1u); // q < 0: rows that read no other rank
}

// local row order [interior | rows that read another rank's DOFs], both parts in ascending brick-major order (stable): the
// halo-touching SpMV tiles shrink from every tile that contains a surface brick (25-57 % of a slab's tiles) to the rows next to
// the cuts (a few per cent), everything else multiplies while the halo travels.  pos_int = exclusive scan of (needed_by == 0).
__global__ __launch_bounds__(256) void k_da_new_index(int64_t n_own, const uint32_t *__restrict__ needed_by, const int32_t *__restrict__ pos_int,
                                                      int64_t n_interior, const int32_t *__restrict__ row_ptr, int32_t *__restrict__ new_of,
                                                      int32_t *__restrict__ len_new)
{
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l > n_own) return;
    if (l == n_own) { len_new[n_own] = 0; return; }
    const int64_t nw = needed_by[l] == 0 ? (int64_t)pos_int[l] : n_interior + (l - pos_int[l]);
    new_of[l] = (int32_t)nw;
    len_new[nw] = row_ptr[l + 1] - row_ptr[l];
}

__global__ __launch_bounds__(256) void k_da_move_rows(int64_t n_own, const int32_t *__restrict__ new_of, const int32_t *__restrict__ row_ptr,
                                                      const int32_t *__restrict__ col, const double *__restrict__ val,
                                                      const int32_t *__restrict__ row_ptr_new, int32_t *__restrict__ col_new,
                                                      double *__restrict__ val_new)
{
    const int sub = threadIdx.x & 15;
    const int64_t group = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int64_t ngroups = ((int64_t)gridDim.x * 256) >> 4;
    for (int64_t l = group; l < n_own; l += ngroups) {
        const int src = row_ptr[l], dst = row_ptr_new[new_of[l]], len = row_ptr[l + 1] - src;
        for (int k = sub; k < len; k += 16) {
            col_new[dst + k] = col[src + k];
            val_new[dst + k] = val[src + k];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_da_move(int64_t n, const int32_t *__restrict__ new_of, const T *__restrict__ src, T *__restrict__ dst)
{
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l < n) dst[new_of[l]] = src[l];
}

__global__ __launch_bounds__(256) void k_da_g2l_own(int64_t n_own, const int32_t *__restrict__ own_global, int32_t *__restrict__ g2l)
{
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l < n_own) g2l[own_global[l]] = (int32_t)l;
}

// the brick-structured form for a rank's local rows: same rule as the single-GPU system (avs_reorder.hip)
static bool dist_brick_wanted(const avs_ctx *c, int64_t n_own)
{
    const int mode = c->opt.brick;
    if (c->brick_shift != 3) return false;
    return mode == 1 || (mode != 0 && n_own >= kBrickMinSystemRows);
}
avs_status dist_build_brick(avs_ctx *c, PcgDist *d)
{
    d->brick.clear();
    d->brick.view(d->brick_view, d->vi);
    if (!dist_brick_wanted(c, d->n_own) || !d->local_ref.p || d->local_ref.n < (size_t)(d->n_own + d->n_halo)) return AVS_OK;
    BrickSource src;
    src.n_rows = d->n_own;
    src.n_cols = d->n_own + d->n_halo;
    src.nnz = d->nnz_local;
    src.row_ptr = d->row_ptr.p;
    src.col = d->col.p;
    src.vi = &d->vi;
    src.val = d->val.p;
    src.vdof = c->vdof.p;
    src.ref_id = d->local_ref.p;
    src.nx = c->desc.nx; src.ny = c->desc.ny; src.nz = c->desc.nz;
    src.levels = c->desc.levels;
    src.brick_shift = c->brick_shift;
    AVS_TRY(build_brick_form(d->brick, src, c->opt, c->stream));
    if (d->brick.ready) {
        const double fill = (double)d->n_own / (double)d->brick.ntiles;
        if (c->opt.brick != 1 && fill < kBrickMinFill) d->brick.release(); // (auto: the word stream serves part-filled tiles better)
        else {
            d->brick.view(d->brick_view, d->vi);
            d->brick_view.walk = fill >= kBrickEighthsFill ? 0 : 1;
            // the float-vector loop launches the float kernel, the mixed-precision loop k_spmv_brick<.., float, double>: the walk is laid out
            // for ITS grid (the fp64 product of the reliable updates follows the plan where its grid is the same, else its strided walk)
            const int view_f32 = d->mixed ? 2 : d->f32 ? 1 : 0;
            d->brick_view.f32 = view_f32;
            if (c->opt.brick_plan) {
                const int walk = d->brick_view.walk;
                AVS_TRY(d->brick.plan_walk(brick_partial_count(d->brick_view), walk, c->opt.brick_cost, c->stream));
                d->brick.view(d->brick_view, d->vi);
                d->brick_view.walk = walk;
                d->brick_view.f32 = view_f32;
            }
            return AVS_OK;
        }
    } else if (c->opt.brick != 1) {
        d->brick.release();
    }
    d->brick.view(d->brick_view, d->vi);
    return AVS_OK;
}

// Everything behind the choice of the owned rows, shared by the replicated-index assembly above and the slab-local one below: the rank's
// rows, halo numbering, send lists, local column ids, tile lists.  Ids live in an id space of `n_ids` entries (brick-major ids / the
// reference's ids); `dom` (null: 0 .. n_dom) lists, in brick-major order, the ids a halo column can have; owner / is_halo / g2l are
// indexed by id.  inv (reference id -> id, null: identity), perm (id -> reference id, null: identity).
// dist_assemble_tail builds the rank's rows and its warm start; everything between the two is dist_tail_from_rows, a function of plain
// arguments (avs_dist_plan_probe runs it on a caller's rows).
//
// The arguments of that core: the rank's n_own rows stand in d->row_ptr / col / val / rhs as assemble_rows leaves them
// (nnz_local entries, columns still in the numbering `inv` reads), d->own_global holds their ids and *ids the reference DOFs behind them;
// g2l already maps the owned ids to 0 .. n_own, is_halo is zero, owner[id] is the id's rank (0xFF: outside the rank's window).  The core
// swaps *ids, like the rows, when it reorders them.  flag and pos hold max(n_own, n_dom) + 1 entries, scan_tmp enough for a scan of as many.
struct TailSource {
    DevBuf<int32_t> *ids = nullptr;
    int64_t n_own = 0, nnz_local = 0;
    const int32_t *dom = nullptr;
    int64_t n_dom = 0;
    const int32_t *inv = nullptr, *perm = nullptr;
    const uint8_t *owner = nullptr;
    uint8_t *is_halo = nullptr;
    int32_t *g2l = nullptr, *flag = nullptr, *pos = nullptr;
    DevBuf<int32_t> *scan_tmp = nullptr;
    bool split = false; // [interior | halo-reading] local row order (rank and world are d's)
    hipStream_t stream = nullptr;
    PlanKeep *keep = nullptr; // null (the product): the halo id list is scratch
};
static avs_status dist_tail_from_rows(PcgDist *d, const TailSource &s);

// PRECONDITION: the caller (dist_assemble_device / dist_assemble_window) has left, in d->ws, ids = the n_own reference DOFs, owner per id, g2l
// with the owned ids set, is_halo zeroed, and flag / pos / scan_tmp reserved for max(n_own, n_dom) + 1 entries; both do so just above their call.
static avs_status dist_assemble_tail(avs_ctx *c, PcgDist *d, int64_t n_own, const int32_t *dom, int64_t n_dom, const int32_t *inv, const int32_t *perm)
{
    hipStream_t st = c->stream;
    DevBuf<int32_t> &ids = d->ws.ids;
    PhaseTrace tr(st, "tail rows", cur_opt().trace_phases != 0);
    // restriction (warm start, also the mass term of the right-hand side) and rows of this rank only;
    // columns still in the reference numbering
    AVS_TRY(build_initial_guess_rows(c, ids.p, n_own));
    tr.mark("initial guess rows");
    int64_t nnz_local = 0;
    AVS_TRY(assemble_rows(c, ids.p, n_own, d->row_ptr, d->col, d->val, d->rhs, &nnz_local, nullptr));
    tr.mark("assemble_rows");
    TailSource s;
    s.ids = &ids;
    s.n_own = n_own;
    s.nnz_local = nnz_local;
    s.dom = dom;
    s.n_dom = n_dom;
    s.inv = inv;
    s.perm = perm;
    s.owner = d->ws.owner.p;
    s.is_halo = d->ws.is_halo.p;
    s.g2l = d->ws.g2l.p;
    s.flag = d->ws.flag.p;
    s.pos = d->ws.pos.p;
    s.scan_tmp = &d->ws.scan_tmp;
    // A slab the brick-structured form will serve keeps the plain ascending (brick-major) row order: its tiles are whole bricks, and the
    // ones that read halo columns are moved to the end of the WALK order instead (build_brick_form), which keeps them full.  With the
    // [interior | halo-reading] split every brick next to a cut would fall into two part-filled tiles.
    s.split = d->world > 1 && cur_opt().dist_split_rows != 0 && !dist_brick_wanted(c, n_own);
    s.stream = st;
    AVS_TRY(dist_tail_from_rows(d, s));
    // warm start of the owned DOFs (in the order the core left the rows in)
    AVS_TRY(d->x0.reserve((size_t)n_own));
    AVS_TRY(d->x.reserve((size_t)n_own));
    if (n_own) hipLaunchKernelGGL(k_gather_i<double>, dim3(grid256(n_own)), dim3(256), 0, st, c->x0.p, ids.p, d->x0.p, n_own);
    AVS_HIP(hipGetLastError());
    AVS_HIP(hipStreamSynchronize(st));
    tr.mark("x0");
    return AVS_OK;
}

// Everything from the rows' marks onward: peer mask, row split, halo numbering, send lists, local column ids, tile lists, local_ref
static avs_status dist_tail_from_rows(PcgDist *d, const TailSource &s)
{
    hipStream_t st = s.stream;
    const int rank = d->rank, world = d->world;
    const int64_t n = s.n_dom, n_own = s.n_own, nnz_local = s.nnz_local;
    const int32_t *dom = s.dom, *inv = s.inv, *perm = s.perm;
    const uint8_t *owner = s.owner;
    uint8_t *is_halo = s.is_halo;
    int32_t *g2l = s.g2l, *flag = s.flag, *pos = s.pos;
    DevBuf<int32_t> &ids = *s.ids, &scan_tmp = *s.scan_tmp;
    PlanGuards *G = s.keep ? &s.keep->guards : nullptr;
    DevBuf<int32_t> &halo_tmp = d->ws.halo_tmp;
    DevBuf<uint32_t> &needed_by = d->ws.needed_by;
    DevBuf<int> &mark_err = d->ws.mark_err;
    AVS_TRY(plan_buf(G, mark_err, 1, true, st));
    AVS_HIP(hipMemsetAsync(mark_err.p, 0, sizeof(int), st));
    PhaseTrace tr(st, "tail", cur_opt().trace_phases != 0);
    AVS_TRY(plan_buf(G, needed_by, (size_t)n_own, true, st));
    if (n_own) hipLaunchKernelGGL(k_da_mark, dim3(8192), dim3(256), 0, st, n_own, d->row_ptr.p, d->col.p, inv, owner, rank, is_halo,
                                  needed_by.p, mark_err.p);
    uint32_t peer_mask = 0u; // (a slab talks to its neighbours: the per-rank scans below run for them only -- each is a scan + a host round trip)
    {
        DevBuf<uint32_t> &pm = d->ws.pm;
        AVS_TRY(plan_buf(G, pm, 1, true, st));
        AVS_HIP(hipMemsetAsync(pm.p, 0, sizeof(uint32_t), st));
        if (n_own) hipLaunchKernelGGL(k_da_peer_mask, dim3(1024), dim3(256), 0, st, n_own, (const uint32_t *)needed_by.p, pm.p);
        int e = 0;
        AVS_HIP(hipMemcpyAsync(&e, mark_err.p, sizeof(int), hipMemcpyDeviceToHost, st));
        AVS_HIP(hipMemcpyAsync(&peer_mask, pm.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        AVS_HIP(hipStreamSynchronize(st));
        AVS_REQUIRE(e == 0, AVS_EINTERNAL, "slab-local assembly: a row reads a column outside the rank's window (index margin too small)");
    }
    tr.mark("mark columns");
    if (s.split && n_own) { // [interior | halo-reading] local row order (see k_da_new_index)
        DevBuf<int32_t> &new_of = d->alt_new_of, &len_new = d->alt_len, &rp2 = d->alt_row_ptr, &col2 = d->alt_col, &own2 = d->alt_own, &ids2 = d->alt_ids;
        DevBuf<double> &val2 = d->alt_val, &rhs2 = d->alt_rhs;
        DevBuf<uint32_t> &nb2 = d->alt_nb;
        AVS_TRY(plan_buf(G, new_of, (size_t)n_own, true, st));
        AVS_TRY(plan_buf(G, len_new, (size_t)n_own + 1, true, st));
        AVS_TRY(plan_buf(G, rp2, (size_t)n_own + 1, true, st));
        AVS_TRY(plan_buf(G, col2, (size_t)nnz_local, true, st));
        AVS_TRY(plan_buf(G, val2, (size_t)nnz_local, true, st));
        AVS_TRY(plan_buf(G, own2, (size_t)n_own, true, st));
        AVS_TRY(plan_buf(G, ids2, (size_t)n_own, true, st));
        AVS_TRY(plan_buf(G, rhs2, (size_t)n_own, true, st));
        AVS_TRY(plan_buf(G, nb2, (size_t)n_own, true, st));
        hipLaunchKernelGGL(k_da_flag_send, dim3(grid256(n_own)), dim3(256), 0, st, n_own, (const uint32_t *)needed_by.p, -1, flag); // q = -1: "reads nobody"
        int64_t n_interior = 0;
        AVS_TRY(scan_flags(flag, pos, n_own, scan_tmp, &n_interior, st));
        if (s.keep) s.keep->n_interior = n_interior;
        hipLaunchKernelGGL(k_da_new_index, dim3(grid256(n_own + 1)), dim3(256), 0, st, n_own, (const uint32_t *)needed_by.p, (const int32_t *)pos,
                           n_interior, (const int32_t *)d->row_ptr.p, new_of.p, len_new.p);
        AVS_TRY(exclusive_scan_i32(len_new.p, rp2.p, n_own, scan_tmp.p, scan_tmp.n, st));
        hipLaunchKernelGGL(k_da_move_rows, dim3(8192), dim3(256), 0, st, n_own, (const int32_t *)new_of.p, (const int32_t *)d->row_ptr.p,
                           (const int32_t *)d->col.p, (const double *)d->val.p, (const int32_t *)rp2.p, col2.p, val2.p);
        const unsigned g1 = grid256(n_own);
        hipLaunchKernelGGL(k_da_move<int32_t>, dim3(g1), dim3(256), 0, st, n_own, (const int32_t *)new_of.p, (const int32_t *)d->own_global.p, own2.p);
        hipLaunchKernelGGL(k_da_move<int32_t>, dim3(g1), dim3(256), 0, st, n_own, (const int32_t *)new_of.p, (const int32_t *)ids.p, ids2.p);
        hipLaunchKernelGGL(k_da_move<double>, dim3(g1), dim3(256), 0, st, n_own, (const int32_t *)new_of.p, (const double *)d->rhs.p, rhs2.p);
        hipLaunchKernelGGL(k_da_move<uint32_t>, dim3(g1), dim3(256), 0, st, n_own, (const int32_t *)new_of.p, (const uint32_t *)needed_by.p, nb2.p);
        hipLaunchKernelGGL(k_da_g2l_own, dim3(g1), dim3(256), 0, st, n_own, (const int32_t *)own2.p, g2l);
        AVS_HIP(hipGetLastError());
        AVS_HIP(hipStreamSynchronize(st));
        swap(d->row_ptr, rp2);
        swap(d->col, col2);
        swap(d->own_global, own2);
        swap(ids, ids2);
        swap(d->val, val2);
        swap(d->rhs, rhs2);
        swap(needed_by, nb2);
    }

    tr.mark("row order split");
    // halo numbering (grouped by owner, ascending) and send lists (ascending owned rows that read a DOF of q)
    PlanPass pass{rank, world, flag, pos, scan_tmp, G, st};
    AVS_TRY(plan_buf(G, halo_tmp, (size_t)(n > 0 ? n : 1), true, st));
    AVS_TRY(number_halo(pass, peer_mask, n, dom, is_halo, owner, n_own, g2l, halo_tmp.p, s.keep != nullptr));
    auto flag_send = [&](int q) { hipLaunchKernelGGL(k_da_flag_send, dim3(grid256(n_own)), dim3(256), 0, st, n_own, needed_by.p, q, flag); };
    AVS_TRY(build_send_lists(d, pass, peer_mask, n_own, flag_send, nullptr, true)); // local row index == local DOF index

    tr.mark("halo + send lists");
    // local column ids + tile lists
    const int T = spmv_tile_rows();
    const int64_t ntiles = (n_own + T - 1) / T;
    DevBuf<int32_t> &tile_bnd = d->ws.tile_bnd, &tile_int = d->ws.tile_int, &tile_pos = d->ws.tile_pos;
    AVS_TRY(plan_buf(G, tile_bnd, (size_t)ntiles + 1, true, st));
    AVS_TRY(plan_buf(G, tile_int, (size_t)ntiles + 1, true, st));
    AVS_TRY(plan_buf(G, tile_pos, (size_t)ntiles + 1, true, st));
    AVS_HIP(hipMemsetAsync(tile_bnd.p, 0, ((size_t)ntiles + 1) * 4, st));
    if (n_own) hipLaunchKernelGGL(k_da_localize, dim3(8192), dim3(256), 0, st, n_own, d->row_ptr.p, d->col.p, g2l, T, tile_bnd.p);
    AVS_TRY(build_tile_lists(d, pass, ntiles, tile_bnd.p, tile_int.p, tile_pos.p, true));

    // reference ids behind the local columns (owned: the assembled rows' DOFs; halo: through the brick-major permutation)
    AVS_TRY(plan_buf(G, d->local_ref, (size_t)(n_own + pass.n_halo), true, st));
    if (n_own) AVS_HIP(hipMemcpyAsync(d->local_ref.p, ids.p, (size_t)n_own * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    if (pass.n_halo) hipLaunchKernelGGL(k_da_halo_ref, dim3(grid256(n)), dim3(256), 0, st, n, (const int32_t *)g2l, perm, n_own, d->local_ref.p, dom);
    AVS_TRY(finish_plan(d, pass, n_own, nnz_local));
    tr.mark("localize, tiles, local_ref");
    return AVS_OK;
}

// cuts[r] = first fine cell of rank r's slab (cuts[world] = extent) from the planes' owners (non-decreasing)
static void cuts_from_plane_owners(const std::vector<int> &po, int world, int shift, int extent, std::vector<int32_t> &cuts)
{
    cuts.assign((size_t)world + 1, extent);
    cuts[0] = 0;
    for (int r = 1; r < world; ++r) {
        int p = 0;
        while (p < (int)po.size() && po[(size_t)p] < r) ++p;
        const long long c = (long long)p << shift;
        cuts[(size_t)r] = (int32_t)(c < extent ? c : extent);
    }
}

// ---------------------------------------------------------------------------------------------
// Slab-local assembly (round 6; SURVEY 8(e): "each GPU assembles the rows it owns from its slab of the pyramids plus a halo").
// The context holds what a slab-local pre-pass lent it (avs_prepass_set_slab): lattices and dof tables valid inside the rank's window,
// GLOBAL reference ids, the ids of the window's DOFs.  Nothing here is sized or swept by the global DOF count except three
// lookup arrays indexed by reference id (owner, halo flag, local id: 6 B per DOF, filled by memset) -- the sweeps run over the window's
// DOFs (brick-major: the stable sort of their brick keys, the same relative order as the global permutation's), the rows are the
// reference's rows bit for bit, and the local order, halo order and send lists equal the replicated-index assembly's for the same cuts.
// ---------------------------------------------------------------------------------------------
struct CutTable {
    int world;
    int cuts[kMaxRanks + 1];
};
__global__ __launch_bounds__(256) void k_win_keys(const int32_t *__restrict__ vdof, const int32_t *__restrict__ wl, int64_t m, int nx, int ny, int nz,
                                                  int shift, int interleave, uint32_t *__restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int4 rec = reinterpret_cast<const int4 *>(vdof)[wl[i]]; // (the key of avs_reorder.hip's k_brick_keys)
    const int level = rec.x & 0xff;
    int px = rec.y << level, py = rec.z << level, pz = rec.w << level;
    px = px < nx ? px : nx - 1;
    py = py < ny ? py : ny - 1;
    pz = pz < nz ? pz : nz - 1;
    const uint32_t bx = (uint32_t)(px >> shift), by = (uint32_t)(py >> shift), bz = (uint32_t)(pz >> shift);
    const uint32_t nbx = (uint32_t)((nx + (1 << shift) - 1) >> shift), nby = (uint32_t)((ny + (1 << shift) - 1) >> shift);
    uint32_t key = (bz * nby + by) * nbx + bx;
    if (interleave) {
        const uint32_t mk = (1u << shift) - 1u;
        key = (key << (3 * shift)) | ((((uint32_t)pz & mk) << (2 * shift)) | (((uint32_t)py & mk) << shift) | ((uint32_t)px & mk));
    }
    keys[i] = key;
}
// owner of every DOF of the window (by the position of its face along the cut axis), own flags
__global__ __launch_bounds__(256) void k_win_owner(int64_t m, const int32_t *__restrict__ vdof, const int32_t *__restrict__ dom, int axis, int extent,
                                                   CutTable T, int rank, uint8_t *__restrict__ owner_ref, int32_t *__restrict__ own_flag)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int32_t id = dom[i];
    const int32_t *t = vdof + 4 * (int64_t)id;
    const int level = t[0] & 0xff;
    long long pos = (long long)t[1 + axis] << level;
    if (pos >= extent) pos = extent - 1;
    int r = 0;
    while (r + 1 < T.world && pos >= T.cuts[r + 1]) ++r;
    owner_ref[id] = (uint8_t)r;
    own_flag[i] = r == rank;
}
// per-plane weights of the rank's rows (non-zeros + 2, as the host planner), in units of 16 so that the sum over
// a plane of a 2048^2 cross-section fits the int32 the ranks exchange
__global__ __launch_bounds__(256) void k_win_plane_weights(int64_t n_own, const int32_t *__restrict__ ids, const int32_t *__restrict__ vdof,
                                                           const int32_t *__restrict__ row_ptr, int axis, int extent, int shift,
                                                           unsigned long long *__restrict__ weight)
{
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= n_own) return;
    atomicAdd(&weight[plane_of_dof(vdof, ids[l], axis, extent, shift)], (unsigned long long)(row_ptr[l + 1] - row_ptr[l]) + 2ull);
}
__global__ __launch_bounds__(256) void k_win_weights_pack(int n, const unsigned long long *__restrict__ w, int32_t *__restrict__ out)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i < n) out[i] = (int32_t)((w[i] + 15ull) >> 4);
}

avs_status dist_assemble_window(avs_ctx *c, PcgDist *d)
{
    hipStream_t st = c->stream;
    const SlabWindow &W = c->slab;
    const int rank = d->rank, world = d->world;
    AVS_REQUIRE(W.world == world && W.rank == rank, AVS_ESTATE, "the slab of the pre-pass (rank %d of %d) is not this context's rank (%d of %d)", W.rank,
                W.world, rank, world);
    AVS_REQUIRE(c->tables_ready && c->wlist[0].p, AVS_ESTATE, "slab-local context without dof tables / window lists");
    const int64_t n = c->n_vel, n_w = c->n_window[0];
    const int axis = W.axis;
    const int extent = axis == 0 ? c->desc.nx : (axis == 1 ? c->desc.ny : c->desc.nz);
    d->cuts.assign(W.cuts, W.cuts + world + 1);
    d->cut_axis = axis;
    PhaseTrace tr(st, "window", cur_opt().trace_phases != 0);

    // the window's velocity DOFs in brick-major order
    DevBuf<uint32_t> &keys_in = d->ws.keys_in, &keys_out = d->ws.keys_out;
    DevBuf<int32_t> &dom = d->ws.dom, &flag = d->ws.flag, &pos = d->ws.pos, &g2l = d->ws.g2l, &scan_tmp = d->ws.scan_tmp, &ids = d->ws.ids;
    DevBuf<uint8_t> &owner = d->ws.owner, &is_halo = d->ws.is_halo;
    DevBuf<char> &sort_tmp = d->ws.sort_tmp;
    AVS_TRY(keys_in.reserve((size_t)(n_w > 0 ? n_w : 1)));
    AVS_TRY(keys_out.reserve((size_t)(n_w > 0 ? n_w : 1)));
    AVS_TRY(dom.reserve((size_t)(n_w > 0 ? n_w : 1)));
    AVS_TRY(flag.reserve((size_t)n_w + 1));
    AVS_TRY(pos.reserve((size_t)n_w + 1));
    AVS_TRY(scan_tmp.reserve(scan_tmp_elems(n_w + 1)));
    AVS_TRY(g2l.reserve((size_t)(n > 0 ? n : 1)));
    AVS_TRY(owner.reserve((size_t)(n > 0 ? n : 1)));
    AVS_TRY(is_halo.reserve((size_t)(n > 0 ? n : 1)));
    AVS_HIP(hipMemsetAsync(g2l.p, 0xFF, (size_t)n * sizeof(int32_t), st));
    AVS_HIP(hipMemsetAsync(owner.p, 0xFF, (size_t)n, st));
    AVS_HIP(hipMemsetAsync(is_halo.p, 0, (size_t)n, st));
    tr.mark("alloc + memsets");
    int interleave = cur_opt().brick_interleave;
    {
        const int bs = c->brick_shift;
        const uint64_t nb = (uint64_t)((c->desc.nx >> bs) + 1) * ((c->desc.ny >> bs) + 1) * ((c->desc.nz >> bs) + 1);
        if ((nb << (3 * bs)) >= (1ull << 32)) interleave = 0;
    }
    if (n_w) {
        hipLaunchKernelGGL(k_win_keys, dim3(grid256(n_w)), dim3(256), 0, st, c->vdof.p, c->wlist[0].p, n_w, c->desc.nx, c->desc.ny, c->desc.nz,
                           c->brick_shift, interleave, keys_in.p);
        size_t tmp_bytes = 0;
        AVS_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys_in.p, keys_out.p, c->wlist[0].p, dom.p, (size_t)n_w, 0, 32, st));
        AVS_TRY(sort_tmp.reserve(tmp_bytes > 0 ? tmp_bytes : 1));
        AVS_HIP(rocprim::radix_sort_pairs(sort_tmp.p, tmp_bytes, keys_in.p, keys_out.p, c->wlist[0].p, dom.p, (size_t)n_w, 0, 32, st)); // stable
        CutTable T{};
        T.world = world;
        for (int r = 0; r <= world; ++r) T.cuts[r] = W.cuts[r];
        hipLaunchKernelGGL(k_win_owner, dim3(grid256(n_w)), dim3(256), 0, st, n_w, c->vdof.p, dom.p, axis, extent, T, rank, owner.p, flag.p);
    }
    tr.mark("keys, sort, owners");
    int64_t n_own = 0;
    AVS_TRY(scan_flags(flag.p, pos.p, n_w, scan_tmp, &n_own, st));
    AVS_TRY(ids.reserve((size_t)(n_own > 0 ? n_own : 1)));
    AVS_TRY(d->own_global.reserve((size_t)n_own));
    if (n_own) {
        hipLaunchKernelGGL(k_plan_scatter, dim3(grid256(n_w)), dim3(256), 0, st, n_w, flag.p, pos.p, (const int32_t *)nullptr, ids.p, g2l.p, 0, dom.p);
        AVS_HIP(hipMemcpyAsync(d->own_global.p, ids.p, (size_t)n_own * sizeof(int32_t), hipMemcpyDeviceToDevice, st)); // (reference ids: avs_dist_get_solution scatters by them)
    }
    tr.mark("own list");
    AVS_TRY(dist_assemble_tail(c, d, n_own, dom.p, n_w, nullptr, nullptr));
    tr.mark("tail");

    // the cuts this frame's weights suggest for the next one: per-plane weights of the own rows, summed over the ranks
    d->next_cuts = d->cuts;
    if (!d->hosted) {
        const int shift = plane_shift(c->desc.levels);
        const int nplanes = (extent + (1 << shift) - 1) >> shift;
        DevBuf<unsigned long long> &weight = d->ws.weight;
        DevBuf<int32_t> &w32 = d->ws.w32;
        AVS_TRY(weight.reserve((size_t)nplanes));
        AVS_TRY(w32.reserve((size_t)nplanes));
        AVS_HIP(hipMemsetAsync(weight.p, 0, (size_t)nplanes * sizeof(unsigned long long), st));
        if (n_own)
            hipLaunchKernelGGL(k_win_plane_weights, dim3(grid256(n_own)), dim3(256), 0, st, n_own, (const int32_t *)d->local_ref.p, c->vdof.p,
                               (const int32_t *)d->row_ptr.p, axis, extent, shift, weight.p);
        hipLaunchKernelGGL(k_win_weights_pack, dim3(grid256(nplanes)), dim3(256), 0, st, nplanes, weight.p, w32.p);
        AVS_TRY(dist_allreduce_i32(d, w32.p, nplanes, st));
        std::vector<int32_t> hw((size_t)nplanes);
        AVS_HIP(hipMemcpyAsync(hw.data(), w32.p, hw.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        AVS_HIP(hipStreamSynchronize(st));
        cuts_from_plane_owners(plane_owners(std::vector<int64_t>(hw.begin(), hw.end()), world), world, shift, extent, d->next_cuts);
    }
    return AVS_OK;
}

avs_status dist_assemble_device(avs_ctx *c, PcgDist *d, int cut_axis, int extent)
{
    hipStream_t st = c->stream;
    const int64_t n = c->n_vel;
    const int rank = d->rank, world = d->world;
    AVS_REQUIRE(world <= 32, AVS_EINVAL, "at most 32 ranks");
    // Cut planes: the slabs are cut between planes of 2^shift fine cells.  The replicated planner (avs_dist_partition, avs_partition.cpp)
    // keeps 2^(levels-1) -- no top-level cell straddles a cut; here, where every rank assembles its own rows, nothing needs that (a DOF
    // belongs to the plane of its own position, whatever it reads is a halo column), and planes of at most 4 cells halve the granularity
    // of the balance at 4 levels: on the 8-way partition of the 512^3 beam a rank's share moved in steps of 12.5 % (868 k .. 994 k rows,
    // 30.5 .. 34.3 us per iteration in the loop-back measurement -- the slowest rank sets the pace).  AVS_DIST_PLANE_SHIFT overrides.
    const int shift = plane_shift(c->desc.levels);
    const int nplanes = (extent + (1 << shift) - 1) >> shift;
    AVS_REQUIRE(nplanes <= 65535, AVS_EINVAL, "too many cut planes");

    // global, index-only: raw triplet count per row (weights) and the brick-major permutation
    DevBuf<int32_t> &raw_count = d->ws.raw_count; // (work arrays kept across frames: see PcgDist::Scratch)
    AVS_TRY(count_raw_rows(c, raw_count));
    AVS_TRY(build_brick_permutation(c, c->brick_shift));

    DevBuf<uint16_t> &plane = d->ws.plane;
    DevBuf<unsigned long long> &weight = d->ws.weight;
    DevBuf<int32_t> &plane_owner = d->ws.plane_owner, &flag = d->ws.flag, &pos = d->ws.pos, &g2l = d->ws.g2l, &scan_tmp = d->ws.scan_tmp, &ids = d->ws.ids;
    DevBuf<uint8_t> &owner = d->ws.owner, &is_halo = d->ws.is_halo;
    AVS_TRY(plane.reserve((size_t)(n > 0 ? n : 1)));
    AVS_TRY(weight.reserve((size_t)nplanes));
    AVS_TRY(plane_owner.reserve((size_t)nplanes));
    AVS_TRY(flag.reserve((size_t)n + 1));
    AVS_TRY(pos.reserve((size_t)n + 1));
    AVS_TRY(g2l.reserve((size_t)(n > 0 ? n : 1)));
    AVS_TRY(scan_tmp.reserve(scan_tmp_elems(n + 1)));
    AVS_TRY(owner.reserve((size_t)(n > 0 ? n : 1)));
    AVS_TRY(is_halo.reserve((size_t)(n > 0 ? n : 1)));
    AVS_HIP(hipMemsetAsync(weight.p, 0, (size_t)nplanes * sizeof(unsigned long long), st));
    AVS_HIP(hipMemsetAsync(is_halo.p, 0, (size_t)n, st));
    AVS_HIP(hipMemsetAsync(g2l.p, 0xFF, (size_t)n * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_plan_planes<true>, dim3(2048), dim3(256), 0, st, n, c->vdof.p, c->perm.p, raw_count.p, cut_axis, extent, shift, nplanes,
                       plane.p, weight.p);
    std::vector<int64_t> h_w;
    std::vector<int> h_po;
    AVS_TRY(owners_from_weights(weight.p, nplanes, world, rank, n, plane.p, plane_owner.p, owner.p, flag.p, h_w, h_po, st));
    cuts_from_plane_owners(h_po, world, shift, extent, d->cuts);
    d->next_cuts = d->cuts;
    d->cut_axis = cut_axis;

    // owned rows (ascending brick-major id) and the DOFs behind them
    int64_t n_own = 0;
    AVS_TRY(scan_flags(flag.p, pos.p, n, scan_tmp, &n_own, st));
    AVS_TRY(d->own_global.reserve((size_t)n_own));
    AVS_TRY(ids.reserve((size_t)(n_own > 0 ? n_own : 1)));
    hipLaunchKernelGGL(k_plan_scatter, dim3(grid256(n)), dim3(256), 0, st, n, flag.p, pos.p, (const int32_t *)nullptr, d->own_global.p,
                       g2l.p, 0);
    if (n_own) hipLaunchKernelGGL(k_gather_i<int32_t>, dim3(grid256(n_own)), dim3(256), 0, st, c->perm.p, d->own_global.p, ids.p, n_own);

    return dist_assemble_tail(c, d, n_own, nullptr, n, c->inv.p, c->perm.p);
}

// storage form of the rank's local rows (avs_get_matrix_format when no global matrix exists)
bool dist_matrix_format(avs_ctx *c, avs_matrix_format *fmt)
{
    if (fmt) { fmt->brick_tiles = 0; fmt->brick_patterns = 0; fmt->brick_pattern_rows = 0; fmt->brick_bytes = 0; }
    PcgDist *d = c->dist;
    if (!d || !d->partitioned) return false;
    fmt->reordered = d->reordered ? 1 : 0;
    fmt->value_table_size = d->vi.table_size;
    fmt->column_bits = d->vi.col_bits;
    fmt->bytes_per_nonzero = d->vi.bytes_per_nonzero();
    fmt->tile_local_tables = d->vi.tile_tables ? 1 : 0;
    fmt->column_windows = d->vi.col_windows ? 1 : 0;
    if (d->brick.ready) {
        fmt->brick_tiles = d->brick.ntiles;
        fmt->brick_patterns = d->brick.patterns;
        fmt->brick_pattern_rows = d->brick.regular_rows;
        fmt->brick_bytes = d->brick.stored_bytes(d->n_own);
        fmt->brick_walk = d->brick_view.walk;
        fmt->brick_value_codes = d->brick.vc ? 1 : 0;
    }
    return true;
}

// the host planner (avs_partition.cpp) on a downloaded copy of the pattern: reference for the device planner
avs_status plan_on_host(avs_ctx *c, PcgDist *d, int cut_axis, int extent, bool ro)
{
    hipStream_t st = c->stream;
    const int64_t n = c->n_vel, nnz = c->nnz;
    const int32_t *g_rp = ro ? c->p_row_ptr.p : c->row_ptr.p, *g_col = ro ? c->p_col.p : c->col.p;
    const double *g_val = ro ? c->p_val.p : c->val.p;
    std::vector<int32_t> h_rp((size_t)n + 1), h_col((size_t)nnz), h_tab((size_t)n * 4), h_owner((size_t)n);
    AVS_HIP(hipMemcpyAsync(h_rp.data(), g_rp, h_rp.size() * 4, hipMemcpyDeviceToHost, st));
    AVS_HIP(hipMemcpyAsync(h_col.data(), g_col, h_col.size() * 4, hipMemcpyDeviceToHost, st));
    AVS_HIP(hipMemcpyAsync(h_tab.data(), c->vdof.p, h_tab.size() * 4, hipMemcpyDeviceToHost, st));
    AVS_HIP(hipStreamSynchronize(st));
    if (ro) { // dof table in the new numbering
        std::vector<int32_t> h_perm((size_t)n), t2((size_t)n * 4);
        AVS_HIP(hipMemcpy(h_perm.data(), c->perm.p, h_perm.size() * 4, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; ++i) memcpy(&t2[(size_t)i * 4], &h_tab[(size_t)h_perm[(size_t)i] * 4], 16);
        h_tab.swap(t2);
    }
    AVS_TRY(avs_plan_owners(n, h_tab.data(), h_rp.data(), c->desc.levels, cut_axis, extent, d->world, h_owner.data()));
    avs_plan *plan = nullptr;
    AVS_TRY(avs_plan_create(n, h_rp.data(), h_col.data(), h_owner.data(), d->rank, d->world, &plan));
    avs_plan_sizes sz{};
    avs_plan_get_sizes(plan, &sz);
    std::vector<int32_t> own((size_t)sz.n_own), rpl((size_t)sz.n_own + 1), cl((size_t)sz.nnz_local), vs((size_t)sz.nnz_local),
        peers((size_t)sz.n_peers), sc((size_t)sz.n_peers), rc((size_t)sz.n_peers), sidx((size_t)sz.n_send);
    avs_plan_get_arrays(plan, own.data(), nullptr, rpl.data(), cl.data(), vs.data(), peers.data(), sc.data(), rc.data(), sidx.data());
    avs_plan_destroy(plan);
    d->n_own = sz.n_own;
    d->n_halo = sz.n_halo;
    d->n_send = sz.n_send;
    d->nnz_local = sz.nnz_local;
    d->peers = peers;
    d->send_counts = sc;
    d->recv_counts = rc;
    AVS_TRY(d->own_global.alloc((size_t)sz.n_own));
    AVS_TRY(d->send_idx.alloc((size_t)sz.n_send));
    AVS_TRY(d->sendbuf.alloc((size_t)sz.n_send));
    AVS_TRY(d->row_ptr.alloc((size_t)sz.n_own + 1));
    AVS_TRY(d->col.alloc((size_t)sz.nnz_local));
    AVS_TRY(d->val.alloc((size_t)sz.nnz_local));
    DevBuf<int32_t> d_vs;
    AVS_TRY(d_vs.alloc((size_t)sz.nnz_local));
    AVS_HIP(hipMemcpyAsync(d->own_global.p, own.data(), own.size() * 4, hipMemcpyHostToDevice, st));
    if (sz.n_send) AVS_HIP(hipMemcpyAsync(d->send_idx.p, sidx.data(), sidx.size() * 4, hipMemcpyHostToDevice, st));
    AVS_HIP(hipMemcpyAsync(d->row_ptr.p, rpl.data(), rpl.size() * 4, hipMemcpyHostToDevice, st));
    if (sz.nnz_local) {
        AVS_HIP(hipMemcpyAsync(d->col.p, cl.data(), cl.size() * 4, hipMemcpyHostToDevice, st));
        AVS_HIP(hipMemcpyAsync(d_vs.p, vs.data(), vs.size() * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_gather_i<double>, dim3(grid256(sz.nnz_local)), dim3(256), 0, st, g_val, d_vs.p, d->val.p, sz.nnz_local);
    }
    AVS_HIP(hipGetLastError());
    AVS_HIP(hipStreamSynchronize(st));
    // tiles of the local SpMV that read no halo column can run while the halo is in flight
    const int T = spmv_tile_rows();
    const int64_t ntiles = (sz.n_own + T - 1) / T;
    std::vector<int32_t> ti, tb;
    for (int64_t t = 0; t < ntiles; ++t) {
        const int64_t r0 = t * T, r1 = std::min<int64_t>(r0 + T, sz.n_own);
        bool touches = false;
        for (int32_t k = rpl[(size_t)r0]; k < rpl[(size_t)r1] && !touches; ++k) touches = cl[(size_t)k] >= sz.n_own;
        (touches ? tb : ti).push_back((int32_t)t);
    }
    d->n_tiles_int = (int)ti.size();
    d->n_tiles_bnd = (int)tb.size();
    AVS_TRY(d->tiles_int.alloc(ti.size()));
    AVS_TRY(d->tiles_bnd.alloc(tb.size()));
    if (!ti.empty()) AVS_HIP(hipMemcpy(d->tiles_int.p, ti.data(), ti.size() * 4, hipMemcpyHostToDevice));
    if (!tb.empty()) AVS_HIP(hipMemcpy(d->tiles_bnd.p, tb.data(), tb.size() * 4, hipMemcpyHostToDevice));
    return AVS_OK;
}

} // namespace avs

using namespace avs;

#ifdef AVS_PROBES
// test entry (C linkage from include/avs_probe.h): the planner cores -- plan_from_source, dist_tail_from_rows -- on the caller's device arrays
template <typename T>
static avs_status plan_probe_out(T *dst, const T *src, int64_t count, int64_t capacity, const char *what)
{
    if (!dst || count == 0) return AVS_OK;
    AVS_REQUIRE(count <= capacity, AVS_EINVAL, "%s: %lld entries exceed the capacity %lld", what, (long long)count, (long long)capacity);
    AVS_HIP(hipMemcpy(dst, src, (size_t)count * sizeof(T), hipMemcpyDeviceToHost));
    return AVS_OK;
}
template <typename T>
static avs_status plan_probe_up(PlanGuards *G, DevBuf<T> &b, const std::vector<T> &h, hipStream_t st)
{
    AVS_TRY(plan_buf(G, b, h.size(), false, st));
    if (!h.empty()) AVS_HIP(hipMemcpyAsync(b.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st));
    AVS_HIP(hipStreamSynchronize(st)); // (h may die before the stream gets there)
    return AVS_OK;
}

avs_status avs_dist_plan_probe(int32_t mode, const avs_dist_plan_input *in, const avs_dist_plan_output *out, avs_dist_plan_info *info,
                               void *stream)
{
    AVS_REQUIRE(info && info->struct_size >= (int32_t)sizeof(avs_dist_plan_info), AVS_EINVAL, "info: struct_size not set");
    info->lds_planes = kPlanLdsPlanes;
    info->scan_tile = scan_tile_elems();
    info->spmv_tile_rows = spmv_tile_rows();
    info->row_group = 16;
    info->max_world = kMaxRanks;
    info->nplanes = info->n_peers = info->n_tiles_int = info->n_tiles_bnd = 0;
    info->n_own = info->n_halo = info->n_send = info->nnz_local = 0;
    info->n_interior = -1;
    info->guard_bytes_hit = 0;
    if (!in || (in->n == 0 && !in->row_ptr)) return AVS_OK; // the limits alone: nothing touches the device
    AVS_REQUIRE(out, AVS_EINVAL, "null argument");
    AVS_REQUIRE(mode == AVS_DIST_PLAN_PROBE_PLAN || mode == AVS_DIST_PLAN_PROBE_TAIL, AVS_EINVAL, "unknown mode %d", mode);
    const bool tail = mode == AVS_DIST_PLAN_PROBE_TAIL;
    const int64_t n = in->n;
    const int rank = in->rank, world = in->world;
    AVS_REQUIRE(n >= 0 && n < (int64_t)INT32_MAX && in->row_ptr, AVS_EINVAL, "bad argument");
    AVS_REQUIRE(world >= 1 && world <= kMaxRanks && rank >= 0 && rank < world, AVS_EINVAL, "rank %d / world %d out of range", rank, world);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    // host copies: everything is checked before the first launch
    std::vector<int32_t> h_rp((size_t)n + 1);
    AVS_HIP(hipMemcpy(h_rp.data(), in->row_ptr, h_rp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    AVS_REQUIRE(h_rp[0] == 0, AVS_EINVAL, "row_ptr[0] must be 0");
    for (int64_t i = 0; i < n; ++i) AVS_REQUIRE(h_rp[(size_t)i + 1] >= h_rp[(size_t)i], AVS_EINVAL, "row_ptr decreases at row %lld", (long long)i);
    const int64_t nnz = h_rp[(size_t)n];
    AVS_REQUIRE(nnz == 0 || (in->col && in->val), AVS_EINVAL, "null matrix arrays");
    std::vector<int32_t> h_col((size_t)nnz);
    if (nnz) AVS_HIP(hipMemcpy(h_col.data(), in->col, h_col.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < nnz; ++k)
        AVS_REQUIRE(h_col[(size_t)k] >= 0 && h_col[(size_t)k] < n, AVS_EINVAL, "column %d of entry %lld outside [0, %lld)", h_col[(size_t)k],
                    (long long)k, (long long)n);

    PcgDist d;
    d.rank = rank;
    d.world = world;
    PlanKeep keep;
    PlanGuards *G = &keep.guards;
    G->spans = 0;
    G->hit = 0;
    if (!tail) {
        AVS_REQUIRE(in->dof, AVS_EINVAL, "null dof records");
        AVS_REQUIRE(in->levels >= 1 && in->levels <= AVS_MAX_LEVELS && in->cut_axis >= 0 && in->cut_axis <= 2 && in->extent >= 1, AVS_EINVAL,
                    "levels %d / cut_axis %d / extent %d out of range", in->levels, in->cut_axis, in->extent);
        const int shift = in->levels - 1;
        const int64_t nplanes = ((int64_t)in->extent + (1 << shift) - 1) >> shift;
        AVS_REQUIRE(nplanes <= 65535, AVS_EINVAL, "too many cut planes");
        std::vector<int32_t> h_dof((size_t)n * 4), h_perm;
        if (n) AVS_HIP(hipMemcpy(h_dof.data(), in->dof, h_dof.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; ++i) {
            const int32_t *t = &h_dof[(size_t)i * 4];
            AVS_REQUIRE((t[0] & 0xff) <= 30 && t[1] >= 0 && t[2] >= 0 && t[3] >= 0, AVS_EINVAL, "dof record %lld out of range", (long long)i);
        }
        if (in->perm) {
            h_perm.resize((size_t)n);
            if (n) AVS_HIP(hipMemcpy(h_perm.data(), in->perm, h_perm.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < n; ++i)
                AVS_REQUIRE(h_perm[(size_t)i] >= 0 && h_perm[(size_t)i] < n, AVS_EINVAL, "perm[%lld] outside [0, %lld)", (long long)i, (long long)n);
        }
        PlanSource s;
        s.n = n;
        s.row_ptr = in->row_ptr;
        s.col = in->col;
        s.val = in->val;
        s.vdof = in->dof;
        s.perm = in->perm;
        s.levels = in->levels;
        s.cut_axis = in->cut_axis;
        s.extent = in->extent;
        s.stream = st;
        s.keep = &keep;
        const avs_status rc = plan_from_source(&d, s);
        info->guard_bytes_hit = G->hit;
        if (rc != AVS_OK) return rc;
        info->nplanes = (int32_t)nplanes;
        if (out->weights || out->plane_owner)
            AVS_REQUIRE(nplanes <= out->plane_capacity, AVS_EINVAL, "%lld planes exceed the capacity %lld", (long long)nplanes, (long long)out->plane_capacity);
        if (out->weights) std::copy(keep.weight.begin(), keep.weight.end(), out->weights);
        if (out->plane_owner) std::copy(keep.plane_owner.begin(), keep.plane_owner.end(), out->plane_owner);
        AVS_TRY(plan_probe_out(out->owner, (const uint8_t *)keep.owner.p, n, n, "owner"));
    } else {
        AVS_REQUIRE(in->owner, AVS_EINVAL, "null owner array");
        AVS_REQUIRE(in->n_dom >= 0 && in->n_dom <= n && (in->dom || in->n_dom == 0), AVS_EINVAL, "dom: %lld entries for %lld ids", (long long)in->n_dom,
                    (long long)n);
        std::vector<uint8_t> h_owner((size_t)n);
        if (n) AVS_HIP(hipMemcpy(h_owner.data(), in->owner, h_owner.size(), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; ++i)
            AVS_REQUIRE(h_owner[(size_t)i] < world || h_owner[(size_t)i] == 0xFF, AVS_EINVAL, "owner[%lld] = %d is no rank", (long long)i, h_owner[(size_t)i]);
        const int64_t n_dom = in->dom ? in->n_dom : n;
        if (in->dom) {
            std::vector<int32_t> h_dom((size_t)n_dom);
            std::vector<uint8_t> seen((size_t)n, 0);
            if (n_dom) AVS_HIP(hipMemcpy(h_dom.data(), in->dom, h_dom.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < n_dom; ++i) {
                const int32_t g = h_dom[(size_t)i];
                AVS_REQUIRE(g >= 0 && g < n && !seen[(size_t)g], AVS_EINVAL, "dom[%lld] = %d outside [0, %lld) or listed twice", (long long)i, g, (long long)n);
                seen[(size_t)g] = 1;
            }
        }
        { // symmetric pattern: the sorted (row, column) pairs equal the sorted (column, row) pairs
            std::vector<uint64_t> a((size_t)nnz), b((size_t)nnz);
            for (int64_t r = 0; r < n; ++r)
                for (int32_t k = h_rp[(size_t)r]; k < h_rp[(size_t)r + 1]; ++k) {
                    a[(size_t)k] = ((uint64_t)r << 32) | (uint32_t)h_col[(size_t)k];
                    b[(size_t)k] = ((uint64_t)(uint32_t)h_col[(size_t)k] << 32) | (uint64_t)r;
                }
            std::sort(a.begin(), a.end());
            std::sort(b.begin(), b.end());
            a.erase(std::unique(a.begin(), a.end()), a.end());
            b.erase(std::unique(b.begin(), b.end()), b.end());
            AVS_REQUIRE(a == b, AVS_EINVAL, "TAIL mode: the pattern is not symmetric");
        }
        // the state after assemble_rows: the rank's rows in ascending id order, columns still global
        std::vector<double> h_val((size_t)nnz);
        if (nnz) AVS_HIP(hipMemcpy(h_val.data(), in->val, h_val.size() * sizeof(double), hipMemcpyDeviceToHost));
        std::vector<int32_t> ids, rp(1, 0), cl, g2l((size_t)n, -1);
        std::vector<double> vl, rhs;
        for (int64_t i = 0; i < n; ++i) {
            if (h_owner[(size_t)i] != rank) continue;
            g2l[(size_t)i] = (int32_t)ids.size();
            ids.push_back((int32_t)i);
            rhs.push_back((double)i);
            cl.insert(cl.end(), h_col.begin() + h_rp[(size_t)i], h_col.begin() + h_rp[(size_t)i + 1]);
            vl.insert(vl.end(), h_val.begin() + h_rp[(size_t)i], h_val.begin() + h_rp[(size_t)i + 1]);
            rp.push_back((int32_t)cl.size());
        }
        const int64_t n_own = (int64_t)ids.size();
        DevBuf<int32_t> d_ids, d_g2l, flag, pos, scan_tmp;
        DevBuf<uint8_t> is_halo;
        AVS_TRY(plan_probe_up(G, d_ids, ids, st));
        AVS_TRY(plan_probe_up(G, d.own_global, ids, st));
        AVS_TRY(plan_probe_up(G, d.row_ptr, rp, st));
        AVS_TRY(plan_probe_up(G, d.col, cl, st));
        AVS_TRY(plan_probe_up(G, d.val, vl, st));
        AVS_TRY(plan_probe_up(G, d.rhs, rhs, st));
        AVS_TRY(plan_probe_up(G, d_g2l, g2l, st));
        const int64_t n_scan = std::max(n_own, n_dom);
        AVS_TRY(plan_buf(G, flag, (size_t)n_scan + 1, false, st));
        AVS_TRY(plan_buf(G, pos, (size_t)n_scan + 1, false, st));
        AVS_TRY(plan_buf(G, scan_tmp, scan_tmp_elems(n_scan + 1), false, st));
        AVS_TRY(plan_buf(G, is_halo, (size_t)n, false, st));
        AVS_HIP(hipMemsetAsync(is_halo.p, 0, (size_t)n, st));
        TailSource s;
        s.ids = &d_ids;
        s.n_own = n_own;
        s.nnz_local = (int64_t)cl.size();
        s.dom = in->dom;
        s.n_dom = n_dom;
        s.owner = in->owner;
        s.is_halo = is_halo.p;
        s.g2l = d_g2l.p;
        s.flag = flag.p;
        s.pos = pos.p;
        s.scan_tmp = &scan_tmp;
        s.split = in->split != 0;
        s.stream = st;
        s.keep = &keep;
        const avs_status rc = dist_tail_from_rows(&d, s);
        info->guard_bytes_hit = G->hit;
        if (rc != AVS_OK) return rc;
        info->n_interior = keep.n_interior;
        AVS_TRY(plan_probe_out(out->local_ref, (const int32_t *)d.local_ref.p, d.n_own + d.n_halo, out->row_capacity, "local_ref"));
        AVS_TRY(plan_probe_out(out->rhs_local, (const double *)d.rhs.p, d.n_own, out->row_capacity, "rhs_local"));
    }
    DevBuf<int32_t> &halo = tail ? d.ws.halo_tmp : keep.halo;
    info->n_own = d.n_own;
    info->n_halo = d.n_halo;
    info->n_send = d.n_send;
    info->nnz_local = d.nnz_local;
    info->n_peers = (int32_t)d.peers.size();
    info->n_tiles_int = d.n_tiles_int;
    info->n_tiles_bnd = d.n_tiles_bnd;
    AVS_TRY(plan_probe_out(out->own_global, (const int32_t *)d.own_global.p, d.n_own, out->row_capacity, "own_global"));
    AVS_TRY(plan_probe_out(out->halo_global, (const int32_t *)halo.p, d.n_halo, out->row_capacity, "halo_global"));
    if (out->row_ptr_local) {
        AVS_REQUIRE(d.n_own <= out->row_capacity, AVS_EINVAL, "row_ptr_local: %lld rows exceed the capacity %lld", (long long)d.n_own, (long long)out->row_capacity);
        AVS_HIP(hipMemcpy(out->row_ptr_local, d.row_ptr.p, ((size_t)d.n_own + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    AVS_TRY(plan_probe_out(out->col_local, (const int32_t *)d.col.p, d.nnz_local, out->nnz_capacity, "col_local"));
    AVS_TRY(plan_probe_out(out->val_local, (const double *)d.val.p, d.nnz_local, out->nnz_capacity, "val_local"));
    AVS_TRY(plan_probe_out(out->send_idx, (const int32_t *)d.send_idx.p, d.n_send, out->send_capacity, "send_idx"));
    AVS_TRY(plan_probe_out(out->tiles_int, (const int32_t *)d.tiles_int.p, (int64_t)d.n_tiles_int, out->row_capacity, "tiles_int"));
    AVS_TRY(plan_probe_out(out->tiles_bnd, (const int32_t *)d.tiles_bnd.p, (int64_t)d.n_tiles_bnd, out->row_capacity, "tiles_bnd"));
    if (out->peers) std::copy(d.peers.begin(), d.peers.end(), out->peers);
    if (out->send_counts) std::copy(d.send_counts.begin(), d.send_counts.end(), out->send_counts);
    if (out->recv_counts) std::copy(d.recv_counts.begin(), d.recv_counts.end(), out->recv_counts);
    return AVS_OK;
}
#endif
