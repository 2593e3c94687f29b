// avs_cells.hip -- the octree's ACTIVE cells as points, on the device
// (reference: HDK_OctreeGrid::outputOctreeGeometry, oct.cpp:245-308; the "Output Octree Geometry" / "Only Output Octree" toggles).
//
// One record per cell labelled AVS_ACTIVE: position (cell centre, world units), pscale (the level's voxel size), level, ijk.  The order is
// the reference's sweep: levels ascending, UT_VoxelArray tile order inside a level (16^3 tiles x fastest, voxels x fastest inside a tile,
// partial tiles holding the voxels that exist) -- the order the numbering pass of avs_prepass.hip hands out ids in.
//
//   k_cell_counts      persistent waves, one wave per strip of 8 x-adjacent 16^3 tiles of the concatenated tile space of all levels: eight
//                      lanes read one 128-byte line of an x-row, each lane its tile's 16 labels as one 16-byte load (rows shorter
//                      than 16: bytewise), 16-bit ACTIVE masks, popcount, sums over the lanes of a tile: one count per tile; non-empty
//                      tiles are appended to a list (the only atomic; nothing below depends on the list's order)
//   k_cell_level_sums  per-level totals of the tile counts in 64 bits (the record count, known before anything is scanned)
//   exclusive_scan_i32 first record of every tile (the scan of the assembly and of the numbering pass)
//   k_cell_emit        persistent workgroups walk the list, thread t owns the x-row (y, z) = (t & 15, t >> 4): the rows are read again, a lane's first record is
//                      offset[tile] + (cells of the waves below, through LDS) + (wave prefix of the popcounts), bit order inside the lane:
//                      thread order followed by bit order IS the sweep order, and a tile's records are consecutive
//
// Everything is integer work or one fp64 -> fp32 rounding: the same labels give the same bytes on every call.
#include <climits>

#include "avs_internal.hpp"

namespace avs {

static constexpr int kCellBlock = 256;
static constexpr int kCellTile = 16;
static_assert(kCellBlock == kCellTile * kCellTile, "one thread per x-row of a 16^3 tile");
static constexpr int kCellStrip = 8;      // x-adjacent tiles a wave counts together: 8 x 16 labels = one 128-byte line per x-row
static constexpr int kCellSumBlocks = 128; // workgroups per level of the 64-bit sums

struct CellLevel {
    const int8_t *lab;
    int n[3];            // cells of the level's lattice
    int ntx, nty, tile0; // tiles per row / column, first tile in the concatenated space
    int vec;             // 1 = every row piece is 16 labels long and 16-byte aligned
    double h;            // voxel size: dx * 2^level
};
// by value; only what differs from level to level is a table (pointer, first tile): the level of a tile is found by an unrolled compare on
// scalar registers (see NumStarts, avs_prepass.hip), the rest follows from the level
struct CellLevels {
    const int8_t *lab[AVS_MAX_LEVELS];
    int tile0[AVS_MAX_LEVELS];  // levels not present: INT_MAX
    int strip0[AVS_MAX_LEVELS]; // first strip (kCellStrip x-adjacent tiles) of the level in the concatenated strip space; not present: INT_MAX
    int n[3];                  // level-0 cells per axis
    int vec_mask;              // bit l: level l is read with 16-byte loads
    int levels, total_tiles, total_strips;
    double dx;
};

__device__ __forceinline__ CellLevel cell_level(const CellLevels &L, int level, const int8_t *lab, int tile0)
{
    CellLevel c;
    c.lab = lab;
    c.tile0 = tile0;
#pragma unroll
    for (int a = 0; a < 3; ++a) c.n[a] = L.n[a] >> level;
    c.ntx = (c.n[0] + kCellTile - 1) / kCellTile;
    c.nty = (c.n[1] + kCellTile - 1) / kCellTile;
    c.vec = (L.vec_mask >> level) & 1;
    c.h = L.dx * (double)(1 << level); // exact
    return c;
}
__device__ __forceinline__ CellLevel cell_level_of_tile(const CellLevels &L, int tile, int &level)
{
    const int8_t *lab = L.lab[0];
    int tile0 = L.tile0[0];
    level = 0;
#pragma unroll
    for (int k = 1; k < AVS_MAX_LEVELS; ++k)
        if (tile >= L.tile0[k]) {
            lab = L.lab[k];
            tile0 = L.tile0[k];
            level = k;
        }
    return cell_level(L, level, lab, tile0);
}
__device__ __forceinline__ CellLevel cell_level_of_strip(const CellLevels &L, int strip, int &strip0)
{
    const int8_t *lab = L.lab[0];
    int tile0 = L.tile0[0], level = 0;
    strip0 = L.strip0[0];
#pragma unroll
    for (int k = 1; k < AVS_MAX_LEVELS; ++k)
        if (strip >= L.strip0[k]) {
            lab = L.lab[k];
            tile0 = L.tile0[k];
            strip0 = L.strip0[k];
            level = k;
        }
    return cell_level(L, level, lab, tile0);
}

// bit b = byte b of the word equals AVS_ACTIVE (exact for any byte value): zero-byte test of w ^ 0x01010101, then the four 0x80 flags
// gathered into a nibble by one multiplication (the partial products land on distinct bits: no carries)
__host__ __device__ __forceinline__ unsigned cell_active_nibble(uint32_t w)
{
    const uint32_t y = w ^ (0x01010101u * (uint32_t)AVS_ACTIVE);
    const uint32_t z = ~((((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y) | 0x7f7f7f7fu);
    return ((z >> 7) * 0x01020408u) >> 24;
}

// x-row r (0 .. 255) of tile (tx, ty, tz) holds the cells (16 tx + x, 16 ty + (r & 15), 16 tz + (r >> 4)).  Rows beyond the lattice (partial
// tiles) do not exist; the address is clamped into the lattice so that a load needs no branch and the loads of several rows are in
// flight together.
__device__ __forceinline__ const int8_t *cell_row(const CellLevel &Lv, int tx, int ty, int tz, int r, bool &exists)
{
    const int j = ty * kCellTile + (r & (kCellTile - 1)), k = tz * kCellTile + (r >> 4);
    exists = j < Lv.n[1] && k < Lv.n[2];
    const int jc = min(j, Lv.n[1] - 1), kc = min(k, Lv.n[2] - 1);
    return Lv.lab + ((size_t)Lv.n[0] * ((size_t)jc + (size_t)Lv.n[1] * (size_t)kc) + (size_t)tx * kCellTile);
}
// bit x of the mask = label x of the row piece is ACTIVE: from one 16-byte load / bytewise for the `ex` labels that exist
__device__ __forceinline__ unsigned cell_mask16(const uint4 &v)
{
    return cell_active_nibble(v.x) | cell_active_nibble(v.y) << 4 | cell_active_nibble(v.z) << 8 | cell_active_nibble(v.w) << 12;
}
__device__ __forceinline__ unsigned cell_mask_bytes(const int8_t *row, int ex)
{
    unsigned m = 0u;
#pragma unroll
    for (int x = 0; x < kCellTile; ++x)
        if (x < ex) m |= (row[x] == (int8_t)AVS_ACTIVE ? 1u : 0u) << x;
    return m;
}
__device__ __forceinline__ unsigned cell_row_mask(const CellLevel &Lv, int tx, int ty, int tz, int r)
{
    bool exists;
    const int8_t *row = cell_row(Lv, tx, ty, tz, r, exists);
    const unsigned m = Lv.vec ? cell_mask16(*reinterpret_cast<const uint4 *>(row)) : cell_mask_bytes(row, min(kCellTile, Lv.n[0] - tx * kCellTile));
    return exists ? m : 0u;
}

// Counts: persistent waves, one wave per STRIP of kCellStrip x-adjacent tiles.  Lane l reads piece (l & 7) of x-row 8 g + (l >> 3), g = 0 ..
// 31: eight lanes read one whole 128-byte line, four loads per lane in flight, no LDS and no barrier; the tiles' counts are the sums over
// the lanes with equal (l & 7).  (A workgroup per tile was dispatch-bound -- 300 k workgroups of one 4-KiB read each at 1024^3 -- and a
// wave per tile read 16 bytes of every line it touched, the other 112 going to waves on other XCDs: 0.7 and 1.5 TB/s.)
__global__ __launch_bounds__(kCellBlock) void k_cell_counts(CellLevels L, int32_t *__restrict__ counts, int32_t *__restrict__ list)
{
    const int lane = (int)threadIdx.x & 63, piece = lane & (kCellStrip - 1), rsub = lane >> 3;
    const int waves = (int)gridDim.x * (kCellBlock / 64);
    for (int w = (int)blockIdx.x * (kCellBlock / 64) + ((int)threadIdx.x >> 6); w < L.total_strips; w += waves) {
        const int gs = __builtin_amdgcn_readfirstlane(w); // wave-uniform: the level lookup stays on scalar registers
        int strip0;
        const CellLevel Lv = cell_level_of_strip(L, gs, strip0);
        const int nsx = (Lv.ntx + kCellStrip - 1) / kCellStrip, strip = gs - strip0;
        const int sx = strip % nsx, ty = (strip / nsx) % Lv.nty, tz = strip / (nsx * Lv.nty);
        const int tx = sx * kCellStrip + piece;
        const bool tile_exists = tx < Lv.ntx;      // (the last strip of a row of fewer than 8 tiles)
        const int txc = min(tx, Lv.ntx - 1);       // ... whose lanes read an existing tile and count nothing
        int c = 0;
        if (Lv.vec) {
            for (int g0 = 0; g0 < kCellBlock / 8; g0 += 4) {
                uint4 v[4];
                bool exists[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const uint4 *>(cell_row(Lv, txc, ty, tz, (g0 + q) * 8 + rsub, exists[q]));
#pragma unroll
                for (int q = 0; q < 4; ++q) c += exists[q] ? __popc(cell_mask16(v[q])) : 0;
            }
        } else {
            for (int g = 0; g < kCellBlock / 8; ++g) c += __popc(cell_row_mask(Lv, txc, ty, tz, g * 8 + rsub));
        }
        if (!tile_exists) c = 0;
#pragma unroll
        for (int o = kCellStrip; o < 64; o <<= 1) c += __shfl_xor(c, o, 64);
        const bool owner = lane < kCellStrip && tile_exists; // lanes 0 .. 7 hold the counts of the strip's tiles
        const int gt = Lv.tile0 + tx + Lv.ntx * (ty + Lv.nty * tz);
        if (owner) counts[gt] = c;
        const unsigned long long app = __ballot(owner && c > 0); // the non-empty ones join the list with one atomic per wave
        if (app) {
            const int first = __ffsll((long long)app) - 1;
            int base = 0;
            if (lane == first) base = atomicAdd(list, __popcll(app));
            base = __shfl(base, first, 64);
            if (owner && c > 0) list[1 + base + __popcll(app & ((1ull << lane) - 1ull))] = gt;
        }
    }
}

// kCellSumBlocks workgroups per level: partial[l * kCellSumBlocks + b] = ACTIVE cells in slice b of level l's tiles, 64-bit (the host
// adds the slices)
__global__ __launch_bounds__(kCellBlock) void k_cell_level_sums(CellLevels L, const int32_t *__restrict__ counts, long long *__restrict__ partial)
{
    __shared__ long long wsum[kCellBlock / 64];
    const int l = (int)blockIdx.y;
    int first = 0, last = 0;
#pragma unroll
    for (int k = 0; k < AVS_MAX_LEVELS; ++k)
        if (k == l) {
            first = L.tile0[k];
            last = k + 1 < AVS_MAX_LEVELS && L.tile0[k + 1] != INT_MAX ? L.tile0[k + 1] : L.total_tiles;
        }
    long long s = 0;
    for (int t = first + (int)(blockIdx.x * kCellBlock + threadIdx.x); t < last; t += kCellSumBlocks * kCellBlock) s += counts[t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[l * kCellSumBlocks + (int)blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// position / ijk: xyz interleaved; any output pointer may be null.  Records at or beyond `capacity` are never stored (the host has checked
// capacity >= the record count: the guard only keeps a lattice that changed under the call from writing out of bounds).
__global__ __launch_bounds__(kCellBlock) void k_cell_emit(CellLevels L, const int32_t *__restrict__ offsets, const int32_t *__restrict__ list, double ox,
                                                          double oy, double oz, long long capacity, float *__restrict__ position,
                                                          float *__restrict__ pscale, int32_t *__restrict__ level_out, int32_t *__restrict__ ijk)
{
    __shared__ int wsum[kCellBlock / 64];
    const int n_list = list[0];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int li = (int)blockIdx.x; li < n_list; li += (int)gridDim.x) {
        const int gt = list[1 + li];
        int level;
        const CellLevel Lv = cell_level_of_tile(L, gt, level);
        const int tile = gt - Lv.tile0;
        const int tx = tile % Lv.ntx, ty = (tile / Lv.ntx) % Lv.nty, tz = tile / (Lv.ntx * Lv.nty);
        unsigned m = cell_row_mask(Lv, tx, ty, tz, t);
        const int c = __popc(m);
        int incl = c; // cells of this wave's rows up to and including this lane's
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int before = incl - c;
#pragma unroll
        for (int w = 0; w < kCellBlock / 64; ++w)
            if (w < wave) before += wsum[w];
        long long rec = (long long)offsets[gt] + before;
        const int j = ty * kCellTile + (t & (kCellTile - 1)), k = tz * kCellTile + (t >> 4);
        const float py = (float)(oy + ((double)j + 0.5) * Lv.h), pz = (float)(oz + ((double)k + 0.5) * Lv.h), ps = (float)Lv.h;
        while (m) {
            const int i = tx * kCellTile + (__ffs(m) - 1);
            m &= m - 1u;
            if (rec < capacity) {
                if (position) {
                    position[3 * rec + 0] = (float)(ox + ((double)i + 0.5) * Lv.h);
                    position[3 * rec + 1] = py;
                    position[3 * rec + 2] = pz;
                }
                if (pscale) pscale[rec] = ps;
                if (level_out) level_out[rec] = level;
                if (ijk) {
                    ijk[3 * rec + 0] = i;
                    ijk[3 * rec + 1] = j;
                    ijk[3 * rec + 2] = k;
                }
            }
            ++rec;
        }
        __syncthreads(); // wsum is reused by the next tile
    }
}

// Shared implementation of avs_get_octree_cells / avs_prepass_get_octree_cells (protocol: include/avs.h).
avs_status export_octree_cells(CellsScratch &S, const CellsSource &src, hipStream_t st, const double *origin, int64_t capacity, float *position,
                               float *pscale, int32_t *level, int32_t *ijk, int64_t *n_cells, int64_t *per_level, avs_memspace where)
{
    *n_cells = 0;
    if (per_level)
        for (int l = 0; l < AVS_MAX_LEVELS; ++l) per_level[l] = 0;
    if (src.levels == 0) return AVS_OK;
    CellLevels L{};
    int64_t tiles = 0, strips = 0;
    for (int l = 0; l < AVS_MAX_LEVELS; ++l) {
        L.tile0[l] = L.strip0[l] = INT_MAX;
        if (l >= src.levels) continue;
        int n[3];
        for (int a = 0; a < 3; ++a) n[a] = src.n[a] >> l;
        AVS_REQUIRE(src.labels[l] && n[0] >= 1 && n[1] >= 1 && n[2] >= 1, AVS_EINTERNAL, "octree cells: level %d has no label lattice", l);
        L.lab[l] = src.labels[l];
        L.tile0[l] = (int)tiles;
        // a row piece is one 16-byte load where the x extent is a whole number of tiles and the lattice starts on a 16-byte boundary
        // (hipMalloc'ed lattices, the context's own copies and the pre-pass's lent ones alike, do)
        if (n[0] % kCellTile == 0 && (reinterpret_cast<uintptr_t>(src.labels[l]) & 15u) == 0) L.vec_mask |= 1 << l;
        L.strip0[l] = (int)strips;
        const int64_t ntx = (n[0] + kCellTile - 1) / kCellTile, ntyz = (int64_t)((n[1] + kCellTile - 1) / kCellTile) * ((n[2] + kCellTile - 1) / kCellTile);
        tiles += ntx * ntyz;
        strips += (ntx + kCellStrip - 1) / kCellStrip * ntyz;
        AVS_REQUIRE(tiles < INT_MAX, AVS_EINVAL, "octree cells: too many tiles for one call");
    }
    for (int a = 0; a < 3; ++a) L.n[a] = src.n[a];
    L.dx = src.dx;
    L.levels = src.levels;
    L.total_tiles = (int)tiles;
    L.total_strips = (int)strips;
    AVS_TRY(S.counts.reserve((size_t)tiles));
    AVS_TRY(S.list.reserve((size_t)tiles + 1));
    AVS_TRY(S.sums.reserve((size_t)AVS_MAX_LEVELS * kCellSumBlocks));
    AVS_HIP(hipMemsetAsync(S.list.p, 0, sizeof(int32_t), st));
    // persistent grids: eight (counts) / four (emit) workgroups per CU
    const int64_t count_wgs = (strips + kCellBlock / 64 - 1) / (kCellBlock / 64);
    const int64_t count_cap = src.grid_cap > 0 ? src.grid_cap : 2048, emit_cap = src.grid_cap > 0 ? src.grid_cap : 1024;
    hipLaunchKernelGGL(k_cell_counts, dim3((unsigned)(count_wgs < count_cap ? count_wgs : count_cap)), dim3(kCellBlock), 0, st, L, S.counts.p, S.list.p);
    hipLaunchKernelGGL(k_cell_level_sums, dim3(kCellSumBlocks, (unsigned)src.levels), dim3(kCellBlock), 0, st, L, (const int32_t *)S.counts.p, S.sums.p);
    AVS_HIP(hipGetLastError());
    std::vector<long long> partial((size_t)src.levels * kCellSumBlocks);
    AVS_HIP(hipMemcpyAsync(partial.data(), S.sums.p, partial.size() * sizeof(long long), hipMemcpyDeviceToHost, st));
    AVS_HIP(hipStreamSynchronize(st)); // the one wait the count needs
    int64_t n = 0;
    for (int l = 0; l < src.levels; ++l) {
        long long sum = 0;
        for (int b = 0; b < kCellSumBlocks; ++b) sum += partial[(size_t)l * kCellSumBlocks + b];
        n += sum;
        if (per_level) per_level[l] = sum;
    }
    *n_cells = n;
    if (capacity == 0 || n == 0) return AVS_OK;
    AVS_REQUIRE(n <= INT32_MAX, AVS_EINVAL, "octree cells: %lld cells, more than the 32-bit tile offsets of one call hold", (long long)n);
    AVS_REQUIRE(capacity >= n, AVS_EINVAL, "octree cells: capacity %lld is below the cell count %lld", (long long)capacity, (long long)n);
    float *dpos = position, *dps = pscale;
    int32_t *dlv = level, *dijk = ijk;
    const size_t nn = (size_t)n;
    if (where == AVS_MEM_HOST) { // staged: the kernel writes scratch kept in the object
        if (position) { AVS_TRY(S.pos.reserve(3 * nn)); dpos = S.pos.p; }
        if (pscale) { AVS_TRY(S.pscale.reserve(nn)); dps = S.pscale.p; }
        if (level) { AVS_TRY(S.level.reserve(nn)); dlv = S.level.p; }
        if (ijk) { AVS_TRY(S.ijk.reserve(3 * nn)); dijk = S.ijk.p; }
    }
    // the count fits the 32-bit tile offsets: now the scan (a count query never gets here)
    AVS_TRY(S.offsets.reserve((size_t)tiles + 1));
    AVS_TRY(S.scan_tmp.reserve(scan_tmp_elems(tiles)));
    AVS_TRY(exclusive_scan_i32(S.counts.p, S.offsets.p, tiles, S.scan_tmp.p, S.scan_tmp.n, st));
    const double o[3] = {origin ? origin[0] : 0., origin ? origin[1] : 0., origin ? origin[2] : 0.};
    const unsigned grid = (unsigned)(tiles < emit_cap ? tiles : emit_cap);
    hipLaunchKernelGGL(k_cell_emit, dim3(grid), dim3(kCellBlock), 0, st, L, (const int32_t *)S.offsets.p, (const int32_t *)S.list.p, o[0], o[1], o[2],
                       (long long)n, dpos, dps, dlv, dijk);
    AVS_HIP(hipGetLastError());
    if (where == AVS_MEM_HOST) {
        if (position) AVS_HIP(copy_out(position, dpos, 3 * nn * sizeof(float), where, st));
        if (pscale) AVS_HIP(copy_out(pscale, dps, nn * sizeof(float), where, st));
        if (level) AVS_HIP(copy_out(level, dlv, nn * sizeof(int32_t), where, st));
        if (ijk) AVS_HIP(copy_out(ijk, dijk, 3 * nn * sizeof(int32_t), where, st));
        AVS_HIP(hipStreamSynchronize(st));
    }
    return AVS_OK;
}

avs_status octree_cells_check_args(int64_t capacity, const int64_t *n_cells, avs_memspace where)
{
    AVS_REQUIRE(n_cells, AVS_EINVAL, "octree cells: n_cells must not be null");
    AVS_REQUIRE(capacity >= 0, AVS_EINVAL, "octree cells: negative capacity");
    AVS_REQUIRE(where == AVS_MEM_HOST || where == AVS_MEM_DEVICE, AVS_EINVAL, "octree cells: unknown memory space %d", (int)where);
    return AVS_OK;
}

} // namespace avs

using namespace avs;

extern "C" avs_status avs_get_octree_cells(avs_ctx *c, const double *origin, int64_t capacity, float *position, float *pscale, int32_t *level,
                                           int32_t *ijk, int64_t *n_cells, int64_t *per_level, avs_memspace where)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c, AVS_EINVAL, "null argument");
    AVS_TRY(octree_cells_check_args(capacity, n_cells, where));
    AVS_REQUIRE(!c->slab.on, AVS_ESTATE, "avs_get_octree_cells: the context holds a slab-local pre-pass (this rank's window only)");
    CellsSource src{};
    for (int l = 0; l < c->desc.levels; ++l) {
        AVS_REQUIRE(c->have_labels[l] && c->labels[l].p, AVS_ESTATE, "avs_get_octree_cells: labels of level %d missing (avs_set_labels / avs_prepass_apply)", l);
        src.labels[l] = c->labels[l].p;
    }
    src.levels = c->desc.levels;
    src.n[0] = c->desc.nx;
    src.n[1] = c->desc.ny;
    src.n[2] = c->desc.nz;
    src.dx = c->desc.dx;
    src.grid_cap = c->opt.cells_grid_cap;
    AVS_HIP(hipSetDevice(c->desc.device));
    Scope scope("Output Octree Geometry"); // oct.cpp:245
    return export_octree_cells(c->cells, src, c->stream, origin, capacity, position, pscale, level, ijk, n_cells, per_level, where);
}
