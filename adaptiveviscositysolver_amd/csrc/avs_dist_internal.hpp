// What the two halves of the multi-GPU layer share: avs_dist.hip (the transport: halo exchange, all-reduces, comm blocks, the C entry
// points) and avs_dist_plan.hip (the partition planners: a rank's plan and local system, built on the device).
#pragma once

#include <rccl/rccl.h>

#include "avs_internal.hpp"

struct avs_local_group; // the in-process group of virtual ranks: avs_dist.hip

namespace avs {

struct PcgDist {
    int rank = 0, world = 1;
    ncclComm_t comm = nullptr;     // all-reduces (solver stream)
    ncclComm_t comm_p2p = nullptr; // halo send/recv (communication stream): a communicator of its own, so that
                                   // operations in flight on two streams never share one communicator
    avs_local_group *group = nullptr;
    int device = 0;

    // plan
    int64_t n_global = 0, n_own = 0, n_halo = 0, n_send = 0, nnz_local = 0;
    std::vector<int32_t> peers, send_counts, recv_counts, send_offs, recv_offs;
    DevBuf<int32_t> send_idx, own_global;
    DevBuf<double> sendbuf;

    // local system
    DevBuf<int32_t> row_ptr, col;
    DevBuf<double> val, rhs, x0, x;
    ValueIndex vi;            // lossless storage form of the LOCAL rows (own dictionaries: the rank's rows hold a subset of the values)
    BrickForm brick;          // brick-structured form of the local rows (round 5; slabs of >= kBrickMinSystemRows rows), avs_brick_build.hip
    BrickView brick_view;
    DevBuf<int32_t> local_ref; // reference DOF id behind every local column [owned | halo] (what the brick builder reads the geometry from)
    PcgWork *pcg = nullptr;
    bool partitioned = false, solved = false, reordered = false;
    bool f32 = false; // AVS_PRECISION_F32 + AVS_OPTION_DIST_F32_VECTORS when this plan was made: the single-reduction loops run on float vectors
    bool resident_f32 = false; // ... + AVS_OPTION_RESIDENT_F32: the CU-resident loop between ranks runs on float vectors too
    bool mixed = false; // AVS_PRECISION_F64 + AVS_OPTION_DIST_MIXED_PRECISION when this plan was made: the single-reduction loops run on float
                        // vectors with fp64 scalars and reliable updates (the brick walk is laid out for the mixed kernel)
    DevBuf<double> recvbuf; // float halo exchange (RCCL / in-process): the peers' entries, widened, before they are narrowed into the vector
    // slab cuts along cut_axis (fine cells, world + 1 entries): the ones this assembly used, and the ones its per-plane weights suggest
    // for the next frame (slab-local assembly: the pre-pass needs the cuts BEFORE anything is counted)
    std::vector<int32_t> cuts, next_cuts;
    int cut_axis = 0;
    // the second set of the local arrays the [interior | halo-reading] row order is written to (swapped in; kept across frames: the
    // allocation of 170 MB of columns and values cost 3.6 ms of a 9-ms slab assembly, 19 ms the first time)
    // work arrays of the assembly (flags, scans, lookups, sort keys ...), kept across frames: twenty hipMalloc / hipFree pairs per
    // assembly were 2 ms of a 7-ms slab assembly
    struct Scratch {
        DevBuf<uint32_t> keys_in, keys_out, needed_by, pm;
        DevBuf<int32_t> dom, flag, pos, g2l, scan_tmp, ids, halo_tmp, tile_bnd, tile_int, tile_pos, w32, plane_owner, raw_count;
        DevBuf<uint16_t> plane;
        DevBuf<uint8_t> owner, is_halo;
        DevBuf<char> sort_tmp;
        DevBuf<int> mark_err;
        DevBuf<unsigned long long> weight;
    } ws;
    DevBuf<int32_t> alt_row_ptr, alt_col, alt_own, alt_ids, alt_new_of, alt_len;
    DevBuf<double> alt_val, alt_rhs;
    DevBuf<uint32_t> alt_nb;

    // direct transport (peer-mapped comm blocks), see avs_internal.hpp
    int transport = AVS_TRANSPORT_RCCL;
    bool hosted = false;          // neither RCCL communicator nor in-process group: the host program carries the blobs
    void *comm_block = nullptr;
    size_t comm_bytes = 0;
    void *peer_block[kMaxRanks] = {};
    bool peer_ipc[kMaxRanks] = {}; // mapped with hipIpcOpenMemHandle (to be closed)
    DevBuf<DistDev> dd;
    DevBuf<int32_t> push_seg;
    DevBuf<uint8_t> tile_flags;
    int push_grid = 0, push_chunk = 0;
    DevBuf<unsigned long long> epoch;
    DevBuf<unsigned> tickets;
    DevBuf<uint8_t> blob_send, blob_recv; // RCCL groups: staging of the blob all-gather ...
    DevBuf<int> vote_word;                // ... and of the transport votes (allocated once, at avs_dist_init)
    DevBuf<unsigned long long> psum; // paranoid mode: per-peer checksum accumulators of the push
    DistDev dd_host{};               // what d->dd holds (the self-test toggles `paranoid` around its rounds)
    bool exclusive_device = true;    // no other rank of the group on this physical GPU
    long long selftest_bad = -1;     // transport self-test of this plan: -1 not run, else the all-gathered count of bad entries
    int selftest_rounds = 0;
    std::vector<uint8_t> blob;
    bool direct_prepared = false, direct_ready = false;
    bool direct_pending = false; // a new plan exists: the (collective) transport set-up runs at the next avs_dist_solve

    // overlap of the exchange with the interior rows
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_ready = nullptr, ev_halo = nullptr;
    DevBuf<int32_t> tiles_int, tiles_bnd;
    int n_tiles_int = 0, n_tiles_bnd = 0;
    bool no_overlap = false;
};

static inline unsigned grid256(int64_t n) { return (unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1); }

template <typename T>
__global__ __launch_bounds__(256) void k_gather_i(const T *__restrict__ src, const int32_t *__restrict__ idx,
                                                  T *__restrict__ dst, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}

// avs_dist.hip
avs_status dist_allreduce_i32(PcgDist *d, int32_t *dev, int64_t count, hipStream_t stream);

// avs_dist_plan.hip: avs_dist_partition's plan (device / host planner), avs_dist_assemble's two assemblies, the brick form of their rows
avs_status plan_on_device(avs_ctx *c, PcgDist *d, int cut_axis, int extent, bool ro);
avs_status plan_on_host(avs_ctx *c, PcgDist *d, int cut_axis, int extent, bool ro);
avs_status dist_assemble_device(avs_ctx *c, PcgDist *d, int cut_axis, int extent);
avs_status dist_assemble_window(avs_ctx *c, PcgDist *d);
avs_status dist_build_brick(avs_ctx *c, PcgDist *d);

} // namespace avs
