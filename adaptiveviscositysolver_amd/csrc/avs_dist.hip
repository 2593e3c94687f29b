// avs_dist.hip -- multi-GPU layer of the PCG solve (no reference counterpart).
//
// One rank = one GPU = one process.  Each rank keeps the rows of the faces in its spatial slab
// (avs_partition.cpp), numbered [owned | halo grouped by owner].  Per CG iteration:
//   C1 halo exchange  pack owned p entries (k_pack) -> ncclSend / ncclRecv inside one group, the
//                     receive lands directly in the halo tail of p (no unpack kernel);
//   C2 all-reduce     ncclAllReduce(sum) of 1-2 fp64 scalars, in place in the device scalar block.
// Both are enqueued on the solver's stream: no host synchronisation inside the iteration.
// Messages are tiny (tens of KB / 8-16 B): the cost is launch + link latency, not xGMI bandwidth.
//
// For single-GPU testing the same code path runs over an in-process transport: "virtual ranks"
// (one avs_ctx and one host thread each, sharing one device) exchange through device-to-device
// copies and a host-side rendezvous.  Slow, but it executes the identical partition / halo /
// reduction logic and is what tests/test_gpu_dist.py checks against the single-rank solve.
//
// This file is the transport and the C entry points.  What a rank exchanges and solves -- its plan and its local system -- is built by
// the partition planners in avs_dist_plan.hip; avs_dist_internal.hpp holds PcgDist and the functions that cross between the two files.
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>

#include "avs_dist_internal.hpp"

struct avs_local_group {
    int world = 0;
    std::mutex m;
    std::condition_variable cv;
    int arrived = 0;
    long generation = 0;
    std::vector<avs::PcgDist *> members;
    std::vector<double> red; // world x 4 staging for all-reduce
    std::vector<int32_t> red_i32; // dist_allreduce_i32
    std::vector<uint8_t> blobs; // world x AVS_DIST_BLOB_BYTES: comm-block descriptors of the direct transport
    int direct_votes = 0;       // members whose direct_connect succeeded (agreement: all or none)
    bool failed = false;

    void barrier()
    {
        std::unique_lock<std::mutex> lk(m);
        const long gen = generation;
        if (++arrived == world) {
            arrived = 0;
            ++generation;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return generation != gen; });
        }
    }
};

namespace avs {

#define AVS_NCCL(call)                                                                                   \
    do {                                                                                                 \
        ncclResult_t r__ = (call);                                                                       \
        if (r__ != ncclSuccess) {                                                                        \
            ::avs::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, ncclGetErrorString(r__));      \
            return AVS_ERCCL;                                                                            \
        }                                                                                                \
    } while (0)

__global__ __launch_bounds__(256) void k_pack(const double *__restrict__ p, const int32_t *__restrict__ idx,
                                              double *__restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = p[idx[i]];
}

__global__ __launch_bounds__(256) void k_scatter_own(const double *__restrict__ x, const int32_t *__restrict__ own_global,
                                                     double *__restrict__ full, int64_t n_own)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_own) full[own_global[i]] = x[i];
}

template <typename T>
__global__ __launch_bounds__(256) void k_pack_wide(const T *__restrict__ p, const int32_t *__restrict__ idx, double *__restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (double)p[idx[i]];
}
__global__ __launch_bounds__(256) void k_unpack_narrow(const double *__restrict__ in, float *__restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (float)in[i];
}

// C1 after the pack: the peers' entries (doubles) land at `land` + recv_offs[i] -- through one NCCL group, or copied out of the peers'
// send buffers between two barriers of the in-process group; `narrow` (nullptr: none) then receives them as floats
static avs_status halo_transfer(PcgDist *d, double *land, float *narrow, hipStream_t stream)
{
    if (d->comm) {
        AVS_NCCL(ncclGroupStart());
        for (size_t i = 0; i < d->peers.size(); ++i) {
            if (d->send_counts[i])
                AVS_NCCL(ncclSend(d->sendbuf.p + d->send_offs[i], (size_t)d->send_counts[i], ncclDouble, d->peers[i], d->comm_p2p, stream));
            if (d->recv_counts[i])
                AVS_NCCL(ncclRecv(land + d->recv_offs[i], (size_t)d->recv_counts[i], ncclDouble, d->peers[i], d->comm_p2p, stream));
        }
        AVS_NCCL(ncclGroupEnd());
    } else { // in-process transport
        avs_local_group *g = d->group;
        AVS_REQUIRE(g, AVS_ESTATE, "multi-GPU layer not initialised");
        AVS_HIP(hipStreamSynchronize(stream)); // my send buffer is packed
        g->barrier();
        for (size_t i = 0; i < d->peers.size(); ++i) {
            if (!d->recv_counts[i]) continue;
            PcgDist *peer = g->members[(size_t)d->peers[i]];
            // where does the peer keep what it sends to me?
            int64_t off = -1;
            for (size_t j = 0; j < peer->peers.size(); ++j)
                if (peer->peers[j] == d->rank) off = peer->send_offs[j];
            AVS_REQUIRE(off >= 0, AVS_EINTERNAL, "peer %d has no send list for rank %d", d->peers[i], d->rank);
            AVS_HIP(hipMemcpyAsync(land + d->recv_offs[i], peer->sendbuf.p + off, (size_t)d->recv_counts[i] * sizeof(double),
                                   hipMemcpyDeviceToDevice, stream));
        }
    }
    if (narrow) {
        if (d->n_halo)
            hipLaunchKernelGGL(k_unpack_narrow, dim3((unsigned)((d->n_halo + 255) / 256)), dim3(256), 0, stream, (const double *)land, narrow,
                               d->n_halo);
        AVS_HIP(hipGetLastError());
    }
    if (d->comm) return AVS_OK;
    AVS_HIP(hipStreamSynchronize(stream));
    d->group->barrier(); // nobody repacks before everybody has copied
    return AVS_OK;
}

// C1: p_ext = [owned | halo]; fills the halo tail from the peers' owned entries
avs_status dist_halo_exchange(PcgDist *d, double *p_ext, hipStream_t stream)
{
    if (d->world == 1) return AVS_OK;
    if (d->n_send)
        hipLaunchKernelGGL(k_pack, dim3((unsigned)((d->n_send + 255) / 256)), dim3(256), 0, stream, p_ext, d->send_idx.p,
                           d->sendbuf.p, d->n_send);
    return halo_transfer(d, p_ext + d->n_own, nullptr, stream);
}

// the same for a float vector [owned | halo]: the entries travel widened to double through the send buffer (exact: they are floats),
// land in recvbuf and are narrowed into the tail
avs_status dist_halo_exchange(PcgDist *d, float *p_ext, hipStream_t stream)
{
    if (d->world == 1) return AVS_OK;
    AVS_TRY(d->recvbuf.reserve((size_t)(d->n_halo > 0 ? d->n_halo : 1)));
    if (d->n_send)
        hipLaunchKernelGGL(k_pack_wide<float>, dim3((unsigned)((d->n_send + 255) / 256)), dim3(256), 0, stream, (const float *)p_ext, d->send_idx.p,
                           d->sendbuf.p, d->n_send);
    return halo_transfer(d, d->recvbuf.p, p_ext + d->n_own, stream);
}

bool dist_tile_lists(PcgDist *d, const int32_t **t_int, int *n_int, const int32_t **t_bnd, int *n_bnd)
{
    if (!d || d->world <= 1 || d->no_overlap || !d->comm_stream || d->n_tiles_int + d->n_tiles_bnd == 0) return false;
    if (!cur_opt().dist_overlap) return false;
    *t_int = d->tiles_int.p; *n_int = d->n_tiles_int;
    *t_bnd = d->tiles_bnd.p; *n_bnd = d->n_tiles_bnd;
    return true;
}

// exchange on the communication stream, ordered after everything enqueued on main_stream so far
avs_status dist_halo_begin(PcgDist *d, double *p_ext, hipStream_t main_stream)
{
    AVS_HIP(hipEventRecord(d->ev_ready, main_stream));
    AVS_HIP(hipStreamWaitEvent(d->comm_stream, d->ev_ready, 0));
    AVS_TRY(dist_halo_exchange(d, p_ext, d->comm_stream));
    AVS_HIP(hipEventRecord(d->ev_halo, d->comm_stream));
    return AVS_OK;
}
avs_status dist_halo_end(PcgDist *d, hipStream_t main_stream)
{
    AVS_HIP(hipStreamWaitEvent(main_stream, d->ev_halo, 0));
    return AVS_OK;
}

// C2: in-place sum of `count` doubles (count <= 4) over all ranks
avs_status dist_allreduce(PcgDist *d, double *dev, int count, hipStream_t stream)
{
    if (d->world == 1) return AVS_OK;
    if (d->comm) {
        AVS_NCCL(ncclAllReduce(dev, dev, (size_t)count, ncclDouble, ncclSum, d->comm, stream));
        return AVS_OK;
    }
    avs_local_group *g = d->group;
    AVS_REQUIRE(g && count <= 4, AVS_ESTATE, "multi-GPU layer not initialised");
    double h[4] = {0, 0, 0, 0};
    AVS_HIP(hipMemcpyAsync(h, dev, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, stream));
    AVS_HIP(hipStreamSynchronize(stream));
    for (int k = 0; k < count; ++k) g->red[(size_t)d->rank * 4 + k] = h[k];
    g->barrier();
    double s[4] = {0, 0, 0, 0};
    for (int r = 0; r < g->world; ++r) // fixed rank order: every rank computes identical sums
        for (int k = 0; k < count; ++k) s[k] += g->red[(size_t)r * 4 + k];
    g->barrier();
    AVS_HIP(hipMemcpyAsync(dev, s, (size_t)count * sizeof(double), hipMemcpyHostToDevice, stream));
    AVS_HIP(hipStreamSynchronize(stream));
    return AVS_OK;
}

// in-place sum of `count` int32 over all ranks (slab-local pre-pass: per-tile DOF counts; slab-local assembly: per-plane weights)
avs_status dist_allreduce_i32(PcgDist *d, int32_t *dev, int64_t count, hipStream_t stream)
{
    if (d->world == 1 || count <= 0) return AVS_OK;
    if (d->comm) {
        AVS_NCCL(ncclAllReduce(dev, dev, (size_t)count, ncclInt32, ncclSum, d->comm, stream));
        return AVS_OK;
    }
    avs_local_group *g = d->group;
    AVS_REQUIRE(g, AVS_ESTATE, "no RCCL communicator and no in-process group: a hosted group sums through the caller's callback");
    std::vector<int32_t> mine((size_t)count);
    AVS_HIP(hipMemcpyAsync(mine.data(), dev, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    AVS_HIP(hipStreamSynchronize(stream));
    g->barrier();
    if (d->rank == 0) g->red_i32.assign((size_t)count, 0);
    g->barrier();
    for (int r = 0; r < g->world; ++r) { // rank after rank: integer sums do not depend on the order, the vector is shared
        if (r == d->rank)
            for (int64_t i = 0; i < count; ++i) g->red_i32[(size_t)i] += mine[(size_t)i];
        g->barrier();
    }
    AVS_HIP(hipMemcpyAsync(dev, g->red_i32.data(), (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    AVS_HIP(hipStreamSynchronize(stream));
    g->barrier(); // nobody clears the vector before everybody has copied it
    return AVS_OK;
}

// world > 1: one all-reduce per iteration instead of two (AVS_DIST_CG=standard keeps Eigen's loop)
bool dist_wants_single_reduction(PcgDist *d)
{
    if (!d || d->world <= 1) return false;
    return !cur_opt().dist_standard_cg;
}

// ---------------------------------------------------------------------------------------------
// Direct transport: set-up.  Each rank allocates its comm block (fine-grained device memory: header + halo area),
// describes it in a blob (IPC handle, pid, raw pointer, where each peer's entries land), the blobs travel (RCCL
// all-gather / in-process group / the host program), every rank maps its peers' blocks and fills its DistDev.
// ---------------------------------------------------------------------------------------------
struct DistBlob {
    uint32_t magic;
    int32_t rank, pid, device;
    uint64_t raw_ptr, bytes;
    int64_t n_halo;
    uint64_t nonce;                 // of the exporting PROCESS: pids alone collide across pid namespaces (containers on one node)
    int32_t recv_off_of[kMaxRanks]; // offset inside my halo area where rank q's entries land (-1: none)
    int32_t recv_cnt_of[kMaxRanks];
    int32_t send_cnt_of[kMaxRanks]; // what I send to rank q: every rank can check every pair from the gathered blobs
    hipIpcMemHandle_t handle;
    int32_t have_handle;
    int32_t pci;                    // physical GPU: domain << 16 | bus << 8 | device (two ranks on one GPU cannot both run the CU-resident loop)
};
static_assert(sizeof(DistBlob) <= AVS_DIST_BLOB_BYTES, "blob does not fit");

// one random 64-bit number per process (not per context): "same process" = same nonce AND same pid
static uint64_t process_nonce()
{
    static const uint64_t nonce = [] {
        uint64_t v = 0;
        if (FILE *f = fopen("/dev/urandom", "rb")) {
            if (fread(&v, sizeof(v), 1, f) != 1) v = 0;
            fclose(f);
        }
        if (!v) { // no urandom: address-space layout + clock + pid
            timespec ts{};
            clock_gettime(CLOCK_REALTIME, &ts);
            v = (uint64_t)(uintptr_t)&v ^ ((uint64_t)ts.tv_nsec << 20) ^ ((uint64_t)ts.tv_sec << 44) ^ (uint64_t)getpid() * 0x9E3779B97F4A7C15ull;
        }
        return v | 1ull; // never 0: a zeroed blob is never "this process"
    }();
    return nonce;
}
static bool same_process(const DistBlob &a, const DistBlob &b) { return a.pid == b.pid && a.nonce == b.nonce && a.nonce != 0; }
constexpr uint32_t kBlobMagic = 0x41565342u; // "AVSB"
constexpr size_t kHeaderBytes = (sizeof(CommHeader) + 255) & ~(size_t)255;

static void direct_release(PcgDist *d)
{
    for (int q = 0; q < kMaxRanks; ++q) {
        if (d->peer_block[q] && d->peer_ipc[q]) (void)hipIpcCloseMemHandle(d->peer_block[q]);
        d->peer_block[q] = nullptr;
        d->peer_ipc[q] = false;
    }
    if (d->comm_block) (void)hipFree(d->comm_block);
    d->comm_block = nullptr;
    d->comm_bytes = 0;
    d->direct_prepared = d->direct_ready = false;
    d->transport = AVS_TRANSPORT_RCCL;
}

// allocates the comm block for the current plan and fills d->blob
static avs_status direct_prepare(avs_ctx *c, PcgDist *d)
{
    direct_release(d);
    AVS_HIP(hipSetDevice(c->desc.device));
    const size_t bytes = kHeaderBytes + (size_t)(d->n_halo > 0 ? d->n_halo : 1) * sizeof(double);
    void *p = nullptr;
    hipError_t e = hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained);
    if (e != hipSuccess || !p) {
        (void)hipGetLastError();
        set_error("direct transport: fine-grained allocation of %zu bytes failed (%s)", bytes, hipGetErrorString(e));
        return AVS_ENOMEM;
    }
    d->comm_block = p;
    d->comm_bytes = bytes;
    AVS_HIP(hipMemset(p, 0, bytes));
    AVS_HIP(hipMemset((char *)p + offsetof(CommHeader, red), 0xFF, sizeof(CommHeader::red))); // partial-sum slots: armed (sentinel)
    DistBlob b;
    memset(&b, 0, sizeof(b));
    b.magic = kBlobMagic;
    b.rank = d->rank;
    b.pid = (int32_t)getpid();
    b.nonce = process_nonce();
    b.device = c->desc.device;
    {
        int dom = 0, bus = 0, dv = 0;
        (void)hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, c->desc.device);
        (void)hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, c->desc.device);
        (void)hipDeviceGetAttribute(&dv, hipDeviceAttributePciDeviceId, c->desc.device);
        (void)hipGetLastError();
        b.pci = (dom << 16) | ((bus & 0xff) << 8) | (dv & 0xff);
    }
    b.raw_ptr = (uint64_t)(uintptr_t)p;
    b.bytes = bytes;
    b.n_halo = d->n_halo;
    for (int q = 0; q < kMaxRanks; ++q) { b.recv_off_of[q] = -1; b.recv_cnt_of[q] = 0; b.send_cnt_of[q] = 0; }
    for (size_t i = 0; i < d->peers.size(); ++i) {
        if (d->recv_counts[i] > 0) {
            b.recv_off_of[d->peers[i]] = d->recv_offs[i];
            b.recv_cnt_of[d->peers[i]] = d->recv_counts[i];
        }
        b.send_cnt_of[d->peers[i]] = d->send_counts[i];
    }
    if (d->world > 1 && hipIpcGetMemHandle(&b.handle, p) == hipSuccess) b.have_handle = 1; // peers in this process need none
    else (void)hipGetLastError();
    d->blob.assign(AVS_DIST_BLOB_BYTES, 0);
    memcpy(d->blob.data(), &b, sizeof(b));
    AVS_TRY(d->dd.alloc(1));
    AVS_TRY(d->epoch.alloc(1));
    AVS_TRY(d->tickets.alloc(2));
    AVS_TRY(d->psum.alloc(kMaxRanks));
    AVS_HIP(hipMemset(d->epoch.p, 0, sizeof(unsigned long long)));
    AVS_HIP(hipMemset(d->tickets.p, 0, 2 * sizeof(unsigned)));
    AVS_HIP(hipMemset(d->psum.p, 0, kMaxRanks * sizeof(unsigned long long)));
    d->direct_prepared = true;
    return AVS_OK;
}

// what I send to q must be what q expects from me (both sides derived their lists independently from the symmetric pattern):
// a mismatch fails here, with a status, instead of hanging in the first exchange -- whatever the transport
static avs_status check_exchange_counts(PcgDist *d, const uint8_t *blobs)
{
    // EVERY pair, from the gathered blobs only: all ranks see the same blobs, so all ranks return the same status (a rank-local
    // verdict would leave the others waiting in the next collective)
    for (int a = 0; a < d->world; ++a)
        for (int q = 0; q < d->world; ++q) {
            if (q == a) continue;
            DistBlob ba, bq;
            memcpy(&ba, blobs + (size_t)a * AVS_DIST_BLOB_BYTES, sizeof(ba));
            memcpy(&bq, blobs + (size_t)q * AVS_DIST_BLOB_BYTES, sizeof(bq));
            if (ba.magic != kBlobMagic || bq.magic != kBlobMagic) continue; // a rank without a block: nothing to compare with
            AVS_REQUIRE(ba.send_cnt_of[q] == bq.recv_cnt_of[a], AVS_EINTERNAL, "rank %d sends %d halo entries to rank %d, which expects %d", a,
                        ba.send_cnt_of[q], q, bq.recv_cnt_of[a]);
        }
    return AVS_OK;
}

// maps the peers' blocks and fills the device-side descriptor; `blobs` = world x AVS_DIST_BLOB_BYTES in rank order
static avs_status direct_connect(avs_ctx *c, PcgDist *d, const uint8_t *blobs, bool check_counts = true)
{
    AVS_REQUIRE(d->direct_prepared, AVS_ESTATE, "direct transport: no comm block (assemble / partition first)");
    AVS_HIP(hipSetDevice(c->desc.device));
    std::vector<DistBlob> all((size_t)d->world);
    for (int q = 0; q < d->world; ++q) {
        memcpy(&all[(size_t)q], blobs + (size_t)q * AVS_DIST_BLOB_BYTES, sizeof(DistBlob));
        AVS_REQUIRE(all[(size_t)q].magic == kBlobMagic && all[(size_t)q].rank == q, AVS_EINVAL, "direct transport: blob %d is not rank %d's", q, q);
    }
    if (check_counts) AVS_TRY(check_exchange_counts(d, blobs)); // (the loop-back measurement aid hands in synthetic blobs)
    const DistBlob &me = all[(size_t)d->rank];
    for (int q = 0; q < d->world; ++q) {
        if (q == d->rank) { d->peer_block[q] = d->comm_block; continue; }
        const DistBlob &b = all[(size_t)q];
        if (same_process(b, me) && me.nonce == process_nonce()) { // same process (in-process group): the pointer itself, peer access when on another GPU
            if (b.device != c->desc.device) {
                const hipError_t e = hipDeviceEnablePeerAccess(b.device, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
                    set_error("direct transport: no peer access from device %d to %d (%s)", c->desc.device, b.device, hipGetErrorString(e));
                    return AVS_EHIP;
                }
                (void)hipGetLastError();
            }
            d->peer_block[q] = (void *)(uintptr_t)b.raw_ptr;
        } else {
            AVS_REQUIRE(b.have_handle, AVS_EHIP, "direct transport: rank %d could not export its comm block", q);
            void *m = nullptr;
            const hipError_t e = hipIpcOpenMemHandle(&m, b.handle, hipIpcMemLazyEnablePeerAccess);
            if (e != hipSuccess || !m) {
                (void)hipGetLastError();
                set_error("direct transport: hipIpcOpenMemHandle(rank %d) failed: %s", q, hipGetErrorString(e));
                return AVS_EHIP;
            }
            d->peer_block[q] = m;
            d->peer_ipc[q] = true;
        }
    }
    DistDev h;
    memset(&h, 0, sizeof(h));
    h.rank = d->rank;
    h.world = d->world;
    h.npeers = (int)d->peers.size();
    h.n_own = d->n_own;
    h.mine = (CommHeader *)d->comm_block;
    h.my_halo = (const double *)((char *)d->comm_block + kHeaderBytes);
    AVS_REQUIRE(h.npeers <= kMaxRanks, AVS_EINVAL, "too many peers");
    for (int i = 0; i < h.npeers; ++i) {
        const int q = d->peers[(size_t)i];
        h.peer_rank[i] = q;
        h.send_off[i] = d->send_offs[(size_t)i];
        h.recv_cnt[i] = d->recv_counts[(size_t)i];
        h.recv_off[i] = d->recv_offs[(size_t)i];
        const int off = all[(size_t)q].recv_off_of[d->rank];
        h.peer_halo_dst[i] = (double *)((char *)d->peer_block[q] + kHeaderBytes) + (off > 0 ? off : 0);
        h.peer_hflag_dst[i] = &((CommHeader *)d->peer_block[q])->hflag[d->rank];
        h.peer_hsum_dst[i] = &((CommHeader *)d->peer_block[q])->hsum[d->rank];
    }
    h.send_off[h.npeers] = (int)d->n_send;
    for (int q = 0; q < d->world; ++q) {
        CommHeader *hq = (CommHeader *)d->peer_block[q];
        h.all_red_dst[q] = &hq->red[0][d->rank][0];
    }
    h.send_idx = d->send_idx.p;
    h.psum = d->psum.p;
    h.inject_stale_round = -1;
    h.paranoid = cur_opt().paranoid != 0;
#ifdef AVS_PROBES
    if (const char *e = getenv("AVS_DIST_INJECT_STALE")) { // test hook: proves the paranoid check sees a stale entry
        h.inject_stale_round = atoll(e);
        h.paranoid = 1;
    }
#endif
    // segments of the send lists per workgroup of the fused update + push kernel (send lists are ascending local row ids)
    {
        sr_update_geometry((long long)d->n_own, &d->push_grid, &d->push_chunk);
        const int G = d->push_grid;
        std::vector<int32_t> sidx((size_t)d->n_send), seg((size_t)(h.npeers > 0 ? h.npeers : 1) * (size_t)(G + 1), 0);
        if (d->n_send) AVS_HIP(hipMemcpy(sidx.data(), d->send_idx.p, sidx.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        std::vector<char> has((size_t)G, 0);
        for (int i = 0; i < h.npeers; ++i) {
            const int32_t *lo = sidx.data() + h.send_off[i], *hi = sidx.data() + h.send_off[i + 1];
            for (int b = 0; b <= G; ++b) {
                const long long first_row = (long long)b * d->push_chunk;
                const int32_t *it = std::lower_bound(lo, hi, first_row, [](int32_t v, long long key) { return (long long)v < key; });
                seg[(size_t)i * (G + 1) + b] = (int32_t)(it - sidx.data());
            }
            for (int b = 0; b < G; ++b)
                if (seg[(size_t)i * (G + 1) + b + 1] > seg[(size_t)i * (G + 1) + b]) has[(size_t)b] = 1;
        }
        int nblocks = 0;
        for (int b = 0; b < G; ++b) nblocks += has[(size_t)b];
        h.n_send_blocks = nblocks;
        AVS_TRY(d->push_seg.alloc(seg.size()));
        AVS_HIP(hipMemcpy(d->push_seg.p, seg.data(), seg.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        h.push_seg = d->push_seg.p;
        h.push_grid = G;
        h.push_chunk = d->push_chunk;
    }
    { // per-tile flag: does the tile read halo columns? (from the plan's list of such tiles)
        const int nt = d->n_tiles_int + d->n_tiles_bnd;
        std::vector<uint8_t> f((size_t)(nt > 0 ? nt : 1), 0);
        std::vector<int32_t> tb((size_t)d->n_tiles_bnd);
        if (d->n_tiles_bnd) AVS_HIP(hipMemcpy(tb.data(), d->tiles_bnd.p, tb.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int32_t t : tb) f[(size_t)t] = 1;
        AVS_TRY(d->tile_flags.alloc(f.size()));
        AVS_HIP(hipMemcpy(d->tile_flags.p, f.data(), f.size(), hipMemcpyHostToDevice));
    }
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->desc.device) != hipSuccess || khz <= 0) {
        (void)hipGetLastError();
        khz = 100000; // 100 MHz constant clock
    }
    long long ms = 20000;
    if (cur_opt().dist_timeout_ms > 0) ms = cur_opt().dist_timeout_ms;
    h.timeout_ticks = (long long)khz * ms;
    AVS_HIP(hipMemcpy(d->dd.p, &h, sizeof(h), hipMemcpyHostToDevice));
    d->dd_host = h;
    d->exclusive_device = true;
    for (int q = 0; q < d->world; ++q)
        if (q != d->rank && all[(size_t)q].pci == me.pci && check_counts) d->exclusive_device = false; // (loop-back: the "peers" are this rank itself)
    d->direct_ready = true;
    d->transport = AVS_TRANSPORT_DIRECT;
    d->selftest_bad = -1;
    d->selftest_rounds = 0;
    return AVS_OK;
}

bool dist_direct_args(PcgDist *d, DirectArgs *out)
{
    if (!d || !d->direct_ready) return false;
    out->dd = d->dd.p;
    out->epoch = d->epoch.p;
    out->push_ticket = d->tickets.p;
    out->fin_ticket = d->tickets.p + 1;
    out->n_send = (int)d->n_send;
    out->npeers = (int)d->peers.size();
    out->push_grid = d->push_grid;
    out->push_chunk = d->push_chunk;
    out->tiles_int = d->tiles_int.p;
    out->tiles_bnd = d->tiles_bnd.p;
    out->n_tiles_int = d->n_tiles_int;
    out->n_tiles_bnd = d->n_tiles_bnd;
    out->tile_flags = d->tile_flags.p;
    out->exclusive_device = d->exclusive_device;
    out->paranoid = d->dd_host.paranoid != 0;
    return true;
}

// Transport self-test (avs_pcg.hip: direct_selftest).  Runs with `paranoid` forced on, then restores the plan's setting.  Returns
// AVS_OK when the rounds ran; *passed tells whether every entry of every round arrived intact and in time ON EVERY RANK (the
// count is all-gathered through the comm blocks, so all ranks agree without another collective).  AVS_DIST_SELFTEST_ROUNDS=0 skips.
static avs_status run_selftest(avs_ctx *c, PcgDist *d, bool *passed)
{
    *passed = true;
    int rounds = cur_opt().dist_selftest_rounds;
    if (cur_opt().dist_loopback) rounds = 0; // a looped-back rank never fills its halo area
    if (rounds <= 0 || !d->direct_ready) return AVS_OK;
    DirectArgs da;
    if (!dist_direct_args(d, &da)) return AVS_OK;
    DistDev h = d->dd_host;
    const int keep_paranoid = h.paranoid;
    h.paranoid = 1;
    AVS_HIP(hipMemcpyAsync(d->dd.p, &h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    long long bad = 0;
    int fault = 0;
    const avs_status st = direct_selftest(da, rounds, c->stream, &bad, &fault);
    h.paranoid = keep_paranoid;
    AVS_HIP(hipMemcpyAsync(d->dd.p, &h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    AVS_HIP(hipStreamSynchronize(c->stream));
    AVS_TRY(st);
    d->selftest_rounds = rounds;
    d->selftest_bad = fault ? -2 : bad;
    *passed = fault == 0 && bad == 0;
    if (!*passed)
        set_error("direct transport self-test failed on rank %d: %lld bad halo entries / checksums in %d rounds, fault %d", d->rank, bad, rounds, fault);
    return AVS_OK;
}

// after a plan exists: choose the transport, exchange the blobs, connect -- all ranks end up with the SAME transport
static avs_status direct_setup(avs_ctx *c, PcgDist *d)
{
    const bool forced = cur_opt().transport == 2;
    const bool off = cur_opt().transport == 1;
    direct_release(d);
    if (d->hosted) { // the host program finishes the set-up (avs_dist_export_blob / avs_dist_import_blobs)
        AVS_REQUIRE(!off, AVS_EINVAL, "a hosted group has no RCCL communicator: AVS_DIST_TRANSPORT=rccl is impossible");
        return direct_prepare(c, d);
    }
    avs_status st = direct_prepare(c, d); // the blobs also carry the send / receive counts every transport must agree on
    std::vector<uint8_t> all((size_t)d->world * AVS_DIST_BLOB_BYTES, 0);
    int ok = st == AVS_OK ? 1 : 0;
    if (d->world == 1) {
        if (ok) memcpy(all.data(), d->blob.data(), AVS_DIST_BLOB_BYTES);
    } else if (d->group) {
        avs_local_group *g = d->group;
        {
            std::lock_guard<std::mutex> lk(g->m);
            if (g->blobs.size() != all.size()) g->blobs.assign(all.size(), 0);
            if (ok) memcpy(g->blobs.data() + (size_t)d->rank * AVS_DIST_BLOB_BYTES, d->blob.data(), AVS_DIST_BLOB_BYTES);
            else memset(g->blobs.data() + (size_t)d->rank * AVS_DIST_BLOB_BYTES, 0, AVS_DIST_BLOB_BYTES);
        }
        g->barrier();
        {
            std::lock_guard<std::mutex> lk(g->m);
            all = g->blobs;
        }
        g->barrier();
    } else if (d->comm) {
        DevBuf<uint8_t> &send = d->blob_send, &recv = d->blob_recv; // (allocated in avs_dist_init: no allocation between collectives)
        AVS_REQUIRE(send.p && recv.n >= all.size(), AVS_EINTERNAL, "blob staging was not allocated at avs_dist_init");
        if (!ok) d->blob.assign(AVS_DIST_BLOB_BYTES, 0);
        AVS_HIP(hipMemcpyAsync(send.p, d->blob.data(), AVS_DIST_BLOB_BYTES, hipMemcpyHostToDevice, c->stream));
        AVS_NCCL(ncclAllGather(send.p, recv.p, AVS_DIST_BLOB_BYTES, ncclUint8, d->comm, c->stream));
        AVS_HIP(hipMemcpyAsync(all.data(), recv.p, all.size(), hipMemcpyDeviceToHost, c->stream));
        AVS_HIP(hipStreamSynchronize(c->stream));
    } else {
        return AVS_OK;
    }
    if (d->world > 1) AVS_TRY(check_exchange_counts(d, all.data())); // (decided from the gathered blobs: the same status on every rank)
    if (off) { // RCCL transport requested: the comm block is not needed
        direct_release(d);
        return AVS_OK;
    }
    // Every decision below is taken from the GATHERED blobs (identical on all ranks), never from a rank-local result, so that no
    // rank leaves while the others enter the vote: a blob without the magic = that rank could not prepare a block = nobody connects.
    bool every = true, shared_device = false;
    for (int a = 0; a < d->world; ++a) {
        DistBlob ba;
        memcpy(&ba, all.data() + (size_t)a * AVS_DIST_BLOB_BYTES, sizeof(ba));
        if (ba.magic != kBlobMagic) { every = false; continue; }
        // Ranks of ONE process on ONE device (virtual ranks, a test set-up) share that device's few hardware queues: the
        // waiting kernel of one rank can sit in the same queue in front of the kernel it waits for (measured:
        // tools/probes/spin_probe.hip, only as many streams as hardware queues make progress).  Such groups keep the
        // host-mediated transport unless AVS_DIST_TRANSPORT=direct insists.
        for (int b2 = a + 1; b2 < d->world; ++b2) {
            DistBlob bb;
            memcpy(&bb, all.data() + (size_t)b2 * AVS_DIST_BLOB_BYTES, sizeof(bb));
            if (bb.magic == kBlobMagic && same_process(ba, bb) && ba.device == bb.device) shared_device = true;
        }
    }
    if (!every || (shared_device && !forced)) {
        direct_release(d);
        if (!every && forced) {
            set_error("direct transport: a rank could not allocate / export its comm block");
            return st != AVS_OK ? st : AVS_ERCCL;
        }
        return AVS_OK;
    }
    st = direct_connect(c, d, all.data());
    ok = st == AVS_OK ? 1 : 0;
    // agreement: one rank that cannot connect sends everybody back to the RCCL transport.  (The vote's device word is allocated
    // before the collective is entered; an allocation failure there is reported as a "no" vote through a host-side 0.)
    auto vote = [&](int mine, int *all_ok) -> avs_status {
        *all_ok = mine;
        if (d->world > 1 && d->group) {
            avs_local_group *g = d->group;
            {
                std::lock_guard<std::mutex> lk(g->m);
                if (d->rank == 0) g->direct_votes = 0;
            }
            g->barrier();
            {
                std::lock_guard<std::mutex> lk(g->m);
                g->direct_votes += mine;
            }
            g->barrier();
            {
                std::lock_guard<std::mutex> lk(g->m);
                *all_ok = g->direct_votes == d->world;
            }
            g->barrier();
        } else if (d->world > 1 && d->comm) {
            AVS_HIP(hipMemcpyAsync(d->vote_word.p, &mine, sizeof(int), hipMemcpyHostToDevice, c->stream));
            AVS_NCCL(ncclAllReduce(d->vote_word.p, d->vote_word.p, 1, ncclInt32, ncclMin, d->comm, c->stream));
            AVS_HIP(hipMemcpyAsync(all_ok, d->vote_word.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
            AVS_HIP(hipStreamSynchronize(c->stream));
        }
        return AVS_OK;
    };
    int all_ok = ok;
    AVS_TRY(vote(ok, &all_ok));
    if (all_ok) {
        // every rank is connected: prove the links before a solve depends on them.  The rounds rendezvous through the comm blocks
        // themselves; the bad-entry count is all-gathered there, and one more vote covers a rank whose rounds timed out.
        bool passed = true;
        const avs_status ts = run_selftest(c, d, &passed);
        int pass_all = (ts == AVS_OK && passed) ? 1 : 0;
        AVS_TRY(vote(pass_all, &pass_all));
        if (!pass_all) {
            all_ok = 0;
            if (st == AVS_OK) st = AVS_ERCCL;
        }
    }
    if (!all_ok) {
        if (forced) {
            if (ok && st == AVS_OK) set_error("direct transport: another rank could not connect");
            return st != AVS_OK ? st : AVS_ERCCL;
        }
        direct_release(d); // quietly: the RCCL / host-mediated transport takes over
    }
    return AVS_OK;
}

void dist_release(avs_ctx *c)
{
    PcgDist *d = c->dist;
    if (!d) return;
    direct_release(d);
    pcg_destroy(d->pcg);
    if (d->comm_p2p && d->comm_p2p != d->comm) (void)ncclCommDestroy(d->comm_p2p);
    if (d->comm) (void)ncclCommDestroy(d->comm);
    if (d->comm_stream) (void)hipStreamDestroy(d->comm_stream);
    if (d->ev_ready) (void)hipEventDestroy(d->ev_ready);
    if (d->ev_halo) (void)hipEventDestroy(d->ev_halo);
    delete d;
    c->dist = nullptr;
}

} // namespace avs

using namespace avs;

extern "C" {

avs_status avs_get_dof_table(avs_ctx *c, avs_index_kind kind, int32_t *table, avs_memspace where)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c && table, AVS_EINVAL, "null argument");
    AVS_REQUIRE(c->tables_ready, AVS_ESTATE, "dof tables not built: call avs_assemble first");
    AVS_HIP(hipSetDevice(c->desc.device));
    const LatBuf<int32_t> &t = kind == AVS_INDEX_VELOCITY ? c->vdof : (kind == AVS_INDEX_EDGE ? c->edof : c->cdof);
    const int64_t n = kind == AVS_INDEX_VELOCITY ? c->n_vel : (kind == AVS_INDEX_EDGE ? c->n_edge : c->n_center);
    AVS_HIP(copy_out(table, t.p, (size_t)n * 4 * sizeof(int32_t), where, c->stream));
    AVS_HIP(hipStreamSynchronize(c->stream));
    return AVS_OK;
}

avs_status avs_dist_get_unique_id(uint8_t id[AVS_UNIQUE_ID_BYTES])
{
    AVS_REQUIRE(id, AVS_EINVAL, "null argument");
    static_assert(sizeof(ncclUniqueId) <= AVS_UNIQUE_ID_BYTES, "unique id does not fit");
    ncclUniqueId u;
    AVS_NCCL(ncclGetUniqueId(&u));
    memset(id, 0, AVS_UNIQUE_ID_BYTES);
    memcpy(id, &u, sizeof(u));
    return AVS_OK;
}

static avs_status new_dist(avs_ctx *c, int rank, int world)
{
    AVS_REQUIRE(c, AVS_EINVAL, "null argument");
    AVS_REQUIRE(world >= 1 && world <= 32 && rank >= 0 && rank < world, AVS_EINVAL, "rank %d / world %d out of range", rank, world);
    dist_release(c);
    c->dist = new (std::nothrow) PcgDist();
    AVS_REQUIRE(c->dist, AVS_ENOMEM, "out of host memory");
    c->dist->rank = rank;
    c->dist->world = world;
    c->dist->device = c->desc.device;
    return AVS_OK;
}

avs_status avs_dist_init(avs_ctx *c, const uint8_t id[AVS_UNIQUE_ID_BYTES], int32_t rank, int32_t world)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c && id, AVS_EINVAL, "null argument");
    AVS_HIP(hipSetDevice(c->desc.device));
    AVS_TRY(new_dist(c, rank, world));
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    AVS_TRY(c->dist->blob_send.alloc(AVS_DIST_BLOB_BYTES)); // staging of the transport set-up collectives: allocated here, so that no
    AVS_TRY(c->dist->blob_recv.alloc((size_t)world * AVS_DIST_BLOB_BYTES)); // rank can fail an allocation BETWEEN two collectives
    AVS_TRY(c->dist->vote_word.alloc(1));
    AVS_NCCL(ncclCommInitRank(&c->dist->comm, world, u, rank));
    // second communicator for the point-to-point traffic (same ranks); without it the exchange shares
    // `comm` and stays on the solver stream (no overlap)
    if (ncclCommSplit(c->dist->comm, 0, rank, &c->dist->comm_p2p, nullptr) != ncclSuccess || !c->dist->comm_p2p) {
        c->dist->comm_p2p = c->dist->comm;
        c->dist->no_overlap = true;
    }
    return AVS_OK;
}

avs_status avs_local_group_create(int32_t world, avs_local_group **out)
{
    AVS_REQUIRE(out && world >= 1 && world <= 32, AVS_EINVAL, "bad argument");
    avs_local_group *g = new (std::nothrow) avs_local_group();
    AVS_REQUIRE(g, AVS_ENOMEM, "out of host memory");
    g->world = world;
    g->members.assign((size_t)world, nullptr);
    g->red.assign((size_t)world * 4, 0.);
    *out = g;
    return AVS_OK;
}

void avs_local_group_destroy(avs_local_group *g) { delete g; }

avs_status avs_dist_init_local(avs_ctx *c, avs_local_group *g, int32_t rank)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c && g, AVS_EINVAL, "null argument");
    AVS_TRY(new_dist(c, rank, g->world));
    c->dist->group = g;
    std::lock_guard<std::mutex> lk(g->m);
    g->members[(size_t)rank] = c->dist;
    return AVS_OK;
}

avs_status avs_dist_init_hosted(avs_ctx *c, int32_t rank, int32_t world)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c, AVS_EINVAL, "null argument");
    AVS_TRY(new_dist(c, rank, world));
    c->dist->hosted = true;
    return AVS_OK;
}

avs_status avs_dist_export_blob(avs_ctx *c, uint8_t blob[AVS_DIST_BLOB_BYTES])
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c && blob, AVS_EINVAL, "null argument");
    AVS_REQUIRE(c->dist && c->dist->direct_prepared, AVS_ESTATE, "no comm block: call avs_dist_assemble / avs_dist_partition first");
    memcpy(blob, c->dist->blob.data(), AVS_DIST_BLOB_BYTES);
    return AVS_OK;
}

// Measurement aid (tools/loopback_scaling.py): ONE rank of a world-size-W partition runs alone on one GPU with its peers
// looped back onto itself -- it pushes its boundary entries (into a scratch area of its own block), raises the flags its peers
// would raise, and all-gathers with itself.  Its halo values stay 0, so it solves a different (still SPD) system; what is
// representative is the TIME of an iteration of that rank's slab: real update + push + interior / halo-touching tiles +
// finalisation with W contributions, minus the xGMI latency.  Never used by a solve that is meant to be right.
static avs_status direct_connect_loopback(avs_ctx *c, PcgDist *d)
{
    AVS_REQUIRE(d->direct_prepared, AVS_ESTATE, "no comm block (assemble / partition first)");
    AVS_HIP(hipSetDevice(c->desc.device));
    // re-allocate the block with a scratch tail for the pushes
    const size_t bytes = kHeaderBytes + (size_t)((d->n_halo > 0 ? d->n_halo : 1) + (d->n_send > 0 ? d->n_send : 1)) * sizeof(double);
    if (d->comm_block) (void)hipFree(d->comm_block);
    d->comm_block = nullptr;
    void *p = nullptr;
    AVS_HIP(hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained));
    AVS_HIP(hipMemset(p, 0, bytes));
    AVS_HIP(hipMemset((char *)p + offsetof(CommHeader, red), 0xFF, sizeof(CommHeader::red)));
    d->comm_block = p;
    d->comm_bytes = bytes;
    std::vector<uint8_t> blobs((size_t)d->world * AVS_DIST_BLOB_BYTES, 0);
    for (int q = 0; q < d->world; ++q) { // every "peer" is me
        DistBlob b;
        memcpy(&b, d->blob.data(), sizeof(b));
        b.rank = q;
        b.raw_ptr = (uint64_t)(uintptr_t)p;
        b.bytes = bytes;
        for (int k = 0; k < kMaxRanks; ++k) { b.recv_off_of[k] = -1; b.recv_cnt_of[k] = 0; }
        for (size_t i = 0; i < d->peers.size(); ++i)
            if (d->peers[i] == q) { // what I send to q lands in the scratch tail, at my send offset
                b.recv_off_of[d->rank] = (int32_t)(d->n_halo + d->send_offs[i]);
                b.recv_cnt_of[d->rank] = d->send_counts[i];
            }
        memcpy(blobs.data() + (size_t)q * AVS_DIST_BLOB_BYTES, &b, sizeof(b));
    }
    AVS_TRY(direct_connect(c, d, blobs.data(), false));
    // the flags my peers would raise are raised by my own push / finalisation
    DistDev h;
    AVS_HIP(hipMemcpy(&h, d->dd.p, sizeof(h), hipMemcpyDeviceToHost));
    CommHeader *mine = (CommHeader *)d->comm_block;
    for (int i = 0; i < h.npeers; ++i) {
        h.peer_hflag_dst[i] = &mine->hflag[h.peer_rank[i]];
        h.peer_hsum_dst[i] = &mine->hsum[h.peer_rank[i]];
    }
    h.paranoid = 0; // the halo area of a looped-back rank is never written: nothing to check
    h.inject_stale_round = -1;
    for (int q = 0; q < d->world; ++q) {
        h.all_red_dst[q] = &mine->red[0][q][0]; // as if rank q had written its sums into my block
    }
    // a peer that only sends to me (no entry from me to it) would never get its flag raised: give every receive a sender
    for (int i = 0; i < h.npeers; ++i)
        AVS_REQUIRE(h.recv_cnt[i] == 0 || h.send_off[i + 1] > h.send_off[i], AVS_EINTERNAL, "loopback: peer %d sends but does not receive", h.peer_rank[i]);
    AVS_HIP(hipMemcpy(d->dd.p, &h, sizeof(h), hipMemcpyHostToDevice));
    d->dd_host = h;
    return AVS_OK;
}

avs_status avs_dist_import_blobs(avs_ctx *c, const uint8_t *blobs)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c, AVS_EINVAL, "null argument");
    AVS_REQUIRE(c->dist, AVS_ESTATE, "call avs_dist_init_hosted first");
    if (cur_opt().dist_loopback) return direct_connect_loopback(c, c->dist);
    AVS_REQUIRE(blobs, AVS_EINVAL, "null argument");
    AVS_TRY(direct_connect(c, c->dist, blobs));
    // hosted group: every rank calls this with the same blobs; the self-test's rounds rendezvous through the comm blocks.  There is
    // no other transport to fall back to, so a failure is an error.
    bool passed = true;
    AVS_TRY(run_selftest(c, c->dist, &passed));
    if (!passed) {
        c->dist->direct_ready = false;
        return AVS_ERCCL;
    }
    return AVS_OK;
}

avs_status avs_dist_partition(avs_ctx *c, int32_t cut_axis)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c, AVS_EINVAL, "null argument");
    AVS_REQUIRE(c->dist, AVS_ESTATE, "call avs_dist_init / avs_dist_init_local first");
    AVS_REQUIRE(c->system_ready, AVS_ESTATE, "avs_assemble must succeed before avs_dist_partition");
    AVS_HIP(hipSetDevice(c->desc.device));
    AVS_REQUIRE(!c->slab.on, AVS_ESTATE, "the context holds a slab-local pre-pass (this rank's window only): only avs_dist_assemble works on it");
    PcgDist *d = c->dist;
    hipStream_t st = c->stream;
    const int64_t n = c->n_vel;
    if (cut_axis < 0) { // longest axis
        cut_axis = 0;
        if (c->desc.ny > c->desc.nx) cut_axis = 1;
        if (c->desc.nz > (cut_axis == 0 ? c->desc.nx : c->desc.ny)) cut_axis = 2;
    }
    AVS_REQUIRE(cut_axis <= 2, AVS_EINVAL, "cut_axis out of range");
    const int extent = cut_axis == 0 ? c->desc.nx : (cut_axis == 1 ? c->desc.ny : c->desc.nz);

    // the solve works on the brick-major numbering when it exists (avs_reorder.hip): partition THAT system,
    // so every rank's local rows keep the brick locality; results are mapped back in avs_dist_get_solution
    const bool ro = c->reordered;
    const double *g_rhs = ro ? c->p_rhs.p : c->rhs.p, *g_x0 = ro ? c->p_x0.p : c->x0.p;
    const bool host_plan = cur_opt().dist_host_plan != 0;
    d->f32 = c->desc.precision == AVS_PRECISION_F32 && c->opt.dist_f32_vectors != 0;
    d->resident_f32 = d->f32 && c->opt.resident_f32 != 0;
    d->mixed = c->desc.precision == AVS_PRECISION_F64 && c->opt.dist_mixed_precision != 0;
    d->vi.clear();
    d->brick.clear();   // (the brick-structured form is built for distributed assemblies only: avs_dist_assemble)
    d->brick.view(d->brick_view, d->vi);
    d->local_ref.release();
    if (host_plan) AVS_TRY(plan_on_host(c, d, cut_axis, extent, ro));
    else AVS_TRY(plan_on_device(c, d, cut_axis, extent, ro));
    avs_plan_sizes sz{};
    sz.n_own = d->n_own;
    sz.n_halo = d->n_halo;
    sz.nnz_local = d->nnz_local;
    sz.n_send = d->n_send;
    d->n_global = n;
    d->send_offs.assign(d->peers.size(), 0);
    d->recv_offs.assign(d->peers.size(), 0);
    {
        int32_t so = 0, ro2 = 0;
        for (size_t i = 0; i < d->peers.size(); ++i) {
            d->send_offs[i] = so;
            d->recv_offs[i] = ro2;
            so += d->send_counts[i];
            ro2 += d->recv_counts[i];
        }
    }
    if (ro && sz.nnz_local) // same lossless compression as the single-GPU solve, on the local rows
        AVS_TRY(build_matrix_index(d->row_ptr.p, d->col.p, d->val.p, sz.n_own, sz.nnz_local, (int64_t)sz.n_own + sz.n_halo, d->vi, st));
    AVS_TRY(d->rhs.alloc((size_t)sz.n_own));
    AVS_TRY(d->x0.alloc((size_t)sz.n_own));
    AVS_TRY(d->x.alloc((size_t)sz.n_own));
    if (sz.n_own) {
        const unsigned g = (unsigned)((sz.n_own + 255) / 256);
        hipLaunchKernelGGL(k_gather_i<double>, dim3(g), dim3(256), 0, st, g_rhs, d->own_global.p, d->rhs.p, sz.n_own);
        hipLaunchKernelGGL(k_gather_i<double>, dim3(g), dim3(256), 0, st, g_x0, d->own_global.p, d->x0.p, sz.n_own);
    }
    AVS_HIP(hipGetLastError());
    AVS_HIP(hipStreamSynchronize(st));
    if (!d->comm_stream) {
        AVS_HIP(hipStreamCreateWithFlags(&d->comm_stream, hipStreamNonBlocking));
        AVS_HIP(hipEventCreateWithFlags(&d->ev_ready, hipEventDisableTiming));
        AVS_HIP(hipEventCreateWithFlags(&d->ev_halo, hipEventDisableTiming));
    }
    pcg_destroy(d->pcg);
    d->pcg = nullptr;
    AVS_TRY(pcg_create(&d->pcg, sz.n_own, sz.n_own + sz.n_halo, st));
    direct_release(d);
    d->direct_pending = true; // planning needs no peer; connecting the transport does, so it waits for avs_dist_solve
    if (d->hosted) AVS_TRY(direct_setup(c, d)); // hosted group: only allocates the block and fills the blob (no collective)
    d->partitioned = true;
    d->reordered = ro;
    d->solved = false;
    return AVS_OK;
}

avs_status avs_dist_assemble(avs_ctx *c, int32_t cut_axis, avs_assembly_info *info)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c, AVS_EINVAL, "null argument");
    AVS_REQUIRE(c->dist, AVS_ESTATE, "call avs_dist_init / avs_dist_init_local first");
    AVS_HIP(hipSetDevice(c->desc.device));
    PcgDist *d = c->dist;
    hipStream_t st = c->stream;
    if (c->slab.on) {
        AVS_REQUIRE(cut_axis < 0 || cut_axis == c->slab.axis, AVS_EINVAL, "the context's lattices were cut along axis %d by the slab-local pre-pass", c->slab.axis);
        cut_axis = c->slab.axis;
    }
    if (cut_axis < 0) { // longest axis
        cut_axis = 0;
        if (c->desc.ny > c->desc.nx) cut_axis = 1;
        if (c->desc.nz > (cut_axis == 0 ? c->desc.nx : c->desc.ny)) cut_axis = 2;
    }
    AVS_REQUIRE(cut_axis <= 2, AVS_EINVAL, "cut_axis out of range");
    const int extent = cut_axis == 0 ? c->desc.nx : (cut_axis == 1 ? c->desc.ny : c->desc.nz);
    Timer t(st);
    avs_assembly_info ai{};
    t.start();
    AVS_TRY(build_stencils(c)); // dof tables + stencils: index-only; every rank builds all of them -- or, on a slab-local context, the ones around its slab
    ai.stencil_ms = t.stop();
    Scope scope("Build Octree Linear System"); // cpp:554: here only this rank's rows
    ai.guess_ms = 0.; // the restriction of the owned DOFs is part of system_ms here
    t.start();
    c->system_ready = false; // no global matrix in this mode
    c->reordered = false;
    d->f32 = c->desc.precision == AVS_PRECISION_F32 && c->opt.dist_f32_vectors != 0;
    d->resident_f32 = d->f32 && c->opt.resident_f32 != 0;
    d->mixed = c->desc.precision == AVS_PRECISION_F64 && c->opt.dist_mixed_precision != 0;
    d->vi.clear();
    if (c->slab.on) AVS_TRY(dist_assemble_window(c, d));
    else AVS_TRY(dist_assemble_device(c, d, cut_axis, extent));
    ai.system_ms = t.stop();
    t.start();
    d->n_global = c->n_vel;
    d->send_offs.assign(d->peers.size(), 0);
    d->recv_offs.assign(d->peers.size(), 0);
    {
        int32_t so = 0, ro2 = 0;
        for (size_t i = 0; i < d->peers.size(); ++i) {
            d->send_offs[i] = so;
            d->recv_offs[i] = ro2;
            so += d->send_counts[i];
            ro2 += d->recv_counts[i];
        }
    }
    if (d->nnz_local) // the rank's own dictionaries: its rows only hold a subset of the global values
        AVS_TRY(build_matrix_index(d->row_ptr.p, d->col.p, d->val.p, d->n_own, d->nnz_local, d->n_own + d->n_halo, d->vi, st));
    AVS_TRY(dist_build_brick(c, d)); // slabs of >= 2 M rows: the brick-structured form of the local rows
    if (!d->comm_stream) {
        AVS_HIP(hipStreamCreateWithFlags(&d->comm_stream, hipStreamNonBlocking));
        AVS_HIP(hipEventCreateWithFlags(&d->ev_ready, hipEventDisableTiming));
        AVS_HIP(hipEventCreateWithFlags(&d->ev_halo, hipEventDisableTiming));
    }
    pcg_destroy(d->pcg);
    d->pcg = nullptr;
    AVS_TRY(pcg_create(&d->pcg, d->n_own, d->n_own + d->n_halo, st));
    direct_release(d);
    d->direct_pending = true;
    if (d->hosted) AVS_TRY(direct_setup(c, d));
    ai.csr_ms = t.stop();
    d->partitioned = true;
    d->reordered = !c->slab.on; // own_global holds brick-major ids: avs_dist_get_solution maps back through c->inv (slab-local: reference ids)
    d->solved = false;
    ai.n_velocity = c->n_vel;
    ai.n_edge = c->n_edge;
    ai.n_center = c->n_center;
    ai.nnz = d->nnz_local;
    ai.raw_triplets = 0;
    if (info) *info = ai;
    return AVS_OK;
}

static avs_status prepass_allreduce_cb(int32_t *dev, int64_t count, void *stream, void *user)
{
    return dist_allreduce_i32(static_cast<PcgDist *>(user), dev, count, reinterpret_cast<hipStream_t>(stream));
}

avs_status avs_dist_bind_prepass(avs_ctx *c, avs_prepass *pp, int32_t cut_axis, const int32_t *cuts)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c && pp, AVS_EINVAL, "null argument");
    AVS_REQUIRE(c->dist, AVS_ESTATE, "call avs_dist_init / avs_dist_init_local first");
    PcgDist *d = c->dist;
    if (d->world <= 1 || !cuts) return avs_prepass_set_slab(pp, 0, nullptr, 1, 0, nullptr, nullptr);
    AVS_REQUIRE(d->comm || d->group, AVS_ESTATE, "a hosted group sums through the caller's own callback: avs_prepass_set_slab");
    if (cut_axis < 0) {
        cut_axis = 0;
        if (c->desc.ny > c->desc.nx) cut_axis = 1;
        if (c->desc.nz > (cut_axis == 0 ? c->desc.nx : c->desc.ny)) cut_axis = 2;
    }
    return avs_prepass_set_slab(pp, cut_axis, cuts, d->world, d->rank, prepass_allreduce_cb, d);
}

avs_status avs_dist_get_cuts(avs_ctx *c, int32_t which, int32_t *cut_axis, int32_t *cuts)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c && cuts, AVS_EINVAL, "null argument");
    AVS_REQUIRE(c->dist && c->dist->partitioned && c->dist->cuts.size() == (size_t)c->dist->world + 1, AVS_ESTATE, "call avs_dist_assemble first");
    const std::vector<int32_t> &v = which ? c->dist->next_cuts : c->dist->cuts;
    for (size_t i = 0; i < v.size(); ++i) cuts[i] = v[i];
    if (cut_axis) *cut_axis = c->dist->cut_axis;
    return AVS_OK;
}

avs_status avs_dist_get_plan_sizes(avs_ctx *c, avs_plan_sizes *s)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c && s, AVS_EINVAL, "null argument");
    AVS_REQUIRE(c->dist && c->dist->partitioned, AVS_ESTATE, "call avs_dist_partition first");
    s->n_own = c->dist->n_own;
    s->n_halo = c->dist->n_halo;
    s->nnz_local = c->dist->nnz_local;
    s->n_send = c->dist->n_send;
    s->n_peers = (int32_t)c->dist->peers.size();
    return AVS_OK;
}

avs_status avs_dist_get_plan_arrays(avs_ctx *c, int32_t *own_global, int32_t *row_ptr_local, int32_t *col_local, int32_t *send_idx,
                                    int32_t *peers, int32_t *send_counts, int32_t *recv_counts, int32_t *tiles_interior,
                                    int32_t *tiles_boundary)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c, AVS_EINVAL, "null argument");
    AVS_REQUIRE(c->dist && c->dist->partitioned, AVS_ESTATE, "call avs_dist_partition first");
    PcgDist *d = c->dist;
    AVS_HIP(hipSetDevice(c->desc.device));
    auto down = [&](int32_t *dst, const int32_t *src, size_t count) -> avs_status {
        if (dst && count) AVS_HIP(hipMemcpy(dst, src, count * sizeof(int32_t), hipMemcpyDeviceToHost));
        return AVS_OK;
    };
    AVS_HIP(hipStreamSynchronize(c->stream));
    AVS_TRY(down(own_global, d->own_global.p, (size_t)d->n_own));
    AVS_TRY(down(row_ptr_local, d->row_ptr.p, (size_t)d->n_own + 1));
    AVS_TRY(down(col_local, d->col.p, (size_t)d->nnz_local));
    AVS_TRY(down(send_idx, d->send_idx.p, (size_t)d->n_send));
    AVS_TRY(down(tiles_interior, d->tiles_int.p, (size_t)d->n_tiles_int));
    AVS_TRY(down(tiles_boundary, d->tiles_bnd.p, (size_t)d->n_tiles_bnd));
    for (size_t i = 0; i < d->peers.size(); ++i) {
        if (peers) peers[i] = d->peers[i];
        if (send_counts) send_counts[i] = d->send_counts[i];
        if (recv_counts) recv_counts[i] = d->recv_counts[i];
    }
    return AVS_OK;
}

avs_status avs_dist_get_overlap_tiles(avs_ctx *c, int32_t *interior, int32_t *boundary)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c && interior && boundary, AVS_EINVAL, "null argument");
    AVS_REQUIRE(c->dist && c->dist->partitioned, AVS_ESTATE, "call avs_dist_partition first");
    *interior = c->dist->n_tiles_int;
    *boundary = c->dist->n_tiles_bnd;
    return AVS_OK;
}

avs_status avs_dist_solve(avs_ctx *c, double tol, int32_t max_iters, avs_solve_info *info)
{
    avs::OptScope opt_scope_(c);
    avs::CancelScope cancel_scope_(c ? &c->cancel : nullptr);
    AVS_REQUIRE(c, AVS_EINVAL, "null argument");
    AVS_REQUIRE(c->dist && c->dist->partitioned, AVS_ESTATE, "call avs_dist_partition first");
    AVS_REQUIRE(tol >= 0. && max_iters >= 0, AVS_EINVAL, "tolerance / max_iterations out of range");
    AVS_HIP(hipSetDevice(c->desc.device));
    PcgDist *d = c->dist;
    AVS_REQUIRE(!d->hosted || d->direct_ready, AVS_ESTATE, "hosted group: exchange the blobs first (avs_dist_export_blob / avs_dist_import_blobs)");
    Scope scope("Solve Linear System"); // cpp:603
    if (d->direct_pending && !d->hosted) { // first solve on this plan: every rank is here, connect the transport
        AVS_TRY(direct_setup(c, d));
        d->direct_pending = false;
    }
    AVS_HIP(hipMemcpyAsync(d->x.p, d->x0.p, (size_t)d->n_own * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    CsrView A;
    A.n = d->n_own;
    A.nnz = d->nnz_local;
    A.row_ptr = d->row_ptr.p;
    A.col = d->col.p;
    A.val = d->val.p;
    d->vi.apply(A);
    A.no_precond = c->no_precond;
    A.brick = d->brick.ready ? &d->brick_view : nullptr;
    A.f32_vectors = d->f32 ? 1 : 0;
    A.resident_f32 = d->resident_f32 ? 1 : 0;
    A.mixed = d->mixed ? 1 : 0; // (AVS_OPTION_DIST_MIXED_PRECISION; AVS_OPTION_MIXED_PRECISION has no effect here)
    avs_solve_info local{};
    const avs_status rc = pcg_solve(d->pcg, A, d->rhs.p, d->x.p, tol, max_iters, c->stream, &local, d);
    c->float_vectors = pcg_float_vectors(d->pcg);
    c->reliable_updates = pcg_reliable_updates(d->pcg);
    if (rc != AVS_OK) {
        // a peer's flag timed out: epochs / tickets of the comm blocks are no longer in step -- every rank sees the same fault
        // (it waits for the same peer) and leaves the direct transport for this plan; the next solve uses the fallback
        if (rc == AVS_ERCCL && d->direct_ready) {
            (void)hipStreamSynchronize(c->stream);
            direct_release(d);
        }
        return rc;
    }
    local.n = d->n_global;
    if (info) *info = local;
    d->solved = true;
    return AVS_OK;
}

#ifdef AVS_PROBES
// measurement / test entry (include/avs_probe.h): the rank's local rows times a caller-supplied [owned | halo] vector, through the
// storage form and kernel the partitioned loops launch (halo in the tail of the vector: the RCCL transport's layout)
avs_status avs_dist_spmv_local_form(avs_ctx *c, const double *x_ext, double *y, int32_t fused_dot, double *dot_out)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c && x_ext && y, AVS_EINVAL, "null argument");
    AVS_REQUIRE(c->dist && c->dist->partitioned, AVS_ESTATE, "call avs_dist_assemble / avs_dist_partition first");
    AVS_HIP(hipSetDevice(c->desc.device));
    PcgDist *d = c->dist;
    CsrView A;
    A.n = d->n_own;
    A.nnz = d->nnz_local;
    A.row_ptr = d->row_ptr.p;
    A.col = d->col.p;
    A.val = d->val.p;
    d->vi.apply(A);
    A.brick = d->brick.ready ? &d->brick_view : nullptr;
    if (A.n == 0) return AVS_OK;
    // a plan latched with AVS_OPTION_DIST_MIXED_PRECISION: the mixed-precision loops' product on the float values of x_ext; fused_dot & 2
    // asks for the fp64 product of its reliable updates instead (as avs_spmv_solver_form)
    if (d->mixed && !(fused_dot & 2)) {
        AVS_TRY(spmv_mixed_probe(A, x_ext, y, (fused_dot & 1) != 0, dot_out, c->stream, d->n_own + d->n_halo));
        return AVS_OK;
    }
    fused_dot &= 1;
    AVS_TRY(probe_spmv_form(A, x_ext, y, fused_dot != 0, dot_out, c->stream));
    AVS_HIP(hipStreamSynchronize(c->stream));
    return AVS_OK;
}
#endif

avs_status avs_dist_get_info(avs_ctx *c, avs_dist_info *info)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c && info, AVS_EINVAL, "null argument");
    AVS_REQUIRE(c->dist, AVS_ESTATE, "call avs_dist_init / avs_dist_init_local first");
    PcgDist *d = c->dist;
    memset(info, 0, sizeof(*info));
    info->world_size = d->world;
    if (d->comm) {
        int cnt = 0;
        AVS_NCCL(ncclCommCount(d->comm, &cnt));
        info->rccl_ranks = cnt;
    }
    info->transport = d->transport;
    info->selftest_rounds = d->selftest_rounds;
    info->selftest_bad_entries = d->selftest_bad;
    info->paranoid = d->direct_ready ? d->dd_host.paranoid : 0;
    if (d->direct_ready) {
        info->graph_replay = c->opt.graph != 0;
        info->launches_per_iteration = 2; // update (+ push), SpMV over all tiles (+ all-gather + scalar step in its finalizer block)
        info->collectives_per_iteration = 0;
        return AVS_OK;
    }
    info->graph_replay = 0;
    const bool sr = dist_wants_single_reduction(d);
    info->launches_per_iteration = d->world == 1 ? 5 : (sr ? 5 : 8);
    info->collectives_per_iteration = d->world == 1 ? 0 : (sr ? 2 : 3);
    return AVS_OK;
}

avs_status avs_dist_get_solution(avs_ctx *c, double *x, int64_t n, avs_memspace where)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c && x, AVS_EINVAL, "null argument");
    AVS_REQUIRE(c->dist && c->dist->solved, AVS_ESTATE, "no solution: call avs_dist_solve first");
    PcgDist *d = c->dist;
    AVS_REQUIRE(n == d->n_global, AVS_EINVAL, "vector length mismatch");
    AVS_HIP(hipSetDevice(c->desc.device));
    hipStream_t st = c->stream;
    DevBuf<double> full;
    AVS_TRY(full.alloc((size_t)n));
    AVS_HIP(hipMemsetAsync(full.p, 0, (size_t)n * sizeof(double), st));
    if (d->n_own)
        hipLaunchKernelGGL(k_scatter_own, dim3((unsigned)((d->n_own + 255) / 256)), dim3(256), 0, st, d->x.p, d->own_global.p, full.p, d->n_own);
    if (d->world > 1 && !d->hosted) { // hosted group: the caller adds the per-rank vectors (owned entries are disjoint, the rest is 0)
        if (d->comm) AVS_NCCL(ncclAllReduce(full.p, full.p, (size_t)n, ncclDouble, ncclSum, d->comm, st));
        else {
            // in-process: sum the host copies in rank order
            avs_local_group *g = d->group;
            std::vector<double> mine((size_t)n);
            AVS_HIP(hipMemcpyAsync(mine.data(), full.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
            AVS_HIP(hipStreamSynchronize(st));
            static std::mutex gm;
            static std::vector<double> acc;
            g->barrier();
            {
                std::lock_guard<std::mutex> lk(gm);
                if (acc.size() != (size_t)n) acc.assign((size_t)n, 0.);
                if (d->rank == 0) std::fill(acc.begin(), acc.end(), 0.);
            }
            g->barrier();
            for (int r = 0; r < g->world; ++r) { // each owner writes disjoint entries; order is irrelevant
                if (r == d->rank) {
                    std::lock_guard<std::mutex> lk(gm);
                    for (int64_t i = 0; i < n; ++i) acc[(size_t)i] += mine[(size_t)i];
                }
                g->barrier();
            }
            AVS_HIP(hipMemcpyAsync(full.p, acc.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
            AVS_HIP(hipStreamSynchronize(st));
            g->barrier();
        }
    }
    // the gathered vector also becomes the context's solution (reference numbering), so that
    // avs_get_solution / avs_transfer_to_regular_grid work on every rank after a partitioned solve
    AVS_TRY(c->x.alloc((size_t)n));
    if (d->reordered) AVS_TRY(unpermute(c, full.p, c->x.p)); // back to the reference's DOF numbering
    else AVS_HIP(hipMemcpyAsync(c->x.p, full.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
    narrow_solution_if_f32(c, c->x.p, n);
    c->solved = true;
    ++c->solution_gen;
    AVS_HIP(copy_out(x, c->x.p, (size_t)n * sizeof(double), where, st));
    AVS_HIP(hipStreamSynchronize(st));
    return AVS_OK;
}

} // extern "C"
