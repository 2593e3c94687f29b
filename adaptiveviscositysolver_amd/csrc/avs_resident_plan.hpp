// avs_resident_plan.hpp -- the integer planning of the CU-resident PCG (avs_pcg_resident.inl) on host arrays: which rows a lane keeps,
// where the workgroups are cut, what a workgroup needs of the LDS, the push segments of a partitioned plan, the waves' stream offsets.
// Plain C++ (no HIP header): compiled once for both libraries, run on the CPU by tests/test_resident_plan_host.py through
// avs_resident_plan_host (include/avs_probe.h).  The geometry the kernels and the plan share is defined here, once.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace avs {

static constexpr int kResThreads = 1024;
static constexpr int kResQuads = 15;     // 128-bit register quads of matrix words per lane (60 VGPRs)
static constexpr int kResQuadWords = 5;  // 25-bit words per quad; a row takes ceil(len / 5) consecutive quads of ONE lane
static constexpr int kResRowsMax = 6;    // rows per lane
static constexpr int kResWordBits = 25;  // value code | workgroup-local column

// lane_meta: register rows (<= kResRowsMax) | streamed rows << 3 (<= 127) | a long row's words beyond the registers << 10 (< 2^22).
// (The kernels spell the fields out with these constants: through the accessors the compiler orders a few operands differently.)
static constexpr uint32_t kLaneRowsMask = 7u, kLaneStreamedMask = 127u;
static constexpr int kLaneStreamedShift = 3, kLaneTailShift = 10, kLaneTailBits = 32 - kLaneTailShift;
constexpr uint32_t lane_meta_of(int rows, int streamed, int tail)
{
    return (uint32_t)rows | (uint32_t)streamed << kLaneStreamedShift | (uint32_t)tail << kLaneTailShift;
}
constexpr int lane_rows(uint32_t meta) { return (int)(meta & kLaneRowsMask); }
constexpr int lane_streamed(uint32_t meta) { return (int)((meta >> kLaneStreamedShift) & kLaneStreamedMask); }
constexpr int lane_tail(uint32_t meta) { return (int)(meta >> kLaneTailShift); }
constexpr int quads_of_words(int words) { return (words + kResQuadWords - 1) / kResQuadWords; }

// ---- lanes: consecutive rows, each in ceil(len / 5) of the lane's quads, at most 6 rows; a row of more than 5 max_quads words sits
// alone, the rest of it is read from memory; after its register rows a lane may take streamed rows ----
struct ResidentLanes {
    std::vector<int32_t> row0;          // first row of the lane
    std::vector<uint32_t> meta;         // lane_meta_of
    std::vector<int32_t> stream_quads;  // quads the lane streams per iteration (cost model, stream layout)
    int64_t streamed_rows = 0, streamed_words = 0;
    int long_lanes = 0, longest_tail = 0, max_lane_streamed = 0;
    int64_t size() const { return (int64_t)row0.size(); }
};
// T: streamed QUADS per lane.  0 while the slab fits the register files; otherwise every lane takes, after its register rows, rows
// worth about T quads (error diffusion keeps the average; equal quads per lane, not equal rows: a wave walks its longest lane's
// stream, and with rows of 3-6 quads an equal-rows split padded the streams by 64 %); at most 127 rows per lane.
// Returns nullptr, or why the rows cannot be laid out (an empty row, a row too long).
const char *form_lanes(const int32_t *rp, int64_t n, int max_quads, double T, ResidentLanes *lanes);
// The two steps around form_lanes for G workgroups.  Registers only: *q_total = the quads of all rows; the pass itself is skipped (no
// lanes) when they exceed what the lanes could hold even at 14 of 15 quads each.  With streams: nothing to do while the lanes stay
// under 93 % of 1024 G; else up to eight passes with a shrinking lane target (lane_fill x 1024 G, x 0.97 each) until they are under
// 96 % -- refused above 97 %, or at once with no_stream; *stream_T = the T of the pass that was kept.  Both return the refusal text.
const char *lanes_in_registers(const int32_t *rp, int64_t n, int G, int max_quads, ResidentLanes *lanes, int64_t *q_total);
const char *lanes_with_streams(const int32_t *rp, int64_t n, int G, int max_quads, double lane_fill, bool no_stream, int64_t q_total,
                               ResidentLanes *lanes, double *stream_T);

// ---- workgroup boundaries by estimated time: the SpMV phase costs per lane (every lane walks its quads; a streamed quad costs what a
// register quad does plus its load), the vector update per row; remote columns cost their workgroup a fill (lane_extra) ----
struct ResidentSplit {
    std::vector<double> lane_w, lane_extra, cum; // per lane: re-weighting factor, remote-column term; prefix sums of the cost (L + 1)
    std::vector<int32_t> wl, wr;                 // first lane / first row of workgroup b (G + 1)
    int max_rows = 0;
};
// equal shares of the remaining cost, a workgroup clipped at 1024 lanes; false: the clips left lanes over (wl does not end at L)
bool split_by_cost(const ResidentLanes &lanes, int G, double stream_cost, ResidentSplit *s);
void split_equal_lanes(int64_t L, int G, std::vector<int32_t> *wl);
// wr[b] = first row of lane wl[b] (n past the last lane); returns the most rows of a workgroup
int workgroup_rows(const std::vector<int32_t> &wl, const ResidentLanes &lanes, int64_t n, std::vector<int32_t> *wr);
// round 0 measured the remote columns rc[b]: spread c_rem x rc[b] over workgroup b's lanes; true when a lane had no term before
bool spread_remote_cost(const std::vector<int32_t> &rc, double c_rem, ResidentSplit *s);

// ---- LDS footprint of workgroup b in entries of the vector type: (4 - t) slices of its rows + remote columns + table entries.
// kRaw: the counts as they are (the estimates that steer the split); kEven: rows and remote columns rounded up to even, as the
// kernel lays them out (what must fit) ----
enum FootprintCounts { kRaw, kEven };
struct ResidentCounts {
    const std::vector<int32_t> &wr, &rc, &tabs; // row boundaries (G + 1), remote columns and (even) table entries per workgroup (G)
    static int64_t count(int64_t v, FootprintCounts c) { return c == kEven ? (v + 1) & ~(int64_t)1 : v; }
    int64_t rows(int b, FootprintCounts c) const { return count(wr[(size_t)b + 1] - wr[(size_t)b], c); }
    int64_t remote(int b, FootprintCounts c) const { return count(rc[(size_t)b], c); }
    int64_t footprint(int t, int b, FootprintCounts c) const { return (int64_t)(4 - t) * rows(b, c) + remote(b, c) + tabs[(size_t)b]; }
};
double total_demand(const ResidentCounts &c, int t);    // sum of the raw footprints
int64_t largest_footprint(const ResidentCounts &c, int t); // the largest even footprint: decides the tier
int max_local_columns(const ResidentCounts &c);            // most (even) rows + remote columns of a workgroup: the word's column bits
double median_footprint(const ResidentCounts &c, int t); // raw
// workgroups above 0.97 limit get their lanes' weights multiplied by 1.12 footprint / limit; true when there was one
bool reweight_offenders(const ResidentCounts &c, int t, double limit, ResidentSplit *s);

// ---- a partitioned plan: seg[i (G + 1) + b] = first entry of peer i's send list (entries send_off[i] .. send_off[i + 1] of send_idx,
// ascending rows) at or past workgroup b's first row; returns the workgroups that push at all ----
int push_segments(const int *send_off, int npeers, const int32_t *send_idx, const std::vector<int32_t> &wr, std::vector<int32_t> *seg);
// workgroups that overlap a halo-reading tile (tile_rows rows each) of the boundary tile list
void halo_workgroups(const int32_t *tiles, int n_tiles, int tile_rows, int64_t n, const std::vector<int32_t> &wr, std::vector<uint8_t> *halo);
// first quad of every wave's lane-interleaved stream (64 x its longest lane's quads each); returns the total
int64_t wave_stream_offsets(const std::vector<int32_t> &wl, const ResidentLanes &lanes, std::vector<int32_t> *soff);

} // namespace avs
