// avs_resident_plan.cpp -- host-side planner of the CU-resident PCG (no device code; see avs_resident_plan.hpp).
//
// Pure integer (and a little double) work on host arrays.  resident_prepare (avs_pcg_resident.inl) drives it between its device
// steps; tests/test_resident_plan_host.py runs it without a GPU.
#include "avs_resident_plan.hpp"

#include <algorithm>

namespace avs {

const char *form_lanes(const int32_t *rp, int64_t n, int max_quads, double T, ResidentLanes *lanes)
{
    const int W = max_quads * kResQuadWords;
    lanes->row0.clear();
    lanes->meta.clear();
    lanes->stream_quads.clear();
    lanes->streamed_rows = lanes->streamed_words = 0;
    lanes->long_lanes = lanes->longest_tail = lanes->max_lane_streamed = 0;
    double debt = 0.;
    for (int64_t i = 0; i < n;) {
        const int Lr = rp[i + 1] - rp[i];
        if (Lr <= 0) return "empty row"; // (every row of this system carries its diagonal, cpp:2768)
        if (Lr > W) { // a long row's lane: one register row, no streamed rows, the tail's words above bit 10
            if (Lr - W >= (1 << kLaneTailBits)) return "row too long";
            lanes->row0.push_back((int32_t)i);
            lanes->meta.push_back(lane_meta_of(1, 0, Lr - W));
            lanes->stream_quads.push_back(0);
            lanes->long_lanes++;
            lanes->longest_tail = std::max(lanes->longest_tail, Lr - W);
            ++i;
            continue;
        }
        int rows = 0, used = 0;
        const int64_t first = i;
        while (i < n && rows < kResRowsMax) {
            const int Li = rp[i + 1] - rp[i];
            if (Li <= 0 || Li > W) break;
            const int k = quads_of_words(Li);
            if (used + k > max_quads) break;
            used += k;
            ++rows;
            ++i;
        }
        debt += T;
        int m = 0, quads = 0;
        while (i < n && m < (int)kLaneStreamedMask) {
            const int Li = rp[i + 1] - rp[i];
            if (Li <= 0) return "empty row";
            const int k = quads_of_words(Li);
            if ((double)k > debt + 0.5 * (double)k) break; // (take the row when at least half of it is owed)
            debt -= (double)k;
            quads += k;
            lanes->streamed_words += Li;
            ++m;
            ++i;
        }
        lanes->row0.push_back((int32_t)first);
        lanes->meta.push_back(lane_meta_of(rows, m, 0));
        lanes->stream_quads.push_back(quads);
        lanes->streamed_rows += m;
        lanes->max_lane_streamed = std::max(lanes->max_lane_streamed, m);
    }
    return nullptr;
}

// (a slab whose quads exceed what the lanes could hold even at 14 of 15 quads each needs streamed rows for certain: the
// registers-only pass -- 2 ns per row on the host -- is skipped)
static bool surely_streams(int64_t q_total, int64_t lane_cap) { return (double)q_total > 14. * 0.93 * (double)lane_cap; }

const char *lanes_in_registers(const int32_t *rp, int64_t n, int G, int max_quads, ResidentLanes *lanes, int64_t *q_total)
{
    lanes->row0.reserve((size_t)n / 4 + 16);
    lanes->meta.reserve((size_t)n / 4 + 16);
    lanes->stream_quads.reserve((size_t)n / 4 + 16);
    int64_t q = 0;
    for (int64_t i = 0; i < n; ++i) q += quads_of_words(rp[i + 1] - rp[i]);
    *q_total = q;
    if (surely_streams(q, (int64_t)G * kResThreads)) return nullptr;
    return form_lanes(rp, n, max_quads, 0., lanes);
}

const char *lanes_with_streams(const int32_t *rp, int64_t n, int G, int max_quads, double lane_fill, bool no_stream, int64_t q_total,
                               ResidentLanes *lanes, double *stream_T)
{
    const int64_t lane_cap = (int64_t)G * kResThreads;
    const bool surely = surely_streams(q_total, lane_cap);
    *stream_T = 0.;
    if (surely || lanes->size() > lane_cap * 93 / 100) {
        if (no_stream) return "too many rows for the register files of this GPU";
        // register quads an average lane holds: measured when the registers-only pass ran, else 12.8 (4-way slab 12.9, 256^3 beam 12.7)
        const double q_lane = surely ? 12.8 : (double)q_total / (double)lanes->size();
        double Lt = lane_fill * (double)lane_cap;
        for (int attempt = 0; attempt < 8; ++attempt, Lt *= 0.97) {
            *stream_T = ((double)q_total - Lt * q_lane) / Lt;
            if (const char *fail = form_lanes(rp, n, max_quads, *stream_T, lanes)) return fail;
            if (lanes->size() <= lane_cap * 96 / 100) break;
        }
        if (lanes->size() > lane_cap * 97 / 100) return "too many rows for the register files of this GPU, even with streamed rows";
    }
    if ((lanes->size() + G - 1) / G > kResThreads) return "too many rows for the register files of this GPU";
    return nullptr;
}

bool split_by_cost(const ResidentLanes &lanes, int G, double stream_cost, ResidentSplit *s)
{
    // measured: ~12.7 ns per lane, ~3.6 ns per row of a workgroup -- workgroups of fine regions have 2x the rows of those in coarse
    // regions at equal lanes
    const double c_lane = 12.7, c_row = 3.6;
    const int64_t L = lanes.size();
    std::vector<double> &cum = s->cum;
    for (int64_t l = 0; l < L; ++l) // (a streamed quad costs what a register quad does plus its load; 15 quads = one lane's walk)
        cum[(size_t)l + 1] = cum[(size_t)l] + s->lane_w[(size_t)l] * (c_lane * (1. + stream_cost * (double)lanes.stream_quads[(size_t)l] / (double)kResQuads) +
                                                                     c_row * (double)(lane_rows(lanes.meta[(size_t)l]) + lane_streamed(lanes.meta[(size_t)l])) +
                                                                     s->lane_extra[(size_t)l]);
    int64_t l0 = 0;
    s->wl[0] = 0;
    for (int b = 1; b <= G; ++b) {
        // equal shares of what is LEFT (a workgroup clipped at 1024 lanes hands its surplus to the following ones)
        const double target = cum[(size_t)l0] + (cum[(size_t)L] - cum[(size_t)l0]) / (double)(G - b + 1);
        int64_t l1 = std::lower_bound(cum.begin() + l0, cum.end(), target) - cum.begin();
        if (b == G) l1 = L;
        l1 = std::min<int64_t>(std::max(l1, l0), std::min<int64_t>(L, l0 + kResThreads));
        s->wl[(size_t)b] = (int32_t)l1;
        l0 = l1;
    }
    return l0 == L;
}

void split_equal_lanes(int64_t L, int G, std::vector<int32_t> *wl)
{
    const int64_t lpw = (L + G - 1) / G;
    for (int b = 0; b <= G; ++b) (*wl)[(size_t)b] = (int32_t)std::min<int64_t>((int64_t)b * lpw, L);
}

int workgroup_rows(const std::vector<int32_t> &wl, const ResidentLanes &lanes, int64_t n, std::vector<int32_t> *wr)
{
    const size_t G = wl.size() - 1;
    int max_rows = 0;
    for (size_t b = 0; b <= G; ++b) (*wr)[b] = wl[b] < lanes.size() ? lanes.row0[(size_t)wl[b]] : (int32_t)n;
    for (size_t b = 0; b < G; ++b) max_rows = std::max(max_rows, (*wr)[b + 1] - (*wr)[b]);
    return max_rows;
}

bool spread_remote_cost(const std::vector<int32_t> &rc, double c_rem, ResidentSplit *s)
{
    bool any = false;
    for (size_t b = 0; b < rc.size(); ++b) {
        const int64_t lanes_b = s->wl[b + 1] - s->wl[b];
        for (int64_t l = s->wl[b]; l < s->wl[b + 1]; ++l) {
            any = any || s->lane_extra[(size_t)l] == 0.;
            s->lane_extra[(size_t)l] = c_rem * (double)rc[b] / (double)(lanes_b > 0 ? lanes_b : 1);
        }
    }
    return any;
}

double total_demand(const ResidentCounts &c, int t)
{
    double demand = 0.;
    for (size_t b = 0; b < c.rc.size(); ++b) demand += (double)c.footprint(t, (int)b, kRaw);
    return demand;
}

int64_t largest_footprint(const ResidentCounts &c, int t)
{
    int64_t worst = 0;
    for (size_t b = 0; b < c.rc.size(); ++b) worst = std::max(worst, c.footprint(t, (int)b, kEven));
    return worst;
}

int max_local_columns(const ResidentCounts &c)
{
    int64_t cols = 0;
    for (size_t b = 0; b < c.rc.size(); ++b) cols = std::max(cols, c.rows((int)b, kEven) + c.remote((int)b, kEven));
    return (int)cols;
}

double median_footprint(const ResidentCounts &c, int t)
{
    const size_t G = c.rc.size();
    std::vector<double> fps(G);
    for (size_t b = 0; b < G; ++b) fps[b] = (double)c.footprint(t, (int)b, kRaw);
    std::nth_element(fps.begin(), fps.begin() + G / 2, fps.end());
    return fps[G / 2];
}

bool reweight_offenders(const ResidentCounts &c, int t, double limit, ResidentSplit *s)
{
    bool any = false;
    for (size_t b = 0; b < c.rc.size(); ++b) {
        const double fp = (double)c.footprint(t, (int)b, kRaw);
        if (fp > 0.97 * limit) {
            any = true;
            for (int64_t l = s->wl[b]; l < s->wl[b + 1]; ++l) s->lane_w[(size_t)l] *= 1.12 * fp / limit;
        }
    }
    return any;
}

int push_segments(const int *send_off, int npeers, const int32_t *send_idx, const std::vector<int32_t> &wr, std::vector<int32_t> *seg)
{
    const size_t G1 = wr.size(), G = G1 - 1;
    seg->assign((size_t)(npeers > 0 ? npeers : 1) * G1, 0);
    for (int i = 0; i < npeers; ++i) {
        const int32_t *lo = send_idx + send_off[i], *hi = send_idx + send_off[i + 1];
        for (size_t b = 0; b <= G; ++b) (*seg)[(size_t)i * G1 + b] = (int32_t)(std::lower_bound(lo, hi, wr[b]) - send_idx);
    }
    int pushing = 0;
    for (size_t b = 0; b < G; ++b) {
        bool any = false;
        for (int i = 0; i < npeers; ++i) any = any || (*seg)[(size_t)i * G1 + b + 1] > (*seg)[(size_t)i * G1 + b];
        pushing += any ? 1 : 0;
    }
    return pushing;
}

void halo_workgroups(const int32_t *tiles, int n_tiles, int tile_rows, int64_t n, const std::vector<int32_t> &wr, std::vector<uint8_t> *halo)
{
    for (int t = 0; t < n_tiles; ++t) {
        const int64_t r0 = (int64_t)tiles[t] * tile_rows, r1 = std::min<int64_t>(r0 + tile_rows, n);
        for (size_t b = 0; b + 1 < wr.size(); ++b)
            if (wr[b] < r1 && wr[b + 1] > r0) (*halo)[b] = 1;
    }
}

int64_t wave_stream_offsets(const std::vector<int32_t> &wl, const ResidentLanes &lanes, std::vector<int32_t> *soff)
{
    const size_t G = wl.size() - 1, wpg = kResThreads / 64;
    soff->assign(G * wpg + 1, 0);
    int64_t run = 0;
    for (size_t b = 0; b < G; ++b)
        for (size_t w = 0; w < wpg; ++w) {
            int mx = 0;
            for (int64_t l = (int64_t)wl[b] + 64 * (int64_t)w; l < std::min<int64_t>((int64_t)wl[b] + 64 * (int64_t)(w + 1), wl[b + 1]); ++l)
                mx = std::max(mx, lanes.stream_quads[(size_t)l]);
            (*soff)[b * wpg + w] = (int32_t)run;
            run += 64 * (int64_t)mx;
        }
    (*soff)[G * wpg] = (int32_t)run;
    return run;
}

} // namespace avs
