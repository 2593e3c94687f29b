// avs_stress_check.hip -- the reference's debug invariants on the edge and centre stress index pyramids, on the device
// (reference: edgeStressUnitTest and centerStresUnitTest, cpp:3001-3298, called at cpp:412-413).
// The nine rules are stated in include/avs.h (avs_check_stress_indices); tests/stress_check_model.py restates them in NumPy.
//
//   k_stress_lattice<0> one launch per level and axis: a thread owns four consecutive entries of the edge lattice in LINEAR order (one
//                       16-byte load; the last entries one by one).  Rule 0 needs the entry alone.  Rules 1 and 2 -- the four cells and
//                       the four faces around the edge, and a level up where a face carries no id -- are read only for the entries that
//                       carry an id, and every id in range counts itself in occ[id].
//   k_stress_lattice<1> one launch per level, the same walk over the cell lattice: rule 4 on the entry alone; rules 5, 6 and 7 -- the
//                       cell's label, its six faces (and their children a level down) and its twelve edges (their children and
//                       grandchildren one and two levels down) -- for the entries that carry an id.
//   k_index_numbering   rules 3 and 8 over the occurrence counters (the kernel of avs_check.hip).
//
// Every rule is independent and every read is bounds-tested first: a cell outside its lattice reads as INACTIVE, an index outside its
// lattice as UNASSIGNED.  The only address formed from a lattice value is occ[id], and that store is under the range test of rule 0 / 4;
// labels and velocity indices are only compared with sentinels, so a garbage pyramid of another kind cannot make the checker fault.
// Counts are 64-bit: a thread counts in registers, a wave adds its lanes and issues one atomic per rule it violated; the first violation
// is one atomicMin of a packed key (lattice_key, avs_report.hpp) per violating wave (raw_add and raw_min, avs_report_device.hpp).  Integer
// work only: the same lattices give the same report.
#include "avs_internal.hpp"
#include "avs_report_device.hpp"

namespace avs {

struct StressLevels { // by value; the level of a launch is a kernel argument: every table lookup is wave-uniform
    const int8_t *lab[AVS_MAX_LEVELS];
    const int32_t *vidx[AVS_MAX_LEVELS][3];
    const int32_t *eidx[AVS_MAX_LEVELS][3];
    int n[3]; // level-0 cells per axis
    int levels;
};

// label of cell c of level l; outside the lattice: INACTIVE
__device__ __forceinline__ int stress_label(const StressLevels &P, int l, const int (&c)[3])
{
    const int n0 = P.n[0] >> l, n1 = P.n[1] >> l, n2 = P.n[2] >> l;
    if ((unsigned)c[0] >= (unsigned)n0 || (unsigned)c[1] >= (unsigned)n1 || (unsigned)c[2] >= (unsigned)n2) return AVS_INACTIVE;
    return P.lab[l][(size_t)c[0] + (size_t)n0 * ((size_t)c[1] + (size_t)n1 * (size_t)c[2])];
}
// velocity index of face c of axis f at level l (one more entry on f); outside the lattice: UNASSIGNED
__device__ __forceinline__ int stress_velocity(const StressLevels &P, int l, int f, const int (&c)[3])
{
    const int n0 = (P.n[0] >> l) + (f == 0 ? 1 : 0), n1 = (P.n[1] >> l) + (f == 1 ? 1 : 0), n2 = (P.n[2] >> l) + (f == 2 ? 1 : 0);
    if ((unsigned)c[0] >= (unsigned)n0 || (unsigned)c[1] >= (unsigned)n1 || (unsigned)c[2] >= (unsigned)n2) return AVS_UNASSIGNED;
    return P.vidx[l][f][(size_t)c[0] + (size_t)n0 * ((size_t)c[1] + (size_t)n1 * (size_t)c[2])];
}
// edge index of edge c of axis a at level l (one more entry on the two other axes); outside the lattice: UNASSIGNED
__device__ __forceinline__ int stress_edge(const StressLevels &P, int l, int a, const int (&c)[3])
{
    const int n0 = (P.n[0] >> l) + (a != 0 ? 1 : 0), n1 = (P.n[1] >> l) + (a != 1 ? 1 : 0), n2 = (P.n[2] >> l) + (a != 2 ? 1 : 0);
    if ((unsigned)c[0] >= (unsigned)n0 || (unsigned)c[1] >= (unsigned)n1 || (unsigned)c[2] >= (unsigned)n2) return AVS_UNASSIGNED;
    return P.eidx[l][a][(size_t)c[0] + (size_t)n0 * ((size_t)c[1] + (size_t)n1 * (size_t)c[2])];
}

// rule 0 / 4: UNASSIGNED, OUTSIDE or an id below n
__device__ __forceinline__ bool stress_value_ok(int v, int n) { return v == AVS_UNASSIGNED || v == AVS_OUTSIDE || (v >= 0 && v < n); }

// rules 0 .. 2 for entry `lin` = e of the edge lattice of (level, axis) + the occurrence count of its id
template <int axis>
__device__ __forceinline__ void stress_check_edge(const StressLevels &P, int level, int v, const int (&e)[3], unsigned long long lin, int n_edge,
                                                  int32_t *__restrict__ occ, unsigned (&cnt)[3], unsigned &active, unsigned long long &key)
{
    if (!stress_value_ok(v, n_edge)) { // rule 0
        ++cnt[0];
        key = min(key, lattice_key(AVS_STRESS_RULE_EDGE_VALUE, level, axis, lin));
    }
    if (v < 0) return;
    ++active;
    if (v < n_edge) atomicAdd(occ + v, 1); // (in range: the only address a lattice value forms)
    const int L = P.levels;
    constexpr int b = (axis + 1) % 3, c = (axis + 2) % 3;
    // rule 1: the cells around the edge, walked as the reference walks them -- e - 1_b - 1_c, e - 1_c, e - 1_b, e -- up to the first one
    // outside the lattice (cpp:3038-3044; the classification that writes the lattice leaves the same way, cpp:1361-1370)
    bool bad = false, walking = true;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int cell[3] = {e[0], e[1], e[2]};
        cell[b] -= (q & 1) ? 0 : 1;
        cell[c] -= (q & 2) ? 0 : 1;
        walking = walking && (unsigned)cell[0] < (unsigned)(P.n[0] >> level) && (unsigned)cell[1] < (unsigned)(P.n[1] >> level) &&
                  (unsigned)cell[2] < (unsigned)(P.n[2] >> level);
        if (!walking) continue;
        const int lab = stress_label(P, level, cell);
        bad |= lab != AVS_ACTIVE && lab != AVS_UP;
    }
    if (bad) {
        ++cnt[1];
        key = min(key, lattice_key(AVS_STRESS_RULE_EDGE_CELLS, level, axis, lin));
    }
    // rule 2: the two faces of each other axis that meet in the edge.  Not examined, where the reference's assert rejects what its own
    // classification writes on the border of the grid: a face on a border plane of its own lattice (never numbered, cpp:1210-1215), and
    // every face of an edge on the upper border plane of b, where rule 1's walk ends after the first cell
    bad = false;
    const bool examined = e[b] != (P.n[b] >> level);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int f = t == 0 ? b : c, o = t == 0 ? c : b;
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            int face[3] = {e[0], e[1], e[2]};
            face[o] -= d;
            if (!examined || face[o] < 0 || face[o] >= (P.n[o] >> level) || face[f] == 0 || face[f] == (P.n[f] >> level)) continue;
            const int w = stress_velocity(P, level, f, face);
            if (w >= 0) continue;
            if (w == AVS_SOLIDBOUNDARY || w == AVS_OUTSIDE) {
                bad |= level != 0;
            } else if (w == AVS_UNASSIGNED) {
                if (level == L - 1) {
                    bad = true;
                    continue;
                }
                const int up[3] = {face[0] >> 1, face[1] >> 1, face[2] >> 1};
                if (e[f] & 1) bad |= stress_label(P, level + 1, up) != AVS_ACTIVE;           // a T-junction inside a coarse cell
                else bad |= stress_velocity(P, level + 1, f, up) == AVS_UNASSIGNED;
            } else {
                bad = true;
            }
        }
    }
    if (bad) {
        ++cnt[2];
        key = min(key, lattice_key(AVS_STRESS_RULE_EDGE_FACES, level, axis, lin));
    }
}

// rules 4 .. 7 for entry `lin` = cell of the centre lattice of `level` + the occurrence count of its id
__device__ __forceinline__ void stress_check_center(const StressLevels &P, int level, int v, const int (&cell)[3], unsigned long long lin, int n_center,
                                                    int32_t *__restrict__ occ, unsigned (&cnt)[4], unsigned &active, unsigned long long &key)
{
    if (!stress_value_ok(v, n_center)) { // rule 4
        ++cnt[0];
        key = min(key, lattice_key(AVS_STRESS_RULE_CENTER_VALUE, level, 0, lin));
    }
    if (v < 0) return;
    ++active;
    if (v < n_center) atomicAdd(occ + v, 1); // (in range: the only address a lattice value forms)
    if (stress_label(P, level, cell) != AVS_ACTIVE) { // rule 5
        ++cnt[1];
        key = min(key, lattice_key(AVS_STRESS_RULE_CENTER_LABEL, level, 0, lin));
    }
    bool bad = false; // rule 6: the six faces, but for those on a border plane of their lattice (never numbered, cpp:1210-1215)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, c = (a + 2) % 3;
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            int face[3] = {cell[0], cell[1], cell[2]};
            face[a] += d;
            if (face[a] == 0 || face[a] == (P.n[a] >> level)) continue;
            const int w = stress_velocity(P, level, a, face);
            if (w >= 0) continue;
            if (w == AVS_UNASSIGNED) {
                if (level == 0) {
                    bad = true;
                    continue;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    int child[3] = {2 * face[0], 2 * face[1], 2 * face[2]};
                    child[b] += q & 1;
                    child[c] += q >> 1;
                    bad |= stress_velocity(P, level - 1, a, child) < 0;
                }
            } else if (w == AVS_OUTSIDE || w == AVS_SOLIDBOUNDARY) {
                bad |= level != 0;
            } else {
                bad = true;
            }
        }
    }
    if (bad) {
        ++cnt[2];
        key = min(key, lattice_key(AVS_STRESS_RULE_CENTER_FACES, level, 0, lin));
    }
    bad = false; // rule 7: the twelve edges
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, c = (a + 2) % 3;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int edge[3] = {cell[0], cell[1], cell[2]};
            edge[b] += q & 1;
            edge[c] += q >> 1;
            if (stress_edge(P, level, a, edge) != AVS_UNASSIGNED) continue;
            if (level == 0) {
                bad = true;
                continue;
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                int child[3] = {2 * edge[0], 2 * edge[1], 2 * edge[2]};
                child[a] += h;
                if (stress_edge(P, level - 1, a, child) >= 0) continue;
                if (level == 1) {
                    bad = true;
                    continue;
                }
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    int grand[3] = {2 * child[0], 2 * child[1], 2 * child[2]};
                    grand[a] += g;
                    bad |= stress_edge(P, level - 2, a, grand) < 0;
                }
            }
        }
    }
    if (bad) {
        ++cnt[3];
        key = min(key, lattice_key(AVS_STRESS_RULE_CENTER_EDGES, level, 0, lin));
    }
}

// kind 0: the edge lattice of (level, axis); kind 1: the centre lattice of level (axis is 0).  f0, f1, f2: the lattice's extents.  The
// axis is a template argument: every coordinate a rule touches is then a register, not an element of an array indexed at run time.
template <int kind, int axis>
__global__ __launch_bounds__(kBlock) void k_stress_lattice(StressLevels P, int level, const int32_t *__restrict__ idx, int quads_ok, int f0,
                                                                 int f1, int f2, int n_ids, int32_t *__restrict__ occ, unsigned long long *__restrict__ raw)
{
    constexpr int kRules = kind == 0 ? 3 : 4;
    const long long total = (long long)f0 * f1 * f2, quads = (total + 3) >> 2;
    unsigned cnt[kRules] = {};
    unsigned active = 0u;
    unsigned long long key = kNoKey;
    for (long long q = (long long)blockIdx.x * kBlock + threadIdx.x; q < quads; q += (long long)gridDim.x * kBlock) {
        const long long e0 = 4 * q;
        int v[4] = {AVS_UNASSIGNED, AVS_UNASSIGNED, AVS_UNASSIGNED, AVS_UNASSIGNED};
        const int nv = (int)min(4ll, total - e0);
        if (quads_ok && nv == 4) {
            const int4 w = *reinterpret_cast<const int4 *>(idx + e0);
            v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (b < nv) v[b] = idx[e0 + b];
        }
        int at[3] = {0, 0, 0};
        // the value rule needs the entry alone; where no entry of the quad carries an id -- most of every lattice -- nothing is divided
        if (v[0] >= 0 || v[1] >= 0 || v[2] >= 0 || v[3] >= 0) {
            if (total <= 0xffffffffll) { // 32-bit division where the lattice allows it
                const unsigned row = (unsigned)e0 / (unsigned)f0;
                at[0] = (int)((unsigned)e0 - row * (unsigned)f0), at[1] = (int)(row % (unsigned)f1), at[2] = (int)(row / (unsigned)f1);
            } else {
                at[0] = (int)(e0 % f0), at[1] = (int)(e0 / f0 % f1), at[2] = (int)(e0 / ((long long)f0 * f1));
            }
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (b < nv) {
                if constexpr (kind == 0) stress_check_edge<axis>(P, level, v[b], at, (unsigned long long)(e0 + b), n_ids, occ, cnt, active, key);
                else stress_check_center(P, level, v[b], at, (unsigned long long)(e0 + b), n_ids, occ, cnt, active, key);
            }
            if (++at[0] == f0) { // the next entry starts a row
                at[0] = 0;
                if (++at[1] == f1) {
                    at[1] = 0;
                    ++at[2];
                }
            }
        }
    }
    constexpr int first_rule = kind == 0 ? AVS_STRESS_RULE_EDGE_VALUE : AVS_STRESS_RULE_CENTER_VALUE; // (the rules of a kind are consecutive)
#pragma unroll
    for (int r = 0; r < kRules; ++r) raw_add(cnt[r], first_rule + r, raw);
    raw_add(active, kind == 0 ? kStressRawEdges : kStressRawCenters, raw);
    raw_min(key, kStressRawKey, raw);
}

// Shared implementation of avs_check_stress_indices / avs_prepass_check_stress_indices (rules and protocol: include/avs.h).  The caller has
// run check_stress_args and the state checks of its object.
avs_status check_stress_indices(StressCheckScratch &S, const StressCheckSource &src, hipStream_t st, uint32_t what, avs_stress_check *report)
{
    if (what == 0 || src.levels == 0) {
        report_hand_over(check_stress_passed(), report);
        return AVS_OK;
    }
    const bool edges = (what & AVS_CHECK_EDGE_INDICES) != 0, centers = (what & AVS_CHECK_CENTER_INDICES) != 0;
    StressLevels P{};
    P.levels = src.levels;
    AVS_REQUIRE(src.levels >= 1 && src.levels <= AVS_MAX_LEVELS, AVS_EINTERNAL, "stress index check: %d levels", src.levels);
    for (int a = 0; a < 3; ++a) {
        P.n[a] = src.n[a];
        AVS_REQUIRE((src.n[a] >> (src.levels - 1)) >= 1, AVS_EINTERNAL, "stress index check: %d levels on a %d x %d x %d lattice", src.levels, src.n[0],
                    src.n[1], src.n[2]);
    }
    for (int l = 0; l < src.levels; ++l) {
        AVS_REQUIRE(src.labels[l], AVS_EINTERNAL, "stress index check: level %d has no label lattice", l);
        P.lab[l] = src.labels[l];
        for (int a = 0; a < 3; ++a) {
            AVS_REQUIRE(src.vidx[l][a] && src.eidx[l][a], AVS_EINTERNAL, "stress index check: level %d axis %d has no velocity or edge index lattice", l, a);
            P.vidx[l][a] = src.vidx[l][a];
            P.eidx[l][a] = src.eidx[l][a];
        }
        AVS_REQUIRE(!centers || src.cidx[l], AVS_EINTERNAL, "stress index check: level %d has no centre index lattice", l);
    }
    AVS_REQUIRE(!edges || (src.n_edge >= 0 && src.n_edge < INT32_MAX), AVS_EINTERNAL, "stress index check: edge count out of range");
    AVS_REQUIRE(!centers || (src.n_center >= 0 && src.n_center < INT32_MAX), AVS_EINTERNAL, "stress index check: centre count out of range");
    AVS_TRY(S.raw.begin(kStressRawWords, kStressRawKey, st));
    if (edges) {
        const int n_edge = (int)src.n_edge;
        AVS_TRY(S.occ_edge.reserve((size_t)n_edge + 1));
        AVS_HIP(hipMemsetAsync(S.occ_edge.p, 0, ((size_t)n_edge + 1) * sizeof(int32_t), st));
        for (int l = 0; l < src.levels; ++l)
            for (int a = 0; a < 3; ++a) {
                int f[3];
                for (int d = 0; d < 3; ++d) f[d] = (src.n[d] >> l) + (d != a ? 1 : 0);
                const long long total = (long long)f[0] * f[1] * f[2];
                const int quads_ok = (reinterpret_cast<uintptr_t>(src.eidx[l][a]) & 15u) == 0 ? 1 : 0;
                const auto kernel = a == 0 ? k_stress_lattice<0, 0> : (a == 1 ? k_stress_lattice<0, 1> : k_stress_lattice<0, 2>);
                hipLaunchKernelGGL(kernel, dim3(report_grid(report_workgroups((total + 3) >> 2), src.grid_cap)), dim3(kBlock), 0, st, P, l, src.eidx[l][a], quads_ok,
                                   f[0], f[1], f[2], n_edge, S.occ_edge.p, S.raw.p);
            }
        if (n_edge > 0)
            hipLaunchKernelGGL(k_index_numbering, dim3(report_grid(report_workgroups(n_edge), src.grid_cap)), dim3(kBlock), 0, st, (const int32_t *)S.occ_edge.p, n_edge,
                               (int)AVS_STRESS_RULE_EDGE_NUMBERING, kStressRawKey, S.raw.p);
    }
    if (centers) {
        const int n_center = (int)src.n_center;
        AVS_TRY(S.occ_center.reserve((size_t)n_center + 1));
        AVS_HIP(hipMemsetAsync(S.occ_center.p, 0, ((size_t)n_center + 1) * sizeof(int32_t), st));
        for (int l = 0; l < src.levels; ++l) {
            const int f[3] = {src.n[0] >> l, src.n[1] >> l, src.n[2] >> l};
            const long long total = (long long)f[0] * f[1] * f[2];
            const int quads_ok = (reinterpret_cast<uintptr_t>(src.cidx[l]) & 15u) == 0 ? 1 : 0;
            hipLaunchKernelGGL((k_stress_lattice<1, 0>), dim3(report_grid(report_workgroups((total + 3) >> 2), src.grid_cap)), dim3(kBlock), 0, st, P, l, src.cidx[l],
                               quads_ok, f[0], f[1], f[2], n_center, S.occ_center.p, S.raw.p);
        }
        if (n_center > 0)
            hipLaunchKernelGGL(k_index_numbering, dim3(report_grid(report_workgroups(n_center), src.grid_cap)), dim3(kBlock), 0, st, (const int32_t *)S.occ_center.p,
                               n_center, (int)AVS_STRESS_RULE_CENTER_NUMBERING, kStressRawKey, S.raw.p);
    }
    unsigned long long raw[kStressRawWords];
    AVS_TRY(S.raw.read(raw, st)); // the one wait: the report is on the host
    report_hand_over(check_stress_report(raw, what, src.n), report);
    return AVS_OK;
}

} // namespace avs

using namespace avs;

extern "C" avs_status avs_check_stress_indices(avs_ctx *c, uint32_t what, avs_stress_check *report)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c, AVS_EINVAL, "null argument");
    const char *why = nullptr;
    if (check_stress_args(what, report, &why) != AVS_OK) {
        set_error("%s", why);
        return AVS_EINVAL;
    }
    AVS_REQUIRE(!c->slab.on, AVS_ESTATE, "avs_check_stress_indices: the context holds a slab-local pre-pass (this rank's window only)");
    StressCheckSource src{};
    if (what != 0) {
        for (int l = 0; l < c->desc.levels; ++l) {
            AVS_REQUIRE(c->have_labels[l] && c->labels[l].p, AVS_ESTATE, "avs_check_stress_indices: labels of level %d missing (avs_set_labels / avs_prepass_apply)", l);
            src.labels[l] = c->labels[l].p;
            for (int a = 0; a < 3; ++a) {
                AVS_REQUIRE(c->have_vidx[l][a] && c->vidx[l][a].p, AVS_ESTATE,
                            "avs_check_stress_indices: velocity indices of level %d axis %d missing (avs_set_index_field / avs_prepass_apply)", l, a);
                AVS_REQUIRE(c->have_eidx[l][a] && c->eidx[l][a].p, AVS_ESTATE,
                            "avs_check_stress_indices: edge indices of level %d axis %d missing (avs_set_index_field / avs_prepass_apply)", l, a);
                src.vidx[l][a] = c->vidx[l][a].p;
                src.eidx[l][a] = c->eidx[l][a].p;
            }
            if (!(what & AVS_CHECK_CENTER_INDICES)) continue;
            AVS_REQUIRE(c->have_cidx[l] && c->cidx[l].p, AVS_ESTATE,
                        "avs_check_stress_indices: centre indices of level %d missing (avs_set_index_field / avs_prepass_apply)", l);
            src.cidx[l] = c->cidx[l].p;
        }
        AVS_REQUIRE(c->n_edge >= 0 && c->n_center >= 0, AVS_ESTATE, "avs_check_stress_indices: DOF counts missing (avs_set_dof_counts / avs_prepass_apply)");
    }
    src.levels = c->desc.levels;
    src.n[0] = c->desc.nx;
    src.n[1] = c->desc.ny;
    src.n[2] = c->desc.nz;
    src.n_edge = c->n_edge;
    src.n_center = c->n_center;
    src.grid_cap = c->opt.cells_grid_cap;
    AVS_HIP(hipSetDevice(c->desc.device));
    Scope scope("Stress Unit Tests"); // cpp:412-413
    return check_stress_indices(c->stress_check, src, c->stream, what, report);
}
