// avs_strain.hip -- strain rates, dissipation and the shear-rate field of a velocity, on the device
// (avs_get_strain_rates / avs_get_shear_rate_field; every convention is stated in include/avs.h, tests/strain_rate_model.py restates
// them in NumPy).  The stencils of avs_build_stencils are rows of the deformation-rate operator: an edge stencil is eps_bc at an edge
// of axis a, a centre list du_a/dx_a at a cell (cpp:443-498).
//
//   k_strain_rates  one lane per stencil, persistent workgroups over chunks of 256 (kBlock) consecutive stencils.  The records are SoA ([k * count
//                   + s]): consecutive lanes load consecutive words; a lane's loop runs to its own cnt (4-12 in practice, cap 32); u is
//                   gathered with plain loads.  Edges: one partial sum of w_e eps_e^2 per chunk.
//   k_cell_shear    one lane per centre id, located through the cdof table (level, ijk): the four slots of each edge axis on the cell's
//                   own level, their children and grandchildren one and two levels down (rule 7 of avs_check_stress_indices), every
//                   index bounds-tested against its lattice and every id against n_edge before it addresses a rate.  One partial sum of
//                   w_c (exx^2 + eyy^2 + ezz^2) per chunk.
//   k_strain_fold   one workgroup per sum folds the partial sums in a fixed order.
//   k_paint_shear   (avs_paint.hpp, shared with avs_viscosity.hip) one lane per four x-adjacent cells of the simulation grid (one 16-byte
//                   store; per cell where the rows or the array do not allow it), x fastest: the lowest ACTIVE cell of the label pyramid
//                   over a cell names, by its centre id, the shear rate.  Only the field_n* window of a padded grid exists in the output.
//
// A partial sum belongs to a CHUNK, not to a workgroup: the sums do not depend on the grid (Options::cells_grid_cap).  Counters are
// 64-bit integers and the maxima the bit patterns of non-negative doubles: a lane accumulates in registers, a wave folds its lanes and
// issues one integer atomic per word it has something for (raw_add and raw_max_bits, avs_report_device.hpp).  No floating atomics: the
// same inputs give the same bytes.
#include <cmath>

#include "avs_device_common.hpp"
#include "avs_paint.hpp"
#include "avs_report_device.hpp"

namespace avs {

// raw summary: 64-bit words
enum {
    kStrainEmptyEdges = 0, kStrainEmptyCenters, kStrainBoundaryEdges, kStrainBoundaryCenters, kStrainNonfinite,
    kStrainLookups, // 4 words: AVS_EDGE_LOOKUP_*
    kStrainEmptyPairs = kStrainLookups + 4,
    kStrainMaxEdge, kStrainMaxCenter, kStrainMaxShear,        // bit patterns of non-negative finite doubles
    kStrainDissipationEdge, kStrainDissipationCenter,         // bit patterns, written by k_strain_fold
    kStrainRawWords
};

struct StrainStencils { // read-only StencilView
    int64_t count;
    const int32_t *cnt, *idx, *bcnt;
    const double *coef, *bval, *weight;
};

// EDGE: the stencils are the edge stresses (partial sums of w eps^2, when `partial` is given); else the centre lists
template <bool EDGE>
__global__ __launch_bounds__(kBlock) void k_strain_rates(StrainStencils S, int cap, int bcap, const double *__restrict__ u, long long n_vel,
                                                               double *__restrict__ rate, double *__restrict__ partial,
                                                               unsigned long long *__restrict__ raw)
{
    __shared__ double lds4[4];
    const long long count = S.count, chunks = (count + kBlock - 1) / kBlock;
    unsigned empty = 0u, boundary = 0u, nonfinite = 0u;
    double max_abs = 0.;
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) { // (the same trips for every thread of the workgroup)
        const long long s = chunk * kBlock + (long long)threadIdx.x;
        double term = 0.;
        if (s < count) {
            const int cnt = min(max(S.cnt[s], 0), cap), bcnt = min(max(S.bcnt[s], 0), bcap);
            double acc = 0.;
            for (int k = 0; k < cnt; ++k) {
                const int32_t id = S.idx[(size_t)k * (size_t)count + (size_t)s];
                const double cf = S.coef[(size_t)k * (size_t)count + (size_t)s];
                const double uv = (unsigned long long)(long long)id < (unsigned long long)n_vel ? u[id] : __longlong_as_double(0x7ff8000000000000ll); // (no such id: not a rate)
                acc = acc + cf * uv;
            }
            for (int k = 0; k < bcnt; ++k) acc = acc + S.bval[(size_t)k * (size_t)count + (size_t)s];
            rate[s] = acc;
            empty += cnt == 0;
            boundary += bcnt > 0;
            if (isfinite(acc)) {
                max_abs = fmax(max_abs, fabs(acc));
                if (EDGE) term = S.weight[s] * (acc * acc);
            } else {
                ++nonfinite;
            }
        }
        if (EDGE && partial) {
            const double t = block_sum(term, lds4);
            if (threadIdx.x == 0) partial[chunk] = t;
        }
    }
    raw_add(empty, EDGE ? kStrainEmptyEdges : kStrainEmptyCenters, raw);
    raw_add(boundary, EDGE ? kStrainBoundaryEdges : kStrainBoundaryCenters, raw);
    raw_add(nonfinite, kStrainNonfinite, raw);
    raw_max_bits(max_abs, EDGE ? kStrainMaxEdge : kStrainMaxCenter, raw);
}

// edge index of edge e of axis a at level l; outside the lattice: UNASSIGNED
__device__ __forceinline__ int strain_edge_index(const PyramidView &P, int l, int a, const I3 &e)
{
    const I3 r = edge_res(P, l, a);
    if ((unsigned)e[0] >= (unsigned)r[0] || (unsigned)e[1] >= (unsigned)r[1] || (unsigned)e[2] >= (unsigned)r[2]) return AVS_UNASSIGNED;
    return P.eidx[l][a][lin(r, e)];
}

__global__ __launch_bounds__(kBlock) void k_cell_shear(PyramidView P, const int32_t *__restrict__ cdof, long long n_center, long long n_edge,
                                                             const double *__restrict__ edge_rate, const double *__restrict__ center_rate,
                                                             const double *__restrict__ cw, double *__restrict__ cell, double *__restrict__ partial,
                                                             unsigned long long *__restrict__ raw)
{
    __shared__ double lds4[4];
    const long long chunks = (n_center + kBlock - 1) / kBlock;
    unsigned looked[4] = {0u, 0u, 0u, 0u}, empty_pairs = 0u;
    double max_shear = 0.;
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const long long cid = chunk * kBlock + (long long)threadIdx.x;
        double term = 0.;
        if (cid < n_center) {
            const int4 rec = *reinterpret_cast<const int4 *>(cdof + 4 * cid); // level | axis << 8, i, j, k
            const int l = rec.x & 0xff;
            const I3 C{{rec.y, rec.z, rec.w}};
            double m[3] = {0., 0., 0.};
            const bool located = l < P.levels; // (a table the library wrote always is)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int b = (a + 1) % 3, c = (a + 2) % 3;
                double sum = 0.;
                int n = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    I3 e = C;
                    e[b] += q & 1;
                    e[c] += q >> 1;
                    const int v = located ? strain_edge_index(P, l, a, e) : AVS_OUTSIDE;
                    if (v >= 0 && v < n_edge) {
                        ++looked[AVS_EDGE_LOOKUP_OWN];
                        sum = sum + edge_rate[v];
                        ++n;
                        continue;
                    }
                    double csum = 0.;
                    int cn = 0;
                    if (v == AVS_UNASSIGNED && l > 0) {
                        for (int h = 0; h < 2; ++h) {
                            I3 child{{2 * e[0], 2 * e[1], 2 * e[2]}};
                            child[a] += h;
                            const int w = strain_edge_index(P, l - 1, a, child);
                            if (w >= 0) {
                                if (w < n_edge) {
                                    ++looked[AVS_EDGE_LOOKUP_CHILD];
                                    csum = csum + edge_rate[w];
                                    ++cn;
                                }
                                continue;
                            }
                            if (l < 2) continue;
                            double gsum = 0.;
                            int gn = 0;
                            for (int g = 0; g < 2; ++g) {
                                I3 grand{{2 * child[0], 2 * child[1], 2 * child[2]}};
                                grand[a] += g;
                                const int x = strain_edge_index(P, l - 2, a, grand);
                                if (x >= 0 && x < n_edge) {
                                    ++looked[AVS_EDGE_LOOKUP_GRANDCHILD];
                                    gsum = gsum + edge_rate[x];
                                    ++gn;
                                }
                            }
                            if (gn) {
                                csum = csum + gsum / (double)gn;
                                ++cn;
                            }
                        }
                    }
                    if (cn) {
                        sum = sum + csum / (double)cn;
                        ++n;
                    } else {
                        ++looked[AVS_EDGE_LOOKUP_SKIPPED];
                    }
                }
                if (n) m[a] = sum / (double)n;
                else ++empty_pairs;
            }
            const double exx = center_rate[cid], eyy = center_rate[cid + n_center], ezz = center_rate[cid + 2 * n_center];
            const double normal = (exx * exx + eyy * eyy) + ezz * ezz;
            const double shear = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
            const double gamma = sqrt(2. * normal + 4. * shear);
            cell[cid] = gamma;
            if (isfinite(gamma)) max_shear = fmax(max_shear, gamma);
            if (isfinite(exx) && isfinite(eyy) && isfinite(ezz)) term = cw[cid] * normal;
        }
        if (partial) {
            const double t = block_sum(term, lds4);
            if (threadIdx.x == 0) partial[chunk] = t;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) raw_add(looked[k], kStrainLookups + k, raw);
    raw_add(empty_pairs, kStrainEmptyPairs, raw);
    raw_max_bits(max_shear, kStrainMaxShear, raw);
}

// workgroup 0: the edges' partial sums -> raw[kStrainDissipationEdge]; workgroup 1: the cells' -> raw[kStrainDissipationCenter].  Thread t adds
// the partial sums t, t + 256, ... in that order, then the block sum of avs_wave.hpp: a fixed order.
__global__ __launch_bounds__(kBlock) void k_strain_fold(const double *__restrict__ partial, long long n_first, long long n_second,
                                                              unsigned long long *__restrict__ raw)
{
    __shared__ double lds4[4];
    const double *p = blockIdx.x == 0 ? partial : partial + n_first;
    const long long n = blockIdx.x == 0 ? n_first : n_second;
    double s = 0.;
    for (long long i = threadIdx.x; i < n; i += kBlock) s = s + p[i];
    s = block_sum(s, lds4);
    if (threadIdx.x == 0) raw[blockIdx.x == 0 ? kStrainDissipationEdge : kStrainDissipationCenter] = (unsigned long long)__double_as_longlong(s);
}

// the shared implementation: any of the five outputs may be null (the entries have checked the arguments and the state)
avs_status strain_run(avs_ctx *c, int32_t which, double *edge_rate, double *center_rate, double *cell_shear, avs_strain_summary *summary,
                             float *field, avs_memspace where)
{
    StrainScratch &S = c->strain;
    hipStream_t st = c->stream;
    const long long ne = c->n_edge, nc = c->n_center, n3 = 3 * nc;
    const bool want_cell = cell_shear || summary || field, want_edge = edge_rate || want_cell, want_center = center_rate || want_cell;
    const bool direct = where == AVS_MEM_DEVICE;
    const double *u = which == AVS_RATES_OF_SOLUTION ? c->x.p : c->x0.p;
    const int cap = c->opt.cells_grid_cap;
    const long long chunks_e = (ne + kBlock - 1) / kBlock, chunks_c = (nc + kBlock - 1) / kBlock;

    double *d_edge = edge_rate, *d_center = center_rate, *d_cell = cell_shear;
    if (want_edge && !(direct && edge_rate)) { AVS_TRY(S.edge.reserve((size_t)ne)); d_edge = S.edge.p; }
    if (want_center && !(direct && center_rate)) { AVS_TRY(S.center.reserve((size_t)n3)); d_center = S.center.p; }
    if (want_cell && !(direct && cell_shear)) { AVS_TRY(S.cell.reserve((size_t)nc)); d_cell = S.cell.p; }
    double *d_partial = nullptr;
    if (summary) { AVS_TRY(S.partial.reserve((size_t)(chunks_e + chunks_c))); d_partial = S.partial.p; }
    AVS_TRY(S.raw.begin(kStrainRawWords, -1, st));

    if (want_edge && ne > 0) {
        const StrainStencils E{ne, c->e_cnt.p, c->e_idx.p, c->e_bcnt.p, c->e_coef.p, c->e_bval.p, c->e_w.p};
        hipLaunchKernelGGL(k_strain_rates<true>, dim3(report_grid(chunks_e, cap)), dim3(kBlock), 0, st, E, (int)AVS_EDGE_STENCIL_CAP,
                           (int)AVS_EDGE_BOUNDARY_CAP, u, (long long)c->n_vel, d_edge, d_partial, S.raw.p);
    }
    if (want_center && n3 > 0) {
        const StrainStencils C{n3, c->c_cnt.p, c->c_idx.p, c->c_bcnt.p, c->c_coef.p, c->c_bval.p, c->c_w.p};
        hipLaunchKernelGGL(k_strain_rates<false>, dim3(report_grid((n3 + kBlock - 1) / kBlock, cap)), dim3(kBlock), 0, st, C,
                           (int)AVS_CENTER_STENCIL_CAP, (int)AVS_CENTER_BOUNDARY_CAP, u, (long long)c->n_vel, d_center, (double *)nullptr, S.raw.p);
    }
    if (want_cell && nc > 0)
        hipLaunchKernelGGL(k_cell_shear, dim3(report_grid(chunks_c, cap)), dim3(kBlock), 0, st, c->view(), (const int32_t *)c->cdof.p, nc, ne,
                           (const double *)d_edge, (const double *)d_center, (const double *)c->c_w.p, d_cell, d_partial ? d_partial + chunks_e : nullptr,
                           S.raw.p);
    if (summary)
        hipLaunchKernelGGL(k_strain_fold, dim3(2), dim3(kBlock), 0, st, (const double *)d_partial, chunks_e, chunks_c, S.raw.p);
    float *d_field = field;
    const long long cells = (long long)c->desc.field_nx * c->desc.field_ny * c->desc.field_nz;
    if (field) {
        if (!direct) { AVS_TRY(S.field.reserve((size_t)cells)); d_field = S.field.p; }
        paint_launch(c, (const double *)d_cell, d_field);
    }
    AVS_HIP(hipGetLastError());
    if (!direct) { // staged: complete on return
        if (edge_rate) AVS_HIP(copy_out(edge_rate, d_edge, (size_t)ne * sizeof(double), where, st));
        if (center_rate) AVS_HIP(copy_out(center_rate, d_center, (size_t)n3 * sizeof(double), where, st));
        if (cell_shear) AVS_HIP(copy_out(cell_shear, d_cell, (size_t)nc * sizeof(double), where, st));
        if (field) AVS_HIP(copy_out(field, d_field, (size_t)cells * sizeof(float), where, st));
    }
    unsigned long long raw[kStrainRawWords];
    if (summary) AVS_TRY(S.raw.read(raw, st));
    else if (!direct) AVS_HIP(hipStreamSynchronize(st));
    if (!summary) return AVS_OK;
    avs_strain_summary full;
    memset(&full, 0, sizeof(full));
    full.struct_size = (int32_t)sizeof(full);
    full.which = which;
    full.n_edge = ne;
    full.n_center = nc;
    full.empty_edges = (int64_t)raw[kStrainEmptyEdges];
    full.empty_centers = (int64_t)raw[kStrainEmptyCenters];
    full.boundary_edges = (int64_t)raw[kStrainBoundaryEdges];
    full.boundary_centers = (int64_t)raw[kStrainBoundaryCenters];
    full.nonfinite = (int64_t)raw[kStrainNonfinite];
    for (int k = 0; k < 4; ++k) full.edge_lookups[k] = (int64_t)raw[kStrainLookups + k];
    full.empty_pairs = (int64_t)raw[kStrainEmptyPairs];
    const auto as_double = [&raw](int word) {
        double v;
        memcpy(&v, &raw[word], sizeof(v));
        return v;
    };
    full.dissipation_edge = as_double(kStrainDissipationEdge);
    full.dissipation_center = as_double(kStrainDissipationCenter);
    full.max_abs_edge_rate = as_double(kStrainMaxEdge);
    full.max_abs_center_rate = as_double(kStrainMaxCenter);
    full.max_shear_rate = as_double(kStrainMaxShear);
    report_hand_over(full, summary);
    return AVS_OK;
}

// arguments, then the state both entries need
avs_status strain_check(avs_ctx *c, const char *entry, int32_t which, const avs_strain_summary *summary, avs_memspace where)
{
    AVS_REQUIRE(which == AVS_RATES_OF_SOLUTION || which == AVS_RATES_OF_INITIAL_GUESS, AVS_EINVAL, "%s: unknown velocity %d", entry, (int)which);
    AVS_REQUIRE(where == AVS_MEM_HOST || where == AVS_MEM_DEVICE, AVS_EINVAL, "%s: unknown memory space %d", entry, (int)where);
    AVS_REQUIRE(!summary || report_size_ok(summary, offsetof(avs_strain_summary, which) + sizeof(int32_t)), AVS_EINVAL,
                "avs_strain_summary.struct_size must be set to sizeof(avs_strain_summary) before the call");
    AVS_REQUIRE(!c->slab.on, AVS_ESTATE, "%s: the context holds a slab-local pre-pass (this rank's window only)", entry);
    AVS_REQUIRE(c->stencils_ready && c->tables_ready, AVS_ESTATE, "%s: no stencils: call avs_build_stencils / avs_assemble first", entry);
    if (which == AVS_RATES_OF_SOLUTION)
        AVS_REQUIRE(c->solved && c->x.p, AVS_ESTATE, "%s: no solution: call avs_solve / avs_set_solution first", entry);
    else
        AVS_REQUIRE(c->guess_ready && !c->guess_partial && c->x0.p, AVS_ESTATE,
                    "%s: no initial guess: call avs_build_initial_guess / avs_assemble first", entry);
    for (int l = 0; l < c->desc.levels; ++l) { // (stencils imply them; the cell and paint passes address them)
        AVS_REQUIRE(c->have_labels[l] && c->labels[l].p && c->have_cidx[l] && c->cidx[l].p, AVS_ESTATE, "%s: labels / centre indices of level %d missing",
                    entry, l);
        for (int a = 0; a < 3; ++a)
            AVS_REQUIRE(c->have_eidx[l][a] && c->eidx[l][a].p, AVS_ESTATE, "%s: edge indices of level %d axis %d missing", entry, l, a);
    }
    AVS_REQUIRE(c->n_edge >= 0 && c->n_center >= 0 && c->n_center <= INT32_MAX / 3, AVS_ESTATE, "%s: DOF counts missing", entry);
    return AVS_OK;
}

} // namespace avs

using namespace avs;

extern "C" avs_status avs_get_strain_rates(avs_ctx *c, int32_t which, double *edge_rate, double *center_rate, double *cell_shear_rate,
                                           avs_strain_summary *summary, avs_memspace where)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c, AVS_EINVAL, "null argument");
    AVS_TRY(strain_check(c, "avs_get_strain_rates", which, summary, where));
    if (!edge_rate && !center_rate && !cell_shear_rate && !summary) return AVS_OK;
    AVS_HIP(hipSetDevice(c->desc.device));
    Scope scope("Strain Rates");
    return strain_run(c, which, edge_rate, center_rate, cell_shear_rate, summary, nullptr, where);
}

extern "C" avs_status avs_get_shear_rate_field(avs_ctx *c, int32_t which, float *field, avs_memspace where)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c && field, AVS_EINVAL, "null argument");
    AVS_TRY(strain_check(c, "avs_get_shear_rate_field", which, nullptr, where));
    AVS_HIP(hipSetDevice(c->desc.device));
    Scope scope("Shear Rate Field");
    return strain_run(c, which, nullptr, nullptr, nullptr, nullptr, field, where);
}
