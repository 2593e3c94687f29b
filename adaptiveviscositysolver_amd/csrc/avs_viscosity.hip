// avs_viscosity.hip -- a shear-dependent viscosity model evaluated on the device and, if asked for, installed as the context's
// AVS_FIELD_VISCOSITY (avs_apply_viscosity_model; every value is defined in include/avs.h, tests/viscosity_model.py restates them in NumPy).
//
//   strain_run            (avs_strain.hip) the cells' shear rates g, fp64, into StrainScratch::cell
//   k_viscosity_model     one lane per centre id: m(g) in fp64, clamped, rounded once to P = (float)m > 0; 0 marks an id without a value
//   k_paint_shear<W, float> (avs_paint.hpp) P painted onto the simulation grid through the label pyramid: 0 = not covered
//   k_viscosity_cells<W>  one workgroup per 64 x 4W column of the simulation grid, marched along z in chunks of kViscZ planes with the
//                         planes z - 1, z, z + 1 of the painted array (and their one-cell rim) in LDS: a covered cell takes P, a cell next to a covered one
//                         the mean of its covered neighbours, any other cell keeps its viscosity; relaxation against the context's
//                         viscosity; the result goes to the caller's array and / or into the window of the padded lattice of the next
//                         install.  W = 4: 16-byte loads and stores (the rule of k_paint_shear), else per cell.
//   k_viscosity_border    the padding of that lattice: every cell outside the window copies the nearest cell of the window.
//
// Counters and extrema are folded as in avs_strain.hip: registers, one wave fold, one integer atomic per word (bit patterns of positive
// floats / non-negative doubles order as their values).  No floating atomics: the same inputs give the same bytes for every grid size.
#include <cfloat>
#include <cmath>

#include "avs_device_common.hpp"
#include "avs_paint.hpp"
#include "avs_report_device.hpp"
#ifdef AVS_PROBES
#include "avs_probe.h"
#endif

namespace avs {

// raw summary: 64-bit words
enum {
    kViscCovered = 0, kViscFringe, kViscUntouched, kViscClampedLow, kViscClampedHigh, kViscNonfinite,
    kViscMaxViscosity,             // bit pattern of a positive float
    kViscMaxShear, kViscMaxChange, // bit patterns of non-negative doubles
    kViscMinViscosity,             // bit pattern of a positive float; all ones: no covered cell
    kViscRawWords
};

constexpr int kViscTileX = 64; // cells of a row a workgroup holds
constexpr int kViscZ = 16;     // planes a workgroup marches through per tile

struct ViscosityParams { // avs_viscosity_model, checked
    int kind;
    double mu_0, mu_inf, lambda, a, n, consistency, tau_y, regularisation, mu_min, mu_max;
};

__global__ __launch_bounds__(kBlock) void k_viscosity_model(ViscosityParams M, const double *__restrict__ shear, const int32_t *__restrict__ cdof,
                                                                  long long n_center, int fx, int fy, int fz, float *__restrict__ model,
                                                                  unsigned long long *__restrict__ raw)
{
    const long long chunks = (n_center + kBlock - 1) / kBlock;
    unsigned low = 0u, high = 0u, nonfinite = 0u;
    double max_shear = 0.;
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const long long cid = chunk * kBlock + (long long)threadIdx.x;
        if (cid >= n_center) continue;
        const double g = shear[cid];
        double m;
        if (M.kind == AVS_VISCOSITY_CARREAU_YASUDA) {
            m = M.mu_inf + (M.mu_0 - M.mu_inf) * pow(1. + pow(M.lambda * g, M.a), (M.n - 1.) / M.a);
        } else {
            m = M.consistency * pow(g, M.n - 1.);
            if (M.tau_y != 0.) {
                const double y = g == 0. ? M.tau_y * M.regularisation : M.tau_y * (-expm1(-M.regularisation * g)) / g;
                m = m + y;
            }
        }
        float p = 0.f;
        if (!finite_bits(g) || m != m) {
            ++nonfinite;
        } else {
            if (m < M.mu_min) {
                m = M.mu_min;
                ++low;
            } else if (m > M.mu_max) {
                m = M.mu_max;
                ++high;
            }
            p = (float)m;
            // the id gives cells of the simulation grid their value: its cell starts inside the window
            const int4 rec = *reinterpret_cast<const int4 *>(cdof + 4 * cid); // level | axis << 8, i, j, k
            const int l = rec.x & 0xff;
            if (l < AVS_MAX_LEVELS && ((long long)rec.y << l) < fx && ((long long)rec.z << l) < fy && ((long long)rec.w << l) < fz)
                max_shear = fmax(max_shear, g);
        }
        model[cid] = p;
    }
    raw_add(low, kViscClampedLow, raw);
    raw_add(high, kViscClampedHigh, raw);
    raw_add(nonfinite, kViscNonfinite, raw);
    raw_max_bits(max_shear, kViscMaxShear, raw);
}

struct ViscosityCells {
    const float *painted;    // (fx, fy, fz), x fastest
    int fx, fy, fz;
    const float *old;        // the context's viscosity lattice (nx, ny, .), or null: old_const
    float old_const;
    int nx, ny;
    float *out_dense;        // (fx, fy, fz) or null
    float *out_lattice;      // (nx, ny, .): the window is written; or null
    double relaxation;
};

// W x-adjacent cells per thread; the workgroup's tile: kViscTileX x (4 W) cells of kViscZ planes.  Four plane slots: the plane staged
// for z + 1 never lands on one of the three the cells of z - 1 may still be reading, so one barrier per plane suffices -- the one that
// also ORs "this plane holds a covered cell" over the workgroup.  Three empty planes (most tiles of a scene are air): every cell of the
// tile's plane keeps its viscosity, and no neighbourhood is read.  A row in LDS: [3 unused | rim | 64 cells | rim | 3 unused], so that
// the cells start on a 16-byte boundary and W = 4 stages and reads them as quads.
template <int W>
__global__ __launch_bounds__(kBlock) void k_viscosity_cells(ViscosityCells A, unsigned long long *__restrict__ raw)
{
    constexpr int TY = kBlock * W / kViscTileX, XO = 3, PX = kViscTileX + 8, PY = TY + 2, QX = kViscTileX / 4;
    __shared__ __align__(16) float plane[4][PY][PX];
    const int tiles_x = (A.fx + kViscTileX - 1) / kViscTileX, tiles_y = (A.fy + TY - 1) / TY, tiles_z = (A.fz + kViscZ - 1) / kViscZ;
    const long long tiles = (long long)tiles_x * tiles_y * tiles_z;
    const int tid = (int)threadIdx.x, lx0 = tid % (kViscTileX / W) * W, ly = tid / (kViscTileX / W);
    unsigned covered = 0u, fringe = 0u, untouched = 0u;
    unsigned long long min_bits = kNoKey, max_bits = 0ull;
    double max_change = 0.;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) { // (the same trips for every thread of the workgroup)
        const int x0 = (int)(tile % tiles_x) * kViscTileX, y0 = (int)(tile / tiles_x % tiles_y) * TY, z0 = (int)(tile / ((long long)tiles_x * tiles_y)) * kViscZ;
        const int z1 = min(z0 + kViscZ, A.fz);
        // plane zz of the painted array with its rim into slot (zz + 4) % 4; outside the simulation grid: 0, not covered.  Returns whether
        // this thread staged a covered cell.
        const auto stage = [&](int zz) {
            float(*dst)[PX] = plane[(zz + 4) & 3];
            const bool z_in = (unsigned)zz < (unsigned)A.fz;
            bool any = false;
            if constexpr (W == 4) { // (fx is a multiple of 4 and the array starts on a 16-byte boundary: so does every quad of a row)
                // PY * QX = 288 quads and 2 PY = 36 rim cells for 256 threads: every thread takes quad `tid`, the first 32 a second quad, the
                // next 36 a rim cell -- at most two loads a thread, both requested before either is parked in LDS (one memory round trip per
                // plane; a loop over the items made two or three for the threads the barrier waits for)
                constexpr int kSecond = PY * QX - kBlock;
                static_assert(kSecond >= 0 && kSecond + 2 * PY <= kBlock, "a quad, and a second quad or a rim cell, per thread");
                const auto quad_at = [&](int i, int &py, int &q) {
                    py = i / QX, q = i - py * QX;
                    const int gx = x0 + 4 * q, gy = y0 + py - 1;
                    return z_in && gx < A.fx && (unsigned)gy < (unsigned)A.fy
                               ? *reinterpret_cast<const float4 *>(A.painted + ((size_t)gx + (size_t)A.fx * ((size_t)gy + (size_t)A.fy * (size_t)zz)))
                               : make_float4(0.f, 0.f, 0.f, 0.f);
                };
                int py0, q0, py1 = 0, q1 = 0, rim_py = 0, rim_px = 0;
                const float4 v0 = quad_at(tid, py0, q0);
                float4 v1 = make_float4(0.f, 0.f, 0.f, 0.f);
                float rim = 0.f;
                const int r = tid - kSecond;
                if (tid < kSecond) {
                    v1 = quad_at(tid + kBlock, py1, q1);
                } else if (r < 2 * PY) {
                    rim_py = r >> 1, rim_px = (r & 1) * (kViscTileX + 1);
                    const int gx = x0 + rim_px - 1, gy = y0 + rim_py - 1;
                    if (z_in && (unsigned)gx < (unsigned)A.fx && (unsigned)gy < (unsigned)A.fy)
                        rim = A.painted[(size_t)gx + (size_t)A.fx * ((size_t)gy + (size_t)A.fy * (size_t)zz)];
                }
                *reinterpret_cast<float4 *>(&dst[py0][XO + 1 + 4 * q0]) = v0;
                if (tid < kSecond) *reinterpret_cast<float4 *>(&dst[py1][XO + 1 + 4 * q1]) = v1;
                else if (r < 2 * PY) dst[rim_py][XO + rim_px] = rim;
                any = v0.x > 0.f || v0.y > 0.f || v0.z > 0.f || v0.w > 0.f || v1.x > 0.f || v1.y > 0.f || v1.z > 0.f || v1.w > 0.f || rim > 0.f;
            } else {
                for (int i = tid; i < PY * (kViscTileX + 2); i += kBlock) {
                    const int py = i / (kViscTileX + 2), px = i - py * (kViscTileX + 2), gx = x0 + px - 1, gy = y0 + py - 1;
                    float v = 0.f;
                    if (z_in && (unsigned)gx < (unsigned)A.fx && (unsigned)gy < (unsigned)A.fy)
                        v = A.painted[(size_t)gx + (size_t)A.fx * ((size_t)gy + (size_t)A.fy * (size_t)zz)];
                    dst[py][XO + px] = v;
                    any |= v > 0.f;
                }
            }
            return any ? 1 : 0;
        };
        __syncthreads(); // (the cells of the tile before may still be reading the slots)
        const int staged_below = stage(z0 - 1), staged_here = stage(z0);
        int any_below = __syncthreads_or(staged_below), any_here = __syncthreads_or(staged_here);
        for (int z = z0; z < z1; ++z) {
            const int any_above = __syncthreads_or(stage(z + 1));
            const bool near_liquid = any_below | any_here | any_above; // (the same for every thread of the workgroup)
            any_below = any_here;
            any_here = any_above;
            const int x = x0 + lx0, y = y0 + ly;
            if (x < A.fx && y < A.fy) { // (W == 4: fx is a multiple of 4, the quad is inside with its first cell)
                const size_t at_dense = (size_t)x + (size_t)A.fx * ((size_t)y + (size_t)A.fy * (size_t)z);
                const size_t at_lattice = (size_t)x + (size_t)A.nx * ((size_t)y + (size_t)A.ny * (size_t)z);
                float old[W], out[W];
                if (!A.old) {
#pragma unroll
                    for (int w = 0; w < W; ++w) old[w] = A.old_const;
                } else if (W == 4) {
                    const float4 o = *reinterpret_cast<const float4 *>(A.old + at_lattice);
                    old[0] = o.x, old[1 % W] = o.y, old[2 % W] = o.z, old[3 % W] = o.w;
                } else {
                    old[0] = A.old[at_lattice];
                }
                if (!near_liquid) {
                    untouched += W;
#pragma unroll
                    for (int w = 0; w < W; ++w) out[w] = old[w];
                } else {
                    const int cy = ly + 1; // the thread's row inside the staged planes
                    float here[W];
                    if (W == 4) {
                        const float4 c = *reinterpret_cast<const float4 *>(&plane[z & 3][cy][XO + 1 + lx0]);
                        here[0] = c.x, here[1 % W] = c.y, here[2 % W] = c.z, here[3 % W] = c.w;
                    } else {
                        here[0] = plane[z & 3][cy][XO + 1 + lx0];
                    }
#pragma unroll
                    for (int w = 0; w < W; ++w) {
                        const int cx = XO + 1 + lx0 + w;
                        float m = here[w];
                        const bool is_covered = m > 0.f;
                        bool keep = false;
                        if (is_covered) {
                            ++covered;
                        } else {
                            double sum = 0.;
                            int count = 0;
                            for (int dz = -1; dz <= 1; ++dz) {
                                const float(*src)[PX] = plane[(z + dz + 4) & 3];
                                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                                    for (int dx = -1; dx <= 1; ++dx) {
                                        const float v = src[cy + dy][cx + dx];
                                        if (v > 0.f) {
                                            sum = sum + (double)v;
                                            ++count;
                                        }
                                    }
                            }
                            if (count) {
                                ++fringe;
                                m = (float)(sum / (double)count);
                            } else {
                                ++untouched;
                                keep = true;
                            }
                        }
                        const float o = old[w];
                        const float v = keep ? o : (A.relaxation == 1. ? m : (float)((double)o + A.relaxation * ((double)m - (double)o)));
                        out[w] = v;
                        if (is_covered) { // extrema: over covered cells
                            const unsigned long long bits = (unsigned long long)__float_as_uint(m);
                            min_bits = bits < min_bits ? bits : min_bits;
                            max_bits = bits > max_bits ? bits : max_bits;
                            if (o > 0.f) {
                                const double change = fabs((double)v - (double)o) / (double)o;
                                if (change == change) max_change = fmax(max_change, change);
                            }
                        }
                    }
                }
                if (W == 4) {
                    const float4 q = make_float4(out[0], out[1 % W], out[2 % W], out[3 % W]);
                    if (A.out_dense) *reinterpret_cast<float4 *>(A.out_dense + at_dense) = q;
                    if (A.out_lattice) *reinterpret_cast<float4 *>(A.out_lattice + at_lattice) = q;
                } else {
                    if (A.out_dense) A.out_dense[at_dense] = out[0];
                    if (A.out_lattice) A.out_lattice[at_lattice] = out[0];
                }
            }
        }
    }
    raw_add(covered, kViscCovered, raw);
    raw_add(fringe, kViscFringe, raw);
    raw_add(untouched, kViscUntouched, raw);
    raw_min(min_bits, kViscMinViscosity, raw);
    raw_max_bits(max_bits, kViscMaxViscosity, raw);
    raw_max_bits(max_change, kViscMaxChange, raw);
}

// the cells of the lattice (nx, ny, nz) outside its window (fx, fy, fz), in three slabs (z >= fz; z < fz and y >= fy; z < fz, y < fy and
// x >= fx): each copies the nearest cell of the window -- the border replication of avs_set_scalar_field.  Cells of the window are read only.
__global__ __launch_bounds__(kBlock) void k_viscosity_border(float *__restrict__ lattice, int nx, int ny, int nz, int fx, int fy, int fz)
{
    const long long na = (long long)nx * ny * (nz - fz), nb = (long long)nx * (ny - fy) * fz, nc = (long long)(nx - fx) * fy * fz;
    for (long long o = (long long)blockIdx.x * kBlock + threadIdx.x; o < na + nb + nc; o += (long long)gridDim.x * kBlock) {
        int i, j, k;
        if (o < na) {
            i = (int)(o % nx), j = (int)(o / nx % ny), k = fz + (int)(o / ((long long)nx * ny));
        } else if (o < na + nb) {
            const long long q = o - na;
            i = (int)(q % nx), j = fy + (int)(q / nx % (ny - fy)), k = (int)(q / ((long long)nx * (ny - fy)));
        } else {
            const long long q = o - na - nb;
            i = fx + (int)(q % (nx - fx)), j = (int)(q / (nx - fx) % fy), k = (int)(q / ((long long)(nx - fx) * fy));
        }
        const int ci = min(i, fx - 1), cj = min(j, fy - 1), ck = min(k, fz - 1);
        lattice[(size_t)i + (size_t)nx * ((size_t)j + (size_t)ny * (size_t)k)] = lattice[(size_t)ci + (size_t)nx * ((size_t)cj + (size_t)ny * (size_t)ck)];
    }
}

// the parameters the chosen kind reads, the clamp and the relaxation; the message names the parameter
static avs_status viscosity_model_check(const avs_viscosity_model *m)
{
    AVS_REQUIRE(m->struct_size >= (int32_t)sizeof(avs_viscosity_model) && m->struct_size <= 4096, AVS_EINVAL,
                "avs_viscosity_model.struct_size must be set to sizeof(avs_viscosity_model) before the call");
    AVS_REQUIRE(m->kind == AVS_VISCOSITY_CARREAU_YASUDA || m->kind == AVS_VISCOSITY_HERSCHEL_BULKLEY, AVS_EINVAL,
                "avs_viscosity_model.kind: unknown model %d", (int)m->kind);
    const auto finite_nonneg = [](double v) { return std::isfinite(v) && v >= 0.; };
    if (m->kind == AVS_VISCOSITY_CARREAU_YASUDA) {
        AVS_REQUIRE(finite_nonneg(m->mu_0), AVS_EINVAL, "avs_viscosity_model.mu_0 must be finite and >= 0");
        AVS_REQUIRE(finite_nonneg(m->mu_inf), AVS_EINVAL, "avs_viscosity_model.mu_inf must be finite and >= 0");
        AVS_REQUIRE(finite_nonneg(m->lambda), AVS_EINVAL, "avs_viscosity_model.lambda must be finite and >= 0");
        AVS_REQUIRE(std::isfinite(m->a) && m->a > 0., AVS_EINVAL, "avs_viscosity_model.a must be finite and > 0");
        AVS_REQUIRE(std::isfinite(m->n), AVS_EINVAL, "avs_viscosity_model.n must be finite");
    } else {
        AVS_REQUIRE(finite_nonneg(m->consistency), AVS_EINVAL, "avs_viscosity_model.consistency must be finite and >= 0");
        AVS_REQUIRE(std::isfinite(m->n), AVS_EINVAL, "avs_viscosity_model.n must be finite");
        AVS_REQUIRE(finite_nonneg(m->tau_y), AVS_EINVAL, "avs_viscosity_model.tau_y must be finite and >= 0");
        AVS_REQUIRE(finite_nonneg(m->regularisation) && (m->tau_y == 0. || m->regularisation > 0.), AVS_EINVAL,
                    "avs_viscosity_model.regularisation must be finite and >= 0, and > 0 with a yield stress");
    }
    AVS_REQUIRE(std::isfinite(m->mu_min) && (float)m->mu_min > 0.f, AVS_EINVAL, "avs_viscosity_model.mu_min must be finite and > 0 as a float");
    AVS_REQUIRE(std::isfinite(m->mu_max) && m->mu_max <= (double)FLT_MAX && m->mu_min <= m->mu_max, AVS_EINVAL,
                "avs_viscosity_model.mu_max must be finite as a float and >= mu_min");
    AVS_REQUIRE(m->relaxation > 0. && m->relaxation <= 1., AVS_EINVAL, "avs_viscosity_model.relaxation must be in (0, 1]");
    return AVS_OK;
}

static avs_status viscosity_run(avs_ctx *c, int32_t which, const avs_viscosity_model *m, float *mu_out, bool install, avs_viscosity_summary *summary,
                                avs_memspace where)
{
    ViscosityScratch &V = c->viscosity;
    hipStream_t st = c->stream;
    const avs_desc &d = c->desc;
    const long long nc = c->n_center, cells = (long long)d.field_nx * d.field_ny * d.field_nz, lattice = (long long)d.nx * d.ny * d.nz;
    const int cap = c->opt.cells_grid_cap;
    const bool direct = where == AVS_MEM_DEVICE;

    // g per centre id, in place in the strain scratch
    AVS_TRY(c->strain.cell.reserve((size_t)nc));
    AVS_TRY(strain_run(c, which, nullptr, nullptr, c->strain.cell.p, nullptr, nullptr, AVS_MEM_DEVICE));
    AVS_TRY(V.model.reserve((size_t)nc));
    AVS_TRY(V.painted.reserve((size_t)cells));
    AVS_TRY(V.raw.begin(kViscRawWords, kViscMinViscosity, st));
    if (nc > 0) {
        const ViscosityParams P{m->kind, m->mu_0, m->mu_inf, m->lambda, m->a, m->n, m->consistency, m->tau_y, m->regularisation, m->mu_min, m->mu_max};
        hipLaunchKernelGGL(k_viscosity_model, dim3(report_grid((nc + kBlock - 1) / kBlock, cap)), dim3(kBlock), 0, st, P, (const double *)c->strain.cell.p,
                           (const int32_t *)c->cdof.p, nc, d.field_nx, d.field_ny, d.field_nz, V.model.p, V.raw.p);
    }
    paint_launch(c, (const float *)V.model.p, V.painted.p);

    float *d_out = mu_out;
    if (mu_out && !direct) { AVS_TRY(V.out.reserve((size_t)cells)); d_out = V.out.p; }
    if (install) AVS_TRY(V.next.alloc((size_t)lattice));
    const bool have_old = !c->visc.is_const && c->visc.buf.p;
    const ViscosityCells A{V.painted.p, d.field_nx, d.field_ny, d.field_nz, have_old ? c->visc.buf.p : nullptr, c->visc.cval, d.nx, d.ny, d_out,
                           install ? V.next.p : nullptr, m->relaxation};
    // 16-byte loads and stores: the rule of k_paint_shear for the dense array; the rows of the lattices then start on 16-byte boundaries too
    const bool quads = d.field_nx % 4 == 0 && d.nx % 4 == 0 && (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0 &&
                       (reinterpret_cast<uintptr_t>(A.old) & 15u) == 0 && (reinterpret_cast<uintptr_t>(A.out_lattice) & 15u) == 0;
    const int ty = quads ? 16 : 4;
    const long long tiles = (long long)((d.field_nx + kViscTileX - 1) / kViscTileX) * ((d.field_ny + ty - 1) / ty) * ((d.field_nz + kViscZ - 1) / kViscZ);
    hipLaunchKernelGGL(quads ? k_viscosity_cells<4> : k_viscosity_cells<1>, dim3(report_grid(tiles, cap)), dim3(kBlock), 0, st, A, V.raw.p);
    if (install && lattice > cells)
        hipLaunchKernelGGL(k_viscosity_border, dim3(report_grid((lattice - cells + kBlock - 1) / kBlock, cap)), dim3(kBlock), 0, st, V.next.p, d.nx,
                           d.ny, d.nz, d.field_nx, d.field_ny, d.field_nz);
    AVS_HIP(hipGetLastError());
    if (mu_out && !direct) AVS_HIP(copy_out(mu_out, d_out, (size_t)cells * sizeof(float), where, st));
    unsigned long long raw[kViscRawWords];
    if (summary) AVS_TRY(V.raw.read(raw, st));
    else if (mu_out && !direct) AVS_HIP(hipStreamSynchronize(st));
    // the pass has read the old lattice and written the next one on the context's stream: they trade places
    if (install) AVS_TRY(install_viscosity_lattice(c, V.next));
    if (!summary) return AVS_OK;
    avs_viscosity_summary full;
    memset(&full, 0, sizeof(full));
    full.struct_size = (int32_t)sizeof(full);
    full.which = which;
    full.kind = m->kind;
    full.installed = install ? 1 : 0;
    full.n_center = nc;
    full.covered = (int64_t)raw[kViscCovered];
    full.fringe = (int64_t)raw[kViscFringe];
    full.untouched = (int64_t)raw[kViscUntouched];
    full.clamped_low = (int64_t)raw[kViscClampedLow];
    full.clamped_high = (int64_t)raw[kViscClampedHigh];
    full.nonfinite = (int64_t)raw[kViscNonfinite];
    const auto as_float = [&raw](int word) {
        const uint32_t bits = (uint32_t)raw[word];
        float v;
        memcpy(&v, &bits, sizeof(v));
        return (double)v;
    };
    const auto as_double = [&raw](int word) {
        double v;
        memcpy(&v, &raw[word], sizeof(v));
        return v;
    };
    full.min_viscosity = raw[kViscMinViscosity] == kNoKey ? 0. : as_float(kViscMinViscosity);
    full.max_viscosity = as_float(kViscMaxViscosity);
    full.max_shear_rate = as_double(kViscMaxShear);
    full.max_relative_change = as_double(kViscMaxChange);
    report_hand_over(full, summary);
    return AVS_OK;
}

} // namespace avs

using namespace avs;

extern "C" avs_status avs_apply_viscosity_model(avs_ctx *c, int32_t which, const avs_viscosity_model *model, float *mu_out, int32_t install,
                                                avs_viscosity_summary *summary, avs_memspace where)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c && model, AVS_EINVAL, "null argument");
    AVS_TRY(strain_check(c, "avs_apply_viscosity_model", which, nullptr, where));
    AVS_REQUIRE(!summary || report_size_ok(summary, offsetof(avs_viscosity_summary, which) + sizeof(int32_t)), AVS_EINVAL,
                "avs_viscosity_summary.struct_size must be set to sizeof(avs_viscosity_summary) before the call");
    AVS_TRY(viscosity_model_check(model));
    if (!mu_out && !install && !summary) return AVS_OK;
    AVS_HIP(hipSetDevice(c->desc.device));
    Scope scope("Viscosity Model");
    return viscosity_run(c, which, model, mu_out, install != 0, summary, where);
}

#ifdef AVS_PROBES
extern "C" avs_status avs_viscosity_lattice_probe(avs_ctx *c, float *lattice, float *constant, int32_t *is_const, avs_memspace where)
{
    AVS_REQUIRE(c && constant && is_const, AVS_EINVAL, "null argument");
    AVS_REQUIRE(where == AVS_MEM_HOST || where == AVS_MEM_DEVICE, AVS_EINVAL, "unknown memory space %d", (int)where);
    AVS_HIP(hipSetDevice(c->desc.device));
    const bool field = !c->visc.is_const && c->visc.buf.p;
    *is_const = field ? 0 : 1;
    *constant = c->visc.cval;
    if (field && lattice) {
        AVS_HIP(copy_out(lattice, c->visc.buf.p, (size_t)c->desc.nx * c->desc.ny * c->desc.nz * sizeof(float), where, c->stream));
        AVS_HIP(hipStreamSynchronize(c->stream));
    }
    return AVS_OK;
}
#endif
