// avs_paint.hpp -- a per-centre-id array painted onto the simulation grid through the label pyramid (avs_strain.hip: the cells' shear
// rates, avs_viscosity.hip: the cells' model viscosities).  One lane per four x-adjacent cells of the simulation grid (one 16-byte store;
// per cell where the rows or the array do not allow it), x fastest: the lowest ACTIVE cell of the label pyramid over a cell names, by its
// centre id, the value.  Only the field_n* window of a padded grid exists in the output.  T: the type of the per-id array (double: rounded
// once to float; float: copied).
#pragma once

#include "avs_device_common.hpp"
#include "avs_report_device.hpp"

namespace avs {

// the value over cell (x, y, z) of the simulation grid: the lowest level whose cell over it is ACTIVE (interp_find_level, avs_post.hip)
template <typename T>
__device__ __forceinline__ float paint_one(const PyramidView &P, long long n_center, const T *__restrict__ cell, int x, int y, int z)
{
    // the labels of every level are requested at once and the lowest ACTIVE one is picked: one memory round trip where a walk up from
    // level 0 makes `levels` dependent reads for every cell of the air
    int8_t lab[AVS_MAX_LEVELS];
#pragma unroll
    for (int l = 0; l < AVS_MAX_LEVELS; ++l) {
        lab[l] = AVS_INACTIVE;
        if (l < P.levels) {
            const I3 r = cell_res(P, l), c{{x >> l, y >> l, z >> l}};
            if (c[0] < r[0] && c[1] < r[1] && c[2] < r[2]) lab[l] = P.labels[l][lin(r, c)];
        }
    }
    int found = -1;
#pragma unroll
    for (int l = AVS_MAX_LEVELS - 1; l >= 0; --l)
        if (lab[l] == AVS_ACTIVE) found = l;
    if (found < 0) return 0.f;
    const I3 r = cell_res(P, found), c{{x >> found, y >> found, z >> found}};
    const int cid = P.cidx[found][lin(r, c)];
    return cid >= 0 && cid < n_center ? (float)cell[cid] : 0.f;
}

// the same for the four cells x .. x + 3 of one row, x a multiple of 4 (and so is the lattice's x extent, and the level-0 lattice starts on a
// 4-byte boundary): the quad shares one 32-bit word of level-0 labels, two labels of level 1 and one label of every level above
template <typename T>
__device__ __forceinline__ float4 paint_quad(const PyramidView &P, long long n_center, const T *__restrict__ cell, int x, int y, int z)
{
    const unsigned lab0 = *reinterpret_cast<const unsigned *>(P.labels[0] + lin(cell_res(P, 0), I3{{x, y, z}}));
    int8_t lab[AVS_MAX_LEVELS], lab1b = AVS_INACTIVE; // lab[l], l >= 1: over x (from level 2 up: over all four); lab1b: level 1 over x + 2
#pragma unroll
    for (int l = 1; l < AVS_MAX_LEVELS; ++l) {
        lab[l] = AVS_INACTIVE;
        if (l < P.levels) {
            const I3 r = cell_res(P, l), c{{x >> l, y >> l, z >> l}};
            if (c[0] < r[0] && c[1] < r[1] && c[2] < r[2]) {
                lab[l] = P.labels[l][lin(r, c)];
                if (l == 1 && c[0] + 1 < r[0]) lab1b = P.labels[1][lin(r, c) + 1];
            }
        }
    }
    float out[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        int found = -1;
#pragma unroll
        for (int l = AVS_MAX_LEVELS - 1; l >= 2; --l)
            if (lab[l] == AVS_ACTIVE) found = l;
        if ((w < 2 ? lab[1] : lab1b) == AVS_ACTIVE) found = 1;
        if ((int8_t)(lab0 >> (8 * w)) == AVS_ACTIVE) found = 0;
        out[w] = 0.f;
        if (found >= 0) {
            const I3 r = cell_res(P, found), c{{(x + w) >> found, y >> found, z >> found}};
            const int cid = P.cidx[found][lin(r, c)];
            if (cid >= 0 && cid < n_center) out[w] = (float)cell[cid];
        }
    }
    return make_float4(out[0], out[1], out[2], out[3]);
}

// field: the simulation grid (fx, fy, fz), x fastest = the lower corner of the octree grid (the padding lies beyond it).  A thread paints W
// x-adjacent cells of one row: W = 4 (one 16-byte store) where fx and nx are multiples of 4, the array starts on a 16-byte boundary and the
// level-0 labels on a 4-byte one, else 1.
template <int W, typename T>
__global__ __launch_bounds__(kBlock) void k_paint_shear(PyramidView P, long long n_center, const T *__restrict__ cell, int fx, int fy, int fz,
                                                              float *__restrict__ field)
{
    const int gx = fx / W; // groups per row
    const long long groups = (long long)gx * fy * fz;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (long long)gridDim.x * kBlock) {
        int x, y, z;
        if (groups <= 0xffffffffll) { // 32-bit division where the grid allows it
            const unsigned row = (unsigned)g / (unsigned)gx;
            x = (int)((unsigned)g - row * (unsigned)gx) * W, y = (int)(row % (unsigned)fy), z = (int)(row / (unsigned)fy);
        } else {
            x = (int)(g % gx) * W, y = (int)(g / gx % fy), z = (int)(g / ((long long)gx * fy));
        }
        if (W == 4) {
            *reinterpret_cast<float4 *>(field + 4 * g) = paint_quad(P, n_center, cell, x, y, z); // (cell x + fx (y + fy z) = 4 g)
        } else {
            field[g] = paint_one(P, n_center, cell, x, y, z);
        }
    }
}

// the alignment rule of the 16-byte stores, for a dense array of the simulation grid that starts at `field`
inline bool paint_quads_ok(const avs_ctx *c, const void *field)
{
    return c->desc.field_nx % 4 == 0 && c->desc.nx % 4 == 0 && (reinterpret_cast<uintptr_t>(field) & 15u) == 0 &&
           (reinterpret_cast<uintptr_t>(c->labels[0].p) & 3u) == 0;
}

// paints `cell` (n_center values by centre id) into the device array `field` on the context's stream
template <typename T>
inline void paint_launch(avs_ctx *c, const T *cell, float *field)
{
    const long long cells = (long long)c->desc.field_nx * c->desc.field_ny * c->desc.field_nz;
    const bool quads = paint_quads_ok(c, field);
    const long long groups = quads ? cells / 4 : cells;
    const auto kernel = quads ? k_paint_shear<4, T> : k_paint_shear<1, T>;
    hipLaunchKernelGGL(kernel, dim3(report_grid((groups + kBlock - 1) / kBlock, c->opt.cells_grid_cap)),
                       dim3(kBlock), 0, c->stream, c->view(), (long long)c->n_center, cell, c->desc.field_nx, c->desc.field_ny, c->desc.field_nz,
                       field);
}

} // namespace avs
