// avs_refine.hpp -- indicator-driven refinement flags of the pre-pass (avs_prepass_set_refinement, include/avs.h): the bit lattice the
// mask kernel (k_mask_labels, avs_prepass.hip) reads, and the host entries of avs_refine.hip that fill and expand it.
#pragma once

#include "avs_internal.hpp"

namespace avs {

// Flags of the OCTREE centre lattice at one bit per cell: wx = ceil(nx / 32) words per x row, rows in (y, z) order, bit (i & 31) of word
// i >> 5 is cell i.  128 MiB at 1024^3 (an int8 lattice is 1 GiB next to lattices that already fill the card).  Cells outside the
// simulation grid hold 0.
// `refined` is counted with one atomic per wave of the mask kernel.  Into ONE word that is 0.1 M (512^3 beam) to 4 M atomics at the ~11 ns
// a contended word takes each -- measured: + 1.1 ms on a 0.5-ms octree phase -- so the waves spread over kRefinedSlots words in cache
// lines of their own and the host adds them up.
constexpr int kRefinedSlots = 256, kRefinedStride = 16 /* words of 8 B: 128 B */, kRefinedBase = 16;
constexpr int kRefineCounters = kRefinedBase + kRefinedSlots * kRefinedStride;

struct RefineState {
    DevBuf<uint32_t> bits, tmp;          // the flags / the dilation's second lattice (allocated by the first call that dilates); kept
    DevBuf<unsigned long long> counters; // [0] seeds, [1] flagged (set call); from kRefinedBase: the slots of refined (mask kernel of the last run)
    int wx = 0;
    bool active = false;
    int32_t dilate = 0;
    float threshold = 0.f;
    int64_t seeds = 0, flagged = 0, refined = 0;
    double set_ms = 0.;
};

// what the flagged instantiation of k_mask_labels is given (by value)
struct RefineView {
    const uint32_t *bits;
    int wx;
    int axis, lo, hi;            // `refined` counts the cells whose coordinate along `axis` lies in [lo, hi): the rank's window
    unsigned long long *refined; // kRefinedSlots slots, kRefinedStride apart
};

inline int refine_row_words(int nx) { return (nx + 31) / 32; }

// indicator (device, sim[0] x sim[1] x sim[2], x fastest) -> seeds -> box dilation by `dilate` cells clipped at the simulation grid, on
// the bit lattice of the oct[0] x oct[1] x oct[2] octree grid; counts and the kernels' time into S.  Returns after the stream has drained.
avs_status refine_set(RefineState &S, const float *indicator, const int sim[3], const int oct[3], float threshold, int dilate, hipStream_t st);
// the flags as 0 / 1 bytes of the octree centre lattice (device array); all zero while S is not active
avs_status refine_expand(const RefineState &S, const int oct[3], int8_t *flags, hipStream_t st);

} // namespace avs
