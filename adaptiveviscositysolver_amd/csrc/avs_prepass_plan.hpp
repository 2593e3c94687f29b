// avs_prepass_plan.hpp -- the integer geometry of a pre-pass run (avs_prepass.hip) on host values: the extents of the lattices, the level
// cap, the ranges a slab-local rank works on along the cut axis, and where every lattice's tiles lie in the numbering's count buffer.
// Plain C++ (no HIP header): compiled once for both libraries, run on the CPU by tests/test_prepass_plan_host.py through
// avs_prepass_plan_host (include/avs_probe.h).
#pragma once
#include <cstdint>

#include "avs.h"

namespace avs {

// extents of a lattice of level `level` on the octree grid n: kind 0 faces across `axis`, 1 edges along `axis`, 2 cells
void lattice_extents(const int n[3], int kind, int level, int axis, int r[3]);
// the levels a grid of n cells can carry (every axis keeps >= 2 cells at the top level), at most `desired`, at least 1; oct.cpp:32-40
int level_cap(const int n[3], int desired);
// the first level of L whose "has an ACTIVE cell" flag is not set (L: none), oct.cpp:198-211
int first_level_without_active(const int *flags, int L);

// Slab-local mode: what a rank touches of level l along the cut axis, in level-l cells [lo, hi).  Without slabs every range is the level.
struct SlabRanges {
    int win_lo[AVS_MAX_LEVELS] = {}, win_hi[AVS_MAX_LEVELS] = {}; // index window (multiples of the tile / the level's end): what the classification fills
    int nl_lo[AVS_MAX_LEVELS] = {}, nl_hi[AVS_MAX_LEVELS] = {};   // labels the classification of the window reads
    int v_lo[AVS_MAX_LEVELS] = {}, v_hi[AVS_MAX_LEVELS] = {};     // labels valid before the level serves as children (mask at level 0, passes 2 / 3 and top above)
    int p1_lo[AVS_MAX_LEVELS] = {}, p1_hi[AVS_MAX_LEVELS] = {};   // parents of pass 1 at level l >= 1
};
// na: cells of level 0 along the cut axis; cuts[rank], cuts[rank + 1]: the rank's slab in level-0 cells (read only when `on`);
// margin: level-l cells classified around the slab (kSlabIndexMargin), tile: entries per tile edge
SlabRanges slab_ranges(int na, int L, bool on, const int *cuts, int rank, int margin, int tile);

// The numbering's tile space.  One batch per counter -- velocity faces, edges, centres (each over ALL levels, level-major, then axis:
// numbering order), regular-grid faces (cpp:1486-1509: one counter over the three axes, the level-0 face lattices again); the four
// count arrays lie behind each other in ONE buffer, each with tiles + 1 entries, + AVS_MAX_LEVELS level flags in slab mode (what the
// ranks sum).  Levels beyond the cap are the tail of their batch: the scans stop before them.
struct TileLayout {
    int64_t seg[5] = {};                      // first count of every batch in the buffer
    int level_tile0[4][AVS_MAX_LEVELS + 1] = {}; // first tile of every level inside a batch (counters 0 .. 2), [L]: the batch's tiles
    int tile0_of[4][AVS_MAX_LEVELS][3] = {};  // first tile of every lattice inside its batch
    int64_t n_exchange = 0;                   // entries of the buffer
    int64_t tiles(int counter) const { return seg[counter + 1] - seg[counter] - 1; }
};
// false: a batch or the buffer has too many tiles for int32 offsets
bool tile_layout(const int n[3], int L, int tile, TileLayout *out);

} // namespace avs
