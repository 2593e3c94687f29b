// avs_prepass_plan.cpp -- the integer geometry of a pre-pass run (no device code; see avs_prepass_plan.hpp).  avs_prepass_run
// (avs_prepass.hip) plans with it before it enqueues anything; tests/test_prepass_plan_host.py runs it without a GPU.
#include "avs_prepass_plan.hpp"

namespace avs {

void lattice_extents(const int n[3], int kind, int level, int axis, int r[3])
{
    for (int a = 0; a < 3; ++a) r[a] = n[a] >> level;
    if (kind == 0) r[axis] += 1;
    else if (kind == 1)
        for (int a = 0; a < 3; ++a) r[a] += (axis != a);
}

int level_cap(const int n[3], int desired)
{
    int L = desired;
    for (int a = 0; a < 3; ++a) {
        int lg = 0;
        while ((1 << (lg + 1)) <= n[a]) ++lg;
        if (lg < L) L = lg;
    }
    return L < 1 ? 1 : L;
}

int first_level_without_active(const int *flags, int L)
{
    int l = 0;
    while (l < L && flags[l]) ++l;
    return l;
}

SlabRanges slab_ranges(int na, int L, bool on, const int *cuts, int rank, int margin, int tile)
{
    SlabRanges R;
    for (int l = 0; l < L; ++l) {
        const int nl = na >> l;
        if (!on) {
            R.win_hi[l] = R.nl_hi[l] = R.v_hi[l] = R.p1_hi[l] = nl;
            continue;
        }
        const int s_lo = cuts[rank] >> l, s_hi = (cuts[rank + 1] + (1 << l) - 1) >> l;
        int lo = s_lo - margin, hi = s_hi + margin;
        lo = lo < 0 ? 0 : lo / tile * tile;
        hi = (hi + tile - 1) / tile * tile;
        if (hi > nl) hi = nl;
        R.win_lo[l] = lo;
        R.win_hi[l] = hi;
        R.nl_lo[l] = lo - 2 < 0 ? 0 : lo - 2;
        R.nl_hi[l] = hi + 2 > nl ? nl : hi + 2;
    }
    if (!on) return R;
    R.v_lo[L - 1] = R.nl_lo[L - 1];
    R.v_hi[L - 1] = R.nl_hi[L - 1];
    for (int l = L - 2; l >= 0; --l) { // pass 2 of a parent reads the face neighbours of its children AFTER their own parents' pass 1
        const int np = na >> (l + 1);
        int a = R.v_lo[l + 1] - 1, b = R.v_hi[l + 1] + 1;
        if (R.nl_lo[l] / 2 < a) a = R.nl_lo[l] / 2;
        if ((R.nl_hi[l] + 1) / 2 > b) b = (R.nl_hi[l] + 1) / 2;
        R.p1_lo[l + 1] = a < 0 ? 0 : a;
        R.p1_hi[l + 1] = b > np ? np : b;
        R.v_lo[l] = 2 * R.p1_lo[l + 1];
        R.v_hi[l] = 2 * R.p1_hi[l + 1];
    }
    // (the mask kernel is pointwise: its box may be any superset -- whole groups of four cells keep it on its vector path along x)
    R.v_lo[0] = R.v_lo[0] / 4 * 4;
    R.v_hi[0] = (R.v_hi[0] + 3) / 4 * 4 > na ? na : (R.v_hi[0] + 3) / 4 * 4;
    return R;
}

bool tile_layout(const int n[3], int L, int tile, TileLayout *out)
{
    TileLayout T;
    const int64_t limit = (1ll << 31) - 1;
    for (int counter = 0; counter < 4; ++counter) {
        int64_t tiles = 0;
        auto add = [&](int kind, int l, int a) {
            int gr[3];
            lattice_extents(n, kind, l, a, gr);
            T.tile0_of[counter][l][a] = (int)tiles;
            tiles += (int64_t)((gr[0] + tile - 1) / tile) * ((gr[1] + tile - 1) / tile) * ((gr[2] + tile - 1) / tile);
        };
        if (counter < 3) {
            for (int l = 0; l < L; ++l) {
                T.level_tile0[counter][l] = (int)tiles;
                for (int a = 0; a < (counter == 2 ? 1 : 3); ++a) add(counter, l, a);
            }
            T.level_tile0[counter][L] = (int)tiles;
        } else
            for (int a = 0; a < 3; ++a) add(0, 0, a);
        if (tiles >= limit) return false;
        T.seg[counter + 1] = T.seg[counter] + tiles + 1;
    }
    T.n_exchange = T.seg[4] + AVS_MAX_LEVELS;
    if (T.n_exchange >= limit) return false;
    *out = T;
    return true;
}

} // namespace avs
