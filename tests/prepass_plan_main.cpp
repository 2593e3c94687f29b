// The pre-pass plan (csrc/avs_prepass_plan.cpp) on the cases of tests/test_prepass_plan_host.py as a stand-alone program, so that it runs
// under the host sanitizers: every rank's ranges of every slab case, the tile layouts, the level caps.  Prints "ok".
#include <cstdio>

#include "avs_prepass_plan.cpp"

using namespace avs;

struct SlabCase { int extent, levels, world; int cuts[5]; };
static const SlabCase kSlab[] = {
    {16, 1, 2, {0, 8, 16}},       {16, 4, 2, {0, 8, 16}},         {64, 3, 2, {0, 32, 64}},        {64, 3, 2, {0, 20, 64}},
    {64, 3, 2, {0, 0, 64}},       {64, 3, 2, {0, 64, 64}},        {32, 3, 4, {0, 8, 16, 24, 32}}, {64, 4, 3, {0, 21, 43, 64}},
    {128, 5, 3, {0, 1, 127, 128}}, {64, 6, 2, {0, 13, 64}},       {256, 4, 3, {0, 100, 101, 256}},
};
struct LayoutCase { int n[3], levels; };
static const LayoutCase kLayout[] = {{{16, 16, 16}, 1}, {{16, 16, 16}, 4}, {{64, 32, 16}, 3}, {{32, 32, 32}, 3}};

static int fail(const char *what, int a, int b, int c)
{
    std::printf("%s: case %d rank %d level %d\n", what, a, b, c);
    return 1;
}

int main()
{
    for (int c = 0; c < (int)(sizeof(kSlab) / sizeof(kSlab[0])); ++c) {
        const SlabCase &S = kSlab[c];
        for (int on = 0; on < 2; ++on)
            for (int rank = 0; rank < (on ? S.world : 1); ++rank) {
                const SlabRanges R = slab_ranges(S.extent, S.levels, on != 0, S.cuts, rank, 12, 16);
                for (int l = 0; l < AVS_MAX_LEVELS; ++l) {
                    const int nl = l < S.levels ? S.extent >> l : 0;
                    const int *lo[4] = {R.win_lo, R.nl_lo, R.v_lo, R.p1_lo}, *hi[4] = {R.win_hi, R.nl_hi, R.v_hi, R.p1_hi};
                    for (int k = 0; k < 4; ++k)
                        if (!(0 <= lo[k][l] && lo[k][l] <= hi[k][l] && hi[k][l] <= nl)) return fail("range outside its level", c, rank, l);
                    if (!on && l < S.levels && !(R.win_lo[l] == 0 && R.win_hi[l] == nl && R.v_hi[l] == nl && R.p1_hi[l] == nl && R.nl_hi[l] == nl))
                        return fail("not the whole level", c, rank, l);
                }
            }
    }
    for (int c = 0; c < (int)(sizeof(kLayout) / sizeof(kLayout[0])); ++c) {
        const LayoutCase &C = kLayout[c];
        TileLayout T;
        if (!tile_layout(C.n, C.levels, 16, &T)) return fail("layout refused", c, 0, 0);
        for (int b = 0; b < 4; ++b)
            if (T.tiles(b) <= 0 || (b < 3 && T.level_tile0[b][C.levels] != T.tiles(b))) return fail("batch total", c, b, 0);
        if (T.n_exchange != T.seg[4] + AVS_MAX_LEVELS || T.tiles(3) != T.level_tile0[0][1]) return fail("buffer size", c, 0, 0);
    }
    const int n16[3] = {16, 16, 16}, n64[3] = {64, 32, 16}, huge[3] = {1 << 20, 1 << 20, 1 << 20};
    if (level_cap(n16, 6) != 4 || level_cap(n64, 6) != 4 || level_cap(n16, 1) != 1) return fail("level cap", 0, 0, 0);
    TileLayout T;
    if (tile_layout(huge, 8, 16, &T)) return fail("2^48 tiles accepted", 0, 0, 0);
    const int flags[4] = {1, 1, 0, 1};
    if (first_level_without_active(flags, 4) != 2 || first_level_without_active(flags, 2) != 2 || first_level_without_active(flags, 0) != 0)
        return fail("first level without an ACTIVE cell", 0, 0, 0);
    std::printf("ok\n");
    return 0;
}
