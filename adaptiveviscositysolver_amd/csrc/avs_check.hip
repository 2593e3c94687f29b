// avs_check.hip -- the reference's debug invariants on the label pyramid and the velocity index pyramid, on the device
// (reference: HDK_OctreeGrid::unitTest, oct.cpp:984-1304, called at cpp:881; octreeVelocityUnitTest, cpp:2896-2999, called at cpp:411).
// The eight rules are stated in include/avs.h (avs_check_octree); tests/octree_check_model.py restates them in NumPy.
//
//   k_check_labels     one launch per level: a thread owns a run of four x-adjacent cells, read as one word (rows shorter than four, or a
//                      lattice that does not start on a word: bytewise; level 0 with rows of whole 16-byte pieces: four runs per thread).  A run that holds an UP or ACTIVE cell also reads the runs next
//                      to it along y and z and the two cells next to it along x: rules 0, 2 and 3 from one read of the level.  Level 0
//                      evaluates rule 1 on the same word: the ancestors of the four cells are one cell per level (two at level 1).
//                      In the piece form sixteen equal INACTIVE or UP labels under uniform ancestors are judged once
//                      (check_piece_passes): cell by cell the pass is bound by instructions (profiles/octree_check.md).
//   k_check_index      one launch per level and axis: a thread owns four consecutive entries of the face lattice (one 16-byte load in
//                      LINEAR order: rows of n + 1 entries never line up with anything, the lattice as a whole does; the last entries
//                      one by one).  Rules 4 and 6 need the entry alone, rule 5 the two cells the face lies between (and the parent of
//                      an UP one) -- only for the faces that carry an id --, and every id in range counts itself in occ[id].
//   k_index_numbering  rule 7 over the occurrence counters (shared with the stress index check, defined here).
//
// Every rule is independent: no label and no index is used as an address.  The only address formed from a lattice value is occ[id], and
// that store is under the range test of rule 4.  Cells outside their lattice are never read (they count as INACTIVE).
// The reciprocity loop of activeUnitTest (oct.cpp:1250-1269) needs no kernel: with rules 1 and 3 holding it cannot fail -- the cell
// reached from the other side of a face is the same ACTIVE cell, its DOWN parent, or its UP child (tests/test_octree_check_model.py
// asserts it on its scenes).
// Counts are 64-bit: a thread counts in registers, a wave adds its lanes and issues one atomic per rule it violated; the first violation
// is one atomicMin of a packed key (lattice_key, avs_report.hpp) per violating wave (raw_commit, avs_report_device.hpp).  Integer work
// only: the same lattices give the same report.
#include "avs_internal.hpp"
#include "avs_report_device.hpp"

namespace avs {

struct CheckLevels { // by value; the level of a launch is a kernel argument: every table lookup is wave-uniform
    const int8_t *lab[AVS_MAX_LEVELS];
    int n[3];      // level-0 cells per axis
    int levels;
    int word_mask; // bit l: the rows of level l are read as whole words
};

// label of cell (i, j, k) of level l; outside the lattice: INACTIVE
__device__ __forceinline__ int check_label(const CheckLevels &P, int l, int i, int j, int k)
{
    const int n0 = P.n[0] >> l, n1 = P.n[1] >> l, n2 = P.n[2] >> l;
    if ((unsigned)i >= (unsigned)n0 || (unsigned)j >= (unsigned)n1 || (unsigned)k >= (unsigned)n2) return AVS_INACTIVE;
    return P.lab[l][(size_t)i + (size_t)n0 * ((size_t)j + (size_t)n1 * (size_t)k)];
}
// labels i0 .. i0 + 3 of row (j, k), byte b = cell i0 + b; cells outside the lattice: INACTIVE
__device__ __forceinline__ uint32_t check_run(const int8_t *lab, int n0, int n1, int n2, bool words, int i0, int j, int k)
{
    if ((unsigned)j >= (unsigned)n1 || (unsigned)k >= (unsigned)n2 || i0 >= n0) return 0u;
    const int8_t *row = lab + ((size_t)n0 * ((size_t)j + (size_t)n1 * (size_t)k) + (size_t)i0);
    if (words) return *reinterpret_cast<const uint32_t *>(row);
    uint32_t w = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (i0 + b < n0) w |= (uint32_t)(uint8_t)row[b] << (8 * b);
    return w;
}
__device__ __forceinline__ int check_byte(uint32_t w, int b) { return (int)(int8_t)(w >> (8 * b)); }

// rule 3 for ACTIVE cell C of `level` and its in-lattice neighbour (ni, nj, nk) = C + s along axis d, whose label is nb
__device__ __forceinline__ bool check_active_face(const CheckLevels &P, int level, int d, int s, int ni, int nj, int nk, int nb)
{
    if (nb == AVS_DOWN) {
        if (level == 0) return true;
        int c[3] = {2 * ni, 2 * nj, 2 * nk};
        c[d] += s > 0 ? 0 : 1; // the children's plane that faces C
        const int o0 = d == 0 ? 1 : 0, o1 = d == 2 ? 1 : 2;
        bool bad = false;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int e[3] = {c[0], c[1], c[2]};
            e[o0] += q & 1;
            e[o1] += q >> 1;
            bad |= check_label(P, level - 1, e[0], e[1], e[2]) != AVS_ACTIVE;
        }
        return bad;
    }
    if (nb == AVS_UP) return level == P.levels - 1 || check_label(P, level + 1, ni >> 1, nj >> 1, nk >> 1) != AVS_ACTIVE;
    return false;
}

// Rules 0 .. 3 for the run of four cells i0 .. i0 + 3 of row (j, k) of `level`, whose labels are the bytes of c.  Level 0 also evaluates rule 1:
// a0[l] / a1[l] are the level-l ancestors of cells 0, 1 / 2, 3 of the run (l = 1 .. L-1; not read at other levels).
__device__ __forceinline__ void check_label_run(const CheckLevels &P, int level, const int8_t *lab, int n0, int n1, int n2, bool words, int i0, int j, int k,
                                                uint32_t c, const int (&a0)[AVS_MAX_LEVELS], const int (&a1)[AVS_MAX_LEVELS], unsigned (&cnt)[4],
                                                unsigned long long &key)
{
    const int L = P.levels;
    const int nv = min(4, n0 - i0);
    const unsigned long long lin0 = (unsigned long long)i0 + (unsigned long long)n0 * ((unsigned long long)j + (unsigned long long)n1 * (unsigned long long)k);
    bool any_up = false, any_act = false;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int v = check_byte(c, b);
        if (b < nv && (unsigned)v > 3u) { // rule 0
            ++cnt[0];
            key = min(key, lattice_key(AVS_RULE_LABEL_VALUE, level, 0, lin0 + b));
        }
        any_up |= b < nv && v == AVS_UP;
        any_act |= b < nv && v == AVS_ACTIVE;
    }
    if (level == 0) { // rule 1: the columns over these four cells
        unsigned bad = 0u, found = 0u; // bit b: cell b.  found: INACTIVE columns have met a DOWN, UP columns their ACTIVE
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int v = check_byte(c, b);
            if (v != AVS_INACTIVE && v != AVS_ACTIVE && v != AVS_UP) bad |= 1u << b;
        }
#pragma unroll
        for (int l = 1; l < AVS_MAX_LEVELS; ++l) {
            if (l >= L) continue;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int v = check_byte(c, b), a = b < 2 ? a0[l] : a1[l];
                const bool f = (found >> b) & 1u;
                bool x = false, nf = f;
                if (v == AVS_INACTIVE) {
                    x = !(a == AVS_DOWN || (a == AVS_INACTIVE && !f));
                    nf = f || a == AVS_DOWN;
                } else if (v == AVS_ACTIVE) {
                    x = a != AVS_DOWN;
                } else if (v == AVS_UP) {
                    x = a == AVS_ACTIVE ? f : (a == AVS_UP ? f : (a == AVS_DOWN ? !f : true));
                    nf = f || a == AVS_ACTIVE;
                }
                bad |= (x ? 1u : 0u) << b;
                found = (found & ~(1u << b)) | (nf ? 1u : 0u) << b;
            }
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (check_byte(c, b) == AVS_UP && !((found >> b) & 1u)) bad |= 1u << b;
            if (b < nv && ((bad >> b) & 1u)) {
                ++cnt[1];
                key = min(key, lattice_key(AVS_RULE_COLUMN, 0, 0, lin0 + b));
            }
        }
    }
    if (!any_up && !any_act) return;
    // the runs next to this one (outside the lattice: INACTIVE, and the in-lattice tests below keep them out of rules 2 and 3)
    const uint32_t ym = check_run(lab, n0, n1, n2, words, i0, j - 1, k), yp = check_run(lab, n0, n1, n2, words, i0, j + 1, k);
    const uint32_t zm = check_run(lab, n0, n1, n2, words, i0, j, k - 1), zp = check_run(lab, n0, n1, n2, words, i0, j, k + 1);
    const int xm = check_label(P, level, i0 - 1, j, k), xp = check_label(P, level, i0 + 4, j, k);
    // sibling block of an UP cell: the x-pair of this run, of the run at j ^ 1, at k ^ 1, and of the diagonal one
    const uint32_t ys = (j & 1) ? ym : yp, zs = (k & 1) ? zm : zp;
    const uint32_t dg = any_up ? check_run(lab, n0, n1, n2, words, i0, j ^ 1, k ^ 1) : 0u;
    const uint32_t up2 = 0x0202u; // two UP labels
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        if (b >= nv) continue;
        const int v = check_byte(c, b), i = i0 + b;
        if (v != AVS_UP && v != AVS_ACTIVE) continue;
        const int nbv[6] = {b > 0 ? check_byte(c, b - 1) : xm, b < 3 ? check_byte(c, b + 1) : xp, check_byte(ym, b), check_byte(yp, b),
                            check_byte(zm, b), check_byte(zp, b)};
        const bool in[6] = {i > 0, i + 1 < n0, j > 0, j + 1 < n1, k > 0, k + 1 < n2};
        bool bad = false;
        if (v == AVS_UP) { // rule 2
            const int sh = 16 * (b >> 1);
            bad = level == L - 1 || ((c >> sh) & 0xffffu) != up2 || ((ys >> sh) & 0xffffu) != up2 || ((zs >> sh) & 0xffffu) != up2 ||
                  ((dg >> sh) & 0xffffu) != up2;
#pragma unroll
            for (int f = 0; f < 6; ++f) bad |= in[f] && nbv[f] != AVS_ACTIVE && nbv[f] != AVS_UP;
            if (bad) {
                ++cnt[2];
                key = min(key, lattice_key(AVS_RULE_UP, level, 0, lin0 + b));
            }
        } else { // rule 3
#pragma unroll
            for (int f = 0; f < 6; ++f) {
                const int d = f >> 1, s = (f & 1) ? 1 : -1;
                if (in[f] && (nbv[f] == AVS_DOWN || nbv[f] == AVS_UP))
                    bad |= check_active_face(P, level, d, s, i + (d == 0 ? s : 0), j + (d == 1 ? s : 0), k + (d == 2 ? s : 0), nbv[f]);
            }
            if (bad) {
                ++cnt[3];
                key = min(key, lattice_key(AVS_RULE_ACTIVE, level, 0, lin0 + b));
            }
        }
    }
}

__device__ __forceinline__ bool check_splat(uint32_t w) { return w == (w & 0xffu) * 0x01010101u; }              // four equal bytes
__device__ __forceinline__ bool check_active_or_up(uint32_t w) { return ((w ^ (w >> 1)) & 0x01010101u) == 0x01010101u && (w & 0xfcfcfcfcu) == 0u; } // every byte is 1 or 2
// the sixteen labels ip .. ip + 15 of row (j, k) of level 0 in the piece form; *inside: the row exists
__device__ __forceinline__ uint4 check_piece(const int8_t *lab, int n0, int n1, int n2, int ip, int j, int k, bool *inside)
{
    *inside = (unsigned)j < (unsigned)n1 && (unsigned)k < (unsigned)n2;
    if (!*inside) return make_uint4(0u, 0u, 0u, 0u);
    return *reinterpret_cast<const uint4 *>(lab + ((size_t)n0 * ((size_t)j + (size_t)n1 * (size_t)k) + (size_t)ip));
}
// true: none of the sixteen level-0 cells of the piece violates rule 0, 1, 2 or 3 (false: not decided here)
__device__ __forceinline__ bool check_piece_passes(const CheckLevels &P, const int8_t *lab, int n0, int n1, int n2, int ip, int j, int k, const uint4 &cw,
                                                   uint32_t w1a, uint32_t w1b, uint32_t w2, int b3a, int b3b, const int (&hi)[AVS_MAX_LEVELS])
{
    const int L = P.levels;
    const uint32_t c0 = cw.x;
    if (!(cw.y == c0 && cw.z == c0 && cw.w == c0 && check_splat(c0))) return false;
    const int v = check_byte(c0, 0);
    if (v != AVS_INACTIVE && v != AVS_UP) return false;
    if (!(w1a == w1b && check_splat(w1a) && check_splat(w2) && b3a == b3b)) return false; // (levels that do not exist were left 0)
    // rule 1, once: the state machine of check_label_run on the one column all sixteen cells share
    bool found = false;
#pragma unroll
    for (int l = 1; l < AVS_MAX_LEVELS; ++l) {
        if (l >= L) continue;
        const int a = l == 1 ? check_byte(w1a, 0) : (l == 2 ? check_byte(w2, 0) : (l == 3 ? b3a : hi[l]));
        if (v == AVS_INACTIVE) {
            if (!(a == AVS_DOWN || (a == AVS_INACTIVE && !found))) return false;
            found = found || a == AVS_DOWN;
        } else {
            if (a == AVS_ACTIVE ? found : (a == AVS_UP ? found : (a == AVS_DOWN ? !found : true))) return false;
            found = found || a == AVS_ACTIVE;
        }
    }
    if (v == AVS_INACTIVE) return true; // rules 2 and 3 are about UP and ACTIVE cells
    if (!found) return false;           // (an ACTIVE ancestor: there is a level above, 0 < L - 1)
    // rule 2: the sibling rows are UP over the piece, the two other rows next to it and the cells at its ends ACTIVE or UP (or outside)
    const uint32_t up4 = 0x01010101u * (uint32_t)AVS_UP;
    bool in;
    const int js = j ^ 1, ks = k ^ 1, jo = (j & 1) ? j + 1 : j - 1, ko = (k & 1) ? k + 1 : k - 1;
    const uint4 sy = check_piece(lab, n0, n1, n2, ip, js, k, &in);
    bool ok = in && sy.x == up4 && sy.y == up4 && sy.z == up4 && sy.w == up4;
    const uint4 sz = check_piece(lab, n0, n1, n2, ip, j, ks, &in);
    ok = ok && in && sz.x == up4 && sz.y == up4 && sz.z == up4 && sz.w == up4;
    const uint4 sd = check_piece(lab, n0, n1, n2, ip, js, ks, &in);
    ok = ok && in && sd.x == up4 && sd.y == up4 && sd.z == up4 && sd.w == up4;
    const uint4 oy = check_piece(lab, n0, n1, n2, ip, jo, k, &in);
    ok = ok && (!in || (check_active_or_up(oy.x) && check_active_or_up(oy.y) && check_active_or_up(oy.z) && check_active_or_up(oy.w)));
    const uint4 oz = check_piece(lab, n0, n1, n2, ip, j, ko, &in);
    ok = ok && (!in || (check_active_or_up(oz.x) && check_active_or_up(oz.y) && check_active_or_up(oz.z) && check_active_or_up(oz.w)));
    if (ip > 0) {
        const int xm = check_label(P, 0, ip - 1, j, k);
        ok = ok && (xm == AVS_ACTIVE || xm == AVS_UP);
    }
    if (ip + 16 < n0) {
        const int xp = check_label(P, 0, ip + 16, j, k);
        ok = ok && (xp == AVS_ACTIVE || xp == AVS_UP);
    }
    return ok;
}

// pieces16: level 0 with rows that are whole 16-byte pieces -- a thread owns sixteen x-adjacent cells (four runs) and requests their labels
// and all their ancestors (eight cells of level 1, four of level 2, two of level 3, one of every level above) before it looks at any:
// seven loads in flight per sixteen cells.  (A run per thread, its ancestors fetched after its word, left the level-0 pass waiting on
// two dependent rounds of loads for every four bytes.)
template <bool pieces16>
__global__ __launch_bounds__(kBlock) void k_check_labels(CheckLevels P, int level_arg, unsigned long long *__restrict__ raw)
{
    const int level = pieces16 ? 0 : level_arg; // (the piece form is level 0's: the compiler drops what only other levels need)
    const int L = P.levels;
    const int n0 = P.n[0] >> level, n1 = P.n[1] >> level, n2 = P.n[2] >> level;
    const int8_t *lab = P.lab[level];
    const bool words = (P.word_mask >> level) & 1;
    unsigned cnt[4] = {0u, 0u, 0u, 0u};
    unsigned long long key = kNoKey;
    // extents are powers of two (avs_create, avs_prepass_create): a run's place in the lattice is shifts and masks, no 64-bit division
    const int sy = __ffs(n1) - 1;
    if (pieces16) {
        const int px = n0 >> 4, sx = __ffs(px) - 1;
        const long long pieces = (long long)px * n1 * n2;
        for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p < pieces; p += (long long)gridDim.x * kBlock) {
            const int ip = 16 * ((int)p & (px - 1)), j = (int)(p >> sx) & (n1 - 1), k = (int)(p >> (sx + sy));
            const uint4 cw = *reinterpret_cast<const uint4 *>(lab + ((size_t)n0 * ((size_t)j + (size_t)n1 * (size_t)k) + (size_t)ip));
            uint32_t w1a = 0u, w1b = 0u, w2 = 0u;
            int b3a = 0, b3b = 0, hi[AVS_MAX_LEVELS] = {};
            if (L > 1) {
                const int m0 = n0 >> 1, m1 = n1 >> 1, m2 = n2 >> 1;
                const bool w = (P.word_mask >> 1) & 1;
                w1a = check_run(P.lab[1], m0, m1, m2, w, ip >> 1, j >> 1, k >> 1);
                w1b = check_run(P.lab[1], m0, m1, m2, w, (ip >> 1) + 4, j >> 1, k >> 1);
            }
            if (L > 2) w2 = check_run(P.lab[2], n0 >> 2, n1 >> 2, n2 >> 2, (P.word_mask >> 2) & 1, ip >> 2, j >> 2, k >> 2);
            if (L > 3) {
                b3a = check_label(P, 3, ip >> 3, j >> 3, k >> 3);
                b3b = check_label(P, 3, (ip >> 3) + 1, j >> 3, k >> 3);
            }
#pragma unroll
            for (int l = 4; l < AVS_MAX_LEVELS; ++l)
                if (l < L) hi[l] = check_label(P, l, ip >> l, j >> l, k >> l);
            // Sixteen equal labels under ancestors that are the same for all sixteen -- the far field and the inside of coarse cells,
            // most of level 0 --: the column is judged once, and a piece of UP cells whose sibling rows are UP and whose other
            // neighbours are UP or ACTIVE breaks nothing.  Whatever does not pass this way takes the cell-by-cell path below, which
            // alone counts: the short cut never reports.  (Cell by cell the pass is bound by instructions, not by memory.)
            if (check_piece_passes(P, lab, n0, n1, n2, ip, j, k, cw, w1a, w1b, w2, b3a, b3b, hi)) continue;
            const uint32_t cs[4] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                int a0[AVS_MAX_LEVELS] = {}, a1[AVS_MAX_LEVELS] = {};
                const uint32_t w1 = u < 2 ? w1a : w1b;
                a0[1] = check_byte(w1, (2 * u) & 3), a1[1] = check_byte(w1, (2 * u + 1) & 3);
                a0[2] = a1[2] = check_byte(w2, u);
                a0[3] = a1[3] = u < 2 ? b3a : b3b;
#pragma unroll
                for (int l = 4; l < AVS_MAX_LEVELS; ++l) a0[l] = a1[l] = hi[l];
                check_label_run(P, level, lab, n0, n1, n2, words, ip + 4 * u, j, k, cs[u], a0, a1, cnt, key);
            }
        }
    } else {
        const int rx = (n0 + 3) >> 2, sx = __ffs(rx) - 1;
        const long long runs = (long long)rx * n1 * n2;
        for (long long r = (long long)blockIdx.x * kBlock + threadIdx.x; r < runs; r += (long long)gridDim.x * kBlock) {
            const int i0 = 4 * ((int)r & (rx - 1)), j = (int)(r >> sx) & (n1 - 1), k = (int)(r >> (sx + sy));
            const uint32_t c = check_run(lab, n0, n1, n2, words, i0, j, k);
            int a0[AVS_MAX_LEVELS] = {}, a1[AVS_MAX_LEVELS] = {};
            if (level == 0) {
#pragma unroll
                for (int l = 1; l < AVS_MAX_LEVELS; ++l) {
                    if (l >= L) continue;
                    a0[l] = check_label(P, l, i0 >> l, j >> l, k >> l);
                    a1[l] = l == 1 ? check_label(P, l, (i0 + 2) >> 1, j >> 1, k >> 1) : a0[l];
                }
            }
            check_label_run(P, level, lab, n0, n1, n2, words, i0, j, k, c, a0, a1, cnt, key);
        }
    }
    const int rules[4] = {AVS_RULE_LABEL_VALUE, AVS_RULE_COLUMN, AVS_RULE_UP, AVS_RULE_ACTIVE};
    raw_commit(cnt, rules, key, kCheckRawKey, raw);
}

// rules 4 .. 6 for entry `lin` = (i, j, k) of the face lattice of (level, axis) + the occurrence count of its id
__device__ __forceinline__ void check_face(const CheckLevels &P, int level, int axis, int v, int i, int j, int k, unsigned long long lin, int n_velocity,
                                           int32_t *__restrict__ occ, unsigned (&cnt)[3], unsigned long long &key)
{
    if (v < AVS_OUTSIDE || v >= n_velocity) { // rule 4
        ++cnt[0];
        key = min(key, lattice_key(AVS_RULE_INDEX_VALUE, level, axis, lin));
    }
    if (level > 0 && (v == AVS_OUTSIDE || v == AVS_SOLIDBOUNDARY)) { // rule 6
        ++cnt[2];
        key = min(key, lattice_key(AVS_RULE_SENTINEL, level, axis, lin));
    }
    if (v < 0) return;
    if (v < n_velocity) atomicAdd(occ + v, 1); // (in range: the only address a lattice value forms)
    // rule 5: the backward cell is one step down the axis, the forward cell has the face's own index
    const int bi = i - (axis == 0 ? 1 : 0), bj = j - (axis == 1 ? 1 : 0), bk = k - (axis == 2 ? 1 : 0);
    const int lb = check_label(P, level, bi, bj, bk), lf = check_label(P, level, i, j, k);
    bool ok = lb == AVS_ACTIVE && lf == AVS_ACTIVE;
    if (level < P.levels - 1) {
        if (lb == AVS_ACTIVE && lf == AVS_UP) ok = check_label(P, level + 1, i >> 1, j >> 1, k >> 1) == AVS_ACTIVE;
        if (lb == AVS_UP && lf == AVS_ACTIVE) ok = check_label(P, level + 1, bi >> 1, bj >> 1, bk >> 1) == AVS_ACTIVE;
    }
    if (!ok) {
        ++cnt[1];
        key = min(key, lattice_key(AVS_RULE_FACE, level, axis, lin));
    }
}

__global__ __launch_bounds__(kBlock) void k_check_index(CheckLevels P, int level, int axis, const int32_t *__restrict__ idx, int quads_ok,
                                                             int n_velocity, int32_t *__restrict__ occ, unsigned long long *__restrict__ raw)
{
    const int f0 = (P.n[0] >> level) + (axis == 0 ? 1 : 0), f1 = (P.n[1] >> level) + (axis == 1 ? 1 : 0), f2 = (P.n[2] >> level) + (axis == 2 ? 1 : 0);
    const long long total = (long long)f0 * f1 * f2, quads = (total + 3) >> 2;
    unsigned cnt[3] = {0u, 0u, 0u};
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
        // rules 4 and 6 need the entry alone; where no entry of the quad carries an id -- most of every lattice -- nothing is divided
        if (!(v[0] >= 0 || v[1] >= 0 || v[2] >= 0 || v[3] >= 0)) {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (b < nv) check_face(P, level, axis, v[b], 0, 0, 0, (unsigned long long)(e0 + b), n_velocity, occ, cnt, key);
            continue;
        }
        int i, j, k;
        if (total <= 0xffffffffll) { // 32-bit division where the lattice allows it
            const unsigned row = (unsigned)e0 / (unsigned)f0;
            i = (int)((unsigned)e0 - row * (unsigned)f0), j = (int)(row % (unsigned)f1), k = (int)(row / (unsigned)f1);
        } else {
            i = (int)(e0 % f0), j = (int)(e0 / f0 % f1), k = (int)(e0 / ((long long)f0 * f1));
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (b < nv) check_face(P, level, axis, v[b], i, j, k, (unsigned long long)(e0 + b), n_velocity, occ, cnt, key);
            if (++i == f0) { // the next entry starts a row
                i = 0;
                if (++j == f1) {
                    j = 0;
                    ++k;
                }
            }
        }
    }
    const int rules[3] = {AVS_RULE_INDEX_VALUE, AVS_RULE_FACE, AVS_RULE_SENTINEL};
    raw_commit(cnt, rules, key, kCheckRawKey, raw);
}

__global__ __launch_bounds__(kBlock) void k_index_numbering(const int32_t *__restrict__ occ, int n_ids, int rule, int key_word,
                                                            unsigned long long *__restrict__ raw)
{
    unsigned cnt = 0u;
    unsigned long long key = kNoKey;
    for (long long id = (long long)blockIdx.x * kBlock + threadIdx.x; id < n_ids; id += (long long)gridDim.x * kBlock)
        if (occ[id] != 1) {
            ++cnt;
            key = min(key, lattice_key(rule, 0, 0, (unsigned long long)id));
        }
    raw_add(cnt, rule, raw);
    raw_min(key, key_word, raw);
}

static bool check_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// Shared implementation of avs_check_octree / avs_prepass_check_octree (rules and protocol: include/avs.h).  The caller has run
// check_octree_args and the state checks of its object.
avs_status check_octree(CheckScratch &S, const CheckSource &src, hipStream_t st, uint32_t what, avs_octree_check *report)
{
    if (what == 0 || src.levels == 0) {
        report_hand_over(check_octree_passed(), report);
        return AVS_OK;
    }
    CheckLevels P{};
    P.levels = src.levels;
    bool empty = false; // a lattice extent of 0: nothing runs
    for (int a = 0; a < 3; ++a) {
        P.n[a] = src.n[a];
        empty = empty || (src.n[a] >> (src.levels - 1)) < 1;
    }
    AVS_REQUIRE(!empty, AVS_EINTERNAL, "octree check: %d levels on a %d x %d x %d lattice", src.levels, src.n[0], src.n[1], src.n[2]);
    AVS_REQUIRE(check_pow2(src.n[0]) && check_pow2(src.n[1]) && check_pow2(src.n[2]), AVS_EINTERNAL, "octree check: the lattice extents are no powers of two");
    for (int l = 0; l < src.levels; ++l) {
        AVS_REQUIRE(src.labels[l], AVS_EINTERNAL, "octree check: level %d has no label lattice", l);
        P.lab[l] = src.labels[l];
        // rows are whole words where the x extent is a multiple of four and the lattice starts on a word (hipMalloc'ed lattices do)
        if (((src.n[0] >> l) & 3) == 0 && (reinterpret_cast<uintptr_t>(src.labels[l]) & 3u) == 0) P.word_mask |= 1 << l;
    }
    const bool indices = (what & AVS_CHECK_VELOCITY_INDICES) != 0;
    AVS_REQUIRE(!indices || (src.n_velocity >= 0 && src.n_velocity < INT32_MAX), AVS_EINTERNAL, "octree check: velocity DOF count out of range");
    AVS_TRY(S.raw.begin(kCheckRawWords, kCheckRawKey, st));
    if (what & AVS_CHECK_LABELS)
        for (int l = 0; l < src.levels; ++l) {
            // level 0 in 16-byte pieces where its rows are whole pieces and the lattice starts on one
            const bool pieces16 = l == 0 && (src.n[0] & 15) == 0 && (reinterpret_cast<uintptr_t>(src.labels[0]) & 15u) == 0;
            const long long runs = (long long)(((src.n[0] >> l) + 3) >> 2) * (src.n[1] >> l) * (src.n[2] >> l);
            const unsigned grid = report_grid(report_workgroups(pieces16 ? runs >> 2 : runs), src.grid_cap);
            if (pieces16) hipLaunchKernelGGL(k_check_labels<true>, dim3(grid), dim3(kBlock), 0, st, P, l, S.raw.p);
            else hipLaunchKernelGGL(k_check_labels<false>, dim3(grid), dim3(kBlock), 0, st, P, l, S.raw.p);
        }
    if (indices) {
        const int nvel = (int)src.n_velocity;
        AVS_TRY(S.occ.reserve((size_t)nvel + 1));
        AVS_HIP(hipMemsetAsync(S.occ.p, 0, ((size_t)nvel + 1) * sizeof(int32_t), st));
        for (int l = 0; l < src.levels; ++l)
            for (int a = 0; a < 3; ++a) {
                AVS_REQUIRE(src.vidx[l][a], AVS_EINTERNAL, "octree check: level %d axis %d has no velocity index lattice", l, a);
                long long total = 1;
                for (int d = 0; d < 3; ++d) total *= (src.n[d] >> l) + (d == a ? 1 : 0);
                const int quads_ok = (reinterpret_cast<uintptr_t>(src.vidx[l][a]) & 15u) == 0 ? 1 : 0;
                hipLaunchKernelGGL(k_check_index, dim3(report_grid(report_workgroups((total + 3) >> 2), src.grid_cap)), dim3(kBlock), 0, st, P, l, a,
                                   src.vidx[l][a], quads_ok, nvel, S.occ.p, S.raw.p);
            }
        if (nvel > 0)
            hipLaunchKernelGGL(k_index_numbering, dim3(report_grid(report_workgroups(nvel), src.grid_cap)), dim3(kBlock), 0, st, (const int32_t *)S.occ.p, nvel,
                               (int)AVS_RULE_NUMBERING, kCheckRawKey, S.raw.p);
    }
    unsigned long long raw[kCheckRawWords];
    AVS_TRY(S.raw.read(raw, st)); // the one wait: the report is on the host
    report_hand_over(check_octree_report(raw, what, src.n), report);
    return AVS_OK;
}

} // namespace avs

using namespace avs;

extern "C" avs_status avs_check_octree(avs_ctx *c, uint32_t what, avs_octree_check *report)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c, AVS_EINVAL, "null argument");
    const char *why = nullptr;
    if (check_octree_args(what, report, &why) != AVS_OK) {
        set_error("%s", why);
        return AVS_EINVAL;
    }
    AVS_REQUIRE(!c->slab.on, AVS_ESTATE, "avs_check_octree: the context holds a slab-local pre-pass (this rank's window only)");
    CheckSource src{};
    if (what != 0)
        for (int l = 0; l < c->desc.levels; ++l) {
            AVS_REQUIRE(c->have_labels[l] && c->labels[l].p, AVS_ESTATE, "avs_check_octree: labels of level %d missing (avs_set_labels / avs_prepass_apply)", l);
            src.labels[l] = c->labels[l].p;
            if (!(what & AVS_CHECK_VELOCITY_INDICES)) continue;
            for (int a = 0; a < 3; ++a) {
                AVS_REQUIRE(c->have_vidx[l][a] && c->vidx[l][a].p, AVS_ESTATE,
                            "avs_check_octree: velocity indices of level %d axis %d missing (avs_set_index_field / avs_prepass_apply)", l, a);
                src.vidx[l][a] = c->vidx[l][a].p;
            }
        }
    if (what & AVS_CHECK_VELOCITY_INDICES) AVS_REQUIRE(c->n_vel >= 0, AVS_ESTATE, "avs_check_octree: DOF counts missing (avs_set_dof_counts / avs_prepass_apply)");
    src.levels = c->desc.levels;
    src.n[0] = c->desc.nx;
    src.n[1] = c->desc.ny;
    src.n[2] = c->desc.nz;
    src.n_velocity = c->n_vel;
    src.grid_cap = c->opt.cells_grid_cap;
    AVS_HIP(hipSetDevice(c->desc.device));
    Scope scope("Octree Unit Test"); // cpp:881, cpp:411
    return check_octree(c->check, src, c->stream, what, report);
}
