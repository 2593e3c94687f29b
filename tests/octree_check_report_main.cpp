// Stand-alone driver of the host side of avs_check_octree that needs no HIP call (csrc/avs_check_report.hpp: argument checks, the packed key
// of the first violation, report packing, the struct_size hand-over) and of what csrc/avs_report.hpp holds for every report header
// (report_size_ok, report_hand_over, lattice_key, lattice_entry_ijk: the direct cases at the end).  tests/test_octree_check_host.py builds it with the host sanitizers
// (-fsanitize=address,undefined) and runs it; it prints "ok" and exits 0, or says which expectation failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "avs_check_report.hpp"

#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

using namespace avs;

int main()
{
    const char *why = nullptr;
    avs_octree_check rep;
    std::memset(&rep, 0, sizeof(rep));
    rep.struct_size = (int32_t)sizeof(rep);
    // argument checks
    EXPECT(check_octree_args(3u, nullptr, &why) == AVS_EINVAL && why);
    EXPECT(check_octree_args(0u, &rep, &why) == AVS_OK);
    EXPECT(check_octree_args(AVS_CHECK_LABELS | AVS_CHECK_VELOCITY_INDICES, &rep, &why) == AVS_OK);
    for (uint32_t what : {4u, 7u, 0x100u, 0x80000001u, 0xffffffffu}) EXPECT(check_octree_args(what, &rep, &why) == AVS_EINVAL);
    for (int32_t size : {0, 4, 7, -8, 4097, INT32_MIN, INT32_MAX}) {
        rep.struct_size = size;
        EXPECT(check_octree_args(1u, &rep, &why) == AVS_EINVAL);
    }
    for (int32_t size : {8, 24, 96, 4096}) {
        rep.struct_size = size;
        EXPECT(check_octree_args(1u, &rep, &why) == AVS_OK);
    }
    // keys order by (rule, level, axis, linear index), and the largest fields do not run into each other
    EXPECT(lattice_key(0, 7, 2, (1ull << kLatticeLinBits) - 1) < lattice_key(1, 0, 0, 0));
    EXPECT(lattice_key(3, 1, 2, (1ull << kLatticeLinBits) - 1) < lattice_key(3, 2, 0, 0));
    EXPECT(lattice_key(5, 2, 0, (1ull << kLatticeLinBits) - 1) < lattice_key(5, 2, 1, 0));
    EXPECT(lattice_key(7, 7, 2, (1ull << kLatticeLinBits) - 1) < kNoKey);
    // a clean raw report
    const int n[3] = {1024, 512, 256};
    unsigned long long raw[kCheckRawWords] = {};
    raw[AVS_OCTREE_RULES] = kNoKey;
    avs_octree_check r = check_octree_report(raw, 3u, n);
    EXPECT(r.passed == 1 && r.first_rule == -1 && r.first_level == -1 && r.first_axis == -1 && r.first_ijk[2] == -1 && r.struct_size == 96);
    // a face of level 2, axis 1 (lattice 256 x 129 x 64): the last entry
    const unsigned long long lin = 256ull * 129ull * 64ull - 1ull;
    raw[AVS_RULE_FACE] = 5000000000ull; // counts are 64-bit
    raw[AVS_RULE_UP] = 3;
    raw[AVS_OCTREE_RULES] = lattice_key(AVS_RULE_FACE, 2, 1, lin);
    r = check_octree_report(raw, 2u, n); // labels not asked for: their counts are dropped
    EXPECT(r.passed == 0 && r.violations[AVS_RULE_UP] == 0 && r.violations[AVS_RULE_FACE] == 5000000000ll);
    EXPECT(r.first_rule == AVS_RULE_FACE && r.first_level == 2 && r.first_axis == 1 && r.first_ijk[0] == 255 && r.first_ijk[1] == 128 && r.first_ijk[2] == 63);
    r = check_octree_report(raw, 1u, n); // only the label rules asked for
    EXPECT(r.violations[AVS_RULE_UP] == 3 && r.violations[AVS_RULE_FACE] == 0 && r.passed == 0);
    // a label of level 7 on a lattice that is one cell wide there; rule 7 reports the id
    const int tiny[3] = {128, 128, 256};
    std::memset(raw, 0, sizeof(raw));
    raw[AVS_RULE_LABEL_VALUE] = 1;
    raw[AVS_OCTREE_RULES] = lattice_key(AVS_RULE_LABEL_VALUE, 7, 0, 1);
    r = check_octree_report(raw, 1u, tiny);
    EXPECT(r.first_level == 7 && r.first_ijk[0] == 0 && r.first_ijk[1] == 0 && r.first_ijk[2] == 1);
    std::memset(raw, 0, sizeof(raw));
    raw[AVS_RULE_NUMBERING] = 2;
    raw[AVS_OCTREE_RULES] = lattice_key(AVS_RULE_NUMBERING, 0, 0, 2147483646ull);
    r = check_octree_report(raw, 2u, tiny);
    EXPECT(r.first_rule == AVS_RULE_NUMBERING && r.first_ijk[0] == 2147483646 && r.first_ijk[1] == 0 && r.first_ijk[2] == 0);
    // the hand-over writes struct_size bytes and not one more: the caller's struct sits at the very end of a heap block
    for (int32_t size : {8, 12, 24, 72, 80, 96}) {
        std::vector<unsigned char> block((size_t)size, 0x5a);
        avs_octree_check *out = reinterpret_cast<avs_octree_check *>(block.data());
        std::memcpy(&out->struct_size, &size, sizeof(size));
        report_hand_over(r, out);
        int32_t back, passed;
        std::memcpy(&back, block.data(), 4);
        std::memcpy(&passed, block.data() + 4, 4);
        EXPECT(back == size && passed == 0);
        if (size >= 24) {
            int64_t v0;
            std::memcpy(&v0, block.data() + 8, 8);
            EXPECT(v0 == 0);
        }
    }
    { // a caller built against a larger, future struct: the bytes behind today's struct stay
        std::vector<unsigned char> block(200, 0x5a);
        const int32_t size = 200;
        std::memcpy(block.data(), &size, sizeof(size));
        report_hand_over(r, reinterpret_cast<avs_octree_check *>(block.data()));
        for (size_t b = sizeof(avs_octree_check); b < block.size(); ++b) EXPECT(block[b] == 0x5a);
    }
    // avs_report.hpp directly.  Admission and hand-over at the edges of struct_size: one below the first member a call writes, at it, at
    // sizeof and above sizeof; the hand-over writes min(struct_size, sizeof) bytes and struct_size stays the caller's
    {
        const int32_t least = (int32_t)(offsetof(avs_octree_check, passed) + sizeof(int32_t)), full = (int32_t)sizeof(avs_octree_check);
        avs_octree_check src = check_octree_passed();
        src.passed = 0;
        src.first_ijk[2] = 77; // the last member
        for (int32_t size : {least - 1, least, full, full + 1, 4096, 4097}) {
            std::vector<unsigned char> block((size_t)size, 0x5a);
            avs_octree_check *out = reinterpret_cast<avs_octree_check *>(block.data());
            std::memcpy(block.data(), &size, sizeof(size));
            EXPECT(report_size_ok(out, (size_t)least) == (size >= least && size <= 4096));
            report_hand_over(src, out);
            int32_t back;
            std::memcpy(&back, block.data(), 4);
            EXPECT(back == size);
            const size_t written = (size_t)(size < full ? size : full);
            EXPECT(std::memcmp(block.data() + 4, reinterpret_cast<const unsigned char *>(&src) + 4, written - 4) == 0);
            for (size_t b = written; b < block.size(); ++b) EXPECT(block[b] == 0x5a);
        }
    }
    // lattice_key: every field comes back at its extremes, alone and together
    {
        const unsigned long long lin_max = (1ull << kLatticeLinBits) - 1;
        for (int rule : {0, 15})
            for (int level : {0, 7})
                for (int axis : {0, 2})
                    for (unsigned long long lin : {0ull, lin_max}) {
                        const unsigned long long key = lattice_key(rule, level, axis, lin);
                        EXPECT(lattice_key_rule(key) == rule && lattice_key_level(key) == level && lattice_key_axis(key) == axis && lattice_key_lin(key) == lin);
                        EXPECT(key < kNoKey);
                    }
        EXPECT(lattice_key(15, 7, 2, lin_max) == (15ull << 45 | 7ull << 42 | 2ull << 40 | lin_max));
    }
    // lattice_entry_ijk on a 2 x 4 x 8 grid at level 1 (cells 1 x 2 x 4): the face lattice of axis 1 is 1 x 3 x 4, the edge lattice of
    // axis 1 is 2 x 2 x 5; every entry, x fastest
    {
        const int grid[3] = {2, 4, 8};
        for (int kind = 0; kind < 2; ++kind) {
            const unsigned mask = kind == 0 ? 1u << 1 : 7u & ~(1u << 1);
            const int e[3] = {kind == 0 ? 1 : 2, kind == 0 ? 3 : 2, kind == 0 ? 4 : 5};
            unsigned long long at = 0;
            for (int k = 0; k < e[2]; ++k)
                for (int j = 0; j < e[1]; ++j)
                    for (int i = 0; i < e[0]; ++i, ++at) {
                        int32_t ijk[3] = {-1, -1, -1};
                        lattice_entry_ijk(at, grid, 1, mask, ijk);
                        EXPECT(ijk[0] == i && ijk[1] == j && ijk[2] == k);
                    }
            EXPECT(at == (kind == 0 ? 12ull : 20ull));
        }
        int32_t ijk[3];
        lattice_entry_ijk(5, grid, 1, 0u, ijk); // the cell lattice itself, 1 x 2 x 4
        EXPECT(ijk[0] == 0 && ijk[1] == 1 && ijk[2] == 2);
    }
    std::puts("ok");
    return 0;
}
