// Stand-alone driver of the host side of avs_check_stress_indices that needs no HIP call (csrc/avs_stress_check_report.hpp: argument checks,
// the packed key of the first violation, report unpacking on the lattices of the three kinds, the struct_size hand-over).
// tests/test_stress_check_host.py builds it with the host sanitizers (-fsanitize=address,undefined) and runs it; it prints "ok" and exits 0,
// or says which expectation failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "avs_stress_check_report.hpp"

#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

using namespace avs;

static bool first_is(const avs_stress_check &r, int rule, int level, int axis, int i, int j, int k)
{
    return r.passed == 0 && r.first_rule == rule && r.first_level == level && r.first_axis == axis && r.first_ijk[0] == i && r.first_ijk[1] == j &&
           r.first_ijk[2] == k;
}

int main()
{
    static_assert(sizeof(avs_stress_check) == 120, "layout of avs_stress_check");
    const int32_t full = (int32_t)sizeof(avs_stress_check), least = (int32_t)(offsetof(avs_stress_check, passed) + sizeof(int32_t));
    const char *why = nullptr;
    avs_stress_check rep;
    std::memset(&rep, 0, sizeof(rep));
    rep.struct_size = full;
    // argument checks
    EXPECT(check_stress_args(3u, nullptr, &why) == AVS_EINVAL && why);
    for (uint32_t what : {0u, 1u, 2u, 3u}) EXPECT(check_stress_args(what, &rep, &why) == AVS_OK);
    for (uint32_t what : {4u, 7u, 0x100u, 0x80000001u, 0xffffffffu}) {
        why = nullptr;
        EXPECT(check_stress_args(what, &rep, &why) == AVS_EINVAL && why);
    }
    for (int32_t size : {0, 4, least - 1, -8, 4097, INT32_MIN, INT32_MAX}) {
        rep.struct_size = size;
        why = nullptr;
        EXPECT(check_stress_args(1u, &rep, &why) == AVS_EINVAL && why && std::strstr(why, "struct_size"));
    }
    for (int32_t size : {least, 24, full - 8, full, 4096}) {
        rep.struct_size = size;
        EXPECT(check_stress_args(1u, &rep, &why) == AVS_OK);
    }
    // keys order by (rule, level, axis, linear index), the largest fields do not run into each other, and every field comes back
    const unsigned long long lin_max = (1ull << kLatticeLinBits) - 1;
    EXPECT(lattice_key(0, 7, 2, lin_max) < lattice_key(1, 0, 0, 0));
    EXPECT(lattice_key(3, 1, 2, lin_max) < lattice_key(3, 2, 0, 0));
    EXPECT(lattice_key(5, 2, 0, lin_max) < lattice_key(5, 2, 1, 0));
    EXPECT(lattice_key(7, 7, 2, lin_max) < lattice_key(8, 0, 0, 0));
    EXPECT(lattice_key(AVS_STRESS_RULES - 1, 7, 2, lin_max) < kNoKey);
    EXPECT(lattice_key(15, 7, 3, lin_max) < kNoKey); // (even a full four-bit rule field stays below "none")
    for (int rule : {0, 8})
        for (int level : {0, 7})
            for (int axis : {0, 2})
                for (unsigned long long lin : {0ull, lin_max}) {
                    const unsigned long long key = lattice_key(rule, level, axis, lin);
                    EXPECT((int)(key >> kLatticeRuleShift & 15u) == rule && (int)(key >> kLatticeLevelShift & 7u) == level &&
                           (int)(key >> kLatticeAxisShift & 3u) == axis && (key & lin_max) == lin);
                }
    // a clean raw report: the active counts come back for the kinds that were asked for
    const int n[3] = {1024, 512, 256};
    unsigned long long raw[kStressRawWords] = {};
    raw[kStressRawKey] = kNoKey;
    raw[kStressRawEdges] = 6000000000ull;
    raw[kStressRawCenters] = 77;
    avs_stress_check r = check_stress_report(raw, 3u, n);
    EXPECT(r.passed == 1 && r.first_rule == -1 && r.first_level == -1 && r.first_axis == -1 && r.first_ijk[0] == -1 && r.first_ijk[2] == -1 && r.struct_size == full);
    EXPECT(r.active_edges == 6000000000ll && r.active_centers == 77);
    r = check_stress_report(raw, 1u, n);
    EXPECT(r.passed == 1 && r.active_edges == 6000000000ll && r.active_centers == 0);
    r = check_stress_report(raw, 2u, n);
    EXPECT(r.passed == 1 && r.active_edges == 0 && r.active_centers == 77);
    // edge lattices of level 2 (cells 256 x 128 x 64): axis 0 is 256 x 129 x 65, axis 1 is 257 x 128 x 65, axis 2 is 257 x 129 x 64 -- the
    // last entry of each, and one in the middle
    raw[AVS_STRESS_RULE_EDGE_FACES] = 5000000000ull; // counts are 64-bit
    raw[AVS_STRESS_RULE_CENTER_LABEL] = 3;
    raw[kStressRawKey] = lattice_key(AVS_STRESS_RULE_EDGE_FACES, 2, 0, 256ull * 129ull * 65ull - 1ull);
    r = check_stress_report(raw, 1u, n); // centres not asked for: their counts are dropped
    EXPECT(r.violations[AVS_STRESS_RULE_CENTER_LABEL] == 0 && r.violations[AVS_STRESS_RULE_EDGE_FACES] == 5000000000ll);
    EXPECT(first_is(r, AVS_STRESS_RULE_EDGE_FACES, 2, 0, 255, 128, 64));
    raw[kStressRawKey] = lattice_key(AVS_STRESS_RULE_EDGE_FACES, 2, 1, 257ull * 128ull * 65ull - 1ull);
    EXPECT(first_is(check_stress_report(raw, 3u, n), AVS_STRESS_RULE_EDGE_FACES, 2, 1, 256, 127, 64));
    raw[kStressRawKey] = lattice_key(AVS_STRESS_RULE_EDGE_FACES, 2, 2, 257ull * 129ull * 64ull - 1ull);
    EXPECT(first_is(check_stress_report(raw, 3u, n), AVS_STRESS_RULE_EDGE_FACES, 2, 2, 256, 128, 63));
    raw[kStressRawKey] = lattice_key(AVS_STRESS_RULE_EDGE_VALUE, 0, 1, 5ull + 1025ull * (7ull + 512ull * 200ull));
    raw[AVS_STRESS_RULE_EDGE_VALUE] = 1;
    EXPECT(first_is(check_stress_report(raw, 3u, n), AVS_STRESS_RULE_EDGE_VALUE, 0, 1, 5, 7, 200));
    r = check_stress_report(raw, 2u, n); // only the centre rules asked for
    EXPECT(r.violations[AVS_STRESS_RULE_CENTER_LABEL] == 3 && r.violations[AVS_STRESS_RULE_EDGE_FACES] == 0 && r.passed == 0);
    // centre lattices are the cell lattices, whatever axis the key carries: level 1 is 512 x 256 x 128
    std::memset(raw, 0, sizeof(raw));
    raw[AVS_STRESS_RULE_CENTER_EDGES] = 1;
    raw[kStressRawKey] = lattice_key(AVS_STRESS_RULE_CENTER_EDGES, 1, 0, 512ull * 256ull * 128ull - 1ull);
    EXPECT(first_is(check_stress_report(raw, 2u, n), AVS_STRESS_RULE_CENTER_EDGES, 1, 0, 511, 255, 127));
    raw[kStressRawKey] = lattice_key(AVS_STRESS_RULE_CENTER_VALUE, 0, 0, 1023ull + 1024ull * (511ull + 512ull * 255ull));
    raw[AVS_STRESS_RULE_CENTER_VALUE] = 1;
    EXPECT(first_is(check_stress_report(raw, 2u, n), AVS_STRESS_RULE_CENTER_VALUE, 0, 0, 1023, 511, 255));
    // a centre of level 7 on a lattice that is one cell wide there; the numbering rules report the id
    const int tiny[3] = {128, 128, 256};
    std::memset(raw, 0, sizeof(raw));
    raw[AVS_STRESS_RULE_CENTER_LABEL] = 1;
    raw[kStressRawKey] = lattice_key(AVS_STRESS_RULE_CENTER_LABEL, 7, 0, 1);
    EXPECT(first_is(check_stress_report(raw, 2u, tiny), AVS_STRESS_RULE_CENTER_LABEL, 7, 0, 0, 0, 1));
    raw[AVS_STRESS_RULE_EDGE_CELLS] = 1; // ... and the x edges there are 1 x 2 x 3
    raw[kStressRawKey] = lattice_key(AVS_STRESS_RULE_EDGE_CELLS, 7, 0, 5);
    EXPECT(first_is(check_stress_report(raw, 1u, tiny), AVS_STRESS_RULE_EDGE_CELLS, 7, 0, 0, 1, 2));
    for (int rule : {AVS_STRESS_RULE_EDGE_NUMBERING, AVS_STRESS_RULE_CENTER_NUMBERING}) {
        std::memset(raw, 0, sizeof(raw));
        raw[rule] = 2;
        raw[kStressRawKey] = lattice_key(rule, 0, 0, 2147483646ull);
        EXPECT(first_is(check_stress_report(raw, 3u, tiny), rule, 0, 0, 2147483646, 0, 0));
    }
    // a key without a count that was asked for (the violation belongs to the other kind): passed
    r = check_stress_report(raw, 1u, tiny);
    EXPECT(r.passed == 1 && r.first_rule == -1);
    r = check_stress_report(raw, 2u, tiny);
    r.active_edges = 11;
    r.active_centers = 12;
    // the hand-over writes struct_size bytes and not one more: the caller's struct sits at the very end of a heap block
    for (int32_t size : {8, 12, 24, 80, 92, full - 8, full}) {
        std::vector<unsigned char> block((size_t)size, 0x5a);
        avs_stress_check *out = reinterpret_cast<avs_stress_check *>(block.data());
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
        if (size >= full - 8) { // one field short: active_edges is there, active_centers is not
            int64_t edges;
            std::memcpy(&edges, block.data() + offsetof(avs_stress_check, active_edges), 8);
            EXPECT(edges == 11);
        }
        if (size == full) {
            int64_t centers;
            std::memcpy(&centers, block.data() + offsetof(avs_stress_check, active_centers), 8);
            EXPECT(centers == 12);
        }
    }
    { // a caller built against a larger, future struct: the bytes behind today's struct stay
        std::vector<unsigned char> block(200, 0x5a);
        const int32_t size = 200;
        std::memcpy(block.data(), &size, sizeof(size));
        report_hand_over(r, reinterpret_cast<avs_stress_check *>(block.data()));
        int32_t back;
        std::memcpy(&back, block.data(), 4);
        EXPECT(back == 200);
        for (size_t b = sizeof(avs_stress_check); b < block.size(); ++b) EXPECT(block[b] == 0x5a);
    }
    std::puts("ok");
    return 0;
}
