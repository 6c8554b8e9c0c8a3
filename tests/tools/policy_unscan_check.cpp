// policy_unscan_check.cpp -- pins the entropy decoder's rows of hpdct_policy.hpp
// on the CPU: one-wave workgroups of which 1, 4, 16 or 64 lanes take an interval
// (up to 8,192, 16,384 and 65,536 intervals, and beyond); the stride loop beyond
// 64 * kUnscanMaxWgs intervals; the marker search and its rank launch.  Built
// and run by tests/test_jpeg_unscan_host.py.
#include <cstdio>

#include "hpdct_policy.hpp"

int main() {
    using namespace hpdct;
    using namespace hpdct::policy;
    int bad = 0;
    auto expect = [&](const char* what, bool ok) {
        if (!ok) ++bad, std::printf("MISMATCH %s\n", what);
    };
    // tests/test_gpu_unscan.py decodes 1025 x 1025 intervals to reach the decode kernel's second turn: a larger
    // cap needs a larger frame there
    expect("kUnscanMaxWgs", kUnscanMaxWgs == 8192u);
    expect("kUnscanChunkBytes", kUnscanChunkBytes == 4096u);
    struct Row {
        uint32_t intervals, lanes, grid;
    };
    const Row rows[] = {{1u, 1u, 1u},           {1024u, 1u, 1024u},      {8192u, 1u, 8192u},     {8193u, 4u, 2049u},
                        {16384u, 4u, 4096u},    {16385u, 16u, 1025u},    {32768u, 16u, 2048u},   {65536u, 16u, 4096u},
                        {65537u, 64u, 1025u},   {131072u, 64u, 2048u},   {262144u, 64u, 4096u},  {524288u, 64u, 8192u},
                        {524289u, 64u, 8192u},  {1050625u, 64u, 8192u},  {0xffffffffu, 64u, 8192u}};
    for (const Row& r : rows)
        for (int natural = 0; natural < 2; ++natural) {
            UnscanCall c;
            c.intervals = r.intervals, c.natural = natural != 0;
            const Choice ch = unscan_decode(c);
            expect("family", ch.family == Family::kUnscan);
            expect("one-wave workgroups", ch.block == 64u && block_of(ch.var) == 64u && ch.cap_wgs == 0u);
            expect("lanes", unscan_lanes(r.intervals) == r.lanes && unscan_lanes_of(ch.var) == r.lanes);
            expect("grid", ch.grid_x == r.grid && ch.grid_y == 1u);
            expect("natural bit", ((ch.var & kScanNatural) != 0u) == (natural != 0));
            expect("no other bit", (ch.var & ~(kScanNatural | kUnscanLanes1 | kUnscanLanes4 | kUnscanLanes16 |
                                               (3u << 12))) == 0u);
            // every interval has a lane in the first turn, or the grid is at its cap
            expect("covered", uint64_t(ch.grid_x) * r.lanes >= r.intervals || ch.grid_x == kUnscanMaxWgs);
        }
    for (int place = 0; place < 2; ++place) {
        struct L {
            uint64_t chunks;
            uint32_t grid;
        };
        for (const L& l : {L{1u, 1u}, L{4u, 1u}, L{5u, 2u}, L{32768u, 8192u}, L{32769u, 8192u}, L{uint64_t(1) << 51, 8192u}}) {
            const Choice ch = unscan_locate(l.chunks, place != 0);
            expect("locate", ch.family == Family::kUnscan && ch.block == 256u && block_of(ch.var) == 256u &&
                                 ch.cap_wgs == 0u && ch.grid_x == l.grid && ch.grid_y == 1u);
            expect("locate bits", (ch.var & kUnscanCount) != 0u && ((ch.var & kUnscanPlace) != 0u) == (place != 0));
        }
    }
    const Choice o = unscan_rank();
    expect("rank", o.family == Family::kUnscan && o.block == 1024u && block_of(o.var) == 1024u && o.grid_x == 1u &&
                       o.grid_y == 1u && o.cap_wgs == 0u && (o.var & kUnscanRank) != 0u);
    if (bad) return std::printf("policy_unscan_check: %d mismatches\n", bad), 1;
    std::printf("policy_unscan_check: ok\n");
    return 0;
}
