// policy_unscan_split_check.cpp -- pins the split entropy decoder's rows of
// hpdct_policy.hpp on the CPU: the geometry (segment, group, rounds, threshold),
// one workgroup of kUnsplitGroup lanes per group of segments or per interval
// under the grid cap, the plan's single workgroup, the clear launch's units and
// the serial pass, which is the parent's decode launch row for row.  The
// parent's own rows (policy_unscan_check.cpp) are not touched.  Built and run by
// tests/test_unscan_split_host.py.
#include <cstdio>

#include "hpdct_policy.hpp"
#include "hpdct_unscan_split.hpp"

int main() {
    using namespace hpdct;
    using namespace hpdct::policy;
    int bad = 0;
    auto expect = [&](const char* what, bool ok) {
        if (!ok) ++bad, std::printf("MISMATCH %s\n", what);
    };
    // tests/unscan_split_inputs.py's stubborn scans need a segment that is a multiple of 32 bytes;
    // the settle and write kernels are built for workgroups of 256
    expect("segment", kUnsplitSegBytes == 256u && kUnsplitSegBytes % 32u == 0u);
    expect("group", kUnsplitGroup == 256u);
    expect("rounds", kUnsplitRounds == 4u);
    expect("threshold", kUnsplitMinBytes == 3328u);
    expect("grid cap", kUnsplitMaxWgs == 65536u);
    expect("the header's names", unsplit::kSegBytes == kUnsplitSegBytes && unsplit::kGroup == kUnsplitGroup &&
                                     unsplit::kRounds == kUnsplitRounds);
    const Choice p = unsplit_plan();
    expect("plan", p.family == Family::kUnsplit && p.block == 1024u && block_of(p.var) == 1024u && p.grid_x == 1u &&
                       p.grid_y == 1u && p.cap_wgs == 0u && (p.var & (7u << 29)) == kUnsplitPlan);
    struct L {
        uint64_t n;
        uint32_t grid;
    };
    for (const L& l : {L{0u, 1u}, L{1u, 1u}, L{833u, 833u}, L{65535u, 65535u}, L{65536u, 65536u}, L{65537u, 65536u},
                       L{uint64_t(1) << 40, 65536u}}) {
        for (int natural = 0; natural < 2; ++natural) {
            const Choice s = unsplit_settle(l.n), w = unsplit_write(l.n, natural != 0);
            expect("settle", s.family == Family::kUnsplit && s.block == 256u && block_of(s.var) == 256u &&
                                 s.cap_wgs == 0u && s.grid_x == l.grid && s.grid_y == 1u &&
                                 (s.var & ~(3u << 12)) == kUnsplitSettle);
            expect("write", w.family == Family::kUnsplit && w.block == 256u && block_of(w.var) == 256u &&
                                w.cap_wgs == 0u && w.grid_x == l.grid && w.grid_y == 1u &&
                                (w.var & ~(3u << 12)) == (kUnsplitWrite | (natural ? kScanNatural : 0u)));
        }
        if (l.n <= 0xffffffffu) {
            const Choice o = unsplit_offsets(static_cast<uint32_t>(l.n));
            expect("offsets", o.family == Family::kUnsplit && o.block == 256u && o.grid_x == l.grid && o.grid_y == 1u &&
                                  (o.var & ~(3u << 12)) == kUnsplitOffsets);
        }
    }
    for (const L& l : {L{1u, 1u}, L{256u, 1u}, L{257u, 2u}, L{uint64_t(8192) * 8192 / 64 * 8, 32768u},
                       L{uint64_t(1) << 34, 65536u}}) {
        const Choice c = unsplit_clear(l.n);
        expect("clear", c.family == Family::kUnsplit && c.block == 256u && c.grid_x == l.grid && c.grid_y == 1u &&
                            (c.var & ~(3u << 12)) == kUnsplitClear);
    }
    for (uint32_t intervals : {1u, 1024u, 8192u, 8193u, 16384u, 16385u, 65536u, 65537u, 1050625u, 0xffffffffu})
        for (int natural = 0; natural < 2; ++natural) {
            UnscanCall c;
            c.intervals = intervals, c.natural = natural != 0;
            const Choice a = unscan_decode(c), b = unsplit_serial(c);
            expect("serial", b.family == Family::kUnsplit && b.var == (a.var | kUnsplitSerial) && b.block == a.block &&
                                 b.grid_x == a.grid_x && b.grid_y == a.grid_y && b.cap_wgs == a.cap_wgs &&
                                 unscan_lanes_of(b.var) == unscan_lanes(intervals));
        }
    // the workspace's budgets: a segment per kUnsplitSegBytes bytes and one more per interval, a group per
    // kUnsplitGroup segments and one more per interval
    const unsplit::Layout l = unsplit::layout(1024u, uint64_t(1) << 20);
    expect("budgets", l.nseg == 4096u + 1024u && l.ngrp == 20u + 1024u && l.bytes % 16u == 0u && l.exits % 16u == 0u &&
                          l.bytes == l.starts + 32u * l.nseg);
    if (bad) return std::printf("policy_unscan_split_check: %d mismatches\n", bad), 1;
    std::printf("policy_unscan_split_check: ok\n");
    return 0;
}
