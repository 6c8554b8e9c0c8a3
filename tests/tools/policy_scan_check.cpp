// policy_scan_check.cpp -- pins the entropy coder's rows of hpdct_policy.hpp on
// the CPU: one-wave workgroups, one per restart interval up to kScanMaxWgs, no
// residency cap; the offsets launch one 1024-thread workgroup.  Built and run by
// tests/test_jpeg_scan_host.py.
#include <cstdio>

#include "hpdct_policy.hpp"

int main() {
    using namespace hpdct;
    using namespace hpdct::policy;
    int bad = 0;
    auto expect = [&](const char* what, bool ok) {
        if (!ok) ++bad, std::printf("MISMATCH %s\n", what);
    };
    // tests/test_gpu_scan_limits.py::test_more_intervals_than_workgroups codes 1025 x 1025 intervals, 2049 past
    // this cap, to reach the coding kernel's second turn: a larger cap needs a larger frame there
    expect("kScanMaxWgs", kScanMaxWgs == (1u << 20));
    for (uint32_t n : {1u, 2u, 512u, 1024u, kScanMaxWgs - 1u, kScanMaxWgs, kScanMaxWgs + 1u, 0xffffffffu})
        for (int natural = 0; natural < 2; ++natural)
            for (int emit = 0; emit < 2; ++emit) {
                ScanCall c;
                c.intervals = n, c.natural = natural != 0;
                const Choice ch = scan_code(c, emit != 0);
                expect("family", ch.family == Family::kScan);
                expect("one-wave workgroups", ch.block == 64u && block_of(ch.var) == 64u && ch.cap_wgs == 0u);
                expect("grid", ch.grid_x == (n < kScanMaxWgs ? n : kScanMaxWgs) && ch.grid_y == 1u);
                expect("natural bit", ((ch.var & kScanNatural) != 0u) == (natural != 0));
                expect("emit bit", ((ch.var & kScanEmit) != 0u) == (emit != 0));
                expect("no other bit", (ch.var & ~(kScanNatural | kScanEmit | (3u << 12))) == 0u);
            }
    const Choice o = scan_offsets();
    expect("offsets", o.family == Family::kScan && o.block == 1024u && block_of(o.var) == 1024u && o.grid_x == 1u &&
                          o.grid_y == 1u && o.cap_wgs == 0u && (o.var & kScanOffsets) != 0u);
    if (bad) return std::printf("policy_scan_check: %d mismatches\n", bad), 1;
    std::printf("policy_scan_check: ok\n");
    return 0;
}
