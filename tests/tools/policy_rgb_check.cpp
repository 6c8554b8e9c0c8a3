// policy_rgb_check.cpp -- pins policy::forward_rgb / inverse_rgb
// (csrc/hpdct_policy.hpp) on the CPU, as policy_blocks_check.cpp pins the plane
// entries: family, variant bits, workgroup size, cap and grid.  Host code only
// (g++); run by tests/test_rgb_host.py.
#include <cstdio>

#include "hpdct_policy.hpp"

using namespace hpdct;
using namespace hpdct::policy;

namespace {

int g_bad = 0;

void expect(const char* what, const Choice& c, unsigned var, uint32_t grid_x) {
    if (c.family == Family::kRgb && c.var == var && c.block == 256u && block_of(c.var) == 256u && c.cap_wgs == 0u &&
        c.grid_x == grid_x && c.grid_y == 1u)
        return;
    ++g_bad;
    std::printf("MISMATCH %s: family %d var 0x%08x block %u cap %u grid %u x %u (expected var 0x%08x grid %u)\n", what,
                static_cast<int>(c.family), c.var, c.block, c.cap_wgs, c.grid_x, c.grid_y, var, grid_x);
}

// a height x width frame: 16x16 MCUs (4:2:0) or 8x8 tiles (4:4:4)
RgbCall call(uint32_t h, uint32_t w, bool s420, int qmode_luma = 0, int qmode_chroma = 0) {
    RgbCall c;
    const uint32_t side = s420 ? 16u : 8u;
    c.units = (h / side) * (w / side);
    c.s420 = s420, c.qmode_luma = qmode_luma, c.qmode_chroma = qmode_chroma;
    return c;
}

}  // namespace

int main() {
    constexpr unsigned kFwd = kVarNT | kBlkStaged;  // 256-thread workgroups: no size bits
    constexpr unsigned kJ = kVarFastDiv | kVarJpegQ;
    // the quotient pairs: (JPEG forms, 3-op), (3-op, 3-op), IEEE division for both otherwise
    expect("fwd 420 8192^2 default tables", forward_rgb(call(8192, 8192, true, 2, 1)),
           kFwd | kRgb420 | kJ | kRgbChromaFastDiv, 1024);
    expect("fwd 420 8192^2 integer tables", forward_rgb(call(8192, 8192, true, 1, 1)),
           kFwd | kRgb420 | kVarFastDiv | kRgbChromaFastDiv, 1024);
    expect("fwd 420 8192^2 IEEE", forward_rgb(call(8192, 8192, true, 0, 0)), kFwd | kRgb420, 1024);
    expect("fwd 420 default luma, fractional chroma", forward_rgb(call(8192, 8192, true, 2, 0)), kFwd | kRgb420, 1024);
    expect("fwd 420 fractional luma, integer chroma", forward_rgb(call(8192, 8192, true, 0, 1)), kFwd | kRgb420, 1024);
    expect("fwd 444 8192^2 default tables", forward_rgb(call(8192, 8192, false, 2, 1)), kFwd | kJ | kRgbChromaFastDiv,
           4096);
    expect("fwd 444 8192^2 integer tables", forward_rgb(call(8192, 8192, false, 1, 1)),
           kFwd | kVarFastDiv | kRgbChromaFastDiv, 4096);
    expect("fwd 444 8192^2 IEEE", forward_rgb(call(8192, 8192, false, 0, 0)), kFwd, 4096);
    // small and ragged frames: the same kernels, one 64-unit set per wave
    expect("fwd 420 16x16", forward_rgb(call(16, 16, true, 2, 1)), kFwd | kRgb420 | kJ | kRgbChromaFastDiv, 1);
    expect("fwd 420 16x1040 (65 MCUs)", forward_rgb(call(16, 1040, true, 2, 1)),
           kFwd | kRgb420 | kJ | kRgbChromaFastDiv, 1);
    expect("fwd 420 48x2032 (381 MCUs, 6 sets)", forward_rgb(call(48, 2032, true, 2, 1)),
           kFwd | kRgb420 | kJ | kRgbChromaFastDiv, 2);
    expect("fwd 444 8x520 (65 tiles)", forward_rgb(call(8, 520, false, 2, 1)), kFwd | kJ | kRgbChromaFastDiv, 1);
    expect("inv 420 8192^2", inverse_rgb(call(8192, 8192, true)), kRgb420, 1024);
    expect("inv 444 8192^2", inverse_rgb(call(8192, 8192, false)), 0u, 4096);
    expect("inv 420 16x1040", inverse_rgb(call(16, 1040, true)), kRgb420, 1);
    expect("inv 444 24x1016 (381 tiles)", inverse_rgb(call(24, 1016, false)), 0u, 2);
    // a table that fails the skip criterion: the full chain on the general (kRgbClip) instantiation
    for (int s = 0; s < 2; ++s) {
        RgbCall full = call(8192, 8192, s != 0);
        full.full_chain = true;
        expect("inv 8192^2 full chain", inverse_rgb(full), kVarFullChain | kRgbClip | (s != 0 ? kRgb420 : 0u),
               s != 0 ? 1024 : 4096);
        full.clip = true;
        expect("inv 8192^2 full chain, clipped frame", inverse_rgb(full),
               kVarFullChain | kRgbClip | (s != 0 ? kRgb420 : 0u), s != 0 ? 1024 : 4096);
        // the flag means nothing to the forward
        RgbCall fwd = call(8192, 8192, s != 0, 2, 1);
        fwd.full_chain = true;
        expect("fwd 8192^2 default tables, full_chain set", forward_rgb(fwd),
               kFwd | (s != 0 ? kRgb420 : 0u) | kJ | kRgbChromaFastDiv, s != 0 ? 1024 : 4096);
    }
    static_assert((kVarFullChain & (kRgbFwdVar | kRgbInvVar | kRgb420 | kRgbChromaFastDiv | kRgbClip | kVarFastDiv |
                                    kVarJpegQ)) == 0u,
                  "kVarFullChain aliases a bit of the existing colour kernels");
    if (g_bad != 0) {
        std::printf("policy_rgb_check: %d rows differ\n", g_bad);
        return 1;
    }
    std::printf("policy_rgb_check: ok\n");
    return 0;
}
