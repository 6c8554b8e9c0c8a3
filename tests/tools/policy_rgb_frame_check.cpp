// policy_rgb_frame_check.cpp -- pins what the colour frame calls launch
// (csrc/hpdct_policy.hpp, rgb_whole_aligned of csrc/hpdct_kernels.h), after
// policy_rgb_check.cpp: a whole-unit frame with an 8-byte aligned base and
// pitch gets exactly the Choice the existing policy rows give (the kernels
// without kRgbClip), a ragged or unaligned one the same launch shape for the
// padded unit grid with kRgbClip.  Host code only (g++); run by
// tests/test_rgb_frame_host.py.
#include <cstdio>

#include "hpdct_policy.hpp"

using namespace hpdct;
using namespace hpdct::policy;

namespace {

int g_bad = 0;

// a height x width frame at `base` with rows `pitch` bytes apart, as hpdct_api.cpp fills the grid
struct Frame {
    uint64_t h, w, pitch;
    uintptr_t base;
    bool s420;
};
RgbGrid grid(const Frame& f) {
    const uint64_t side = f.s420 ? 16u : 8u;
    const uint64_t uy = (f.h + side - 1u) / side, ux = (f.w + side - 1u) / side;
    return RgbGrid{static_cast<uint32_t>(uy * ux), static_cast<uint32_t>(ux), f.pitch, f.h, f.w};
}
RgbCall call(const Frame& f, int qmode_luma = 0, int qmode_chroma = 0) {
    const RgbGrid g = grid(f);
    RgbCall c;
    c.units = g.nunits, c.s420 = f.s420, c.qmode_luma = qmode_luma, c.qmode_chroma = qmode_chroma;
    c.clip = !rgb_whole_aligned(reinterpret_cast<const void*>(f.base), g, f.s420);
    return c;
}
// the call the existing entry points make for the padded size
RgbCall dense(uint32_t hp, uint32_t wp, bool s420, int qmode_luma = 0, int qmode_chroma = 0) {
    RgbCall c;
    const uint32_t side = s420 ? 16u : 8u;
    c.units = (hp / side) * (wp / side);
    c.s420 = s420, c.qmode_luma = qmode_luma, c.qmode_chroma = qmode_chroma;
    return c;
}

bool same(const Choice& a, const Choice& b) {
    return a.family == b.family && a.var == b.var && a.block == b.block && a.cap_wgs == b.cap_wgs &&
           a.grid_x == b.grid_x && a.grid_y == b.grid_y;
}
void expect_same(const char* what, const Choice& got, const Choice& want) {
    if (same(got, want) && (got.var & kRgbClip) == 0u) return;
    ++g_bad;
    std::printf("MISMATCH %s: var 0x%08x block %u cap %u grid %u x %u (expected var 0x%08x grid %u x %u)\n", what,
                got.var, got.block, got.cap_wgs, got.grid_x, got.grid_y, want.var, want.grid_x, want.grid_y);
}
// the padded grid's Choice with the clip bit and nothing else
void expect_clip(const char* what, const Choice& got, Choice want) {
    want.var |= kRgbClip;
    if (same(got, want) && block_of(got.var) == 256u) return;
    ++g_bad;
    std::printf("MISMATCH %s: var 0x%08x block %u cap %u grid %u x %u (expected var 0x%08x grid %u x %u)\n", what,
                got.var, got.block, got.cap_wgs, got.grid_x, got.grid_y, want.var, want.grid_x, want.grid_y);
}

}  // namespace

int main() {
    constexpr uintptr_t kBase = uintptr_t(1) << 20;
    // whole units, aligned base and pitch: the existing rows, dense or pitched, every quotient pair
    for (int s = 0; s < 2; ++s) {
        const bool s420 = s != 0;
        for (int ql = 0; ql <= 2; ++ql)
            for (int qc = 0; qc <= 1; ++qc) {
                expect_same("fwd 8192^2 dense", forward_rgb(call({8192, 8192, 3 * 8192, kBase, s420}, ql, qc)),
                            forward_rgb(dense(8192, 8192, s420, ql, qc)));
                expect_same("fwd 8192^2 pitch + 64",
                            forward_rgb(call({8192, 8192, 3 * 8192 + 64, kBase + 8, s420}, ql, qc)),
                            forward_rgb(dense(8192, 8192, s420, ql, qc)));
            }
        expect_same("inv 8192^2 dense", inverse_rgb(call({8192, 8192, 3 * 8192, kBase, s420})),
                    inverse_rgb(dense(8192, 8192, s420)));
        expect_same("inv 128x1024 pitch + 64", inverse_rgb(call({128, 1024, 3 * 1024 + 64, kBase, s420})),
                    inverse_rgb(dense(128, 1024, s420)));
        expect_same("fwd 16x16", forward_rgb(call({16, 16, 48, kBase, s420}, 2, 1)),
                    forward_rgb(dense(16, 16, s420, 2, 1)));
    }
    // 8184 is whole 8x8 tiles (4:4:4: no clip, pitch 24552 = 8 * 3069) and half an MCU short (4:2:0: clip)
    expect_same("fwd 444 8184^2", forward_rgb(call({8184, 8184, 3 * 8184, kBase, false}, 2, 1)),
                forward_rgb(dense(8184, 8184, false, 2, 1)));
    expect_clip("fwd 420 8184^2", forward_rgb(call({8184, 8184, 3 * 8184, kBase, true}, 2, 1)),
                forward_rgb(dense(8192, 8192, true, 2, 1)));
    expect_clip("inv 420 8184^2", inverse_rgb(call({8184, 8184, 3 * 8184, kBase, true})),
                inverse_rgb(dense(8192, 8192, true)));
    // ragged sizes: the padded grid's wave count
    expect_clip("fwd 420 1080x1920", forward_rgb(call({1080, 1920, 3 * 1920, kBase, true}, 2, 1)),
                forward_rgb(dense(1088, 1920, true, 2, 1)));
    expect_clip("fwd 444 667x1000", forward_rgb(call({667, 1000, 3000, kBase, false}, 1, 1)),
                forward_rgb(dense(672, 1000, false, 1, 1)));
    expect_clip("fwd 420 667x1000 IEEE", forward_rgb(call({667, 1000, 3000, kBase, true}, 0, 0)),
                forward_rgb(dense(672, 1008, true, 0, 0)));
    expect_clip("inv 444 13x515", inverse_rgb(call({13, 515, 1545, kBase, false})), inverse_rgb(dense(16, 520, false)));
    expect_clip("inv 420 1x1", inverse_rgb(call({1, 1, 3, kBase, true})), inverse_rgb(dense(16, 16, true)));
    // whole units, but an unaligned pitch or base
    expect_clip("fwd 444 24x1016 pitch + 1", forward_rgb(call({24, 1016, 3 * 1016 + 1, kBase, false}, 2, 1)),
                forward_rgb(dense(24, 1016, false, 2, 1)));
    expect_clip("fwd 420 128x1024 pitch + 4", forward_rgb(call({128, 1024, 3 * 1024 + 4, kBase, true}, 2, 1)),
                forward_rgb(dense(128, 1024, true, 2, 1)));
    expect_clip("fwd 420 128x1024 base + 1", forward_rgb(call({128, 1024, 3 * 1024, kBase + 1, true}, 2, 1)),
                forward_rgb(dense(128, 1024, true, 2, 1)));
    expect_clip("inv 444 64x512 base + 4", inverse_rgb(call({64, 512, 3 * 512, kBase + 4, false})),
                inverse_rgb(dense(64, 512, false)));
    // a table that fails the skip criterion: one full-chain choice per padded grid, the general instantiation,
    // for whole aligned frames and ragged ones alike
    for (int s = 0; s < 2; ++s) {
        const bool s420 = s != 0;
        RgbCall whole = call({128, 1024, 3 * 1024, kBase, s420}), ragged = call({25, 1033, 3 * 1033, kBase, s420});
        whole.full_chain = ragged.full_chain = true;
        Choice want = inverse_rgb(dense(128, 1024, s420));
        want.var |= kVarFullChain;
        expect_clip("inv 128x1024 full chain", inverse_rgb(whole), want);
        want = inverse_rgb(dense(32, 1040, s420));
        want.var |= kVarFullChain;
        expect_clip("inv 25x1033 full chain", inverse_rgb(ragged), want);
    }
    // the numbers themselves, once: 1080p 4:2:0 is 68 x 120 = 8160 MCUs, 128 waves, 32 workgroups
    const Choice c = forward_rgb(call({1080, 1920, 3 * 1920, kBase, true}, 2, 1));
    if (c.grid_x != 32u || c.block != 256u || c.cap_wgs != 0u ||
        c.var != (kVarNT | kBlkStaged | kRgb420 | kVarFastDiv | kVarJpegQ | kRgbChromaFastDiv | kRgbClip)) {
        ++g_bad;
        std::printf("MISMATCH 1080p 4:2:0 forward: var 0x%08x grid %u\n", c.var, c.grid_x);
    }
    if (g_bad != 0) {
        std::printf("policy_rgb_frame_check: %d rows differ\n", g_bad);
        return 1;
    }
    std::printf("policy_rgb_frame_check: ok\n");
    return 0;
}
