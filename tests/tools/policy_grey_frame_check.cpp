// policy_grey_frame_check.cpp -- pins what the grey frame calls launch
// (csrc/hpdct_policy.hpp, grey_whole_aligned of csrc/hpdct_grey_frame.h), after
// policy_rgb_frame_check.cpp: a whole-tile frame with an 8-byte aligned base and
// pitch gets the launch shape and variant of the blocks rows (forward_blocks /
// inverse_blocks to uint8) under the grey family, a ragged or unaligned one the
// same for the padded tile grid with kGreyClip.  Host code only (g++); run by
// tests/test_grey_frame_host.py.
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
};
GreyGrid grid(const Frame& f) {
    const uint64_t ty = (f.h + 7u) / 8u, tx = (f.w + 7u) / 8u;
    return GreyGrid{static_cast<uint32_t>(ty * tx), static_cast<uint32_t>(tx), f.pitch, f.h, f.w};
}
GreyCall call(const Frame& f, int qmode = 0, bool full_chain = false) {
    const GreyGrid g = grid(f);
    GreyCall c;
    c.tiles = g.ntiles, c.qmode = qmode, c.full_chain = full_chain;
    c.clip = !grey_whole_aligned(reinterpret_cast<const void*>(f.base), g);
    return c;
}
// the call hpdct_forward_blocks / hpdct_inverse_blocks (uint8) make for the padded size
Call blocks(uint32_t hp, uint32_t wp, int qmode = 0, bool full_chain = false) {
    Call c;
    c.g = TileGrid{(hp / 8u) * (wp / 8u), wp / 8u, wp};
    c.qmode = qmode, c.out = Elem::kU8, c.full_chain = full_chain;
    return c;
}

// the blocks row's launch under the grey family, with `extra` variant bits
void expect(const char* what, const Choice& got, Choice want, unsigned extra) {
    want.family = Family::kGrey, want.var |= extra;
    if (got.family == want.family && got.var == want.var && got.block == want.block && got.cap_wgs == want.cap_wgs &&
        got.grid_x == want.grid_x && got.grid_y == want.grid_y && block_of(got.var) == got.block)
        return;
    ++g_bad;
    std::printf("MISMATCH %s: var 0x%08x block %u cap %u grid %u x %u (expected var 0x%08x grid %u x %u)\n", what,
                got.var, got.block, got.cap_wgs, got.grid_x, got.grid_y, want.var, want.grid_x, want.grid_y);
}

}  // namespace

int main() {
    constexpr uintptr_t kBase = uintptr_t(1) << 20;
    // whole tiles, aligned base and pitch: the blocks rows, dense or pitched, every quotient
    for (int q = 0; q <= 2; ++q) {
        expect("fwd 8192^2 dense", forward_grey(call({8192, 8192, 8192, kBase}, q)), forward_blocks(blocks(8192, 8192, q)),
               0u);
        expect("fwd 8192^2 pitch + 64", forward_grey(call({8192, 8192, 8192 + 64, kBase + 8}, q)),
               forward_blocks(blocks(8192, 8192, q)), 0u);
        expect("fwd 1080x1920", forward_grey(call({1080, 1920, 1920, kBase}, q)), forward_blocks(blocks(1080, 1920, q)),
               0u);
    }
    expect("inv 8192^2 dense", inverse_grey(call({8192, 8192, 8192, kBase})), inverse_blocks(blocks(8192, 8192)), 0u);
    expect("inv 24x1016 pitch + 40", inverse_grey(call({24, 1016, 1056, kBase})), inverse_blocks(blocks(24, 1016)), 0u);
    expect("fwd 8x8", forward_grey(call({8, 8, 8, kBase}, 2)), forward_blocks(blocks(8, 8, 2)), 0u);
    // ragged sizes: the padded grid's wave count, the clip bit and nothing else
    expect("fwd 1x1", forward_grey(call({1, 1, 1, kBase}, 2)), forward_blocks(blocks(8, 8, 2)), kGreyClip);
    expect("fwd 7x9", forward_grey(call({7, 9, 9, kBase}, 1)), forward_blocks(blocks(8, 16, 1)), kGreyClip);
    expect("fwd 13x515", forward_grey(call({13, 515, 515, kBase}, 0)), forward_blocks(blocks(16, 520, 0)), kGreyClip);
    expect("fwd 13x515 pitch 520", forward_grey(call({13, 515, 520, kBase}, 2)), forward_blocks(blocks(16, 520, 2)),
           kGreyClip);
    expect("fwd 667x1000", forward_grey(call({667, 1000, 1000, kBase}, 2)), forward_blocks(blocks(672, 1000, 2)),
           kGreyClip);
    expect("fwd 8185x8190 pitch 8192", forward_grey(call({8185, 8190, 8192, kBase}, 2)),
           forward_blocks(blocks(8192, 8192, 2)), kGreyClip);
    expect("inv 17x512", inverse_grey(call({17, 512, 512, kBase})), inverse_blocks(blocks(24, 512)), kGreyClip);
    expect("inv 1x1", inverse_grey(call({1, 1, 1, kBase})), inverse_blocks(blocks(8, 8)), kGreyClip);
    expect("inv 1083x1920", inverse_grey(call({1083, 1920, 1920, kBase})), inverse_blocks(blocks(1088, 1920)), kGreyClip);
    // whole tiles, but an unaligned pitch or base
    expect("fwd 24x1016 pitch + 1", forward_grey(call({24, 1016, 1017, kBase}, 2)), forward_blocks(blocks(24, 1016, 2)),
           kGreyClip);
    expect("fwd 24x1016 pitch + 4", forward_grey(call({24, 1016, 1020, kBase}, 2)), forward_blocks(blocks(24, 1016, 2)),
           kGreyClip);
    expect("fwd 24x1016 base + 3", forward_grey(call({24, 1016, 1016, kBase + 3}, 2)),
           forward_blocks(blocks(24, 1016, 2)), kGreyClip);
    expect("inv 64x512 base + 4", inverse_grey(call({64, 512, 512, kBase + 4})), inverse_blocks(blocks(64, 512)),
           kGreyClip);
    // a table that fails the skip criterion: the blocks row's full-chain choice for the padded grid, the general
    // instantiation, for whole aligned frames and ragged ones alike
    expect("inv 64x512 full chain", inverse_grey(call({64, 512, 512, kBase}, 0, true)),
           inverse_blocks(blocks(64, 512, 0, true)), kGreyClip);
    expect("inv 13x515 full chain", inverse_grey(call({13, 515, 515, kBase}, 0, true)),
           inverse_blocks(blocks(16, 520, 0, true)), kGreyClip);
    // the numbers themselves, once: 1080x1920 is 135 x 240 = 32400 tiles, 507 waves, 127 workgroups
    const Choice f = forward_grey(call({1080, 1920, 1920, kBase}, 2));
    if (f.grid_x != 127u || f.block != 256u || f.cap_wgs != 0u || f.family != Family::kGrey ||
        f.var != (kVarNT | kBlkStaged | kVarFastDiv | kVarJpegQ)) {
        ++g_bad;
        std::printf("MISMATCH 1080x1920 forward: var 0x%08x grid %u\n", f.var, f.grid_x);
    }
    const Choice i = inverse_grey(call({1083, 1920, 1920, kBase}));
    if (i.grid_x != 128u || i.block != 256u || i.cap_wgs != 0u || i.var != (kVarNT | kGreyClip)) {
        ++g_bad;
        std::printf("MISMATCH 1083x1920 inverse: var 0x%08x grid %u\n", i.var, i.grid_x);
    }
    const Choice fc = inverse_grey(call({64, 512, 512, kBase}, 0, true));
    if (fc.var != (kVarFullChain | kGreyClip) || fc.block != 256u) {
        ++g_bad;
        std::printf("MISMATCH full chain inverse: var 0x%08x block %u\n", fc.var, fc.block);
    }
    if (g_bad != 0) {
        std::printf("policy_grey_frame_check: %d rows differ\n", g_bad);
        return 1;
    }
    std::printf("policy_grey_frame_check: ok\n");
    return 0;
}
