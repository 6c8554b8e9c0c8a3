// policy_blocks_check.cpp -- pins policy::forward_blocks / inverse_blocks
// (csrc/hpdct_policy.hpp) on the CPU, as policy_check.cpp pins the other
// entries: family, variant bits, workgroup size, cap and grid.  Host code only
// (g++); run by tests/test_blocks_host.py.
#include <cstdio>

#include "hpdct_policy.hpp"

using namespace hpdct;
using namespace hpdct::policy;

namespace {

int g_bad = 0;

void expect(const char* what, const Choice& c, unsigned var, uint32_t grid_x) {
    if (c.family == Family::kBlocks && c.var == var && c.block == 256u && block_of(c.var) == 256u && c.cap_wgs == 0u &&
        c.grid_x == grid_x && c.grid_y == 1u)
        return;
    ++g_bad;
    std::printf("MISMATCH %s: family %d var 0x%08x block %u cap %u grid %u x %u (expected var 0x%08x grid %u)\n", what,
                static_cast<int>(c.family), c.var, c.block, c.cap_wgs, c.grid_x, c.grid_y, var, grid_x);
}

Call call(uint32_t h, uint64_t w, Elem out, int qmode, int mapping = HPDCT_MAPPING_AUTO) {
    Call c;
    const uint32_t tx = static_cast<uint32_t>(w / 8u);
    c.g = TileGrid{(h / 8u) * tx, tx, w};
    c.out = out, c.qmode = qmode, c.mapping = mapping;
    return c;
}

}  // namespace

int main() {
    constexpr unsigned kFwd = kVarNT | kBlkStaged;  // 256-thread workgroups: no size bits
    constexpr unsigned kJ = kVarFastDiv | kVarJpegQ;
    expect("fwd 8192^2 default table", forward_blocks(call(8192, 8192, Elem::kU8, 2)), kFwd | kJ, 4096);
    expect("fwd 8192^2 integer table", forward_blocks(call(8192, 8192, Elem::kU8, 1)), kFwd | kVarFastDiv, 4096);
    expect("fwd 8192^2 IEEE", forward_blocks(call(8192, 8192, Elem::kU8, 0)), kFwd, 4096);
    // small frames and forced mappings: still the tile kernel (one 64-tile set per wave)
    expect("fwd 8x8", forward_blocks(call(8, 8, Elem::kU8, 2)), kFwd | kJ, 1);
    expect("fwd 8x520 (65 tiles)", forward_blocks(call(8, 520, Elem::kU8, 2)), kFwd | kJ, 1);
    expect("fwd 64x2056 (2056 tiles, 33 sets)", forward_blocks(call(64, 2056, Elem::kU8, 2)), kFwd | kJ, 9);
    expect("fwd 1024^2 forced octet", forward_blocks(call(1024, 1024, Elem::kU8, 2, HPDCT_MAPPING_OCTET)), kFwd | kJ,
           64);
    expect("inv 8192^2 -> fp32", inverse_blocks(call(8192, 8192, Elem::kF32, 0)), kVarNT | kVarLdsStore, 4096);
    expect("inv 8192x8200 -> fp32", inverse_blocks(call(8192, 8200, Elem::kF32, 0)),
           kVarNT | kVarLdsStore | kVarStraddle, 4100);
    expect("inv 8192x8200 -> u8", inverse_blocks(call(8192, 8200, Elem::kU8, 0)), kVarNT, 4100);
    expect("inv 1024^2 -> u8 forced duo", inverse_blocks(call(1024, 1024, Elem::kU8, 0, HPDCT_MAPPING_DUO)), kVarNT,
           64);
    // a table that fails the skip criterion: the plain full-chain kernel for either output, whatever the width
    for (Elem out : {Elem::kF32, Elem::kU8}) {
        Call full = call(8192, 8200, out, 0);
        full.full_chain = true;
        expect("inv 8192x8200 full chain", inverse_blocks(full), kVarFullChain, 4100);
        full = call(24, 1016, out, 0, HPDCT_MAPPING_OCTET);
        full.full_chain = true;
        expect("inv 24x1016 full chain forced octet", inverse_blocks(full), kVarFullChain, 2);
    }
    // the flag means nothing to the forward
    {
        Call fwd = call(8192, 8192, Elem::kU8, 2);
        fwd.full_chain = true;
        expect("fwd 8192^2 default table, full_chain set", forward_blocks(fwd), kFwd | kJ, 4096);
    }
    static_assert(kInvFullVar == kVarFullChain && block_of(kInvFullVar) == 256u, "the plain full-chain variant");
    static_assert((kVarFullChain & (blocks_inv_var(Elem::kF32) | blocks_inv_var(Elem::kU8) | kVarStraddle | kBlocksFwdVar |
                                    kVarFastDiv | kVarJpegQ)) == 0u,
                  "kVarFullChain aliases a bit of the existing block kernels");
    if (g_bad != 0) {
        std::printf("policy_blocks_check: %d rows differ\n", g_bad);
        return 1;
    }
    std::printf("policy_blocks_check: ok\n");
    return 0;
}
