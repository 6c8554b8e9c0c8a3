// policy_check.cpp -- pins the kernel-selection policy (csrc/hpdct_policy.hpp)
// on the CPU: for a table of calls, the kernel family, variant bits, workgroup
// size, residency cap and grid the library launches.  Every mapping computes
// the same bits, so no GPU test can tell a wrong tier from the right one; a
// change of a threshold or a cap has to change a row here.  Host code only
// (g++, as tests/tools/asan.mk builds the host sources); run by
// tests/test_policy.py.
#include <cstdio>

#include "hpdct_policy.hpp"

using namespace hpdct;
using namespace hpdct::policy;

namespace {

int g_rows = 0, g_bad = 0;

TileGrid frame(uint32_t height, uint64_t width) {
    const uint32_t tx = static_cast<uint32_t>(width / 8u);
    return TileGrid{(height / 8u) * tx, tx, width};
}

void expect(const char* what, const Choice& c, Family family, unsigned var, uint32_t block, uint32_t cap,
            uint32_t grid_x, uint32_t grid_y = 1) {
    ++g_rows;
    // the families whose kernels take kVar: its workgroup-size bits say the same as block
    const bool kvar = family == Family::kTile || family == Family::kOctet || family == Family::kDuo ||
                      family == Family::kRowFirstDuo;
    if (c.family == family && c.var == var && c.block == block && c.cap_wgs == cap && c.grid_x == grid_x &&
        c.grid_y == grid_y && (!kvar || block_of(c.var) == c.block))
        return;
    ++g_bad;
    std::printf("MISMATCH %s:\n  got      family %d var 0x%08x block %u cap %u grid %u x %u\n"
                "  expected family %d var 0x%08x block %u cap %u grid %u x %u\n",
                what, static_cast<int>(c.family), c.var, c.block, c.cap_wgs, c.grid_x, c.grid_y,
                static_cast<int>(family), var, block, cap, grid_x, grid_y);
}

Call fwd(uint32_t h, uint64_t w, Elem in, Elem out, int qmode, int mapping = HPDCT_MAPPING_AUTO, uint32_t cus = 256) {
    Call c;
    c.g = frame(h, w), c.in = in, c.out = out, c.qmode = qmode, c.mapping = mapping, c.cus = cus;
    return c;
}

RtCall rt(uint32_t h, uint64_t w, int recon, bool sums, bool slot, int qmode, int mapping = HPDCT_MAPPING_AUTO) {
    RtCall c;
    c.g = frame(h, w), c.recon = recon, c.sums = sums, c.slot = slot, c.qmode = qmode, c.mapping = mapping;
    return c;
}

}  // namespace

int main() {
    constexpr Elem U8 = Elem::kU8, I8 = Elem::kI8, F32 = Elem::kF32;
    constexpr unsigned kJ = kVarFastDiv | kVarJpegQ;
    constexpr unsigned kTileF32 = kVarNT | kVarLdsStore;  // + the workgroup-size bits
    constexpr unsigned kOctF32 = kVarNT | kOctRestage;
    constexpr int TILE = HPDCT_MAPPING_TILE, OCTET = HPDCT_MAPPING_OCTET, DUO = HPDCT_MAPPING_DUO;

    // --- forward uint8 -> fp32, the default table (qmode 2) ---
    expect("u8->f32 8192^2", forward(fwd(8192, 8192, U8, F32, 2)), Family::kDuoFwdU8, kJ, 256, 4, 8192);
    // 32768 tiles = 1024 duo waves = kDuoFwdMinWavesPerCU * 256: the AUTO threshold, and one tile row below it
    expect("u8->f32 2048x1024", forward(fwd(2048, 1024, U8, F32, 2)), Family::kDuoFwdU8, kJ, 256, 4, 256);
    expect("u8->f32 2040x1024", forward(fwd(2040, 1024, U8, F32, 2)), Family::kOctet, kOctF32 | kVarFastDiv, 256, 0,
           1020);
    expect("u8->f32 1024^2", forward(fwd(1024, 1024, U8, F32, 2)), Family::kOctet, kOctF32 | kVarFastDiv, 256, 0, 512);
    // tiles_x 513: 4104 sets, 17 per CU
    expect("u8->f32 4096x4104", forward(fwd(4096, 4104, U8, F32, 2)), Family::kTile,
           with_block<1024>(kTileF32 | kJ | kVarStraddle), 1024, 0, 257);
    // 513 x 1025 tiles: 8217 sets, 33 per CU
    expect("u8->f32 4104x8200", forward(fwd(4104, 8200, U8, F32, 2)), Family::kTile,
           with_block<64>(kTileF32 | kJ | kVarStraddle | kVarPacked | kVarHoistRun), 64, 7, 8217);
    expect("u8->f32 8192^2 forced tile", forward(fwd(8192, 8192, U8, F32, 2, TILE)), Family::kTile,
           with_block<64>(kTileF32 | kJ | kVarPacked | kVarHoistRun), 64, 7, 16384);
    expect("u8->f32 8192^2 forced octet", forward(fwd(8192, 8192, U8, F32, 2, OCTET)), Family::kOctet,
           kOctF32 | kVarFastDiv, 256, 0, 32768);
    expect("u8->f32 8192^2 forced duo", forward(fwd(8192, 8192, U8, F32, 2, DUO)), Family::kDuoFwdU8, kJ, 256, 4, 8192);
    expect("u8->f32 64x256 forced duo", forward(fwd(64, 256, U8, F32, 2, DUO)), Family::kDuoFwdU8, kJ, 256, 4, 2);
    expect("u8->f32 64x256 auto", forward(fwd(64, 256, U8, F32, 2)), Family::kOctet, kOctF32 | kVarFastDiv, 256, 0, 8);
    expect("u8->f32 8192^2 IEEE", forward(fwd(8192, 8192, U8, F32, 0)), Family::kTile,
           with_block<64>(kTileF32 | kVarPacked | kVarHoistRun), 64, 7, 16384);
    expect("u8->f32 8192^2 qmode 1", forward(fwd(8192, 8192, U8, F32, 1)), Family::kDuoFwdU8, kVarFastDiv, 256, 4, 8192);
    {  // another level shift: no duo forward, the tile kernel
        Call c = fwd(8192, 8192, U8, F32, 1);
        c.shift128 = false;
        expect("u8->f32 8192^2 shift 0", forward(c), Family::kTile,
               with_block<64>(kTileF32 | kVarFastDiv | kVarPacked | kVarHoistRun), 64, 7, 16384);
    }
    // the thresholds scale with the CU count: at 304 CUs 1024 duo waves are
    // below 4 per CU, and 8217 sets are 28 per CU (1024-thread workgroups)
    expect("u8->f32 2048x1024, 304 CUs", forward(fwd(2048, 1024, U8, F32, 2, HPDCT_MAPPING_AUTO, 304)), Family::kOctet,
           kOctF32 | kVarFastDiv, 256, 0, 1024);
    expect("u8->f32 4104x8200, 304 CUs", forward(fwd(4104, 8200, U8, F32, 2, HPDCT_MAPPING_AUTO, 304)), Family::kTile,
           with_block<1024>(kTileF32 | kJ | kVarStraddle), 1024, 0, 514);

    // 8192 sets are exactly kBigWgSetsPerCU per CU (the C4 slab): still 1024-thread workgroups (33: 4104x8200 above)
    expect("u8->f32 2048x16384 forced tile", forward(fwd(2048, 16384, U8, F32, 2, TILE)), Family::kTile,
           with_block<1024>(kTileF32 | kJ), 1024, 0, 512);

    // --- forward uint8 -> int8 ---
    // the octet cut, kOctetSetsPerCU * 256 = 2048 sets: 2040 sets below it, 2048 at it
    expect("u8->i8 2040x4096", forward(fwd(2040, 4096, U8, I8, 1)), Family::kOctet, kVarNT | kVarFastDiv, 256, 0, 4080);
    expect("u8->i8 2048x4096", forward(fwd(2048, 4096, U8, I8, 1)), Family::kTile, kVarNT | kVarI8Pack | kVarFastDiv,
           256, 0, 512);
    expect("u8->i8 8192^2 qmode 2", forward(fwd(8192, 8192, U8, I8, 2)), Family::kTile,
           with_block<64>(kVarNT | kVarI8Pack | kJ), 64, 20, 16384);
    expect("u8->i8 8192^2 qmode 1", forward(fwd(8192, 8192, U8, I8, 1)), Family::kTile,
           kVarNT | kVarI8Pack | kVarFastDiv, 256, 0, 4096);

    // --- forward fp32 -> fp32 (qmode 1: the checked quotient) ---
    expect("f32->f32 8192^2", forward(fwd(8192, 8192, F32, F32, 1)), Family::kDuo,
           with_block<64>(kVarNT | kVarFastDivChecked), 64, 10, 32768);
    {
        Call c = fwd(8192, 8192, F32, F32, 1);
        c.writeback = true;
        expect("f32->f32 8192^2 write-back", forward(c), Family::kDuo, with_block<64>(kVarNT | kVarFastDivChecked), 64,
               10, 32768);
    }
    // 8192 duo waves < kDuoCapWavesPerCU * 256
    expect("f32->f32 4096^2", forward(fwd(4096, 4096, F32, F32, 1)), Family::kDuo, kVarNT | kVarFastDivChecked, 256, 0,
           2048);
    // the duo cap, kDuoCapWavesPerCU * 256 = 16384 duo waves: 16320 below it, 16384 at it
    expect("f32->f32 2040x16384", forward(fwd(2040, 16384, F32, F32, 1)), Family::kDuo, kVarNT | kVarFastDivChecked, 256,
           0, 4080);
    expect("f32->f32 2048x16384", forward(fwd(2048, 16384, F32, F32, 1)), Family::kDuo,
           with_block<64>(kVarNT | kVarFastDivChecked), 64, 10, 16384);
    expect("f32->f32 8192^2 IEEE", forward(fwd(8192, 8192, F32, F32, 0)), Family::kDuo, kVarNT, 256, 0, 8192);
    {
        Call c = fwd(8192, 8192, F32, F32, 1);
        c.row_first = true;
        expect("f32->f32 row-first 8192^2", forward(c), Family::kRowFirstDuo, with_block<64>(kVarNT), 64, 10, 32768);
        c.g = frame(4096, 4096);
        expect("f32->f32 row-first 4096^2", forward(c), Family::kRowFirstDuo, kVarNT, 256, 0, 2048);
        c.g = frame(8192, 8192), c.mapping = TILE;
        expect("f32->f32 row-first forced tile", forward(c), Family::kTile,
               with_block<512>(kTileF32 | kVarRowFirst), 512, 0, 2048);
    }

    // --- inverse ---
    {
        Call c = fwd(8192, 8192, F32, F32, 0);
        expect("inv f32->f32 8192^2", inverse(c), Family::kDuo, with_block<64>(kVarNT), 64, 10, 32768);
        c.wb_dequant = true;
        expect("inv f32->f32 dequant write-back", inverse(c), Family::kDuo, with_block<64>(kVarNT | kVarWbDequant), 64,
               10, 32768);
        c.mapping = TILE;
        expect("inv f32->f32 dequant write-back, forced tile", inverse(c), Family::kTile,
               with_block<512>(kTileF32 | kVarWbDequant), 512, 0, 2048);
        c.mapping = OCTET;
        expect("inv f32->f32 dequant write-back, forced octet", inverse(c), Family::kOctet, kOctF32 | kVarWbDequant, 256,
               0, 32768);
    }
    expect("inv f32->u8 8192^2", inverse(fwd(8192, 8192, F32, U8, 0)), Family::kDuo, with_block<512>(kVarNT), 512, 0,
           4096);
    expect("inv i8->f32 4096x4104", inverse(fwd(4096, 4104, I8, F32, 0)), Family::kTile,
           with_block<512>(kTileF32 | kVarStraddle), 512, 0, 513);
    // int8 coefficients under a table that fails the skip criterion: the plain full-chain variant of the
    // mapping's kernel (256-thread workgroups, no staging, no straddle form), for either output
    for (Elem out : {F32, U8}) {
        Call c = fwd(4096, 4104, I8, out, 0);
        c.full_chain = true;
        expect("inv i8 4096x4104 full chain", inverse(c), Family::kTile, kVarFullChain, 256, 0, 1026);
        c.mapping = OCTET;
        expect("inv i8 4096x4104 full chain, forced octet", inverse(c), Family::kOctet, kVarFullChain, 256, 0, 8208);
        c.mapping = DUO;  // no duo kernel takes int8: as AUTO
        expect("inv i8 4096x4104 full chain, forced duo", inverse(c), Family::kTile, kVarFullChain, 256, 0, 1026);
        c = fwd(1024, 1024, I8, out, 0);
        c.full_chain = true;
        expect("inv i8 1024^2 full chain (AUTO: octet)", inverse(c), Family::kOctet, kVarFullChain, 256, 0, 512);
        // nothing is skipped without dequantisation or with a caller's T: the flag is not read
        c = fwd(4096, 4096, I8, out, 0);
        c.full_chain = true, c.quant = false;
        expect("inv i8 4096^2 no dequant, full_chain set", inverse(c), Family::kTile, prod_var(out), 512, 0, 512);
        c.quant = true, c.builtin_t = false;
        expect("inv i8 4096^2 caller's T, full_chain set", inverse(c), Family::kTile, prod_var(out), 512, 0, 512);
    }
    {
        // fp32 coefficients keep every term anyway: the flag is not read
        Call c = fwd(8192, 8192, F32, F32, 0);
        c.full_chain = true;
        expect("inv f32->f32 8192^2, full_chain set", inverse(c), Family::kDuo, with_block<64>(kVarNT), 64, 10, 32768);
    }
    static_assert(kInvFullVar == kVarFullChain, "the plain full-chain variant: 256 threads, no other bit");
    static_assert((kVarFullChain & (prod_var(F32) | prod_var(U8) | prod_var(I8) | oct_var(F32) | oct_var(U8) | kDuoVar |
                                    kVarStraddle | kVarWbDequant | kVarRowFirst | kProductOnlyVarBits | kVarFastDiv |
                                    kF32OneWaveForm | (3u << 12))) == 0u,
                  "kVarFullChain aliases a bit of the existing plane kernels");

    // --- frame lists, uint8 -> fp32, qmode 2 ---
    {
        Call c = fwd(512, 512, U8, F32, 2);
        expect("frames 1 x 512^2", forward_frames(c), Family::kTile, with_block<512>(kTileF32 | kJ), 512, 0, 8, 1);
        c.frames = 16;  // 128 duo waves each: the duo rule on the whole list
        expect("frames 16 x 512^2", forward_frames(c), Family::kDuoFwdU8, kJ, 256, 4, 32, 16);
        // 1024 x 1032: 258 ragged sets per frame; 15 / 16 / 31 / 32 frames are 16 / 17 / 32 / 33 sets per CU
        c.g = frame(1024, 1032);
        constexpr unsigned kCapped = with_block<64>(kTileF32 | kJ | kVarStraddle | kVarPacked);
        c.frames = 15;
        expect("frames 15 x 1024x1032", forward_frames(c), Family::kTile, with_block<512>(kTileF32 | kJ | kVarStraddle),
               512, 0, 33, 15);
        c.frames = 16;
        expect("frames 16 x 1024x1032", forward_frames(c), Family::kTile, kCapped, 64, 12, 258, 16);
        c.frames = 31;
        expect("frames 31 x 1024x1032", forward_frames(c), Family::kTile, kCapped, 64, 12, 258, 31);
        c.frames = 32;
        expect("frames 32 x 1024x1032", forward_frames(c), Family::kTile, kCapped, 64, 7, 258, 32);
        c.out = I8;
        expect("frames 32 x 1024x1032 int8", forward_frames(c), Family::kTile, kVarNT | kVarI8Pack | kJ, 256, 0, 65, 32);
    }

    // --- round trip, 8192^2 ---
    expect("rt u8 recon + sums", roundtrip(rt(8192, 8192, kRtReconU8, true, true, 2)), Family::kRtDuo, kJ, 256, 0, 8192);
    expect("rt u8 recon", roundtrip(rt(8192, 8192, kRtReconU8, false, false, 2)), Family::kRtDuo, kJ, 256, 4, 8192);
    expect("rt f32 recon + sums", roundtrip(rt(8192, 8192, kRtReconF32, true, true, 2)), Family::kRtDuo, kJ, 256, 4,
           8192);
    expect("rt sums only", roundtrip(rt(8192, 8192, kRtReconNone, true, true, 1)), Family::kRtDuo, kVarFastDiv, 256, 0,
           8192);
    expect("rt forward alone", roundtrip(rt(8192, 8192, kRtReconNone, false, false, 2)), Family::kDuoFwdU8, kJ, 256, 4,
           8192);
    expect("rt width 8200", roundtrip(rt(8192, 8200, kRtReconU8, true, true, 2)), Family::kRtTile, kJ | kVarStraddle,
           256, 0, 4100);
    expect("rt forced tile", roundtrip(rt(8192, 8192, kRtReconU8, true, true, 2, TILE)), Family::kRtTile, kJ, 256, 0,
           4096);
    expect("rt IEEE", roundtrip(rt(8192, 8192, kRtReconU8, true, true, 0)), Family::kRtTile, 0u, 256, 0, 4096);
    expect("rt IEEE width 8200", roundtrip(rt(8192, 8200, kRtReconU8, true, true, 0)), Family::kRtTile, 0u, 256, 0, 4100);
    expect("rt sums without a slot", roundtrip(rt(8192, 8192, kRtReconU8, true, false, 2)), Family::kRtTile, kJ, 256, 0,
           4096);
    // the duo kernels' 32-bit row offsets: widths below 2^22 px only
    expect("rt width 2^22", roundtrip(rt(8, uint64_t(1) << 22, kRtReconU8, false, false, 2)), Family::kRtTile, kJ, 256, 0,
           2048);
    expect("rt width 2^22 - 256", roundtrip(rt(8, (uint64_t(1) << 22) - 256, kRtReconU8, false, false, 2)),
           Family::kRtDuo, kJ, 256, 4, 4096);
    expect("u8->f32 width 2^22 forced duo", forward(fwd(8, uint64_t(1) << 22, U8, F32, 2, DUO)), Family::kTile,
           with_block<1024>(kTileF32 | kJ), 1024, 0, 512);

    if (g_bad != 0) {
        std::printf("policy_check: %d of %d rows differ\n", g_bad, g_rows);
        return 1;
    }
    std::printf("policy_check: ok (%d rows)\n", g_rows);
    return 0;
}
