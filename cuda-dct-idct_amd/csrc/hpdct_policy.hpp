// hpdct_policy.hpp -- which kernel a call launches.  Pure host functions of
// their arguments (no HIP call, no global); the launchers instantiate what they
// return, tests/tools/policy_check.cpp pins the table on the CPU.
#pragma once

#include <type_traits>

#include "hpdct.h"
#include "hpdct_grey_frame.h"
#include "hpdct_kernels.h"

namespace hpdct {
namespace policy {

// kTile: fdct / idct / fdct_frames_kernel; kDuo: the fp32 duo kernels;
// kDuoFwdU8: fdct_duo_u8(_frames)_kernel; kRt*: the round-trip kernels
// kBlocks: fdct_blocks_kernel / idct_blocks_kernel (hpdct_blocks.hpp)
// kRgb: fdct_rgb_kernel / idct_rgb_kernel (hpdct_rgb.hpp)
// kScan: scan_code_kernel / scan_offsets_kernel (hpdct_scan.hpp)
// kUnscan: unscan_locate_kernel / unscan_rank_kernel / unscan_decode_kernel (hpdct_unscan.hpp)
// kUnsplit: the unsplit_*_kernel of hpdct_unscan_split.hip
// kGrey: fdct_grey_frame_kernel / idct_grey_frame_kernel (hpdct_grey_frame.hpp)
enum class Family { kTile, kOctet, kDuo, kDuoFwdU8, kRowFirstDuo, kRtDuo, kRtTile, kBlocks, kRgb, kScan, kUnscan, kUnsplit, kGrey };
enum class Elem { kU8, kI8, kF32 };

// var: the kernel's kVar; kDuoFwdU8 and kRt* carry their quotient and straddle bits there
struct Choice {
    Family family;
    unsigned var;
    uint32_t block, cap_wgs;  // threads per workgroup; resident workgroups per CU at most (0: no cap)
    uint32_t grid_x, grid_y;
};
// A forward, inverse or frame-list call: frames of g per launch; quant also
// means dequantise; wb_dequant: the inverse's dq_out; qmode as launch_fdct.
struct Call {
    TileGrid g{};
    uint32_t frames = 1;
    Elem in = Elem::kU8, out = Elem::kF32;
    bool quant = true, builtin_t = true, writeback = false, wb_dequant = false, row_first = false, shift128 = true;
    int qmode = 0, mapping = HPDCT_MAPPING_AUTO;
    uint32_t cus = 256;
    // integer-input inverses with the built-in T: the table fails skip_zero_exact (hpdct_api.cpp) for the
    // input type's range, so the kernel keeps every term of T (kVarFullChain)
    bool full_chain = false;
};
// A round trip (launch_roundtrip).  slot: its sums have a spread slot.
struct RtCall {
    TileGrid g{};
    int recon = kRtReconNone;
    bool sums = false, slot = false;
    int qmode = 0, mapping = HPDCT_MAPPING_AUTO;
    uint32_t cus = 256;
};

// waves of a launch: one per 64-tile set, per 8 tiles (octet) or per 32 (duo)
constexpr uint32_t tile_waves(const TileGrid& g) { return (g.ntiles + 63u) / 64u; }
constexpr uint32_t octet_waves(const TileGrid& g) { return (g.ntiles + 7u) / 8u; }
constexpr uint32_t duo_waves(const TileGrid& g) { return (g.ntiles + 31u) / 32u; }
// workgroups of `block` threads holding `waves` waves
constexpr uint32_t wgs_for(uint32_t waves, uint32_t block) { return (waves + block / 64u - 1u) / (block / 64u); }

// Residency caps (round 3).  The DRAM serves the headline's mix of 1 B/px
// reads and 4 B/px non-temporal writes best with few concurrent streams: its
// access pattern alone runs at 0.72 of 8 TB/s with the hardware's default
// residency and at 0.75-0.80 with 12-4 waves per CU (tools/kbench3 "occpat",
// profiles/r03/m/).  The arithmetic needs more than one wave per SIMD to issue
// at full rate, so the u8 -> fp32 tile kernel runs in one-wave workgroups with
// at most kF32CapWavesPerCU resident per CU.  The cap is a
// dynamic-LDS reservation (hpdct_residency.hpp).
// 10 in round 3; 7 since round 4: 56.9-57.1 against 57.7-58.4 us at 8192^2
// with the per-position quantiser (profiles/r04/b/kb3_jqcap_8192.log; 6 waves
// per CU: 64.8 us, profiles/r04/a/kb3_jqf_8192.log)
constexpr uint32_t kF32CapWavesPerCU = 7;

// Product variant choice (measured on MI355X, tools/kbench.hip).
//
// Tile-per-lane kernels (hpdct_kernels_impl.hpp), for frames of >= 8 tile
// sets (64 tiles each) per CU: fp32 planes are stored through the LDS
// re-staging with non-temporal stores (1 KiB contiguous per store
// instruction), 8-bit planes with non-temporal stores; the int8 output with
// the SDWA byte-pack conversion; the fast quotient where the caller proved it
// legal.  512-thread workgroups (1-3 % faster than 256 on every kernel in
// round 1), except the int8 output: 256-thread workgroups since its JPEG-form
// quantiser (round 4: 8192^2 28.9 against 29.8-30.0 us with 512,
// profiles/r04/a/kb3_jqi8_8192.log), and with the JPEG forms one-wave
// workgroups under a residency cap (forward, kI8CapWavesPerCU).
constexpr unsigned prod_var(Elem out) {
    return (out == Elem::kI8 ? with_block<256>(kVarNT | kVarI8Pack) : with_block<512>(kVarNT)) |
           (out == Elem::kF32 ? kVarLdsStore : 0u);
}
// Octet kernels (hpdct_octet.hpp, 8 lanes per tile) for smaller frames,
// where the tile-per-lane grid is too short to fill 256 CUs (1024^2: 6.2 ->
// 3.7 us).  256-thread workgroups; fp32 rows re-staged for 256-B runs.
constexpr unsigned oct_var(Elem out) { return kVarNT | (out == Elem::kF32 ? kOctRestage : 0u); }
constexpr uint32_t kOctetSetsPerCU = 8;
// Duo kernels (hpdct_duo.hpp, 2 lanes per tile, 1 KiB row loads and stores)
// for fp32 -> fp32 at the other sizes (8192^2: forward 102.4 -> 89.6 us,
// inverse 93.3 -> 88.0 us, compat forward with write-back 159 -> 136 us).
constexpr unsigned kDuoVar = kVarNT;

// duo_in: fp32 coefficients or pixels in the reference's pass order (duo-capable)
inline Family pick_mapping(const Call& c, bool duo_in) {
    if (c.mapping == HPDCT_MAPPING_TILE) return Family::kTile;
    if (c.mapping == HPDCT_MAPPING_OCTET) return Family::kOctet;
    if (c.mapping == HPDCT_MAPPING_DUO && duo_in) return Family::kDuo;
    if (tile_waves(c.g) < kOctetSetsPerCU * c.cus) return Family::kOctet;
    return duo_in ? Family::kDuo : Family::kTile;
}

// uint8 -> fp32 tile kernels (the headline):
//  - frames of at most kBigWgSetsPerCU sets per CU, where the whole grid is
//    one or two rounds of resident waves: 1024-thread workgroups, no cap
//    (4096^2: 16.3 us against 18.2-20.0 capped at 7-12; 2048 x 16384 (32 sets
//    per CU, the C4 8-way slab): 32.6 against 33.3-34.5 capped at 7-12 --
//    round 4, profiles/r04/c/kb3_capsz_*.log; round 3 had capped 17-32 sets
//    per CU at 12 per CU);
//  - larger frames: one-wave workgroups, at most kF32CapWavesPerCU resident
//    per CU (16384^2: 214.8-215.6 us at 7, 219-220 at 8-10, 222 at 12,
//    250 uncapped 1024-thread).  Round 3, before the per-position
//    quantiser and the cap of 7: 8192^2: 58.6-58.7 us at 9-10 waves/CU
//    against 61.8-62.1 for the uncapped 512-thread kernel and 62.5 for the
//    uncapped one-wave kernel; 16384^2: 218-219 against 238; 2048 x 16384:
//    33.7 against 35.0 (profiles/r03/m/kb3_occsz_*.log).  With the cap the
//    packed-fp32 transform (kVarPacked) gains another 1-2 % (8192^2: 57.6 at
//    10 waves/CU against 58.7 for the scalar form).
constexpr uint32_t kBigWgSetsPerCU = 32;
// kVarHoistRun (round 5): the whole-run test once per set and each
// row's store one row later: 56.5 against 57.4-57.7 us at 8192^2,
// bit-exact (tools/kbench3 group hoist, profiles/r05/o/)
constexpr unsigned kF32OneWaveForm = kVarPacked | kVarHoistRun;
// frame lists keep round 3's tiers: uncapped 512-thread workgroups up to 16
// sets per CU, capped at 12 waves per CU up to 32, packed without the hoist
constexpr uint32_t kFramesUncappedSetsPerCU = 16;
constexpr uint32_t kMidCapSetsPerCU = 32;
constexpr uint32_t kF32CapWavesPerCUMid = 12;
// uint8 -> int8 with the default JPEG table's forms: one-wave workgroups, at
// most kI8CapWavesPerCU resident per CU (round 4, two boxes: 8192^2
// 29.6-31.1 against 30.8-32.6 us for 256-thread workgroups, 4096^2 9.1-9.2
// against 9.5-9.6, 16384^2 equal; 24 per CU: 30.0-32.2.
// profiles/r04/f/kb3_i8cap_*.log, profiles/r04/g/kb3_i8cap_*.log)
constexpr uint32_t kI8CapWavesPerCU = 20;
// fp32 -> fp32 duo inverse and row-first kernels: the headline's residency cap
// once the grid holds at least kDuoCapWavesPerCU of their waves (32 tiles each)
// per CU: one-wave workgroups, at most kDuoCapWaves resident per CU.  8192^2
// inverse 86.0 against 89.0-89.4 us (profiles/r03/m/kb3_invb_8192.log); driver
// bench: idct_all_blocks_cuda 89.7 -> 86.8, cublasDCTv2 pair 139.3 / 139.5 ->
// 137.3 / 132.4.
constexpr uint32_t kDuoCapWavesPerCU = 64;
constexpr uint32_t kDuoCapWaves = 10;
// uint8 -> quantised fp32 forward on the two-lanes-per-tile mapping (round 6;
// fdct_duo_u8_kernel): kDuoFwdBlock-thread workgroups, at most kDuoFwdCapWgs
// resident per CU (16 waves); AUTO takes it from kDuoFwdMinWavesPerCU of its
// 32-tile waves per CU (below that, 1024^2 and smaller, the octet kernel is as
// fast); forced "duo" takes it at any size, forced "tile" or "octet" never.
constexpr uint32_t kDuoFwdBlock = 256, kDuoFwdCapWgs = 4, kDuoFwdMinWavesPerCU = 4;
// Round-trip duo kernel: 256-thread workgroups, 6 waves per SIMD (74 VGPRs,
// no spills; 7 and 8 spill and run slower, tools/kb_rt, profiles/r05/a/).
// Whole runs only: the kRun = false kernel (ragged widths, 92 VGPRs) is
// slower than the tile kernel there (4096 x 4104: 36.9 against 31.9 us with
// sums, profiles/r05/b/kb_rt_ragged.log).
// Round 6: at most kDuoRtCapWgs workgroups (16 waves) per CU, by the
// dynamic-LDS reservation, for the fp32 reconstruction and for every round
// trip without sums: 8192^2 fp32 reconstruction + sums 100.2-100.3 against
// 106.6-106.7 us uncapped, without sums 98.9 against 102.4; uint8
// reconstruction without sums 67.2 against 68.4 (tools/kb_rt group f32cap,
// profiles/r06/kb_rt_f32cap.log).  The uint8 reconstruction with sums (the C3
// one pass) gains nothing from it (group rtcap) and stays uncapped.
constexpr uint32_t kDuoRtBlock = 256, kDuoRtCapWgs = 4;
constexpr uint32_t kRtBlock = 256;  // the round-trip tile kernel's workgroup (hpdct_roundtrip.hpp)

// The uint8-input duo kernels (fdct_duo_u8_kernel, roundtrip_duo_kernel) take
// whole 32-tile runs only, and address a wave's rows with 32-bit byte offsets
// from the wave's base (DuoAddr, 2 k width + 4 lane fp32 words), which stay
// below 2^32 for widths below 2^22 pixels.
inline bool duo_u8_runs(const TileGrid& g) { return g.tiles_x % 32u == 0u && g.width < (uint64_t(1) << 22); }

// quotient bits of a uint8-input kernel for qmode 0 / 1 / 2
constexpr unsigned quot_bits(int qmode) { return qmode == 2 ? kVarFastDiv | kVarJpegQ : qmode == 1 ? kVarFastDiv : 0u; }
inline Choice duo_fwd_u8(const Call& c) {
    return {Family::kDuoFwdU8, quot_bits(c.qmode), kDuoFwdBlock, kDuoFwdCapWgs,
            wgs_for(duo_waves(c.g), kDuoFwdBlock), c.frames};
}
// the size rule on the whole list of frames
inline bool duo_fwd_u8_fits(const Call& c) {
    if (c.mapping == HPDCT_MAPPING_TILE || c.mapping == HPDCT_MAPPING_OCTET || !duo_u8_runs(c.g)) return false;
    return c.mapping == HPDCT_MAPPING_DUO ||
           static_cast<uint64_t>(c.g.ntiles / 32u) * c.frames >= uint64_t(kDuoFwdMinWavesPerCU) * c.cus;
}

// a kernel of `var` in workgroups of its own size, one per wave-group of `waves`
inline Choice uncapped(Family f, unsigned var, uint32_t waves, uint32_t frames = 1) {
    return {f, var, block_of(var), 0u, wgs_for(waves, block_of(var)), frames};
}
inline Choice one_wave(Family f, unsigned var, uint32_t cap, uint32_t waves, uint32_t frames = 1) {
    return {f, with_block<64>(var), 64u, cap, waves, frames};
}
// the fp32 duo kernels' cap (kDuoCapWavesPerCU)
inline Choice duo_f32(Family f, unsigned var, bool cappable, const Call& c) {
    if (cappable && duo_waves(c.g) >= kDuoCapWavesPerCU * c.cus) return one_wave(f, var, kDuoCapWaves, duo_waves(c.g));
    return uncapped(f, var, duo_waves(c.g));
}

// launch_fdct: uint8 or fp32 in, fp32 or int8 out
inline Choice forward(const Call& c) {
    const bool f32 = c.in == Elem::kF32 && c.out == Elem::kF32;
    const unsigned base = prod_var(c.out);
    if (f32 && c.row_first) {  // cublasDCTv2 pass order: duo (rows first), or tile when forced
        if (c.mapping != HPDCT_MAPPING_TILE) return duo_f32(Family::kRowFirstDuo, kDuoVar, true, c);
        return uncapped(Family::kTile, base | kVarRowFirst, tile_waves(c.g));
    }
    // the verified quotient: integer table, uint8 input, built-in T
    const bool fastdiv_ok = c.in == Elem::kU8 && c.quant && c.builtin_t && !c.writeback;
    if (fastdiv_ok && c.out == Elem::kF32 && c.qmode != 0 && c.shift128 && duo_fwd_u8_fits(c)) return duo_fwd_u8(c);
    const Family map = pick_mapping(c, f32);
    if (map == Family::kDuo) {
        // The checked 3-op quotient (integer table: the JPEG default, the drop-in
        // surface) takes the inverse's residency cap since round 6: 8192^2
        // dct_all_blocks_cuda 125.7 against 131.5 us uncapped, without the
        // write-back 88.1 against 89.5 (tools/kbench3 groups dropcap / fwdcap,
        // profiles/r06/).  With IEEE division (any other table) it stays uncapped:
        // VALU-heavier, the cap made it slower (round 3: 91.6 -> 101.8 us).
        const bool checked = c.quant && c.qmode != 0;
        return duo_f32(Family::kDuo, kDuoVar | (checked ? kVarFastDivChecked : 0u), checked, c);
    }
    // the default JPEG table's per-position forms: tile kernels (the octet
    // mapping of small frames keeps the verified quotient everywhere)
    if (map == Family::kOctet)
        return uncapped(Family::kOctet, oct_var(c.out) | (fastdiv_ok && c.qmode != 0 ? kVarFastDiv : 0u),
                        octet_waves(c.g));
    // uint8 -> fp32 rows at a width that is not a multiple of 512 px: the
    // straddle-capable variant (two-run staged stores, kVarStraddle)
    const bool straddle = c.in == Elem::kU8 && c.out == Elem::kF32 && c.builtin_t && c.g.tiles_x % 64u != 0u;
    const unsigned var = base | (fastdiv_ok ? quot_bits(c.qmode) : 0u) | (straddle ? kVarStraddle : 0u);
    const uint32_t sets = tile_waves(c.g);
    if (c.in == Elem::kU8 && c.out == Elem::kF32) {
        if ((sets + c.cus - 1u) / c.cus <= kBigWgSetsPerCU) return uncapped(Family::kTile, with_block<1024>(var), sets);
        return one_wave(Family::kTile, var | kF32OneWaveForm, kF32CapWavesPerCU, sets);
    }
    if (c.in == Elem::kU8 && c.out == Elem::kI8 && (var & kVarJpegQ) != 0u)
        return one_wave(Family::kTile, var, kI8CapWavesPerCU, sets);
    return uncapped(Family::kTile, var, sets);
}

// launch_fdct_frames: c.frames uint8 frames of c.g, quantised, built-in T
inline Choice forward_frames(const Call& c) {
    // the duo forward (round 6), as for one frame
    if (c.out == Elem::kF32 && c.qmode != 0 && duo_fwd_u8_fits(c)) return duo_fwd_u8(c);
    const bool straddle = c.out == Elem::kF32 && c.g.tiles_x % 64u != 0u;
    const unsigned var = prod_var(c.out) | quot_bits(c.qmode) | (straddle ? kVarStraddle : 0u);
    const uint32_t sets = tile_waves(c.g);
    if (c.out == Elem::kF32) {
        // the headline's residency cap when the whole list is a large grid
        const uint64_t per_cu = (static_cast<uint64_t>(sets) * c.frames + c.cus - 1u) / c.cus;
        if (per_cu > kFramesUncappedSetsPerCU)
            return one_wave(Family::kTile, var | kVarPacked,
                            per_cu <= kMidCapSetsPerCU ? kF32CapWavesPerCUMid : kF32CapWavesPerCU, sets, c.frames);
    }
    return uncapped(Family::kTile, var, sets, c.frames);
}

// The integer-input inverses (int8 plane, int16 blocks, colour) with the built-in T skip T's zero entries,
// which is bit-exact while no operand or partial sum of the two passes can overflow.  A table that fails that
// criterion (Call::full_chain, RgbCall::full_chain) takes this plain variant of the same kernel instead: every
// term kept, 256-thread workgroups, per-lane stores, neither LDS staging nor non-temporal stores.
constexpr unsigned kInvFullVar = with_block<256>(kVarFullChain);
// launch_idct: fp32 or int8 coefficients in, fp32 or uint8 pixels out
inline Choice inverse(const Call& c) {
    const bool f32 = c.in == Elem::kF32 && c.out == Elem::kF32;
    const unsigned wb = c.quant && c.wb_dequant ? kVarWbDequant : 0u;
    if (f32 && c.row_first) {  // cublasDCTv2 pass order: duo (rows first), or tile when forced
        if (c.mapping != HPDCT_MAPPING_TILE) return duo_f32(Family::kRowFirstDuo, kDuoVar, true, c);
        return uncapped(Family::kTile, prod_var(c.out) | kVarRowFirst | wb, tile_waves(c.g));
    }
    // fp32 coefficients -> fp32 or uint8 pixels: the duo kernel's 1 KiB row loads
    // (8192^2 -> uint8: 61.8 -> 56.7 us, profiles/r01/mappings/kbench2_inv_i8.log)
    const bool duo_in = c.in == Elem::kF32 && (f32 || c.out == Elem::kU8);
    const Family map = pick_mapping(c, duo_in);
    // int8 coefficients through a table that fails the skip criterion: the plain full-chain instantiation of
    // the mapping's kernel (256-thread workgroups, per-lane stores; its speed does not matter)
    if (c.full_chain && c.in == Elem::kI8 && c.quant && c.builtin_t) {
        if (map == Family::kOctet) return uncapped(Family::kOctet, kInvFullVar, octet_waves(c.g));
        return uncapped(Family::kTile, kInvFullVar, tile_waves(c.g));
    }
    if (map == Family::kDuo) {
        // uint8 output: 512-thread workgroups (56.7 vs 57.6 us with 256), never capped
        const unsigned dv = (c.out == Elem::kU8 ? with_block<512>(kDuoVar) : kDuoVar) | wb;
        return duo_f32(Family::kDuo, dv, f32, c);
    }
    if (map == Family::kOctet) return uncapped(Family::kOctet, oct_var(c.out) | (f32 ? wb : 0u), octet_waves(c.g));
    // int8 -> fp32 straddling sets: two-run staged stores (kVarStraddle)
    const bool straddle = c.in == Elem::kI8 && c.out == Elem::kF32 && c.builtin_t && c.g.tiles_x % 64u != 0u;
    return uncapped(Family::kTile, prod_var(c.out) | (f32 ? wb : 0u) | (straddle ? kVarStraddle : 0u),
                    tile_waves(c.g));
}

// JPEG-style int16 blocks (hpdct_blocks.hpp): the tile-per-lane mapping only
// (c.mapping is not read), the int8 kernels' shape: 256-thread workgroups,
// non-temporal stores, no residency cap.  Forward store path: the LDS-staged
// 1 KiB runs (kBlkStaged) against eight 16-B stores per lane at a 128-B stride,
// tools/kb_blocks A/B (DESIGN.md "int16 coefficient blocks").
constexpr unsigned kBlocksFwdStore = kBlkStaged;
constexpr unsigned kBlocksFwdVar = with_block<256>(kVarNT) | kBlocksFwdStore;
// launch_fdct_blocks: uint8 in, built-in T, level shift 128; c.g and c.qmode
inline Choice forward_blocks(const Call& c) {
    return uncapped(Family::kBlocks, kBlocksFwdVar | quot_bits(c.qmode), tile_waves(c.g));
}
// launch_idct_blocks: c.g and c.out (fp32 or uint8 pixels); fp32 rows
// LDS-re-staged, two-run staged stores for straddling sets (kVarStraddle)
constexpr unsigned blocks_inv_var(Elem out) {
    return with_block<256>(kVarNT) | (out == Elem::kF32 ? kVarLdsStore : 0u);
}
inline Choice inverse_blocks(const Call& c) {
    if (c.full_chain) return uncapped(Family::kBlocks, kInvFullVar, tile_waves(c.g));
    const bool straddle = c.out == Elem::kF32 && c.g.tiles_x % 64u != 0u;
    return uncapped(Family::kBlocks, blocks_inv_var(c.out) | (straddle ? kVarStraddle : 0u), tile_waves(c.g));
}

// Grey frames of any size and row pitch (hpdct_grey_frame.hpp): the blocks rows
// above over the PADDED tile grid, the same workgroup size, non-temporal stores
// and LDS-staged forward; hpdct_set_mapping is not read.
struct GreyCall {
    uint32_t tiles = 0;  // the padded tile grid's
    int qmode = 0;       // forward only
    // clip: the frame is not whole tiles, or its base or row pitch is not 8-byte
    // aligned (grey_whole_aligned is false): the same launch shape with kGreyClip,
    // the kernels' general instantiation.  A speed decision only: both
    // instantiations give a whole aligned frame the same bytes.
    bool clip = false;
    // inverse only: the table fails the skip criterion for int16 blocks (kVarFullChain)
    bool full_chain = false;
    // HPDCT_FRAME_DCT: the exact DCT's matrix (kFrameDct).  Rows of its own below: the launch shape and the clip
    // rule of the HpApprDCT row, never the per-position quotient forms (proven under HpApprDCT's bounds only;
    // qmode 2 runs as 1), and no full chain (the matrix has no zero to skip)
    bool dct = false;
};
constexpr uint32_t grey_waves(const GreyCall& c) { return c.tiles / 64u + (c.tiles % 64u != 0u); }
// the quotient bits under the exact DCT: IEEE division or the verified 3-op quotient
constexpr unsigned quot_bits_dct(int qmode) { return qmode != 0 ? kVarFastDiv : 0u; }
constexpr unsigned kGreyFwdVar = kBlocksFwdVar;
constexpr unsigned kGreyFwdDctVar = kGreyFwdVar | kFrameDct;
inline Choice forward_grey(const GreyCall& c) {
    if (c.dct)
        return uncapped(Family::kGrey, kGreyFwdDctVar | quot_bits_dct(c.qmode) | (c.clip ? kGreyClip : 0u),
                        grey_waves(c));
    return uncapped(Family::kGrey, kGreyFwdVar | quot_bits(c.qmode) | (c.clip ? kGreyClip : 0u), grey_waves(c));
}
// Inverse: uint8 pixels only; per-lane 8-byte row stores, as the blocks inverse to uint8
constexpr unsigned kGreyInvVar = blocks_inv_var(Elem::kU8);
constexpr unsigned kGreyInvDctVar = kGreyInvVar | kFrameDct;
inline Choice inverse_grey(const GreyCall& c) {
    // the exact DCT: whatever full_chain says
    if (c.dct) return uncapped(Family::kGrey, kGreyInvDctVar | (c.clip ? kGreyClip : 0u), grey_waves(c));
    // the full chain: one instantiation, the general one (kGreyClip takes whole aligned frames too)
    if (c.full_chain) return uncapped(Family::kGrey, kInvFullVar | kGreyClip, grey_waves(c));
    return uncapped(Family::kGrey, kGreyInvVar | (c.clip ? kGreyClip : 0u), grey_waves(c));
}

// Colour frames (hpdct_rgb.hpp): one lane per unit (an 8x8 pixel tile for
// 4:4:4, a 16x16 MCU for 4:2:0), 64 units per wave, 256-thread workgroups, no
// residency cap (their LDS image already holds a CU to 5 (4:4:4) or 2 (4:2:0)
// workgroups); hpdct_set_mapping is not read.
struct RgbCall {
    uint32_t units = 0;
    bool s420 = false;
    int qmode_luma = 0, qmode_chroma = 0;  // forward only; chroma 0 or 1
    // units counts the padded unit grid.  clip: the frame is not whole units, or
    // its base or row pitch is not 8-byte aligned (rgb_whole_aligned is false):
    // the same launch shape with kRgbClip, the kernels' general instantiation
    bool clip = false;
    // inverse only: a table fails the skip criterion for int16 blocks (kVarFullChain)
    bool full_chain = false;
    // HPDCT_FRAME_DCT (kFrameDct), as GreyCall::dct: rows of its own, qmode_luma 2 runs as 1, no full chain
    bool dct = false;
};
constexpr uint32_t rgb_waves(const RgbCall& c) { return c.units / 64u + (c.units % 64u != 0u); }
// Forward: block stores LDS-staged into 1 KiB runs (kBlkStaged, as the plane
// kernel's A/B chose), non-temporal.  Quotient pairs (luma, chroma) the launchers
// hold: (JPEG forms, 3-op), (3-op, 3-op), and IEEE division for both when
// either table is not all integers in 1..255 (every form gives the same result).
constexpr unsigned kRgbFwdVar = with_block<256>(kVarNT) | kBlkStaged;
constexpr unsigned kRgbFwdDctVar = kRgbFwdVar | kFrameDct;
constexpr unsigned kRgbInvDctVar = with_block<256>(0u) | kFrameDct;
inline Choice forward_rgb(const RgbCall& c) {
    const bool fast = c.qmode_luma != 0 && c.qmode_chroma != 0;
    if (c.dct)
        return uncapped(Family::kRgb,
                        kRgbFwdDctVar | (c.s420 ? kRgb420 : 0u) | (fast ? kVarFastDiv | kRgbChromaFastDiv : 0u) |
                            (c.clip ? kRgbClip : 0u),
                        rgb_waves(c));
    return uncapped(Family::kRgb,
                    kRgbFwdVar | (c.s420 ? kRgb420 : 0u) | (fast ? quot_bits(c.qmode_luma) | kRgbChromaFastDiv : 0u) |
                        (c.clip ? kRgbClip : 0u),
                    rgb_waves(c));
}
// Inverse: per-lane loads of whole blocks, plain per-lane RGB row stores
constexpr unsigned kRgbInvVar = with_block<256>(0u);
inline Choice inverse_rgb(const RgbCall& c) {
    // the exact DCT: whatever full_chain says
    if (c.dct)
        return uncapped(Family::kRgb, kRgbInvDctVar | (c.s420 ? kRgb420 : 0u) | (c.clip ? kRgbClip : 0u), rgb_waves(c));
    // the full chain: one instantiation per subsampling, the general one (kRgbClip takes whole aligned frames too)
    if (c.full_chain) return uncapped(Family::kRgb, kInvFullVar | kRgbClip | (c.s420 ? kRgb420 : 0u), rgb_waves(c));
    return uncapped(Family::kRgb, kRgbInvVar | (c.s420 ? kRgb420 : 0u) | (c.clip ? kRgbClip : 0u), rgb_waves(c));
}

// The entropy coder (hpdct_scan.hpp): its measure and emit launches run one
// wave per restart interval in one-wave workgroups, no residency cap (a wave
// holds 37,480 bytes of LDS: its tables 2,176, its staged blocks 8,448, its
// lanes' own words 13,568 and its bit buffer 13,288); beyond
// kScanMaxWgs intervals a workgroup takes every kScanMaxWgs-th one.  The
// offsets launch is one 1024-thread workgroup.  hpdct_set_mapping is not read.
// Under the caller's tables (tables: scan_code_tables_kernel) the same launches,
// a wave's lanes' words 14,080 and its bit buffer 13,328 bytes (a block of 1665 bits).
struct ScanCall {
    uint32_t intervals = 1;
    bool natural = false;
    bool tables = false;
};
constexpr uint32_t kScanMaxWgs = 1u << 20;
inline Choice scan_code(const ScanCall& c, bool emit) {
    return {Family::kScan,
            with_block<64>((c.natural ? kScanNatural : 0u) | (emit ? kScanEmit : 0u) | (c.tables ? kScanTables : 0u)),
            64u, 0u, c.intervals < kScanMaxWgs ? c.intervals : kScanMaxWgs, 1u};
}
inline Choice scan_offsets() { return {Family::kScan, with_block<1024>(kScanOffsets), 1024u, 0u, 1u, 1u}; }
// The statistics pass (hpdct_scan_hist.hpp): one lane per block in 256-thread
// workgroups, a grid-stride loop under a cap of kScanHistMaxWgs workgroups (8
// per CU of 256), so that the 1024-bin flush of a workgroup is paid once per
// 256 blocks at most.  It does not read restart_interval beyond the DC predecessor.
constexpr uint32_t kScanHistMaxWgs = 2048;
inline Choice scan_hist(uint64_t blocks, bool natural) {
    const uint64_t wgs = (blocks + 255u) / 256u;
    return {Family::kScan, with_block<256>(kScanHist | (natural ? kScanNatural : 0u)), 256u, 0u,
            wgs < kScanHistMaxWgs ? static_cast<uint32_t>(wgs < 1u ? 1u : wgs) : kScanHistMaxWgs, 1u};
}

// The entropy decoder (hpdct_unscan.hpp).  Huffman decoding is serial inside a
// restart interval: one LANE walks one interval, in one-wave workgroups (the
// tables and a lane's block row are 3,488 bytes of LDS with one lane, 11,792
// with 64).  A lane's walk is a chain of dependent instructions, and lanes of
// one wave that sit in different branches of the walk run one after the other,
// so few lanes per wave are fastest while every wave is resident at once (the
// device holds 256 CUs x 32 = kUnscanMaxWgs one-wave workgroups), and many
// lanes per wave once the waves would queue.  Measured at 8192^2 grey, noise /
// smooth, offsets given, us (tools/unscan_probe.py against builds with the rows
// moved, profiles/r11/unscan_policy_ab.log):
//    16,384 intervals:  1 lane 8,109 / 446   4 lanes 2,878 / 209   16 lanes 3,299 / 204
//    32,768:            4 lanes 2,549 / 169  16 lanes 1,588 / 105
//    65,536:           16 lanes   954 / 69   64 lanes 1,113 / 69
//   131,072:            4 lanes 2,568 / 156  16 lanes   834 / 65   64 lanes 578 / 58
// Hence 1 lane up to kUnscanMaxWgs intervals (an 8192^2 frame at one MCU row
// per interval has 1,024), 4 up to 16,384, 16 up to 65,536, all 64 beyond;
// beyond 64 * kUnscanMaxWgs intervals a workgroup takes every kUnscanMaxWgs-th
// group of 64.  The marker search runs one wave per 4096-byte chunk in
// 256-thread workgroups under the same grid cap, its ranks in one 1024-thread
// workgroup.  hpdct_set_mapping is not read.
struct UnscanCall {
    uint32_t intervals = 1;
    bool natural = false;
    bool tables = false;  // unscan_decode_tables_kernel: the caller's tables (3,648 bytes of LDS instead of 3,280)
};
constexpr uint32_t kUnscanMaxWgs = 8192;
constexpr uint32_t kUnscanChunkBytes = 4096;
constexpr uint32_t kUnscanLanes4Max = 16384, kUnscanLanes16Max = 65536;
constexpr uint32_t unscan_lanes(uint32_t intervals) {
    return intervals <= kUnscanMaxWgs ? 1u : intervals <= kUnscanLanes4Max ? 4u : intervals <= kUnscanLanes16Max ? 16u : 64u;
}
inline Choice unscan_decode(const UnscanCall& c) {
    const uint32_t lanes = unscan_lanes(c.intervals);
    const uint32_t wgs = c.intervals / lanes + (c.intervals % lanes != 0u);
    const unsigned bit = lanes == 16u ? kUnscanLanes16 : lanes == 4u ? kUnscanLanes4 : lanes == 1u ? kUnscanLanes1 : 0u;
    return {Family::kUnscan, with_block<64>((c.natural ? kScanNatural : 0u) | bit | (c.tables ? kScanTables : 0u)), 64u,
            0u, wgs < kUnscanMaxWgs ? wgs : kUnscanMaxWgs, 1u};
}
// chunks: ceil(scan bytes / kUnscanChunkBytes), at least 1
inline Choice unscan_locate(uint64_t chunks, bool place) {
    const uint64_t wgs = (chunks + 3u) / 4u;
    return {Family::kUnscan, with_block<256>(kUnscanCount | (place ? kUnscanPlace : 0u)), 256u, 0u,
            wgs < kUnscanMaxWgs ? static_cast<uint32_t>(wgs) : kUnscanMaxWgs, 1u};
}
inline Choice unscan_rank() { return {Family::kUnscan, with_block<1024>(kUnscanRank), 1024u, 0u, 1u, 1u}; }

// The split entropy decoder (hpdct_unscan_split.hpp): a lane walks a SEGMENT of
// kUnsplitSegBytes bytes, a workgroup of kUnsplitGroup lanes a group of as many
// consecutive segments of one interval, and kUnsplitRounds launches after the
// first carry a changed exit from one group to the next.  A segment must hold
// several block ends for the walks to fall into step (a block of noise at the
// default table is some 50 bytes), and a CPU simulation needed 1-4 rounds of
// neighbour exchange at 256 bytes for all but scans without a single EOB; those
// rounds run inside a group, in LDS, so a launch between groups is needed only
// where a wrong exit crosses a group's end.  The settle and write kernels keep
// the tables and a state per lane in LDS (10.5 KiB a workgroup), no block row.
// An interval of at most (kUnsplitRounds + 1) groups, 320 KiB, always settles;
// a longer one that does not is walked by one lane, as every interval shorter
// than kUnsplitMinBytes is.  The threshold, measured at 8192^2 with every
// interval split against hpdct_decode_scan on the same scans, offsets given, us
// (tools/unscan_split_probe.py, profiles/r12/unscan_split_probe.log and
// unscan_split_threshold.log; the two passes differ by under 1 %):
//   bytes an interval (intervals)      serial     split
//        220  (131,072) grey noise        578    34,868
//        875   (32,768) grey noise      1,584    20,963
//      1,749   (16,384) grey noise      2,869    12,607
//      2,172      (512) 4:2:0 smooth    4,088     2,985
//      3,496    (8,192) grey noise      8,053     7,247
//      6,718    (4,096) 4:2:0 noise     8,885     7,238
//      6,990    (4,096) grey noise      9,250     4,948
//     13,978    (2,048) grey noise     16,571     3,861
//     27,954    (1,024) grey noise     35,671     2,963    (one MCU row)
//     53,734      (512) 4:2:0 noise    57,979     4,696    (one MCU row)
//    891,110        (1) 1080p noise   780,994     2,600    (no restart markers)
// A group holds one interval's segments only, so thousands of short intervals
// run workgroups of a few lanes each, and the chain costs 2 ms at 8192^2 whatever
// it decodes (the clear of 128 MiB of blocks, eleven launches).  3,496 bytes is
// the shortest interval at which the split call won with thousands of intervals;
// the threshold is the 13 segments below it.  (At 2,172 bytes it won with 512.)
constexpr uint32_t kUnsplitSegBytes = 256, kUnsplitGroup = 256, kUnsplitRounds = 4;
constexpr uint64_t kUnsplitMinBytes = 3328;
constexpr uint32_t kUnsplitMaxWgs = 1u << 16;  // beyond: a workgroup takes every kUnsplitMaxWgs-th group
inline Choice unsplit_plan() { return {Family::kUnsplit, with_block<1024>(kUnsplitPlan), 1024u, 0u, 1u, 1u}; }
// groups: the budget of groups (every one may be in use)
inline Choice unsplit_groups(uint64_t groups, unsigned kind, bool natural) {
    return {Family::kUnsplit, with_block<256>(kind | (natural ? kScanNatural : 0u)), 256u, 0u,
            groups < kUnsplitMaxWgs ? static_cast<uint32_t>(groups < 1u ? 1u : groups) : kUnsplitMaxWgs, 1u};
}
// tables: the kernels that stage the caller's tables (unsplit_*_tables_kernel), the same launches
inline Choice unsplit_settle(uint64_t groups, bool tables = false) {
    return unsplit_groups(groups, kUnsplitSettle | (tables ? kScanTables : 0u), false);
}
inline Choice unsplit_write(uint64_t groups, bool natural, bool tables = false) {
    return unsplit_groups(groups, kUnsplitWrite | (tables ? kScanTables : 0u), natural);
}
// one workgroup per interval
inline Choice unsplit_offsets(uint32_t intervals) { return unsplit_groups(intervals, kUnsplitOffsets, false); }
// units: 16-byte pieces of all the frame's blocks, one per lane
inline Choice unsplit_clear(uint64_t units) { return unsplit_groups((units + 255u) / 256u, kUnsplitClear, false); }
// the serial pass: the parent's decode launch for this interval count
inline Choice unsplit_serial(const UnscanCall& c) {
    Choice ch = unscan_decode(c);
    ch.family = Family::kUnsplit, ch.var |= kUnsplitSerial;
    return ch;
}

// launch_roundtrip.  The two-lanes-per-tile round trip (hpdct_rt_duo.hpp) for
// the verified quotient (qmode 1 or 2) with any reconstruction, when its sums
// (if any) have a spread slot, the width is a multiple of 256 pixels (whole
// 32-tile runs per wave) and the mapping is not forced to "tile"; 8192^2
// with sums and a uint8 reconstruction 74.3-74.8 us against 78.4 for the
// tile kernel with the same sums path, without sums 67.0 against 76.8
// (tools/kb_rt, profiles/r05/f/).  Otherwise the tile-per-lane kernel (IEEE
// division, ragged widths, forced tile mapping, widths from 2^22 pixels).
inline Choice roundtrip(const RtCall& c) {
    const unsigned q = quot_bits(c.qmode);
    if (c.qmode != 0 && (!c.sums || c.slot) && duo_u8_runs(c.g) && c.mapping != HPDCT_MAPPING_TILE) {
        // neither a reconstruction nor sums: the forward alone, capped
        if (c.recon == kRtReconNone && !c.sums)
            return {Family::kDuoFwdU8, q, kDuoFwdBlock, kDuoFwdCapWgs, wgs_for(duo_waves(c.g), kDuoFwdBlock), 1u};
        return {Family::kRtDuo, q, kDuoRtBlock, c.recon == kRtReconF32 || !c.sums ? kDuoRtCapWgs : 0u,
                wgs_for(duo_waves(c.g), kDuoRtBlock), 1u};
    }
    // straddling sets: two-run staged stores (the verified quotient's kernels)
    const bool straddle = c.qmode != 0 && c.g.tiles_x % 64u != 0u;
    return {Family::kRtTile, q | (straddle ? kVarStraddle : 0u), kRtBlock, 0u, wgs_for(tile_waves(c.g), kRtBlock), 1u};
}

// Runtime -> compile time: f gets a std::integral_constant of the quotient
// bits, one variant bit or the workgroup size (kOk false: no such kernel, 0).
template <bool kOk, typename F>
auto with_quotient(unsigned var, F&& f) {
    if constexpr (kOk) {
        if ((var & kVarJpegQ) != 0u) return f(std::integral_constant<unsigned, kVarFastDiv | kVarJpegQ>{});
        if ((var & kVarFastDiv) != 0u) return f(std::integral_constant<unsigned, kVarFastDiv>{});
    }
    return f(std::integral_constant<unsigned, 0u>{});
}
constexpr int qmode_of(unsigned bits) { return (bits & kVarJpegQ) != 0u ? 2 : (bits & kVarFastDiv) != 0u ? 1 : 0; }
template <unsigned kBit, bool kOk, typename F>
auto with_bit(unsigned var, F&& f) {
    if constexpr (kOk)
        if ((var & kBit) != 0u) return f(std::integral_constant<unsigned, kBit>{});
    return f(std::integral_constant<unsigned, 0u>{});
}
template <uint32_t kA, uint32_t kB, typename F>
auto with_block_size(uint32_t block, F&& f) {
    if constexpr (kA != kB)
        if (block == kA) return f(std::integral_constant<uint32_t, kA>{});
    return f(std::integral_constant<uint32_t, kB>{});
}

}  // namespace policy
}  // namespace hpdct
