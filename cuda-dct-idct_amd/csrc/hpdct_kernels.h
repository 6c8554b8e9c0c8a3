// hpdct_kernels.h -- host-visible declarations of the gfx950 kernels
// (launchers are explicit template instantiations in hpdct_fwd_*.hip /
// hpdct_inv.hip; the kernels themselves are in hpdct_kernels_impl.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace hpdct {

constexpr uint32_t kBlockThreads = 256;  // 4 wave64 per workgroup

// Compile-time kernel variants (bit flags) of the product kernels.  Bits not
// listed here are the tools' A/B variants (tools/kbench_variants.hpp).
enum : unsigned {
    kVarFastDiv = 1u,  // quotient by  q0=c*r; e=fma(-q0,Q,c); q=fma(e,r,q0)  (r = RN(1/Q)).  Gives the same
                       // roundf() as IEEE c/Q for every |c| <= 4096 and every integer Q in 1..255
                       // (exhaustive: tests/tools/verify_fastdiv.*); enabled unconditionally only for such
                       // tables with uint8 input and the built-in T (|C| <= 1024); fp32 input with such a
                       // table takes it per output row under kVarFastDivChecked.
    kVarLdsStore = 8u, // fp32 rows re-staged through LDS so every store instruction writes 1 KiB contiguous
    kVarNT = 16u,      // non-temporal (streaming) stores for the output planes
    // bits 12..13: workgroup size: 0 -> 256 threads, 1 -> 64, 2 -> 512, 3 -> 1024
    kVarRowFirst = 1u << 14,  // cublasDCTv2 pass order (row pass first), fp32 compat path
    kVarWbDequant = 1u << 15, // inverse: write q*Q back into the fp32 coefficient input
                              // (in-place multiply_matrices of main_cublass_2.cu:285)
    kVarFastDivChecked = 1u << 26,  // fp32 input (any T), integer table in 1..255: the 3-op quotient for an
                                    // output row when every lane's 8 values have |C| <= 4096 (wave-uniform
                                    // test, NaN/inf fail it), IEEE division otherwise: exact either way
                                    // (verify_fastdiv covers every |C| <= 4096)
    kVarPacked = 1u << 19,    // uint8 -> fp32 or int8 quantised, built-in T: packed-fp32 transform and
                              // quotient (fdct_tile_pk; fp32: 844 instead of 1,308 VALU instructions per set)
    kVarI8Pack = 1u << 17,    // int8 output: round-half-away folded into the truncating cvt, and each
                              // coefficient converted straight into its byte (SDWA dst_sel, one op)
    kVarJpegQ = 1u << 11,     // the DEFAULT JPEG table, uint8 input, built-in T, level shift 128 (with
                              // kVarFastDiv): per position the 3-op form F or H where it is proven exact
                              // below that position's |C| bound, the 6-op form elsewhere
                              // (hpdct_quant_forms.h, tests/tools/verify_quant_pos.c)
    kVarHoistRun = 1u << 20,  // packed u8 -> fp32 forward (the capped headline kernel): the whole-run test
                              // (split == 64) taken once per set, two straight-line copies of the body, and in
                              // the whole-run copy each row's re-staged stores issued one row later, after the
                              // next row's LDS writes (tools/kbench3 group hoist: 56.5 against 57.4-57.7 us)
    kVarStraddle = 1u << 30,  // fp32 LDS-staged rows: a 64-tile set that straddles two tile rows (width not a
                              // multiple of 512 px) stores two contiguous runs per instruction instead of
                              // 32 B per lane; launched only for such widths (the branch costs the
                              // power-of-two frames ~3 %, profiles/r01/ab_straddle.log)
    kVarFullChain = 1u << 27, // integer-input inverses with the built-in T (int8 plane, int16 blocks, colour):
                              // every term of T kept, zero entries too.  For a table so large that q * Q or
                              // a partial sum may overflow (skip_zero_exact of hpdct_api.cpp fails): 0 * inf = NaN
                              // as in the reference.  Clear: the zero terms are skipped.  (The tools use
                              // this bit for a forward-only diagnostic of their own kernels.)
};
// the octet kernels' own variant bit (hpdct_octet.hpp)
enum : unsigned {
    kOctRestage = 1u << 20,  // octet output rows re-staged through LDS: each store instruction writes
                             // four 256-B runs (a whole row of the wave's 8 tiles each) instead of
                             // 16-B pieces at a 32-B stride
};
// the block-format kernels' own variant bit (hpdct_blocks.hpp)
enum : unsigned {
    kBlkStaged = 1u << 21,  // forward: a whole 64-tile set's 8 KiB of int16 blocks re-staged through LDS, so
                            // each store instruction writes 1 KiB contiguous instead of 16 B per lane at a
                            // 128-B stride (tools/kb_blocks A/B)
};
// the colour kernels' own variant bits (hpdct_rgb.hpp; they also read kBlkStaged)
enum : unsigned {
    kRgb420 = 1u << 22,            // 4:2:0: one lane per 16x16 MCU (clear: 4:4:4, one lane per 8x8 pixel tile)
    kRgbChromaFastDiv = 1u << 23,  // forward: the verified 3-op quotient for Cb and Cr (the chroma table's
                                   // entries are all integers in 1..255); the luma quotient is in the
                                   // kVarFastDiv / kVarJpegQ bits as everywhere
    kRgbClip = 1u << 24,           // the general instantiation: a frame that is not whole units (edge-replicated
                                   // on the way in, cropped on the way out) or whose base or row pitch is not
                                   // 8-byte aligned; clear: whole units, 8-byte loads and stores everywhere
};
// the frame kernels' own variant bit (hpdct_grey_frame.hpp and the colour kernels of hpdct_rgb.hpp)
enum : unsigned {
    kFrameDct = 1u << 18,  // HPDCT_FRAME_DCT: the built-in matrix is the exact DCT's (tables::kTDct, every term:
                           // it has no zero, so kVarFullChain means nothing), and the inverse rounds its pixels
                           // (R + 128.5f, clamp, truncate).  Never with kVarJpegQ: the per-position forms are
                           // proven under HpApprDCT's bounds only.  Instantiated in the hpdct_dct_*.hip units
};
// the entropy coder's own variant bits (hpdct_scan.hpp)
enum : unsigned {
    kScanNatural = 1u << 25,  // the blocks are row-major inside (HPDCT_BLOCKS_NATURAL): permuted on load
    kScanEmit = 1u << 28,     // scan_code_kernel: the emit launch (clear: the measure launch)
    kScanOffsets = 1u << 29,  // scan_offsets_kernel
    kScanTables = 1u << 27,   // scan_code_tables_kernel, unscan_decode_tables_kernel: the caller's Huffman tables
                              // (a HuffBlob in device memory) instead of Annex K's
    kScanHist = 1u << 30,     // scan_hist_kernel (hpdct_scan_hist.hpp)
};
// the entropy decoder's own variant bits (hpdct_unscan.hpp; its decode kernel also reads kScanNatural:
// permuted on store)
enum : unsigned {
    kUnscanLanes16 = 1u << 20,  // unscan_decode_kernel: 16, 4 or 1 lanes of each wave take an interval
    kUnscanLanes4 = 1u << 21,   // (none of the three: all 64)
    kUnscanLanes1 = 1u << 22,
    kUnscanCount = 1u << 23,    // unscan_locate_kernel: the counting pass (with kUnscanPlace: the placing pass)
    kUnscanPlace = 1u << 24,
    kUnscanRank = 1u << 28,     // unscan_rank_kernel
};
constexpr uint32_t unscan_lanes_of(unsigned var) {
    return (var & kUnscanLanes16) ? 16u : (var & kUnscanLanes4) ? 4u : (var & kUnscanLanes1) ? 1u : 64u;
}
// Runtime -> compile time, as policy::with_bit: f gets var's kUnscanLanes* bit (0: all 64 lanes) as a
// std::integral_constant.  The serial decoder and the split decoder's serial launch pick their kernel through it.
template <typename F>
auto with_lanes(unsigned var, F&& f) {
    switch (unscan_lanes_of(var)) {
        case 1u: return f(std::integral_constant<unsigned, kUnscanLanes1>{});
        case 4u: return f(std::integral_constant<unsigned, kUnscanLanes4>{});
        case 16u: return f(std::integral_constant<unsigned, kUnscanLanes16>{});
        default: return f(std::integral_constant<unsigned, 0u>{});
    }
}
// the split entropy decoder's kernels (hpdct_unscan_split.hpp): which one, in bits 29..31; its serial kernel also
// reads the kUnscanLanes* bits, its write and serial kernels kScanNatural
enum : unsigned {
    kUnsplitPlan = 1u << 29,
    kUnsplitSettle = 2u << 29,
    kUnsplitOffsets = 3u << 29,
    kUnsplitClear = 4u << 29,
    kUnsplitWrite = 5u << 29,
    kUnsplitSerial = 6u << 29,
};
// Bits only the product kernels give a meaning to: the tools' A/B variant
// bits must stay clear of them (static_assert in tools/kbench_variants.hpp).
constexpr unsigned kProductOnlyVarBits = kVarFastDivChecked | kVarJpegQ;
constexpr uint32_t block_of(unsigned var) {
    return ((var >> 12) & 3u) == 1u ? 64u : ((var >> 12) & 3u) == 2u ? 512u : ((var >> 12) & 3u) == 3u ? 1024u : kBlockThreads;
}
template <unsigned kVar>
constexpr uint32_t kBlock = block_of(kVar);
// kV with its workgroup-size bits set for kThreads threads
template <uint32_t kThreads>
constexpr unsigned with_block(unsigned kV) {
    static_assert(kThreads == 64 || kThreads == 256 || kThreads == 512 || kThreads == 1024, "workgroup size");
    return (kV & ~(3u << 12)) | ((kThreads == 64 ? 1u : kThreads == 512 ? 2u : kThreads == 1024 ? 3u : 0u) << 12);
}

// 64 floats passed by value as a kernel argument (lands in SGPRs)
struct Mat64 {
    float v[64];
};

// Quantiser parameters passed by value: Q and RN(1/Q) (the latter is used
// only by the verified fast quotient).
struct QParams {
    Mat64 q;
    Mat64 r;
};

namespace policy { struct Choice; }  // what a call launches (hpdct_policy.hpp)

// Tile geometry of one launch: ntiles = (height/8) * (width/8) < 2^32.
struct TileGrid {
    uint32_t ntiles;
    uint32_t tiles_x;
    uint64_t width;  // elements per image row
};

// qmode (the quotient): 0 IEEE division; 1 the 3-operation quotient (only
// legal for a table whose entries are all integers in 1..255 with uint8 input
// and the built-in T, or fp32 input behind the duo kernels' range check; the
// caller checks); 2 as 1 plus the default JPEG table's per-position 3-op forms
// (hpdct_quant_forms.h: only the default table, uint8 input, built-in T,
// shift 128).  shift is 128 (reference level shift) or 0.
// row_first: cublasDCTv2 pass order (fp32 -> fp32 only).
template <typename TIn, typename TOut, bool kQuant, bool kBuiltinT, bool kWriteback>
hipError_t launch_fdct(const TIn* img, TOut* out, float* shifted, const TileGrid& g, const float* t_dev,
                       const QParams& q, float shift, int qmode, bool row_first, hipStream_t s);

// dq_out (fp32 -> fp32 with dequantisation only, else nullptr): q*Q is also
// written there (the in-place multiply of the cublasDCTv2 inverse).
// full_chain: q fails the skip criterion for int8 coefficients (read for int8
// input dequantised with the built-in T only: the kVarFullChain kernels).
template <typename TIn, typename TOut, bool kDequant, bool kBuiltinT>
hipError_t launch_idct(const TIn* coef, TOut* out, float* dq_out, const TileGrid& g, const float* t_dev,
                       const Mat64& q, float shift, bool row_first, bool full_chain, hipStream_t s);

// Round trip (hpdct_roundtrip.hpp): uint8 frame -> fp32 quantised
// coefficients + optional reconstruction + optional quality sums, built-in T.
// Device accumulators, the layout of hpdct_roundtrip_sums (include/hpdct.h).
struct RtSums {
    unsigned long long sse_f32_fx;  // sum (x - (R+128))^2 * 2^16, per-tile fp32 sums rounded
    unsigned long long sse_u8;      // sum (x - u8(R+128))^2, exact
    unsigned long long sum_x2;      // sum x^2, exact
};
enum : int { kRtReconNone = 0, kRtReconU8 = 1, kRtReconF32 = 2 };
// fast: integer table in 1..255 with int8-range quotients (verified quotient);
// sums may be nullptr (no statistics), recon nullptr with kRtReconNone.
// zero_sums: the launch overwrites *sums, else adds to it.  The kernel adds
// into a library spread slot kept per sums pointer and a one-wave kernel folds
// it into *sums (a memset of *sums and the tile kernel when no slot can be had).
hipError_t launch_roundtrip(const uint8_t* img, float* coef, void* recon, int recon_kind, RtSums* sums,
                            const TileGrid& g, const QParams& qp, int fast, bool zero_sums, hipStream_t s);
// The pieces launch_roundtrip (hpdct_roundtrip.hip) launches as policy::roundtrip chose (c):
//  - the tile-per-lane kernels, one unit per reconstruction kind
//    (hpdct_rt_tile_{u8,f32,none}.hip); sums: the struct (or spread
//    sub-slot 0) the workgroups add into, or nullptr;
//  - the two-lanes-per-tile kernel (hpdct_rt_duo.hip): the verified quotient, a
//    uint8 reconstruction (recon) or none (nullptr); spread: a zeroed spread slot
//    (kRtSpread sub-slots, hpdct_roundtrip.hpp) the waves add into, or
//    nullptr for no sums;
//  - the finish kernel folding a spread slot into *dst (overwrite, or add
//    when accumulate) and zeroing it.
hipError_t launch_rt_tile_u8(const uint8_t* img, float* coef, void* recon, RtSums* sums, const TileGrid& g,
                             const QParams& qp, const policy::Choice& c, hipStream_t s);
hipError_t launch_rt_tile_f32(const uint8_t* img, float* coef, void* recon, RtSums* sums, const TileGrid& g,
                              const QParams& qp, const policy::Choice& c, hipStream_t s);
hipError_t launch_rt_tile_none(const uint8_t* img, float* coef, void* recon, RtSums* sums, const TileGrid& g,
                               const QParams& qp, const policy::Choice& c, hipStream_t s);
hipError_t launch_rt_duo(const uint8_t* img, float* coef, void* recon, int recon_kind, unsigned long long* spread,
                         const TileGrid& g, const QParams& qp, const policy::Choice& c, hipStream_t s);
hipError_t launch_rt_duo_f32(const uint8_t* img, float* coef, void* recon, unsigned long long* spread,
                             const TileGrid& g, const QParams& qp, const policy::Choice& c, hipStream_t s);
hipError_t launch_rt_finish(RtSums* dst, unsigned long long* spread, bool accumulate, hipStream_t s);
// the spread slot of a sums pointer back to its device's free list
// (hpdct_roundtrip_release_sums); false when the pointer had none
bool release_sums_slot(const void* sums);

// uint8 -> quantised fp32 forward on the two-lanes-per-tile mapping (round 6;
// fdct_duo_u8_kernel, hpdct_rt_duo.hpp), as policy::forward chose it (c):
// built-in T, level shift 128, tiles_x a multiple of 32, width below 2^22 px.
hipError_t launch_fdct_duo_u8(const uint8_t* img, float* coef, const TileGrid& g, const QParams& qp,
                              const policy::Choice& c, hipStream_t s);

// A list of frames per launch (hpdct_forward_frames): up to kMaxFramesPerLaunch
// device pointer pairs travel in the kernel arguments (1 KiB).
constexpr int kMaxFramesPerLaunch = 64;
template <typename TOut>
struct FrameTable {
    const uint8_t* in[kMaxFramesPerLaunch];
    TOut* out[kMaxFramesPerLaunch];
};
// n <= kMaxFramesPerLaunch frames of grid g, uint8 -> TOut (float or int8_t),
// built-in T, quantised with q (qmode as launch_fdct).
template <typename TOut>
hipError_t launch_fdct_frames(const FrameTable<TOut>& ft, int n, const TileGrid& g, const QParams& q, int qmode,
                              hipStream_t s);
// the duo forward over such a list (fp32 out; c.grid_y frames)
hipError_t launch_fdct_duo_u8_frames(const FrameTable<float>& ft, const TileGrid& g, const QParams& qp,
                                     const policy::Choice& c, hipStream_t s);

// JPEG-style int16 coefficient blocks (hpdct_blocks.hpp): block t = tile t in
// row-major tile order, 64 int16 each, zig-zag or (natural) row-major inside.
// Tile-per-lane kernels only, as policy::forward_blocks / inverse_blocks choose.
// Forward: uint8 frame, built-in T, level shift 128, quantised with qp (qmode
// as launch_fdct; the caller proved |q| <= 32767).
hipError_t launch_fdct_blocks(const uint8_t* img, int16_t* blocks, const TileGrid& g, const QParams& qp, int qmode,
                              bool natural, hipStream_t s);
// Inverse: blocks -> fp32 pixels (R + 128, no clamp; out_f32) or uint8 (clamp + truncate).
// full_chain: q fails the skip criterion for int16 coefficients (the kVarFullChain kernel)
hipError_t launch_idct_blocks(const int16_t* blocks, void* out, bool out_f32, const TileGrid& g, const Mat64& q,
                              bool natural, bool full_chain, hipStream_t s);

// Colour frames (hpdct_rgb.hpp): interleaved uint8 RGB <-> three int16 block
// arrays (Y, Cb, Cr), 4:4:4 or 4:2:0, one launch per direction.  A lane owns
// one unit: an 8x8 pixel tile (4:4:4) or a 16x16 MCU (4:2:0), 64 units in
// row-major unit order per wave.  nunits < 2^32.  The unit grid covers the
// padded frame (height and width rounded up to whole units); the kernels
// without kRgbClip read nunits, units_x and pitch only.
struct RgbGrid {
    uint32_t nunits;
    uint32_t units_x;  // units per row of units
    uint64_t pitch;    // bytes from one image row to the next (>= 3 * width)
    uint64_t height;   // the frame's own rows and pixels per row
    uint64_t width;
};
// whole units, base and pitch 8-byte aligned: the kernels without kRgbClip
inline bool rgb_whole_aligned(const void* rgb, const RgbGrid& g, bool s420) {
    const uint64_t side = s420 ? 16u : 8u;
    return g.height % side == 0u && g.width % side == 0u && g.pitch % 8u == 0u &&
           reinterpret_cast<uintptr_t>(rgb) % 8u == 0u;
}
// Forward: built-in T, level shift 128; Y quantised with ql, Cb and Cr with qc
// (qmode_* as launch_fdct; the caller proved |q| <= 32767 for both tables).
hipError_t launch_fdct_rgb(const uint8_t* rgb, int16_t* y, int16_t* cb, int16_t* cr, const RgbGrid& g, bool s420,
                           const QParams& ql, const QParams& qc, int qmode_luma, int qmode_chroma, bool natural,
                           hipStream_t s);
// Inverse: blocks -> uint8 components (clamp + truncate) -> RGB.  full_chain: ql or qc fails the skip
// criterion for int16 coefficients (the kVarFullChain kernels)
hipError_t launch_idct_rgb(const int16_t* y, const int16_t* cb, const int16_t* cr, uint8_t* rgb, const RgbGrid& g,
                           bool s420, const Mat64& ql, const Mat64& qc, bool natural, bool full_chain,
                           hipStream_t s);
// the per-subsampling units of the forward (hpdct_rgb_fwd420.hip / hpdct_rgb_fwd444.hip), as c chose
hipError_t launch_fdct_rgb_420(const uint8_t* rgb, int16_t* y, int16_t* cb, int16_t* cr, const RgbGrid& g,
                               const QParams& ql, const QParams& qc, bool natural, const policy::Choice& c,
                               hipStream_t s);
hipError_t launch_fdct_rgb_444(const uint8_t* rgb, int16_t* y, int16_t* cb, int16_t* cr, const RgbGrid& g,
                               const QParams& ql, const QParams& qc, bool natural, const policy::Choice& c,
                               hipStream_t s);
// the same with kRgbClip (hpdct_rgb_fwd420_clip.hip / hpdct_rgb_fwd444_clip.hip)
hipError_t launch_fdct_rgb_420_clip(const uint8_t* rgb, int16_t* y, int16_t* cb, int16_t* cr, const RgbGrid& g,
                                    const QParams& ql, const QParams& qc, bool natural, const policy::Choice& c,
                                    hipStream_t s);
hipError_t launch_fdct_rgb_444_clip(const uint8_t* rgb, int16_t* y, int16_t* cb, int16_t* cr, const RgbGrid& g,
                                    const QParams& ql, const QParams& qc, bool natural, const policy::Choice& c,
                                    hipStream_t s);

// The same two calls under HPDCT_FRAME_DCT (kFrameDct; hpdct_dct_rgb_fwd420.hip, hpdct_dct_rgb_fwd444.hip,
// hpdct_dct_rgb_inv.hip): the exact DCT's matrix, the inverse's pixels rounded.  qmode_* 0 or 1 (a 2 is
// taken as 1: no per-position forms); the inverse has no full_chain, it keeps every term anyway.
hipError_t launch_fdct_rgb_dct(const uint8_t* rgb, int16_t* y, int16_t* cb, int16_t* cr, const RgbGrid& g, bool s420,
                               const QParams& ql, const QParams& qc, int qmode_luma, int qmode_chroma, bool natural,
                               hipStream_t s);
hipError_t launch_fdct_rgb_dct_420(const uint8_t* rgb, int16_t* y, int16_t* cb, int16_t* cr, const RgbGrid& g,
                                   const QParams& ql, const QParams& qc, bool natural, const policy::Choice& c,
                                   hipStream_t s);
hipError_t launch_fdct_rgb_dct_444(const uint8_t* rgb, int16_t* y, int16_t* cb, int16_t* cr, const RgbGrid& g,
                                   const QParams& ql, const QParams& qc, bool natural, const policy::Choice& c,
                                   hipStream_t s);
// the same with kRgbClip (hpdct_dct_rgb_fwd420_clip.hip / hpdct_dct_rgb_fwd444_clip.hip)
hipError_t launch_fdct_rgb_dct_420_clip(const uint8_t* rgb, int16_t* y, int16_t* cb, int16_t* cr, const RgbGrid& g,
                                        const QParams& ql, const QParams& qc, bool natural, const policy::Choice& c,
                                        hipStream_t s);
hipError_t launch_fdct_rgb_dct_444_clip(const uint8_t* rgb, int16_t* y, int16_t* cb, int16_t* cr, const RgbGrid& g,
                                        const QParams& ql, const QParams& qc, bool natural, const policy::Choice& c,
                                        hipStream_t s);
hipError_t launch_idct_rgb_dct(const int16_t* y, const int16_t* cb, const int16_t* cr, uint8_t* rgb, const RgbGrid& g,
                               bool s420, const Mat64& ql, const Mat64& qc, bool natural, hipStream_t s);

hipError_t launch_fill_hash(uint8_t* out, uint64_t n, uint64_t seed, uint64_t first, hipStream_t s);

// int8 wire coefficients -> fp32 plane (hpdct_decode.hip)
hipError_t launch_decode_i8_f32(const int8_t* in, float* out, uint64_t n, hipStream_t s);

// hpdct_floor_probe (hpdct_probe.hip): kind 0 an empty kernel, 1 a u8 -> fp32
// copy, both on the grid the uint8 -> fp32 forward of g launches
hipError_t launch_floor_probe(int kind, const uint8_t* in, float* out, const TileGrid& g, hipStream_t s);
// hpdct_copy_ceiling (hpdct_probe.hip): element bytes 1 or 4 (o1_bytes 0: no
// second output), n a multiple of 2048, at most cap_waves resident per CU
hipError_t launch_copy_ceiling(const void* in, int in_bytes, void* o0, int o0_bytes, void* o1, int o1_bytes,
                               uint64_t n, uint32_t cap_waves, hipStream_t s);

// hpdct_mapping in force (0 auto, 1 tile, 2 octet, 3 duo); hpdct_api.cpp.
int mapping_mode();

// Records msg as hpdct_last_error_string() of this thread and returns st
// (hpdct_api.cpp; every C-ABI error return goes through it).
int set_last_error(int st, const char* msg);

}  // namespace hpdct
