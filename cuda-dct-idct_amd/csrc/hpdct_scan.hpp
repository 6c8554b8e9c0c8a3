// hpdct_scan.hpp -- the baseline-JPEG entropy coder (hpdct_encode_scan): int16
// coefficient blocks -> the Huffman-coded bytes of one interleaved scan (ITU-T
// T.81 baseline, the typical tables of Annex K.3).  The host part (the tables,
// the scan's geometry, the bound) is plain C++: hpdct_api_jpeg.cpp includes it
// under g++ too.  The kernels are compiled by hpdct_scan.hip only (HPDCT_SCAN_KERNELS).
// fill_codes is the one builder of the coder's entries, for Annex K's constants
// and a caller's blob alike; launch_scan is the one launch path for both.
//
// Three launches, one chain:
//   1. measure  one wave per restart interval, 64 blocks of the interval (in
//               scan order) per step, one lane per block.  A lane walks its
//               block once, gathering its codes in a register and writing them
//               as whole words to its own LDS words; a wave prefix sum of the
//               bit lengths gives the bit offsets, the lanes OR their words
//               into the wave's LDS bit buffer at those offsets, and the wave
//               counts the 0xFF bytes of the whole bytes;
//               the partial byte is carried into the next step.  Result: the
//               interval's exact byte length (stuffing, padding and marker
//               included) and its count of uncodable coefficients.
//   2. offsets  one workgroup: exclusive scan of the lengths (in place), the
//               total, `truncated`, the out-of-range total.
//   3. emit     the same coding again; each 256-byte piece of the bit buffer is
//               stuffed by a wave prefix count of its 0xFF bytes and stored at
//               its final offset.  Nothing is stored when the scan does not fit.
// No workgroup waits on another, every loop bound follows from the launch
// arguments, and the result does not depend on scheduling.  An interval is
// coded by ONE wave, step after step: the call is parallel across intervals
// only, so restart_interval = 0 (one interval) serialises the whole frame.
#pragma once

#include <stdint.h>

#include "hpdct.h"
#include "hpdct_kernels.h"
#include "hpdct_zigzag.h"

namespace hpdct {
namespace unscan {
struct HuffBlob;  // hpdct_unscan.hpp
}
namespace scan {

// ITU-T T.81 Annex K.3, tables K.3 - K.6: bits[l-1] = number of codes of length
// l, vals = the symbols in order of increasing code length.  The one definition: hpdct_huffman_table, the
// device constants below and in hpdct_unscan.hpp, and huff::annex_k (hpdct_huffman.hpp) all read it.
constexpr hpdct_huffman_spec kDcLuma = {
    {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr hpdct_huffman_spec kDcChroma = {
    {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr hpdct_huffman_spec kAcLuma = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    162};
constexpr hpdct_huffman_spec kAcChroma = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    162};
// kind: 0 DC luma, 1 AC luma, 2 DC chroma, 3 AC chroma (hpdct_huffman_table)
constexpr const hpdct_huffman_spec& spec_of(int kind) {
    return kind == 0 ? kDcLuma : kind == 1 ? kAcLuma : kind == 2 ? kDcChroma : kAcChroma;
}

// The coder's tables as the kernels index them: entry = (code length << 16) |
// code, at [symbol].  ac[0], ac[1]: luma, chroma (256 entries, symbol =
// run << 4 | size); dc[0], dc[1]: 16 entries, symbol = category.
struct CodeTables {
    uint32_t ac[2][256];
    uint32_t dc[2][16];
};
constexpr int kCodeTableWords = 2 * 256 + 2 * 16;
// the entries of one table, for Annex K's specs at compile time and a caller's at run time (huff::fill_blob);
// a symbol without a code keeps the entry it had (0: length 0)
constexpr void fill_codes(const hpdct_huffman_spec& s, uint32_t* e) {
    uint32_t code = 0;
    int k = 0;
    for (uint32_t len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.bits[len - 1]; ++i) e[s.vals[k++]] = (len << 16) | code++;
        code <<= 1;
    }
}
constexpr CodeTables make_code_tables() {
    CodeTables t{};
    fill_codes(kAcLuma, t.ac[0]);
    fill_codes(kAcChroma, t.ac[1]);
    fill_codes(kDcLuma, t.dc[0]);
    fill_codes(kDcChroma, t.dc[1]);
    return t;
}
// the longest code of a table
constexpr int longest_code(const hpdct_huffman_spec& s) {
    int l = 0;
    for (int i = 0; i < 16; ++i)
        if (s.bits[i] != 0) l = i + 1;
    return l;
}

// The largest categories baseline Huffman codes: a DC difference of 11 bits
// (|d| <= 2047), an AC value of 10 bits (|v| <= 1023).  A coefficient beyond
// them is counted (hpdct_scan_info.out_of_range) and coded with the largest
// category and its low bits, so a block never exceeds kMaxBlockBits.
constexpr int kMaxDcCat = 11, kMaxAcCat = 10;
// Worst case of one block: the longest DC code + 11 bits, then 63 times the
// longest AC code + 10 bits (a block whose coefficient 63 is non-zero has no
// EOB; a ZRL replaces 16 coefficients and is shorter than they are).
constexpr int kMaxDcBits = (longest_code(kDcLuma) > longest_code(kDcChroma) ? longest_code(kDcLuma)
                                                                            : longest_code(kDcChroma)) +
                           kMaxDcCat;
constexpr int kMaxAcBits = (longest_code(kAcLuma) > longest_code(kAcChroma) ? longest_code(kAcLuma)
                                                                            : longest_code(kAcChroma)) +
                           kMaxAcCat;
constexpr int kMaxBlockBits = kMaxDcBits + 63 * kMaxAcBits;  // 22 + 63 * 26 = 1660
static_assert(kMaxBlockBits == 1660, "Annex K tables");

// hpdct_scan_bound: an interval of B_i bits gives at most B_i / 8 + 1 bytes
// once padded, at most twice that once stuffed (every byte 0xFF), plus its two
// marker bytes: the sum over the intervals is at most
// 2 * (kMaxBlockBits / 8) * blocks + 4 * intervals = 415 * blocks + 4 * intervals.
constexpr int64_t kBoundPerBlock = 2 * kMaxBlockBits / 8;
static_assert(kBoundPerBlock * 8 == 2 * kMaxBlockBits, "whole bytes");
constexpr int64_t kBoundPerInterval = 4;

// Geometry of a scan: MCUs in row-major order, `per_interval` of them per
// restart interval (the last interval may be shorter).
struct ScanGrid {
    uint32_t nmcu;          // MCUs of the frame (< 2^32)
    uint32_t mcus_x;        // MCUs per MCU row
    uint32_t per_interval;  // restart_interval, or nmcu when it is 0
    uint32_t intervals;     // ceil(nmcu / per_interval)
    uint32_t bpm;           // blocks per MCU: 1 (grey), 3 (4:4:4) or 6 (4:2:0)
};
// the workspace: uint64 length-then-offset per interval, then uint32
// out-of-range count per interval; 12 bytes per interval, rounded up to 16
constexpr int64_t workspace_bytes(uint64_t intervals) {
    return static_cast<int64_t>((intervals * 12u + 15u) / 16u * 16u);
}

// The wave's bit buffer: 64 blocks of kMaxBlockBits and the 7 carried bits, one
// word of slack for the two-word OR of the last code: 3322 words, 13 KiB.
constexpr uint32_t kBitWords = (64u * kMaxBlockBits + 7u + 31u) / 32u + 1u;
constexpr uint32_t kBlkStride = 33;  // dwords per staged block: 32 + 1, so the lanes' rows start in 64 banks
// a lane's own words for its block's bits: ceil(1660 / 32) = 52, an odd stride for the same reason
constexpr uint32_t kPrivStride = (kMaxBlockBits + 31) / 32 + 1;
static_assert(kPrivStride % 2u == 1u, "odd stride");

// Under a caller's tables (hpdct_encode_scan_tables) a code has up to 16 bits
// in every table: a block reaches (16 + 11) + 63 * (16 + 10) = 1665 bits.
constexpr int kMaxBlockBitsT = (16 + kMaxDcCat) + 63 * (16 + kMaxAcCat);
static_assert(kMaxBlockBitsT == 1665, "16-bit codes");
// hpdct_scan_bound_tables: 2 * 1665 / 8 = 416.25 bytes a block, rounded up
constexpr int64_t kBoundPerBlockT = (2 * kMaxBlockBitsT + 7) / 8;
static_assert(kBoundPerBlockT == 417, "rounded up");
constexpr uint32_t kBitWordsT = (64u * kMaxBlockBitsT + 7u + 31u) / 32u + 1u;  // 3332 words
constexpr uint32_t kPrivStrideT = (kMaxBlockBitsT + 31) / 32 + 2;              // 53 words and two: 55, odd
static_assert(kPrivStrideT % 2u == 1u && kPrivStrideT > (kMaxBlockBitsT + 31) / 32, "odd stride");

}  // namespace scan

// The three launches on s, as policy::scan_code / scan_offsets choose them
// (hpdct_scan.hip).  cb == cr == nullptr with g.bpm == 1; workspace holds
// scan::workspace_bytes(g.intervals) bytes, 16-byte aligned; user_offs
// (g.intervals + 1 entries) may be nullptr.  blob nullptr: Annex K's kernels;
// else the caller's tables, a HuffBlob (hpdct_unscan.hpp) in device memory, of
// which the coder reads the leading scan::CodeTables.  The caller checked everything.
hipError_t launch_scan(const int16_t* y, const int16_t* cb, const int16_t* cr, const scan::ScanGrid& g, bool natural,
                       uint8_t* out, uint64_t capacity, hpdct_scan_info* info, uint64_t* user_offs, void* workspace,
                       const unscan::HuffBlob* blob, hipStream_t s);
// hpdct_scan_histogram (hpdct_scan_hist.hpp): a memset of counts (4 * 256 uint64) and one launch
hipError_t launch_scan_hist(const int16_t* y, const int16_t* cb, const int16_t* cr, const scan::ScanGrid& g,
                            bool natural, uint64_t* counts, hipStream_t s);

}  // namespace hpdct

// the kernels: for the unit that defines HPDCT_SCAN_KERNELS (hpdct_scan.hip) only
#if defined(__HIPCC__) && defined(HPDCT_SCAN_KERNELS)

#include "hpdct_tile.hpp"  // unroll<N>

namespace hpdct {

__device__ const scan::CodeTables kScanCodeTables = scan::make_code_tables();

// inclusive prefix sum over the wave's 64 lanes
__device__ inline uint32_t scan_wave_prefix(uint32_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// ORs the low n bits of val (1 <= n <= 32) into the buffer at bit position pos,
// MSB first: bit p of the stream is bit 31 - p % 32 of word p / 32
__device__ inline void scan_or_bits(uint32_t* bits, uint32_t pos, uint32_t val, uint32_t n) {
    const uint32_t o = pos & 31u;
    const uint64_t x = static_cast<uint64_t>(val) << (64u - o - n);
    atomicOr(&bits[pos >> 5], static_cast<uint32_t>(x >> 32));
    if (static_cast<uint32_t>(x) != 0u) atomicOr(&bits[(pos >> 5) + 1u], static_cast<uint32_t>(x));
}

// One block, walked once: blk its 64 coefficients in zig-zag order (32 dwords
// of LDS), nz the mask of its non-zero AC coefficients (bit n: coefficient n),
// dc the DC difference, ac / dc_tab the component's tables.  The codes
// are gathered in a 64-bit register and leave it as whole words, MSB first,
// into priv (the lane's own kPrivStride words: no other lane touches them); the
// last word's unused low bits are 0.  Returns the block's bit length
// (<= kMaxBlockBits); oor counts the coefficients baseline cannot code.
// kCustom: the tables are a caller's, untrusted: a length is clamped to 16 (so a
// put takes at most 16 + 11 = 27 bits and the block at most kMaxBlockBitsT), and
// a symbol without a code (length 0) is counted in oor as well.
template <bool kCustom = false>
__device__ inline uint32_t scan_walk(const uint32_t* blk, uint64_t nz, int dc, const uint32_t* ac,
                                     const uint32_t* dc_tab, uint32_t* priv, uint32_t& oor) {
    uint64_t acc = 0;           // the low nacc bits are pending
    uint32_t nacc = 0, nw = 0;  // nacc < 32 between puts
    auto put = [&](uint32_t entry, uint32_t cat, uint32_t extra) {
        uint32_t clen = entry >> 16;
        if constexpr (kCustom) {
            clen = clen > 16u ? 16u : clen;
            oor += clen == 0u;
        }
        const uint32_t n = clen + cat;  // 1..26; kCustom: 0..27, and nacc + n <= 58 bits of acc
        acc = (acc << n) | (((entry & 0xffffu) << cat) | extra);
        nacc += n;
        if (nacc >= 32u) {
            nacc -= 32u;
            priv[nw++] = static_cast<uint32_t>(acc >> nacc);
        }
    };
    {
        const uint32_t a = static_cast<uint32_t>(dc < 0 ? -dc : dc);
        uint32_t cat = 32u - static_cast<uint32_t>(__clz(a));  // __clz(0) = 32
        if (cat > scan::kMaxDcCat) cat = scan::kMaxDcCat, ++oor;
        put(dc_tab[cat], cat, static_cast<uint32_t>(dc < 0 ? dc - 1 : dc) & ((1u << cat) - 1u));
    }
    // the non-zero AC coefficients only, in scan order: nz has bit n set for zig-zag coefficient n != 0
    const int16_t* c16 = reinterpret_cast<const int16_t*>(blk);
    uint32_t prev = 0;
    while (nz != 0ull) {  // at most 63 turns
        const uint32_t k = static_cast<uint32_t>(__builtin_ctzll(nz));
        nz &= nz - 1ull;
        uint32_t run = k - prev - 1u;
        prev = k;
        const int c = c16[k];
        for (; run >= 16u; run -= 16u) put(ac[0xf0], 0u, 0u);  // ZRL
        const uint32_t a = static_cast<uint32_t>(c < 0 ? -c : c);
        uint32_t cat = 32u - static_cast<uint32_t>(__clz(a));
        if (cat > scan::kMaxAcCat) cat = scan::kMaxAcCat, ++oor;
        put(ac[(run << 4) | cat], cat, static_cast<uint32_t>(c < 0 ? c - 1 : c) & ((1u << cat) - 1u));
    }
    if (prev != 63u) put(ac[0], 0u, 0u);  // EOB, unless coefficient 63 is non-zero
    if (nacc != 0u) priv[nw] = static_cast<uint32_t>(acc << (32u - nacc));
    return 32u * nw + nacc;
}

// ORs the lane's len bits (whole words in priv, MSB first, zero beyond len) into
// the wave's buffer from bit position pos on
__device__ inline void scan_place(uint32_t* bits, uint32_t pos, const uint32_t* priv, uint32_t len) {
    const uint32_t o = pos & 31u;
    uint32_t idx = pos >> 5;
    for (uint32_t w = 0; 32u * w < len; ++w, ++idx) {
        const uint32_t v = priv[w];
        atomicOr(&bits[idx], v >> o);
        if (o != 0u && (v << (32u - o)) != 0u) atomicOr(&bits[idx + 1u], v << (32u - o));
    }
}

// Where block j of an interval that starts at MCU m0 lies: its array, its index
// there, and the block whose DC predicts it (prev, nullptr at an interval's start).
struct ScanBlockRef {
    const int16_t* blk;
    const int16_t* prev;
    uint32_t chroma;  // 0: the luma tables, 1: the chroma tables
};
__device__ inline ScanBlockRef scan_locate(const int16_t* y, const int16_t* cb, const int16_t* cr,
                                           const scan::ScanGrid& g, uint64_t m0, uint64_t j) {
    const uint64_t ml = j / g.bpm, m = m0 + ml;
    const uint32_t k = static_cast<uint32_t>(j % g.bpm);
    ScanBlockRef r;
    if (g.bpm == 6u && k < 4u) {
        // Y(dy, dx) of MCU (my, mx) is tile (2 my + dy, 2 mx + dx) of the Y plane
        const uint64_t my = m / g.mcus_x, mx = m % g.mcus_x, tx = 2ull * g.mcus_x;
        const uint64_t t = (2u * my + (k >> 1)) * tx + 2u * mx + (k & 1u);
        r.blk = y + 64u * t, r.chroma = 0u;
        if (k != 0u) {
            const uint32_t kp = k - 1u;
            r.prev = y + 64u * ((2u * my + (kp >> 1)) * tx + 2u * mx + (kp & 1u));
        } else if (ml != 0u) {
            const uint64_t pm = m - 1u, py = pm / g.mcus_x, px = pm % g.mcus_x;
            r.prev = y + 64u * ((2u * py + 1u) * tx + 2u * px + 1u);
        } else {
            r.prev = nullptr;
        }
        return r;
    }
    const uint32_t comp = g.bpm == 6u ? k - 3u : k;  // 0 Y, 1 Cb, 2 Cr
    const int16_t* base = comp == 0u ? y : comp == 1u ? cb : cr;
    r.blk = base + 64u * m, r.chroma = comp != 0u;
    r.prev = ml != 0u ? r.blk - 64 : nullptr;
    return r;
}

// Launches 1 (kVar without kScanEmit) and 3 (with it); one wave per workgroup,
// workgroup b takes the intervals b, b + gridDim.x, ...
//   measure: lens[i] = the byte length of interval i, oor[i] its uncodable coefficients
//   emit:    lens[i] holds the interval's byte offset (the offsets kernel ran);
//            the bytes go to out, below capacity only, and only if !info->truncated
// kVar with kScanTables: tab_src is the caller's (untrusted) tables and the
// buffers are sized for blocks of kMaxBlockBitsT bits; else Annex K's.
template <unsigned kVar>
__device__ inline void scan_code_body(const int16_t* __restrict__ y, const int16_t* __restrict__ cb,
                                      const int16_t* __restrict__ cr, const scan::ScanGrid& g,
                                      uint64_t* __restrict__ lens, uint32_t* __restrict__ oor,
                                      const hpdct_scan_info* __restrict__ info, uint8_t* __restrict__ out,
                                      const uint64_t capacity, const uint32_t* __restrict__ tab_src) {
    constexpr bool kEmit = (kVar & kScanEmit) != 0u;
    constexpr bool kNatural = (kVar & kScanNatural) != 0u;
    constexpr bool kCustom = (kVar & kScanTables) != 0u;
    constexpr uint32_t kPriv = kCustom ? scan::kPrivStrideT : scan::kPrivStride;
    constexpr uint32_t kBits = kCustom ? scan::kBitWordsT : scan::kBitWords;
    __shared__ uint32_t s_tab[scan::kCodeTableWords];
    __shared__ uint32_t s_blk[64u * scan::kBlkStride];
    __shared__ uint32_t s_priv[64u * kPriv];
    __shared__ uint32_t s_bits[kBits];
    const uint32_t lane = threadIdx.x;
    if constexpr (kEmit) {
        if (info->truncated != 0u) return;
    }
    {
        static_assert(sizeof(scan::CodeTables) == 4u * scan::kCodeTableWords, "tables are packed");
        for (uint32_t i = lane; i < static_cast<uint32_t>(scan::kCodeTableWords); i += 64u) s_tab[i] = tab_src[i];
    }
    uint32_t* const my_blk = s_blk + lane * scan::kBlkStride;
    uint32_t* const my_priv = s_priv + lane * kPriv;

    for (uint64_t iv = blockIdx.x; iv < g.intervals; iv += gridDim.x) {
        const uint64_t m0 = iv * g.per_interval;
        const uint64_t mcount = g.nmcu - m0 < g.per_interval ? g.nmcu - m0 : g.per_interval;
        const uint64_t nblk = mcount * g.bpm;
        const bool last_interval = iv + 1u == g.intervals;
        uint32_t carry_n = 0, carry_v = 0;   // the partial byte carried into the next step: carry_n bits, value carry_v
        uint64_t data_bytes = 0;             // measure: whole bytes before stuffing
        uint32_t ff_acc = 0, oor_acc = 0;    // measure, per lane
        uint64_t out_pos = 0;                // emit: where the next byte goes
        if constexpr (kEmit) out_pos = lens[iv];

        for (uint64_t base = 0; base < nblk; base += 64u) {
            const uint64_t j = base + lane;
            const bool active = j < nblk;
            __syncthreads();  // the previous step's readers of s_bits are done (and s_tab is loaded)
            int dcdiff = 0;
            uint32_t chroma = 0;
            uint64_t nz = 0;
            if (active) {
                const ScanBlockRef r = scan_locate(y, cb, cr, g, m0, j);
                chroma = r.chroma;
                // the load and permutation below are also scan_stage of hpdct_scan_hist.hpp: keep the two in step
                uint32_t v[32];
                const uint4* p = reinterpret_cast<const uint4*>(r.blk);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const uint4 t = p[q];
                    v[4 * q] = t.x, v[4 * q + 1] = t.y, v[4 * q + 2] = t.z, v[4 * q + 3] = t.w;
                }
                const int dc0 = static_cast<int16_t>(v[0] & 0xffffu);
                dcdiff = dc0 - (r.prev ? static_cast<int>(*r.prev) : 0);
                // element n of the staged block = zig-zag coefficient n (natural blocks are permuted here)
                unroll<32>([&](auto w) {
                    uint32_t d = v[w];
                    if constexpr (kNatural) {
                        constexpr int e0 = zigzag::kOrder[2 * w], e1 = zigzag::kOrder[2 * w + 1];
                        const uint32_t lo = (v[e0 >> 1] >> (16 * (e0 & 1))) & 0xffffu;
                        const uint32_t hi = (v[e1 >> 1] >> (16 * (e1 & 1))) & 0xffffu;
                        d = lo | (hi << 16);
                    }
                    my_blk[w] = d;
                    nz |= static_cast<uint64_t>((d & 0xffffu) != 0u) << (2 * w);
                    nz |= static_cast<uint64_t>((d >> 16) != 0u) << (2 * w + 1);
                });
                nz &= ~1ull;  // the DC is coded as a difference
            }
            const uint32_t* ac = s_tab + 256u * chroma;
            const uint32_t* dct = s_tab + 512u + 16u * chroma;
            const uint32_t len = active ? scan_walk<kCustom>(my_blk, nz, dcdiff, ac, dct, my_priv, oor_acc) : 0u;
            const uint32_t incl = scan_wave_prefix(len, lane);
            const uint32_t nbits = carry_n + __shfl(incl, 63, 64);
            const uint32_t words = (nbits + 31u) / 32u + 1u;  // <= kBits
            for (uint32_t i = lane; i < words; i += 64u) s_bits[i] = 0u;
            __syncthreads();
            if (lane == 0u && carry_n != 0u) atomicOr(&s_bits[0], carry_v << (32u - carry_n));
            scan_place(s_bits, carry_n + incl - len, my_priv, len);
            uint32_t nbytes = nbits >> 3, rem = nbits & 7u;
            if (base + 64u >= nblk && rem != 0u) {
                // the interval's end: the partial byte is padded with 1 bits
                if (lane == 0u) scan_or_bits(s_bits, nbits, (1u << (8u - rem)) - 1u, 8u - rem);
                ++nbytes, rem = 0u;
            }
            __syncthreads();
            carry_n = rem;
            if (rem != 0u) carry_v = ((s_bits[nbytes >> 2] >> (24u - 8u * (nbytes & 3u))) & 0xffu) >> (8u - rem);
            if constexpr (!kEmit) data_bytes += nbytes;
            // the whole bytes, 256 per pass (four per lane): count or stuff the 0xFF bytes
            for (uint32_t b0 = 0; b0 < nbytes; b0 += 256u) {
                const uint32_t idx = b0 + 4u * lane;
                const uint32_t valid = idx < nbytes ? (nbytes - idx < 4u ? nbytes - idx : 4u) : 0u;
                const uint32_t w = valid != 0u ? s_bits[idx >> 2] : 0u;
                uint32_t nff = 0;
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) nff += k < valid && ((w >> (24u - 8u * k)) & 0xffu) == 0xffu;
                if constexpr (!kEmit) {
                    ff_acc += nff;
                } else {
                    const uint32_t inc = scan_wave_prefix(nff, lane);
                    uint64_t pos = out_pos + 4u * lane + (inc - nff);
#pragma unroll
                    for (uint32_t k = 0; k < 4u; ++k) {
                        if (k < valid) {
                            const uint32_t byte = (w >> (24u - 8u * k)) & 0xffu;
                            if (pos < capacity) out[pos] = static_cast<uint8_t>(byte);
                            ++pos;
                            if (byte == 0xffu) {
                                if (pos < capacity) out[pos] = 0u;
                                ++pos;
                            }
                        }
                    }
                    out_pos += (nbytes - b0 < 256u ? nbytes - b0 : 256u) + __shfl(inc, 63, 64);
                }
            }
        }
        // every interval but the last is followed by RSTm, m = interval index mod 8
        if constexpr (kEmit) {
            if (!last_interval && lane == 0u) {
                if (out_pos < capacity) out[out_pos] = 0xffu;
                if (out_pos + 1u < capacity) out[out_pos + 1u] = static_cast<uint8_t>(0xd0u + (iv & 7u));
            }
        } else {
            const uint32_t ff = __shfl(scan_wave_prefix(ff_acc, lane), 63, 64);
            const uint32_t bad = __shfl(scan_wave_prefix(oor_acc, lane), 63, 64);
            if (lane == 0u) {
                lens[iv] = data_bytes + ff + (last_interval ? 0u : 2u);
                oor[iv] = bad;
            }
        }
    }
}

template <unsigned kVar>
__global__ __launch_bounds__(64) void scan_code_kernel(const int16_t* __restrict__ y, const int16_t* __restrict__ cb,
                                                       const int16_t* __restrict__ cr, const scan::ScanGrid g,
                                                       uint64_t* __restrict__ lens, uint32_t* __restrict__ oor,
                                                       const hpdct_scan_info* __restrict__ info,
                                                       uint8_t* __restrict__ out, const uint64_t capacity) {
    static_assert((kVar & kScanTables) == 0u, "Annex K");
    scan_code_body<kVar>(y, cb, cr, g, lens, oor, info, out, capacity, &kScanCodeTables.ac[0][0]);
}
// the same under the caller's tables (kVar carries kScanTables): tables, the leading scan::CodeTables of a HuffBlob
template <unsigned kVar>
__global__ __launch_bounds__(64) void scan_code_tables_kernel(
    const int16_t* __restrict__ y, const int16_t* __restrict__ cb, const int16_t* __restrict__ cr,
    const scan::ScanGrid g, uint64_t* __restrict__ lens, uint32_t* __restrict__ oor,
    const hpdct_scan_info* __restrict__ info, uint8_t* __restrict__ out, const uint64_t capacity,
    const uint32_t* __restrict__ tables) {
    static_assert((kVar & kScanTables) != 0u, "the caller's tables");
    scan_code_body<kVar>(y, cb, cr, g, lens, oor, info, out, capacity, tables);
}

// Launch 2, one workgroup of 1024 threads: lens[i] (byte lengths) becomes the
// byte offset of interval i, in place; the total, `truncated` and the
// out-of-range total go to *info, the offsets (n + 1 entries) to user_offs when
// given.  Thread t owns the intervals [t * chunk, (t + 1) * chunk).
__global__ __launch_bounds__(1024) void scan_offsets_kernel(uint64_t* __restrict__ lens,
                                                            const uint32_t* __restrict__ oor, const uint32_t n,
                                                            uint64_t* __restrict__ user_offs,
                                                            hpdct_scan_info* __restrict__ info,
                                                            const uint64_t capacity) {
    __shared__ uint64_t s_sum[1024];
    __shared__ unsigned long long s_oor;
    const uint32_t t = threadIdx.x;
    const uint64_t chunk = (static_cast<uint64_t>(n) + 1023u) / 1024u;
    const uint64_t b = t * chunk < n ? t * chunk : n, e = b + chunk < n ? b + chunk : n;
    if (t == 0u) s_oor = 0ull;
    uint64_t sum = 0, bad = 0;
    for (uint64_t i = b; i < e; ++i) sum += lens[i], bad += oor[i];
    s_sum[t] = sum;
    __syncthreads();
    if (bad != 0u) atomicAdd(&s_oor, static_cast<unsigned long long>(bad));  // integer: order-independent
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint64_t o = t >= d ? s_sum[t - d] : 0u;
        __syncthreads();
        s_sum[t] += o;
        __syncthreads();
    }
    uint64_t run = s_sum[t] - sum;
    for (uint64_t i = b; i < e; ++i) {
        const uint64_t l = lens[i];
        lens[i] = run;
        if (user_offs) user_offs[i] = run;
        run += l;
    }
    if (t == 1023u) {
        const uint64_t total = s_sum[1023];
        if (user_offs) user_offs[n] = total;
        info->bytes = total;
        info->truncated = total > capacity ? 1u : 0u;
        info->out_of_range = s_oor > 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(s_oor);
    }
}

}  // namespace hpdct

#endif  // HPDCT_SCAN_KERNELS
