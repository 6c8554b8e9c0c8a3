// hpdct_grey_frame.hpp -- grey frames of any size, row pitch and alignment:
// a uint8 frame <-> the int16 blocks of the frame padded to whole 8x8 tiles
// (hpdct_forward_grey_frame / hpdct_inverse_grey_frame; include/hpdct.h has the
// contract in full).  The quant table travels in the kernel arguments.
//
// The mapping and every piece of arithmetic are hpdct_blocks.hpp's: one lane
// per tile, one 64-tile set per wave, over the PADDED tile grid, so block index
// = tile index and a whole set's blocks are one contiguous 8 KiB run whatever
// the width.  Only the pixel side differs: GreyGrid carries the row pitch and
// the frame's own height and width, and every byte offset is 64-bit.
//
//   forward  a tile wholly inside the frame, with an 8-byte aligned base and
//            pitch, loads its eight 8-byte rows with the pitch as the stride.
//            kGreyClip: a tile cut by the right or bottom edge (or every tile,
//            when base or pitch is not 8-byte aligned: a wave-uniform test)
//            fills the same RawTile from 64 byte loads at row min(r, height-1),
//            column min(x, width-1).  Behind the load: fdct_tile, the level
//            shift, quantise_biased_at, the pair packing and the staged or
//            per-lane block stores of fdct_blocks_kernel.
//   inverse  the lane's block, dequantised, through idct_tile; each row + 128,
//            clamped and truncated as store_row does for uint8, as one 8-byte
//            store.  kGreyClip: rows at or beyond the height are not stored, and
//            a row that the width cuts (or every row of an unaligned frame) is
//            stored byte by byte below the width.
// A tile of padding only does not exist: Hp - height < 8 and Wp - width < 8, so
// every tile of the padded grid holds at least one pixel of the frame.
#pragma once

#include "hpdct_blocks.hpp"
#include "hpdct_grey_frame.h"

namespace hpdct {

namespace {

// this wave's set and the number of sets, as blocks_nsets (ntiles < 2^32: no sum may wrap)
__device__ __forceinline__ uint32_t grey_nsets(const GreyGrid& g) { return g.ntiles / 64u + (g.ntiles % 64u != 0u); }

// The tile whose first pixel is (y0, x0) (inside the h x w frame), edge-
// replicated: byte j of row i comes from row min(y0 + i, h - 1), column
// min(x0 + j, w - 1).  Byte loads: any base, any pitch.
__device__ __forceinline__ void grey_load_clamped(RawTile<uint8_t>& raw, const uint8_t* __restrict__ img,
                                                  uint64_t pitch, uint64_t h, uint64_t w, uint64_t y0, uint64_t x0) {
    const uint32_t last = static_cast<uint32_t>(w - 1u - x0 < 7u ? w - 1u - x0 : 7u);  // the tile's last live column
    // Column by column, so that a load's address is its row's pointer and an immediate offset (sixteen address
    // registers for the tile; a clamped column index per load would make it 64 address pairs): column j of all
    // eight rows is loaded where it lies inside the frame and copied from column j - 1 where it does not.
    const uint8_t* row[8];
    uint32_t b[8][8];
    unroll<8>([&](auto i) {
        const uint64_t y = y0 + i < h ? y0 + i : h - 1u;
        row[i] = img + y * pitch + x0;
        b[i][0] = row[i][0];
    });
    unroll<7>([&](auto jj) {
        constexpr int j = jj + 1;
        if (static_cast<uint32_t>(j) <= last) {
            unroll<8>([&](auto i) { b[i][j] = row[i][j]; });
        } else {
            unroll<8>([&](auto i) { b[i][j] = b[i][j - 1]; });
        }
    });
    unroll<8>([&](auto i) {
        raw.r[i] = make_uint2(b[i][0] | (b[i][1] << 8) | (b[i][2] << 16) | (b[i][3] << 24),
                              b[i][4] | (b[i][5] << 8) | (b[i][6] << 16) | (b[i][7] << 24));
    });
}

}  // namespace

// ---------------------------------------------------------------------------
// Forward.  kVar: the quotient bits (kVarFastDiv, kVarJpegQ), kVarNT, kBlkStaged,
// kGreyClip and the workgroup size.  Everything behind the load is
// fdct_blocks_kernel's code (hpdct_blocks.hpp), its LDS image included.
// ---------------------------------------------------------------------------
template <bool kNatural, unsigned kVar>
__global__ __launch_bounds__(kBlock<kVar>, 1) void fdct_grey_frame_kernel(const uint8_t* __restrict__ img,
                                                                       int16_t* __restrict__ blocks, GreyGrid g,
                                                                       QParams qp, Mat64 qbytes) {
    constexpr bool kNT = (kVar & kVarNT) != 0;
    constexpr bool kClip = (kVar & kGreyClip) != 0;
    // kFrameDct: the exact DCT's matrix.  The 3-op quotient holds there (|C| < 4096), the per-position forms do not
    constexpr bool kDct = (kVar & kFrameDct) != 0;
    static_assert(!kDct || (kVar & kVarJpegQ) == 0, "the per-position quotient forms are proven for HpApprDCT only");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blocks_wave<kVar>();
    if (wave >= grey_nsets(g)) return;
    const uint32_t t0 = wave * 64u;
    if (t0 + lane >= g.ntiles) return;
    const uint32_t ty = (t0 + lane) / g.tiles_x, tx = (t0 + lane) - ty * g.tiles_x;
    const uint64_t pitch = g.pitch;
    const uint64_t y0 = static_cast<uint64_t>(ty) * 8u, x0 = static_cast<uint64_t>(tx) * 8u;

    const TSource<true, true, kDct> T(nullptr);
    // fdct_blocks_kernel's level shift, transform, quantiser and pair packing: the tile -> the block's 32 dwords
    // (kQuot: the quotient bits; every form gives the same integers.  Q from tq, 1/Q from qp.r)
    auto block_of = [&](const RawTile<uint8_t>& raw, uint32_t (&w)[32], const Mat64& tq, auto kQuot)
        __attribute__((always_inline)) {
        float x[8][8];
        raw.to_float(x, 128.0f);
        fdct_tile(T, x, [&](auto v, float (&c)[8]) {
            unroll<8>([&](auto u) {
                constexpr int pos = v * 8 + u;
                constexpr int n = zigzag::element_of(kNatural, pos);
                constexpr int mate = zigzag::position_of(kNatural, n ^ 1);  // rows arrive in order, columns too
                const int32_t q =
                    static_cast<int32_t>(quantise_biased_at<decltype(kQuot)::value, pos>(c[u], tq.v[pos], qp.r.v[pos]));
                if constexpr (mate > pos) {
                    w[n / 2] = static_cast<uint32_t>(q);
                } else if constexpr ((n & 1) != 0) {
                    w[n / 2] = pack_i16x2(static_cast<int32_t>(w[n / 2]), q);
                } else {
                    w[n / 2] = pack_i16x2(q, static_cast<int32_t>(w[n / 2]));
                }
            });
        });
    };
    uint32_t w[32];
    if constexpr (kClip) {
        // The edge lanes and the interior lanes each run the load AND the transform in a branch of their own and
        // meet again with the block's 32 dwords.  Meeting right behind the load, with the transform once, costs
        // the interior tiles a wave per SIMD: hipcc then schedules the whole transform with the tile's registers
        // ready at its start, converts all 64 pixels first (121-123 VGPRs against 92-93 with the JPEG forms, 102
        // against 80 with IEEE division) and keeps the 3-op quotient's 128 operands in SGPRs at once (48
        // spilled).  As two straight-line copies each branch compiles as fdct_blocks_kernel does.  A wave with
        // lanes of both kinds (one per tile row of an aligned frame, at its right edge) runs both.  The asm
        // comments differ so that the compiler does not merge the copies back into one.
        // The byte branch divides (IEEE), whatever the call's quotient is: the same integers (the 3-op forms are
        // launched only where they are proven equal to the division), and it reads Q alone, from qbytes, a
        // second copy of the table in the kernel arguments.  So the two branches share no operand.  Operands
        // they share are fetched once, before the branch, and held in SGPRs across it: with the same form in
        // both that is up to 128 values for the 102 SGPRs there are (8-64 spilled), and with one copy of Q it is
        // all of Q, which leaves the interior branch a 16-register window for 1/Q and 104 VGPRs.
        const bool aligned8 = ((reinterpret_cast<uintptr_t>(img) | pitch) & 7u) == 0u;  // wave-uniform
        if (!aligned8 || y0 + 8u > g.height || x0 + 8u > g.width) {
            RawTile<uint8_t> raw;
            grey_load_clamped(raw, img, pitch, g.height, g.width, y0, x0);
            block_of(raw, w, qbytes, std::integral_constant<unsigned, 0u>{});
            asm volatile("; grey frame: a tile by bytes");
        } else {
            RawTile<uint8_t> raw;
            raw.load(img + y0 * pitch + x0, pitch);
            block_of(raw, w, qp.q, std::integral_constant<unsigned, kVar & (kVarFastDiv | kVarJpegQ)>{});
            asm volatile("; grey frame: a tile by rows");
        }
    } else {
        RawTile<uint8_t> raw;
        raw.load(img + y0 * pitch + x0, pitch);
        block_of(raw, w, qp.q, std::integral_constant<unsigned, kVar & (kVarFastDiv | kVarJpegQ)>{});
    }

    // 64-bit byte offsets: ntiles * 128 passes 2^32 from 2^25 tiles
    char* const out = reinterpret_cast<char*>(blocks);
    if constexpr ((kVar & kBlkStaged) != 0) {
        __shared__ uint4 stage[kBlock<kVar> / 64u][512];
        if (g.ntiles - t0 >= 64u) {  // wave-uniform: every lane of the wave is here
            char* const image = reinterpret_cast<char*>(stage[__builtin_amdgcn_readfirstlane(threadIdx.x / 64u)]);
            const uint32_t wr = lane * 128u + 16u * (lane & 7u);
            unroll<8>([&](auto c) {
                *reinterpret_cast<uint4*>(image + (wr ^ (16u * c))) =
                    make_uint4(w[4 * c], w[4 * c + 1], w[4 * c + 2], w[4 * c + 3]);
            });
            // the pick-up reads other lanes' deposits: keep the compiler from moving it up
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // chunk j * 64 + lane of the set's run: chunk lane & 7 of lane j * 8 + lane / 8
            const uint32_t rd = (lane >> 3) * 128u + 16u * ((lane & 7u) ^ (lane >> 3));
            char* const run = out + static_cast<uint64_t>(t0) * 128u + 16u * lane;
            unroll<8>([&](auto j) {
                const uint4 v = *reinterpret_cast<const uint4*>(image + rd + 1024u * j);
                st16<kNT>(reinterpret_cast<uint4*>(run + 1024u * j), v);
            });
            return;
        }
    }
    uint4* const dst = reinterpret_cast<uint4*>(out + static_cast<uint64_t>(t0 + lane) * 128u);
    unroll<8>([&](auto c) { st16<kNT>(dst + c, make_uint4(w[4 * c], w[4 * c + 1], w[4 * c + 2], w[4 * c + 3])); });
}

// ---------------------------------------------------------------------------
// Inverse: int16 blocks -> uint8 pixels.  kVar: kVarNT (the pixel stores),
// kGreyClip, kVarFullChain (every term of T kept, as idct_blocks_kernel) and
// the workgroup size.  The load, the dequantisation and the transform are
// idct_blocks_kernel's; a whole row is store_row's 8-byte store, so a wave's
// row is 512 contiguous bytes.
// ---------------------------------------------------------------------------
template <bool kNatural, unsigned kVar>
__global__ __launch_bounds__(kBlock<kVar>, 1) void idct_grey_frame_kernel(const int16_t* __restrict__ blocks,
                                                                       uint8_t* __restrict__ out, GreyGrid g,
                                                                       Mat64 q) {
    constexpr bool kNT = (kVar & kVarNT) != 0;
    constexpr bool kClip = (kVar & kGreyClip) != 0;
    // kFrameDct: the exact DCT's matrix (no zero: every term kept), and the pixel is R + 128.5f, clamped and
    // truncated: round half up, as JPEG decoders do, in place of the reference's R + 128 truncated
    constexpr bool kDct = (kVar & kFrameDct) != 0;
    constexpr float kShift = kDct ? 128.5f : 128.0f;
    const TSource<true, (kVar & kVarFullChain) == 0, kDct> T(nullptr);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blocks_wave<kVar>();
    if (wave >= grey_nsets(g)) return;
    const uint32_t t0 = wave * 64u;
    if (t0 + lane >= g.ntiles) return;
    const uint32_t ty = (t0 + lane) / g.tiles_x, tx = (t0 + lane) - ty * g.tiles_x;
    const uint64_t pitch = g.pitch;
    const uint64_t y0 = static_cast<uint64_t>(ty) * 8u, x0 = static_cast<uint64_t>(tx) * 8u;
    uint8_t* const dst = out + y0 * pitch + x0;
    // kGreyClip: the rows and columns of the tile inside the frame (at least one of each: no tile is padding only)
    uint32_t live_rows = 8u, live_cols = 8u;
    bool whole_rows = true;
    if constexpr (kClip) {
        const bool aligned8 = ((reinterpret_cast<uintptr_t>(out) | pitch) & 7u) == 0u;  // wave-uniform
        live_rows = static_cast<uint32_t>(g.height - y0 < 8u ? g.height - y0 : 8u);
        live_cols = static_cast<uint32_t>(g.width - x0 < 8u ? g.width - x0 : 8u);
        whole_rows = aligned8 && live_cols == 8u;
    }

    const uint4* const src = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(blocks) +
                                                            static_cast<uint64_t>(t0 + lane) * 128u);
    uint4 r[8];
    unroll<8>([&](auto c) { r[c] = src[c]; });
    float d[8][8];
    unroll<32>([&](auto k) {
        constexpr int p0 = zigzag::position_of(kNatural, 2 * k), p1 = zigzag::position_of(kNatural, 2 * k + 1);
        const uint32_t word = dword_of<k % 4>(r[k / 4]);
        // multiply_matrices (utils_kernels.cu:55): D = q * Q
        d[p0 / 8][p0 % 8] = static_cast<float>(static_cast<int32_t>(static_cast<int16_t>(word & 0xffffu))) * q.v[p0];
        d[p1 / 8][p1 % 8] = static_cast<float>(static_cast<int32_t>(word) >> 16) * q.v[p1];
    });
    if constexpr (!kClip) {
        idct_tile(T, d, [&](auto v, float (&row)[8]) {
            // add_matrix_scalar (utils_kernels.cu:29): R + 128
            unroll<8>([&](auto u) { row[u] = row[u] + kShift; });
            store_row<kNT>(dst + v * pitch, row);
        });
    } else {
        // The transform stays straight-line code: each row waits as the 8 bytes store_row would write (a row of P
        // dies as its pixels are packed, so the 16 registers cost no occupancy), and the stores, which branch
        // per lane, come after it.
        uint2 px[8];
        idct_tile(T, d, [&](auto v, float (&row)[8]) {
            unroll<8>([&](auto u) { row[u] = row[u] + kShift; });
            // convertToUnsignedChar, as store_row packs it
            px[v] = make_uint2(pack_u8x4(row[0], row[1], row[2], row[3]), pack_u8x4(row[4], row[5], row[6], row[7]));
        });
        if (whole_rows) {
            unroll<8>([&](auto v) {
                if (static_cast<uint32_t>(v) < live_rows) st<kNT>(reinterpret_cast<uint2*>(dst + v * pitch), px[v]);
            });
        } else {
            unroll<8>([&](auto v) {
                if (static_cast<uint32_t>(v) < live_rows) {
                    uint8_t* const pb = dst + v * pitch;
                    unroll<8>([&](auto b) {
                        if (static_cast<uint32_t>(b) < live_cols)
                            pb[b] = static_cast<uint8_t>(((b < 4 ? px[v].x : px[v].y) >> (8 * (b % 4))) & 0xffu);
                    });
                }
            });
        }
    }
}

}  // namespace hpdct
