// hpdct_blocks.hpp -- JPEG-style int16 coefficient blocks: forward (uint8
// frame -> blocks) and inverse (blocks -> fp32 or uint8 pixels) kernels on the
// tile-per-lane mapping of hpdct_kernels_impl.hpp, one 64-tile set per wave.
//
// Layout: block t = tile t in row-major tile order (t = by * tiles_x + bx), 64
// int16 = 128 B each, so a 64-tile set is one contiguous 8 KiB run whatever the
// frame width; element n of a block is the quantised coefficient at row-major
// position zigzag[n] (or n in natural order).  A lane holds its whole tile in
// registers with compile-time indices, so the scan order is a register renaming.
//
// Arithmetic: exactly the uint8 -> fp32 forward's (fdct_tile, the quantiser
// forms of quantise_biased_at) with the final v_trunc_f32 replaced by the
// truncating v_cvt_i32_f32, as the int8 wire format does: the same integers,
// -0.0 becomes 0.  The inverse dequantises (float)q * Q and runs idct_tile with
// the zero terms of T skipped.  That is exact only while q * Q and every
// partial sum stay finite, which the table alone does not promise (any finite
// entry is legal: 32767 * 2e34 is infinite, and 0 * inf is NaN in the
// reference): the host launches the kVarFullChain variant, which keeps every
// term, for a table that fails its criterion (skip_zero_exact, hpdct_api.cpp).
#pragma once

#include "hpdct_kernels_impl.hpp"
#include "hpdct_zigzag.h"

namespace hpdct {

namespace {

// two int32 in int16 range -> one dword (v_cvt_pk_i16_i32; it saturates, which
// the host's range rule never lets happen)
__device__ __forceinline__ uint32_t pack_i16x2(int32_t lo, int32_t hi) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pk_i16(lo, hi));
}

template <int kI>
__device__ __forceinline__ uint32_t dword_of(const uint4& v) {
    static_assert(kI >= 0 && kI < 4, "dword");
    if constexpr (kI == 0) return v.x;
    else if constexpr (kI == 1) return v.y;
    else if constexpr (kI == 2) return v.z;
    else return v.w;
}

template <bool kNT>
__device__ __forceinline__ void st16(uint4* p, const uint4& v) {
    if constexpr (kNT) {
        __builtin_nontemporal_store(v.x, &p->x);
        __builtin_nontemporal_store(v.y, &p->y);
        __builtin_nontemporal_store(v.z, &p->z);
        __builtin_nontemporal_store(v.w, &p->w);
    } else {
        *p = v;
    }
}

// this wave's set and the number of sets (ntiles < 2^32: no sum may wrap)
__device__ __forceinline__ uint32_t blocks_nsets(const TileGrid& g) { return g.ntiles / 64u + (g.ntiles % 64u != 0u); }
template <unsigned kVar>
__device__ __forceinline__ uint32_t blocks_wave() {
    return __builtin_amdgcn_readfirstlane(blockIdx.x * (kBlock<kVar> / 64u) + threadIdx.x / 64u);
}

// walk_sets' split / seg of the set starting at tile t0 (wave-uniform; t0 <
// ntiles), for the pixel side of the inverse: 64 when the set is 64 valid tiles
// of one tile row, k in 1..63 (kVarStraddle only) when its first k tiles end a
// tile row and the rest start the next, else 0 (per-lane stores).
template <unsigned kVar>
__device__ __forceinline__ uint32_t blocks_split(const TileGrid& g, uint32_t t0, uint32_t lane, const TilePos& p,
                                                 uint64_t& seg) {
    const bool whole = g.ntiles - t0 >= 64u;
    const uint32_t ty0 = t0 / g.tiles_x, tx0 = t0 - ty0 * g.tiles_x;
    const uint32_t k = g.tiles_x - tx0;  // tiles of the set left in tile row ty0
    if (!whole) {
        seg = 0;
        return 0u;
    }
    if (k >= 64u) {
        seg = p.base - 8u * static_cast<uint64_t>(lane);
        return 64u;
    }
    seg = static_cast<uint64_t>(ty0) * 8u * g.width + static_cast<uint64_t>(tx0) * 8u;
    if constexpr ((kVar & kVarStraddle) == 0) return 0u;
    return 64u - k <= g.tiles_x ? k : 0u;
}

}  // namespace

// ---------------------------------------------------------------------------
// Forward: uint8 frame -> int16 blocks.  kVar: the quotient bits (kVarFastDiv,
// kVarJpegQ), kVarNT, the workgroup size and kBlkStaged.
//
// The 64 results are packed two per dword as they are produced: the first of a
// pair to arrive waits as an int32 in the pair's register, the second packs
// both (one v_cvt_pk_i16_i32 per dword), so the 32 dwords of the block are all
// that stays live beside the shrinking P of the second pass.
//
// Stores.  direct: the lane's 128 B as eight 16-B stores (lanes at a 128-B
// stride).  kBlkStaged, whole sets: the lanes deposit their blocks in a
// wave-private 8 KiB LDS image and store it back as eight instructions of
// 1 KiB contiguous each.  Image: 16-B chunk c of lane l at l * 128 +
// 16 * (c ^ (l & 7)); ds_write_b128 works in groups of 8 contiguous lanes over
// 32 banks, ds_read_b128 in four 16-lane groups over 64 banks, and the XOR
// makes both conflict-free (the linear image is an 8-way conflict on every
// write).  LDS accesses of one wave execute in order, so there is no barrier.
// 8 KiB per wave = 32 KiB per 256-thread workgroup: 5 workgroups (20 waves) per
// CU by LDS, which is not the limit while the kernel holds more than 96 VGPRs
// (4 waves per SIMD = 16 per CU).
// ---------------------------------------------------------------------------
template <bool kNatural, unsigned kVar>
__global__ __launch_bounds__(kBlock<kVar>, 1) void fdct_blocks_kernel(const uint8_t* __restrict__ img,
                                                                   int16_t* __restrict__ blocks, TileGrid g,
                                                                   QParams qp) {
    constexpr bool kNT = (kVar & kVarNT) != 0;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blocks_wave<kVar>();
    if (wave >= blocks_nsets(g)) return;
    const uint32_t t0 = wave * 64u;
    const TilePos p = tile_pos(g, t0 + lane);
    if (!p.valid) return;

    const TSource<true, true> T(nullptr);
    RawTile<uint8_t> raw;
    raw.load(img + p.base, g.width);
    float x[8][8];
    raw.to_float(x, 128.0f);

    uint32_t w[32];
    fdct_tile(T, x, [&](auto v, float (&c)[8]) {
        unroll<8>([&](auto u) {
            constexpr int pos = v * 8 + u;
            constexpr int n = zigzag::element_of(kNatural, pos);
            constexpr int mate = zigzag::position_of(kNatural, n ^ 1);  // rows arrive in order, columns too
            const int32_t q =
                static_cast<int32_t>(quantise_biased_at<kVar, pos>(c[u], qp.q.v[pos], qp.r.v[pos]));
            if constexpr (mate > pos) {
                w[n / 2] = static_cast<uint32_t>(q);
            } else if constexpr ((n & 1) != 0) {
                w[n / 2] = pack_i16x2(static_cast<int32_t>(w[n / 2]), q);
            } else {
                w[n / 2] = pack_i16x2(q, static_cast<int32_t>(w[n / 2]));
            }
        });
    });

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
// Inverse: int16 blocks -> pixels (TOut float: R + 128, no clamp; uint8_t:
// clamp + truncate).  kVar: RowSink's bits (kVarNT, kVarLdsStore and
// kVarStraddle for fp32 rows), the workgroup size and kVarFullChain (every term
// of T kept; clear: its zero entries skipped).  The lane loads its
// block's 128 contiguous bytes; the halves sign-extend to fp32 straight into
// their row-major places.
// ---------------------------------------------------------------------------
template <typename TOut, bool kNatural, unsigned kVar>
__global__ __launch_bounds__(kBlock<kVar>, 1) void idct_blocks_kernel(const int16_t* __restrict__ blocks,
                                                                   TOut* __restrict__ out, TileGrid g, Mat64 q) {
    const TSource<true, (kVar & kVarFullChain) == 0> T(nullptr);
    float4* const slots = wave_slots<kVar>();
    const RowSink<kVar, TOut> sink{out, g.width, slots};
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blocks_wave<kVar>();
    if (wave >= blocks_nsets(g)) return;
    const uint32_t t0 = wave * 64u;
    const TilePos p = tile_pos(g, t0 + lane);
    uint64_t seg;
    const uint32_t split = blocks_split<kVar>(g, t0, lane, p, seg);
    if (!p.valid) return;

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
    idct_tile(T, d, [&](auto v, float (&row)[8]) {
        // add_matrix_scalar (utils_kernels.cu:29): R + 128
        unroll<8>([&](auto u) { row[u] = row[u] + 128.0f; });
        sink(v, p, split, seg, row);
    });
}

}  // namespace hpdct
