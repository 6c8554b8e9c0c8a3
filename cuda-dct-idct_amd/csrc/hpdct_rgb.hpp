// hpdct_rgb.hpp -- colour frames: interleaved uint8 RGB <-> three arrays of
// JPEG-style int16 coefficient blocks (Y, Cb, Cr), 4:4:4 or 4:2:0, one launch
// per direction.  The contract (include/hpdct.h has it in full):
//
//   forward, per pixel, int32:
//     Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//     Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
//     Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
//   4:2:0: a chroma sample is (a + b + c + d + 2) >> 2 over the 2x2 quad of the
//   converted per-pixel values.  Each component plane then goes through
//   fdct_blocks_kernel's arithmetic (hpdct_blocks.hpp): fdct_tile, the level
//   shift 128, quantise_biased_at, the truncating int16 convert.
//   inverse: each component through idct_blocks_kernel's arithmetic to uint8
//   (clamp + truncate), 4:2:0 chroma replicated 2x2, then with flooring shifts
//     R = clamp255(Y + (( 91881 (Cr-128) + 32768) >> 16))
//     G = clamp255(Y + ((-22554 (Cb-128) - 46802 (Cr-128) + 32768) >> 16))
//     B = clamp255(Y + ((116130 (Cb-128) + 32768) >> 16))
//
// Mapping: one lane per unit, 64 units in row-major unit order per wave.  A unit
// is an 8x8 pixel tile (4:4:4: three blocks) or a 16x16 MCU (4:2:0: four Y
// blocks, one Cb, one Cr).  The lane walks the unit's Y tiles in a run-time
// loop (the transform's code exists once per table): per tile 8 rows x 24 B of
// RGB (three 8-B loads a row; the next tile's are issued before the current
// one's arithmetic), the conversion, the transform, the block.  The chroma of
// the unit waits as packed bytes (32 VGPRs, never as floats); a second
// run-time loop transforms Cb then Cr under the chroma table.
//
// Block stores (forward).  Block index of a chroma tile = unit index, so the
// 64 chroma blocks of a whole set are one contiguous 8 KiB run whatever the
// width, and so are the Y blocks of 4:4:4: fdct_blocks_kernel's XOR-swizzled
// LDS image, eight store instructions of 1 KiB each.  4:2:0 Y: when the set's
// 64 MCUs lie in one MCU row, each of its two Y tile rows is one 16 KiB run of
// 128 blocks (lane l owns blocks 2l and 2l+1); the image is 16 KiB, deposited
// over the two tiles of the row and stored as sixteen 1 KiB instructions.  16-B
// chunk c of block b sits at 128 b + 16 (c ^ s), s = b & 7 (8 KiB image) or
// (b >> 1) & 7 (16 KiB image): the eight lanes of a ds_write_b128 group hit
// eight different 16-B columns, the sixteen lanes of a ds_read_b128 group read
// two whole 128-B blocks.  Other sets (a ragged last one, 4:2:0 Y sets over two
// MCU rows) store their blocks straight from the lane.
//
// Frames of any size and row pitch (hpdct_forward_rgb_frame / _inverse_rgb_frame).
// The unit grid covers the frame padded to whole units, RgbGrid carries the row
// pitch and the frame's own height and width.  Whole units with an 8-byte
// aligned base and pitch run the kernels as above; anything else runs the
// kRgbClip instantiation: a tile cut by the frame's edge (or every tile, when
// base or pitch is not 8-byte aligned) is loaded byte by byte from clamped
// coordinates (the last column and row repeated) and stored byte by byte below
// 3 * width, rows beyond the height not at all.  Unit and block indices, and so
// the staged block stores, are the same in both.
#pragma once

#include "hpdct_blocks.hpp"

namespace hpdct {

namespace {

// 8 rows x 24 B of interleaved RGB: the 8x8 pixel tile at p (8-byte aligned)
struct RawRgb {
    uint2 r[8][3];
    __device__ __forceinline__ void load(const uint8_t* __restrict__ p, uint64_t pitch) {
        unroll<8>([&](auto i) {
            const uint2* src = reinterpret_cast<const uint2*>(p + i * pitch);
            r[i][0] = src[0];
            r[i][1] = src[1];
            r[i][2] = src[2];
        });
    }
    // The same tile for any base and pitch, edge-replicated: the tile's first
    // pixel is (y0, x0) of the padded frame, byte kB of row kI comes from row
    // min(y0 + kI, h - 1), pixel min(x0 + kB / 3, w - 1) of the h x w frame.
    // Byte loads (kRgbClip: edge units, and every unit of an unaligned frame).
    __device__ __forceinline__ void load_clamped(const uint8_t* __restrict__ rgb, uint64_t pitch, uint64_t h,
                                                 uint64_t w, uint64_t y0, uint64_t x0) {
        const uint64_t xc = x0 < w ? x0 : w - 1u;
        uint32_t xo[8];  // byte offset of pixel j from pixel xc
        unroll<8>([&](auto j) { xo[j] = x0 + j < w ? 3u * j : 3u * static_cast<uint32_t>(w - 1u - xc); });
        unroll<8>([&](auto i) {
            const uint64_t y = y0 + i < h ? y0 + i : h - 1u;
            const uint8_t* const row = rgb + y * pitch + 3u * xc;
            uint32_t px[8];  // B << 16 | G << 8 | R
            unroll<8>([&](auto j) {
                const uint8_t* const p = row + xo[j];
                px[j] = static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 8) |
                        (static_cast<uint32_t>(p[2]) << 16);
            });
            r[i][0] = make_uint2(px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16));
            r[i][1] = make_uint2((px[2] >> 16) | (px[3] << 8), px[4] | (px[5] << 24));
            r[i][2] = make_uint2((px[5] >> 8) | (px[6] << 16), (px[6] >> 16) | (px[7] << 8));
        });
    }
    // byte kB (0..23) of row kI
    template <int kI, int kB>
    __device__ __forceinline__ int32_t byte() const {
        constexpr int d = kB / 4;
        const uint32_t w = (d & 1) ? r[kI][d / 2].y : r[kI][d / 2].x;
        return static_cast<int32_t>((w >> (8 * (kB % 4))) & 0xffu);
    }
};

__device__ __forceinline__ int32_t rgb_y(int32_t r, int32_t g, int32_t b) {
    return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
}
__device__ __forceinline__ int32_t rgb_cb(int32_t r, int32_t g, int32_t b) {
    return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
}
__device__ __forceinline__ int32_t rgb_cr(int32_t r, int32_t g, int32_t b) {
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}
__device__ __forceinline__ int32_t clamp255(int32_t v) { return min(max(v, 0), 255); }

// fdct_tile (hpdct_tile.hpp) fed one input row at a time: the same 128 FMA
// chains, each in its own order over i, so the same bits; the first pass's
// chains advance together as row i arrives instead of one column at a time.
// Only one row of X is live beside P, which is what lets the conversion run
// row by row in front of the transform (64 fewer VGPRs at the peak).
template <int kI, typename TS>
__device__ __forceinline__ void fdct_feed_row(const TS& T, const float (&xr)[8], float (&p)[8][8]) {
    // P = T . X   (main_newAppr.cu:193-197): P[v][col] = sum_i T[v][i] X[i][col]
    unroll<8>([&](auto v) {
        unroll<8>([&](auto col) {
            p[v][col] = T.template mac<v * 8 + kI>(xr[col], kI == 0 ? 0.0f : p[v][col]);
        });
    });
}
template <typename TS, typename Emit>
__device__ __forceinline__ void fdct_finish(const TS& T, const float (&p)[8][8], Emit&& emit) {
    // C = P . T^T (main_newAppr.cu:206-209): C[v][u] = sum_i P[v][i] T[u][i]
    unroll<8>([&](auto v) {
        float c[8];
        unroll<8>([&](auto u) {
            float s = 0.0f;
            unroll<8>([&](auto i) { s = T.template mac<u * 8 + i>(p[v][i], s); });
            c[u] = s;
        });
        emit(v, c);
    });
}

// The chroma of a row is wanted only after the Y transform, and hipcc sinks its
// whole computation there, keeping every extracted byte of the tile alive
// across the transform (some 190 VGPRs).  An empty volatile asm on the packed
// results keeps the computation where it is written.
__device__ __forceinline__ void pin_here(uint32_t& a, uint32_t& b) { asm volatile("" : "+v"(a), "+v"(b)); }

// Converts one 8x8 pixel tile row by row: on_row(i, Y - 128) (exact integers
// in fp32) and the tile's chroma as packed bytes.  4:4:4: cb[2 i + h] holds pixels 4h..4h+3 of
// row i (16 dwords).  4:2:0: cb[i] holds the four 2x2 averages of rows 2i,
// 2i+1 (4 dwords, the tile's quadrant of the MCU's chroma tile).
template <bool k420, typename OnRow>
__device__ __forceinline__ void rgb_convert_tile(const RawRgb& raw, OnRow&& on_row, uint32_t (&cb)[k420 ? 4 : 16],
                                                 uint32_t (&cr)[k420 ? 4 : 16]) {
    uint32_t hb[4], hr[4];  // 4:2:0: the even row's horizontal pair sums
    unroll<8>([&](auto i) {
        uint32_t b8[8], r8[8];
        float xr[8];
        unroll<8>([&](auto j) {
            const int32_t r = raw.template byte<i, 3 * j>(), g = raw.template byte<i, 3 * j + 1>(),
                          b = raw.template byte<i, 3 * j + 2>();
            xr[j] = static_cast<float>(rgb_y(r, g, b)) - 128.0f;
            b8[j] = static_cast<uint32_t>(rgb_cb(r, g, b));
            r8[j] = static_cast<uint32_t>(rgb_cr(r, g, b));
        });
        on_row(i, xr);
        // keeps the next rows' conversion from being scheduled ahead of this row's FMAs
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (!k420) {
            unroll<2>([&](auto h) {
                cb[2 * i + h] = b8[4 * h] | (b8[4 * h + 1] << 8) | (b8[4 * h + 2] << 16) | (b8[4 * h + 3] << 24);
                cr[2 * i + h] = r8[4 * h] | (r8[4 * h + 1] << 8) | (r8[4 * h + 2] << 16) | (r8[4 * h + 3] << 24);
                pin_here(cb[2 * i + h], cr[2 * i + h]);
            });
        } else if constexpr (i % 2 == 0) {
            unroll<4>([&](auto j) {
                hb[j] = b8[2 * j] + b8[2 * j + 1];
                hr[j] = r8[2 * j] + r8[2 * j + 1];
                pin_here(hb[j], hr[j]);
            });
        } else {
            uint32_t qb[4], qr[4];
            unroll<4>([&](auto j) {
                qb[j] = (hb[j] + b8[2 * j] + b8[2 * j + 1] + 2) >> 2;
                qr[j] = (hr[j] + r8[2 * j] + r8[2 * j + 1] + 2) >> 2;
            });
            cb[i / 2] = qb[0] | (qb[1] << 8) | (qb[2] << 16) | (qb[3] << 24);
            cr[i / 2] = qr[0] | (qr[1] << 8) | (qr[2] << 16) | (qr[3] << 24);
            pin_here(cb[i / 2], cr[i / 2]);
        }
    });
}

// The dword of a unit's packed chroma tile holding columns 4 kH .. 4 kH + 3 of
// row kRow.  4:4:4: as rgb_convert_tile leaves it.  4:2:0: the quadrants in the
// order the Y tiles are walked (k = 2 r + c), four dwords each.
template <bool k420>
constexpr int chroma_dword(int row, int h) {
    return k420 ? 4 * (2 * (row / 4) + h) + row % 4 : 2 * row + h;
}

// ---- block stores ----------------------------------------------------------
template <bool kNT>
__device__ __forceinline__ void rgb_store_direct(char* out, uint64_t block, const uint32_t (&w)[32]) {
    uint4* const dst = reinterpret_cast<uint4*>(out + block * 128u);
    unroll<8>([&](auto c) { st16<kNT>(dst + c, make_uint4(w[4 * c], w[4 * c + 1], w[4 * c + 2], w[4 * c + 3])); });
}
// block b of the wave's LDS image (kPair: the 16 KiB image, b = 2 lane + c)
template <bool kPair>
__device__ __forceinline__ void rgb_stage_deposit(char* image, uint32_t b, const uint32_t (&w)[32]) {
    const uint32_t s = kPair ? (b >> 1) & 7u : b & 7u;
    const uint32_t wr = b * 128u + 16u * s;
    unroll<8>([&](auto c) {
        *reinterpret_cast<uint4*>(image + (wr ^ (16u * c))) =
            make_uint4(w[4 * c], w[4 * c + 1], w[4 * c + 2], w[4 * c + 3]);
    });
}
// the image's first kInstr KiB to run, 1 KiB contiguous per store instruction.
// The pick-up reads other lanes' deposits and the next deposit overwrites what
// other lanes pick up: the compiler may move neither across.
template <bool kNT, bool kPair, int kInstr>
__device__ __forceinline__ void rgb_stage_flush(const char* image, char* run, uint32_t lane) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    unroll<kInstr>([&](auto j) {
        // chunk j * 64 + lane of the run: chunk lane & 7 of block j * 8 + lane / 8
        const uint32_t b = 8u * j + (lane >> 3);
        const uint32_t s = kPair ? (b >> 1) & 7u : b & 7u;
        const uint4 v = *reinterpret_cast<const uint4*>(image + b * 128u + 16u * ((lane & 7u) ^ s));
        st16<kNT>(reinterpret_cast<uint4*>(run + 1024u * j + 16u * lane), v);
    });
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace

// fdct_blocks_kernel's second pass, quantiser and packing of one tile: P -> the
// block's 32 dwords.  A macro over the kernel's own QParams argument: handing
// the QParams to a device function by reference makes hipcc keep the quotient
// operands in scratch memory (hpdct_kernels_impl.hpp).
#define HPDCT_RGB_BLOCK_OF(kQuot, kNatural, T, qp, p, w)                                                     \
    fdct_finish(T, p, [&](auto v, float (&c)[8]) {                                                          \
        unroll<8>([&](auto u) {                                                                             \
            constexpr int pos = v * 8 + u;                                                                  \
            constexpr int n = zigzag::element_of(kNatural, pos);                                            \
            constexpr int mate = zigzag::position_of(kNatural, n ^ 1);                                      \
            const int32_t q =                                                                               \
                static_cast<int32_t>(quantise_biased_at<(kQuot), pos>(c[u], (qp).q.v[pos], (qp).r.v[pos])); \
            if constexpr (mate > pos) {                                                                     \
                w[n / 2] = static_cast<uint32_t>(q);                                                        \
            } else if constexpr ((n & 1) != 0) {                                                            \
                w[n / 2] = pack_i16x2(static_cast<int32_t>(w[n / 2]), q);                                   \
            } else {                                                                                        \
                w[n / 2] = pack_i16x2(q, static_cast<int32_t>(w[n / 2]));                                   \
            }                                                                                               \
        });                                                                                                 \
    })

// ---------------------------------------------------------------------------
// Forward.  kVar: kRgb420, the luma quotient bits (kVarFastDiv, kVarJpegQ),
// kRgbChromaFastDiv, kVarNT, kBlkStaged, kRgbClip and the workgroup size.
// kRgbClip: the unit grid covers the frame padded to whole units, and a tile
// that the frame's edge cuts (or every tile, when base or pitch is not 8-byte
// aligned) is loaded by RawRgb::load_clamped; a tile inside the frame keeps
// the 8-byte loads.  Everything behind the load is the same code.
// ---------------------------------------------------------------------------
template <bool kNatural, unsigned kVar>
__global__ __launch_bounds__(kBlock<kVar>, (kVar & kRgb420) != 0 ? 2 : 3) void fdct_rgb_kernel(const uint8_t* __restrict__ rgb,
                                                                int16_t* __restrict__ yb, int16_t* __restrict__ cbb,
                                                                int16_t* __restrict__ crb, RgbGrid g, QParams ql,
                                                                QParams qc) {
    constexpr bool k420 = (kVar & kRgb420) != 0;
    constexpr bool kNT = (kVar & kVarNT) != 0;
    constexpr bool kStaged = (kVar & kBlkStaged) != 0;
    constexpr bool kClip = (kVar & kRgbClip) != 0;
    constexpr unsigned kQL = kVar & (kVarFastDiv | kVarJpegQ);
    constexpr unsigned kQC = (kVar & kRgbChromaFastDiv) != 0 ? kVarFastDiv : 0u;
    constexpr uint32_t kSide = k420 ? 16u : 8u;  // pixels per unit side
    constexpr int kYTiles = k420 ? 4 : 1;

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blocks_wave<kVar>();
    if (wave >= g.nunits / 64u + (g.nunits % 64u != 0u)) return;
    const uint32_t u0 = wave * 64u;  // wave-uniform
    if (u0 + lane >= g.nunits) return;
    const uint32_t unit = u0 + lane;
    const uint32_t uy = unit / g.units_x, ux = unit - uy * g.units_x;
    const uint64_t pitch = g.pitch;  // 64-bit byte offsets throughout: 3 H W passes 2^32
    const uint8_t* const src = rgb + static_cast<uint64_t>(uy) * kSide * pitch + static_cast<uint64_t>(ux) * kSide * 3u;
    const bool aligned8 = !kClip || ((reinterpret_cast<uintptr_t>(rgb) | pitch) & 7u) == 0u;  // wave-uniform
    // Y tile (tr, tc) of the unit
    auto load_tile = [&](RawRgb& raw, uint32_t tr, uint32_t tc) {
        const uint8_t* const p = src + static_cast<uint64_t>(tr) * 8u * pitch + tc * 24u;
        if constexpr (kClip) {
            const uint64_t y0 = static_cast<uint64_t>(uy) * kSide + 8u * tr, x0 = static_cast<uint64_t>(ux) * kSide + 8u * tc;
            if (!aligned8 || y0 + 8u > g.height || x0 + 8u > g.width) {
                raw.load_clamped(rgb, pitch, g.height, g.width, y0, x0);
                return;
            }
        }
        raw.load(p, pitch);
    };
    // every lane of the wave is live (the staged stores need all 64)
    const bool whole = g.nunits - u0 >= 64u;

    __shared__ uint4 stage[kStaged ? kBlock<kVar> / 64u : 1u][kStaged ? (k420 ? 1024 : 512) : 1];
    char* const image = reinterpret_cast<char*>(stage[kStaged ? __builtin_amdgcn_readfirstlane(threadIdx.x / 64u) : 0u]);

    // kFrameDct: the exact DCT's matrix.  The 3-op quotient holds there (|C| < 4096), the per-position forms do not
    constexpr bool kDct = (kVar & kFrameDct) != 0;
    static_assert(!kDct || (kVar & kVarJpegQ) == 0, "the per-position quotient forms are proven for HpApprDCT only");
    const TSource<true, true, kDct> T(nullptr);
    uint32_t cb[16] = {}, cr[16] = {};  // the unit's chroma tile, chroma_dword<k420>
    char* const yout = reinterpret_cast<char*>(yb);

    if constexpr (!k420) {
        RawRgb raw;
        load_tile(raw, 0u, 0u);
        float p[8][8];
        rgb_convert_tile<false>(raw, [&](auto i, const float (&xr)[8]) { fdct_feed_row<i>(T, xr, p); }, cb, cr);
        uint32_t w[32];
        HPDCT_RGB_BLOCK_OF(kQL, kNatural, T, ql, p, w);
        if (kStaged && whole) {
            rgb_stage_deposit<false>(image, lane, w);
            rgb_stage_flush<kNT, false, 8>(image, yout + static_cast<uint64_t>(u0) * 128u, lane);
        } else {
            rgb_store_direct<kNT>(yout, unit, w);
        }
    } else {
        // 4:2:0: Y tile k = 2 r + c of the MCU is tile (2 uy + r, 2 ux + c) of the Y plane
        const uint32_t tiles_x = 2u * g.units_x;
        const uint32_t uy0 = u0 / g.units_x, ux0 = u0 - uy0 * g.units_x;  // the set's first MCU
        const bool one_row = whole && g.units_x - ux0 >= 64u;
        RawRgb cur;
        load_tile(cur, 0u, 0u);
#pragma clang loop unroll(disable)
        for (int k = 0; k < kYTiles; ++k) {
            const uint32_t r = static_cast<uint32_t>(k) >> 1, c = static_cast<uint32_t>(k) & 1u;
            if constexpr (kDct) {
                // The DCT's first pass has no zero term and seven constants where HpApprDCT has four: with the next
                // tile's 48 registers live across it the kernel passes its 256 VGPRs and spills to scratch (4-8
                // VGPRs).  So under the DCT a tile is asked for when its turn comes, not one tile ahead; the CU's
                // other waves cover the wait.
                if (k != 0) load_tile(cur, r, c);
            }
            RawRgb nxt = cur;
            if constexpr (!kDct) {
                if (k + 1 < kYTiles)
                    load_tile(nxt, static_cast<uint32_t>((k + 1) >> 1), static_cast<uint32_t>((k + 1) & 1));
            }
            float p[8][8];
            uint32_t nb[4], nr[4];
            rgb_convert_tile<true>(cur, [&](auto i, const float (&xr)[8]) { fdct_feed_row<i>(T, xr, p); }, nb, nr);
            // quadrant k to its place: the array moves up by one quadrant per tile
            unroll<12>([&](auto i) {
                cb[i] = cb[i + 4];
                cr[i] = cr[i + 4];
            });
            unroll<4>([&](auto i) {
                cb[12 + i] = nb[i];
                cr[12 + i] = nr[i];
            });
            uint32_t w[32];
            HPDCT_RGB_BLOCK_OF(kQL, kNatural, T, ql, p, w);
            if (kStaged && one_row) {
                rgb_stage_deposit<true>(image, 2u * lane + c, w);
                if (c == 1u) {
                    const uint64_t t0 = static_cast<uint64_t>(2u * uy0 + r) * tiles_x + 2u * ux0;
                    rgb_stage_flush<kNT, true, 16>(image, yout + t0 * 128u, lane);
                }
            } else {
                rgb_store_direct<kNT>(yout, static_cast<uint64_t>(2u * uy + r) * tiles_x + 2u * ux + c, w);
            }
            cur = nxt;
        }
    }

    // Cb, then Cr: chroma block index = unit index
    uint32_t cq[16];
    unroll<16>([&](auto i) { cq[i] = cb[i]; });
#pragma clang loop unroll(disable)
    for (int comp = 0; comp < 2; ++comp) {
        float p[8][8];
        unroll<8>([&](auto i) {
            float xr[8];
            unroll<8>([&](auto j) { xr[j] = byte_f32(cq[chroma_dword<k420>(i, j / 4)], j % 4) - 128.0f; });
            fdct_feed_row<i>(T, xr, p);
        });
        uint32_t w[32];
        HPDCT_RGB_BLOCK_OF(kQC, kNatural, T, qc, p, w);
        char* const out = reinterpret_cast<char*>(comp == 0 ? cbb : crb);
        if (kStaged && whole) {
            rgb_stage_deposit<false>(image, lane, w);
            rgb_stage_flush<kNT, false, 8>(image, out + static_cast<uint64_t>(u0) * 128u, lane);
        } else {
            rgb_store_direct<kNT>(out, unit, w);
        }
        unroll<16>([&](auto i) { cq[i] = cr[i]; });
    }
}

// ---------------------------------------------------------------------------
// Inverse.  kVar: kRgb420, kVarNT (the RGB stores), kRgbClip, kVarFullChain
// (as idct_blocks_kernel) and the workgroup size.  kRgbClip: rows at or beyond the frame's height are not stored, and a
// row that the width cuts (or every row, when base or pitch is not 8-byte
// aligned) is stored byte by byte, below 3 * width only.
// The chroma tiles first, kept as packed uint8 (clamp + truncate: the values
// hpdct_inverse_blocks gives for HPDCT_U8), then each Y tile's RGB rows: three
// 8-B stores per row and lane.
// ---------------------------------------------------------------------------
#define HPDCT_RGB_TILE_OF(kNatural, T, q, src, emit)                                                                  \
    do {                                                                                                              \
        uint4 rr[8];                                                                                                  \
        unroll<8>([&](auto c) { rr[c] = (src)[c]; });                                                                 \
        float d[8][8];                                                                                                \
        unroll<32>([&](auto k) {                                                                                      \
            constexpr int p0 = zigzag::position_of(kNatural, 2 * k), p1 = zigzag::position_of(kNatural, 2 * k + 1);   \
            const uint32_t word = dword_of<k % 4>(rr[k / 4]);                                                         \
            d[p0 / 8][p0 % 8] =                                                                                       \
                static_cast<float>(static_cast<int32_t>(static_cast<int16_t>(word & 0xffffu))) * (q).v[p0];           \
            d[p1 / 8][p1 % 8] = static_cast<float>(static_cast<int32_t>(word) >> 16) * (q).v[p1];                     \
        });                                                                                                           \
        idct_tile(T, d, emit);                                                                                        \
    } while (0)

template <bool kNatural, unsigned kVar>
__global__ __launch_bounds__(kBlock<kVar>, 1) void idct_rgb_kernel(const int16_t* __restrict__ yb,
                                                                const int16_t* __restrict__ cbb,
                                                                const int16_t* __restrict__ crb,
                                                                uint8_t* __restrict__ rgb, RgbGrid g, Mat64 ql,
                                                                Mat64 qc) {
    constexpr bool k420 = (kVar & kRgb420) != 0;
    constexpr bool kNT = (kVar & kVarNT) != 0;
    constexpr bool kClip = (kVar & kRgbClip) != 0;
    constexpr uint32_t kSide = k420 ? 16u : 8u;
    constexpr int kYTiles = k420 ? 4 : 1;

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blocks_wave<kVar>();
    if (wave >= g.nunits / 64u + (g.nunits % 64u != 0u)) return;
    if (wave * 64u + lane >= g.nunits) return;
    const uint32_t unit = wave * 64u + lane;
    const uint32_t uy = unit / g.units_x, ux = unit - uy * g.units_x;
    const uint64_t pitch = g.pitch;
    const bool aligned8 = !kClip || ((reinterpret_cast<uintptr_t>(rgb) | pitch) & 7u) == 0u;  // wave-uniform
    uint8_t* const dst = rgb + static_cast<uint64_t>(uy) * kSide * pitch + static_cast<uint64_t>(ux) * kSide * 3u;
    const uint32_t tiles_x = (k420 ? 2u : 1u) * g.units_x;

    // kVarFullChain: a table under which q * Q or a partial sum may overflow; every term of T kept
    // kFrameDct: the exact DCT's matrix (no zero: every term kept), and each component is R + 128.5f, clamped and
    // truncated: round half up, as JPEG decoders do, in place of the reference's R + 128 truncated
    constexpr bool kDct = (kVar & kFrameDct) != 0;
    constexpr float kShift = kDct ? 128.5f : 128.0f;
    const TSource<true, (kVar & kVarFullChain) == 0, kDct> T(nullptr);
    // row v of a chroma tile: dwords 2 v (columns 0..3) and 2 v + 1
    uint32_t cb[16] = {}, cr[16] = {};
#pragma clang loop unroll(disable)
    for (int comp = 0; comp < 2; ++comp) {
        const uint4* const src = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(comp == 0 ? cbb : crb) +
                                                                static_cast<uint64_t>(unit) * 128u);
        unroll<16>([&](auto i) { cb[i] = cr[i]; });
        auto keep = [&](auto v, float (&row)[8]) {
            unroll<8>([&](auto u) { row[u] = row[u] + kShift; });
            cr[2 * v] = pack_u8x4(row[0], row[1], row[2], row[3]);
            cr[2 * v + 1] = pack_u8x4(row[4], row[5], row[6], row[7]);
        };
        HPDCT_RGB_TILE_OF(kNatural, T, qc, src, keep);
    }

#pragma clang loop unroll(disable)
    for (int k = 0; k < kYTiles; ++k) {
        const uint32_t r = static_cast<uint32_t>(k) >> 1, c = static_cast<uint32_t>(k) & 1u;
        // the tile's first pixel in the padded frame; kRgbClip: rows and bytes of the tile inside the frame
        const uint64_t y0 = static_cast<uint64_t>(uy) * kSide + 8u * r, x0 = static_cast<uint64_t>(ux) * kSide + 8u * c;
        uint32_t live_rows = 8u, live_bytes = 24u;
        if constexpr (kClip) {
            if (y0 >= g.height || x0 >= g.width) continue;  // a tile of padding only
            live_rows = static_cast<uint32_t>(g.height - y0 < 8u ? g.height - y0 : 8u);
            live_bytes = 3u * static_cast<uint32_t>(g.width - x0 < 8u ? g.width - x0 : 8u);
        }
        const bool whole_rows = aligned8 && live_bytes == 24u;
        const uint64_t t = static_cast<uint64_t>((k420 ? 2u : 1u) * uy + r) * tiles_x + (k420 ? 2u : 1u) * ux + c;
        const uint4* const src = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(yb) + t * 128u);
        // 4:2:0: the tile's quadrant of the chroma tiles, rows 4 r .. 4 r + 3, columns 4 c .. 4 c + 3
        uint32_t qb[4], qr[4];
        if constexpr (k420) {
            unroll<4>([&](auto i) {
                const uint32_t b0 = c ? cb[2 * i + 1] : cb[2 * i], b1 = c ? cb[2 * (4 + i) + 1] : cb[2 * (4 + i)];
                const uint32_t r0 = c ? cr[2 * i + 1] : cr[2 * i], r1 = c ? cr[2 * (4 + i) + 1] : cr[2 * (4 + i)];
                qb[i] = r ? b1 : b0;
                qr[i] = r ? r1 : r0;
            });
        }
        uint8_t* const out = dst + static_cast<uint64_t>(r) * 8u * pitch + c * 24u;
        auto emit_rgb = [&](auto v, float (&row)[8]) {
            uint32_t px[24];
            unroll<8>([&](auto u) {
                const int32_t y = static_cast<int32_t>(min(cvt_u32_sat(row[u] + kShift), 255u));
                const uint32_t wb = k420 ? qb[v / 2] : cb[2 * v + u / 4], wr = k420 ? qr[v / 2] : cr[2 * v + u / 4];
                constexpr int sh = 8 * (k420 ? u / 2 : u % 4);
                const int32_t b = static_cast<int32_t>((wb >> sh) & 0xffu) - 128;
                const int32_t rr2 = static_cast<int32_t>((wr >> sh) & 0xffu) - 128;
                px[3 * u] = static_cast<uint32_t>(clamp255(y + ((91881 * rr2 + 32768) >> 16)));
                px[3 * u + 1] = static_cast<uint32_t>(clamp255(y + ((-22554 * b - 46802 * rr2 + 32768) >> 16)));
                px[3 * u + 2] = static_cast<uint32_t>(clamp255(y + ((116130 * b + 32768) >> 16)));
            });
            if constexpr (kClip) {
                if (static_cast<uint32_t>(v) >= live_rows) return;
                if (!whole_rows) {
                    uint8_t* const pb = out + v * pitch;
                    unroll<24>([&](auto b) {
                        if (static_cast<uint32_t>(b) < live_bytes) pb[b] = static_cast<uint8_t>(px[b]);
                    });
                    return;
                }
            }
            uint32_t o[6];
            unroll<6>([&](auto d) {
                o[d] = px[4 * d] | (px[4 * d + 1] << 8) | (px[4 * d + 2] << 16) | (px[4 * d + 3] << 24);
            });
            uint2* const p = reinterpret_cast<uint2*>(out + v * pitch);
            st<kNT>(p, make_uint2(o[0], o[1]));
            st<kNT>(p + 1, make_uint2(o[2], o[3]));
            st<kNT>(p + 2, make_uint2(o[4], o[5]));
        };
        HPDCT_RGB_TILE_OF(kNatural, T, ql, src, emit_rgb);
    }
}

}  // namespace hpdct
