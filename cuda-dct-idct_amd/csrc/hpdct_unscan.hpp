// hpdct_unscan.hpp -- the baseline-JPEG entropy decoder (hpdct_decode_scan): the
// bytes of one interleaved Huffman scan -> int16 coefficient blocks, the inverse
// of hpdct_scan.hpp under the same tables, geometry and interval rules.
//
// The walk of ONE restart interval (byte fetch and unstuffing, symbol decode,
// the index and DC checks, the status, the zero fill) is plain C++ for host and
// device alike: unscan::walk_interval.  The kernel is a wrapper that gives each
// lane an interval, stages the tables and the lane's block row in LDS and calls
// it; tests/tools/asan_unscan_check.cpp calls the very same function on the CPU
// under ASan + UBSan over the corrupt corpus.  The input is untrusted:
//   - the walk's trip count is bounded by the interval's block count alone (at
//     most 64 symbol steps per block), never by "while bits remain";
//   - every byte fetch is guarded by the interval's end;
//   - every store goes to the block the block counter names; the one index
//     that comes from decoded data, the coefficient's, is checked <= 63 first.
//
// Up to four launches, one chain:
//   1. count   (no offsets given) one wave per 4096-byte chunk counts the FF Dn
//              pairs whose first byte the chunk holds;
//   2. rank    one workgroup: the counts become ranks (exclusive sum, in place),
//              *info is initialised (always launched);
//   3. place   (no offsets given) the same search again: the position of the
//              j-th marker goes to the workspace for j < intervals, the rank
//              within a wave by ballot and popcount; the numbering is checked;
//   4. decode  one lane per interval.
// No workgroup waits on another; the only atomics are integer sums.
//
// unscan::fill_decode is the one builder of a decode table, for Annex K's
// constants (make_decode_tables, at compile time) and a caller's blob
// (huff::fill_blob, hpdct_huffman.hpp) alike; launch_unscan is the one launch
// path for both.  The decode kernel keeps an instantiation for each: the
// caller's tables are untrusted and cost masks in the walk, and what those
// would cost the Annex K path is unmeasured.
#pragma once

#include <stdint.h>

#include <type_traits>

#include "hpdct.h"
#include "hpdct_kernels.h"
#include "hpdct_scan.hpp"
#include "hpdct_zigzag.h"

#if defined(__HIPCC__)
#define HPDCT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HPDCT_HD inline
#endif

namespace hpdct {
namespace unscan {

// the codes of an interval's status (hpdct.h): status = code + 256 * block
enum : uint32_t { kOk = 0, kRange = 1, kMarker = 2, kEnd = 3, kCode = 4, kIndex = 5, kDc = 6, kTail = 7, kMissing = 8 };

// The four Annex K tables as the walk reads them, kind as scan::spec_of (0 DC
// luma, 1 AC luma, 2 DC chroma, 3 AC chroma).  look[peek >> 8] = (length << 8) |
// symbol for the codes of 8 bits or fewer, 0 for the prefix of a longer one;
// those are found canonically: the first length l in 9..16 with
// (peek >> (16 - l)) <= maxcode[l] has the symbol vals[code + valoff[l]]
// (maxcode[l] = -1: no code of that length).
struct DecodeTables {
    uint16_t look[4][256];
    int32_t maxcode[4][18];
    int32_t valoff[4][18];
    uint8_t vals[4][164];
};
constexpr int kTableWords = static_cast<int>(sizeof(DecodeTables) / 4u);
static_assert(sizeof(DecodeTables) == 4u * kTableWords && sizeof(DecodeTables) == 3280u, "tables are packed");
// table `kind` of Tab (DecodeTables, or DecodeTablesWide below: they differ in the width of vals), for Annex K's
// specs at compile time and a caller's at run time (huff::fill_blob); a lookup slot no code of 8 bits or fewer
// covers keeps what it had (0)
template <class Tab>
constexpr void fill_decode(const hpdct_huffman_spec& s, Tab& t, int kind) {
    int code = 0, k = 0;
    for (int l = 0; l < 18; ++l) t.maxcode[kind][l] = -1, t.valoff[kind][l] = 0;
    for (int len = 1; len <= 16; ++len) {
        t.valoff[kind][len] = k - code;
        for (int i = 0; i < s.bits[len - 1]; ++i) {
            if (len <= 8)
                for (int f = 0; f < (1 << (8 - len)); ++f)
                    t.look[kind][(code << (8 - len)) | f] = static_cast<uint16_t>((len << 8) | s.vals[k]);
            t.vals[kind][k] = s.vals[k];
            ++k, ++code;
        }
        if (s.bits[len - 1] != 0) t.maxcode[kind][len] = code - 1;
        code <<= 1;
    }
}
constexpr DecodeTables make_decode_tables() {
    DecodeTables t{};
    for (int kind = 0; kind < 4; ++kind) fill_decode(scan::spec_of(kind), t, kind);
    return t;
}

// The same tables for a caller's DHT (hpdct_huffman.hpp fills them): room for
// 256 symbols a table.  Their contents are the caller's data, so the walk masks
// the one index it forms from them (kUntrusted below) and clamps their lengths.
struct DecodeTablesWide {
    uint16_t look[4][256];
    int32_t maxcode[4][18];
    int32_t valoff[4][18];
    uint8_t vals[4][256];
};
static_assert(sizeof(DecodeTablesWide) == 3648u, "tables are packed");
// what hpdct_huffman_prepare writes and the *_tables calls read: the coder's
// entries (scan::CodeTables), then the decoder's tables
struct HuffBlob {
    scan::CodeTables code;
    DecodeTablesWide dec;
};
static_assert(sizeof(HuffBlob) == 5824u && sizeof(HuffBlob) % 16u == 0u, "the blob is packed");
template <class Tab>
constexpr bool kUntrusted = std::is_same_v<Tab, DecodeTablesWide>;

// zigzag::kOrder as the device constant the decoders stage into LDS (kUnscanOrder, kUnsplitOrder)
struct ZigzagOrder {
    uint8_t v[64];
};
constexpr ZigzagOrder make_zigzag_order() {
    ZigzagOrder o{};
    for (int n = 0; n < 64; ++n) o.v[n] = zigzag::kOrder[n];
    return o;
}

// The workspace: the byte position of the j-th marker for j < intervals
// (uint64), then a uint64 per 4096-byte chunk of the scan (its marker count,
// then its rank); both parts 16-byte multiples.
constexpr uint32_t kChunkBytes = 4096;
constexpr uint64_t chunks_of(uint64_t bytes) { return bytes == 0u ? 1u : (bytes + kChunkBytes - 1u) / kChunkBytes; }
constexpr uint64_t marker_words(uint64_t intervals) { return (intervals + 1u) / 2u * 2u; }
constexpr int64_t workspace_bytes(uint64_t intervals, uint64_t bytes) {
    return static_cast<int64_t>(8u * (marker_words(intervals) + (chunks_of(bytes) + 1u) / 2u * 2u));
}

// a restart marker at p: FF D0..D7, both bytes inside the scan
HPDCT_HD bool marker_at(const uint8_t* scan, uint64_t p, uint64_t bytes) {
    return p + 1u < bytes && scan[p] == 0xffu && (scan[p + 1u] & 0xf8u) == 0xd0u;
}

// Where interval i's bytes are, [lo, hi): returns kOk, or kRange / kMissing
// (lo = hi = 0 then).  offs: the caller's table, untrusted.
HPDCT_HD uint32_t bounds_given(const uint64_t* offs, uint64_t i, uint64_t intervals, uint64_t bytes, uint64_t& lo,
                               uint64_t& hi) {
    lo = offs[i];
    hi = offs[i + 1u];
    const uint64_t cut = i + 1u == intervals ? 0u : 2u;  // the marker's two bytes
    if (hi < cut || lo > hi - cut || hi - cut > bytes) {
        lo = hi = 0u;
        return kRange;
    }
    hi -= cut;
    return kOk;
}
// mpos: the markers' positions in byte order, `found` of them (those below `intervals` are stored)
HPDCT_HD uint32_t bounds_located(const uint64_t* mpos, uint64_t found, uint64_t i, uint64_t bytes, uint64_t& lo,
                                 uint64_t& hi) {
    if (i > found) {
        lo = hi = 0u;
        return kMissing;
    }
    lo = i == 0u ? 0u : mpos[i - 1u] + 2u;
    hi = i < found ? mpos[i] : bytes;
    return kOk;
}

typedef int16_t __attribute__((may_alias)) CoefAlias;
struct alignas(16) Vec16 {
    uint32_t x, y, z, w;
} __attribute__((may_alias));

// The bits of one interval, MSB first, unstuffed as they are fetched: the top
// `avail` bits of acc are valid, the rest 0.  err: why the fetch stopped
// (kMarker, kEnd), reported only if a bit beyond `avail` is asked for.  The
// bytes come through a one-word cache: the aligned 8 bytes around pos when they
// lie wholly inside [lo, hi), else the single byte.
struct Reader {
    const uint8_t* scan;
    uint64_t lo, pos, hi;
    uint64_t acc;
    uint32_t avail, err;
    uint64_t cword, cbase;
    uint32_t cn;
};
HPDCT_HD uint32_t byte_at(Reader& r, uint64_t p) {  // lo <= p < hi
    if (p - r.cbase >= r.cn) {
        const uint64_t mis = reinterpret_cast<uintptr_t>(r.scan + p) & 7u;
        if (p >= mis && p - mis >= r.lo && p - mis + 8u <= r.hi) {
            r.cbase = p - mis;
            __builtin_memcpy(&r.cword, __builtin_assume_aligned(r.scan + r.cbase, 8), 8);
            r.cn = 8u;
        } else {
            r.cbase = p, r.cword = r.scan[p], r.cn = 1u;
        }
    }
    return static_cast<uint32_t>(r.cword >> (8u * (p - r.cbase))) & 0xffu;
}
// at least 32 bits afterwards, or err says why not
HPDCT_HD void fill(Reader& r) {
    for (int f = 0; f < 4; ++f) {
        if (r.avail >= 32u || r.err != 0u) break;
        if (r.pos >= r.hi) {
            r.err = kEnd;
            break;
        }
        const uint32_t b = byte_at(r, r.pos);
        if (b == 0xffu) {
            if (r.pos + 1u >= r.hi) {
                r.err = kEnd;
                break;
            }
            if (byte_at(r, r.pos + 1u) != 0u) {
                r.err = kMarker;
                break;
            }
            r.pos += 2u;
        } else {
            r.pos += 1u;
        }
        r.acc |= static_cast<uint64_t>(b) << (56u - r.avail);
        r.avail += 8u;
    }
}
// One Huffman symbol of table `kind`: kOk and the symbol, or the status code.  A
// code is matched against the 16 bits ahead (zeros beyond the fetched ones); a
// match longer than what was fetched, or none, is the fetch's error, as it is
// for a reader that takes one bit at a time: a code is never a prefix of another.
template <class Tab>
HPDCT_HD uint32_t symbol(Reader& r, const Tab* t, uint32_t kind, uint32_t& sym) {
    fill(r);
    const uint32_t peek = static_cast<uint32_t>(r.acc >> 48);
    const uint32_t e = t->look[kind][peek >> 8];
    uint32_t len = e >> 8;
    sym = e & 0xffu;
    if (len == 0u) {
        len = 17u;
        for (uint32_t l = 9; l <= 16u; ++l) {
            const int32_t code = static_cast<int32_t>(peek >> (16u - l));
            if (code <= t->maxcode[kind][l]) {
                len = l;
                if constexpr (kUntrusted<Tab>)
                    sym = t->vals[kind][(static_cast<uint32_t>(code) + static_cast<uint32_t>(t->valoff[kind][l])) & 255u];
                else
                    sym = t->vals[kind][code + t->valoff[kind][l]];
                break;
            }
        }
    }
    if (len > 16u) return r.avail >= 16u ? static_cast<uint32_t>(kCode) : r.err;
    if (len > r.avail) return r.err;
    r.acc <<= len;
    r.avail -= len;
    return kOk;
}
// n <= 15 extra bits extended to the value they code (a negative v as v + 2^n - 1); after symbol()'s fill
HPDCT_HD uint32_t extra(Reader& r, uint32_t n, int32_t& value) {
    value = 0;
    if (n == 0u) return kOk;
    if (n > r.avail) {
        fill(r);
        if (n > r.avail) return r.err;
    }
    const int32_t v = static_cast<int32_t>(r.acc >> (64u - n));
    r.acc <<= n;
    r.avail -= n;
    value = v >= (1 << (n - 1u)) ? v : v - (1 << n) + 1;
    return kOk;
}

// Where block (MCU m, position k in the MCU) lies, as scan_locate of hpdct_scan.hpp: k < bpm, m < nmcu.
HPDCT_HD int16_t* block_of_mcu(int16_t* y, int16_t* cb, int16_t* cr, const scan::ScanGrid& g, uint32_t m, uint32_t k) {
    if (g.bpm == 6u && k < 4u) {
        const uint64_t my = m / g.mcus_x, mx = m % g.mcus_x, tx = 2ull * g.mcus_x;
        return y + 64u * ((2u * my + (k >> 1)) * tx + 2u * mx + (k & 1u));
    }
    const uint32_t comp = g.bpm == 6u ? k - 3u : k;
    return (comp == 0u ? y : comp == 1u ? cb : cr) + 64ull * m;
}
// the staged block (32 dwords) to its place, eight 16-byte stores; then the row is zero again
HPDCT_HD void store_block(int16_t* dst, uint32_t* row) {
    Vec16* d = reinterpret_cast<Vec16*>(dst);
    for (int q = 0; q < 8; ++q) {
        const Vec16 v = {row[4 * q], row[4 * q + 1], row[4 * q + 2], row[4 * q + 3]};
        d[q] = v;
        row[4 * q] = row[4 * q + 1] = row[4 * q + 2] = row[4 * q + 3] = 0u;
    }
}

// Interval iv of the scan, its bytes scan[lo, hi) (pre != 0: kRange or
// kMissing, nothing is read): decodes its blocks into y / cb / cr (cb == cr ==
// nullptr with g.bpm == 1) and returns the status.  row: 32 dwords of the
// caller's, for this walk alone.  kNatural: a block's coefficient n is stored
// at zigzag::kOrder[n].  Every block of the interval is written exactly once.
// Tab: DecodeTables (Annex K) or DecodeTablesWide (the caller's, untrusted).
template <bool kNatural, class Tab = DecodeTables>
HPDCT_HD uint64_t walk_interval(const uint8_t* scan, uint64_t lo, uint64_t hi, uint32_t pre, uint64_t iv,
                                const scan::ScanGrid& g, const Tab* t, const uint8_t* order, uint32_t* row,
                                int16_t* y, int16_t* cb, int16_t* cr) {
    const uint64_t m0 = iv * g.per_interval;
    const uint64_t mcount = g.nmcu - m0 < g.per_interval ? g.nmcu - m0 : g.per_interval;
    const uint64_t nblk = mcount * g.bpm;
    Reader r{scan, lo, lo, hi, 0u, 0u, 0u, 0u, 0u, 0u};
    CoefAlias* const coef = reinterpret_cast<CoefAlias*>(row);
    for (int i = 0; i < 32; ++i) row[i] = 0u;
    uint64_t b = 0;                     // the block being decoded
    uint32_t m = static_cast<uint32_t>(m0), kk = 0;  // its MCU and its position there
    uint32_t k = 0;                     // the next coefficient; 0: the DC is next
    int32_t pred0 = 0, pred1 = 0, pred2 = 0;
    uint32_t code = pre;
    // one turn = one symbol: the DC and at most 63 AC symbols per block
    for (uint64_t step = 0, limit = 64u * nblk; step < limit && b < nblk && code == kOk; ++step) {
        const uint32_t comp = g.bpm == 6u ? (kk < 4u ? 0u : kk - 3u) : kk;
        const uint32_t chroma = comp != 0u ? 2u : 0u;
        uint32_t sym = 0;
        bool done = false;
        if (k == 0u) {
            code = symbol(r, t, chroma, sym);
            if (code != kOk) break;
            int32_t diff;
            if constexpr (kUntrusted<Tab>) sym &= 15u;  // hpdct_huffman_prepare refuses a DC symbol above 15
            code = extra(r, sym, diff);
            if (code != kOk) break;
            const int32_t pred = (comp == 0u ? pred0 : comp == 1u ? pred1 : pred2) + diff;
            if (pred < -32768 || pred > 32767) {
                code = kDc;
                break;
            }
            if (comp == 0u) pred0 = pred; else if (comp == 1u) pred1 = pred; else pred2 = pred;
            coef[0] = static_cast<int16_t>(pred);
            k = 1u;
        } else {
            code = symbol(r, t, chroma + 1u, sym);
            if (code != kOk) break;
            const uint32_t run = sym >> 4, n = sym & 15u;
            if (n == 0u) {
                if (run == 15u) {
                    k += 16u;  // ZRL
                    if (k > 64u) {
                        code = kIndex;
                        break;
                    }
                } else {
                    done = true;  // EOB
                }
            } else {
                k += run;
                if (k > 63u) {
                    code = kIndex;
                    break;
                }
                int32_t v;
                code = extra(r, n, v);
                if (code != kOk) break;
                coef[kNatural ? order[k] : k] = static_cast<int16_t>(v);
                ++k;
            }
        }
        if (done || k >= 64u) {
            store_block(block_of_mcu(y, cb, cr, g, m, kk), row);
            ++b, k = 0u;
            if (++kk == g.bpm) kk = 0u, ++m;
        }
    }
    if (code == kOk) {
        // every block decoded: the rest of the current byte is 1 bits and the interval ends with it
        const uint32_t pad = r.avail & 7u;
        const bool ones = pad == 0u || (r.acc >> (64u - pad)) == (1u << pad) - 1u;
        return r.avail < 8u && r.pos == r.hi && ones ? 0u : static_cast<uint64_t>(kTail);
    }
    // the failing block and every later one: 64 zeros
    const uint64_t failed = b;
    for (int i = 0; i < 32; ++i) row[i] = 0u;
    for (; b < nblk; ++b) {
        store_block(block_of_mcu(y, cb, cr, g, m, kk), row);
        if (++kk == g.bpm) kk = 0u, ++m;
    }
    return code + 256u * failed;
}

}  // namespace unscan

// The launches on s, as policy::unscan_* choose them (hpdct_unscan.hip).  offs
// (g.intervals + 1 entries) may be nullptr: the markers are located then, and
// workspace holds unscan::workspace_bytes(g.intervals, bytes) bytes, 16-byte
// aligned.  status (g.intervals entries) may be nullptr.  blob nullptr: Annex K's
// kernels; else the caller's tables, a HuffBlob in device memory.  The caller checked everything.
hipError_t launch_unscan(const uint8_t* scan, uint64_t bytes, const uint64_t* offs, int16_t* y, int16_t* cb,
                         int16_t* cr, const scan::ScanGrid& g, bool natural, hpdct_decode_info* info, uint64_t* status,
                         void* workspace, const unscan::HuffBlob* blob, hipStream_t s);
// the marker search's launches alone (count, rank, place; the rank launch alone with offsets), for hpdct_unscan_split.hpp
hipError_t launch_unscan_locate(const uint8_t* scan, uint64_t bytes, const uint64_t* offs, const scan::ScanGrid& g,
                                hpdct_decode_info* info, void* workspace, hipStream_t s);

}  // namespace hpdct

// the kernels: for the unit that defines HPDCT_UNSCAN_KERNELS (hpdct_unscan.hip) only
#if defined(__HIPCC__) && defined(HPDCT_UNSCAN_KERNELS)

namespace hpdct {

__device__ const unscan::DecodeTables kUnscanTables = unscan::make_decode_tables();
__device__ const unscan::ZigzagOrder kUnscanOrder = unscan::make_zigzag_order();

__device__ inline uint32_t unscan_wave_sum(uint32_t v) {
#pragma unroll
    for (uint32_t d = 32; d != 0u; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Launches 1 (kUnscanCount alone) and 3 (with kUnscanPlace): wave w takes the
// chunks w, w + waves, ...; 64 bytes of a chunk per step, one per lane.
//   count: counts[c] = the markers whose first byte is in chunk c
//   place: counts[c] holds the rank of the chunk's first marker (the rank
//          kernel ran); mpos[j] = the position of marker j, for j < intervals;
//          a marker j < intervals - 1 whose number is not j mod 8 is counted in
//          info->marker_errors
template <unsigned kVar>
__global__ __launch_bounds__(256) void unscan_locate_kernel(const uint8_t* __restrict__ scan, const uint64_t bytes,
                                                            const uint64_t nchunks, uint64_t* __restrict__ counts,
                                                            uint64_t* __restrict__ mpos, const uint32_t intervals,
                                                            hpdct_decode_info* __restrict__ info) {
    constexpr bool kPlace = (kVar & kUnscanPlace) != 0u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = blockIdx.x * 4ull + threadIdx.x / 64u, waves = gridDim.x * 4ull;
    uint32_t wrong = 0;
    for (uint64_t c = wave; c < nchunks; c += waves) {
        uint64_t rank = 0;
        uint32_t n = 0;
        if constexpr (kPlace) rank = counts[c];
        for (uint32_t s = 0; s < unscan::kChunkBytes / 64u; ++s) {
            const uint64_t p = c * unscan::kChunkBytes + s * 64u + lane;
            const bool mk = unscan::marker_at(scan, p, bytes);
            if constexpr (kPlace) {
                const uint64_t mask = __ballot(mk);
                const uint64_t j = rank + static_cast<uint64_t>(__popcll(mask & ((1ull << lane) - 1ull)));
                if (mk && j < intervals) {
                    mpos[j] = p;
                    if (j + 1u < intervals && (scan[p + 1u] & 7u) != (j & 7u)) ++wrong;
                }
                rank += static_cast<uint64_t>(__popcll(mask));
            } else {
                n += mk;
            }
        }
        if constexpr (!kPlace) {
            n = unscan_wave_sum(n);
            if (lane == 0u) counts[c] = n;
        }
    }
    if constexpr (kPlace) {
        wrong = unscan_wave_sum(wrong);
        if (lane == 0u && wrong != 0u) atomicAdd(&info->marker_errors, wrong);  // integer: order-independent
    }
}

// Launch 2, one workgroup of 1024 threads: counts[c] becomes the number of
// markers before chunk c (in place), *info = {0, the total, 0, 0}.  n == 0 (the
// offsets were given): *info is cleared and nothing else.  Thread t owns the
// chunks [t * per, (t + 1) * per).
__global__ __launch_bounds__(1024) void unscan_rank_kernel(uint64_t* __restrict__ counts, const uint64_t n,
                                                           hpdct_decode_info* __restrict__ info) {
    __shared__ uint64_t s_sum[1024];
    const uint32_t t = threadIdx.x;
    const uint64_t per = (n + 1023u) / 1024u;
    const uint64_t b = t * per < n ? t * per : n, e = b + per < n ? b + per : n;
    uint64_t sum = 0;
    for (uint64_t i = b; i < e; ++i) sum += counts[i];
    s_sum[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint64_t o = t >= d ? s_sum[t - d] : 0u;
        __syncthreads();
        s_sum[t] += o;
        __syncthreads();
    }
    uint64_t run = s_sum[t] - sum;
    for (uint64_t i = b; i < e; ++i) {
        const uint64_t c = counts[i];
        counts[i] = run;
        run += c;
    }
    if (t == 1023u) {
        const uint64_t total = s_sum[1023];
        info->bad_intervals = 0u;
        info->markers_found = total > 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(total);
        info->marker_errors = 0u;
        info->reserved = 0u;
    }
}

// Launch 4; one wave per workgroup, its first kLanes lanes take an interval
// each: workgroup b the intervals b * kLanes + lane, then every gridDim.x-th
// such group.  offs != nullptr: the caller's table; else mpos and
// info->markers_found, as the launches before wrote them.  Tab and tab_src: the
// tables' type and where they are staged from (sizeof(Tab) bytes, 4-byte aligned).
template <unsigned kVar, class Tab>
__device__ inline void unscan_decode_body(const uint8_t* __restrict__ scan, const uint64_t bytes,
                                          const uint64_t* __restrict__ offs, const uint64_t* __restrict__ mpos,
                                          int16_t* __restrict__ y, int16_t* __restrict__ cb, int16_t* __restrict__ cr,
                                          const scan::ScanGrid& g, hpdct_decode_info* __restrict__ info,
                                          uint64_t* __restrict__ status, const uint32_t* __restrict__ tab_src) {
    constexpr uint32_t kLanes = unscan_lanes_of(kVar);
    constexpr bool kNatural = (kVar & kScanNatural) != 0u;
    constexpr uint32_t kWords = static_cast<uint32_t>(sizeof(Tab) / 4u);
    __shared__ uint32_t s_tab[kWords];
    __shared__ uint32_t s_row[kLanes * scan::kBlkStride];
    __shared__ uint8_t s_order[64];
    const uint32_t lane = threadIdx.x;
    {
        for (uint32_t i = lane; i < kWords; i += 64u) s_tab[i] = tab_src[i];
        s_order[lane] = kUnscanOrder.v[lane];
    }
    __syncthreads();
    const Tab* tab = reinterpret_cast<const Tab*>(s_tab);
    const uint64_t found = offs ? 0u : info->markers_found;
    uint32_t bad = 0;
    for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kLanes; base < g.intervals;
         base += static_cast<uint64_t>(gridDim.x) * kLanes) {
        const uint64_t iv = base + lane;
        if (lane < kLanes && iv < g.intervals) {
            uint64_t lo, hi;
            const uint32_t pre = offs ? unscan::bounds_given(offs, iv, g.intervals, bytes, lo, hi)
                                      : unscan::bounds_located(mpos, found, iv, bytes, lo, hi);
            const uint64_t st = unscan::walk_interval<kNatural>(scan, lo, hi, pre, iv, g, tab, s_order,
                                                                s_row + lane * scan::kBlkStride, y, cb, cr);
            if (status) status[iv] = st;
            bad += st != 0u;
        }
    }
    bad = unscan_wave_sum(bad);
    if (lane == 0u && bad != 0u) atomicAdd(&info->bad_intervals, bad);  // integer: order-independent
}
template <unsigned kVar>
__global__ __launch_bounds__(64) void unscan_decode_kernel(const uint8_t* __restrict__ scan, const uint64_t bytes,
                                                           const uint64_t* __restrict__ offs,
                                                           const uint64_t* __restrict__ mpos, int16_t* __restrict__ y,
                                                           int16_t* __restrict__ cb, int16_t* __restrict__ cr,
                                                           const scan::ScanGrid g, hpdct_decode_info* __restrict__ info,
                                                           uint64_t* __restrict__ status) {
    static_assert(sizeof(unscan::DecodeTables) == 4u * unscan::kTableWords, "tables are packed");
    unscan_decode_body<kVar, unscan::DecodeTables>(scan, bytes, offs, mpos, y, cb, cr, g, info, status,
                                                   reinterpret_cast<const uint32_t*>(&kUnscanTables));
}
// the same under the caller's tables (kVar carries kScanTables): blob, a HuffBlob in device memory
template <unsigned kVar>
__global__ __launch_bounds__(64) void unscan_decode_tables_kernel(
    const uint8_t* __restrict__ scan, const uint64_t bytes, const uint64_t* __restrict__ offs,
    const uint64_t* __restrict__ mpos, int16_t* __restrict__ y, int16_t* __restrict__ cb, int16_t* __restrict__ cr,
    const scan::ScanGrid g, hpdct_decode_info* __restrict__ info, uint64_t* __restrict__ status,
    const unscan::HuffBlob* __restrict__ blob) {
    unscan_decode_body<kVar, unscan::DecodeTablesWide>(scan, bytes, offs, mpos, y, cb, cr, g, info, status,
                                                       reinterpret_cast<const uint32_t*>(&blob->dec));
}

}  // namespace hpdct

#endif  // HPDCT_UNSCAN_KERNELS
