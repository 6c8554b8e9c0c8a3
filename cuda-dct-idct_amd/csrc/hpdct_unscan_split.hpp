// hpdct_unscan_split.hpp -- the self-synchronising entropy decoder
// (hpdct_decode_scan_split): hpdct_unscan.hpp's decoder made parallel INSIDE a
// restart interval.  The results are those of hpdct_decode_scan, bit for bit.
//
// An interval of at least split_min_bytes bytes is cut into segments of
// kSegBytes bytes; one lane walks one segment (unsplit::walk_segment, plain C++
// for host and device as walk_interval is; tests/tools/asan_unscan_split_check.cpp
// runs the whole algorithm with it on the CPU).  The state of a walk when a
// symbol starts is SegState: the raw byte that holds the next bit and the bit in
// it, the position kk in the MCU, the next coefficient k.  Neither the block
// number nor the DC predictors belong to it: sums over the segments give those.
//
// The launches, one chain, all unconditional (the host reads nothing back):
//   locate   hpdct_unscan.hpp's count / rank / place (rank alone with offsets);
//   plan     one workgroup: the segments and groups of every interval (exclusive
//            sums), the interval of every group, the info's last four words;
//   settle   kRounds + 1 launches of one kernel.  A workgroup of kGroup lanes
//            owns kGroup consecutive segments of one interval (a group).  Launch
//            0: every lane walks its segment from its boundary (segment 0 of an
//            interval: from the true start), then lane t walks again from lane
//            t - 1's exit while that differs from what it started from, until
//            the group is the chain of walks from the group's entry (at most
//            kGroup turns, in LDS).  Launch L >= 1: a group whose entry differs
//            from the exit its predecessor group had after launch L - 1 settles
//            again from that exit.  The groups' last exits are double-buffered
//            between launches, so the result does not depend on scheduling;
//   offsets  one workgroup per interval: the fixed point is checked (every
//            group's entry is its predecessor's last exit), the segments' block
//            counts and DC sums become first blocks and first predictors, the
//            error flags, the block count and the interval's end are judged;
//   clear    the blocks of the intervals that passed are zeroed;
//   write    every lane walks its segment once more and stores the non-zero
//            coefficients and the DC values (checked to fit int16);
//   serial   hpdct_unscan.hpp's walk_interval, one lane per interval, for every
//            interval that was not split or did not pass; the status array.
// A clean status never comes from the split path without the fixed point (the
// only proof that the exits are the true ones: segment 0 entered at the true
// start, every other segment at its predecessor's exit), the block count and
// the end-of-interval check.
//
// The bound: after launch L the groups 0..L of an interval are final, so an
// interval of at most kRounds + 1 groups, (kRounds + 1) * kGroup * kSegBytes
// bytes, is always at its fixed point after the last launch, whatever it holds.
// No workgroup waits on another; the only atomics are integer sums, ors and a max.
#pragma once

#include "hpdct_policy.hpp"
#include "hpdct_unscan.hpp"

namespace hpdct {
namespace unsplit {

constexpr uint32_t kSegBytes = policy::kUnsplitSegBytes, kGroup = policy::kUnsplitGroup, kRounds = policy::kUnsplitRounds;

// bits of an interval's flag word
enum : uint32_t { kIvSplit = 1u, kIvUnsettled = 2u, kIvBad = 4u, kIvDc = 8u };

// Where a walk stands when a symbol starts, and what the walk that got there
// saw: bits = bit (0..7) | kk << 3 | k << 6 | kSegErr; nblk: the blocks that
// walk completed.  An ENTRY is a state with nblk = 0 and no flag (entry_of).
struct alignas(16) SegState {
    uint64_t pos;
    uint32_t bits, nblk;
};
static_assert(sizeof(SegState) == 16u, "a state packs into 16 bytes");
constexpr uint32_t kSegErr = 1u << 13, kSegStateMask = kSegErr - 1u;
HPDCT_HD bool same(const SegState& a, const SegState& b) { return a.pos == b.pos && a.bits == b.bits && a.nblk == b.nblk; }
HPDCT_HD SegState entry_of(const SegState& exit) { return SegState{exit.pos, exit.bits & kSegStateMask, 0u}; }

// per segment, what the offsets launch sums: the DC differences a walk decoded, per component
struct alignas(16) SegDc {
    int32_t sum[3];
    uint32_t pad;
};
// per segment, what the write launch starts from: its first block (the one in progress at its entry) and predictors
struct alignas(16) SegStart {
    uint64_t block;
    int64_t pred[3];
};

// The workspace: hpdct_unscan.hpp's (markers, chunk counts), then the arrays
// below, each a 16-byte multiple.  The budget: an honest offsets table (or the
// located markers) cuts the scan into disjoint intervals, whose segments number
// at most ceil(bytes / kSegBytes) + intervals and whose groups at most
// ceil(segments / kGroup) + intervals.
struct Layout {
    uint64_t nseg, ngrp;  // the budgets
    uint64_t ivseg, ivgrp, ivflag, totals, grpiv, gentry, glast, exits, dcs, starts, bytes;  // byte offsets; the total
};
constexpr uint64_t up16(uint64_t n) { return (n + 15u) / 16u * 16u; }
constexpr Layout layout(uint64_t intervals, uint64_t bytes) {
    Layout l{};
    l.nseg = (bytes + kSegBytes - 1u) / kSegBytes + intervals;
    l.ngrp = (l.nseg + kGroup - 1u) / kGroup + intervals;
    uint64_t at = static_cast<uint64_t>(unscan::workspace_bytes(intervals, bytes));
    l.ivseg = at, at += up16(8u * (intervals + 1u));
    l.ivgrp = at, at += up16(8u * (intervals + 1u));
    l.ivflag = at, at += up16(4u * intervals);
    l.totals = at, at += 16u;
    l.grpiv = at, at += up16(4u * l.ngrp);
    l.gentry = at, at += 16u * l.ngrp;
    l.glast = at, at += 32u * l.ngrp;
    l.exits = at, at += 16u * l.nseg;
    l.dcs = at, at += 16u * l.nseg;
    l.starts = at, at += 32u * l.nseg;
    l.bytes = at;
    return l;
}
struct Ws {
    uint64_t* ivseg;   // [intervals + 1] first segment of an interval (exclusive sum)
    uint64_t* ivgrp;   // [intervals + 1] first group
    uint32_t* ivflag;  // [intervals]
    uint64_t* totals;  // groups, segments in use
    uint32_t* grpiv;   // [ngrp] the interval of a group
    SegState* gentry;  // [ngrp] the entry a group last settled from
    SegState* glast;   // [2][ngrp] a group's last exit after the launch of that parity
    SegState* exits;   // [nseg]
    SegDc* dcs;        // [nseg]
    SegStart* starts;  // [nseg]
    uint64_t ngrp, nseg;
};
inline Ws carve(void* workspace, const Layout& l) {
    uint8_t* b = static_cast<uint8_t*>(workspace);
    return Ws{reinterpret_cast<uint64_t*>(b + l.ivseg),  reinterpret_cast<uint64_t*>(b + l.ivgrp),
              reinterpret_cast<uint32_t*>(b + l.ivflag), reinterpret_cast<uint64_t*>(b + l.totals),
              reinterpret_cast<uint32_t*>(b + l.grpiv),  reinterpret_cast<SegState*>(b + l.gentry),
              reinterpret_cast<SegState*>(b + l.glast),  reinterpret_cast<SegState*>(b + l.exits),
              reinterpret_cast<SegDc*>(b + l.dcs),       reinterpret_cast<SegStart*>(b + l.starts),
              l.ngrp,                                    l.nseg};
}

// the segments of an interval [lo, hi) with bounds status pre: 0 = it is not split
HPDCT_HD uint64_t segments_of(uint32_t pre, uint64_t lo, uint64_t hi, uint64_t split_min) {
    const uint64_t len = hi - lo;
    if (pre != unscan::kOk || len == 0u || len < split_min) return 0u;
    return (len + kSegBytes - 1u) / kSegBytes;
}
// a + b, at most cap (a, b <= cap < 2^62): associative, so a scan may use it
HPDCT_HD uint64_t sat_add(uint64_t a, uint64_t b, uint64_t cap) { return a + b < cap ? a + b : cap; }

// Where segment q of the interval starts its speculative walk: the true start
// for q = 0; else its first byte, or the byte after it when that first byte is
// the 00 of a stuffed FF 00 (the FF still inside the interval).
HPDCT_HD SegState boundary_entry(const uint8_t* scan, uint64_t lo, uint64_t hi, uint64_t q) {
    uint64_t p = lo + q * kSegBytes;
    if (q != 0u && p < hi && scan[p] == 0u && scan[p - 1u] == 0xffu) ++p;
    return SegState{p, 0u, 0u};
}

// The raw byte that holds the reader's next bit, and the bit in it.  The bits
// it holds came from the (avail + 7) / 8 data bytes before r.pos, none before
// `floor`, where the reader started; a data byte 00 never follows an FF.
HPDCT_HD uint64_t next_bit_at(const unscan::Reader& r, uint64_t floor, uint32_t& bit) {
    uint64_t p = r.pos;
    for (uint32_t n = (r.avail + 7u) >> 3; n != 0u; --n) {
        --p;
        if (r.scan[p] == 0u && p > floor && r.scan[p - 1u] == 0xffu) --p;
    }
    bit = (8u - (r.avail & 7u)) & 7u;
    return p;
}

// what a walk does with the values it decodes
struct CountSink {  // the settle launches: the DC sums alone
    int32_t sum[3] = {0, 0, 0};
    HPDCT_HD void dc(uint32_t comp, int32_t diff) {
        if (comp == 0u) sum[0] += diff; else if (comp == 1u) sum[1] += diff; else sum[2] += diff;
    }
    HPDCT_HD void ac(uint32_t, int32_t) {}
    HPDCT_HD void end_block() {}
};
// The write launch: block `block` of the interval (its first MCU m0, nblk
// blocks) is in progress.  Every store goes to a block below nblk, its address
// from the block number alone; the coefficient index is the walk's, <= 63.
template <bool kNatural>
struct StoreSink {
    int16_t *y, *cb, *cr;
    scan::ScanGrid g;
    const uint8_t* order;
    uint64_t block, nblk;
    uint32_t m, kk;  // the block's MCU and its position there
    int64_t pred[3];
    bool dc_bad = false;
    unscan::CoefAlias* dst = nullptr;
    HPDCT_HD void seek() {
        dst = block < nblk ? reinterpret_cast<unscan::CoefAlias*>(unscan::block_of_mcu(y, cb, cr, g, m, kk)) : nullptr;
    }
    HPDCT_HD void dc(uint32_t comp, int32_t diff) {
        const int64_t p = (comp == 0u ? pred[0] : comp == 1u ? pred[1] : pred[2]) + diff;  // constant indices: registers
        if (comp == 0u) pred[0] = p; else if (comp == 1u) pred[1] = p; else pred[2] = p;
        if (p < -32768 || p > 32767) dc_bad = true;
        if (dst) dst[0] = static_cast<int16_t>(p);
    }
    HPDCT_HD void ac(uint32_t k, int32_t v) {
        if (dst) dst[kNatural ? order[k] : k] = static_cast<int16_t>(v);
    }
    HPDCT_HD void end_block() {
        ++block;
        if (++kk == g.bpm) kk = 0u, ++m;
        seek();
    }
};

// One segment of the interval scan[lo, hi): the walk from `entry` until a symbol
// would start at or past `end` (the segment's end, <= hi).  Nothing outside
// [lo, hi) is read.  Returns the exit.  A walk never stops at an error: on CODE
// (one bit is dropped) and INDEX it sets kSegErr, ends the block and goes on;
// MARKER and END leave no bit to go on with, so the walk ends at hi with kSegErr
// -- except the END of a DC symbol that hpdct_decode_scan's rule for the
// interval's last byte accepts (fewer than 8 bits left, all 1, no byte left):
// the clean end of an interval, exit at hi without a flag.  Every turn consumes
// at least a bit and starts before `end`, at most 8 * kSegBytes bits after the
// entry: the loop's bound is never the reason it ends.
// Tab: unscan::DecodeTables (Annex K) or unscan::DecodeTablesWide (the caller's, untrusted).
template <class Sink, class Tab>
HPDCT_HD SegState walk_segment(const uint8_t* scan, uint64_t lo, uint64_t hi, uint64_t end, const SegState& entry,
                               uint32_t bpm, const Tab* t, Sink& sink) {
    using namespace unscan;
    if (entry.pos >= end) return entry_of(entry);  // a symbol of an earlier segment covers this one
    uint32_t kk = (entry.bits >> 3) & 7u, k = (entry.bits >> 6) & 127u, nblk = 0, flags = 0;
    Reader r{scan, lo, entry.pos, hi, 0u, 0u, 0u, 0u, 0u, 0u};
    if (const uint32_t bit = entry.bits & 7u) {
        fill(r);
        if (r.avail < bit) return SegState{hi, kSegErr, 0u};
        r.acc <<= bit, r.avail -= bit;
    }
    for (uint32_t turn = 0; turn < 8u * kSegBytes + 32u; ++turn) {
        if (r.pos >= end) {  // the bytes fetched reach the end: where does the next symbol start?
            uint32_t bit;
            if (next_bit_at(r, entry.pos, bit) >= end) break;
        }
        const uint32_t comp = bpm == 6u ? (kk < 4u ? 0u : kk - 3u) : kk;
        const uint32_t chroma = comp != 0u ? 2u : 0u;
        uint32_t sym = 0, code;
        bool done = false;
        if (k == 0u) {
            code = symbol(r, t, chroma, sym);
            if (code == kEnd) {
                const uint32_t pad = r.avail & 7u;
                if (r.avail < 8u && r.pos == r.hi && (pad == 0u || (r.acc >> (64u - pad)) == (1u << pad) - 1u))
                    return SegState{hi, (kk << 3) | flags, nblk};
            }
            int32_t diff = 0;
            if constexpr (kUntrusted<Tab>) sym &= 15u;  // hpdct_huffman_prepare refuses a DC symbol above 15
            if (code == kOk) code = extra(r, sym, diff);
            if (code == kOk) sink.dc(comp, diff), k = 1u;
        } else {
            code = symbol(r, t, chroma + 1u, sym);
            if (code == kOk) {
                const uint32_t run = sym >> 4, n = sym & 15u;
                if (n == 0u) {
                    if (run != 15u) done = true;  // EOB
                    else if ((k += 16u) > 64u) code = kIndex;
                } else if ((k += run) > 63u) {
                    code = kIndex;
                } else {
                    int32_t v;
                    code = extra(r, n, v);
                    if (code == kOk) sink.ac(k, v), ++k;
                }
            }
        }
        if (code != kOk) {
            flags = kSegErr;
            if (code == kMarker || code == kEnd) return SegState{hi, kSegErr, nblk};
            if (code == kCode) r.acc <<= 1, r.avail -= 1u;  // symbol() took nothing: 16 bits or more are there
            done = true;
        }
        if (done || k >= 64u) {
            sink.end_block();
            ++nblk, k = 0u;
            if (++kk == bpm) kk = 0u;
        }
    }
    uint32_t bit;
    const uint64_t at = next_bit_at(r, entry.pos, bit);
    return SegState{at, bit | (kk << 3) | (k << 6) | flags, nblk};
}

// whether the last exit of a split interval is the end hpdct_decode_scan accepts: at hi, between two MCUs
HPDCT_HD bool ends_clean(const SegState& last, uint64_t hi) { return last.pos == hi && last.bits == 0u; }

}  // namespace unsplit

// The launches on s (hpdct_unscan_split.hip).  workspace: unsplit::layout(g.intervals, bytes).bytes bytes, 16-byte
// aligned; split_min >= 1.  blob nullptr: Annex K's kernels; else the caller's tables, a HuffBlob
// (hpdct_unscan.hpp) in device memory.  The caller checked everything.
hipError_t launch_unscan_split(const uint8_t* scan, uint64_t bytes, const uint64_t* offs, int16_t* y, int16_t* cb,
                               int16_t* cr, const scan::ScanGrid& g, bool natural, uint64_t split_min,
                               hpdct_decode_split_info* info, uint64_t* status, void* workspace,
                               const unscan::HuffBlob* blob, hipStream_t s);

}  // namespace hpdct
