// hpdct_unscan_split.hip -- the split entropy decoder's kernels and launches (hpdct_unscan_split.hpp): one launch
// function, launch_unscan_split, for Annex K's tables and the caller's.
#include "hpdct_unscan_split.hpp"
#include "hpdct_launch.hpp"

namespace hpdct {

namespace {

using unsplit::SegDc;
using unsplit::SegStart;
using unsplit::SegState;
using unsplit::Ws;
constexpr uint32_t kG = unsplit::kGroup, kS = unsplit::kSegBytes;

__device__ const unscan::DecodeTables kUnsplitTables = unscan::make_decode_tables();
__device__ const unscan::ZigzagOrder kUnsplitOrder = unscan::make_zigzag_order();

// what every kernel gets of the call
struct Call {
    const uint8_t* scan;
    uint64_t bytes;
    const uint64_t* offs;  // or nullptr: mpos and info->markers_found
    const uint64_t* mpos;
    scan::ScanGrid g;
    uint64_t split_min;
};
__device__ inline uint32_t bounds_of(const Call& c, uint64_t found, uint64_t iv, uint64_t& lo, uint64_t& hi) {
    return c.offs ? unscan::bounds_given(c.offs, iv, c.g.intervals, c.bytes, lo, hi)
                  : unscan::bounds_located(c.mpos, found, iv, c.bytes, lo, hi);
}
__device__ inline uint64_t blocks_of(const scan::ScanGrid& g, uint64_t iv) {
    const uint64_t m0 = iv * g.per_interval;
    return (g.nmcu - m0 < g.per_interval ? g.nmcu - m0 : g.per_interval) * g.bpm;
}
// Tab's words from src (the built-in tables, or the decoder's part of a caller's blob) to LDS
template <uint32_t kThreads, class Tab>
__device__ inline void stage_tables(uint32_t* s_tab, const uint32_t* __restrict__ src) {
    for (uint32_t i = threadIdx.x; i < static_cast<uint32_t>(sizeof(Tab) / 4u); i += kThreads) s_tab[i] = src[i];
}
__device__ inline const uint32_t* builtin_tables() { return reinterpret_cast<const uint32_t*>(&kUnsplitTables); }
__device__ inline const uint32_t* blob_tables(const unscan::HuffBlob* blob) {
    return reinterpret_cast<const uint32_t*>(&blob->dec);
}

// The plan, one workgroup of 1024 threads; thread t owns the intervals [t * per, (t + 1) * per).  An interval's
// segments and groups come out of the budgets ws.nseg and ws.ngrp: it is split only if the segments of all
// intervals up to it fit (with honest offsets they always do), so every index below stays inside the workspace.
__global__ __launch_bounds__(1024) void unsplit_plan_kernel(const Call c, const Ws ws,
                                                            hpdct_decode_split_info* __restrict__ info) {
    __shared__ uint64_t s_seg[1024], s_grp[1024];
    __shared__ unsigned long long s_tot[2];
    const uint32_t t = threadIdx.x;
    const uint64_t n = c.g.intervals, cap = ws.nseg + 1u;
    const uint64_t per = (n + 1023u) / 1024u;
    const uint64_t b = t * per < n ? t * per : n, e = b + per < n ? b + per : n;
    const uint64_t found = c.offs ? 0u : info->markers_found;
    if (t < 2u) s_tot[t] = 0u;
    uint64_t seg = 0, grp = 0;
    for (uint64_t iv = b; iv < e; ++iv) {
        uint64_t lo, hi;
        const uint32_t pre = bounds_of(c, found, iv, lo, hi);
        const uint64_t k = unsplit::segments_of(pre, lo, hi, c.split_min);
        seg = unsplit::sat_add(seg, k < cap ? k : cap, cap);
        grp = unsplit::sat_add(grp, k < cap ? (k + kG - 1u) / kG : cap, cap);
    }
    s_seg[t] = seg, s_grp[t] = grp;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint64_t os = t >= d ? s_seg[t - d] : 0u, og = t >= d ? s_grp[t - d] : 0u;
        __syncthreads();
        s_seg[t] = unsplit::sat_add(os, s_seg[t], cap), s_grp[t] = unsplit::sat_add(og, s_grp[t], cap);
        __syncthreads();
    }
    uint64_t rs = t == 0u ? 0u : s_seg[t - 1u], rg = t == 0u ? 0u : s_grp[t - 1u];  // before this thread's intervals
    uint64_t tot_s = 0, tot_g = 0;
    for (uint64_t iv = b; iv < e; ++iv) {
        uint64_t lo, hi;
        const uint32_t pre = bounds_of(c, found, iv, lo, hi);
        uint64_t k = unsplit::segments_of(pre, lo, hi, c.split_min);
        const uint64_t after = unsplit::sat_add(rs, k < cap ? k : cap, cap);
        const bool fits = k != 0u && after <= ws.nseg;  // then every interval before it fitted as well
        ws.ivseg[iv] = rs, ws.ivgrp[iv] = rg;
        ws.ivflag[iv] = fits ? unsplit::kIvSplit : 0u;
        if (fits) {
            const uint64_t ng = (k + kG - 1u) / kG;
            for (uint64_t j = 0; j < ng; ++j) ws.grpiv[rg + j] = static_cast<uint32_t>(iv);
            tot_s = after, tot_g = rg + ng;
        }
        rs = after, rg = unsplit::sat_add(rg, k < cap ? (k + kG - 1u) / kG : cap, cap);
    }
    if (e == n && b <= n && t == (n == 0u ? 0u : static_cast<uint32_t>((n - 1u) / per))) ws.ivseg[n] = rs, ws.ivgrp[n] = rg;
    atomicMax(&s_tot[0], static_cast<unsigned long long>(tot_g));
    atomicMax(&s_tot[1], static_cast<unsigned long long>(tot_s));
    __syncthreads();
    if (t == 0u) {
        ws.totals[0] = s_tot[0], ws.totals[1] = s_tot[1];
        info->split_intervals = 0u, info->serial_intervals = 0u, info->unsettled_intervals = 0u, info->rounds = 0u;
    }
}

// where group `grp` lies: its interval, the interval's bytes, its first segment (within the interval and in the
// arrays) and how many it has
struct GroupAt {
    uint64_t iv, lo, hi, q0, seg0;
    uint32_t n;
};
__device__ inline GroupAt group_at(const Call& c, const Ws& ws, uint64_t found, uint64_t grp) {
    GroupAt a;
    a.iv = ws.grpiv[grp];
    bounds_of(c, found, a.iv, a.lo, a.hi);
    const uint64_t nseg = (a.hi - a.lo + kS - 1u) / kS;
    a.q0 = (grp - ws.ivgrp[a.iv]) * kG;
    a.seg0 = ws.ivseg[a.iv] + a.q0;
    a.n = static_cast<uint32_t>(nseg - a.q0 < kG ? nseg - a.q0 : kG);
    return a;
}

// The settle launches; `launch` is 0 .. kRounds.  Workgroup w takes the groups w, w + gridDim.x, ...
// Tab and src: the tables' type and where they are staged from.
template <class Tab>
__device__ inline void unsplit_settle_body(const Call& c, const Ws& ws, const uint32_t launch,
                                           hpdct_decode_split_info* __restrict__ info,
                                           const uint32_t* __restrict__ src) {
    __shared__ uint32_t s_tab[sizeof(Tab) / 4u];
    __shared__ SegState s_ex[kG];
    const uint32_t t = threadIdx.x;
    stage_tables<kG, Tab>(s_tab, src);
    __syncthreads();
    const Tab* tab = reinterpret_cast<const Tab*>(s_tab);
    const uint64_t found = c.offs ? 0u : info->markers_found, groups = ws.totals[0];
    const SegState* last_in = ws.glast + ((launch + 1u) & 1u) * ws.ngrp;
    SegState* last_out = ws.glast + (launch & 1u) * ws.ngrp;
    for (uint64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const GroupAt a = group_at(c, ws, found, grp);
        const bool active = t < a.n;
        const uint64_t q = a.q0 + t;
        const uint64_t end = a.lo + (q + 1u) * kS < a.hi ? a.lo + (q + 1u) * kS : a.hi;
        SegState entry{0u, 0u, 0u}, ex{0u, 0u, 0u};
        bool dirty = false;
        if (launch == 0u) {
            if (active) entry = unsplit::boundary_entry(c.scan, a.lo, a.hi, q), dirty = true;
        } else {
            // uniform: this group's entry against its predecessor's last exit after the launch before
            if (a.q0 == 0u) {
                if (t == 0u) last_out[grp] = last_in[grp];
                continue;
            }
            const SegState pred = unsplit::entry_of(last_in[grp - 1u]);
            if (unsplit::same(pred, ws.gentry[grp])) {
                if (t == 0u) last_out[grp] = last_in[grp];
                continue;
            }
            if (t == 0u) atomicMax(&info->rounds, launch);
            if (active) {
                ex = ws.exits[a.seg0 + t];
                entry = t == 0u ? pred : unsplit::entry_of(ws.exits[a.seg0 + t - 1u]);
                dirty = t == 0u;
            }
        }
        __syncthreads();  // the round before is done with s_ex
        s_ex[t] = ex;
        unsplit::CountSink sink;
        bool walked = false;
        for (uint32_t round = 0; round <= kG; ++round) {
            if (dirty) {
                sink = unsplit::CountSink();
                ex = unsplit::walk_segment(c.scan, a.lo, a.hi, end, entry, c.g.bpm, tab, sink);
                s_ex[t] = ex;
                walked = true;
            }
            if (!__syncthreads_or(dirty ? 1 : 0)) break;
            dirty = false;
            if (active && t > 0u) {
                const SegState cand = unsplit::entry_of(s_ex[t - 1u]);
                if (!unsplit::same(cand, entry)) entry = cand, dirty = true;
            }
            __syncthreads();
        }
        if (active) {
            if (walked) {
                ws.exits[a.seg0 + t] = ex;
                ws.dcs[a.seg0 + t] = SegDc{{sink.sum[0], sink.sum[1], sink.sum[2]}, 0u};
            }
            if (t == 0u) ws.gentry[grp] = entry;
            if (t == a.n - 1u) last_out[grp] = ex;
        }
    }
}

__global__ __launch_bounds__(256) void unsplit_settle_kernel(const Call c, const Ws ws, const uint32_t launch,
                                                             hpdct_decode_split_info* __restrict__ info) {
    unsplit_settle_body<unscan::DecodeTables>(c, ws, launch, info, builtin_tables());
}
__global__ __launch_bounds__(256) void unsplit_settle_tables_kernel(const Call c, const Ws ws, const uint32_t launch,
                                                                    hpdct_decode_split_info* __restrict__ info,
                                                                    const unscan::HuffBlob* __restrict__ blob) {
    unsplit_settle_body<unscan::DecodeTablesWide>(c, ws, launch, info, blob_tables(blob));
}

// The offsets launch: workgroup w takes the intervals w, w + gridDim.x, ...; thread t the segments
// [t * per, (t + 1) * per) of the interval.
__global__ __launch_bounds__(256) void unsplit_offsets_kernel(const Call c, const Ws ws,
                                                              hpdct_decode_split_info* __restrict__ info) {
    __shared__ uint64_t s_blk[256];
    __shared__ int64_t s_dc[3][256];
    __shared__ uint32_t s_flag;
    const uint32_t t = threadIdx.x;
    const uint64_t found = c.offs ? 0u : info->markers_found;
    const SegState* last = ws.glast + (unsplit::kRounds & 1u) * ws.ngrp;
    for (uint64_t iv = blockIdx.x; iv < c.g.intervals; iv += gridDim.x) {
        if (ws.ivflag[iv] == 0u) continue;  // uniform
        uint64_t lo, hi;
        bounds_of(c, found, iv, lo, hi);
        const uint64_t nseg = (hi - lo + kS - 1u) / kS, ngrp = (nseg + kG - 1u) / kG;
        const uint64_t seg0 = ws.ivseg[iv], grp0 = ws.ivgrp[iv];
        __syncthreads();  // the interval before is done with the shared arrays
        if (t == 0u) s_flag = 0u;
        __syncthreads();
        uint32_t flag = 0;
        for (uint64_t j = 1u + t; j < ngrp; j += 256u)
            if (!unsplit::same(ws.gentry[grp0 + j], unsplit::entry_of(last[grp0 + j - 1u]))) flag |= unsplit::kIvUnsettled;
        const uint64_t per = (nseg + 255u) / 256u;
        const uint64_t b = t * per < nseg ? t * per : nseg, e = b + per < nseg ? b + per : nseg;
        uint64_t blk = 0;
        int64_t dc[3] = {0, 0, 0};
        for (uint64_t s = b; s < e; ++s) {
            const SegState x = ws.exits[seg0 + s];
            const SegDc d = ws.dcs[seg0 + s];
            if (x.bits & unsplit::kSegErr) flag |= unsplit::kIvBad;
            blk += x.nblk;
            for (int k = 0; k < 3; ++k) dc[k] += d.sum[k];
        }
        s_blk[t] = blk;
        for (int k = 0; k < 3; ++k) s_dc[k][t] = dc[k];
        __syncthreads();
        for (uint32_t d = 1; d < 256u; d <<= 1) {
            const uint64_t ob = t >= d ? s_blk[t - d] : 0u;
            int64_t od[3];
            for (int k = 0; k < 3; ++k) od[k] = t >= d ? s_dc[k][t - d] : 0;
            __syncthreads();
            s_blk[t] += ob;
            for (int k = 0; k < 3; ++k) s_dc[k][t] += od[k];
            __syncthreads();
        }
        SegStart run{s_blk[t] - blk, {s_dc[0][t] - dc[0], s_dc[1][t] - dc[1], s_dc[2][t] - dc[2]}};
        for (uint64_t s = b; s < e; ++s) {
            ws.starts[seg0 + s] = run;
            run.block += ws.exits[seg0 + s].nblk;
            const SegDc d = ws.dcs[seg0 + s];
            for (int k = 0; k < 3; ++k) run.pred[k] += d.sum[k];
        }
        if (t == 255u) {
            if (s_blk[255] != blocks_of(c.g, iv)) flag |= unsplit::kIvBad;
            if (!unsplit::ends_clean(ws.exits[seg0 + nseg - 1u], hi)) flag |= unsplit::kIvBad;
        }
        if (flag != 0u) atomicOr(&s_flag, flag);
        __syncthreads();
        if (t == 0u) {
            ws.ivflag[iv] = unsplit::kIvSplit | s_flag;
            atomicAdd(&info->split_intervals, 1u);
            if (s_flag & unsplit::kIvUnsettled) atomicAdd(&info->unsettled_intervals, 1u);
        }
    }
}

// The clear launch: lane i the 16-byte piece i of the frame's blocks, MCU by MCU; zero where the interval passed.
__global__ __launch_bounds__(256) void unsplit_clear_kernel(const Ws ws, int16_t* __restrict__ y,
                                                            int16_t* __restrict__ cb, int16_t* __restrict__ cr,
                                                            const scan::ScanGrid g) {
    const uint64_t units = static_cast<uint64_t>(g.nmcu) * g.bpm * 8u;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < units; i += gridDim.x * 256ull) {
        const uint64_t blk = i >> 3;
        const uint32_t m = static_cast<uint32_t>(blk / g.bpm), kk = static_cast<uint32_t>(blk % g.bpm);
        if (ws.ivflag[m / g.per_interval] != unsplit::kIvSplit) continue;
        unscan::Vec16* d = reinterpret_cast<unscan::Vec16*>(unscan::block_of_mcu(y, cb, cr, g, m, kk)) + (i & 7u);
        *d = unscan::Vec16{0u, 0u, 0u, 0u};
    }
}

// The write launch: the groups as the settle launches take them; a lane of an interval that passed walks its
// segment from the entry the fixed point gives it and stores what it decodes.
template <unsigned kVar, class Tab>
__device__ inline void unsplit_write_body(const Call& c, const Ws& ws, int16_t* __restrict__ y,
                                          int16_t* __restrict__ cb, int16_t* __restrict__ cr,
                                          const hpdct_decode_split_info* __restrict__ info,
                                          const uint32_t* __restrict__ src) {
    constexpr bool kNatural = (kVar & kScanNatural) != 0u;
    __shared__ uint32_t s_tab[sizeof(Tab) / 4u];
    __shared__ uint8_t s_order[64];
    const uint32_t t = threadIdx.x;
    stage_tables<kG, Tab>(s_tab, src);
    if (t < 64u) s_order[t] = kUnsplitOrder.v[t];
    __syncthreads();
    const Tab* tab = reinterpret_cast<const Tab*>(s_tab);
    const uint64_t found = c.offs ? 0u : info->markers_found, groups = ws.totals[0];
    for (uint64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const GroupAt a = group_at(c, ws, found, grp);
        if ((ws.ivflag[a.iv] & ~unsplit::kIvDc) != unsplit::kIvSplit || t >= a.n) continue;
        const uint64_t q = a.q0 + t;
        const uint64_t end = a.lo + (q + 1u) * kS < a.hi ? a.lo + (q + 1u) * kS : a.hi;
        const SegState entry = t == 0u ? ws.gentry[grp] : unsplit::entry_of(ws.exits[a.seg0 + t - 1u]);
        const SegStart st = ws.starts[a.seg0 + t];
        unsplit::StoreSink<kNatural> sink;
        sink.y = y, sink.cb = cb, sink.cr = cr, sink.g = c.g, sink.order = s_order;
        sink.block = st.block, sink.nblk = blocks_of(c.g, a.iv);
        sink.m = static_cast<uint32_t>(a.iv * c.g.per_interval + st.block / c.g.bpm);
        sink.kk = static_cast<uint32_t>(st.block % c.g.bpm);
        for (int k = 0; k < 3; ++k) sink.pred[k] = st.pred[k];
        sink.seek();
        unsplit::walk_segment(c.scan, a.lo, a.hi, end, entry, c.g.bpm, tab, sink);
        if (sink.dc_bad) atomicOr(&ws.ivflag[a.iv], unsplit::kIvDc);
    }
}

template <unsigned kVar>
__global__ __launch_bounds__(256) void unsplit_write_kernel(const Call c, const Ws ws, int16_t* __restrict__ y,
                                                            int16_t* __restrict__ cb, int16_t* __restrict__ cr,
                                                            const hpdct_decode_split_info* __restrict__ info) {
    unsplit_write_body<kVar, unscan::DecodeTables>(c, ws, y, cb, cr, info, builtin_tables());
}
template <unsigned kVar>
__global__ __launch_bounds__(256) void unsplit_write_tables_kernel(const Call c, const Ws ws, int16_t* __restrict__ y,
                                                                   int16_t* __restrict__ cb, int16_t* __restrict__ cr,
                                                                   const hpdct_decode_split_info* __restrict__ info,
                                                                   const unscan::HuffBlob* __restrict__ blob) {
    unsplit_write_body<kVar, unscan::DecodeTablesWide>(c, ws, y, cb, cr, info, blob_tables(blob));
}

// The serial launch: unscan_decode_kernel's shape; an interval that passed gets status 0, every other one
// hpdct_unscan.hpp's walk, which writes all its blocks.
template <unsigned kVar, class Tab>
__device__ inline void unsplit_serial_body(const Call& c, const Ws& ws, int16_t* __restrict__ y,
                                           int16_t* __restrict__ cb, int16_t* __restrict__ cr,
                                           hpdct_decode_split_info* __restrict__ info, uint64_t* __restrict__ status,
                                           const uint32_t* __restrict__ src) {
    constexpr uint32_t kLanes = unscan_lanes_of(kVar);
    constexpr bool kNatural = (kVar & kScanNatural) != 0u;
    __shared__ uint32_t s_tab[sizeof(Tab) / 4u];
    __shared__ uint32_t s_row[kLanes * scan::kBlkStride];
    __shared__ uint8_t s_order[64];
    const uint32_t lane = threadIdx.x;
    stage_tables<64, Tab>(s_tab, src);
    s_order[lane] = kUnsplitOrder.v[lane];
    __syncthreads();
    const Tab* tab = reinterpret_cast<const Tab*>(s_tab);
    const uint64_t found = c.offs ? 0u : info->markers_found;
    uint32_t bad = 0, serial = 0;
    for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kLanes; base < c.g.intervals;
         base += static_cast<uint64_t>(gridDim.x) * kLanes) {
        const uint64_t iv = base + lane;
        if (lane < kLanes && iv < c.g.intervals) {
            uint64_t st = 0;
            if (ws.ivflag[iv] != unsplit::kIvSplit) {
                uint64_t lo, hi;
                const uint32_t pre = bounds_of(c, found, iv, lo, hi);
                st = unscan::walk_interval<kNatural>(c.scan, lo, hi, pre, iv, c.g, tab, s_order,
                                                     s_row + lane * scan::kBlkStride, y, cb, cr);
                ++serial;
            }
            if (status) status[iv] = st;
            bad += st != 0u;
        }
    }
    for (uint32_t d = 32; d != 0u; d >>= 1) bad += __shfl_xor(bad, d, 64), serial += __shfl_xor(serial, d, 64);
    if (lane == 0u && bad != 0u) atomicAdd(&info->bad_intervals, bad);  // integer: order-independent
    if (lane == 0u && serial != 0u) atomicAdd(&info->serial_intervals, serial);
}

template <unsigned kVar>
__global__ __launch_bounds__(64) void unsplit_serial_kernel(const Call c, const Ws ws, int16_t* __restrict__ y,
                                                            int16_t* __restrict__ cb, int16_t* __restrict__ cr,
                                                            hpdct_decode_split_info* __restrict__ info,
                                                            uint64_t* __restrict__ status) {
    unsplit_serial_body<kVar, unscan::DecodeTables>(c, ws, y, cb, cr, info, status, builtin_tables());
}
template <unsigned kVar>
__global__ __launch_bounds__(64) void unsplit_serial_tables_kernel(const Call c, const Ws ws, int16_t* __restrict__ y,
                                                                   int16_t* __restrict__ cb, int16_t* __restrict__ cr,
                                                                   hpdct_decode_split_info* __restrict__ info,
                                                                   uint64_t* __restrict__ status,
                                                                   const unscan::HuffBlob* __restrict__ blob) {
    unsplit_serial_body<kVar, unscan::DecodeTablesWide>(c, ws, y, cb, cr, info, status, blob_tables(blob));
}

// The pick between the two instantiations of a kernel, for each of the three launches that read the Huffman
// tables: kTables, of variant kV | kScanTables, reads the caller's blob, its last argument; kBuiltin, of variant
// kV, holds Annex K's (blob nullptr).  kTables is named first, as the code object holds the pair
// (profiles/r14/README.md).
template <unsigned kV, auto kTables, auto kBuiltin, typename... Args>
hipError_t launch_choice_tables(const policy::Choice& ch, hipStream_t s, const unscan::HuffBlob* blob,
                                const Args&... args) {
    if (blob) return launch_choice<(kV | kScanTables), kTables>(ch, s, args..., blob);
    return launch_choice<kV, kBuiltin>(ch, s, args...);
}

}  // namespace

hipError_t launch_unscan_split(const uint8_t* scan, uint64_t bytes, const uint64_t* offs, int16_t* y, int16_t* cb,
                               int16_t* cr, const scan::ScanGrid& g, bool natural, uint64_t split_min,
                               hpdct_decode_split_info* info, uint64_t* status, void* workspace,
                               const unscan::HuffBlob* blob, hipStream_t s) {
    const bool tables = blob != nullptr;
    if (hipError_t e = launch_unscan_locate(scan, bytes, offs, g, reinterpret_cast<hpdct_decode_info*>(info), workspace, s))
        return e;
    const unsplit::Layout lay = unsplit::layout(g.intervals, bytes);
    const Ws ws = unsplit::carve(workspace, lay);
    const Call c{scan, bytes, offs, static_cast<const uint64_t*>(workspace), g, split_min};
    constexpr unsigned kPlanV = with_block<1024>(kUnsplitPlan), kSettleV = with_block<256>(kUnsplitSettle);
    constexpr unsigned kOffsetsV = with_block<256>(kUnsplitOffsets), kClearV = with_block<256>(kUnsplitClear);
    if (hipError_t e = launch_choice<kPlanV, unsplit_plan_kernel>(policy::unsplit_plan(), s, c, ws, info)) return e;
    for (uint32_t launch = 0; launch <= unsplit::kRounds; ++launch)
        if (hipError_t e = launch_choice_tables<kSettleV, unsplit_settle_tables_kernel, unsplit_settle_kernel>(
                policy::unsplit_settle(lay.ngrp, tables), s, blob, c, ws, launch, info))
            return e;
    if (hipError_t e = launch_choice<kOffsetsV, unsplit_offsets_kernel>(policy::unsplit_offsets(g.intervals), s, c, ws, info))
        return e;
    const uint64_t units = static_cast<uint64_t>(g.nmcu) * g.bpm * 8u;
    if (hipError_t e = launch_choice<kClearV, unsplit_clear_kernel>(policy::unsplit_clear(units), s, ws, y, cb, cr, g))
        return e;
    const hpdct_decode_split_info* cinfo = info;
    const policy::Choice cw = policy::unsplit_write(lay.ngrp, natural, tables);
    if (hipError_t e = policy::with_bit<kScanNatural, true>(cw.var, [&](auto kN) {
            constexpr unsigned kV = with_block<256>(kUnsplitWrite | decltype(kN)::value);
            return launch_choice_tables<kV, unsplit_write_tables_kernel<(kV | kScanTables)>, unsplit_write_kernel<kV>>(
                cw, s, blob, c, ws, y, cb, cr, cinfo);
        }))
        return e;
    policy::UnscanCall pc;
    pc.intervals = g.intervals, pc.natural = natural, pc.tables = tables;
    const policy::Choice cs = policy::unsplit_serial(pc);
    return with_lanes(cs.var, [&](auto kL) {
        return policy::with_bit<kScanNatural, true>(cs.var, [&](auto kN) {
            constexpr unsigned kV = with_block<64>(kUnsplitSerial | decltype(kN)::value | decltype(kL)::value);
            return launch_choice_tables<kV, unsplit_serial_tables_kernel<(kV | kScanTables)>, unsplit_serial_kernel<kV>>(
                cs, s, blob, c, ws, y, cb, cr, info, status);
        });
    });
}

}  // namespace hpdct
