// asan_unscan_split_check.cpp -- the split entropy decoder under ASan + UBSan,
// CPU only: a stand-alone program linked with the sanitised host sources of the C ABI (g++; asan.mk's HOST)
// and the library's kernel objects, as asan_unscan_check.cpp is.  No kernel is
// launched: every device call here fails its checks first.
//   1. the refusals of hpdct_decode_scan_split and
//      hpdct_decode_split_workspace_bytes: those of hpdct_decode_scan, a negative
//      split_min_bytes, a workspace one byte short;
//   2. the whole algorithm of hpdct_unscan_split.hpp with lanes as loops over the
//      very unsplit::walk_segment the kernels call -- the plan, the settle
//      launches, the offsets, the clear, the write and the serial pass -- over
//      the corpus tests/test_unscan_split_host.py wrote next to this program
//      (unscan_corpus.bin, split_min_bytes = 1), every array of the workspace in
//      a heap buffer of exactly its budget, the scan at each of the eight
//      addresses mod 8, both block orders; the blocks and status are compared
//      with unscan::walk_interval's and the file's, the four counters with the
//      restatement's (unscan_split_counts.bin).
// Built and run by tests/test_unscan_split_host.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "hpdct.h"
#include "hpdct_unscan_split.hpp"

namespace {
int g_bad = 0;
void expect(const char* what, int got, int want, const char* text = nullptr) {
    const bool ok = got == want && (!text || std::strstr(hpdct_last_error_string(), text));
    if (!ok) {
        ++g_bad;
        std::printf("MISMATCH %s: status %d (expected %d), last error \"%s\"\n", what, got, want,
                    hpdct_last_error_string());
    }
}
void expect_eq(const char* what, int64_t got, int64_t want) {
    if (got != want) {
        ++g_bad;
        std::printf("MISMATCH %s: %lld (expected %lld)\n", what, static_cast<long long>(got),
                    static_cast<long long>(want));
    }
}

void refusals() {
    // never dereferenced: validation fails first.  Far apart, 16-byte aligned.
    auto fake = [](int shift) { return uintptr_t(1) << shift; };
    const uintptr_t Y = fake(30), CB = fake(31), CR = fake(32), SCAN = fake(33), INFO = fake(34), OFFS = fake(35),
                    WS = fake(36), ST = fake(37);
    struct Call {
        uintptr_t scan;
        int64_t bytes;
        uintptr_t offs, y, cb, cr;
        int64_t h, w;
        int sub;
        int64_t ri;
        unsigned flags;
        int64_t split_min;
        uintptr_t info, st, ws;
        int64_t wsb;  // too small: the last thing judged, so a call that passes every other check ends there
    };
    const Call ok{SCAN, 4096, OFFS, Y, CB, CR, 16, 32, 1, 0, 0u, 0, INFO, ST, WS, 0};
    auto dec = [](const Call& c) {
        return hpdct_decode_scan_split(reinterpret_cast<const uint8_t*>(c.scan), c.bytes,
                                       reinterpret_cast<const uint64_t*>(c.offs), reinterpret_cast<int16_t*>(c.y),
                                       reinterpret_cast<int16_t*>(c.cb), reinterpret_cast<int16_t*>(c.cr), c.h, c.w,
                                       static_cast<hpdct_subsampling>(c.sub), c.ri, c.flags, c.split_min,
                                       reinterpret_cast<hpdct_decode_split_info*>(c.info),
                                       reinterpret_cast<uint64_t*>(c.st), reinterpret_cast<void*>(c.ws), c.wsb, nullptr);
    };
    auto with = [&](auto f) {
        Call c = ok;
        f(c);
        return dec(c);
    };
    const char* kEnd = "workspace too small";
    expect("all good", dec(ok), 1, kEnd);
    expect("split_min 1", with([](Call& c) { c.split_min = 1; }), 1, kEnd);
    expect("split_min int64 max", with([](Call& c) { c.split_min = std::numeric_limits<int64_t>::max(); }), 1, kEnd);
    expect("split_min -1", with([](Call& c) { c.split_min = -1; }), 1, "split_min_bytes");
    expect("grey", with([](Call& c) { c.cb = c.cr = 0, c.h = 8, c.w = 8, c.sub = 77; }), 1, kEnd);
    expect("no offsets", with([](Call& c) { c.offs = 0; }), 1, kEnd);
    expect("no status", with([](Call& c) { c.st = 0; }), 1, kEnd);
    expect("null y", with([](Call& c) { c.y = 0; }), 1, "null");
    expect("null scan", with([](Call& c) { c.scan = 0; }), 1, "null");
    expect("null info", with([](Call& c) { c.info = 0; }), 1, "null");
    expect("null workspace", with([](Call& c) { c.ws = 0; }), 1, "null");
    expect("cb without cr", with([](Call& c) { c.cr = 0; }), 1, "null");
    expect("cr without cb", with([](Call& c) { c.cb = 0; }), 1, "null");
    expect("0 rows", with([](Call& c) { c.h = 0; }), 1, "multiples of");
    expect("420 24 rows", with([](Call& c) { c.h = 24; }), 1, "multiples of 16");
    expect("444 24 rows", with([](Call& c) { c.h = 24, c.sub = 0; }), 1, kEnd);
    expect("444 12 rows", with([](Call& c) { c.h = 12, c.sub = 0; }), 1, "multiples of 8");
    expect("2^23 squared", with([](Call& c) { c.h = c.w = int64_t(1) << 23; }), 1, "too large");
    expect("subsampling 2", with([](Call& c) { c.sub = 2; }), 1, "subsampling");
    expect("interval -1", with([](Call& c) { c.ri = -1; }), 1, "restart_interval");
    expect("interval 65536", with([](Call& c) { c.ri = 65536; }), 1, "restart_interval");
    expect("interval 65535", with([](Call& c) { c.ri = 65535; }), 1, kEnd);
    expect("flag 0x80", with([](Call& c) { c.flags = 0x80u; }), 2);
    expect("natural", with([](Call& c) { c.flags = HPDCT_BLOCKS_NATURAL; }), 1, kEnd);
    expect("bytes -1", with([](Call& c) { c.bytes = -1; }), 1, "negative");
    expect("bytes 0", with([](Call& c) { c.bytes = 0; }), 1, kEnd);
    expect("y + 8", with([](Call& c) { c.y += 8; }), 1, "aligned");
    expect("cb + 2", with([](Call& c) { c.cb += 2; }), 1, "aligned");
    expect("cr + 4", with([](Call& c) { c.cr += 4; }), 1, "aligned");
    expect("workspace + 8", with([](Call& c) { c.ws += 8; }), 1, "aligned");
    expect("offsets + 8", with([](Call& c) { c.offs += 8; }), 1, "aligned");
    expect("status + 8", with([](Call& c) { c.st += 8; }), 1, "aligned");
    expect("info + 4", with([](Call& c) { c.info += 4; }), 1, "aligned");
    expect("info + 8", with([](Call& c) { c.info += 8; }), 1, kEnd);
    expect("scan + 1", with([](Call& c) { c.scan += 1; }), 1, kEnd);
    // overlaps: y 1024 bytes, cb and cr 256, scan 4096, info 32, offsets 16 (24 with two intervals), status 8 (16)
    const int64_t need = hpdct_decode_split_workspace_bytes(16, 32, 3, HPDCT_SUBSAMPLING_420, 0, 4096);
    const int64_t need2 = hpdct_decode_split_workspace_bytes(16, 32, 3, HPDCT_SUBSAMPLING_420, 1, 4096);
    expect("cb in y", with([&](Call& c) { c.cb = Y + 1008; }), 1, "overlap");
    expect("cb after y", with([&](Call& c) { c.cb = Y + 1024; }), 1, kEnd);
    expect("scan in y", with([&](Call& c) { c.scan = Y + 1023, c.bytes = 1; }), 1, "overlap");
    expect("scan up to y", with([&](Call& c) { c.scan = Y - 4096; }), 1, kEnd);
    expect("info in scan", with([&](Call& c) { c.info = SCAN + 4088; }), 1, "overlap");
    expect("scan in the info's last words", with([&](Call& c) { c.scan = INFO + 16; }), 1, "overlap");
    expect("scan after info", with([&](Call& c) { c.scan = INFO + 32; }), 1, kEnd);
    expect("offsets on info", with([&](Call& c) { c.offs = INFO; }), 1, "overlap");
    expect("status on info", with([&](Call& c) { c.st = INFO; }), 1, "overlap");
    expect("status in offsets", with([&](Call& c) { c.ri = 1, c.st = OFFS + 16; }), 1, "overlap");
    expect("status after offsets", with([&](Call& c) { c.ri = 1, c.st = OFFS + 32; }), 1, kEnd);
    expect("workspace in status", with([&](Call& c) { c.ws = ST; }), 1, "overlap");
    expect("workspace after status", with([&](Call& c) { c.ws = ST + 16; }), 1, kEnd);
    expect("status in workspace", with([&](Call& c) { c.st = WS + uintptr_t(need) - 16; }), 1, "overlap");
    expect("status after workspace", with([&](Call& c) { c.st = WS + uintptr_t(need); }), 1, kEnd);
    expect("top of the address space", with([](Call& c) { c.scan = ~uintptr_t(0) - 100; }), 1, "wrap");
    expect("workspace one byte short", with([&](Call& c) { c.wsb = need - 1; }), 1, kEnd);
    expect("workspace one byte short, two intervals", with([&](Call& c) { c.ri = 1, c.wsb = need2 - 1; }), 1, kEnd);
    expect("workspace int64 min", with([](Call& c) { c.wsb = std::numeric_limits<int64_t>::min(); }), 1, kEnd);

    const auto S444 = HPDCT_SUBSAMPLING_444, S420 = HPDCT_SUBSAMPLING_420;
    const hpdct::unsplit::Layout l = hpdct::unsplit::layout(1, 4096);
    expect_eq("budget of segments", static_cast<int64_t>(l.nseg), 4096 / hpdct::unsplit::kSegBytes + 1);
    expect_eq("workspace 16x32 420/0, 4096", need, static_cast<int64_t>(l.bytes));
    expect_eq("workspace multiple of 16", need % 16, 0);
    expect_eq("workspace above the serial call's", need > hpdct_decode_workspace_bytes(16, 32, 3, S420, 0, 4096), 1);
    expect_eq("workspace negative bytes", hpdct_decode_split_workspace_bytes(16, 32, 3, S420, 0, -1), -1);
    expect_eq("workspace bad components", hpdct_decode_split_workspace_bytes(16, 32, 2, S420, 1, 0), -1);
    expect_eq("workspace bad size", hpdct_decode_split_workspace_bytes(16, 24, 3, S420, 1, 0), -1);
    expect_eq("workspace bad interval", hpdct_decode_split_workspace_bytes(16, 32, 3, S444, 65536, 0), -1);
    int s = 0, g = 0, r = 0;
    hpdct_decode_split_geometry(&s, &g, &r);
    hpdct_decode_split_geometry(nullptr, nullptr, nullptr);
    expect_eq("geometry", s == int(hpdct::unsplit::kSegBytes) && g == int(hpdct::unsplit::kGroup) &&
                              r == int(hpdct::unsplit::kRounds), 1);
}

struct File {
    std::vector<uint8_t> d;
    size_t p = 0;
    bool ok = true;
    bool load(const std::string& path) {
        std::FILE* fp = std::fopen(path.c_str(), "rb");
        if (!fp) return false;
        uint8_t buf[65536];
        for (size_t n; (n = std::fread(buf, 1, sizeof(buf), fp)) > 0;) d.insert(d.end(), buf, buf + n);
        std::fclose(fp);
        return true;
    }
    void read(void* out, size_t n) {
        if (n == 0u) return;
        if (p + n > d.size()) {
            ok = false;
            return;
        }
        std::memcpy(out, d.data() + p, n);
        p += n;
    }
    uint32_t u32() {
        uint32_t v = 0;
        read(&v, 4);
        return v;
    }
};

struct Counts {
    uint32_t split = 0, serial = 0, unsettled = 0, rounds = 0;
};

// an array of the workspace: exactly n elements on the heap
template <typename T>
std::unique_ptr<T[]> exact(uint64_t n) {
    return std::unique_ptr<T[]>(new T[n]);
}

// hpdct_unscan_split.hip's launches, lanes and workgroups as loops.  offs: the caller's table or nullptr (mpos, found).
template <bool kNatural>
Counts decode_split(const uint8_t* scan, uint64_t bytes, const uint64_t* offs, const uint64_t* mpos, uint64_t found,
                    const hpdct::scan::ScanGrid& g, uint64_t split_min, int16_t* y, int16_t* cb, int16_t* cr,
                    uint64_t* status) {
    using namespace hpdct;
    using namespace hpdct::unsplit;
    static const unscan::DecodeTables tables = unscan::make_decode_tables();
    uint8_t order[64];
    for (int n = 0; n < 64; ++n) order[n] = zigzag::kOrder[n];
    const Layout l = layout(g.intervals, bytes);
    const uint64_t n = g.intervals;
    auto ivseg = exact<uint64_t>(n + 1), ivgrp = exact<uint64_t>(n + 1);
    auto ivflag = exact<uint32_t>(n);
    auto grpiv = exact<uint32_t>(l.ngrp);
    auto gentry = exact<SegState>(l.ngrp), glast = exact<SegState>(2 * l.ngrp);
    auto exits = exact<SegState>(l.nseg);
    auto dcs = exact<SegDc>(l.nseg);
    auto starts = exact<SegStart>(l.nseg);
    auto bounds = [&](uint64_t iv, uint64_t& lo, uint64_t& hi) {
        return offs ? unscan::bounds_given(offs, iv, n, bytes, lo, hi) : unscan::bounds_located(mpos, found, iv, bytes, lo, hi);
    };
    auto blocks_of = [&](uint64_t iv) {
        const uint64_t m0 = iv * g.per_interval;
        return (g.nmcu - m0 < g.per_interval ? g.nmcu - m0 : g.per_interval) * g.bpm;
    };
    Counts c;
    // plan
    uint64_t rs = 0, rg = 0, groups = 0;
    const uint64_t cap = l.nseg + 1u;
    for (uint64_t iv = 0; iv < n; ++iv) {
        uint64_t lo, hi;
        const uint32_t pre = bounds(iv, lo, hi);
        const uint64_t k = segments_of(pre, lo, hi, split_min);
        const uint64_t after = sat_add(rs, k < cap ? k : cap, cap);
        const bool fits = k != 0u && after <= l.nseg;
        ivseg[iv] = rs, ivgrp[iv] = rg, ivflag[iv] = fits ? kIvSplit : 0u;
        if (fits) {
            const uint64_t ng = (k + kGroup - 1u) / kGroup;
            for (uint64_t j = 0; j < ng; ++j) grpiv[rg + j] = static_cast<uint32_t>(iv);
            groups = rg + ng;
        }
        rs = after, rg = sat_add(rg, k < cap ? (k + kGroup - 1u) / kGroup : cap, cap);
    }
    struct At {
        uint64_t iv, lo, hi, q0, seg0;
        uint32_t cnt;
    };
    auto group_at = [&](uint64_t grp) {
        At a;
        a.iv = grpiv[grp];
        bounds(a.iv, a.lo, a.hi);
        const uint64_t nseg = (a.hi - a.lo + kSegBytes - 1u) / kSegBytes;
        a.q0 = (grp - ivgrp[a.iv]) * kGroup, a.seg0 = ivseg[a.iv] + a.q0;
        a.cnt = static_cast<uint32_t>(nseg - a.q0 < kGroup ? nseg - a.q0 : kGroup);
        return a;
    };
    auto seg_end = [](const At& a, uint32_t t) {
        const uint64_t e = a.lo + (a.q0 + t + 1u) * kSegBytes;
        return e < a.hi ? e : a.hi;
    };
    // settle
    for (uint32_t launch = 0; launch <= kRounds; ++launch) {
        const SegState* last_in = glast.get() + ((launch + 1u) & 1u) * l.ngrp;
        SegState* last_out = glast.get() + (launch & 1u) * l.ngrp;
        for (uint64_t grp = 0; grp < groups; ++grp) {
            const At a = group_at(grp);
            SegState entry0;
            if (launch == 0u) {
                entry0 = boundary_entry(scan, a.lo, a.hi, a.q0);
            } else {
                if (a.q0 == 0u || same(entry_of(last_in[grp - 1u]), gentry[grp])) {
                    last_out[grp] = last_in[grp];
                    continue;
                }
                entry0 = entry_of(last_in[grp - 1u]);
                if (c.rounds < launch) c.rounds = launch;
            }
            // the fixed point of the group's rounds: the chain from entry0; at launch 0 every lane walked from its
            // boundary first, which leaves no trace in it
            SegState entry = entry0;
            for (uint32_t t = 0; t < a.cnt; ++t) {
                if (launch == 0u) {  // the speculative walk, for the sanitizers
                    CountSink spec;
                    walk_segment(scan, a.lo, a.hi, seg_end(a, t), boundary_entry(scan, a.lo, a.hi, a.q0 + t), g.bpm,
                                 &tables, spec);
                }
                CountSink sink;
                const SegState ex = walk_segment(scan, a.lo, a.hi, seg_end(a, t), entry, g.bpm, &tables, sink);
                exits[a.seg0 + t] = ex;
                dcs[a.seg0 + t] = SegDc{{sink.sum[0], sink.sum[1], sink.sum[2]}, 0u};
                entry = entry_of(ex);
            }
            gentry[grp] = entry0;
            last_out[grp] = exits[a.seg0 + a.cnt - 1u];
        }
    }
    // offsets
    const SegState* last = glast.get() + (kRounds & 1u) * l.ngrp;
    for (uint64_t iv = 0; iv < n; ++iv) {
        if (ivflag[iv] == 0u) continue;
        uint64_t lo, hi;
        bounds(iv, lo, hi);
        const uint64_t nseg = (hi - lo + kSegBytes - 1u) / kSegBytes, ngrp = (nseg + kGroup - 1u) / kGroup;
        uint32_t flag = 0;
        for (uint64_t j = 1; j < ngrp; ++j)
            if (!same(gentry[ivgrp[iv] + j], entry_of(last[ivgrp[iv] + j - 1u]))) flag |= kIvUnsettled;
        SegStart run{0u, {0, 0, 0}};
        for (uint64_t s = 0; s < nseg; ++s) {
            const SegState x = exits[ivseg[iv] + s];
            if (x.bits & kSegErr) flag |= kIvBad;
            starts[ivseg[iv] + s] = run;
            run.block += x.nblk;
            for (int k = 0; k < 3; ++k) run.pred[k] += dcs[ivseg[iv] + s].sum[k];
        }
        if (run.block != blocks_of(iv) || !ends_clean(exits[ivseg[iv] + nseg - 1u], hi)) flag |= kIvBad;
        ivflag[iv] = kIvSplit | flag;
        ++c.split;
        if (flag & kIvUnsettled) ++c.unsettled;
    }
    // clear
    for (uint64_t blk = 0; blk < uint64_t(g.nmcu) * g.bpm; ++blk) {
        const uint32_t m = static_cast<uint32_t>(blk / g.bpm), kk = static_cast<uint32_t>(blk % g.bpm);
        if (ivflag[m / g.per_interval] == kIvSplit) std::memset(unscan::block_of_mcu(y, cb, cr, g, m, kk), 0, 128);
    }
    // write
    for (uint64_t grp = 0; grp < groups; ++grp) {
        const At a = group_at(grp);
        if ((ivflag[a.iv] & ~kIvDc) != kIvSplit) continue;
        for (uint32_t t = 0; t < a.cnt; ++t) {
            const SegState entry = t == 0u ? gentry[grp] : entry_of(exits[a.seg0 + t - 1u]);
            const SegStart st = starts[a.seg0 + t];
            StoreSink<kNatural> sink;
            sink.y = y, sink.cb = cb, sink.cr = cr, sink.g = g, sink.order = order;
            sink.block = st.block, sink.nblk = blocks_of(a.iv);
            sink.m = static_cast<uint32_t>(a.iv * g.per_interval + st.block / g.bpm);
            sink.kk = static_cast<uint32_t>(st.block % g.bpm);
            for (int k = 0; k < 3; ++k) sink.pred[k] = st.pred[k];
            sink.seek();
            const SegState ex = walk_segment(scan, a.lo, a.hi, seg_end(a, t), entry, g.bpm, &tables, sink);
            if (!same(ex, exits[a.seg0 + t])) ++g_bad, std::printf("MISMATCH the write walk's exit\n");
            if (sink.dc_bad) ivflag[a.iv] |= kIvDc;
        }
    }
    // serial
    for (uint64_t iv = 0; iv < n; ++iv) {
        uint64_t st = 0;
        if (ivflag[iv] != kIvSplit) {
            uint64_t lo, hi;
            const uint32_t pre = bounds(iv, lo, hi);
            alignas(16) uint32_t row[32];
            st = unscan::walk_interval<kNatural>(scan, lo, hi, pre, iv, g, &tables, order, row, y, cb, cr);
            ++c.serial;
        }
        status[iv] = st;
    }
    return c;
}

// one case of the corpus.  shift: the scan's address mod 8; it ends where its heap buffer ends.
template <bool kNatural>
bool run_case(File& f, const Counts* want_counts, uint32_t index, uint32_t shift, Counts& total) {
    using namespace hpdct;
    const uint32_t comps = f.u32(), sub = f.u32(), ty = f.u32(), tx = f.u32(), ri = f.u32(), has_offs = f.u32(),
                   intervals = f.u32(), want_found = f.u32(), want_errors = f.u32();
    f.u32();
    uint64_t bytes = 0;
    f.read(&bytes, 8);
    if (!f.ok || comps == 0u || bytes > f.d.size()) return false;
    const bool s420 = comps == 3u && sub == 1u;
    scan::ScanGrid g;
    g.mcus_x = s420 ? tx / 2u : tx;
    g.nmcu = (s420 ? ty / 2u : ty) * g.mcus_x;
    g.per_interval = ri == 0u ? g.nmcu : ri;
    g.intervals = g.nmcu / g.per_interval + (g.nmcu % g.per_interval != 0u);
    g.bpm = comps == 1u ? 1u : s420 ? 6u : 3u;
    if (g.intervals != intervals) return false;
    std::unique_ptr<uint8_t[]> scan_heap(new uint8_t[shift + bytes]);
    if ((reinterpret_cast<uintptr_t>(scan_heap.get()) & 7u) != 0u) return false;
    std::memset(scan_heap.get(), 0xff, shift);
    uint8_t* const scan_buf = scan_heap.get() + shift;
    f.read(scan_buf, bytes);
    std::unique_ptr<uint64_t[]> offs(new uint64_t[has_offs ? intervals + 1u : 0u]);
    if (has_offs) f.read(offs.get(), 8u * (intervals + 1u));
    std::vector<uint64_t> want_status(intervals), status(intervals), serial_status(intervals);
    f.read(want_status.data(), 8u * intervals);
    const size_t ny = 64u * ty * tx, nc = comps == 3u ? 64u * g.nmcu : 0u;
    std::vector<int16_t> want_y(ny), want_cb(nc), want_cr(nc);
    f.read(want_y.data(), 2u * ny), f.read(want_cb.data(), 2u * nc), f.read(want_cr.data(), 2u * nc);
    if (!f.ok) return false;
    auto y = exact<int16_t>(ny), cb = exact<int16_t>(nc), cr = exact<int16_t>(nc);
    auto sy = exact<int16_t>(ny), scb = exact<int16_t>(nc), scr = exact<int16_t>(nc);
    std::memset(y.get(), 0x5a, 2u * ny);
    if (nc) std::memset(cb.get(), 0x5a, 2u * nc), std::memset(cr.get(), 0x5a, 2u * nc);

    std::unique_ptr<uint64_t[]> mpos(new uint64_t[intervals]);
    uint64_t found = 0, errors = 0;
    if (!has_offs)
        for (uint64_t p = 0; p < bytes; ++p)
            if (unscan::marker_at(scan_buf, p, bytes)) {
                if (found < intervals) {
                    mpos[found] = p;
                    if (found + 1u < intervals && (scan_buf[p + 1u] & 7u) != (found & 7u)) ++errors;
                }
                ++found;
            }
    bool same = found == want_found && errors == want_errors;
    const Counts c = decode_split<kNatural>(scan_buf, bytes, has_offs ? offs.get() : nullptr, mpos.get(), found, g, 1u,
                                            y.get(), nc ? cb.get() : nullptr, nc ? cr.get() : nullptr, status.data());
    // the parent's walk, interval by interval
    static const unscan::DecodeTables tables = unscan::make_decode_tables();
    uint8_t order[64];
    for (int n = 0; n < 64; ++n) order[n] = zigzag::kOrder[n];
    for (uint64_t iv = 0; iv < intervals; ++iv) {
        uint64_t lo, hi;
        const uint32_t pre = has_offs ? unscan::bounds_given(offs.get(), iv, intervals, bytes, lo, hi)
                                      : unscan::bounds_located(mpos.get(), found, iv, bytes, lo, hi);
        alignas(16) uint32_t row[32];
        serial_status[iv] = unscan::walk_interval<kNatural>(scan_buf, lo, hi, pre, iv, g, &tables, order, row, sy.get(),
                                                            nc ? scb.get() : nullptr, nc ? scr.get() : nullptr);
    }
    same = same && status == want_status && serial_status == want_status;
    same = same && std::memcmp(y.get(), sy.get(), 2u * ny) == 0;
    if (nc) same = same && std::memcmp(cb.get(), scb.get(), 2u * nc) == 0 && std::memcmp(cr.get(), scr.get(), 2u * nc) == 0;
    auto blocks_equal = [&](const int16_t* got, const std::vector<int16_t>& want) {
        for (size_t i = 0; i < want.size(); ++i) {
            const size_t n = i & 63u, at = kNatural ? (i - n) + zigzag::kOrder[n] : i;
            if (got[at] != want[i]) return false;
        }
        return true;
    };
    same = same && blocks_equal(y.get(), want_y) && blocks_equal(cb.get(), want_cb) && blocks_equal(cr.get(), want_cr);
    if (want_counts) {
        const Counts& w = want_counts[index];
        same = same && c.split == w.split && c.serial == w.serial && c.unsettled == w.unsettled && c.rounds == w.rounds;
    }
    if (shift == 0u && !kNatural)
        total.split += c.split, total.serial += c.serial, total.unsettled += c.unsettled,
            total.rounds = total.rounds < c.rounds ? c.rounds : total.rounds;
    if (!same) {
        ++g_bad;
        if (g_bad < 20)
            std::printf("MISMATCH corpus case %u (%s order, address %u mod 8): split %u serial %u unsettled %u rounds %u\n",
                        index, kNatural ? "natural" : "zig-zag", shift, c.split, c.serial, c.unsettled, c.rounds);
    }
    return true;
}

void corpus(const char* argv0) {
    std::string dir(argv0);
    const size_t slash = dir.rfind('/');
    dir = slash == std::string::npos ? std::string(".") : dir.substr(0, slash);
    File f, counts;
    if (!f.load(dir + "/unscan_corpus.bin")) {
        ++g_bad;
        std::printf("MISMATCH %s/unscan_corpus.bin: not found\n", dir.c_str());
        return;
    }
    const uint32_t count = f.u32();
    std::vector<Counts> want;
    if (counts.load(dir + "/unscan_split_counts.bin")) {  // the restatement's four counters per case
        want.resize(count);
        counts.read(want.data(), sizeof(Counts) * count);
        if (!counts.ok || counts.p != counts.d.size()) ++g_bad, std::printf("MISMATCH unscan_split_counts.bin: its size\n");
    } else {
        ++g_bad, std::printf("MISMATCH %s/unscan_split_counts.bin: not found\n", dir.c_str());
    }
    uint32_t done = 0;
    Counts total;
    for (; done < count; ++done) {
        const size_t at = f.p;
        bool read = true;
        for (uint32_t shift = 0; shift < 8u && read; ++shift) {
            f.p = at;
            read = run_case<false>(f, want.empty() ? nullptr : want.data(), done, shift, total);
            if (read && (shift == 0u || shift == 5u)) {
                f.p = at;
                read = run_case<true>(f, want.empty() ? nullptr : want.data(), done, shift, total);
            }
        }
        if (!read) break;
    }
    if (done != count || f.p != f.d.size() || count < 1000u) {
        ++g_bad;
        std::printf("MISMATCH corpus file: %u of %u cases read\n", done, count);
    }
    std::printf("asan_unscan_split_check: %u corpus cases, eight addresses, both block orders; intervals split %u, "
                "walked by one lane %u, unsettled %u, most rounds %u\n",
                done, total.split, total.serial, total.unsettled, total.rounds);
}
}  // namespace

int main(int, char** argv) {
    refusals();
    corpus(argv[0]);
    if (g_bad) {
        std::printf("asan_unscan_split_check: %d mismatches\n", g_bad);
        return 1;
    }
    std::printf("asan_unscan_split_check: ok\n");
    return 0;
}
