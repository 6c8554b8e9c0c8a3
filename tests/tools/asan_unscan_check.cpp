// asan_unscan_check.cpp -- the entropy decoder's host side under ASan + UBSan,
// CPU only: a stand-alone program linked with the sanitised host sources of the C ABI (g++; asan.mk's HOST)
// and the library's kernel objects, as asan_scan_check.cpp is.  No kernel is
// launched: every device call here fails its checks first.
//   1. the refusals of hpdct_decode_scan and hpdct_decode_workspace_bytes;
//   2. hpdct_jpeg_parse on every truncation and every single-byte corruption of
//      a valid file, each in a heap buffer of exactly its size;
//   3. unscan::walk_interval, the very function the decode kernel wraps, over the
//      corrupt corpus tests/unscan_corpus.py wrote next to this program
//      (unscan_corpus.bin), scans, offset tables and block arrays in heap buffers
//      of exactly their size, compared with what tests/jpeg_unscan.py expects;
//      every scan at each of the eight addresses mod 8 (the walk's byte cache
//      loads aligned words, so what it loads depends on where the scan lies).
// Built and run by tests/test_jpeg_unscan_host.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "hpdct.h"
#include "hpdct_unscan.hpp"

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
        uintptr_t info, st, ws;
        int64_t wsb;  // too small: the last thing judged, so a call that passes every other check ends there
    };
    const Call ok{SCAN, 4096, OFFS, Y, CB, CR, 16, 32, 1, 0, 0u, INFO, ST, WS, 0};
    auto dec = [](const Call& c) {
        return hpdct_decode_scan(reinterpret_cast<const uint8_t*>(c.scan), c.bytes,
                                 reinterpret_cast<const uint64_t*>(c.offs), reinterpret_cast<int16_t*>(c.y),
                                 reinterpret_cast<int16_t*>(c.cb), reinterpret_cast<int16_t*>(c.cr), c.h, c.w,
                                 static_cast<hpdct_subsampling>(c.sub), c.ri, c.flags,
                                 reinterpret_cast<hpdct_decode_info*>(c.info), reinterpret_cast<uint64_t*>(c.st),
                                 reinterpret_cast<void*>(c.ws), c.wsb, nullptr);
    };
    auto with = [&](auto f) {
        Call c = ok;
        f(c);
        return dec(c);
    };
    const char* kEnd = "workspace too small";
    expect("all good", dec(ok), 1, kEnd);
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
    expect("int64 min", with([](Call& c) { c.h = std::numeric_limits<int64_t>::min(); }), 1, "multiples of");
    expect("2^23 squared", with([](Call& c) { c.h = c.w = int64_t(1) << 23; }), 1, "too large");
    expect("subsampling 2", with([](Call& c) { c.sub = 2; }), 1, "subsampling");
    expect("interval -1", with([](Call& c) { c.ri = -1; }), 1, "restart_interval");
    expect("interval 65536", with([](Call& c) { c.ri = 65536; }), 1, "restart_interval");
    expect("interval 65535", with([](Call& c) { c.ri = 65535; }), 1, kEnd);
    expect("flag 0x80", with([](Call& c) { c.flags = 0x80u; }), 2);
    expect("natural", with([](Call& c) { c.flags = HPDCT_BLOCKS_NATURAL; }), 1, kEnd);
    expect("bytes -1", with([](Call& c) { c.bytes = -1; }), 1, "negative");
    expect("bytes int64 max", with([](Call& c) { c.bytes = std::numeric_limits<int64_t>::max(); }), 1, "overlap");
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
    // overlaps: y 1024 bytes, cb and cr 256, scan 4096, info 16, offsets 16 (24 with two intervals), status 8 (16),
    // workspace 32 (one marker word pair, one chunk word pair)
    expect("cb in y", with([&](Call& c) { c.cb = Y + 1008; }), 1, "overlap");
    expect("cb after y", with([&](Call& c) { c.cb = Y + 1024; }), 1, kEnd);
    expect("scan in y", with([&](Call& c) { c.scan = Y + 1023, c.bytes = 1; }), 1, "overlap");
    expect("scan up to y", with([&](Call& c) { c.scan = Y - 4096; }), 1, kEnd);
    expect("info in scan", with([&](Call& c) { c.info = SCAN + 4088; }), 1, "overlap");
    expect("offsets on info", with([&](Call& c) { c.offs = INFO; }), 1, "overlap");
    expect("status on info", with([&](Call& c) { c.st = INFO; }), 1, "overlap");
    expect("status in offsets", with([&](Call& c) { c.ri = 1, c.st = OFFS + 16; }), 1, "overlap");
    expect("status after offsets", with([&](Call& c) { c.ri = 1, c.st = OFFS + 32; }), 1, kEnd);
    expect("workspace in status", with([&](Call& c) { c.ws = ST; }), 1, "overlap");
    expect("workspace after status", with([&](Call& c) { c.ws = ST + 16; }), 1, kEnd);
    expect("status in workspace", with([&](Call& c) { c.st = WS + 16; }), 1, "overlap");
    expect("status after workspace", with([&](Call& c) { c.st = WS + 32; }), 1, kEnd);
    expect("top of the address space", with([](Call& c) { c.scan = ~uintptr_t(0) - 100; }), 1, "wrap");
    expect("workspace 31", with([](Call& c) { c.wsb = 31; }), 1, kEnd);
    expect("workspace int64 min", with([](Call& c) { c.wsb = std::numeric_limits<int64_t>::min(); }), 1, kEnd);

    const auto S444 = HPDCT_SUBSAMPLING_444, S420 = HPDCT_SUBSAMPLING_420;
    expect_eq("workspace 16x32 420/0, 4096", hpdct_decode_workspace_bytes(16, 32, 3, S420, 0, 4096), 32);
    expect_eq("workspace 16x32 420/0, 4097", hpdct_decode_workspace_bytes(16, 32, 3, S420, 0, 4097), 32);
    expect_eq("workspace 16x32 420/0, 8193", hpdct_decode_workspace_bytes(16, 32, 3, S420, 0, 8193), 48);
    expect_eq("workspace 24x1016/1", hpdct_decode_workspace_bytes(24, 1016, 1, S444, 1, 0), 8 * 382 + 16);
    expect_eq("workspace negative bytes", hpdct_decode_workspace_bytes(16, 32, 3, S420, 0, -1), -1);
    expect_eq("workspace bad components", hpdct_decode_workspace_bytes(16, 32, 2, S420, 1, 0), -1);
    expect_eq("workspace bad size", hpdct_decode_workspace_bytes(16, 24, 3, S420, 1, 0), -1);
    expect_eq("workspace bad interval", hpdct_decode_workspace_bytes(16, 32, 3, S420, 65536, 0), -1);
}

// a valid file: the library's own header, a scan of `scan` bytes, EOI
std::vector<uint8_t> make_file(int components, hpdct_subsampling sub, int64_t ri, const std::vector<uint8_t>& scan) {
    uint8_t head[1024];
    int64_t n = 0;
    expect("header", hpdct_jpeg_header(head, sizeof(head), &n, 45, 70, components, sub, nullptr, nullptr, ri), 0);
    std::vector<uint8_t> f(head, head + n);
    f.insert(f.end(), scan.begin(), scan.end());
    f.push_back(0xff), f.push_back(0xd9);
    return f;
}
int parse_exact(const uint8_t* data, size_t n, hpdct_jpeg_layout* out) {
    std::unique_ptr<uint8_t[]> heap(new uint8_t[n ? n : 1]);  // n bytes are the file: one past them is an ASan report
    if (n) std::memcpy(heap.get(), data, n);
    return hpdct_jpeg_parse(n ? heap.get() : heap.get(), static_cast<int64_t>(n), out);
}

void parser() {
    const std::vector<uint8_t> scan = {0x12, 0x34, 0xff, 0x00, 0x56, 0xff, 0xd0, 0x78, 0xff, 0xd1, 0x9a};
    hpdct_jpeg_layout lay;
    for (int variant = 0; variant < 3; ++variant) {
        const int comps = variant == 0 ? 1 : 3;
        const hpdct_subsampling sub = variant == 2 ? HPDCT_SUBSAMPLING_420 : HPDCT_SUBSAMPLING_444;
        const std::vector<uint8_t> f = make_file(comps, sub, variant == 1 ? 0 : 5, scan);
        expect("parse whole", parse_exact(f.data(), f.size(), &lay), 0);
        expect_eq("height", lay.height, 45);
        expect_eq("width", lay.width, 70);
        expect_eq("components", lay.components, comps);
        expect_eq("sub", lay.sub, sub);
        expect_eq("restart interval", lay.restart_interval, variant == 1 ? 0 : 5);
        expect_eq("scan offset", lay.scan_offset, static_cast<int64_t>(f.size() - scan.size() - 2));
        expect_eq("scan bytes", lay.scan_bytes, static_cast<int64_t>(scan.size()));
        for (size_t n = 0; n < f.size(); ++n) {
            const int st = parse_exact(f.data(), n, &lay);
            if (st != 1) ++g_bad, std::printf("MISMATCH truncation to %zu: status %d\n", n, st);
        }
        // every byte replaced by five other values: any status, no sanitizer report
        std::vector<uint8_t> g = f;
        for (size_t i = 0; i < f.size(); ++i)
            for (uint8_t v : {uint8_t(0x00), uint8_t(0xff), uint8_t(f[i] ^ 0x01), uint8_t(f[i] ^ 0x80), uint8_t(f[i] + 1)}) {
                g[i] = v;
                const int st = parse_exact(g.data(), g.size(), &lay);
                if (st < 0 || st > 2) ++g_bad, std::printf("MISMATCH corruption at %zu: status %d\n", i, st);
                g[i] = f[i];
            }
    }
    expect("parse null file", hpdct_jpeg_parse(nullptr, 10, &lay), 1, "null");
    const uint8_t soi[2] = {0xff, 0xd8};
    expect("parse null layout", hpdct_jpeg_parse(soi, 2, nullptr), 1, "null");
    expect("parse negative length", hpdct_jpeg_parse(soi, -1, &lay), 1, "negative");
}

struct File {
    std::vector<uint8_t> d;
    size_t p = 0;
    bool ok = true;
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

// one case of the corpus through the walker, as the kernels go through it: the markers located by a plain loop.
// shift: the scan's address mod 8; it ends where its heap buffer ends, the bytes before it are FF.
template <bool kNatural>
bool run_case(File& f, uint32_t index, uint32_t shift) {
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
    // exact-size heap buffers (at least one element: a zero-size new[] may not be read at all, which is the point)
    std::unique_ptr<uint8_t[]> scan_heap(new uint8_t[shift + bytes]);  // operator new[]: 16-byte aligned
    if ((reinterpret_cast<uintptr_t>(scan_heap.get()) & 7u) != 0u) return false;
    std::memset(scan_heap.get(), 0xff, shift);
    uint8_t* const scan_buf = scan_heap.get() + shift;
    f.read(scan_buf, bytes);
    std::unique_ptr<uint64_t[]> offs(new uint64_t[has_offs ? intervals + 1u : 0u]);
    if (has_offs) f.read(offs.get(), 8u * (intervals + 1u));
    std::vector<uint64_t> want_status(intervals);
    f.read(want_status.data(), 8u * intervals);
    const size_t ny = 64u * ty * tx, nc = comps == 3u ? 64u * g.nmcu : 0u;
    std::vector<int16_t> want_y(ny), want_cb(nc), want_cr(nc);
    f.read(want_y.data(), 2u * ny), f.read(want_cb.data(), 2u * nc), f.read(want_cr.data(), 2u * nc);
    if (!f.ok) return false;
    std::unique_ptr<int16_t[]> y(new int16_t[ny]), cb(new int16_t[nc]), cr(new int16_t[nc]);
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
    static const unscan::DecodeTables tables = unscan::make_decode_tables();
    uint8_t order[64];
    for (int n = 0; n < 64; ++n) order[n] = zigzag::kOrder[n];
    bool same = found == want_found && errors == want_errors;
    for (uint64_t iv = 0; iv < intervals; ++iv) {
        uint64_t lo, hi;
        const uint32_t pre = has_offs ? unscan::bounds_given(offs.get(), iv, intervals, bytes, lo, hi)
                                      : unscan::bounds_located(mpos.get(), found, iv, bytes, lo, hi);
        alignas(16) uint32_t row[32];
        const uint64_t st = unscan::walk_interval<kNatural>(scan_buf, lo, hi, pre, iv, g, &tables, order, row,
                                                            y.get(), nc ? cb.get() : nullptr, nc ? cr.get() : nullptr);
        same = same && st == want_status[iv];
    }
    auto blocks_equal = [&](const int16_t* got, const std::vector<int16_t>& want) {
        for (size_t i = 0; i < want.size(); ++i) {
            const size_t n = i & 63u, at = kNatural ? (i - n) + zigzag::kOrder[n] : i;
            if (got[at] != want[i]) return false;
        }
        return true;
    };
    same = same && blocks_equal(y.get(), want_y) && blocks_equal(cb.get(), want_cb) && blocks_equal(cr.get(), want_cr);
    if (!same) {
        ++g_bad;
        if (g_bad < 20)
            std::printf("MISMATCH corpus case %u (%s order, address %u mod 8)\n", index,
                        kNatural ? "natural" : "zig-zag", shift);
    }
    return true;
}

void corpus(const char* argv0) {
    std::string path(argv0);
    const size_t slash = path.rfind('/');
    path = (slash == std::string::npos ? std::string(".") : path.substr(0, slash)) + "/unscan_corpus.bin";
    std::FILE* fp = std::fopen(path.c_str(), "rb");
    if (!fp) {
        ++g_bad;
        std::printf("MISMATCH %s: not found\n", path.c_str());
        return;
    }
    File f;
    uint8_t buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof(buf), fp)) > 0;) f.d.insert(f.d.end(), buf, buf + n);
    std::fclose(fp);
    const uint32_t count = f.u32();
    uint32_t done = 0;
    for (; done < count; ++done) {
        // zig-zag order at every address mod 8, natural order (the same walk, another store index) at two
        const size_t at = f.p;
        bool read = true;
        for (uint32_t shift = 0; shift < 8u && read; ++shift) {
            f.p = at;
            read = run_case<false>(f, done, shift);
            if (read && (shift == 0u || shift == 5u)) {
                f.p = at;
                read = run_case<true>(f, done, shift);
            }
        }
        if (!read) break;
    }
    if (done != count || f.p != f.d.size() || count < 1000u) {
        ++g_bad;
        std::printf("MISMATCH corpus file: %u of %u cases read\n", done, count);
    }
    std::printf("asan_unscan_check: %u corpus cases, eight addresses, both block orders\n", done);
}
}  // namespace

int main(int, char** argv) {
    refusals();
    parser();
    corpus(argv[0]);
    if (g_bad) {
        std::printf("asan_unscan_check: %d mismatches\n", g_bad);
        return 1;
    }
    std::printf("asan_unscan_check: ok\n");
    return 0;
}
