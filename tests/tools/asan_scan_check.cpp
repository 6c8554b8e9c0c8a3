// asan_scan_check.cpp -- drives the validation paths of hpdct_encode_scan, the
// host calls beside it (hpdct_scan_bound, hpdct_scan_workspace_bytes,
// hpdct_huffman_table) and the header writer hpdct_jpeg_header under ASan +
// UBSan, CPU only: a stand-alone program linked with the sanitised host sources
// of the C ABI (g++; asan.mk's HOST) and the library's kernel objects, as
// asan_rgb_frame_check.cpp is.  No
// kernel is launched: every device call here fails its checks first.
// Built and run by tests/test_jpeg_scan_host.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>

#include "hpdct.h"

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
}  // namespace

int main() {
    // never dereferenced: validation fails first.  Far apart, 16-byte aligned.
    auto fake = [](int shift) { return uintptr_t(1) << shift; };
    const uintptr_t Y = fake(30), CB = fake(31), CR = fake(32), SCAN = fake(33), INFO = fake(34), OFFS = fake(35),
                    WS = fake(36);
    const auto S444 = HPDCT_SUBSAMPLING_444, S420 = HPDCT_SUBSAMPLING_420;
    struct Call {
        uintptr_t y, cb, cr;
        int64_t h = 16, w = 32;
        int sub = 1;
        int64_t ri = 0;
        unsigned flags = 0;
        uintptr_t scan;
        int64_t cap = 4096;
        uintptr_t info, offs, ws;
        int64_t wsb = 0;  // too small: the last thing judged, so a call that passes every other check ends there
    };
    const Call ok{Y, CB, CR, 16, 32, 1, 0, 0u, SCAN, 4096, INFO, OFFS, WS, 0};
    auto enc = [](const Call& c) {
        return hpdct_encode_scan(reinterpret_cast<const int16_t*>(c.y), reinterpret_cast<const int16_t*>(c.cb),
                                 reinterpret_cast<const int16_t*>(c.cr), c.h, c.w, static_cast<hpdct_subsampling>(c.sub),
                                 c.ri, c.flags, reinterpret_cast<uint8_t*>(c.scan), c.cap,
                                 reinterpret_cast<hpdct_scan_info*>(c.info), reinterpret_cast<uint64_t*>(c.offs),
                                 reinterpret_cast<void*>(c.ws), c.wsb, nullptr);
    };
    auto with = [&](auto f) {
        Call c = ok;
        f(c);
        return enc(c);
    };
    const char* kEnd = "workspace too small";
    expect("all good", enc(ok), 1, kEnd);
    expect("grey", with([](Call& c) { c.cb = c.cr = 0, c.h = 8, c.w = 8, c.sub = 77; }), 1, kEnd);
    expect("no offsets", with([](Call& c) { c.offs = 0; }), 1, kEnd);
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
    expect("negative width", with([](Call& c) { c.w = -32; }), 1, "multiples of");
    expect("int64 min", with([](Call& c) { c.h = std::numeric_limits<int64_t>::min(); }), 1, "multiples of");
    expect("int64 max", with([](Call& c) { c.w = std::numeric_limits<int64_t>::max() - 15; }), 1, "too large");
    expect("2^23 squared", with([](Call& c) { c.h = c.w = int64_t(1) << 23; }), 1, "too large");
    expect("subsampling 2", with([](Call& c) { c.sub = 2; }), 1, "subsampling");
    expect("subsampling -1", with([](Call& c) { c.sub = -1; }), 1, "subsampling");
    expect("interval -1", with([](Call& c) { c.ri = -1; }), 1, "restart_interval");
    expect("interval 65536", with([](Call& c) { c.ri = 65536; }), 1, "restart_interval");
    expect("interval int64 max", with([](Call& c) { c.ri = std::numeric_limits<int64_t>::max(); }), 1,
           "restart_interval");
    expect("interval 65535", with([](Call& c) { c.ri = 65535; }), 1, kEnd);
    expect("interval 1", with([](Call& c) { c.ri = 1; }), 1, kEnd);
    expect("flag 0x80", with([](Call& c) { c.flags = 0x80u; }), 2);
    expect("natural", with([](Call& c) { c.flags = HPDCT_BLOCKS_NATURAL; }), 1, kEnd);
    expect("capacity -1", with([](Call& c) { c.cap = -1; }), 1, "capacity");
    expect("capacity int64 max", with([](Call& c) { c.cap = std::numeric_limits<int64_t>::max(); }), 1, "overlap");
    expect("capacity 0", with([](Call& c) { c.cap = 0; }), 1, kEnd);
    expect("y + 8", with([](Call& c) { c.y += 8; }), 1, "aligned");
    expect("cb + 2", with([](Call& c) { c.cb += 2; }), 1, "aligned");
    expect("cr + 4", with([](Call& c) { c.cr += 4; }), 1, "aligned");
    expect("workspace + 8", with([](Call& c) { c.ws += 8; }), 1, "aligned");
    expect("offsets + 8", with([](Call& c) { c.offs += 8; }), 1, "aligned");
    expect("info + 4", with([](Call& c) { c.info += 4; }), 1, "aligned");
    expect("info + 8", with([](Call& c) { c.info += 8; }), 1, kEnd);
    expect("scan + 1", with([](Call& c) { c.scan += 1; }), 1, kEnd);
    // overlaps: y 1024 bytes, cb and cr 256, scan 4096, info 16, offsets 16 (24 with two intervals), workspace 16 (32)
    expect("cb in y", with([&](Call& c) { c.cb = Y + 1008; }), 1, "overlap");
    expect("cb after y", with([&](Call& c) { c.cb = Y + 1024; }), 1, kEnd);
    expect("cr in cb", with([&](Call& c) { c.cr = CB + 240; }), 1, "overlap");
    expect("scan in y", with([&](Call& c) { c.scan = Y + 1023, c.cap = 1; }), 1, "overlap");
    expect("scan before y", with([&](Call& c) { c.scan = Y - 4095; }), 1, "overlap");
    expect("scan up to y", with([&](Call& c) { c.scan = Y - 4096; }), 1, kEnd);
    expect("info in scan", with([&](Call& c) { c.info = SCAN + 4088; }), 1, "overlap");
    expect("info after scan", with([&](Call& c) { c.info = SCAN + 4096; }), 1, kEnd);
    expect("offsets on info", with([&](Call& c) { c.offs = INFO; }), 1, "overlap");
    expect("workspace in offsets", with([&](Call& c) { c.ri = 1, c.ws = OFFS + 16; }), 1, "overlap");
    expect("workspace after offsets", with([&](Call& c) { c.ri = 1, c.ws = OFFS + 32; }), 1, kEnd);
    expect("offsets in workspace", with([&](Call& c) { c.ri = 1, c.offs = WS + 16; }), 1, "overlap");
    expect("top of the address space", with([](Call& c) { c.scan = ~uintptr_t(0) - 100; }), 1, "wrap");
    expect("workspace 15", with([](Call& c) { c.wsb = 15; }), 1, kEnd);
    expect("workspace int64 min", with([](Call& c) { c.wsb = std::numeric_limits<int64_t>::min(); }), 1, kEnd);

    expect_eq("bound 1,1", hpdct_scan_bound(1, 1), 419);
    expect_eq("bound negative", hpdct_scan_bound(-1, 0), -1);
    expect_eq("bound overflow", hpdct_scan_bound(std::numeric_limits<int64_t>::max(), 1), -1);
    expect_eq("bound overflow 2", hpdct_scan_bound(1, std::numeric_limits<int64_t>::max()), -1);
    expect_eq("workspace 24x1016/127", hpdct_scan_workspace_bytes(24, 1016, 1, S444, 127), 48);
    expect_eq("workspace 16x32 420/1", hpdct_scan_workspace_bytes(16, 32, 3, S420, 1), 32);
    expect_eq("workspace bad components", hpdct_scan_workspace_bytes(16, 32, 2, S420, 1), -1);
    expect_eq("workspace bad size", hpdct_scan_workspace_bytes(16, 24, 3, S420, 1), -1);
    expect_eq("workspace bad interval", hpdct_scan_workspace_bytes(16, 32, 3, S420, 65536), -1);

    // the tables, each output on the heap at its exact size: a write past one is an ASan report
    for (int kind = 0; kind < 4; ++kind) {
        const int want = kind % 2 == 0 ? 12 : 162;
        std::unique_ptr<uint8_t[]> bits(new uint8_t[16]), vals(new uint8_t[want]);
        int n = -1;
        hpdct_huffman_table(kind, bits.get(), vals.get(), &n);
        int sum = 0;
        for (int i = 0; i < 16; ++i) sum += bits[i];
        expect_eq("huffman table size", n, want);
        expect_eq("huffman table bits", sum, want);
        hpdct_huffman_table(kind, nullptr, nullptr, nullptr);
    }
    int none = -1;
    hpdct_huffman_table(4, nullptr, nullptr, &none);
    expect_eq("huffman kind 4", none, 0);
    hpdct_huffman_table(-1, nullptr, nullptr, &none);
    expect_eq("huffman kind -1", none, 0);

    // the header, into a heap buffer of exactly its length
    float good[64], bad[64];
    for (int i = 0; i < 64; ++i) good[i] = bad[i] = static_cast<float>(1 + 4 * i);
    good[63] = 255.0f;
    int64_t n = -1;
    uint8_t probe[1];
    expect("header size query", hpdct_jpeg_header(probe, 0, &n, 45, 77, 3, S420, good, good, 5), 1, "too small");
    const int64_t full = n;
    expect_eq("420 header with DRI", full, 2 + 18 + 134 + 19 + (4 + 4 * 17 + 24 + 324) + 6 + 14);
    {
        std::unique_ptr<uint8_t[]> h(new uint8_t[full]);
        expect("header exact", hpdct_jpeg_header(h.get(), full, &n, 45, 77, 3, S420, good, good, 5), 0);
        expect_eq("header length", n, full);
        expect_eq("SOI", (h[0] << 8) | h[1], 0xffd8);
        expect_eq("SOS tail", h[full - 2], 63);
        expect("header one short", hpdct_jpeg_header(h.get(), full - 1, &n, 45, 77, 3, S420, good, good, 5), 1,
               "too small");
    }
    {
        expect("grey size query", hpdct_jpeg_header(probe, 0, &n, 8, 65535, 1, static_cast<hpdct_subsampling>(9),
                                                    nullptr, nullptr, 0), 1, "too small");
        expect_eq("grey header", n, 2 + 18 + 69 + 13 + (4 + 2 * 17 + 12 + 162) + 10);
        std::unique_ptr<uint8_t[]> h(new uint8_t[n]);
        expect("grey header", hpdct_jpeg_header(h.get(), n, &n, 8, 65535, 1, S444, nullptr, bad, 0), 0);
    }
    uint8_t big[1024];
    expect("header null out", hpdct_jpeg_header(nullptr, 1024, &n, 45, 77, 3, S420, good, good, 0), 1, "null");
    expect("header null length", hpdct_jpeg_header(big, 1024, nullptr, 45, 77, 3, S420, good, good, 0), 1, "null");
    expect("header 65536 rows", hpdct_jpeg_header(big, 1024, &n, 65536, 77, 3, S420, good, good, 0), 1, "65535");
    expect("header 0 columns", hpdct_jpeg_header(big, 1024, &n, 45, 0, 3, S420, good, good, 0), 1, "65535");
    expect("header 2 components", hpdct_jpeg_header(big, 1024, &n, 45, 77, 2, S420, good, good, 0), 1, "components");
    expect("header subsampling", hpdct_jpeg_header(big, 1024, &n, 45, 77, 3, static_cast<hpdct_subsampling>(2), good,
                                                   good, 0), 1, "subsampling");
    expect("header interval", hpdct_jpeg_header(big, 1024, &n, 45, 77, 3, S420, good, good, 65536), 1,
           "restart_interval");
    expect("header capacity", hpdct_jpeg_header(big, -1, &n, 45, 77, 3, S420, good, good, 0), 1, "capacity");
    const float wrong[] = {0.0f, 256.0f, 0.5f, 16.5f, -3.0f, std::nanf(""), std::numeric_limits<float>::infinity(),
                           3.0e9f};
    for (float v : wrong) {
        bad[17] = v;
        expect("header luma entry", hpdct_jpeg_header(big, 1024, &n, 45, 77, 3, S420, bad, good, 0), 3, "luma");
        expect("header chroma entry", hpdct_jpeg_header(big, 1024, &n, 45, 77, 3, S420, good, bad, 0), 3, "chroma");
    }
    // the library table when it is no JPEG table
    float quarter[64];
    for (float& v : quarter) v = 0.25f;
    expect("set table", hpdct_set_quant_table(quarter), 0);
    expect("header library table", hpdct_jpeg_header(big, 1024, &n, 45, 77, 3, S420, nullptr, nullptr, 0), 3, "luma");
    expect("reset table", hpdct_set_quant_table(nullptr), 0);
    expect("header defaults", hpdct_jpeg_header(big, 1024, &n, 45, 77, 3, S420, nullptr, nullptr, 0), 0);

    if (g_bad) {
        std::printf("asan_scan_check: %d mismatches\n", g_bad);
        return 1;
    }
    std::printf("asan_scan_check: ok\n");
    return 0;
}
