// asan_huffman_check.cpp -- the caller's Huffman tables under ASan + UBSan, CPU
// only: a stand-alone program linked with the sanitised host sources of the C ABI (g++; asan.mk's HOST) and
// the library's kernel objects, as asan_unscan_check.cpp is.  No kernel is
// launched.  DHT contents and table blobs are untrusted, so:
//   1. hpdct_huffman_prepare, hpdct_huffman_optimal and hpdct_jpeg_parse_tables
//      over mutated DHT segments: every byte of the DHT of three files (the built
//      tables, optimal tables of random counts, Annex K) set to 0, 1 and 0xFF, and
//      every truncation of each file, each in a heap buffer of exactly its size;
//      every table parse accepts must pass prepare, and the other way round;
//      the same for every DHT segment of the three optimised fixtures
//      (tests/golden/pillow_opt_*.jpg, found beside this source file);
//   2. unscan::walk_interval, the very function the decode kernel wraps, under
//      DecodeTablesWide: the built tables, the optimal tables, the fixtures'
//      tables and blobs of random bytes, over several hundred scans (random
//      bytes, the fixtures' own scans whole, cut and with flipped bits), scan,
//      blocks and blob in heap buffers of exactly their size;
//   3. the split walker likewise: unsplit::walk_segment over every segment of
//      each of those scans, speculatively from its boundary entry (the settle
//      launches' CountSink) and chained from the exits (the write launch's
//      StoreSink).
// Built and run by tests/test_huffman_tables_host.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "hpdct.h"
#include "hpdct_huffman.hpp"
#include "hpdct_unscan_split.hpp"

namespace {
int g_bad = 0;
void fail(const char* what, long a = 0, long b = 0) {
    if (++g_bad < 20) std::printf("MISMATCH %s (%ld, %ld): \"%s\"\n", what, a, b, hpdct_last_error_string());
}
uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>(g_rng >> 33);
}

hpdct_huffman_spec built_dc() {
    hpdct_huffman_spec s;
    std::memset(&s, 0, sizeof(s));
    const uint8_t vals[16] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15, 11};
    for (int i = 0; i < 16; ++i) s.bits[i] = 1, s.vals[i] = vals[i];
    s.nvals = 16;
    return s;
}
hpdct_huffman_spec built_ac() {
    hpdct_huffman_spec s;
    std::memset(&s, 0, sizeof(s));
    const uint8_t first[7] = {0x00, 0x01, 0x11, 0x02, 0xf0, 0x21, 0x03};
    int k = 0;
    for (int i = 0; i < 7; ++i) s.bits[i] = 1, s.vals[k++] = first[i];
    s.bits[15] = 249;
    for (int v = 0; v < 256; ++v) {
        bool is_first = false;
        for (uint8_t f : first) is_first = is_first || f == v;
        if (!is_first) s.vals[k++] = static_cast<uint8_t>(v);
    }
    s.nvals = k;
    return s;
}
hpdct_huffman_spec random_optimal(int nsym, bool dc) {
    uint64_t counts[256] = {};
    for (int i = 0; i < nsym; ++i) counts[dc ? rnd() % 12u : rnd() % 256u] += 1u + (rnd() % 1000u) * (rnd() % 7u == 0u);
    counts[0] += 1;  // the EOB / category 0
    hpdct_huffman_spec s;
    if (hpdct_huffman_optimal(counts, &s) != 0) fail("optimal");
    return s;
}

std::vector<uint8_t> make_file(const hpdct_huffman_spec* specs, int components, hpdct_subsampling sub) {
    uint8_t head[2048];
    int64_t n = 0;
    if (hpdct_jpeg_header_tables(head, sizeof(head), &n, 45, 70, components, sub, nullptr, nullptr, 3, specs) != 0)
        fail("header");
    std::vector<uint8_t> f(head, head + n);
    for (uint8_t b : {0x12, 0x34, 0xff, 0x00, 0x56, 0xff, 0xd0, 0x78, 0xff, 0xd9}) f.push_back(b);
    return f;
}
int parse_exact(const uint8_t* data, size_t n, hpdct_jpeg_layout* lay, hpdct_huffman_spec* specs) {
    std::unique_ptr<uint8_t[]> heap(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(heap.get(), data, n);
    return hpdct_jpeg_parse_tables(heap.get(), static_cast<int64_t>(n), lay, specs);
}

// every byte of every DHT segment of the file f set to 0, 1 and 0xFF, and every truncation of f
void mutate_dht(const std::vector<uint8_t>& f) {
    hpdct_jpeg_layout lay;
    hpdct_huffman_spec got[4];
    std::unique_ptr<uint8_t[]> blob(new uint8_t[hpdct_huffman_blob_bytes()]);
    std::vector<uint8_t> g = f;
    int segments = 0;
    for (size_t at = 2; f[at + 1] != 0xda; at += 2u + ((f[at + 2] << 8) | f[at + 3])) {
        if (f[at + 1] != 0xc4) continue;
        ++segments;
        const size_t len = 2u + ((f[at + 2] << 8) | f[at + 3]);
        for (size_t i = at; i < at + len; ++i)
            for (uint8_t v : {uint8_t(0x00), uint8_t(0x01), uint8_t(0xff)}) {
                g[i] = v;
                const int st = parse_exact(g.data(), g.size(), &lay, got);
                if (st < 0 || st > 2) fail("mutation status", static_cast<long>(i), st);
                // what parse accepts, prepare accepts
                if (st == 0 && hpdct_huffman_prepare(got, blob.get(), hpdct_huffman_blob_bytes()) != 0)
                    fail("parse accepted what prepare refuses", static_cast<long>(i), v);
                g[i] = f[i];
            }
    }
    if (segments == 0) fail("no DHT segment");
    for (size_t n = 0; n < f.size(); ++n)
        if (parse_exact(f.data(), n, &lay, got) != 1) fail("truncation", static_cast<long>(n));
}

// the three optimised fixtures, beside this source file
std::vector<std::vector<uint8_t>> fixtures() {
    std::string dir(__FILE__);
    const size_t slash = dir.rfind('/');
    dir = (slash == std::string::npos ? std::string(".") : dir.substr(0, slash)) + "/../golden/";
    std::vector<std::vector<uint8_t>> out;
    for (const char* name : {"pillow_opt_grey_rows.jpg", "pillow_opt_420_blocks3.jpg", "pillow_opt_444_norestart.jpg"}) {
        std::vector<uint8_t> d;
        if (std::FILE* fp = std::fopen((dir + name).c_str(), "rb")) {
            uint8_t buf[4096];
            for (size_t n; (n = std::fread(buf, 1, sizeof(buf), fp)) > 0;) d.insert(d.end(), buf, buf + n);
            std::fclose(fp);
        }
        if (d.size() < 100u) fail(name);
        out.push_back(d);
    }
    return out;
}

void tables_and_files() {
    for (const std::vector<uint8_t>& f : fixtures())
        if (f.size() >= 100u) mutate_dht(f);
    hpdct_huffman_spec sets[3][4];
    sets[0][0] = sets[0][2] = built_dc(), sets[0][1] = sets[0][3] = built_ac();
    sets[1][0] = random_optimal(40, true), sets[1][1] = random_optimal(3000, false);
    sets[1][2] = random_optimal(5, true), sets[1][3] = random_optimal(60, false);
    for (int k = 0; k < 4; ++k) sets[2][k] = hpdct::huff::annex_k(k);
    std::unique_ptr<uint8_t[]> blob(new uint8_t[hpdct_huffman_blob_bytes()]);
    for (int set = 0; set < 3; ++set) {
        if (hpdct_huffman_prepare(sets[set], blob.get(), hpdct_huffman_blob_bytes()) != 0) fail("prepare", set);
        if (hpdct_huffman_prepare(sets[set], blob.get(), hpdct_huffman_blob_bytes() - 1) != 1) fail("capacity", set);
        for (int variant = 0; variant < 2; ++variant) {
            const int comps = variant == 0 ? 3 : 1;
            const std::vector<uint8_t> f = make_file(sets[set], comps, HPDCT_SUBSAMPLING_420);
            hpdct_jpeg_layout lay;
            hpdct_huffman_spec got[4];
            if (parse_exact(f.data(), f.size(), &lay, got) != 0) fail("parse whole", set, variant);
            for (int k = 0; k < 2 * (comps == 3 ? 2 : 1); ++k)
                if (!hpdct::huff::same_table(got[k], sets[set][k])) fail("round trip", set, k);
            if (comps == 1 && (got[2].nvals != 0 || got[3].nvals != 0)) fail("grey chroma tables", set);
            mutate_dht(f);
        }
    }
    // prepare on random specs: any verdict, no report; an accepted spec has a Kraft sum within 1
    for (int t = 0; t < 2000; ++t) {
        hpdct_huffman_spec s[4];
        for (int k = 0; k < 4; ++k) {
            s[k] = sets[t % 3][k];
            for (int m = rnd() % 3u; m > 0; --m) reinterpret_cast<uint8_t*>(&s[k])[rnd() % sizeof(s[k])] = rnd() & 0xffu;
        }
        hpdct_huffman_prepare(s, blob.get(), hpdct_huffman_blob_bytes());
    }
    hpdct_huffman_spec out;
    uint64_t counts[256];
    for (int t = 0; t < 300; ++t) {
        for (int i = 0; i < 256; ++i) counts[i] = rnd() % 4u == 0u ? 0u : (uint64_t(rnd()) << (rnd() % 7u)) >> (rnd() % 31u);
        if (hpdct_huffman_optimal(counts, &out) != 0) fail("optimal status");
        if (hpdct::huff::defect(out, 1) != nullptr) fail("optimal gives a table prepare refuses", t);
    }
    // Fibonacci counts up to 2^38 and beyond: a tree deeper than 32
    uint64_t a = 1, b = 1;
    std::memset(counts, 0, sizeof(counts));
    for (int i = 0; i < 70; ++i) {
        counts[i] = a;
        const uint64_t c = a + b;
        a = b, b = c;
    }
    if (hpdct_huffman_optimal(counts, &out) != 0 || hpdct::huff::defect(out, 1) != nullptr || out.nvals != 70)
        fail("optimal, deep tree", out.nvals);
}

// scans through walk_interval under `blob`: exact-size heap buffers, any status
void walk_all(const hpdct::unscan::HuffBlob& src, const std::vector<std::vector<uint8_t>>& scans, int& walked) {
    using namespace hpdct;
    std::unique_ptr<unscan::HuffBlob> blob(new unscan::HuffBlob(src));
    uint8_t order[64];
    for (int n = 0; n < 64; ++n) order[n] = zigzag::kOrder[n];
    for (size_t i = 0; i < scans.size(); ++i) {
        const std::vector<uint8_t>& sc = scans[i];
        const uint32_t variant = static_cast<uint32_t>(i % 3u);
        scan::ScanGrid g;
        g.bpm = variant == 0u ? 1u : variant == 1u ? 3u : 6u;
        g.mcus_x = 3u, g.nmcu = 6u, g.per_interval = 6u, g.intervals = 1u;
        const size_t ny = 64u * g.nmcu * (g.bpm == 6u ? 4u : 1u), nc = g.bpm == 1u ? 0u : 64u * g.nmcu;
        std::unique_ptr<int16_t[]> y(new int16_t[ny]), cb(new int16_t[nc ? nc : 1]), cr(new int16_t[nc ? nc : 1]);
        const uint32_t shift = static_cast<uint32_t>(i % 8u);
        std::unique_ptr<uint8_t[]> heap(new uint8_t[shift + sc.size() + 1u]);
        std::memcpy(heap.get() + shift + 1u, sc.data(), sc.size());  // ends where the buffer ends
        alignas(16) uint32_t row[32];
        const uint8_t* base = heap.get() + shift + 1u;
        const uint64_t st = i % 2u ? unscan::walk_interval<true>(base, 0, sc.size(), 0u, 0, g, &blob->dec, order, row,
                                                                 y.get(), nc ? cb.get() : nullptr, nc ? cr.get() : nullptr)
                                   : unscan::walk_interval<false>(base, 0, sc.size(), 0u, 0, g, &blob->dec, order, row,
                                                                  y.get(), nc ? cb.get() : nullptr, nc ? cr.get() : nullptr);
        if ((st & 255u) > 8u) fail("status code", static_cast<long>(st));
        // the split walker over the same bytes: every segment from its boundary entry, then the chain of exits
        const uint64_t n = sc.size(), nblk = static_cast<uint64_t>(g.nmcu) * g.bpm;
        const uint64_t nseg = (n + unsplit::kSegBytes - 1u) / unsplit::kSegBytes;
        unsplit::SegState entry{0u, 0u, 0u};
        unsplit::StoreSink<false> store;
        store.y = y.get(), store.cb = nc ? cb.get() : nullptr, store.cr = nc ? cr.get() : nullptr, store.g = g;
        store.order = order, store.block = 0u, store.nblk = nblk, store.m = 0u, store.kk = 0u;
        store.pred[0] = store.pred[1] = store.pred[2] = 0;
        store.seek();
        for (uint64_t q = 0; q < nseg; ++q) {
            const uint64_t end = (q + 1u) * unsplit::kSegBytes < n ? (q + 1u) * unsplit::kSegBytes : n;
            unsplit::CountSink count;
            const unsplit::SegState spec = unsplit::boundary_entry(base, 0, n, q);
            unsplit::walk_segment(base, 0, n, end, spec, g.bpm, &blob->dec, count);
            if (q == 0u) entry = spec;
            const unsplit::SegState ex = unsplit::walk_segment(base, 0, n, end, entry, g.bpm, &blob->dec, store);
            if (ex.pos > n) fail("exit past the end", static_cast<long>(ex.pos));
            entry = unsplit::entry_of(ex);
        }
        ++walked;
    }
}

void walker() {
    using namespace hpdct;
    std::vector<std::vector<uint8_t>> scans;
    for (int t = 0; t < 300; ++t) {
        std::vector<uint8_t> s(rnd() % 400u);
        const uint32_t kind = rnd() % 4u;
        for (uint8_t& b : s) b = kind == 0u ? rnd() & 0xffu : kind == 1u ? (rnd() % 5u ? 0x00 : rnd() & 0xffu)
                                 : kind == 2u ? (rnd() % 9u ? 0xff : 0x00) : (rnd() & rnd() & 0xffu);
        scans.push_back(s);
    }
    int walked = 0;
    unscan::HuffBlob blob;
    hpdct_huffman_spec specs[4];
    specs[0] = specs[2] = built_dc(), specs[1] = specs[3] = built_ac();
    huff::fill_blob(specs, blob);
    walk_all(blob, scans, walked);
    specs[0] = random_optimal(40, true), specs[1] = random_optimal(3000, false);
    specs[2] = random_optimal(5, true), specs[3] = random_optimal(60, false);
    huff::fill_blob(specs, blob);
    walk_all(blob, scans, walked);
    for (const std::vector<uint8_t>& f : fixtures()) {  // the fixtures' tables, over all the scans and their own
        hpdct_jpeg_layout lay;
        if (f.size() < 100u || hpdct_jpeg_parse_tables(f.data(), static_cast<int64_t>(f.size()), &lay, specs) != 0) {
            fail("fixture");
            continue;
        }
        const std::vector<uint8_t> own(f.begin() + lay.scan_offset, f.begin() + lay.scan_offset + lay.scan_bytes);
        std::vector<std::vector<uint8_t>> mine = scans;
        mine.push_back(own);
        for (int t = 0; t < 60; ++t) {
            std::vector<uint8_t> d(own.begin(), own.begin() + (t % 3 ? own.size() : rnd() % own.size()));
            if (!d.empty()) d[rnd() % d.size()] ^= static_cast<uint8_t>(1u << (rnd() % 8u));
            mine.push_back(d);
        }
        huff::fill_blob(specs, blob);
        walk_all(blob, mine, walked);
    }
    std::memset(specs, 0, sizeof(specs));  // four empty tables: every symbol is CODE or the fetch's error
    huff::fill_blob(specs, blob);
    walk_all(blob, scans, walked);
    for (int t = 0; t < 6; ++t) {  // blobs prepare never wrote
        uint8_t* p = reinterpret_cast<uint8_t*>(&blob);
        for (size_t i = 0; i < sizeof(blob); ++i) p[i] = t == 0 ? 0xff : t == 1 ? 0x80 : rnd() & 0xffu;
        walk_all(blob, scans, walked);
    }
    std::printf("asan_huffman_check: %d walks\n", walked);
    if (walked < 2000) fail("too few walks", walked);
}
}  // namespace

int main() {
    tables_and_files();
    walker();
    if (g_bad) {
        std::printf("asan_huffman_check: %d mismatches\n", g_bad);
        return 1;
    }
    std::printf("asan_huffman_check: ok\n");
    return 0;
}
