// hpdct_api_jpeg.cpp -- the extern "C" boundary of the entropy codec (include/hpdct.h): hpdct_*scan*,
// hpdct_huffman_*, hpdct_jpeg_* and hpdct_decode_*.  Validation and dispatch as in hpdct_api.cpp, whose helpers it
// shares through hpdct_api_internal.hpp.  Each pair of entry points (Annex K, the caller's tables) is one body:
// d_tables or specs NULL means Annex K all the way down to the launch functions (hpdct_scan.hpp, hpdct_unscan.hpp,
// hpdct_unscan_split.hpp), which pick the kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <limits>
#include <string>
#include <vector>

#include "hpdct.h"
#include "hpdct_api_internal.hpp"
#include "hpdct_huffman.hpp"
#include "hpdct_kernels.h"
#include "hpdct_scan.hpp"
#include "hpdct_unscan.hpp"
#include "hpdct_unscan_split.hpp"
#include "hpdct_zigzag.h"

using namespace hpdct::api;
using hpdct::TileGrid;

namespace {

// The scan's geometry from the padded frame's size: components 1 (grey; sub
// not read) or 3, restart_interval 0..65535.
hpdct_status scan_geometry(int64_t height, int64_t width, int components, hpdct_subsampling sub,
                           int64_t restart_interval, hpdct::scan::ScanGrid& g, uint64_t blocks[3]) {
    if (components != 1 && components != 3) return fail(HPDCT_ERROR_INVALID_VALUE, "components must be 1 or 3");
    if (components == 3)
        if (hpdct_status st = check_subsampling(sub)) return st;
    const bool s420 = components == 3 && sub == HPDCT_SUBSAMPLING_420;
    const int64_t side = s420 ? 16 : 8;
    if (height <= 0 || width <= 0 || (height % side) != 0 || (width % side) != 0)
        return fail(HPDCT_ERROR_INVALID_VALUE, "height and width must be positive multiples of " +
                                                   std::to_string(side) + " (the padded frame; got " +
                                                   std::to_string(height) + "x" + std::to_string(width) + ")");
    TileGrid yg;
    if (hpdct_status st = make_grid(height, width, yg)) return st;
    if (restart_interval < 0 || restart_interval > 65535)
        return fail(HPDCT_ERROR_INVALID_VALUE, "restart_interval must be 0..65535 (got " +
                                                   std::to_string(restart_interval) + ")");
    units_of(yg, s420, g.nmcu, g.mcus_x);
    g.per_interval = restart_interval == 0 ? g.nmcu : static_cast<uint32_t>(restart_interval);
    g.intervals = g.nmcu / g.per_interval + (g.nmcu % g.per_interval != 0u);
    g.bpm = components == 1 ? 1u : s420 ? 6u : 3u;
    blocks[0] = yg.ntiles;
    blocks[1] = blocks[2] = components == 1 ? 0u : g.nmcu;
    return HPDCT_SUCCESS;
}

// a table for a JPEG file: every entry an integer in 1..255
hpdct_status header_table(const float* q, const char* name, uint8_t out_zigzag[64]) {
    for (int n = 0; n < 64; ++n) {
        const float v = q[hpdct::zigzag::kOrder[n]];
        if (!byte_integer(v))
            return fail(HPDCT_ERROR_RANGE, std::string(name) + " quant table: a baseline JPEG file takes integers "
                                                               "in 1..255 only");
        out_zigzag[n] = static_cast<uint8_t>(v);
    }
    return HPDCT_SUCCESS;
}

// hpdct_scan_bound and hpdct_scan_bound_tables: per_block is the worst case of a block under the tables in question
int64_t scan_bound(int64_t blocks, int64_t intervals, int64_t per_block) {
    constexpr int64_t kMax = std::numeric_limits<int64_t>::max();
    constexpr int64_t kPerInterval = hpdct::scan::kBoundPerInterval;
    if (blocks < 0 || intervals < 0 || blocks > kMax / (2 * per_block) || intervals > kMax / (2 * kPerInterval))
        return -1;
    return per_block * blocks + kPerInterval * intervals;
}

// the caller's table blob: 16-byte aligned, disjoint from what the call writes
hpdct_status check_tables(const void* d_tables, const Span* written, int n) {
    if (!aligned(d_tables, 16)) return fail(HPDCT_ERROR_INVALID_VALUE, "d_tables must be 16-byte aligned");
    for (int i = 0; i < n; ++i) {
        const Span pair[2] = {written[i], {d_tables, sizeof(hpdct::unscan::HuffBlob), "tables"}};
        if (hpdct_status st = check_disjoint(pair, 2, kWrapMsg, nullptr)) return st;
    }
    return HPDCT_SUCCESS;
}

// hpdct_encode_scan and hpdct_encode_scan_tables: d_tables nullptr is Annex K
hpdct_status encode_scan_any(const int16_t* d_y, const int16_t* d_cb, const int16_t* d_cr, int64_t height,
                             int64_t width, hpdct_subsampling sub, int64_t restart_interval, unsigned flags,
                             uint8_t* d_scan, int64_t capacity, hpdct_scan_info* d_info,
                             uint64_t* d_interval_offsets, void* d_workspace, int64_t workspace_bytes,
                             const void* d_tables, void* stream) {
    if ((d_cb == nullptr) != (d_cr == nullptr))
        return fail(HPDCT_ERROR_INVALID_VALUE, "null block pointer: d_cb and d_cr are both given or both NULL");
    const int components = d_cb ? 3 : 1;
    hpdct::scan::ScanGrid g;
    uint64_t blocks[3];
    if (hpdct_status st = scan_geometry(height, width, components, sub, restart_interval, g, blocks)) return st;
    if (!d_y || !d_scan || !d_info || !d_workspace)
        return fail(HPDCT_ERROR_INVALID_VALUE, "null block, scan, info or workspace pointer");
    if (flags & ~HPDCT_BLOCKS_NATURAL) return fail(HPDCT_ERROR_UNSUPPORTED, "unknown block flag bits");
    if (capacity < 0) return fail(HPDCT_ERROR_INVALID_VALUE, "negative capacity");
    if (!aligned(d_y, 16) || !aligned(d_cb, 16) || !aligned(d_cr, 16) || !aligned(d_workspace, 16) ||
        !aligned(d_interval_offsets, 16) || !aligned(d_info, 8))
        return fail(HPDCT_ERROR_INVALID_VALUE,
                    "block, workspace and offsets pointers must be 16-byte aligned, d_info 8-byte aligned");
    const int64_t need = hpdct::scan::workspace_bytes(g.intervals);
    // only the part of the workspace the call uses counts; the refusal names the two buffers
    const Span spans[7] = {
        {d_y, static_cast<size_t>(blocks[0]) * 128u, "y"},
        {d_cb, static_cast<size_t>(blocks[1]) * 128u, "cb"},
        {d_cr, static_cast<size_t>(blocks[2]) * 128u, "cr"},
        {d_scan, static_cast<size_t>(capacity), "scan"},
        {d_info, sizeof(hpdct_scan_info), "info"},
        {d_interval_offsets, d_interval_offsets ? (static_cast<size_t>(g.intervals) + 1u) * sizeof(uint64_t) : 0u,
         "offsets"},
        {d_workspace, static_cast<size_t>(need), "workspace"}};
    if (hpdct_status st = check_disjoint(spans, 7, kWrapMsg, nullptr)) return st;
    if (workspace_bytes < need)
        return fail(HPDCT_ERROR_INVALID_VALUE, "workspace too small: " + std::to_string(need) + " bytes needed (got " +
                                                   std::to_string(workspace_bytes) + ")");
    if (d_tables)  // against what the call writes: scan, info, offsets, workspace
        if (hpdct_status st = check_tables(d_tables, spans + 3, 4)) return st;
    return device_status(hpdct::launch_scan(d_y, d_cb, d_cr, g, (flags & HPDCT_BLOCKS_NATURAL) != 0, d_scan,
                                            static_cast<uint64_t>(capacity), d_info, d_interval_offsets, d_workspace,
                                            static_cast<const hpdct::unscan::HuffBlob*>(d_tables),
                                            static_cast<hipStream_t>(stream)),
                         "entropy coder kernel launch");
}

// What hpdct_decode_scan and hpdct_decode_scan_split check, alike: everything but the launch.  split: the info
// struct and the workspace are the split call's.  d_tables: the caller's blob or nullptr, judged last.
hpdct_status check_decode(const uint8_t* d_scan, int64_t bytes, const uint64_t* d_interval_offsets, int16_t* d_y,
                          int16_t* d_cb, int16_t* d_cr, int64_t height, int64_t width, hpdct_subsampling sub,
                          int64_t restart_interval, unsigned flags, const void* d_info,
                          const uint64_t* d_interval_status, const void* d_workspace, int64_t workspace_bytes,
                          bool split, const void* d_tables, hpdct::scan::ScanGrid& g) {
    if ((d_cb == nullptr) != (d_cr == nullptr))
        return fail(HPDCT_ERROR_INVALID_VALUE, "null block pointer: d_cb and d_cr are both given or both NULL");
    const int components = d_cb ? 3 : 1;
    uint64_t blocks[3];
    if (hpdct_status st = scan_geometry(height, width, components, sub, restart_interval, g, blocks)) return st;
    if (!d_scan || !d_y || !d_info || !d_workspace)
        return fail(HPDCT_ERROR_INVALID_VALUE, "null scan, block, info or workspace pointer");
    if (flags & ~HPDCT_BLOCKS_NATURAL) return fail(HPDCT_ERROR_UNSUPPORTED, "unknown block flag bits");
    if (bytes < 0) return fail(HPDCT_ERROR_INVALID_VALUE, "negative scan length");
    if (!aligned(d_y, 16) || !aligned(d_cb, 16) || !aligned(d_cr, 16) || !aligned(d_workspace, 16) ||
        !aligned(d_interval_offsets, 16) || !aligned(d_interval_status, 16) || !aligned(d_info, 8))
        return fail(HPDCT_ERROR_INVALID_VALUE,
                    "block, workspace, offsets and status pointers must be 16-byte aligned, d_info 8-byte aligned");
    const int64_t need = split ? static_cast<int64_t>(hpdct::unsplit::layout(g.intervals, static_cast<uint64_t>(bytes)).bytes)
                               : hpdct::unscan::workspace_bytes(g.intervals, static_cast<uint64_t>(bytes));
    // only the part of the workspace the call uses counts; the refusal names the two buffers
    const Span spans[8] = {
        {d_y, static_cast<size_t>(blocks[0]) * 128u, "y"},
        {d_cb, static_cast<size_t>(blocks[1]) * 128u, "cb"},
        {d_cr, static_cast<size_t>(blocks[2]) * 128u, "cr"},
        {d_scan, static_cast<size_t>(bytes), "scan"},
        {d_info, split ? sizeof(hpdct_decode_split_info) : sizeof(hpdct_decode_info), "info"},
        {d_interval_offsets, d_interval_offsets ? (static_cast<size_t>(g.intervals) + 1u) * sizeof(uint64_t) : 0u,
         "offsets"},
        {d_interval_status, d_interval_status ? static_cast<size_t>(g.intervals) * sizeof(uint64_t) : 0u, "status"},
        {d_workspace, static_cast<size_t>(need), "workspace"}};
    if (hpdct_status st = check_disjoint(spans, 8, kWrapMsg, nullptr)) return st;
    if (workspace_bytes < need)
        return fail(HPDCT_ERROR_INVALID_VALUE, "workspace too small: " + std::to_string(need) + " bytes needed (got " +
                                                   std::to_string(workspace_bytes) + ")");
    if (!d_tables) return HPDCT_SUCCESS;
    // against what the call writes, in this order: y, cb, cr, info, status, workspace
    const Span written[6] = {spans[0], spans[1], spans[2], spans[4], spans[6], spans[7]};
    return check_tables(d_tables, written, 6);
}

// The four decode entry points: split (hpdct_decode_scan_split*: d_info a hpdct_decode_split_info, and
// split_min_bytes is read) or not; d_tables nullptr is Annex K.
hpdct_status decode_any(const uint8_t* d_scan, int64_t bytes, const uint64_t* d_interval_offsets, int16_t* d_y,
                        int16_t* d_cb, int16_t* d_cr, int64_t height, int64_t width, hpdct_subsampling sub,
                        int64_t restart_interval, unsigned flags, bool split, int64_t split_min_bytes, void* d_info,
                        uint64_t* d_interval_status, void* d_workspace, int64_t workspace_bytes, const void* d_tables,
                        void* stream) {
    if (split && split_min_bytes < 0) return fail(HPDCT_ERROR_INVALID_VALUE, "negative split_min_bytes");
    hpdct::scan::ScanGrid g;
    if (hpdct_status st = check_decode(d_scan, bytes, d_interval_offsets, d_y, d_cb, d_cr, height, width, sub,
                                       restart_interval, flags, d_info, d_interval_status, d_workspace,
                                       workspace_bytes, split, d_tables, g))
        return st;
    const bool natural = (flags & HPDCT_BLOCKS_NATURAL) != 0;
    const auto* blob = static_cast<const hpdct::unscan::HuffBlob*>(d_tables);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!split)
        return device_status(hpdct::launch_unscan(d_scan, static_cast<uint64_t>(bytes), d_interval_offsets, d_y, d_cb,
                                                  d_cr, g, natural, static_cast<hpdct_decode_info*>(d_info),
                                                  d_interval_status, d_workspace, blob, s),
                             "entropy decoder kernel launch");
    const uint64_t split_min = split_min_bytes == 0 ? hpdct::policy::kUnsplitMinBytes : static_cast<uint64_t>(split_min_bytes);
    return device_status(hpdct::launch_unscan_split(d_scan, static_cast<uint64_t>(bytes), d_interval_offsets, d_y, d_cb,
                                                    d_cr, g, natural, split_min,
                                                    static_cast<hpdct_decode_split_info*>(d_info), d_interval_status,
                                                    d_workspace, blob, s),
                         "split entropy decoder kernel launch");
}

// hpdct_jpeg_parse (specs nullptr: the selected tables must be Annex K's) and hpdct_jpeg_parse_tables (specs
// given: they are judged as hpdct_huffman_prepare judges them, and returned)
hpdct_status jpeg_parse_any(const uint8_t* f, int64_t n, hpdct_jpeg_layout* out, hpdct_huffman_spec* specs) {
    if (!f || !out) return fail(HPDCT_ERROR_INVALID_VALUE, "null file or layout pointer");
    if (n < 0) return fail(HPDCT_ERROR_INVALID_VALUE, "negative file length");
    auto bad = [](const std::string& why) { return fail(HPDCT_ERROR_INVALID_VALUE, "not a whole JPEG file: " + why); };
    auto no = [](const std::string& why) { return fail(HPDCT_ERROR_UNSUPPORTED, "not a file hpdct_decode_scan decodes: " + why); };
    if (n < 2 || f[0] != 0xffu || f[1] != 0xd8u) return bad("no SOI");
    struct Huff {
        bool have = false;
        uint8_t bits[16];
        int nvals = 0;
        uint8_t vals[256];
    };
    std::vector<Huff> ht(8);  // [class * 4 + destination]
    float qt[4][64];
    bool have_q[4] = {false, false, false, false};
    bool have_sof = false;
    int nc = 0, cid[3] = {0, 0, 0}, chv[3] = {0, 0, 0}, ctq[3] = {0, 0, 0};
    int64_t height = 0, width = 0, ri = 0, p = 2;
    for (;;) {
        if (p + 2 > n) return bad("it ends before SOS");
        if (f[p] != 0xffu) return bad("a marker is expected at byte " + std::to_string(p));
        const unsigned m = f[p + 1];
        if (m == 0xffu) {  // a fill byte
            ++p;
            continue;
        }
        if (m == 0x00u || m == 0x01u || (m >= 0xd0u && m <= 0xd9u)) return bad("marker FF " + std::to_string(m) + " before SOS");
        if (p + 4 > n) return bad("it ends inside a segment header");
        const int64_t len = (f[p + 2] << 8) | f[p + 3];
        if (len < 2 || p + 2 + len > n) return bad("a segment runs past the end");
        const uint8_t* seg = f + p + 4;
        const int64_t sl = len - 2;
        p += 2 + len;
        if (m == 0xdbu) {  // DQT: one table or several
            for (int64_t q = 0; q < sl; q += 65) {
                const unsigned pq = seg[q] >> 4, tq = seg[q] & 15u;
                if (pq == 1u) return no("a 16-bit DQT");
                if (pq != 0u || tq > 3u || q + 65 > sl) return bad("a malformed DQT");
                for (int i = 0; i < 64; ++i) {
                    if (seg[q + 1 + i] == 0u) return bad("a zero DQT entry");
                    qt[tq][hpdct::zigzag::kOrder[i]] = static_cast<float>(seg[q + 1 + i]);
                }
                have_q[tq] = true;
            }
        } else if (m == 0xc4u) {  // DHT: one table or several
            for (int64_t q = 0; q < sl;) {
                const unsigned tc = seg[q] >> 4, th = seg[q] & 15u;
                if (tc > 1u || th > 3u || q + 17 > sl) return bad("a malformed DHT");
                Huff& h = ht[tc * 4u + th];
                int count = 0;
                for (int i = 0; i < 16; ++i) count += (h.bits[i] = seg[q + 1 + i]);
                if (count > 256 || q + 17 + count > sl) {
                    h.have = false;
                    return bad("a malformed DHT");
                }
                memcpy(h.vals, seg + q + 17, static_cast<size_t>(count));
                h.nvals = count, h.have = true;
                q += 17 + count;
            }
        } else if (m == 0xc0u) {  // SOF0
            if (have_sof) return bad("two frame headers");
            if (sl < 6) return bad("a malformed SOF0");
            if (seg[0] != 8u) return no("samples of " + std::to_string(seg[0]) + " bits (8 only)");
            height = (seg[1] << 8) | seg[2], width = (seg[3] << 8) | seg[4], nc = seg[5];
            if (nc != 1 && nc != 3) return no(std::to_string(nc) + " components (1 or 3 only)");
            if (sl != 6 + 3 * nc || height == 0 || width == 0) return bad("a malformed SOF0");
            for (int c = 0; c < nc; ++c) {
                cid[c] = seg[6 + 3 * c], chv[c] = seg[7 + 3 * c], ctq[c] = seg[8 + 3 * c];
                if (ctq[c] > 3) return bad("a malformed SOF0");
            }
            have_sof = true;
        } else if (m >= 0xc1u && m <= 0xcfu && m != 0xc8u) {  // the other frame types, DAC
            return no(m == 0xccu ? std::string("arithmetic coding") : "a frame that is not SOF0 (baseline sequential)");
        } else if (m == 0xddu) {  // DRI
            if (sl != 2) return bad("a malformed DRI");
            ri = (seg[0] << 8) | seg[1];
        } else if (m == 0xdau) {  // SOS
            if (!have_sof) return bad("SOS before SOF0");
            if (sl < 1) return bad("a malformed SOS");
            const int ns = seg[0];
            if (ns < 1 || ns > 4 || sl != 4 + 2 * ns) return bad("a malformed SOS");
            if (ns != nc) return no("more than one scan (a scan of " + std::to_string(ns) + " of " + std::to_string(nc) +
                                    " components)");
            if (seg[1 + 2 * ns] != 0u || seg[2 + 2 * ns] != 63u || seg[3 + 2 * ns] != 0u)
                return no("Ss / Se / Ah / Al other than 0 / 63 / 0 / 0");
            if (nc == 1 ? chv[0] != 0x11
                        : !((chv[0] == 0x11 || chv[0] == 0x22) && chv[1] == 0x11 && chv[2] == 0x11))
                return no("sampling other than 1x1 (grey), 1x1 / 1x1 / 1x1 or 2x2 / 1x1 / 1x1");
            for (int c = 0; c < nc; ++c) {
                if (seg[1 + 2 * c] != cid[c]) return bad("the scan's components are not the frame's");
                if (!have_q[ctq[c]]) return bad("a component's quant table is missing");
                const unsigned td = seg[2 + 2 * c] >> 4, ta = seg[2 + 2 * c] & 15u;
                if (td > 3u || ta > 3u) return bad("a malformed SOS");
                for (int ac = 0; ac < 2; ++ac) {
                    const Huff& h = ht[static_cast<unsigned>(ac) * 4u + (ac ? ta : td)];
                    if (!h.have) return bad("a component's Huffman table is missing");
                    const int kind = (c == 0 ? 0 : 2) + ac;
                    hpdct_huffman_spec t;
                    memset(&t, 0, sizeof(t));
                    memcpy(t.bits, h.bits, 16);
                    memcpy(t.vals, h.vals, static_cast<size_t>(h.nvals));
                    t.nvals = h.nvals;
                    if (specs) {
                        if (const char* why = hpdct::huff::defect(t, kind))
                            return fail(HPDCT_ERROR_INVALID_VALUE, std::string("component ") + std::to_string(c) +
                                                                       "'s " + hpdct::huff::kind_name(kind) +
                                                                       " Huffman table: " + why);
                        if (c < 2)
                            specs[kind] = t;
                        else if (!hpdct::huff::same_table(specs[kind], t))
                            return no("Cb and Cr on different Huffman tables");
                        continue;
                    }
                    if (!hpdct::huff::same_table(t, hpdct::scan::spec_of(kind)))
                        return no(std::string("component ") + std::to_string(c) + "'s " + (ac ? "AC" : "DC") +
                                  " Huffman table differs from the Annex K " +
                                  (c == 0 ? "luminance" : "chrominance") + " table");
                }
            }
            if (nc == 3 && memcmp(qt[ctq[1]], qt[ctq[2]], sizeof(qt[0])) != 0)
                return no("Cb and Cr on different quant tables");
            break;
        } else if ((m >= 0xe0u && m <= 0xefu) || m == 0xfeu) {
            // APPn, COM: skipped
        } else {
            return no("a segment FF " + std::to_string(m));
        }
    }
    // the scan: to the first marker that is neither FF 00 nor RSTn
    int64_t q = p;
    for (;; ++q) {
        if (q + 2 > n) return bad("no EOI after the scan");
        if (f[q] != 0xffu) continue;
        const unsigned b = f[q + 1];
        if (b == 0x00u || (b >= 0xd0u && b <= 0xd7u)) {
            ++q;
            continue;
        }
        if (b == 0xd9u) break;
        if (b == 0xffu) continue;
        if (b == 0xdau || b == 0xc4u || b == 0xdbu || b == 0xddu) return no("more than one scan");
        return bad("marker FF " + std::to_string(b) + " inside the scan");
    }
    out->height = height, out->width = width, out->components = nc;
    out->sub = nc == 3 && chv[0] == 0x22 ? HPDCT_SUBSAMPLING_420 : HPDCT_SUBSAMPLING_444;
    out->restart_interval = ri, out->scan_offset = p, out->scan_bytes = q - p;
    memcpy(out->q_luma, qt[ctq[0]], sizeof(out->q_luma));
    if (nc == 3) memcpy(out->q_chroma, qt[ctq[1]], sizeof(out->q_chroma));
    return HPDCT_SUCCESS;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------
// Entropy coding: hpdct_encode_scan, hpdct_jpeg_header (hpdct_scan.hpp)
// ---------------------------------------------------------------------------
int64_t hpdct_scan_bound(int64_t blocks, int64_t intervals) {
    return scan_bound(blocks, intervals, hpdct::scan::kBoundPerBlock);
}
int64_t hpdct_scan_bound_tables(int64_t blocks, int64_t intervals) {
    return scan_bound(blocks, intervals, hpdct::scan::kBoundPerBlockT);
}

int64_t hpdct_scan_workspace_bytes(int64_t height, int64_t width, int components, hpdct_subsampling sub,
                                   int64_t restart_interval) {
    hpdct::scan::ScanGrid g;
    uint64_t blocks[3];
    if (scan_geometry(height, width, components, sub, restart_interval, g, blocks) != HPDCT_SUCCESS) return -1;
    return hpdct::scan::workspace_bytes(g.intervals);
}

hpdct_status hpdct_encode_scan(const int16_t* d_y, const int16_t* d_cb, const int16_t* d_cr, int64_t height,
                               int64_t width, hpdct_subsampling sub, int64_t restart_interval, unsigned flags,
                               uint8_t* d_scan, int64_t capacity, hpdct_scan_info* d_info,
                               uint64_t* d_interval_offsets, void* d_workspace, int64_t workspace_bytes,
                               void* stream) {
    return encode_scan_any(d_y, d_cb, d_cr, height, width, sub, restart_interval, flags, d_scan, capacity, d_info,
                           d_interval_offsets, d_workspace, workspace_bytes, nullptr, stream);
}

hpdct_status hpdct_encode_scan_tables(const int16_t* d_y, const int16_t* d_cb, const int16_t* d_cr, int64_t height,
                                      int64_t width, hpdct_subsampling sub, int64_t restart_interval, unsigned flags,
                                      uint8_t* d_scan, int64_t capacity, hpdct_scan_info* d_info,
                                      uint64_t* d_interval_offsets, void* d_workspace, int64_t workspace_bytes,
                                      const void* d_tables, void* stream) {
    return encode_scan_any(d_y, d_cb, d_cr, height, width, sub, restart_interval, flags, d_scan, capacity, d_info,
                           d_interval_offsets, d_workspace, workspace_bytes, d_tables, stream);
}

hpdct_status hpdct_scan_histogram(const int16_t* d_y, const int16_t* d_cb, const int16_t* d_cr, int64_t height,
                                  int64_t width, hpdct_subsampling sub, int64_t restart_interval, unsigned flags,
                                  uint64_t* d_counts, void* stream) {
    if ((d_cb == nullptr) != (d_cr == nullptr))
        return fail(HPDCT_ERROR_INVALID_VALUE, "null block pointer: d_cb and d_cr are both given or both NULL");
    const int components = d_cb ? 3 : 1;
    hpdct::scan::ScanGrid g;
    uint64_t blocks[3];
    if (hpdct_status st = scan_geometry(height, width, components, sub, restart_interval, g, blocks)) return st;
    if (!d_y || !d_counts) return fail(HPDCT_ERROR_INVALID_VALUE, "null block or counts pointer");
    if (flags & ~HPDCT_BLOCKS_NATURAL) return fail(HPDCT_ERROR_UNSUPPORTED, "unknown block flag bits");
    if (!aligned(d_y, 16) || !aligned(d_cb, 16) || !aligned(d_cr, 16) || !aligned(d_counts, 16))
        return fail(HPDCT_ERROR_INVALID_VALUE, "block and counts pointers must be 16-byte aligned");
    const Span spans[4] = {{d_y, static_cast<size_t>(blocks[0]) * 128u, "y"},
                           {d_cb, static_cast<size_t>(blocks[1]) * 128u, "cb"},
                           {d_cr, static_cast<size_t>(blocks[2]) * 128u, "cr"},
                           {d_counts, 4u * 256u * sizeof(uint64_t), "counts"}};
    if (hpdct_status st = check_disjoint(spans, 4, kWrapMsg, nullptr)) return st;
    return device_status(hpdct::launch_scan_hist(d_y, d_cb, d_cr, g, (flags & HPDCT_BLOCKS_NATURAL) != 0, d_counts,
                                                 static_cast<hipStream_t>(stream)),
                         "scan histogram kernel launch");
}

int64_t hpdct_huffman_blob_bytes(void) { return static_cast<int64_t>(sizeof(hpdct::unscan::HuffBlob)); }

hpdct_status hpdct_huffman_prepare(const hpdct_huffman_spec specs[4], void* h_blob, int64_t capacity) {
    if (!specs || !h_blob) return fail(HPDCT_ERROR_INVALID_VALUE, "null specs or blob pointer");
    if (capacity < static_cast<int64_t>(sizeof(hpdct::unscan::HuffBlob)))
        return fail(HPDCT_ERROR_INVALID_VALUE, "blob buffer too small: " +
                                                   std::to_string(sizeof(hpdct::unscan::HuffBlob)) + " bytes needed");
    for (int kind = 0; kind < 4; ++kind)
        if (const char* why = hpdct::huff::defect(specs[kind], kind))
            return fail(HPDCT_ERROR_INVALID_VALUE, std::string(hpdct::huff::kind_name(kind)) + " Huffman table: " + why);
    hpdct::unscan::HuffBlob blob;
    hpdct::huff::fill_blob(specs, blob);
    memcpy(h_blob, &blob, sizeof(blob));  // h_blob: any alignment
    return HPDCT_SUCCESS;
}

hpdct_status hpdct_huffman_optimal(const uint64_t counts[256], hpdct_huffman_spec* out) {
    if (!counts || !out) return fail(HPDCT_ERROR_INVALID_VALUE, "null counts or spec pointer");
    for (int i = 0; i < 256; ++i)  // the sum of all of them stays below 2^63
        if (counts[i] > (1ull << 54)) return fail(HPDCT_ERROR_INVALID_VALUE, "a count above 2^54");
    hpdct::huff::optimal(counts, *out);
    return HPDCT_SUCCESS;
}

void hpdct_huffman_table(int kind, uint8_t* bits16, uint8_t* vals, int* nvals) {
    if (kind < 0 || kind > 3) {
        if (nvals) *nvals = 0;
        return;
    }
    const hpdct_huffman_spec& s = hpdct::scan::spec_of(kind);
    if (bits16) memcpy(bits16, s.bits, 16);
    if (vals) memcpy(vals, s.vals, static_cast<size_t>(s.nvals));
    if (nvals) *nvals = s.nvals;
}

hpdct_status hpdct_jpeg_header(uint8_t* h_out, int64_t capacity, int64_t* bytes, int64_t height, int64_t width,
                               int components, hpdct_subsampling sub, const float* q_luma64,
                               const float* q_chroma64, int64_t restart_interval) {
    return hpdct_jpeg_header_tables(h_out, capacity, bytes, height, width, components, sub, q_luma64, q_chroma64,
                                    restart_interval, nullptr);
}

hpdct_status hpdct_jpeg_header_tables(uint8_t* h_out, int64_t capacity, int64_t* bytes, int64_t height, int64_t width,
                                      int components, hpdct_subsampling sub, const float* q_luma64,
                                      const float* q_chroma64, int64_t restart_interval,
                                      const hpdct_huffman_spec specs[4]) {
    if (!h_out || !bytes) return fail(HPDCT_ERROR_INVALID_VALUE, "null header or length pointer");
    if (components != 1 && components != 3) return fail(HPDCT_ERROR_INVALID_VALUE, "components must be 1 or 3");
    if (components == 3)
        if (hpdct_status st = check_subsampling(sub)) return st;
    if (height < 1 || height > 65535 || width < 1 || width > 65535)
        return fail(HPDCT_ERROR_INVALID_VALUE, "a JPEG frame is 1..65535 pixels a side (got " +
                                                   std::to_string(height) + "x" + std::to_string(width) + ")");
    if (restart_interval < 0 || restart_interval > 65535)
        return fail(HPDCT_ERROR_INVALID_VALUE, "restart_interval must be 0..65535 (got " +
                                                   std::to_string(restart_interval) + ")");
    if (capacity < 0) return fail(HPDCT_ERROR_INVALID_VALUE, "negative capacity");
    uint8_t qz[2][64];
    const QState lib = current_qstate();
    if (hpdct_status st = header_table(q_luma64 ? q_luma64 : lib.qp.q.v, "luma", qz[0])) return st;
    if (components == 3)
        if (hpdct_status st = header_table(q_chroma64 ? q_chroma64 : kChromaQ, "chroma", qz[1])) return st;
    const int ntab = components == 3 ? 2 : 1;
    hpdct_huffman_spec tab[4];  // what DHT carries: the caller's, else Annex K's
    for (int k = 0; k < 2 * ntab; ++k) {
        tab[k] = specs ? specs[k] : hpdct::huff::annex_k(k);
        if (const char* why = hpdct::huff::defect(tab[k], k))
            return fail(HPDCT_ERROR_INVALID_VALUE, std::string(hpdct::huff::kind_name(k)) + " Huffman table: " + why);
    }
    std::vector<uint8_t> h;
    h.reserve(700);
    auto u8 = [&](unsigned v) { h.push_back(static_cast<uint8_t>(v)); };
    auto u16 = [&](unsigned v) { u8(v >> 8), u8(v & 0xffu); };
    u16(0xffd8);  // SOI
    u16(0xffe0), u16(16);  // APP0: JFIF 1.01, no density unit, aspect 1:1, no thumbnail
    for (unsigned c : {0x4au, 0x46u, 0x49u, 0x46u, 0u, 1u, 1u, 0u}) u8(c);
    u16(1), u16(1), u8(0), u8(0);
    u16(0xffdb), u16(2 + 65 * ntab);  // DQT: 8-bit entries in zig-zag order
    for (int t = 0; t < ntab; ++t) {
        u8(t);
        for (int i = 0; i < 64; ++i) u8(qz[t][i]);
    }
    const bool s420 = components == 3 && sub == HPDCT_SUBSAMPLING_420;
    u16(0xffc0), u16(8 + 3 * components), u8(8), u16(static_cast<unsigned>(height)),
        u16(static_cast<unsigned>(width)), u8(components);  // SOF0
    for (int c = 0; c < components; ++c) u8(c + 1), u8(c == 0 && s420 ? 0x22 : 0x11), u8(c == 0 ? 0 : 1);
    unsigned dht = 2;  // DHT: DC and AC luminance, then (3 components) chrominance
    for (int k = 0; k < 2 * ntab; ++k) dht += 17u + static_cast<unsigned>(tab[k].nvals);
    u16(0xffc4), u16(dht);
    for (int k = 0; k < 2 * ntab; ++k) {
        const hpdct_huffman_spec& s = tab[k];
        u8(((k & 1) << 4) | (k >> 1));  // class (0 DC, 1 AC) << 4 | destination
        for (int i = 0; i < 16; ++i) u8(s.bits[i]);
        for (int i = 0; i < s.nvals; ++i) u8(s.vals[i]);
    }
    if (restart_interval > 0) u16(0xffdd), u16(4), u16(static_cast<unsigned>(restart_interval));  // DRI
    u16(0xffda), u16(6 + 2 * components), u8(components);  // SOS
    for (int c = 0; c < components; ++c) u8(c + 1), u8(c == 0 ? 0x00 : 0x11);
    u8(0), u8(63), u8(0);
    *bytes = static_cast<int64_t>(h.size());
    if (capacity < *bytes)
        return fail(HPDCT_ERROR_INVALID_VALUE, "header buffer too small: " + std::to_string(*bytes) + " bytes needed");
    memcpy(h_out, h.data(), h.size());
    return HPDCT_SUCCESS;
}

// ---------------------------------------------------------------------------
// Entropy decoding: hpdct_decode_scan, hpdct_jpeg_parse (hpdct_unscan.hpp)
// ---------------------------------------------------------------------------
int64_t hpdct_decode_workspace_bytes(int64_t height, int64_t width, int components, hpdct_subsampling sub,
                                     int64_t restart_interval, int64_t scan_bytes) {
    hpdct::scan::ScanGrid g;
    uint64_t blocks[3];
    if (scan_bytes < 0 || scan_geometry(height, width, components, sub, restart_interval, g, blocks) != HPDCT_SUCCESS)
        return -1;
    return hpdct::unscan::workspace_bytes(g.intervals, static_cast<uint64_t>(scan_bytes));
}

int64_t hpdct_decode_split_workspace_bytes(int64_t height, int64_t width, int components, hpdct_subsampling sub,
                                           int64_t restart_interval, int64_t scan_bytes) {
    hpdct::scan::ScanGrid g;
    uint64_t blocks[3];
    if (scan_bytes < 0 || scan_geometry(height, width, components, sub, restart_interval, g, blocks) != HPDCT_SUCCESS)
        return -1;
    return static_cast<int64_t>(hpdct::unsplit::layout(g.intervals, static_cast<uint64_t>(scan_bytes)).bytes);
}

void hpdct_decode_split_geometry(int* segment_bytes, int* group_segments, int* rounds) {
    if (segment_bytes) *segment_bytes = static_cast<int>(hpdct::unsplit::kSegBytes);
    if (group_segments) *group_segments = static_cast<int>(hpdct::unsplit::kGroup);
    if (rounds) *rounds = static_cast<int>(hpdct::unsplit::kRounds);
}

hpdct_status hpdct_decode_scan(const uint8_t* d_scan, int64_t bytes, const uint64_t* d_interval_offsets, int16_t* d_y,
                               int16_t* d_cb, int16_t* d_cr, int64_t height, int64_t width, hpdct_subsampling sub,
                               int64_t restart_interval, unsigned flags, hpdct_decode_info* d_info,
                               uint64_t* d_interval_status, void* d_workspace, int64_t workspace_bytes, void* stream) {
    return decode_any(d_scan, bytes, d_interval_offsets, d_y, d_cb, d_cr, height, width, sub, restart_interval, flags,
                      false, 0, d_info, d_interval_status, d_workspace, workspace_bytes, nullptr, stream);
}

hpdct_status hpdct_decode_scan_tables(const uint8_t* d_scan, int64_t bytes, const uint64_t* d_interval_offsets,
                                      int16_t* d_y, int16_t* d_cb, int16_t* d_cr, int64_t height, int64_t width,
                                      hpdct_subsampling sub, int64_t restart_interval, unsigned flags,
                                      hpdct_decode_info* d_info, uint64_t* d_interval_status, void* d_workspace,
                                      int64_t workspace_bytes, const void* d_tables, void* stream) {
    return decode_any(d_scan, bytes, d_interval_offsets, d_y, d_cb, d_cr, height, width, sub, restart_interval, flags,
                      false, 0, d_info, d_interval_status, d_workspace, workspace_bytes, d_tables, stream);
}

hpdct_status hpdct_decode_scan_split(const uint8_t* d_scan, int64_t bytes, const uint64_t* d_interval_offsets,
                                     int16_t* d_y, int16_t* d_cb, int16_t* d_cr, int64_t height, int64_t width,
                                     hpdct_subsampling sub, int64_t restart_interval, unsigned flags,
                                     int64_t split_min_bytes, hpdct_decode_split_info* d_info,
                                     uint64_t* d_interval_status, void* d_workspace, int64_t workspace_bytes,
                                     void* stream) {
    return decode_any(d_scan, bytes, d_interval_offsets, d_y, d_cb, d_cr, height, width, sub, restart_interval, flags,
                      true, split_min_bytes, d_info, d_interval_status, d_workspace, workspace_bytes, nullptr, stream);
}

hpdct_status hpdct_decode_scan_split_tables(const uint8_t* d_scan, int64_t bytes, const uint64_t* d_interval_offsets,
                                            int16_t* d_y, int16_t* d_cb, int16_t* d_cr, int64_t height, int64_t width,
                                            hpdct_subsampling sub, int64_t restart_interval, unsigned flags,
                                            int64_t split_min_bytes, hpdct_decode_split_info* d_info,
                                            uint64_t* d_interval_status, void* d_workspace, int64_t workspace_bytes,
                                            const void* d_tables, void* stream) {
    return decode_any(d_scan, bytes, d_interval_offsets, d_y, d_cb, d_cr, height, width, sub, restart_interval, flags,
                      true, split_min_bytes, d_info, d_interval_status, d_workspace, workspace_bytes, d_tables, stream);
}

hpdct_status hpdct_jpeg_parse(const uint8_t* f, int64_t n, hpdct_jpeg_layout* out) {
    return jpeg_parse_any(f, n, out, nullptr);
}

hpdct_status hpdct_jpeg_parse_tables(const uint8_t* f, int64_t n, hpdct_jpeg_layout* out, hpdct_huffman_spec specs[4]) {
    if (!specs) return fail(HPDCT_ERROR_INVALID_VALUE, "null specs pointer");
    hpdct_huffman_spec got[4];
    memset(got, 0, sizeof(got));
    if (hpdct_status st = jpeg_parse_any(f, n, out, got)) return st;
    memcpy(specs, got, sizeof(got));
    return HPDCT_SUCCESS;
}

}  // extern "C"
