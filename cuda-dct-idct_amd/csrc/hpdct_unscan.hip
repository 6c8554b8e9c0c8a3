// hpdct_unscan.hip -- the entropy decoder's launches (hpdct_unscan.hpp).
#define HPDCT_UNSCAN_KERNELS
#include "hpdct_unscan.hpp"
#include "hpdct_launch.hpp"

namespace hpdct {

namespace {
template <unsigned kLaneBit>
hipError_t launch_unscan_decode(const policy::Choice& c, hipStream_t s, const uint8_t* scan, uint64_t bytes,
                                const uint64_t* offs, const uint64_t* mpos, int16_t* y, int16_t* cb, int16_t* cr,
                                const scan::ScanGrid& g, hpdct_decode_info* info, uint64_t* status) {
    return policy::with_bit<kScanNatural, true>(c.var, [&](auto kN) {
        constexpr unsigned kV = with_block<64>(decltype(kN)::value | kLaneBit);
        return launch_choice<kV, unscan_decode_kernel<kV>>(c, s, scan, bytes, offs, mpos, y, cb, cr, g, info, status);
    });
}
template <unsigned kLaneBit>
hipError_t launch_unscan_decode_tables(const policy::Choice& c, hipStream_t s, const uint8_t* scan, uint64_t bytes,
                                       const uint64_t* offs, const uint64_t* mpos, int16_t* y, int16_t* cb,
                                       int16_t* cr, const scan::ScanGrid& g, hpdct_decode_info* info,
                                       uint64_t* status, const unscan::HuffBlob* blob) {
    return policy::with_bit<kScanNatural, true>(c.var, [&](auto kN) {
        constexpr unsigned kV = with_block<64>(decltype(kN)::value | kLaneBit | kScanTables);
        return launch_choice<kV, unscan_decode_tables_kernel<kV>>(c, s, scan, bytes, offs, mpos, y, cb, cr, g, info,
                                                                  status, blob);
    });
}
}  // namespace

hipError_t launch_unscan_locate(const uint8_t* scan, uint64_t bytes, const uint64_t* offs, const scan::ScanGrid& g,
                                hpdct_decode_info* info, void* workspace, hipStream_t s) {
    // the workspace: a uint64 per interval (a marker's position), then a uint64 per chunk (its count, then its rank)
    uint64_t* mpos = static_cast<uint64_t*>(workspace);
    uint64_t* counts = mpos + unscan::marker_words(g.intervals);
    const uint64_t nchunks = offs ? 0u : unscan::chunks_of(bytes);
    constexpr unsigned kCountV = with_block<256>(kUnscanCount), kPlaceV = with_block<256>(kUnscanCount | kUnscanPlace);
    if (!offs)
        if (hipError_t e = launch_choice<kCountV, unscan_locate_kernel<kCountV>>(
                policy::unscan_locate(nchunks, false), s, scan, bytes, nchunks, counts, mpos, g.intervals, info))
            return e;
    constexpr unsigned kRankV = with_block<1024>(kUnscanRank);
    if (hipError_t e = launch_choice<kRankV, unscan_rank_kernel>(policy::unscan_rank(), s, counts, nchunks, info))
        return e;
    if (!offs)
        if (hipError_t e = launch_choice<kPlaceV, unscan_locate_kernel<kPlaceV>>(
                policy::unscan_locate(nchunks, true), s, scan, bytes, nchunks, counts, mpos, g.intervals, info))
            return e;
    return hipSuccess;
}

hipError_t launch_unscan(const uint8_t* scan, uint64_t bytes, const uint64_t* offs, int16_t* y, int16_t* cb,
                         int16_t* cr, const scan::ScanGrid& g, bool natural, hpdct_decode_info* info, uint64_t* status,
                         void* workspace, hipStream_t s) {
    if (hipError_t e = launch_unscan_locate(scan, bytes, offs, g, info, workspace, s)) return e;
    const uint64_t* mpos = static_cast<const uint64_t*>(workspace);
    policy::UnscanCall pc;
    pc.intervals = g.intervals, pc.natural = natural;
    const policy::Choice c = policy::unscan_decode(pc);
    const uint64_t* cmpos = mpos;
    switch (unscan_lanes_of(c.var)) {
        case 1u: return launch_unscan_decode<kUnscanLanes1>(c, s, scan, bytes, offs, cmpos, y, cb, cr, g, info, status);
        case 4u: return launch_unscan_decode<kUnscanLanes4>(c, s, scan, bytes, offs, cmpos, y, cb, cr, g, info, status);
        case 16u:
            return launch_unscan_decode<kUnscanLanes16>(c, s, scan, bytes, offs, cmpos, y, cb, cr, g, info, status);
        default: return launch_unscan_decode<0u>(c, s, scan, bytes, offs, cmpos, y, cb, cr, g, info, status);
    }
}

hipError_t launch_unscan_tables(const uint8_t* scan, uint64_t bytes, const uint64_t* offs, int16_t* y, int16_t* cb,
                                int16_t* cr, const scan::ScanGrid& g, bool natural, hpdct_decode_info* info,
                                uint64_t* status, void* workspace, const void* d_tables, hipStream_t s) {
    if (hipError_t e = launch_unscan_locate(scan, bytes, offs, g, info, workspace, s)) return e;
    const uint64_t* mpos = static_cast<const uint64_t*>(workspace);
    const unscan::HuffBlob* blob = static_cast<const unscan::HuffBlob*>(d_tables);
    policy::UnscanCall pc;
    pc.intervals = g.intervals, pc.natural = natural, pc.tables = true;
    const policy::Choice c = policy::unscan_decode(pc);
    switch (unscan_lanes_of(c.var)) {
        case 1u:
            return launch_unscan_decode_tables<kUnscanLanes1>(c, s, scan, bytes, offs, mpos, y, cb, cr, g, info, status,
                                                              blob);
        case 4u:
            return launch_unscan_decode_tables<kUnscanLanes4>(c, s, scan, bytes, offs, mpos, y, cb, cr, g, info, status,
                                                              blob);
        case 16u:
            return launch_unscan_decode_tables<kUnscanLanes16>(c, s, scan, bytes, offs, mpos, y, cb, cr, g, info,
                                                               status, blob);
        default:
            return launch_unscan_decode_tables<0u>(c, s, scan, bytes, offs, mpos, y, cb, cr, g, info, status, blob);
    }
}

}  // namespace hpdct
