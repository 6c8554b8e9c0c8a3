// hpdct_unscan.hip -- the entropy decoder's launches (hpdct_unscan.hpp).  The kernels are named here in the order
// the code object holds them (profiles/r14/README.md): all of Annex K's, then all that read the caller's tables.
#define HPDCT_UNSCAN_KERNELS
#include "hpdct_unscan.hpp"
#include "hpdct_launch.hpp"

namespace hpdct {

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
                         void* workspace, const unscan::HuffBlob* blob, hipStream_t s) {
    if (hipError_t e = launch_unscan_locate(scan, bytes, offs, g, info, workspace, s)) return e;
    const uint64_t* mpos = static_cast<const uint64_t*>(workspace);
    policy::UnscanCall pc;
    pc.intervals = g.intervals, pc.natural = natural, pc.tables = blob != nullptr;
    const policy::Choice c = policy::unscan_decode(pc);
    // kT: 0 for Annex K's kernels, kScanTables for those that read the caller's blob
    auto decode = [&](auto kT) {
        return with_lanes(c.var, [&](auto kL) {
            return policy::with_bit<kScanNatural, true>(c.var, [&](auto kN) {
                constexpr unsigned kV = with_block<64>(decltype(kN)::value | decltype(kL)::value | decltype(kT)::value);
                if constexpr (decltype(kT)::value != 0u)
                    return launch_choice<kV, unscan_decode_tables_kernel<kV>>(c, s, scan, bytes, offs, mpos, y, cb, cr,
                                                                              g, info, status, blob);
                else
                    return launch_choice<kV, unscan_decode_kernel<kV>>(c, s, scan, bytes, offs, mpos, y, cb, cr, g,
                                                                       info, status);
            });
        });
    };
    if (!blob) return decode(std::integral_constant<unsigned, 0u>{});
    return decode(std::integral_constant<unsigned, kScanTables>{});
}

}  // namespace hpdct
