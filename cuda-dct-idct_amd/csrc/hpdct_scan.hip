// hpdct_scan.hip -- the entropy coder's three launches (hpdct_scan.hpp) and its statistics pass
// (hpdct_scan_hist.hpp).
#define HPDCT_SCAN_KERNELS
#include "hpdct_scan.hpp"
#include "hpdct_launch.hpp"
#include "hpdct_scan_hist.hpp"

namespace hpdct {

namespace {
template <unsigned kEmitBit>
hipError_t launch_scan_code(const policy::Choice& c, hipStream_t s, const int16_t* y, const int16_t* cb,
                            const int16_t* cr, const scan::ScanGrid& g, uint64_t* lens, uint32_t* oor,
                            const hpdct_scan_info* info, uint8_t* out, uint64_t capacity) {
    return policy::with_bit<kScanNatural, true>(c.var, [&](auto kN) {
        constexpr unsigned kV = with_block<64>(decltype(kN)::value | kEmitBit);
        return launch_choice<kV, scan_code_kernel<kV>>(c, s, y, cb, cr, g, lens, oor, info, out, capacity);
    });
}
template <unsigned kEmitBit>
hipError_t launch_scan_code_tables(const policy::Choice& c, hipStream_t s, const int16_t* y, const int16_t* cb,
                                   const int16_t* cr, const scan::ScanGrid& g, uint64_t* lens, uint32_t* oor,
                                   const hpdct_scan_info* info, uint8_t* out, uint64_t capacity,
                                   const uint32_t* tables) {
    return policy::with_bit<kScanNatural, true>(c.var, [&](auto kN) {
        constexpr unsigned kV = with_block<64>(decltype(kN)::value | kEmitBit | kScanTables);
        return launch_choice<kV, scan_code_tables_kernel<kV>>(c, s, y, cb, cr, g, lens, oor, info, out, capacity,
                                                              tables);
    });
}

// tables == nullptr: Annex K
hipError_t launch_scan_any(const int16_t* y, const int16_t* cb, const int16_t* cr, const scan::ScanGrid& g,
                           bool natural, uint8_t* out, uint64_t capacity, hpdct_scan_info* info, uint64_t* user_offs,
                           void* workspace, const uint32_t* tables, hipStream_t s) {
    policy::ScanCall pc;
    pc.intervals = g.intervals, pc.natural = natural, pc.tables = tables != nullptr;
    // the workspace: a uint64 per interval (its length, then its offset), then a uint32 per interval
    uint64_t* lens = static_cast<uint64_t*>(workspace);
    uint32_t* oor = reinterpret_cast<uint32_t*>(lens + g.intervals);
    const hpdct_scan_info* cinfo = info;
    if (hipError_t e = tables ? launch_scan_code_tables<0u>(policy::scan_code(pc, false), s, y, cb, cr, g, lens, oor,
                                                            cinfo, out, capacity, tables)
                              : launch_scan_code<0u>(policy::scan_code(pc, false), s, y, cb, cr, g, lens, oor, cinfo,
                                                     out, capacity))
        return e;
    constexpr unsigned kOffV = with_block<1024>(kScanOffsets);
    const uint32_t* coor = oor;
    if (hipError_t e = launch_choice<kOffV, scan_offsets_kernel>(policy::scan_offsets(), s, lens, coor, g.intervals,
                                                                 user_offs, info, capacity))
        return e;
    if (tables)
        return launch_scan_code_tables<kScanEmit>(policy::scan_code(pc, true), s, y, cb, cr, g, lens, oor, cinfo, out,
                                                  capacity, tables);
    return launch_scan_code<kScanEmit>(policy::scan_code(pc, true), s, y, cb, cr, g, lens, oor, cinfo, out, capacity);
}
}  // namespace

hipError_t launch_scan(const int16_t* y, const int16_t* cb, const int16_t* cr, const scan::ScanGrid& g, bool natural,
                       uint8_t* out, uint64_t capacity, hpdct_scan_info* info, uint64_t* user_offs, void* workspace,
                       hipStream_t s) {
    return launch_scan_any(y, cb, cr, g, natural, out, capacity, info, user_offs, workspace, nullptr, s);
}

hipError_t launch_scan_tables(const int16_t* y, const int16_t* cb, const int16_t* cr, const scan::ScanGrid& g,
                              bool natural, uint8_t* out, uint64_t capacity, hpdct_scan_info* info,
                              uint64_t* user_offs, void* workspace, const void* d_tables, hipStream_t s) {
    return launch_scan_any(y, cb, cr, g, natural, out, capacity, info, user_offs, workspace,
                           static_cast<const uint32_t*>(d_tables), s);
}

}  // namespace hpdct
