// hpdct_scan.hip -- the entropy coder's three launches (hpdct_scan.hpp) and its statistics pass
// (hpdct_scan_hist.hpp).
#define HPDCT_SCAN_KERNELS
#include "hpdct_scan.hpp"
#include "hpdct_launch.hpp"
#include "hpdct_scan_hist.hpp"
#include "hpdct_unscan.hpp"  // unscan::HuffBlob

namespace hpdct {

namespace {
// the measure launch, or with kScanEmit the emit launch.  The policy's kScanTables bit (set where the call has a
// blob) picks the kernel that reads the caller's tables, the coder's part of the blob; else Annex K's.  Tables
// outermost: the code object holds a launch's caller's-tables kernels before its Annex K ones (profiles/r14/README.md).
template <unsigned kEmitBit>
hipError_t launch_scan_code(const policy::Choice& c, hipStream_t s, const int16_t* y, const int16_t* cb,
                            const int16_t* cr, const scan::ScanGrid& g, uint64_t* lens, uint32_t* oor,
                            const hpdct_scan_info* info, uint8_t* out, uint64_t capacity,
                            const unscan::HuffBlob* blob) {
    return policy::with_bit<kScanTables, true>(c.var, [&](auto kT) {
        return policy::with_bit<kScanNatural, true>(c.var, [&](auto kN) {
            constexpr unsigned kV = with_block<64>(decltype(kN)::value | decltype(kT)::value | kEmitBit);
            if constexpr (decltype(kT)::value != 0u) {
                const uint32_t* tables = &blob->code.ac[0][0];
                return launch_choice<kV, scan_code_tables_kernel<kV>>(c, s, y, cb, cr, g, lens, oor, info, out,
                                                                      capacity, tables);
            } else {
                return launch_choice<kV, scan_code_kernel<kV>>(c, s, y, cb, cr, g, lens, oor, info, out, capacity);
            }
        });
    });
}
}  // namespace

hipError_t launch_scan(const int16_t* y, const int16_t* cb, const int16_t* cr, const scan::ScanGrid& g, bool natural,
                       uint8_t* out, uint64_t capacity, hpdct_scan_info* info, uint64_t* user_offs, void* workspace,
                       const unscan::HuffBlob* blob, hipStream_t s) {
    policy::ScanCall pc;
    pc.intervals = g.intervals, pc.natural = natural, pc.tables = blob != nullptr;
    // the workspace: a uint64 per interval (its length, then its offset), then a uint32 per interval
    uint64_t* lens = static_cast<uint64_t*>(workspace);
    uint32_t* oor = reinterpret_cast<uint32_t*>(lens + g.intervals);
    if (hipError_t e = launch_scan_code<0u>(policy::scan_code(pc, false), s, y, cb, cr, g, lens, oor, info, out,
                                            capacity, blob))
        return e;
    constexpr unsigned kOffV = with_block<1024>(kScanOffsets);
    const uint32_t* coor = oor;
    if (hipError_t e = launch_choice<kOffV, scan_offsets_kernel>(policy::scan_offsets(), s, lens, coor, g.intervals,
                                                                 user_offs, info, capacity))
        return e;
    return launch_scan_code<kScanEmit>(policy::scan_code(pc, true), s, y, cb, cr, g, lens, oor, info, out, capacity,
                                       blob);
}

}  // namespace hpdct
