// hpdct_api_internal.hpp -- what the units of the extern "C" boundary share (hpdct_api.cpp, which defines what is
// declared here, and hpdct_api_jpeg.cpp): the last-error text, the buffer checks, the frame's grid and the
// library-owned quantiser.  Host only; not part of the ABI: the namespace is hidden, libhpdct.so does not export it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "hpdct.h"
#include "hpdct_kernels.h"

namespace hpdct {
namespace api __attribute__((visibility("hidden"))) {

// every refusal: the text goes to the calling thread's hpdct_last_error_string
hpdct_status fail(hpdct_status st, const std::string& msg);
hpdct_status device_status(hipError_t e, const char* what);

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// A caller's buffer as the overlap checks see it.  The address is an integer:
// an extent up to 2^63 past a pointer is no pointer arithmetic.
struct Span {
    uintptr_t p;
    size_t n;
    const char* name;
    Span(const void* ptr, size_t bytes, const char* nm = "") : p(reinterpret_cast<uintptr_t>(ptr)), n(bytes), name(nm) {}
};

// No two of the spans may share a byte.  Spans of zero bytes (an optional
// buffer left out) are skipped; a span whose end would wrap the address space
// is refused with `wrap_msg`, then the first overlapping pair with
// `overlap_msg`, or, when that is NULL, with the two spans' names.
hpdct_status check_disjoint(const Span* s, int count, const char* wrap_msg, const char* overlap_msg);
constexpr const char* kWrapMsg = "a buffer would wrap the address space";

hpdct_status check_subsampling(hpdct_subsampling sub);

// the tile grid of a frame whose sides are positive multiples of 8, below 2^32 tiles
hpdct_status make_grid(int64_t height, int64_t width, TileGrid& g);
// the units of a padded frame (8x8 tiles, or 16x16 MCUs for 4:2:0) from its
// tile grid: how many, and how many in a row
inline void units_of(const TileGrid& g, bool s420, uint32_t& nunits, uint32_t& units_x) {
    nunits = s420 ? g.ntiles / 4u : g.ntiles;
    units_x = s420 ? g.tiles_x / 2u : g.tiles_x;
}

// an integer in 1..255: what the verified quotient and a baseline JPEG file take
inline bool byte_integer(float v) { return v >= 1.0f && v <= 255.0f && v == std::floor(v); }

// The library-owned quantiser: the table, its reciprocals and the two
// properties the launches need, computed once per hpdct_set_quant_table
// (not per call) and copied out under the mutex.
struct QState {
    QParams qp;
    bool fastdiv_ok;  // integers in 1..255: the verified 3-op quotient is exact
    bool int8_ok;     // |q| <= 127 for uint8 input with the built-in T
    bool jpeg;        // bit for bit the default JPEG table: the per-position
                      // 3-op forms of hpdct_quant_forms.h apply (uint8 input,
                      // built-in T, level shift 128)
    bool int16_ok;    // |q| <= 32767 for uint8 input with the built-in T (int16 blocks)
    bool skip16_ok;   // skip_zero_exact for int16 blocks: the block and colour inverses may skip T's zeros
    bool skip8_ok;    // the same for int8 coefficients (hpdct_inverse with HPDCT_I8 input)
};
QState current_qstate();

// JPEG Annex K.2, the chrominance table
extern const float kChromaQ[64];

}  // namespace api
}  // namespace hpdct
