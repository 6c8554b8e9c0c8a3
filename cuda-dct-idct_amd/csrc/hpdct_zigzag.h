// hpdct_zigzag.h -- the JPEG zig-zag scan of an 8x8 block, one copy for the
// host (hpdct_zigzag_order) and the block kernels (hpdct_blocks.hpp), which
// index it with compile-time constants only.  Plain C++: hpdct_api.cpp and
// hpdct_api_jpeg.cpp include it under g++ too.
#pragma once

namespace hpdct {
namespace zigzag {

// kOrder[n] = 8 * v + u of the n-th coefficient of the scan
constexpr unsigned char kOrder[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                      12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                      35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                      58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// row-major position of element n of a block (zig-zag or natural order)
constexpr int position_of(bool natural, int n) { return natural ? n : kOrder[n]; }
// element index of row-major position pos
constexpr int element_of(bool natural, int pos) {
    if (natural) return pos;
    for (int n = 0; n < 64; ++n)
        if (kOrder[n] == pos) return n;
    return -1;
}

}  // namespace zigzag
}  // namespace hpdct
