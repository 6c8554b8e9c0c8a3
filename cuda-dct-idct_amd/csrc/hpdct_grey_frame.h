// hpdct_grey_frame.h -- host-visible declarations of the grey frame kernels
// (hpdct_grey_frame.hpp): a uint8 frame of any height, width, row pitch and
// alignment <-> the int16 blocks of the frame padded to whole tiles, quantised
// with a table that travels in the kernel arguments.  The launchers are in
// hpdct_grey_frame_fwd.hip, hpdct_grey_frame_fwd_clip.hip and
// hpdct_grey_frame_inv.hip.
#pragma once

#include "hpdct_kernels.h"

namespace hpdct {

// the grey frame kernels' own variant bit
enum : unsigned {
    kGreyClip = 1u << 24,  // the general instantiation: a frame that is not whole tiles (edge-replicated on the
                           // way in, cropped on the way out) or whose base or row pitch is not 8-byte aligned;
                           // clear: whole tiles, 8-byte loads and stores everywhere
};

// Tile geometry of one launch.  The tile grid covers the padded frame (height
// and width rounded up to 8): ntiles = (Hp/8) * (Wp/8) < 2^32, block index =
// tile index.  The kernels without kGreyClip read ntiles, tiles_x and pitch only.
struct GreyGrid {
    uint32_t ntiles;
    uint32_t tiles_x;  // tiles per tile row: Wp / 8
    uint64_t pitch;    // bytes from one image row to the next (>= width)
    uint64_t height;   // the frame's own rows and pixels per row
    uint64_t width;
};
// whole tiles, base and pitch 8-byte aligned: the kernels without kGreyClip
inline bool grey_whole_aligned(const void* image, const GreyGrid& g) {
    return g.height % 8u == 0u && g.width % 8u == 0u && g.pitch % 8u == 0u &&
           reinterpret_cast<uintptr_t>(image) % 8u == 0u;
}

// Forward: built-in T, level shift 128, quantised with qp (qmode as launch_fdct;
// the caller proved |q| <= 32767): hpdct_forward_blocks' arithmetic on the
// edge-replicated padded frame.
hipError_t launch_fdct_grey_frame(const uint8_t* image, int16_t* blocks, const GreyGrid& g, const QParams& qp,
                                  int qmode, bool natural, hipStream_t s);
// the two units of the forward (hpdct_grey_frame_fwd.hip / hpdct_grey_frame_fwd_clip.hip), as c chose
hipError_t launch_fdct_grey_frame_whole(const uint8_t* image, int16_t* blocks, const GreyGrid& g, const QParams& qp,
                                        bool natural, const policy::Choice& c, hipStream_t s);
hipError_t launch_fdct_grey_frame_clip(const uint8_t* image, int16_t* blocks, const GreyGrid& g, const QParams& qp,
                                       bool natural, const policy::Choice& c, hipStream_t s);
// Inverse: blocks -> uint8 pixels (clamp + truncate), the top-left height x width of the padded frame.
// full_chain: q fails the skip criterion for int16 coefficients (the kVarFullChain kernel)
hipError_t launch_idct_grey_frame(const int16_t* blocks, uint8_t* image, const GreyGrid& g, const Mat64& q,
                                  bool natural, bool full_chain, hipStream_t s);
// The same two calls under HPDCT_FRAME_DCT (kFrameDct; hpdct_dct_grey_fwd.hip, hpdct_dct_grey_inv.hip): the exact
// DCT's matrix, the inverse's pixels rounded.  qmode 0 or 1 (a 2 is taken as 1: no per-position forms); the inverse
// has no full_chain, it keeps every term anyway.
hipError_t launch_fdct_grey_frame_dct(const uint8_t* image, int16_t* blocks, const GreyGrid& g, const QParams& qp,
                                      int qmode, bool natural, hipStream_t s);
hipError_t launch_idct_grey_frame_dct(const int16_t* blocks, uint8_t* image, const GreyGrid& g, const Mat64& q,
                                      bool natural, hipStream_t s);

}  // namespace hpdct
