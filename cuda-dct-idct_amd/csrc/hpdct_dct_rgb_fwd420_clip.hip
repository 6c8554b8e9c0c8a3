// hpdct_dct_rgb_fwd420_clip.hip -- the 4:2:0 colour forward kernels under
// HPDCT_FRAME_DCT, general instantiation (kRgbClip with kFrameDct, hpdct_rgb.hpp):
// frames that are not whole MCUs, or whose base or row pitch is not 8-byte
// aligned.
#include "hpdct_rgb_launch.hpp"

namespace hpdct {

hipError_t launch_fdct_rgb_dct_420_clip(const uint8_t* rgb, int16_t* y, int16_t* cb, int16_t* cr, const RgbGrid& g,
                                        const QParams& ql, const QParams& qc, bool natural, const policy::Choice& c,
                                        hipStream_t s) {
    return launch_fdct_rgb_dct_as<kRgb420 | kRgbClip>(rgb, y, cb, cr, g, ql, qc, natural, c, s);
}

}  // namespace hpdct
