// hpdct_dct_rgb_fwd444.hip -- the 4:4:4 colour forward kernels under
// HPDCT_FRAME_DCT (hpdct_rgb.hpp with kFrameDct): whole tiles, base and pitch
// 8-byte aligned.
#include "hpdct_rgb_launch.hpp"

namespace hpdct {

hipError_t launch_fdct_rgb_dct_444(const uint8_t* rgb, int16_t* y, int16_t* cb, int16_t* cr, const RgbGrid& g,
                                   const QParams& ql, const QParams& qc, bool natural, const policy::Choice& c,
                                   hipStream_t s) {
    return launch_fdct_rgb_dct_as<0u>(rgb, y, cb, cr, g, ql, qc, natural, c, s);
}

}  // namespace hpdct
