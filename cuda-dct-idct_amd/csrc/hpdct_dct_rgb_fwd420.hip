// hpdct_dct_rgb_fwd420.hip -- the 4:2:0 colour forward kernels under
// HPDCT_FRAME_DCT (hpdct_rgb.hpp with kFrameDct) and launch_fdct_rgb_dct, which
// asks the policy and hands 4:4:4 to hpdct_dct_rgb_fwd444.hip and the kRgbClip
// instantiations to the two hpdct_dct_rgb_fwd*_clip.hip units (so the four
// compile in parallel).
#include "hpdct_rgb_launch.hpp"

namespace hpdct {

hipError_t launch_fdct_rgb_dct_420(const uint8_t* rgb, int16_t* y, int16_t* cb, int16_t* cr, const RgbGrid& g,
                                   const QParams& ql, const QParams& qc, bool natural, const policy::Choice& c,
                                   hipStream_t s) {
    return launch_fdct_rgb_dct_as<kRgb420>(rgb, y, cb, cr, g, ql, qc, natural, c, s);
}

hipError_t launch_fdct_rgb_dct(const uint8_t* rgb, int16_t* y, int16_t* cb, int16_t* cr, const RgbGrid& g, bool s420,
                               const QParams& ql, const QParams& qc, int qmode_luma, int qmode_chroma, bool natural,
                               hipStream_t s) {
    policy::RgbCall pc;
    pc.units = g.nunits, pc.s420 = s420, pc.qmode_luma = qmode_luma, pc.qmode_chroma = qmode_chroma;
    pc.clip = !rgb_whole_aligned(rgb, g, s420), pc.dct = true;
    const policy::Choice c = policy::forward_rgb(pc);
    if (c.family != policy::Family::kRgb) return hipErrorInvalidDeviceFunction;
    if ((c.var & kRgbClip) != 0u) {
        if (s420) return launch_fdct_rgb_dct_420_clip(rgb, y, cb, cr, g, ql, qc, natural, c, s);
        return launch_fdct_rgb_dct_444_clip(rgb, y, cb, cr, g, ql, qc, natural, c, s);
    }
    if (s420) return launch_fdct_rgb_dct_420(rgb, y, cb, cr, g, ql, qc, natural, c, s);
    return launch_fdct_rgb_dct_444(rgb, y, cb, cr, g, ql, qc, natural, c, s);
}

}  // namespace hpdct
