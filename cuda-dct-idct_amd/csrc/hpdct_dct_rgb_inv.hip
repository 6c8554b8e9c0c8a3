// hpdct_dct_rgb_inv.hip -- the colour inverse kernels under HPDCT_FRAME_DCT
// (hpdct_rgb.hpp with kFrameDct): the exact DCT's matrix, every term, each
// component rounded (R + 128.5f, clamp, truncate) before the unchanged
// fixed-point conversion; both subsamplings, with and without kRgbClip, for
// every table.
#include "hpdct_rgb.hpp"
#include "hpdct_launch.hpp"

namespace hpdct {

hipError_t launch_idct_rgb_dct(const int16_t* y, const int16_t* cb, const int16_t* cr, uint8_t* rgb, const RgbGrid& g,
                               bool s420, const Mat64& ql, const Mat64& qc, bool natural, hipStream_t s) {
    policy::RgbCall pc;
    pc.units = g.nunits, pc.s420 = s420, pc.clip = !rgb_whole_aligned(rgb, g, s420), pc.dct = true;
    const policy::Choice c = policy::inverse_rgb(pc);
    if (c.family != policy::Family::kRgb) return hipErrorInvalidDeviceFunction;
    return policy::with_bit<kRgb420, true>(c.var, [&](auto kS) {
        return policy::with_bit<kRgbClip, true>(c.var, [&](auto kC) {
            constexpr unsigned kV = policy::kRgbInvDctVar | decltype(kS)::value | decltype(kC)::value;
            if (natural) return launch_choice<kV, idct_rgb_kernel<true, kV>>(c, s, y, cb, cr, rgb, g, ql, qc);
            return launch_choice<kV, idct_rgb_kernel<false, kV>>(c, s, y, cb, cr, rgb, g, ql, qc);
        });
    });
}

}  // namespace hpdct
