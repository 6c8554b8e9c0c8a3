// hpdct_rgb_launch.hpp -- instantiates the colour forward kernels of one
// subsampling as policy::forward_rgb chose (hpdct_rgb_fwd420.hip,
// hpdct_rgb_fwd444.hip; their kRgbClip instantiations in hpdct_rgb_fwd420_clip.hip
// and hpdct_rgb_fwd444_clip.hip, four units that compile side by side).
#pragma once

#include "hpdct_rgb.hpp"
#include "hpdct_launch.hpp"

namespace hpdct {

// kSub: kRgb420 or 0, with or without kRgbClip.  The quotient pairs of
// policy::forward_rgb: luma JPEG forms or 3-op with the 3-op chroma quotient,
// or IEEE division for both.
template <unsigned kSub>
hipError_t launch_fdct_rgb_as(const uint8_t* rgb, int16_t* y, int16_t* cb, int16_t* cr, const RgbGrid& g,
                              const QParams& ql, const QParams& qc, bool natural, const policy::Choice& c,
                              hipStream_t s) {
    return policy::with_quotient<true>(c.var, [&](auto kQ) {
        constexpr unsigned kQv = decltype(kQ)::value;
        constexpr unsigned kV = policy::kRgbFwdVar | kSub | kQv | (kQv != 0u ? kRgbChromaFastDiv : 0u);
        if (natural) return launch_choice<kV, fdct_rgb_kernel<true, kV>>(c, s, rgb, y, cb, cr, g, ql, qc);
        return launch_choice<kV, fdct_rgb_kernel<false, kV>>(c, s, rgb, y, cb, cr, g, ql, qc);
    });
}

// The same under HPDCT_FRAME_DCT (kFrameDct; hpdct_dct_rgb_fwd420.hip, hpdct_dct_rgb_fwd444.hip and their *_clip.hip
// units).  The quotient pairs of policy::forward_rgb's DCT row: the 3-op quotient for both tables or IEEE division
// for both, never the per-position forms.
template <unsigned kSub>
hipError_t launch_fdct_rgb_dct_as(const uint8_t* rgb, int16_t* y, int16_t* cb, int16_t* cr, const RgbGrid& g,
                                  const QParams& ql, const QParams& qc, bool natural, const policy::Choice& c,
                                  hipStream_t s) {
    if ((c.var & kVarJpegQ) != 0u) return hipErrorInvalidDeviceFunction;
    return policy::with_bit<kVarFastDiv, true>(c.var, [&](auto kQ) {
        constexpr unsigned kQv = decltype(kQ)::value;
        constexpr unsigned kV = policy::kRgbFwdDctVar | kSub | kQv | (kQv != 0u ? kRgbChromaFastDiv : 0u);
        if (natural) return launch_choice<kV, fdct_rgb_kernel<true, kV>>(c, s, rgb, y, cb, cr, g, ql, qc);
        return launch_choice<kV, fdct_rgb_kernel<false, kV>>(c, s, rgb, y, cb, cr, g, ql, qc);
    });
}

}  // namespace hpdct
