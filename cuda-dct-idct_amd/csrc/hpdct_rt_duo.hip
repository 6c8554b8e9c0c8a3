// hpdct_rt_duo.hip -- the two-lanes-per-tile round trip (hpdct_rt_duo.hpp),
// the uint8 -> fp32 duo forward and the sums finish kernel.
#include "hpdct_rt_duo.hpp"

namespace hpdct {

static_assert(policy::kDuoFwdBlock == 256, "fdct_duo_u8_kernel is built for 256-thread workgroups");

hipError_t launch_fdct_duo_u8(const uint8_t* img, float* coef, const TileGrid& g, const QParams& qp,
                              const policy::Choice& c, hipStream_t s) {
    return policy::with_bit<kVarJpegQ, true>(c.var, [&](auto kJ) {
        return launch_capped<fdct_duo_u8_kernel<decltype(kJ)::value != 0u ? 2 : 1>>(dim3(c.grid_x), dim3(c.block),
                                                                                  c.cap_wgs, s, img, coef, g, qp);
    });
}

hipError_t launch_fdct_duo_u8_frames(const FrameTable<float>& ft, const TileGrid& g, const QParams& qp,
                                     const policy::Choice& c, hipStream_t s) {
    return policy::with_bit<kVarJpegQ, true>(c.var, [&](auto kJ) {
        return launch_capped<fdct_duo_u8_frames_kernel<decltype(kJ)::value != 0u ? 2 : 1>>(
            dim3(c.grid_x, c.grid_y), dim3(c.block), c.cap_wgs, s, ft, g, qp);
    });
}

hipError_t launch_rt_duo(const uint8_t* img, float* coef, void* recon, int recon_kind, unsigned long long* spread,
                         const TileGrid& g, const QParams& qp, const policy::Choice& c, hipStream_t s) {
    // neither a reconstruction nor sums: the forward alone
    if (c.family == policy::Family::kDuoFwdU8) return launch_fdct_duo_u8(img, coef, g, qp, c, s);
    if (recon_kind == kRtReconF32) return launch_rt_duo_f32(img, coef, recon, spread, g, qp, c, s);
    if (recon_kind == kRtReconU8) return rt_duo_detail::go_r<kRtReconU8>(img, coef, recon, spread, g, qp, c, s);
    return rt_duo_detail::go_r<kRtReconNone>(img, coef, nullptr, spread, g, qp, c, s);
}

hipError_t launch_rt_finish(RtSums* dst, unsigned long long* spread, bool accumulate, hipStream_t s) {
    return launch_capped<rt_spread_finish_kernel<>>(dim3(1), dim3(64), 0, s, dst, spread, accumulate ? 1 : 0);
}

}  // namespace hpdct
