// hpdct_grey_frame_fwd_clip.hip -- the grey frame forward kernels with kGreyClip
// (hpdct_grey_frame.hpp): frames that are not whole tiles, or whose base or row
// pitch is not 8-byte aligned.
#include "hpdct_grey_frame.hpp"
#include "hpdct_launch.hpp"

namespace hpdct {

hipError_t launch_fdct_grey_frame_clip(const uint8_t* image, int16_t* blocks, const GreyGrid& g, const QParams& qp,
                                       bool natural, const policy::Choice& c, hipStream_t s) {
    return policy::with_quotient<true>(c.var, [&](auto kQ) {
        constexpr unsigned kV = policy::kGreyFwdVar | kGreyClip | decltype(kQ)::value;
        if (natural) return launch_choice<kV, fdct_grey_frame_kernel<true, kV>>(c, s, image, blocks, g, qp, qp.q);
        return launch_choice<kV, fdct_grey_frame_kernel<false, kV>>(c, s, image, blocks, g, qp, qp.q);
    });
}

}  // namespace hpdct
