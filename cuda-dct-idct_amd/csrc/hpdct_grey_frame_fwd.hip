// hpdct_grey_frame_fwd.hip -- launcher of the grey frame forward kernels
// (hpdct_grey_frame.hpp), and the instantiations without kGreyClip: whole tiles,
// base and pitch 8-byte aligned.  The general ones are in
// hpdct_grey_frame_fwd_clip.hip so the two compile in parallel.
#include "hpdct_grey_frame.hpp"
#include "hpdct_launch.hpp"

namespace hpdct {

hipError_t launch_fdct_grey_frame_whole(const uint8_t* image, int16_t* blocks, const GreyGrid& g, const QParams& qp,
                                        bool natural, const policy::Choice& c, hipStream_t s) {
    return policy::with_quotient<true>(c.var, [&](auto kQ) {
        constexpr unsigned kV = policy::kGreyFwdVar | decltype(kQ)::value;
        if (natural) return launch_choice<kV, fdct_grey_frame_kernel<true, kV>>(c, s, image, blocks, g, qp, qp.q);
        return launch_choice<kV, fdct_grey_frame_kernel<false, kV>>(c, s, image, blocks, g, qp, qp.q);
    });
}

hipError_t launch_fdct_grey_frame(const uint8_t* image, int16_t* blocks, const GreyGrid& g, const QParams& qp,
                                  int qmode, bool natural, hipStream_t s) {
    policy::GreyCall pc;
    pc.tiles = g.ntiles, pc.qmode = qmode, pc.clip = !grey_whole_aligned(image, g);
    const policy::Choice c = policy::forward_grey(pc);
    if (c.family != policy::Family::kGrey) return hipErrorInvalidDeviceFunction;
    if ((c.var & kGreyClip) != 0u) return launch_fdct_grey_frame_clip(image, blocks, g, qp, natural, c, s);
    return launch_fdct_grey_frame_whole(image, blocks, g, qp, natural, c, s);
}

}  // namespace hpdct
