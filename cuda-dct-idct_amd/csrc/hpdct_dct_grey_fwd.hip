// hpdct_dct_grey_fwd.hip -- the grey frame forward kernels under HPDCT_FRAME_DCT
// (hpdct_grey_frame.hpp with kFrameDct): the exact DCT's matrix as immediates,
// with and without kGreyClip, IEEE division or the verified 3-op quotient.  A
// unit of its own: the HpApprDCT units' code objects do not change with it.
#include "hpdct_grey_frame.hpp"
#include "hpdct_launch.hpp"

namespace hpdct {

hipError_t launch_fdct_grey_frame_dct(const uint8_t* image, int16_t* blocks, const GreyGrid& g, const QParams& qp,
                                      int qmode, bool natural, hipStream_t s) {
    policy::GreyCall pc;
    pc.tiles = g.ntiles, pc.qmode = qmode, pc.clip = !grey_whole_aligned(image, g), pc.dct = true;
    const policy::Choice c = policy::forward_grey(pc);
    if (c.family != policy::Family::kGrey || (c.var & kVarJpegQ) != 0u) return hipErrorInvalidDeviceFunction;
    return policy::with_bit<kGreyClip, true>(c.var, [&](auto kC) {
        return policy::with_bit<kVarFastDiv, true>(c.var, [&](auto kQ) {
            constexpr unsigned kV = policy::kGreyFwdDctVar | decltype(kC)::value | decltype(kQ)::value;
            if (natural) return launch_choice<kV, fdct_grey_frame_kernel<true, kV>>(c, s, image, blocks, g, qp, qp.q);
            return launch_choice<kV, fdct_grey_frame_kernel<false, kV>>(c, s, image, blocks, g, qp, qp.q);
        });
    });
}

}  // namespace hpdct
