// hpdct_dct_grey_inv.hip -- the grey frame inverse kernels under HPDCT_FRAME_DCT
// (hpdct_grey_frame.hpp with kFrameDct): the exact DCT's matrix, every term,
// pixels rounded (R + 128.5f, clamp, truncate); with and without kGreyClip, for
// every table.
#include "hpdct_grey_frame.hpp"
#include "hpdct_launch.hpp"

namespace hpdct {

hipError_t launch_idct_grey_frame_dct(const int16_t* blocks, uint8_t* image, const GreyGrid& g, const Mat64& q,
                                      bool natural, hipStream_t s) {
    policy::GreyCall pc;
    pc.tiles = g.ntiles, pc.clip = !grey_whole_aligned(image, g), pc.dct = true;
    const policy::Choice c = policy::inverse_grey(pc);
    if (c.family != policy::Family::kGrey) return hipErrorInvalidDeviceFunction;
    return policy::with_bit<kGreyClip, true>(c.var, [&](auto kC) {
        constexpr unsigned kV = policy::kGreyInvDctVar | decltype(kC)::value;
        if (natural) return launch_choice<kV, idct_grey_frame_kernel<true, kV>>(c, s, blocks, image, g, q);
        return launch_choice<kV, idct_grey_frame_kernel<false, kV>>(c, s, blocks, image, g, q);
    });
}

}  // namespace hpdct
