// hpdct_grey_frame_inv.hip -- launcher of the grey frame inverse kernels
// (hpdct_grey_frame.hpp).
#include "hpdct_grey_frame.hpp"
#include "hpdct_launch.hpp"

namespace hpdct {

hipError_t launch_idct_grey_frame(const int16_t* blocks, uint8_t* image, const GreyGrid& g, const Mat64& q,
                                  bool natural, bool full_chain, hipStream_t s) {
    policy::GreyCall pc;
    pc.tiles = g.ntiles, pc.clip = !grey_whole_aligned(image, g), pc.full_chain = full_chain;
    const policy::Choice c = policy::inverse_grey(pc);
    if (c.family != policy::Family::kGrey) return hipErrorInvalidDeviceFunction;
    if ((c.var & kVarFullChain) != 0u) {  // the general instantiation only
        constexpr unsigned kV = policy::kInvFullVar | kGreyClip;
        if (natural) return launch_choice<kV, idct_grey_frame_kernel<true, kV>>(c, s, blocks, image, g, q);
        return launch_choice<kV, idct_grey_frame_kernel<false, kV>>(c, s, blocks, image, g, q);
    }
    return policy::with_bit<kGreyClip, true>(c.var, [&](auto kC) {
        constexpr unsigned kV = policy::kGreyInvVar | decltype(kC)::value;
        if (natural) return launch_choice<kV, idct_grey_frame_kernel<true, kV>>(c, s, blocks, image, g, q);
        return launch_choice<kV, idct_grey_frame_kernel<false, kV>>(c, s, blocks, image, g, q);
    });
}

}  // namespace hpdct
