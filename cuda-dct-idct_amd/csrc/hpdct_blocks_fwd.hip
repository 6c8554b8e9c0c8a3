// hpdct_blocks_fwd.hip -- launcher of the int16 block forward kernels
// (hpdct_blocks.hpp; the inverse is in hpdct_blocks_inv.hip so the two compile
// in parallel).
#include "hpdct_blocks.hpp"
#include "hpdct_launch.hpp"

namespace hpdct {

hipError_t launch_fdct_blocks(const uint8_t* img, int16_t* blocks, const TileGrid& g, const QParams& qp, int qmode,
                              bool natural, hipStream_t s) {
    policy::Call pc;
    pc.g = g, pc.qmode = qmode, pc.cus = device_cus();
    const policy::Choice c = policy::forward_blocks(pc);
    if (c.family != policy::Family::kBlocks) return hipErrorInvalidDeviceFunction;
    return policy::with_quotient<true>(c.var, [&](auto kQ) {
        constexpr unsigned kV = policy::kBlocksFwdVar | decltype(kQ)::value;
        if (natural) return launch_choice<kV, fdct_blocks_kernel<true, kV>>(c, s, img, blocks, g, qp);
        return launch_choice<kV, fdct_blocks_kernel<false, kV>>(c, s, img, blocks, g, qp);
    });
}

}  // namespace hpdct
