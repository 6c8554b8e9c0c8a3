// hpdct_blocks_inv.hip -- launcher of the int16 block inverse kernels
// (hpdct_blocks.hpp).
#include "hpdct_blocks.hpp"
#include "hpdct_launch.hpp"

namespace hpdct {

namespace {
template <typename TOut>
hipError_t launch_idct_blocks_as(const int16_t* blocks, TOut* out, const TileGrid& g, const Mat64& q, bool natural,
                                 bool full_chain, hipStream_t s) {
    policy::Call pc;
    pc.g = g, pc.out = kElem<TOut>, pc.cus = device_cus(), pc.full_chain = full_chain;
    const policy::Choice c = policy::inverse_blocks(pc);
    if (c.family != policy::Family::kBlocks) return hipErrorInvalidDeviceFunction;
    if ((c.var & kVarFullChain) != 0u) {
        constexpr unsigned kV = policy::kInvFullVar;
        if (natural) return launch_choice<kV, idct_blocks_kernel<TOut, true, kV>>(c, s, blocks, out, g, q);
        return launch_choice<kV, idct_blocks_kernel<TOut, false, kV>>(c, s, blocks, out, g, q);
    }
    return policy::with_bit<kVarStraddle, std::is_same_v<TOut, float>>(c.var, [&](auto kS) {
        constexpr unsigned kV = policy::blocks_inv_var(kElem<TOut>) | decltype(kS)::value;
        if (natural) return launch_choice<kV, idct_blocks_kernel<TOut, true, kV>>(c, s, blocks, out, g, q);
        return launch_choice<kV, idct_blocks_kernel<TOut, false, kV>>(c, s, blocks, out, g, q);
    });
}
}  // namespace

hipError_t launch_idct_blocks(const int16_t* blocks, void* out, bool out_f32, const TileGrid& g, const Mat64& q,
                              bool natural, bool full_chain, hipStream_t s) {
    if (out_f32) return launch_idct_blocks_as(blocks, static_cast<float*>(out), g, q, natural, full_chain, s);
    return launch_idct_blocks_as(blocks, static_cast<uint8_t*>(out), g, q, natural, full_chain, s);
}

}  // namespace hpdct
