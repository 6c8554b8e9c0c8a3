// hpdct_inv.hip -- inverse kernels, fp32 coefficients in (int8 in: hpdct_inv_i8.hip).  Kernels: hpdct_kernels_impl.hpp.
#include "hpdct_launch.hpp"

namespace hpdct {
#define HPDCT_INV(TI, TO, DQ, BT)                                                                          \
    template <>                                                                                             \
    hipError_t launch_idct<TI, TO, DQ, BT>(const TI* a, TO* b, float* w, const TileGrid& g, const float* t,  \
                                           const Mat64& q, float sh, bool rf, bool fc, hipStream_t s) {     \
        return launch_idct_impl<TI, TO, DQ, BT>(a, b, w, g, t, q, sh, rf, fc, s);                           \
    }
#define HPDCT_INV_T(TI, TO, DQ) HPDCT_INV(TI, TO, DQ, true) HPDCT_INV(TI, TO, DQ, false)
HPDCT_INV_T(float, float, true)
HPDCT_INV_T(float, float, false)
HPDCT_INV_T(float, uint8_t, true)
HPDCT_INV_T(float, uint8_t, false)
}  // namespace hpdct
