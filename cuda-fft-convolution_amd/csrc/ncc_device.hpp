// ncc_device.hpp -- device helpers shared by the units of the matching scores (kernels_ncc.hip, kernels_score.hip)
#pragma once
#include "kernels.hpp"
#include "ncc.hpp"

namespace fc {
namespace {

// the fold of ncc.hpp's lanes in LDS, a barrier per step: every thread of the workgroup returns the sum
__device__ __forceinline__ double fold_lanes(double* part, int t, double mine) {
    part[t] = mine;
    __syncthreads();
    for (int s = FC_NCC_LANES / 2; s > 0; s >>= 1) {
        if (t < s) part[t] += part[t + s];
        __syncthreads();
    }
    const double r = part[0];
    __syncthreads();
    return r;
}
template <bool OUT16>
FC_D void put(std::conditional_t<OUT16, uint16_t, float>* d, float x, [[maybe_unused]] int bf16) {
    if constexpr (OUT16) {
        // a 16-bit map is the ROUNDED fp32 product: behind this the compiler cannot merge the multiply and the conversion into one
        // mixed-precision instruction that rounds the exact product once
        asm volatile("" : "+v"(x));
        *d = fc_map16(x, bf16 != 0);
    } else *d = x;
}

}  // namespace
}  // namespace fc
