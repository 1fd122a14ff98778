// kernels_common.hpp -- device-side glue shared by the kernels_*_g<G>.hip translation units: the phase
// context that binds the workgroup bodies to HIP threads and barriers, the dynamic-LDS symbol and
// the one launch helper (per-device LDS attribute, launch, error).  (One translation unit per kernel family and
// group of configurations: they compile in parallel, and which kernels share a unit is part of how they compile --
// kernels_rows_multi.inc -- so the cut is not to be moved lightly.)
#pragma once
#include <atomic>
#include <type_traits>

#include "kernels.hpp"

namespace fc {
namespace {

extern __shared__ __attribute__((aligned(16))) unsigned char fc_smem[];

// Raises the dynamic-LDS limit of a kernel once per device (the attribute is per device; a
// process may drive several GPUs through different plans): one mask per kernel instantiation, shared by
// every launcher and query of that kernel.
// (the per-device threads of fftconv_multi_convolve come through here at the same time: the mask is atomic)
template <auto Kernel>
hipError_t ensure_lds_attr() {
    static std::atomic<unsigned long long> done_mask{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (done_mask.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) done_mask.fetch_or(bit, std::memory_order_release);
    return e;
}
// the launch of a kernel with `lds` bytes of dynamic LDS on `nt` threads per workgroup
template <auto Kernel, class... Args>
hipError_t launch_lds(dim3 grid, int nt, size_t lds, hipStream_t s, Args... a) {
    const hipError_t e = ensure_lds_attr<Kernel>();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(Kernel, grid, dim3(nt), lds, s, a...);
    return hipGetLastError();
}

template <class State>
struct DevPhaseCtx {
    State st;
    template <class F>
    __device__ __forceinline__ void phase(F&& f) {
        f((int)threadIdx.x, st);
        __syncthreads();
    }
    template <class F>
    __device__ __forceinline__ void phase_nosync(F&& f) {
        f((int)threadIdx.x, st);
    }
    template <bool NOSYNC, class F>
    __device__ __forceinline__ void phase_dbg(F&& f) {
        f((int)threadIdx.x, st);
        if (!NOSYNC) __syncthreads();
    }
};

}  // namespace
}  // namespace fc
