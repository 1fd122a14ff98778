// kernels_cols_fwd.inc -- the forward-column kernel (fast_cols_fwd.hpp).
// Included by kernels_cols_fwd_g<G>.hip with FC_TU_GROUP = G: defines group G's entry points (kernels.hpp) over that group of column
// configurations.
#include "kernels_common.hpp"

namespace fc {
namespace {

template <class Cfg, int NZ2>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_cols_fwd(FastColsFwdArgs a) {
    DevPhaseCtx<ColFwdState> ctx;
    fast_cols_fwd_body<Cfg, NZ2>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)gridDim.x);
}

// Image columns and kernel columns in ONE launch: the two passes are independent (the kernels' h-transform is the
// only image-independent part of a convolve) and each is a small launch of its own at small problem sizes -- cfg1: 16 + 2
// tiles, cfg2: 64 + 64 -- where a kernel boundary (~1.5 us + ramp) is a visible part of the step.  A workgroup first takes
// its share of the image tiles, then of the kernel tiles, the second share rotated by the number of image tiles so that
// workgroups without an image tile start on the kernels at once.
template <class Cfg, int NZ2B>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_cols_fwd_pair(FastColsFwdArgs a, FastColsFwdArgs b) {
    DevPhaseCtx<ColFwdState> ctx;
    const int wg = (int)blockIdx.x, nwg = (int)gridDim.x;
    fast_cols_fwd_body<Cfg, Cfg::R2>(ctx, reinterpret_cast<c32*>(fc_smem), a, wg, nwg);
    const int wgb = (int)(((unsigned)wg + (unsigned)nwg - (unsigned)(a.ntiles % nwg)) % (unsigned)nwg);
    fast_cols_fwd_body<Cfg, NZ2B>(ctx, reinterpret_cast<c32*>(fc_smem), b, wgb, nwg);
}

struct FastColsFwdPairLauncher {
    const FastColsFwdArgs& a;
    const FastColsFwdArgs& b;
    int num_cus;
    hipStream_t s;
    hipError_t err = hipSuccess;
    template <class Cfg, int NZ2B>
    void go() {
        const size_t lds = (size_t)Cfg::LDS_ELEMS * sizeof(c32);
        if (!fast_cols_fwd_pair_queues_ok(a, b)) { err = hipErrorInvalidValue; return; }
        err = launch_lds<k_fast_cols_fwd_pair<Cfg, NZ2B>>(dim3(persistent_grid(lds, Cfg::NT, num_cus, a.ntiles + b.ntiles)), Cfg::NT, lds, s, a, b);
    }
};

struct FastColsFwdLauncher {
    const FastColsFwdArgs& a;
    int num_cus;
    hipStream_t s;
    hipError_t err = hipSuccess;
    template <class Cfg, int NZ2>
    void go() {
        const size_t lds = (size_t)Cfg::LDS_ELEMS * sizeof(c32);
        err = launch_lds<k_fast_cols_fwd<Cfg, NZ2>>(dim3(persistent_grid(lds, Cfg::NT, num_cus, a.ntiles)), Cfg::NT, lds, s, a);
    }
};

}  // namespace

template <>
GroupResult launch_fast_cols_fwd_group<FC_TU_GROUP>(int M, int T, bool pruned, const FastColsFwdArgs& a, int num_cus, hipStream_t s) {
    FastColsFwdLauncher l{a, num_cus, s};
    if (!fast_cols_fwd_dispatch_group<FC_TU_GROUP>(M, T, pruned, l)) return {};
    return l.err;
}

template <>
GroupResult launch_fast_cols_fwd_pair_group<FC_TU_GROUP>(int M, int T, const FastColsFwdArgs& image, const FastColsFwdArgs& kernels,
                                                        bool kernels_pruned, int num_cus, hipStream_t s) {
    FastColsFwdPairLauncher l{image, kernels, num_cus, s};
    if (!fast_cols_fwd_dispatch_group<FC_TU_GROUP>(M, T, kernels_pruned, l)) return {};
    return l.err;
}

}  // namespace fc
