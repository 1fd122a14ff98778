// kernels_cols_fwd_border.inc -- the forward-column kernel of an image with a border (fast_cols_fwd.hpp: Bd; border.hpp; plan
// entry fftconv_plan_set_border): the indices of the extended image mapped in the load, image only -- fp32 pixels, the full
// variant (NZ2 = R2), static deal and dynamic tile queue as the plain kernel (a.queue).  Included by
// kernels_cols_fwd_border_g<G>.hip with FC_TU_GROUP = G: translation units of their own, so that every other kernel compiles
// exactly what it compiled before.  One instantiation per configuration: the mode is a uniform of the launch (BorderLoad).
#include "kernels_common.hpp"

namespace fc {
namespace {

template <class Cfg>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_cols_fwd_border(FastColsFwdArgs a, BorderLoad bd) {
    DevPhaseCtx<ColFwdState> ctx;
    fast_cols_fwd_body<Cfg, Cfg::R2, float, Bordered>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)gridDim.x, PixelLoad{}, bd);
}

struct FastColsFwdBorderLauncher {
    const FastColsFwdArgs& a;
    BorderLoad bd;
    int num_cus;
    hipStream_t s;
    hipError_t err = hipSuccess;
    template <class Cfg>
    void go() {
        if constexpr (!fast_cols_fwd_border_built(Cfg::M)) { err = hipErrorInvalidValue; return; }      // (fast_paths.hpp: not instantiated)
        else {
        const size_t lds = (size_t)Cfg::LDS_ELEMS * sizeof(c32);
        const dim3 grid(persistent_grid(lds, Cfg::NT, num_cus, a.ntiles));
        err = launch_lds<k_fast_cols_fwd_border<Cfg>>(grid, Cfg::NT, lds, s, a, bd);
        }
    }
};

}  // namespace

template <>
GroupResult launch_fast_cols_fwd_border_group<FC_TU_GROUP>(int M, int T, const FastColsFwdArgs& a, const BorderLoad& bd, int num_cus, hipStream_t s) {
    FastColsFwdBorderLauncher l{a, bd, num_cus, s};
    if (!fast_cols_dispatch_group<FC_TU_GROUP>(M, T, l)) return {};
    return l.err;
}

}  // namespace fc
