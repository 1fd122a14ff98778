// kernels_cols_fwd_px.inc -- the forward-column kernel of an image of typed pixels (fast_cols_fwd.hpp: Px; pixel_format.hpp; plan
// entry fftconv_plan_set_images_typed): uint8 / uint16 / fp16 / bf16 elements converted in the load, image only -- the full
// variant (NZ2 = R2), static deal and dynamic tile queue as the fp32 kernel (a.queue).  Included by kernels_cols_fwd_px_g<G>.hip
// with FC_TU_GROUP = G: translation units of their own, so that every other kernel compiles exactly what it compiled before.
// One instantiation per (configuration, element size): which of the 16-bit formats the elements are is a uniform of the launch
// (PixelLoad::format), as the fp16 / bf16 choice of k_fast_cols16 is.
#include "kernels_common.hpp"

namespace fc {
namespace {

template <class Cfg, class Px>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_cols_fwd_px(FastColsFwdArgs a, PixelLoad px) {
    DevPhaseCtx<ColFwdState> ctx;
    fast_cols_fwd_body<Cfg, Cfg::R2, Px>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)gridDim.x, px);
}

struct FastColsFwdPxLauncher {
    const FastColsFwdArgs& a;
    PixelLoad px;
    int num_cus;
    hipStream_t s;
    hipError_t err = hipSuccess;
    template <class Cfg>
    void go() {
        if constexpr (!fast_cols_fwd_px_built(Cfg::M)) { err = hipErrorInvalidValue; return; }      // (fast_paths.hpp: not instantiated)
        else {
        const size_t lds = (size_t)Cfg::LDS_ELEMS * sizeof(c32);
        const dim3 grid(persistent_grid(lds, Cfg::NT, num_cus, a.ntiles));
        if (fc_pixel_elem_bytes(px.format) == 1) err = launch_lds<k_fast_cols_fwd_px<Cfg, Pixel8>>(grid, Cfg::NT, lds, s, a, px);
        else err = launch_lds<k_fast_cols_fwd_px<Cfg, Pixel16>>(grid, Cfg::NT, lds, s, a, px);
        }
    }
};

}  // namespace

template <>
GroupResult launch_fast_cols_fwd_px_group<FC_TU_GROUP>(int M, int T, const FastColsFwdArgs& a, const PixelLoad& px, int num_cus, hipStream_t s) {
    FastColsFwdPxLauncher l{a, px, num_cus, s};
    if (!fast_cols_dispatch_group<FC_TU_GROUP>(M, T, l)) return {};
    return l.err;
}

}  // namespace fc
