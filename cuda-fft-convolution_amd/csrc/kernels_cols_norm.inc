// kernels_cols_norm.inc -- the output-column kernel with the fused scale of normalised maps (fast_cols.hpp: NORM; plan entry
// fftconv_plan_set_normalisation): the rectangle family in fp32 whose value pairs are multiplied by the scale plane D at their
// window coordinate ahead of the store.  Included by kernels_cols_norm_g<G>.hip with FC_TU_GROUP = G, as kernels_cols_rect.inc is:
// translation units of their own, so that every other kernel compiles exactly what it compiled before.  Two instantiations
// (static deal, dynamic tile queue) per configuration, named k_fast_cols_norm so that no report filter of the other families
// picks them up.  A plan without a rectangle launches them with the whole window as its rectangle.
#include "kernels_common.hpp"

namespace fc {
namespace {

template <class Cfg, bool DYN>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_cols_norm(FastColsArgs a, FastColsNormArgs n) {
    DevPhaseCtx<ColPairState<Cfg>> ctx;
    fast_cols_body<Cfg, true, false, DYN, false, true, true>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)gridDim.x, &n);
}

// `shape`: what fast_cols_norm_launch_shape decided (fast_paths.hpp): the rectangle launch in shape.a, the scale planes in shape.n
struct FastColsNormLauncher {
    const FastColsShape& sh;
    hipStream_t s;
    hipError_t err = hipSuccess;
    template <class Cfg>
    void go() {
        if constexpr (!fast_cols_norm_built(Cfg::M)) { err = hipErrorInvalidValue; return; }      // (fast_paths.hpp: not instantiated)
        else {
        const size_t lds = (size_t)Cfg::LDS_ELEMS * sizeof(c32);
        if (sh.variant == FastColsVariant::TILED_DYN) err = launch_lds<k_fast_cols_norm<Cfg, true>>(dim3(sh.grid), Cfg::NT, lds, s, sh.a, sh.n);
        else err = launch_lds<k_fast_cols_norm<Cfg, false>>(dim3(sh.grid), Cfg::NT, lds, s, sh.a, sh.n);
        }
    }
};

}  // namespace

template <>
GroupResult launch_fast_cols_norm_group<FC_TU_GROUP>(int M, int T, const FastColsShape& shape, hipStream_t s) {
    FastColsNormLauncher l{shape, s};
    if (!fast_cols_dispatch_group<FC_TU_GROUP>(M, T, l)) return {};
    return l.err;
}

}  // namespace fc
