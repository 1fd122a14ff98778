// kernels_cols_sqdiff.inc -- the output-column kernel with the fused additive store of matching score 4, SQDIFF (fast_cols.hpp: ADD;
// plan entry fftconv_plan_set_match_score): the rectangle family in fp32 whose value pairs become v + (Q + c) -- the plane Q at their
// window coordinate, c the constant of the map's kernel -- ahead of the store.  Included by kernels_cols_sqdiff_g<G>.hip with
// FC_TU_GROUP = G, as kernels_cols_norm.inc is: translation units of their own, so that every other kernel compiles exactly what it
// compiled before.  Two instantiations (static deal, dynamic tile queue) per configuration, named k_fast_cols_sqdiff so that no
// report filter of the other families picks them up.  A plan without a rectangle launches them with the whole window as its rectangle.
#include "kernels_common.hpp"

namespace fc {
namespace {

template <class Cfg, bool DYN>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_cols_sqdiff(FastColsArgs a, FastColsSqdiffArgs q) {
    DevPhaseCtx<ColPairState<Cfg>> ctx;
    fast_cols_body<Cfg, true, false, DYN, false, true, false, true>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)gridDim.x, nullptr, &q);
}

// `shape`: what fast_cols_sqdiff_launch_shape decided (fast_paths.hpp): the rectangle launch in shape.a, planes and constants in shape.q
struct FastColsSqdiffLauncher {
    const FastColsShape& sh;
    hipStream_t s;
    hipError_t err = hipSuccess;
    template <class Cfg>
    void go() {
        if constexpr (!fast_cols_sqdiff_built(Cfg::M)) { err = hipErrorInvalidValue; return; }      // (fast_paths.hpp: not instantiated)
        else {
        const size_t lds = (size_t)Cfg::LDS_ELEMS * sizeof(c32);
        if (sh.variant == FastColsVariant::TILED_DYN) err = launch_lds<k_fast_cols_sqdiff<Cfg, true>>(dim3(sh.grid), Cfg::NT, lds, s, sh.a, sh.q);
        else err = launch_lds<k_fast_cols_sqdiff<Cfg, false>>(dim3(sh.grid), Cfg::NT, lds, s, sh.a, sh.q);
        }
    }
};

}  // namespace

template <>
GroupResult launch_fast_cols_sqdiff_group<FC_TU_GROUP>(int M, int T, const FastColsShape& shape, hipStream_t s) {
    FastColsSqdiffLauncher l{shape, s};
    if (!fast_cols_dispatch_group<FC_TU_GROUP>(M, T, l)) return {};
    return l.err;
}

}  // namespace fc
