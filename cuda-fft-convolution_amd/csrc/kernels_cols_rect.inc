// kernels_cols_rect.inc -- the output-column kernel with the rectangle store (fast_cols.hpp: RECT; plan entry
// fftconv_plan_set_output_rect): the maps are a dense rectangle of the window, written by the output kernel itself.
// Included by kernels_cols_rect_g<G>.hip (fp32 maps: k_fast_cols_rect) and kernels_cols_rect16_g<G>.hip (FC_TU_OUT16 = 1: 16-bit
// maps, k_fast_cols_rect16) with FC_TU_GROUP = G, as kernels_cols.inc is: translation units of their own, so that the
// plain kernels compile exactly what they compiled before.  Tiled intermediate and unsliced launches only: two
// instantiations (static deal, dynamic tile queue) per configuration and element class.
#include "kernels_common.hpp"

#ifndef FC_TU_OUT16
#define FC_TU_OUT16 0
#endif

namespace fc {
namespace {

#if FC_TU_OUT16
#define FC_K_FAST_COLS_RECT k_fast_cols_rect16
#define FC_LAUNCH_FAST_COLS_RECT_GROUP launch_fast_cols_rect16_group
template <class Cfg, bool DYN>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_cols_rect16(FastColsArgs a) {
    DevPhaseCtx<ColPairState<Cfg>> ctx;
    fast_cols_body<Cfg, true, false, DYN, true, true>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)gridDim.x);
}
#else
#define FC_K_FAST_COLS_RECT k_fast_cols_rect
#define FC_LAUNCH_FAST_COLS_RECT_GROUP launch_fast_cols_rect_group
template <class Cfg, bool DYN>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_cols_rect(FastColsArgs a) {
    DevPhaseCtx<ColPairState<Cfg>> ctx;
    fast_cols_body<Cfg, true, false, DYN, false, true>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)gridDim.x);
}
#endif

// `shape`: what fast_cols_rect_launch_shape decided (the caller's: it knows the rectangle)
struct FastColsRectLauncher {
    const FastColsShape& sh;
    hipStream_t s;
    hipError_t err = hipSuccess;
    template <class Cfg>
    void go() {
        if constexpr (!fast_cols_rect_built(Cfg::M)) { err = hipErrorInvalidValue; return; }      // (fast_paths.hpp: not instantiated)
        else {
        const size_t lds = (size_t)Cfg::LDS_ELEMS * sizeof(c32);
        if (sh.variant == FastColsVariant::TILED_DYN) err = launch_lds<FC_K_FAST_COLS_RECT<Cfg, true>>(dim3(sh.grid), Cfg::NT, lds, s, sh.a);
        else err = launch_lds<FC_K_FAST_COLS_RECT<Cfg, false>>(dim3(sh.grid), Cfg::NT, lds, s, sh.a);
        }
    }
};

}  // namespace

template <>
GroupResult FC_LAUNCH_FAST_COLS_RECT_GROUP<FC_TU_GROUP>(int M, int T, const FastColsShape& shape, hipStream_t s) {
    FastColsRectLauncher l{shape, s};
    if (!fast_cols_dispatch_group<FC_TU_GROUP>(M, T, l)) return {};
    return l.err;
}

}  // namespace fc
