// kernels_cols_rect.inc -- the rectangle family of the output-column kernel (fast_cols.hpp: the RECT stores; plan entry
// fftconv_plan_set_output_rect): the maps are a dense rectangle of the window, written by the output kernel itself.  Included with
// FC_TU_GROUP = G, as kernels_cols.inc is, by five kinds of translation unit, one kernel each:
//   kernels_cols_rect_g<G>.hip                       k_fast_cols_rect     fp32 maps
//   kernels_cols_rect16_g<G>.hip    FC_TU_OUT16 = 1  k_fast_cols_rect16   16-bit maps
//   kernels_cols_norm_g<G>.hip      FC_TU_NORM = 1   k_fast_cols_norm     fp32 maps times the scale plane of normalised maps (NORM;
//                                                                         fftconv_plan_set_normalisation, scores 1 and 3)
//   kernels_cols_sqdiff_g<G>.hip    FC_TU_SQDIFF = 1 k_fast_cols_sqdiff   fp32 maps plus Q + c of matching score 4 (ADD;
//                                                                         fftconv_plan_set_match_score)
//   kernels_cols_stride_g<G>.hip    FC_TU_STRIDE = 1 k_fast_cols_stride   fp32 maps, every sh-th row and sw-th column (STRIDE;
//                                                                         fftconv_plan_set_output_stride)
// With FC_TU_EXTREMA = 1 beside none of the others, FC_TU_NORM or FC_TU_SQDIFF: the same three fp32 stores with the per-map extrema found
// in the store (EXT; fftconv_plan_set_extrema), under names of their own again --
//   kernels_cols_ext_g<G>.hip         k_fast_cols_rect_ext     kernels_cols_norm_ext_g<G>.hip    k_fast_cols_norm_ext
//   kernels_cols_sqdiff_ext_g<G>.hip  k_fast_cols_sqdiff_ext
// Translation units of their own, so that every other kernel compiles exactly what it compiled before, and kernel names of their
// own, so that no report filter of one family picks up another.  Tiled intermediate and unsliced launches only: two instantiations
// (static deal, dynamic tile queue) per configuration and kernel.  A plan without a rectangle launches the NORM / ADD kernels with
// the whole window as its rectangle.
#include "kernels_common.hpp"

#ifndef FC_TU_OUT16
#define FC_TU_OUT16 0
#endif
#ifndef FC_TU_NORM
#define FC_TU_NORM 0
#endif
#ifndef FC_TU_SQDIFF
#define FC_TU_SQDIFF 0
#endif
#ifndef FC_TU_STRIDE
#define FC_TU_STRIDE 0
#endif
#ifndef FC_TU_EXTREMA
#define FC_TU_EXTREMA 0
#endif

namespace fc {
namespace {

// FC_RECT_KERNEL: the unit's kernel; FC_RECT_GROUP / FC_RECT_BUILT: its group entry (kernels.hpp) and its list of built configurations
// (fast_paths.hpp); FC_RECT_ARGS(sh): the kernel's arguments from the launch shape -- the plane's device struct is filled here
#if FC_TU_EXTREMA && FC_TU_SQDIFF
#define FC_RECT_KERNEL k_fast_cols_sqdiff_ext
#define FC_RECT_GROUP launch_fast_cols_rect_add_ext_group
#define FC_RECT_BUILT fast_cols_sqdiff_ext_built
#define FC_RECT_ARGS(sh) (sh).a, fast_cols_sqdiff_args((sh).plane), (sh).extrema
template <class Cfg, bool DYN>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_cols_sqdiff_ext(FastColsArgs a, FastColsSqdiffArgs q, FastColsExtremaArgs x) {
    DevPhaseCtx<ColPairState<Cfg>> ctx;
    fast_cols_body<Cfg, true, false, DYN, ColStore::RECT_ADD, true>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)gridDim.x, q, x);
}
#elif FC_TU_EXTREMA && FC_TU_NORM
#define FC_RECT_KERNEL k_fast_cols_norm_ext
#define FC_RECT_GROUP launch_fast_cols_rect_scale_ext_group
#define FC_RECT_BUILT fast_cols_norm_ext_built
#define FC_RECT_ARGS(sh) (sh).a, fast_cols_norm_args((sh).plane), (sh).extrema
template <class Cfg, bool DYN>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_cols_norm_ext(FastColsArgs a, FastColsNormArgs n, FastColsExtremaArgs x) {
    DevPhaseCtx<ColPairState<Cfg>> ctx;
    fast_cols_body<Cfg, true, false, DYN, ColStore::RECT_SCALE, true>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)gridDim.x, n, x);
}
#elif FC_TU_EXTREMA
#define FC_RECT_KERNEL k_fast_cols_rect_ext
#define FC_RECT_GROUP launch_fast_cols_rect_ext_group
#define FC_RECT_BUILT fast_cols_rect_ext_built
#define FC_RECT_ARGS(sh) (sh).a, (sh).extrema
template <class Cfg, bool DYN>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_cols_rect_ext(FastColsArgs a, FastColsExtremaArgs x) {
    DevPhaseCtx<ColPairState<Cfg>> ctx;
    fast_cols_body<Cfg, true, false, DYN, ColStore::RECT, true>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)gridDim.x, x);
}
#elif FC_TU_STRIDE
#define FC_RECT_KERNEL k_fast_cols_stride
#define FC_RECT_GROUP launch_fast_cols_rect_stride_group
#define FC_RECT_BUILT fast_cols_stride_built
#define FC_RECT_ARGS(sh) (sh).a, (sh).stride
template <class Cfg, bool DYN>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_cols_stride(FastColsArgs a, FastColsStrideArgs st) {
    DevPhaseCtx<ColPairState<Cfg>> ctx;
    fast_cols_body<Cfg, true, false, DYN, ColStore::RECT_STRIDE>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)gridDim.x, st);
}
#elif FC_TU_SQDIFF
#define FC_RECT_KERNEL k_fast_cols_sqdiff
#define FC_RECT_GROUP launch_fast_cols_rect_add_group
#define FC_RECT_BUILT fast_cols_sqdiff_built
#define FC_RECT_ARGS(sh) (sh).a, fast_cols_sqdiff_args((sh).plane)
template <class Cfg, bool DYN>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_cols_sqdiff(FastColsArgs a, FastColsSqdiffArgs q) {
    DevPhaseCtx<ColPairState<Cfg>> ctx;
    fast_cols_body<Cfg, true, false, DYN, ColStore::RECT_ADD>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)gridDim.x, q);
}
#elif FC_TU_NORM
#define FC_RECT_KERNEL k_fast_cols_norm
#define FC_RECT_GROUP launch_fast_cols_rect_scale_group
#define FC_RECT_BUILT fast_cols_norm_built
#define FC_RECT_ARGS(sh) (sh).a, fast_cols_norm_args((sh).plane)
template <class Cfg, bool DYN>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_cols_norm(FastColsArgs a, FastColsNormArgs n) {
    DevPhaseCtx<ColPairState<Cfg>> ctx;
    fast_cols_body<Cfg, true, false, DYN, ColStore::RECT_SCALE>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)gridDim.x, n);
}
#elif FC_TU_OUT16
#define FC_RECT_KERNEL k_fast_cols_rect16
#define FC_RECT_GROUP launch_fast_cols_rect16_group
#define FC_RECT_BUILT fast_cols_rect_built
#define FC_RECT_ARGS(sh) (sh).a
template <class Cfg, bool DYN>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_cols_rect16(FastColsArgs a) {
    DevPhaseCtx<ColPairState<Cfg>> ctx;
    fast_cols_body<Cfg, true, false, DYN, ColStore::RECT16>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)gridDim.x);
}
#else
#define FC_RECT_KERNEL k_fast_cols_rect
#define FC_RECT_GROUP launch_fast_cols_rect_group
#define FC_RECT_BUILT fast_cols_rect_built
#define FC_RECT_ARGS(sh) (sh).a
template <class Cfg, bool DYN>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_cols_rect(FastColsArgs a) {
    DevPhaseCtx<ColPairState<Cfg>> ctx;
    fast_cols_body<Cfg, true, false, DYN, ColStore::RECT>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)gridDim.x);
}
#endif

// `shape`: what fast_cols_rect_launch_shape decided (the caller's: it knows the rectangle and the plane)
struct FastColsRectLauncher {
    const FastColsShape& sh;
    hipStream_t s;
    hipError_t err = hipSuccess;
    template <class Cfg>
    void go() {
        if constexpr (!FC_RECT_BUILT(Cfg::M)) { err = hipErrorInvalidValue; return; }      // (fast_paths.hpp: not instantiated)
        else {
        const size_t lds = (size_t)Cfg::LDS_ELEMS * sizeof(c32);
        if (sh.variant == FastColsVariant::TILED_DYN) err = launch_lds<FC_RECT_KERNEL<Cfg, true>>(dim3(sh.grid), Cfg::NT, lds, s, FC_RECT_ARGS(sh));
        else err = launch_lds<FC_RECT_KERNEL<Cfg, false>>(dim3(sh.grid), Cfg::NT, lds, s, FC_RECT_ARGS(sh));
        }
    }
};

}  // namespace

template <>
GroupResult FC_RECT_GROUP<FC_TU_GROUP>(int M, int T, const FastColsShape& shape, hipStream_t s) {
    FastColsRectLauncher l{shape, s};
    if (!fast_cols_dispatch_group<FC_TU_GROUP>(M, T, l)) return {};
    return l.err;
}

}  // namespace fc
