// kernels_rows_filter.inc -- the multi-map spectral-row kernel with a spectral filter in its product phase (fast_rows_multi.hpp:
// FILTER; spectral_filter.hpp; fftconv_plan_set_spectral_filter).  F = 1, the walk over kernels.
// Included by kernels_rows_filter_g<G>.hip with FC_TU_GROUP = G: each translation unit instantiates the row configurations of one
// group of fast_paths.hpp -- one kernel per (length, NZ2) of the lengths that are built (fast_rows_filter_built), serving every
// mode -- and defines that group's entry point.  A kernel of its own name: the plain kernels of kernels_rows_multi.inc come out of
// the build as they were.
#include "kernels_common.hpp"

namespace fc {
namespace {

// (the grid and the image coordinate: as k_fast_rows_multi)
template <class Cfg, int NZ2>
__global__ void __launch_bounds__(Cfg::NT, fast_rows_filter_min_waves(Cfg::L)) k_fast_rows_filter(FastRowsArgs a, int rows, int kernels, int per_wg) {
    const RowsWalk w = rows_walk_3d((int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z, kernels, per_wg);
    rows_shift_to_image(a.S, a.Y, w.image, a.s_image_stride, kernels, a.y_kernel_stride);
    DevPhaseCtx<RowMultiState<Cfg, false, true>> ctx;
    fast_rows_multi_body<Cfg, NZ2, true, false, true>(ctx, reinterpret_cast<c32*>(fc_smem), a, w.group, w.kernel0, w.nk, rows);
}

struct FastRowsFilterLauncher {
    const FastRowsArgs& a;
    int rows, kernels, per_wg;
    hipStream_t s;
    hipError_t err = hipSuccess;
    template <class Cfg, int NZ2>
    void go() {
        if constexpr (fast_rows_filter_built(Cfg::L)) {
            const FastRowsGrid g = fast_rows_grid(rows, Cfg::RPW, kernels, per_wg);
            err = launch_lds<k_fast_rows_filter<Cfg, NZ2>>(dim3(g.groups, g.walks, rows_images(a.images)), Cfg::NT, (size_t)Cfg::LDS_ELEMS * sizeof(c32), s, a,
                                                           rows, kernels, per_wg);
        } else {
            err = hipErrorInvalidValue;      // not built: the plan never asks (fftconv_plan_set_spectral_filter refuses the mode)
        }
    }
};

}  // namespace

template <>
GroupResult launch_fast_rows_filter_group<FC_TU_GROUP>(int L, int nz2, const FastRowsArgs& a, int rows, int kernels, int kernels_per_wg, hipStream_t s) {
    FastRowsFilterLauncher l{a, rows, kernels, kernels_per_wg, s};
    if (!fast_rows_dispatch_group<FC_TU_GROUP>(L, nz2, l)) return {};
    return l.err;
}

}  // namespace fc
