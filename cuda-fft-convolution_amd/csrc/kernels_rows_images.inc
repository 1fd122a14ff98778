// kernels_rows_images.inc -- the image-walk spectral-row kernel (fast_rows_images.hpp; plan option "image_walk").
// Included by kernels_rows_images_g<G>.hip with FC_TU_GROUP = G: each translation unit instantiates the row lengths of one
// group of fast_paths.hpp -- one kernel per length that is built (fast_rows_images_built) -- and defines that group's entry point.
#include "kernels_common.hpp"

namespace fc {
namespace {

// (`a`: the arguments of the LAUNCH -- a.images spectra from a.S on, a.kernels_per_image kernels; the block's kernel and images are
//  scalar arithmetic on blockIdx.x, fast_paths.hpp: rows_walk_images)
template <class Cfg>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_rows_images(FastRowsArgs a, int rows, int groups, int iwalks, int per_wg) {
    const RowsImageWalk w = rows_walk_images((int)blockIdx.x, groups, a.kernels_per_image, iwalks, a.images, per_wg);
    if (w.group >= groups) return;
    DevPhaseCtx<RowImagesState<Cfg>> ctx;
    fast_rows_images_body<Cfg>(ctx, reinterpret_cast<c32*>(fc_smem), a, w.group, w.kernel, w.image0, w.ni, rows);
}

struct FastRowsImagesLauncher {
    const FastRowsArgs& a;
    int rows, per_wg;
    hipStream_t s;
    hipError_t err = hipSuccess;
    template <class Cfg>
    void go() {
        if constexpr (fast_rows_images_built(Cfg::L)) {
            const int groups = fast_rows_grid(rows, Cfg::RPW, 1, 1).groups, iwalks = rows_image_walks(a.images, per_wg);
            err = launch_lds<k_fast_rows_images<Cfg>>(dim3(rows_images_grid(groups, a.kernels_per_image, iwalks)), Cfg::NT,
                                                      (size_t)Cfg::LDS_ELEMS * sizeof(c32), s, a, rows, groups, iwalks, per_wg);
        } else {
            err = hipErrorInvalidValue;      // not built: the plan never asks (fast_rows_images_available)
        }
    }
};

}  // namespace

template <>
GroupResult launch_fast_rows_images_group<FC_TU_GROUP>(int L, const FastRowsArgs& a, int rows, int images_per_wg, hipStream_t s) {
    FastRowsImagesLauncher l{a, rows, images_per_wg, s};
    if (!fast_rows_fwd_dispatch_group<FC_TU_GROUP>(L, l)) return {};
    return l.err;
}

}  // namespace fc
