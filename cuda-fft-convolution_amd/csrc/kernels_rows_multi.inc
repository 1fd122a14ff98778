// kernels_rows_multi.inc -- the multi-map spectral-row kernel (fast_rows_multi.hpp), the default.
// Included by kernels_rows_multi_g<G>.hip with FC_TU_GROUP = G: each translation unit instantiates the row
// configurations of one group of fast_paths.hpp and defines that group's entry points (kernels.hpp).
#include "kernels_common.hpp"

namespace fc {
namespace {

template <class Cfg, int NZ2, bool LINEAR>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_rows_multi(FastRowsArgs a, int rows, int kernels, int per_wg) {
    // (`kernels`: the kernels per image of the launch; blockIdx.z: the image of a batch -- its spectrum and its slots of the
    //  intermediate are two scalar multiply-adds on the uniform bases, the body sees one image)
    const RowsWalk w = rows_walk_3d((int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z, kernels, per_wg);
    rows_shift_to_image(a.S, a.Y, w.image, a.s_image_stride, kernels, a.y_kernel_stride);
    DevPhaseCtx<RowMultiState<Cfg>> ctx;
    fast_rows_multi_body<Cfg, NZ2, LINEAR>(ctx, reinterpret_cast<c32*>(fc_smem), a, w.group, w.kernel0, w.nk, rows);
}

// (Keep the F > 1 kernels in THIS translation unit: compiled in one of their own -- tried for the build time --
// the same source comes out with 49 instead of 27 spilled registers at L = 4224 and the row kernel 20 % slower at
// F = 2 ... 8; hipcc -Rpass-analysis=kernel-resource-usage shows it, tools/f_scaling.py measures it.)
// F > 1: the walk over (map, feature) pairs.  XCD-aware 1-D grid as k_fast_rows' order 2: blocks b and b + 8
// share an XCD (round-robin dispatch; a speed assumption only), XCD x walks row groups x, x + 8, ... with the
// walk index fastest, so the workgroups that need the same F image-spectrum rows run side by side on one L2.
// Image batches: the walk index runs over (image, walk) pairs, the image the slower of the two (fast_paths.hpp: rows_walk_flat);
// `kernels` and `walks` count per image, a.images is the number of images of the launch.
template <class Cfg, int NZ2, bool LINEAR>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_rows_multi_f(FastRowsArgs a, int rows, int kernels, int per_wg, int groups, int walks) {
    const RowsWalk w = rows_walk_flat((int)blockIdx.x, groups, walks, a.images, kernels, per_wg);
    if (w.group >= groups) return;
    rows_shift_to_image(a.S, a.Y, w.image, a.s_image_stride, kernels, a.y_kernel_stride);
    DevPhaseCtx<RowMultiState<Cfg, true>> ctx;
    fast_rows_multi_body<Cfg, NZ2, LINEAR, true>(ctx, reinterpret_cast<c32*>(fc_smem), a, w.group, w.kernel0, w.nk, rows);
}

// resident workgroups per CU of the F = 1 multi-map kernel a launch with these arguments would use (the runtime's
// occupancy calculator: registers, LDS, waves)
struct FastRowsMultiOccupancy {
    const FastRowsArgs& a;
    int result = 0;
    hipError_t err = hipSuccess;
    template <class Cfg, int NZ2>
    void go() {
        fast_rows_visit_linear<Cfg>(a, [&](auto linear) {
            constexpr auto kernel = k_fast_rows_multi<Cfg, NZ2, linear.value>;
            err = ensure_lds_attr<kernel>();
            if (err != hipSuccess) return;
            err = hipOccupancyMaxActiveBlocksPerMultiprocessor(&result, reinterpret_cast<const void*>(kernel), Cfg::NT, (size_t)Cfg::LDS_ELEMS * sizeof(c32));
        });
    }
};

struct FastRowsMultiLauncher {
    const FastRowsArgs& a;
    int rows, kernels, per_wg;
    hipStream_t s;
    hipError_t err = hipSuccess;
    template <class Cfg, int NZ2>
    void go() {
        const size_t lds = (size_t)Cfg::LDS_ELEMS * sizeof(c32);
        const FastRowsGrid g = fast_rows_grid(rows, Cfg::RPW, kernels, per_wg);
        const int images = rows_images(a.images);      // (`kernels`: per image)
        fast_rows_visit_linear<Cfg>(a, [&](auto linear) {
            if (a.F > 1) err = launch_lds<k_fast_rows_multi_f<Cfg, NZ2, linear.value>>(dim3(g.flat * images), Cfg::NT, lds, s, a, rows, kernels, per_wg, g.groups, g.walks);
            else err = launch_lds<k_fast_rows_multi<Cfg, NZ2, linear.value>>(dim3(g.groups, g.walks, images), Cfg::NT, lds, s, a, rows, kernels, per_wg);
        });
    }
};

}  // namespace

template <>
GroupResult fast_rows_multi_wgs_per_cu_group<FC_TU_GROUP>(int L, int nz2, const FastRowsArgs& a, int* wgs_per_cu) {
    FastRowsMultiOccupancy q{a};
    if (!fast_rows_dispatch_group<FC_TU_GROUP>(L, nz2, q)) return {};
    if (q.err == hipSuccess && wgs_per_cu) *wgs_per_cu = q.result;
    return q.err;
}

template <>
GroupResult launch_fast_rows_multi_group<FC_TU_GROUP>(int L, int nz2, const FastRowsArgs& a, int rows, int kernels, int kernels_per_wg, hipStream_t s) {
    FastRowsMultiLauncher l{a, rows, kernels, kernels_per_wg, s};
    if (!fast_rows_dispatch_group<FC_TU_GROUP>(L, nz2, l)) return {};
    return l.err;
}

}  // namespace fc
