// kernels_cols.inc -- the output-column kernel (fast_cols.hpp).
// Included by kernels_cols_g<G>.hip with FC_TU_GROUP = G: defines group G's entry point (kernels.hpp) over that group of column
// configurations.
#include "kernels_common.hpp"

namespace fc {
namespace {

template <class Cfg, bool TILED, bool SLICED = false, bool DYN = false>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_cols(FastColsArgs a) {
    DevPhaseCtx<std::conditional_t<TILED, ColPairState<Cfg>, ColState<Cfg>>> ctx;
    fast_cols_body<Cfg, TILED, SLICED, DYN>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)gridDim.x);
}

struct FastColsLauncher {
    const FastColsArgs& a;
    int max_wg;
    hipStream_t s;
    hipError_t err = hipSuccess;
    template <class Cfg>
    void go() {
        const size_t lds = (size_t)Cfg::LDS_ELEMS * sizeof(c32);
        const FastColsShape sh = fast_cols_launch_shape(Cfg::M, Cfg::T, a, persistent_want(lds, Cfg::NT, max_wg));
        fast_cols_visit_variant<Cfg>(sh.variant, [&](auto tiled, auto sliced, auto dyn) {
            err = launch_lds<k_fast_cols<Cfg, tiled.value, sliced.value, dyn.value>>(dim3(sh.grid), Cfg::NT, lds, s, sh.a);
        });
    }
};

}  // namespace

template <>
GroupResult launch_fast_cols_group<FC_TU_GROUP>(int M, int T, const FastColsArgs& a, int num_cus, hipStream_t s) {
    FastColsLauncher l{a, num_cus, s};
    if (!fast_cols_dispatch_group<FC_TU_GROUP>(M, T, l)) return {};
    return l.err;
}

}  // namespace fc
