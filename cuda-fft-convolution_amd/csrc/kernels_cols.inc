// kernels_cols.inc -- the output-column kernel (fast_cols.hpp).
// Included by kernels_cols_g<G>.hip with FC_TU_GROUP = G: defines group G's entry point (kernels.hpp) over that group of column
// configurations.  kernels_cols16_g<G>.hip include it with FC_TU_OUT16 = 1 as well: the same configurations and launch
// decisions with 16-bit maps (k_fast_cols16; fp16 or bf16 by FastColsArgs::out_format), in translation units of their own so
// that the fp32 units compile exactly what they compiled before and the new ones build beside them.
#include "kernels_common.hpp"

#ifndef FC_TU_OUT16
#define FC_TU_OUT16 0
#endif

namespace fc {
namespace {

#if FC_TU_OUT16
#define FC_K_FAST_COLS k_fast_cols16
#define FC_LAUNCH_FAST_COLS_GROUP launch_fast_cols16_group
template <class Cfg, bool TILED, bool SLICED = false, bool DYN = false>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_cols16(FastColsArgs a) {
    DevPhaseCtx<std::conditional_t<TILED, ColPairState<Cfg>, ColState<Cfg>>> ctx;
    fast_cols_body<Cfg, TILED, SLICED, DYN, ColStore::PAIRS16>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)gridDim.x);
}
#else
#define FC_K_FAST_COLS k_fast_cols
#define FC_LAUNCH_FAST_COLS_GROUP launch_fast_cols_group
template <class Cfg, bool TILED, bool SLICED = false, bool DYN = false>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_cols(FastColsArgs a) {
    DevPhaseCtx<std::conditional_t<TILED, ColPairState<Cfg>, ColState<Cfg>>> ctx;
    fast_cols_body<Cfg, TILED, SLICED, DYN>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)gridDim.x);
}
#endif

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
            err = launch_lds<FC_K_FAST_COLS<Cfg, tiled.value, sliced.value, dyn.value>>(dim3(sh.grid), Cfg::NT, lds, s, sh.a);
        });
    }
};

}  // namespace

template <>
GroupResult FC_LAUNCH_FAST_COLS_GROUP<FC_TU_GROUP>(int M, int T, const FastColsArgs& a, int num_cus, hipStream_t s) {
    FastColsLauncher l{a, num_cus, s};
    if (!fast_cols_dispatch_group<FC_TU_GROUP>(M, T, l)) return {};
    return l.err;
}

}  // namespace fc
