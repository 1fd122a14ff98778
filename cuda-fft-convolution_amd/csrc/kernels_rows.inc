// kernels_rows.inc -- the forward image-row kernel (fast_rows_fwd.hpp).  (Until round 4 also the one-map spectral-row kernel
// of fast_rows.hpp: single-map launches now take the multi-map walk with one map per workgroup -- the one-map form kept part
// of its per-thread state in scratch behind a vmcnt(0), and was one more kernel per configuration to build.)
// Included by kernels_rows_g<G>.hip with FC_TU_GROUP = G: defines group G's entry point (kernels.hpp) over that group of row
// configurations.
#include "kernels_common.hpp"

namespace fc {
namespace {

template <class Cfg>
__global__ void __launch_bounds__(Cfg::NT, 3) k_fast_rows_fwd(FastRowsFwdArgs a, int rows) {
    DevPhaseCtx<RowFwdState> ctx;
    fast_rows_fwd_body<Cfg>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, rows);
}

struct FastRowsFwdLauncher {
    const FastRowsFwdArgs& a;
    int rows;
    hipStream_t s;
    hipError_t err = hipSuccess;
    template <class Cfg>
    void go() {
        err = launch_lds<k_fast_rows_fwd<Cfg>>(dim3(fast_rows_grid(rows, Cfg::RPW, 1, 1).groups), Cfg::NT, (size_t)Cfg::LDS_ELEMS * sizeof(c32), s, a, rows);
    }
};

}  // namespace

template <>
GroupResult launch_fast_rows_fwd_group<FC_TU_GROUP>(int L, const FastRowsFwdArgs& a, int rows, hipStream_t s) {
    FastRowsFwdLauncher l{a, rows, s};
    if (!fast_rows_fwd_dispatch_group<FC_TU_GROUP>(L, l)) return {};
    return l.err;
}

}  // namespace fc
