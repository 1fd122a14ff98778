// emu_runners.hpp -- TEST-ONLY: the host contexts and runner objects that execute the specialised workgroup bodies
// sequentially (see emu.cpp).  Shared by emu.cpp and the per-group translation units emu_rows_g*.cpp / emu_cols_g*.cpp,
// which instantiate one group of configurations of fast_paths.hpp each.  Which instantiation runs and on what grid is decided
// by the product's own launch decisions (fast_paths.hpp), so the bodies tested here are the ones the launchers launch.
#pragma once
#include <vector>

#include "pipeline.hpp"

namespace emu {
using namespace fc;

struct HostCtx {
    int tid = 0, nthreads = 1;
    void sync() const {}
};

// Phase-structured bodies (fast_rows.hpp): every phase is run for all NT threads before the
// next one starts, with one State per emulated thread.
template <class State>
struct HostPhaseCtx {
    int NT;
    std::vector<State> st;
    explicit HostPhaseCtx(int nt) : NT(nt), st(nt) {}
    template <class F>
    void phase(F&& f) {
        for (int t = 0; t < NT; t++) f(t, st[t]);
    }
    template <class F>
    void phase_nosync(F&& f) {
        for (int t = 0; t < NT; t++) f(t, st[t]);
    }
    template <bool NOSYNC, class F>
    void phase_dbg(F&& f) {
        for (int t = 0; t < NT; t++) f(t, st[t]);
    }
};

struct EmuFastRows {
    const FastRowsArgs& a;
    c32* lds;
    int rows;
    int group = 0;     // > 1: multi-map body, walks of `group` consecutive kernels per workgroup (the product's kernels_per_wg)
    int kernels = 1;   // kernels of the launch: their column spectra at a.A + k * a_kernel_stride, their rows of the
                       // intermediate at a.Y + k * y_kernel_stride (as a launch of the product: every workgroup walks
                       // DISTINCT kernels, so the walk's indexing is exercised, the last walk partial where `group`
                       // does not divide `kernels`)
    template <class Cfg, int NZ2>
    void go() {
        // (always the walk over maps / (map, feature) pairs, as the product's launchers: walks of one map where group <= 1)
        const int per_wg = group > 1 ? group : 1;
        const FastRowsGrid g = fast_rows_grid(rows, Cfg::RPW, kernels, per_wg);
        fast_rows_visit_linear<Cfg>(a, [&](auto linear) {
            for (int walk = 0; walk < g.walks; walk++) {
                const int kernel0 = walk * per_wg;
                const int nk = kernels - kernel0 < per_wg ? kernels - kernel0 : per_wg;
                for (int grp = 0; grp < g.groups; grp++) {
                    for (int i = 0; i < Cfg::LDS_ELEMS; i++) lds[i] = mk(1e30f, -1e30f);
                    if (a.F > 1) {   // the walk over (map, feature) pairs
                        HostPhaseCtx<RowMultiState<Cfg, true>> ctx(Cfg::NT);
                        fast_rows_multi_body<Cfg, NZ2, linear.value, true>(ctx, lds, a, grp, kernel0, nk, rows);
                    } else {
                        HostPhaseCtx<RowMultiState<Cfg>> ctx(Cfg::NT);
                        fast_rows_multi_body<Cfg, NZ2, linear.value>(ctx, lds, a, grp, kernel0, nk, rows);
                    }
                }
            }
        });
    }
};

struct EmuFastRowsFwd {
    const FastRowsFwdArgs& a;
    c32* lds;
    int rows;
    template <class Cfg>
    void go() {
        for (int grp = 0; grp < fast_rows_grid(rows, Cfg::RPW, 1, 1).groups; grp++) {
            for (int i = 0; i < Cfg::LDS_ELEMS; i++) lds[i] = mk(1e30f, -1e30f);
            HostPhaseCtx<RowFwdState> ctx(Cfg::NT);
            fast_rows_fwd_body<Cfg>(ctx, lds, a, grp, rows);
        }
    }
};

struct EmuFastColsFwd {
    const FastColsFwdArgs& a;
    c32* lds;
    int nwg;
    template <class Cfg, int NZ2>
    void go() {
        for (int wg = 0; wg < nwg; wg++) {
            for (int i = 0; i < Cfg::LDS_ELEMS; i++) lds[i] = mk(1e30f, -1e30f);
            HostPhaseCtx<ColFwdState> ctx(Cfg::NT);
            fast_cols_fwd_body<Cfg, NZ2>(ctx, lds, a, wg, nwg);
        }
    }
};

struct EmuFastCols {
    const FastColsArgs& a;
    c32* lds;
    int nwg;           // "persistent workgroups" of an unsliced launch
    template <class Cfg>
    void go() {
        // The product's launch shape with the emulator's deliberate differences: 8 persistent workgroups where the launcher
        // would slice the tail round, so that the sliced body runs on the CPU tier too (e.g. 18 tiles = 2 full rounds of
        // 8 + 2 tiles in 4 slices each) ...
        FastColsShape sh = fast_cols_launch_shape(Cfg::M, Cfg::T, a, 8);
        // ... chunks of two tiles from the dynamic queue (the counters are zero between launches: the last workgroup out
        // zeroes them), and the caller's `nwg` workgroups for every unsliced launch, so that a workgroup takes several tiles
        if (sh.variant == FastColsVariant::TILED_DYN) sh.a.queue_shift = 1;
        if (sh.variant != FastColsVariant::TILED_SLICED) sh.grid = nwg;
        fast_cols_visit_variant<Cfg>(sh.variant, [&](auto tiled, auto sliced, auto dyn) {
            for (int wg = 0; wg < sh.grid; wg++) {
                for (int i = 0; i < Cfg::LDS_ELEMS; i++) lds[i] = mk(1e30f, -1e30f);
                HostPhaseCtx<std::conditional_t<tiled.value, ColPairState<Cfg>, ColState<Cfg>>> ctx(Cfg::NT);
                fast_cols_body<Cfg, tiled.value, sliced.value, dyn.value>(ctx, lds, sh.a, wg, sh.grid);
            }
        });
    }
};

// per-group entry points (the specialisation for group G is defined in emu_rows_g<G>.cpp / emu_cols_g<G>.cpp; emu.cpp tries
// the groups in order); false: no configuration of that group matches
template <int G> bool fast_rows_group(int L, int nz2, EmuFastRows& run);
template <int G> bool fast_rows_fwd_group(int L, EmuFastRowsFwd& run);
template <int G> bool fast_cols_group(int M, int T, EmuFastCols& run);
template <int G> bool fast_cols_fwd_group(int M, int T, bool pruned, EmuFastColsFwd& run);

}  // namespace emu
