// fast_paths.hpp -- registry of the specialised (compile-time) kernel configurations.
//
// The generic kernels (kernels_body.hpp) handle every supported length; the configurations
// listed here replace the two hot kernels for the transform lengths that matter (the BASELINE
// configs), chosen so that every stage keeps most lanes busy and the LDS budget allows
// 3 waves per SIMD.  The planner prefers these lengths (planner.hpp: choose_length).
#pragma once
#include <array>
#include <type_traits>
#include <vector>

#include "fast_cols.hpp"
#include "fast_cols_fwd.hpp"
#include "fast_rows.hpp"
#include "fast_rows_fwd.hpp"
#include "fast_rows_images.hpp"
#include "fast_rows_multi.hpp"
#include "planner.hpp"

namespace fc {

// planner factors of the two awkward BASELINE windows (see fast_rows_factor): above ~0.5 the planner prefers the next
// convenient length (1152 / 4224) and crops; exact_window plans use the window's own kernels regardless
constexpr double FC_FACTOR_1088 = 0.60, FC_FACTOR_4160 = 0.60;

// X(L, R1, R2, R3, NT, RPW, NZ2): see fast_rows.hpp.  RPW rows of L = R1 x R2 x R3 points per workgroup of NT threads, chosen so that
// RPW * R1 * R2 (the stage-3 butterflies, one per thread) fill the lanes and stage 2 takes one round where possible; NZ2 = non-zero
// stage-2 inputs the variant reads (kernel width <= NZ2 * R3), listed ascending per length (the dispatcher takes the first that
// covers the kernel).  What shaped the list (history/; A/B files under profiles/):
//   * BASELINE: 4224 = 8.24.22 (cfg3; cfg4's 4160 window runs on it and crops), 2112 = 8.12.22 x2 (cfg5), 1152 = 8.12.12 x2 (cfg2's
//     1088 window), 288 = 4.6.12 x8 (cfg1).  4160 = 8.20.26 and 1088 = 8.17.8 are those two windows' OWN kernels (round 5's search over
//     their radix splits, r05d_native_window_search.txt: 10.16.26 -> 8.20.26 -4 %, 17.4.16 x2 -> 8.17.8 -2 %; 16.10.26, 5.32.26, 8.26.20,
//     20.8.26, 16.13.20, 13.16.20 and 4.17.16, 17.4.16 x3 measured slower): still slower than the convenient length + crop
//     (r05e_native_window_ab.txt), used by exact_window plans only (planner factors above).
//   * Round 4 filled the ladder (r04z_size_sweep.txt): a transform is at most ~1.13 x the padded size per dimension above 1000 pixels.
//   * Long rows: 160 KB of LDS hold two rows of >= 7040 points (one 640- / 768-thread workgroup per CU); 5120 ... 6144 run one row per
//     256-thread workgroup, three workgroups per CU (r04g: -11 ... -25 % against the R1 = 16 forms on 320 / 384 threads).  More than
//     128 VGPRs forbid a second 6-wave workgroup on a CU (round 3), hence no 384-thread configurations.
//   * Stage 3 reads and writes its run of R3 values 16 bytes at a time, lane q's run R3 * 8 bytes after lane q - 1's: 128 bytes at
//     R3 = 16 -- every lane of an LDS access group on the same banks (8-way conflict), 4-way at R3 = 24, 2-way at 12 / 20, none at 10,
//     14, 18, 22, 26.  The R3 = 16 forms went (r04h_row_and_column_configs_ab.txt: rows -11 ... -25 %); 4608 as 8.32.18 and 1152 as
//     8.8.18 x4 measured SLOWER than the R3 = 24 / 12 forms -- bank conflicts are one term, not the whole cost.
//   * Late round 4: 384, 480, 672, 864, 960 (images of 300-900 pixels had only 576 and 768 between 288 and 1088) and 1280, 3360 into the
//     widest gaps above (r04t / r04u size sweeps).  1440 = 8.10.18 x2 (M = 720 = 6.10.12) and 1680 = 10.12.14 x2 (M = 840 = 6.10.14) were
//     built too and dropped: a 1440 x 1440 transform took 402 us per 64 maps against 375 for 1536 x 1536, 1680 x 1680 as long as 1760 x 1760.
//   * A search over every admissible (R1, R2, R3, threads) of each length (tools/config_variant.py, r04i_config_search_*.txt) moved
//     4608 to 12.16.24 (-5 %), 6144 to 16.16.24 (-10 %), 3072 to 16.16.12 (-9 %) and 2560 to 16.16.10 (-14 %): a power-of-two stage 2
//     of 16 points against 24 / 32.  No rule came out of it -- 5120 as 16.16.20 is 6 % SLOWER than 8.32.20, 4608 as 16.16.18 14 % slower
//     than 12.16.24 -- and everything else it tried was within noise (+-3 %) or slower (up to +90 %); the list is what survived.
//   * Radix orders at 4224 (round 2): 8.24.22 25.0 us per map, 12.16.22 25.6, 11.16.24 27.3, 16.12.22 28.0: small R1, fat stage 3.
// Three groups, one translation unit each per kernel family (kernels_rows*_g?.hip, tests/emu/emu_rows_g?.cpp).  A fourth group
// takes three edits: its table macro (and its branch in FC_ROW_CONFIGS_OF_GROUP), FC_ROW_GROUPS, and a _g3 file per family with
// its Makefile entry -- the fan-out over the groups (first_group below) follows FC_ROW_GROUPS.  The columns likewise.
#define FC_FAST_ROW_CONFIGS_G0(X)   \
    X(8448, 16, 24, 22, 768, 2, 3)  \
    X(8448, 16, 24, 22, 768, 2, 6)  \
    X(8448, 16, 24, 22, 768, 2, 24) \
    X(7680, 16, 24, 20, 768, 2, 4)  \
    X(7680, 16, 24, 20, 768, 2, 24) \
    X(7040, 10, 32, 22, 640, 2, 3)  \
    X(7040, 10, 32, 22, 640, 2, 6)  \
    X(7040, 10, 32, 22, 640, 2, 32) \
    X(6144, 16, 16, 24, 256, 1, 3)  \
    X(6144, 16, 16, 24, 256, 1, 6)  \
    X(6144, 16, 16, 24, 256, 1, 16) \
    X(5632, 16, 16, 22, 256, 1, 3)  \
    X(5632, 16, 16, 22, 256, 1, 16) \
    X(5120, 8, 32, 20, 256, 1, 4)   \
    X(5120, 8, 32, 20, 256, 1, 7)   \
    X(5120, 8, 32, 20, 256, 1, 32)
#define FC_FAST_ROW_CONFIGS_G1(X)   \
    X(4608, 12, 16, 24, 192, 1, 3)  \
    X(4608, 12, 16, 24, 192, 1, 6)  \
    X(4608, 12, 16, 24, 192, 1, 16) \
    X(4224, 8, 24, 22, 192, 1, 3)   \
    X(4224, 8, 24, 22, 192, 1, 6)   \
    X(4224, 8, 24, 22, 192, 1, 24)  \
    X(4160, 8, 20, 26, 192, 1, 3)   \
    X(4160, 8, 20, 26, 192, 1, 5)   \
    X(4160, 8, 20, 26, 192, 1, 20)  \
    X(3840, 8, 24, 20, 192, 1, 4)   \
    X(3840, 8, 24, 20, 192, 1, 24)  \
    X(3520, 10, 16, 22, 192, 1, 3)  \
    X(3520, 10, 16, 22, 192, 1, 16) \
    X(3360, 10, 24, 14, 256, 1, 5)  \
    X(3360, 10, 24, 14, 256, 1, 10) \
    X(3360, 10, 24, 14, 256, 1, 24) \
    X(3072, 16, 16, 12, 256, 1, 6)  \
    X(3072, 16, 16, 12, 256, 1, 16) \
    X(2816, 8, 16, 22, 192, 1, 3)   \
    X(2816, 8, 16, 22, 192, 1, 16)  \
    X(2560, 16, 16, 10, 256, 1, 7)  \
    X(2560, 16, 16, 10, 256, 1, 16)
#define FC_FAST_ROW_CONFIGS_G2(X)   \
    X(2304, 8, 16, 18, 256, 2, 4)   \
    X(2304, 8, 16, 18, 256, 2, 16)  \
    X(2112, 8, 12, 22, 192, 2, 3)   \
    X(2112, 8, 12, 22, 192, 2, 12)  \
    X(1920, 8, 12, 20, 192, 2, 3)   \
    X(1920, 8, 12, 20, 192, 2, 12)  \
    X(1760, 10, 8, 22, 192, 2, 3)   \
    X(1760, 10, 8, 22, 192, 2, 8)   \
    X(1536, 8, 16, 12, 256, 2, 3)   \
    X(1536, 8, 16, 12, 256, 2, 6)   \
    X(1536, 8, 16, 12, 256, 2, 16)  \
    X(1344, 6, 16, 14, 192, 2, 3)   \
    X(1344, 6, 16, 14, 192, 2, 16)  \
    X(1280, 8, 16, 10, 256, 2, 4)   \
    X(1280, 8, 16, 10, 256, 2, 7)   \
    X(1280, 8, 16, 10, 256, 2, 16)  \
    X(1152, 8, 12, 12, 192, 2, 3)   \
    X(1152, 8, 12, 12, 192, 2, 6)   \
    X(1152, 8, 12, 12, 192, 2, 12)  \
    X(1088, 8, 17, 8, 192, 1, 4)    \
    X(1088, 8, 17, 8, 192, 1, 8)    \
    X(1088, 8, 17, 8, 192, 1, 17)   \
    X(960, 6, 16, 10, 192, 2, 4)    \
    X(960, 6, 16, 10, 192, 2, 7)    \
    X(960, 6, 16, 10, 192, 2, 16)   \
    X(864, 4, 12, 18, 192, 4, 4)    \
    X(864, 4, 12, 18, 192, 4, 12)   \
    X(768, 4, 16, 12, 256, 4, 3)    \
    X(768, 4, 16, 12, 256, 4, 6)    \
    X(768, 4, 16, 12, 256, 4, 16)   \
    X(672, 4, 12, 14, 192, 4, 3)    \
    X(672, 4, 12, 14, 192, 4, 12)   \
    X(576, 4, 12, 12, 192, 4, 3)    \
    X(576, 4, 12, 12, 192, 4, 12)   \
    X(480, 4, 12, 10, 192, 4, 4)    \
    X(480, 4, 12, 10, 192, 4, 12)   \
    X(384, 4, 8, 12, 192, 6, 3)     \
    X(384, 4, 8, 12, 192, 6, 8)     \
    X(288, 4, 6, 12, 192, 8, 3)     \
    X(288, 4, 6, 12, 192, 8, 6)
#define FC_FAST_ROW_CONFIGS(X) FC_FAST_ROW_CONFIGS_G0(X) FC_FAST_ROW_CONFIGS_G1(X) FC_FAST_ROW_CONFIGS_G2(X)
constexpr int FC_ROW_GROUPS = 3;
// the configurations of group G only
#define FC_ROW_CONFIGS_OF_GROUP(G, X)                                   \
    do {                                                                \
        if constexpr ((G) == 0) { FC_FAST_ROW_CONFIGS_G0(X) }           \
        else if constexpr ((G) == 1) { FC_FAST_ROW_CONFIGS_G1(X) }      \
        else { FC_FAST_ROW_CONFIGS_G2(X) }                              \
    } while (0)

struct FastRowsInfo {
    bool ok = false;
    int L = 0, R1 = 0, R2 = 0, R3 = 0, NT = 0, RPW = 1;
    int max_kw = 0;      // largest kernel width the fast kernel accepts
    size_t lds_bytes = 0;
};

// Is there a fast row kernel for transform length L able to take kernels up to max_kw wide?
inline FastRowsInfo fast_rows_lookup(int L, int max_kw) {
    FastRowsInfo r;
#define FC_X(LL, A, B, C, NTT, RP, NZ)                                                    \
    if (!r.ok && L == LL) {                                                               \
        using Cfg = RowCfg<LL, A, B, C, NTT, RP>;                                         \
        if (max_kw <= Cfg::m1) {                                                          \
            r.ok = true; r.L = LL; r.R1 = A; r.R2 = B; r.R3 = C; r.NT = NTT; r.RPW = RP;  \
            r.max_kw = Cfg::m1; r.lds_bytes = (size_t)Cfg::LDS_ELEMS * sizeof(c32);       \
        }                                                                                 \
    }
    FC_FAST_ROW_CONFIGS(FC_X)
#undef FC_X
    return r;
}

inline bool fast_rows_length(int L, int max_kw) { return fast_rows_lookup(L, max_kw < 1 ? 1 : max_kw).ok; }

// Cost per point of a specialised length relative to the planner's generic estimate (planner.hpp: LengthFactor; 0 = no
// specialised kernel).  0.45 is what the specialised kernels measure against the generic ones; the two BASELINE windows
// that are awkward to factor carry what their own kernels measure against the next convenient length + crop
// (profiles/r04*_native_window_ab.txt): 1088 = 2^6 x 17 against 1152, 4160 = 2^6 x 5 x 13 against 4224.
inline double fast_rows_factor(int L, int max_kw) {
    if (!fast_rows_length(L, max_kw)) return 0.0;
    if (L == 1088) return FC_FACTOR_1088;
    if (L == 4160) return FC_FACTOR_4160;
    if (L >= 5120) return 0.60;      // the long-row configurations run at ~270 Gpx/s-equivalent against ~360 up to 4608 points
    return 0.45;
}

// Tries f(std::integral_constant<int, G>{}) for the groups G = 0 .. N-1 in order and stops at the first result that tests true
// (a match: true, or an engaged optional); no match: the last group's (false / empty) result.
template <int N, int G = 0, class F>
inline auto first_group(F&& f) {
    if constexpr (G + 1 < N) {
        if (auto r = f(std::integral_constant<int, G>{})) return r;
        return first_group<N, G + 1>(f);
    } else {
        return f(std::integral_constant<int, G>{});
    }
}

// Calls run.template go<Cfg, NZ2>() for the first listed configuration of length L (in group G: the translation units
// of a kernel family instantiate one group each) whose NZ2 covers `nz2_needed` (configurations are listed with
// ascending NZ2).  false if there is none.
template <int G, class Runner>
inline bool fast_rows_dispatch_group(int L, int nz2_needed, Runner&& run) {
#define FC_X(LL, A, B, C, NTT, RP, NZ)                          \
    if (L == LL && nz2_needed <= NZ) {                          \
        run.template go<RowCfg<LL, A, B, C, NTT, RP>, NZ>();    \
        return true;                                            \
    }
    FC_ROW_CONFIGS_OF_GROUP(G, FC_X);
#undef FC_X
    return false;
}
// Forward image-row kernel (fast_rows_fwd.hpp): one instantiation per length -- the first listed configuration of that
// length (nz2_needed = 0), the NZ2 dropped: run.template go<Cfg>().
template <class Runner>
struct DropNZ2 {
    Runner& run;
    template <class Cfg, int>
    void go() { run.template go<Cfg>(); }
};
template <int G, class Runner>
inline bool fast_rows_fwd_dispatch_group(int L, Runner&& run) {
    return fast_rows_dispatch_group<G>(L, 0, DropNZ2<std::remove_reference_t<Runner>>{run});
}

// Image-walk spectral-row kernel (fast_rows_images.hpp; plan option "image_walk"): one instantiation per length -- its forward
// part runs once per walk and reads every stage-2 input, so the NZ2 of the list does not enter (fast_rows_fwd_dispatch_group
// finds the length's configuration).  A length whose kernel would spill registers, use scratch or hold fewer than the 3 waves
// per SIMD of its launch bounds in the build's reports (csrc/*.rpt) is NOT built and listed here: a plan of that length keeps the
// kernel walk (read-only option "image_walk_active" 0).  The built ones and the ones listed here add up to the 32 lengths.
// At the 168 registers of three waves per SIMD, kf + the product + the butterfly's temporaries leave no room at these six:
// 4160 = 8.20.26 spills 72 registers (radix 26), 7040 = 10.32.22 x2 20 (a 32-point stage 2 beside two rows' constants), and
// 6144, 5120, 4608 and 1920 (stage 3 of 24 / 20 points) each park one stage-1 base twiddle in scratch and fetch it back in
// every map's P5 -- little, but a scratch access shares the in-order memory counter with the stores and the row in flight.
constexpr int FC_ROWS_IMAGES_NOT_BUILT[] = {7040, 6144, 5120, 4608, 4160, 1920};
constexpr bool fast_rows_images_built(int L) {
    for (int x : FC_ROWS_IMAGES_NOT_BUILT)
        if (x == L) return false;
    return true;
}
inline bool fast_rows_images_available(int L, int max_kw) { return fast_rows_lookup(L, max_kw < 1 ? 1 : max_kw).ok && fast_rows_images_built(L); }

// Spectral filter (fast_rows_multi.hpp: FILTER; spectral_filter.hpp; plan entry fftconv_plan_set_spectral_filter): the F = 1 kernel
// walk with the filter's pointwise function in place of the product -- one instantiation per (length, NZ2), the mode a uniform of
// the launch, in kernels of their own name (kernels_rows_filter_g<G>.hip).  The rule for a variant: no spilled register and no
// scratch in the build's reports (csrc/kernels_rows_filter_g*.rpt); it may hold fewer waves per SIMD than its plain sibling.
// Compiled as the plain kernels are, seven lengths spilled (4 ... 57 registers at the 168 of three waves per SIMD).  Two of them fit
// once the walk forms its stage-1 twiddle chain again per map instead of keeping the even powers (RowMultiState: KEEP is off under
// FILTER -- 4224 and 3520, 9 spilled registers with them kept, 159 and 156 registers without).  Four run on launch bounds of two waves per SIMD
// (fast_rows_filter_min_waves): 2112 (173 registers), 864 (172), 4608 (169 at NZ2 = 16) and 4160 (185: radix 26).  The last one, 7040
// = 10.32.22 x2, cannot be relaxed -- its workgroup of 640 threads is ten waves, three per SIMD whatever the bounds say -- and
// spills 4 registers: it is NOT built and listed here, and the setter refuses modes 1 and 2 on a plan of that length (a caller
// creates the plan with kernel_path 1).  The built ones and the ones listed here add up to the 32 lengths
// (tests/test_spectral_filter_host.py holds the reports against it).
constexpr int FC_ROWS_FILTER_NOT_BUILT[] = {7040};
constexpr bool fast_rows_filter_built(int L) {
    for (int x : FC_ROWS_FILTER_NOT_BUILT)
        if (x == L) return false;
    return true;
}
// minimum waves per SIMD of a filter kernel's launch bounds: the plain kernels' 3, or 2 (up to 256 registers)
constexpr int FC_ROWS_FILTER_TWO_WAVES[] = {4608, 4160, 2112, 864};
constexpr int fast_rows_filter_min_waves(int L) {
    for (int x : FC_ROWS_FILTER_TWO_WAVES)
        if (x == L) return 2;
    return 3;
}

// Host tables of a fast row configuration.
struct FastRowsTables {
    Plan1D plan;               // radices (R1, R2, R3)
    std::vector<c32> tw1;      // w_L^j, j < m1
    std::vector<c32> tw2;      // stage-2 table
    std::vector<int> relayout; // register-order index -> generic position (RowsFwdArgs::out_map)
};

inline FastRowsTables make_fast_rows_tables(const FastRowsInfo& fi, const Plan1D& generic) {
    FastRowsTables t;
    t.plan = make_plan1d_seq(fi.L, {fi.R1, fi.R2, fi.R3});
    const int m1 = fi.L / fi.R1;
    const StageDesc& s1 = t.plan.desc.st[0];
    const StageDesc& s2 = t.plan.desc.st[1];
    t.tw1.assign(t.plan.tw.begin() + s1.tw_off, t.plan.tw.begin() + s1.tw_off + m1);
    t.tw2.assign(t.plan.tw.begin() + s2.tw_off, t.plan.tw.begin() + s2.tw_off + (fi.R2 - 1) * fi.R3);
    const int NB3 = fi.R1 * fi.R2;
    t.relayout.assign(fi.L, 0);
    for (int k = 0; k < fi.L; k++) {
        int p = t.plan.pos[k];
        int q = p / fi.R3, a = p % fi.R3;
        int ro = ((a >> 1) * NB3 + q) * 2 + (a & 1);
        t.relayout[ro] = generic.pos[k];
    }
    return t;
}

// ---------------------------------------------------------------------------------------
// Output (column) kernel configurations: X(M, R1, R2, R3, T, NT), see fast_cols.hpp: M = R1 x R2 x R3 complex points (transform
// length 2M along h), T columns per tile, NT = R1 * R2 * T threads (one stage-3 butterfly per thread).  T = 16 (full 128-byte lines of
// the tiled intermediate) while 16 columns fit the LDS (M <= 1056), 8 up to M = 2304, 4 above.  The forward column kernel
// (fast_cols_fwd.hpp) runs the same configurations.
//   * cfg3: M = 2112 = 6.16.22, 8 columns, 768 threads (8.12.22 until the round-4 search: 6.16.22 is 4 % faster, roofline fraction
//     0.68 -> 0.71; 4 columns / 384 threads, two workgroups per CU, measured 47.8 against 36.1 us per map in round 1); cfg5: 1056 =
//     6.8.22; cfg2: 576 = 6.8.12; cfg1: 144 = 4.6.6.
//   * Round 4: the R3 = 16 / 24 forms were replaced (stage-3 bank conflicts, see the row list): output kernel -2 ... -15 % for eleven
//     lengths (r04h_row_and_column_configs_ab.txt); 1024-thread workgroups (16 waves, <= 128 VGPRs) where R3 = 10 / 12 / 18 needs
//     them.  M = 1152 as 8.8.18 / T = 16, 576 as 4.8.18 and 288 as 6.8.6 measured no better than the listed forms.
//   * The same search (r04i_config_search_*.txt): M = 3520 as 10.16.22 (-4 %), 1760 as 5.16.22 (-6 %); 1056 as 3.16.22, 1152 as 12.8.12,
//     576 as 3.16.12 / 4.12.12, 1408 as 4.16.22 within noise over three repetitions and left alone.
//   * M = 2080 = 8.13.20 (832 threads) and 544 = 17.4.8 (8 columns): the cfg4 / cfg2 windows' own kernels (exact_window plans).  Round 5
//     (r05d_native_window_search.txt): 8.10.26 (radix 26 beside seven rounds of prefetch: 12 spilled registers) -> 8.13.20 on 832 threads
//     (128 registers: 4 spilled), -12 % (13.8.20 -11 %, 4.20.26 -6 %, 5.16.26 / 10.8.26 +-1 %, 4.26.20 +23 %); 544 as 8-column tiles 17.4.8: the output
//     kernel itself +6 % at 64 maps, but the forward column passes (image, kernels) get twice the tiles: the step -1 % at 64 maps,
//     -11 % at cfg2's 16 (2.17.16 / 17.2.16 at 16 columns: no difference).
#define FC_FAST_COL_CONFIGS_G0(X) \
    X(4224, 8, 24, 22, 4, 768)    \
    X(3840, 8, 24, 20, 4, 768)    \
    X(3520, 10, 16, 22, 4, 640)    \
    X(3072, 8, 32, 12, 4, 1024)    \
    X(2816, 8, 16, 22, 4, 512)    \
    X(2560, 8, 32, 10, 4, 1024)    \
    X(2304, 8, 16, 18, 8, 1024)    \
    X(2112, 6, 16, 22, 8, 768)    \
    X(2080, 8, 13, 20, 8, 832)    \
    X(1920, 8, 12, 20, 8, 768)    \
    X(1760, 5, 16, 22, 8, 640)    \
    X(1680, 6, 20, 14, 8, 960)
#define FC_FAST_COL_CONFIGS_G1(X) \
    X(1536, 8, 16, 12, 8, 1024)    \
    X(1408, 8, 8, 22, 8, 512)    \
    X(1280, 8, 16, 10, 8, 1024)    \
    X(1152, 8, 12, 12, 8, 768)    \
    X(1056, 6, 8, 22, 16, 768)    \
    X(960, 6, 8, 20, 16, 768)     \
    X(880, 5, 8, 22, 16, 640)     \
    X(768, 8, 8, 12, 16, 1024)     \
    X(672, 6, 8, 14, 16, 768)     \
    X(640, 8, 8, 10, 16, 1024)    \
    X(576, 6, 8, 12, 16, 768)     \
    X(544, 17, 4, 8, 8, 544)      \
    X(480, 6, 8, 10, 16, 768)     \
    X(432, 6, 6, 12, 16, 576)     \
    X(384, 4, 8, 12, 16, 512)     \
    X(336, 4, 6, 14, 16, 384)     \
    X(288, 4, 6, 12, 16, 384)     \
    X(240, 4, 6, 10, 16, 384)     \
    X(192, 4, 8, 6, 16, 512)      \
    X(144, 4, 6, 6, 16, 384)
#define FC_FAST_COL_CONFIGS(X) FC_FAST_COL_CONFIGS_G0(X) FC_FAST_COL_CONFIGS_G1(X)
constexpr int FC_COL_GROUPS = 2;
#define FC_COL_CONFIGS_OF_GROUP(G, X)                                   \
    do {                                                                \
        if constexpr ((G) == 0) { FC_FAST_COL_CONFIGS_G0(X) }           \
        else { FC_FAST_COL_CONFIGS_G1(X) }                              \
    } while (0)

struct FastColsInfo {
    bool ok = false;
    int M = 0, R1 = 0, R2 = 0, R3 = 0, T = 0, NT = 0;
    size_t lds_bytes = 0;
};

inline FastColsInfo fast_cols_lookup(int M) {
    FastColsInfo r;
#define FC_X(MM, A, B, C, TT, NTT)                                                   \
    if (!r.ok && M == MM) {                                                          \
        using Cfg = ColCfg<MM, A, B, C, TT, NTT>;                                    \
        r.ok = true; r.M = MM; r.R1 = A; r.R2 = B; r.R3 = C; r.T = TT; r.NT = NTT;   \
        r.lds_bytes = (size_t)Cfg::LDS_ELEMS * sizeof(c32);                          \
    }
    FC_FAST_COL_CONFIGS(FC_X)
#undef FC_X
    return r;
}

inline bool fast_cols_length(int M, int) { return fast_cols_lookup(M).ok; }
inline double fast_cols_factor(int M, int) {
    if (!fast_cols_lookup(M).ok) return 0.0;
    if (M == 544) return FC_FACTOR_1088;
    if (M == 2080) return FC_FACTOR_4160;
    if (M >= 2560) return 0.60;      // 4-column tiles
    return 0.45;
}

// Measured cost of the two hot kernels per point of their transforms, picoseconds (profiles/r04k_cost_per_point_by_length.txt:
// the multi-map row kernel per point of a spectrum row, the output kernel per complex point of a stored column; one MI355X,
// 63 x 63 kernels, 16-64 maps per launch).  The block-wise planner (fftconv_api.cpp: choose_save_tiling) weighs block
// transforms against each other and against one pass with them; only the ratios matter.
inline double fast_rows_ps(int L) {
    switch (L) {
        case 1152: return 2.52; case 1344: return 2.71; case 1536: return 2.21; case 1760: return 2.53; case 1920: return 2.39;
        case 2112: return 2.41; case 2304: return 2.23; case 2560: return 2.38; case 2816: return 2.43; case 3072: return 2.12;
        case 3520: return 2.55; case 3840: return 2.42; case 4224: return 2.39; case 4608: return 2.42; case 5120: return 2.38;
        case 5632: return 2.40; case 6144: return 2.38; case 7040: return 2.86; case 7680: return 2.62; case 8448: return 2.78;
        case 1088: case 4160: return 2.9;
        default: return 2.7;             // the small lengths (launch-bound at their own sizes)
    }
}
inline double fast_cols_ps(int M) {
    switch (M) {
        case 576: return 2.94; case 672: return 2.84; case 768: return 2.97; case 880: return 3.06; case 960: return 2.84;
        case 1056: return 2.94; case 1152: return 2.89; case 1280: return 2.78; case 1408: return 3.01; case 1536: return 2.83;
        case 1760: return 2.95; case 1920: return 2.92; case 2112: return 2.80; case 2304: return 2.80;
        case 2560: return 3.76; case 2816: return 3.66; case 3072: return 3.62; case 3520: return 3.70; case 3840: return 3.69;
        case 4224: return 3.67;
        case 544: case 2080: return 3.3;
        default: return 3.1;
    }
}

// Calls run.template go<Cfg>() for the configuration (M, T) if group G lists it; false if it does not.
template <int G, class Runner>
inline bool fast_cols_dispatch_group(int M, int T, Runner&& run) {
#define FC_X(MM, A, B, C, TT, NTT)                          \
    if (M == MM && T == TT) {                               \
        run.template go<ColCfg<MM, A, B, C, TT, NTT>>();    \
        return true;                                        \
    }
    FC_COL_CONFIGS_OF_GROUP(G, FC_X);
#undef FC_X
    return false;
}
// Forward column kernel (fast_cols_fwd.hpp): same configurations, with the pruned choice added: run.template go<Cfg, NZ2>()
// with NZ2 = 3 (pruned, short kernels; where R2 > 3) or R2 (any input length).
template <class Runner>
struct WithPrunedChoice {
    Runner& run;
    bool pruned;
    template <class Cfg>
    void go() {
        if constexpr (Cfg::R2 > 3) {
            if (pruned) { run.template go<Cfg, 3>(); return; }
        }
        run.template go<Cfg, Cfg::R2>();
    }
};
template <int G, class Runner>
inline bool fast_cols_fwd_dispatch_group(int M, int T, bool pruned, Runner&& run) {
    return fast_cols_dispatch_group<G>(M, T, WithPrunedChoice<std::remove_reference_t<Runner>>{run, pruned});
}

// may the pruned variant take columns of h_in samples?  (one non-zero input per stage-1 butterfly,
// at most 3 non-zero inputs per stage-2 butterfly)
inline bool fast_cols_fwd_pruned_ok(const FastColsInfo& fi, int h_in) {
    const int nz = (h_in + 1) / 2, m1 = fi.M / fi.R1;
    return fi.R2 > 3 && nz <= m1 && nz <= 3 * fi.R3;
}

// Typed image pixels (pixel_format.hpp; plan entry fftconv_plan_set_images_typed): the image's forward column kernel converts
// uint8 / uint16 / fp16 / bf16 elements in its load -- the full variant (NZ2 = R2) of every configuration, one instantiation per
// element size, the 16-bit format a uniform of the launch.  A configuration whose typed kernel spills registers, uses scratch
// or drops below the 3 waves per SIMD of its launch bounds in the build's reports (csrc/*.rpt) is NOT built and listed here:
// its plans convert the image into the fp32 staging first (kernels_pixels.hip), as every plan without the specialised forward
// column kernel does.  The list is EMPTY: all 32 configurations are within the bound for both element sizes (40 ... 125 VGPRs,
// 4 ... 8 waves per SIMD; tests/test_pixel_format_host.py holds the reports against it).
constexpr std::array<int, 0> FC_COLS_FWD_PX_NOT_BUILT{};
constexpr bool fast_cols_fwd_px_built(int M) {
    for (int x : FC_COLS_FWD_PX_NOT_BUILT)
        if (x == M) return false;
    return true;
}
inline bool fast_cols_fwd_px_available(int M) { return fast_cols_lookup(M).ok && fast_cols_fwd_px_built(M); }
// Whether a typed call on a plan with these settings converts in the column kernel's load (fftconv_plan::pixel_direct, read-only
// option "pixel_direct"): "pixel_store" 1 on a one-pass plan whose image column pass is the specialised kernel and has the
// typed instantiation.  Everything else is staged.
inline bool fast_cols_fwd_px_direct(bool pixel_store, bool blockwise, bool fast_fwd, int M) {
    return pixel_store && !blockwise && fast_fwd && fast_cols_fwd_px_available(M);
}
// The pixel uniforms of a typed forward column launch: the format, and the load form -- a pair of rows in one load only where
// pixel_pair_load_ok (pixel_format.hpp) says every pair of the launch is aligned for it
inline PixelLoad fast_cols_fwd_pixel_load(const FastColsFwdArgs& a, int format) {
    PixelLoad px;
    px.format = format;
    px.wide = pixel_pair_load_ok(reinterpret_cast<uintptr_t>(a.in), a.in_col_pitch, a.in_plane_stride, fc_pixel_elem_bytes(format)) ? 1 : 0;
    return px;
}

// Border modes (border.hpp; plan entry fftconv_plan_set_border): the image's forward column kernel maps the indices of the
// extended image in its load -- fp32 pixels, the full variant (NZ2 = R2) of every configuration, ONE instantiation per
// configuration, the mode a uniform of the launch.  A configuration whose bordered kernel spills registers, uses scratch or loses a
// wave per SIMD against its plain sibling in the build's reports (csrc/*.rpt) is NOT built and listed here: its plans take the
// staged route (kernels_pixels.hip: k_extend_image writes the extended image into the plan's staging), as every plan without the
// specialised forward column kernel does (tests/test_border_host.py holds the reports against the list).  Listed: 544 (the
// bordered kernel spills 28 registers into 116 bytes of scratch at 3 waves, its plain sibling holds 110 VGPRs at 4) and 1280, 1536,
// 1680, 2304 (7 waves per SIMD where the plain kernel has 8).  The other 27 keep their sibling's waves without spills.
constexpr std::array<int, 5> FC_COLS_FWD_BORDER_NOT_BUILT{544, 1280, 1536, 1680, 2304};
constexpr bool fast_cols_fwd_border_built(int M) {
    for (int x : FC_COLS_FWD_BORDER_NOT_BUILT)
        if (x == M) return false;
    return true;
}
inline bool fast_cols_fwd_border_available(int M) { return fast_cols_lookup(M).ok && fast_cols_fwd_border_built(M); }
// Whether an image on a plan with a border on and these settings is mapped in the column kernel's load (fftconv_plan::border_direct,
// read-only option "border_direct"): "border_store" 1 on a one-pass plan whose image column pass is the specialised kernel and has
// the bordered instantiation.  Everything else is staged.
inline bool fast_cols_fwd_border_direct(bool border_store, bool blockwise, bool fast_fwd, int M) {
    return border_store && !blockwise && fast_fwd && fast_cols_fwd_border_available(M);
}

// Sliced tail round of the output kernel (fast_cols.hpp, SLICED): for the small transforms (M <= 1056: the launches of
// small problems are a handful of rounds of tiles) a last, partial round of `rem` tiles on `want` persistent workgroups is
// cut into S = 2^k column slices per tile, S <= want / rem and at least 2 columns per slice.  Fills in the tail fields
// of `a` (and shrinks a.ntiles to the full rounds) and returns the grid to launch; false: launch unsliced.
constexpr int FC_SLICE_MAX_M = 1056;
inline bool fast_cols_slice_plan(int M, int T, int want, FastColsArgs& a, int& grid) {
    a.tail_first = a.tail_tiles = a.slice_shift = 0;
    if (!a.y_tiled || M > FC_SLICE_MAX_M || want < 2 || a.ntiles <= 0) return false;
    if (T & (T - 1)) return false;        // slices are power-of-two fractions of a tile ...
    const int full_rounds = a.ntiles / want, rem = a.ntiles - full_rounds * want;
    // (launches of less than one round stay whole: cfg1's 18 tiles as 144 two-column slices took 24.6 instead of 22.3 us
    //  per step -- every slice pays the tile's whole phase latency)
    if (rem == 0 || full_rounds == 0) return false;
    int shift = 0;
    // ... of an EVEN number of columns: the gather and the landing work on column pairs (fast_cols.hpp)
    while ((2 << shift) * rem <= want && (T >> (shift + 1)) >= 2 && ((T >> (shift + 1)) & 1) == 0) shift++;
    if (shift == 0) return false;
    a.tail_first = full_rounds * want;
    a.tail_tiles = rem;
    a.slice_shift = shift;
    a.ntiles = full_rounds * want;
    grid = want;
    return true;
}

// ---- Launch decisions: which instantiation a launch runs, with which arguments, on what grid.  Plain host code: the launchers
// ---- (kernels_*.inc) and the CPU tier's runners (tests/emu/emu_runners.hpp) both call these, so neither can drift from the other.

// Row kernel: f(std::bool_constant<LINEAR>{}) -- LINEAR is true for every configuration (RowCfg asserts that m1 is a whole number
// of half layout tiles), so there is nothing left to decide at run time and one instantiation per configuration
template <class Cfg, class F>
inline void fast_rows_visit_linear(const FastRowsArgs&, F&& f) {
    f(std::true_type{});
}
// Row kernels: `groups` workgroups of RPW rows by `walks` of per_wg kernels (the F = 1 grid; the forward rows use the groups alone);
// `flat`: the 1-D grid of the F > 1 walk, groups rounded up to whole rounds of the 8 XCDs
struct FastRowsGrid { int groups, walks, flat; };
inline FastRowsGrid fast_rows_grid(int rows, int rpw, int kernels, int per_wg) {
    const int groups = (rows + rpw - 1) / rpw, walks = (kernels + per_wg - 1) / per_wg;
    return {groups, walks, 8 * ((groups + 7) / 8) * walks};
}

// ---- Image batches (fftconv_plan_set_images): a launch of the spectral-row kernels covers `images` image spectra times the
// ---- kernels_per_image kernels of the launch.  The image coordinate is resolved by the __global__ wrappers with the functions
// ---- below -- scalar arithmetic on the uniform bases of the by-value arguments -- and the specialised bodies run unchanged on
// ---- ONE image (the generic body is handed the image in its map slot: rows_generic_slot).
// ---- Written once: the wrappers (kernels_rows_multi.inc, kernels.hip) and the CPU tier (tests/image_batch_host) call this text.
struct RowsWalk { int image, group, kernel0, nk; };   // kernels [kernel0, kernel0 + nk) of one image, for row group `group`
FC_HD int rows_images(int images) { return images > 1 ? images : 1; }
// F = 1 and the generic kernels: a 3-D grid (row group, walk, image) -- blockIdx.z is the image; the grid has exactly the
// walks of fast_rows_grid, so nk >= 1
FC_HD RowsWalk rows_walk_3d(int bx, int by, int bz, int kernels_per_image, int per_wg) {
    const int kernel0 = by * per_wg;
    return {bz, bx, kernel0, kernels_per_image - kernel0 < per_wg ? kernels_per_image - kernel0 : per_wg};
}
// F > 1: the XCD-aware 1-D grid of k_fast_rows_multi_f.  Blocks b and b + 8 share an XCD, XCD x walks the row groups x, x + 8, ...
// with the (image, walk) pair fastest and the image the slower of the two: the workgroups that read the same F rows of one
// image's spectrum still sit side by side on one L2.  `walks`: walks per image.  group >= groups: the padding of the last round
// of XCDs, no work.
FC_HD RowsWalk rows_walk_flat(int b, int groups, int walks, int images, int kernels_per_image, int per_wg) {
    const int xcd = b & 7, sq = b >> 3;
    const int per_group = walks * rows_images(images);
    const int gl = sq / per_group;
    const int iw = sq - gl * per_group;
    const int image = iw / walks;
    const int walk = iw - image * walks;
    const int kernel0 = walk * per_wg;
    return {image, gl * 8 + xcd, kernel0, kernels_per_image - kernel0 < per_wg ? kernels_per_image - kernel0 : per_wg};
}
// Image walk (fast_rows_images.hpp): a workgroup of (row group, kernel) walks the images [image0, image0 + ni) of the launch,
// iwalks walks of per_wg images each (the last one shorter: a walk never runs past the images of the launch).  Flat XCD-aware
// 1-D grid of 8 * ceil(groups / 8) * iwalks * kernels_per_image blocks as rows_walk_flat: blocks b and b + 8 share an XCD, XCD x
// takes the row groups x, x + 8, ...; within a row group the KERNEL is the fastest coordinate and the image walk the next, so
// the kernels_per_image workgroups that read the same image-spectrum rows sit side by side on one L2 (a speed assumption
// only).  group >= groups: the padding of the last round of XCDs, no work.
struct RowsImageWalk { int group, kernel, image0, ni; };
FC_HD int rows_image_walks(int images, int per_wg) { return (rows_images(images) + per_wg - 1) / per_wg; }
FC_HD RowsImageWalk rows_walk_images(int b, int groups, int kernels_per_image, int iwalks, int images, int per_wg) {
    const int xcd = b & 7, sq = b >> 3;
    const int per_group = iwalks * kernels_per_image;
    const int gl = sq / per_group;
    const int r = sq - gl * per_group;
    const int iw = r / kernels_per_image;
    const int image0 = iw * per_wg, left = rows_images(images) - image0;
    return {gl * 8 + xcd, r - iw * kernels_per_image, image0, left < per_wg ? left : per_wg};
}
inline int rows_images_grid(int groups, int kernels_per_image, int iwalks) { return 8 * ((groups + 7) / 8) * iwalks * kernels_per_image; }
// generic kernel (kernels_body.hpp: spectral_rows_body), grid (row, kernel of the image, image): the map's slot in Y, which the
// body splits again with SpectralRowsArgs::kernels_per_image
FC_HD int rows_generic_slot(int by, int bz, int kernels_per_image) { return bz * kernels_per_image + by; }
// the bases of one image of the launch: its spectrum, and its kernels_per_image slots of the intermediate (in place, in the
// wrapper's by-value copy of the arguments)
FC_HD void rows_shift_to_image(const c32*& S, c32*& Y, int image, size_t s_image_stride, int kernels_per_image, size_t y_kernel_stride) {
    S += (size_t)image * s_image_stride;
    Y += (size_t)(image * kernels_per_image) * y_kernel_stride;
}

// Persistent column kernels: as many workgroups as fit at once (LDS-limited), one or two per CU ...
inline int persistent_want(size_t lds_bytes, int nt, int num_cus) {
    const int by_lds = (int)(FC_LDS_BUDGET / lds_bytes), by_threads = 768 / nt;
    const int per_cu = by_lds < by_threads ? by_lds : by_threads;
    return num_cus * (per_cu < 1 ? 1 : per_cu);
}
// ... and no more than there are tiles
inline int persistent_grid(size_t lds_bytes, int nt, int num_cus, int ntiles) {
    const int want = persistent_want(lds_bytes, nt, num_cus);
    return ntiles < want ? ntiles : want;
}
// image-and-kernels pair launch with the dynamic tile queue: a counter each, or none
inline bool fast_cols_fwd_pair_queues_ok(const FastColsFwdArgs& a, const FastColsFwdArgs& b) {
    return (!a.queue && !b.queue) || (a.queue && b.queue && a.queue != b.queue);
}

// Output kernel: the instantiation fast_cols_body<Cfg, TILED, SLICED, DYN> of a launch, its arguments and its grid on `want`
// persistent workgroups.  Small transforms on the tiled intermediate deal a partial last round of tiles in column slices
// (fast_cols_slice_plan), statically: that wins over the dynamic tile queue (fast_cols.hpp; chunks of one tile per workgroup
// of an XCD), which the row-major intermediate ignores.
enum class FastColsVariant { ROW_MAJOR, TILED, TILED_SLICED, TILED_DYN };
// The plane a launch combines its maps with, on the host: the planes of the plan's images ([image][window column][pitch rows] fp32,
// plane_elems apart) multiplied into the values (Scale: D, Dc) or added to them with the constant of the map's kernel (Add: Q and
// consts, consts[0] the launch's first kernel).  Map m of the launch belongs to image (first + m) / per_image and, Add, takes
// consts[(first + m) % per_image].  The rectangle family's launch fills the device argument structs of fast_cols.hpp from it
// (fast_cols_norm_args, fast_cols_sqdiff_args); the crop / pad launchers of kernels.hpp take it as it is.
enum class PlaneKind { None, Scale, Add };
struct MapPlane {
    PlaneKind kind = PlaneKind::None;
    const float* plane = nullptr;
    const float* consts = nullptr;
    size_t plane_elems = 0;
    int pitch = 0, first = 0, per_image = 0;
};
inline FastColsNormArgs fast_cols_norm_args(const MapPlane& p) { return {p.plane, p.plane_elems, p.pitch, p.first, p.per_image}; }
inline FastColsSqdiffArgs fast_cols_sqdiff_args(const MapPlane& p) { return {p.plane, p.consts, p.plane_elems, p.pitch, p.first, p.per_image}; }
struct FastColsShape {
    FastColsVariant variant;
    FastColsArgs a;
    int grid;
    MapPlane plane{};          // the rectangle family's fused scale / additive store only (fast_cols_rect_launch_shape below)
    bool strided = false;      // the strided store (fast_cols_stride_launch_shape below): the launch is k_fast_cols_stride's, with `stride`
    FastColsStrideArgs stride{};
    FastColsExtremaArgs extrema{};      // per-map extrema found in the store (launch_fast_cols_rect_extrema, kernels.hpp): where the waves' partials go
};
inline FastColsShape fast_cols_launch_shape(int M, int T, const FastColsArgs& a, int want) {
    FastColsShape r{FastColsVariant::TILED_SLICED, a, 0};
    r.a.queue = nullptr;
    if (fast_cols_slice_plan(M, T, want, r.a, r.grid)) return r;
    r.a = a;
    r.grid = a.ntiles < want ? a.ntiles : want;
    r.variant = !a.y_tiled ? FastColsVariant::ROW_MAJOR : a.queue ? FastColsVariant::TILED_DYN : FastColsVariant::TILED;
    if (r.variant == FastColsVariant::TILED_DYN) {
        r.a.queue_shift = 0;
        while ((16 << r.a.queue_shift) <= r.grid) r.a.queue_shift++;
    }
    return r;
}
// f(bool_constant<TILED>, bool_constant<SLICED>, bool_constant<DYN>) of a variant (SLICED exists for the small transforms only)
template <class Cfg, class F>
inline void fast_cols_visit_variant(FastColsVariant v, F&& f) {
    using yes = std::true_type;
    using no = std::false_type;
    if (v == FastColsVariant::TILED) f(yes{}, no{}, no{});
    else if (v == FastColsVariant::TILED_SLICED) { if constexpr (Cfg::M <= FC_SLICE_MAX_M) f(yes{}, yes{}, no{}); }
    else if (v == FastColsVariant::TILED_DYN) f(yes{}, no{}, yes{});
    else f(no{}, no{}, no{});
}

// Rectangle store (fast_cols.hpp: RECT; plan entry fftconv_plan_set_output_rect): the output kernel writes the dense maps of
// rows [off_h, off_h + out_h) of columns [off_w, off_w + out_w) of the window itself.  Instantiated for the tiled intermediate,
// unsliced, static deal and dynamic queue.  Two configurations are NOT built, because their rectangle kernels would spill
// registers (M = 544: 10-12 VGPRs where the plain kernel spills none; M = 2080: one more than the plain kernel's 4 with 16-bit
// maps -- the own kernels of the 1088 / 4160 windows, which only exact_window plans run): their plans crop the staged
// window, as every plan without the specialised kernel does.
constexpr bool fast_cols_rect_built(int M) { return M != 544 && M != 2080; }
inline bool fast_cols_rect_available(int M, bool y_tiled) { return y_tiled && fast_cols_lookup(M).ok && fast_cols_rect_built(M); }
// The launch of nk rectangle maps: `a` as fast_cols_args gives it for nk whole windows, with `out` the first dense
// rectangle map and out_kernel_stride the elements between two of them (>= out_h * out_w).  Only the tiles that hold a column
// of the rectangle are launched (the others are never gathered or transformed); the pair store is kept where every pair of
// rows is whole and aligned -- off_h, out_h, the map stride and the element offset of `out` from a pair boundary all even --
// which is uniform over the launch.  The rectangle must lie inside the window (pipeline.hpp: output_rect_error).
// `plane`: the fused scale of normalised maps (fast_cols.hpp: NORM) or the fused additive store of score 4 (ADD) -- fp32 maps, the
// rectangle the plan's or, on a plan without one, the whole window (which keeps the pair stores).
inline FastColsShape fast_cols_rect_launch_shape(int T, const FastColsArgs& a, int off_h, int off_w, int out_h, int out_w, int want, const MapPlane& plane = {}) {
    FastColsShape r{a.queue ? FastColsVariant::TILED_DYN : FastColsVariant::TILED, a, 0, plane};
    const int nk = a.tiles_per_kernel > 0 ? a.ntiles / a.tiles_per_kernel : 0;
    const int tile_lo = off_w / T, tile_hi = (off_w + out_w + T - 1) / T;
    r.a.h_lo = off_h; r.a.fft_h = off_h + out_h; r.a.out_pitch = out_h;
    r.a.w_first = tile_lo * T; r.a.tiles_per_kernel = tile_hi - tile_lo; r.a.ntiles = r.a.tiles_per_kernel * nk;
    r.a.rect_w_lo = off_w; r.a.rect_w_n = out_w;
    const size_t elem = fc_map_elem_bytes(a.out_format);
    r.a.rect_wide = (off_h % 2 == 0 && out_h % 2 == 0 && a.out_kernel_stride % 2 == 0 && reinterpret_cast<uintptr_t>(a.out) % (2 * elem) == 0) ? 1 : 0;
    r.a.tail_first = r.a.tail_tiles = r.a.slice_shift = 0;
    r.grid = r.a.ntiles < want ? r.a.ntiles : want;
    if (r.variant == FastColsVariant::TILED_DYN) {
        r.a.queue_shift = 0;
        while ((16 << r.a.queue_shift) <= r.grid) r.a.queue_shift++;
    }
    return r;
}

// Strided store (fast_cols.hpp: STRIDE; plan entry fftconv_plan_set_output_stride): the fp32 rectangle kernel stores every sh-th row
// and sw-th column of the extent, counted from its first row and column.  Built by the family's rule: a configuration whose kernel
// spills a vector register, uses scratch or drops below 3 waves per SIMD in the build's reports (csrc/kernels_cols_stride_g*.rpt) is
// NOT built and listed here; its plans sample while the staged window is cropped.  M = 544 and 2080 started here: their rectangle
// kernels are not built either.
constexpr int FC_COLS_STRIDE_NOT_BUILT[] = {544, 2080};
constexpr bool fast_cols_stride_built(int M) {
    for (int x : FC_COLS_STRIDE_NOT_BUILT)
        if (x == M) return false;
    return true;
}
inline bool fast_cols_stride_available(int M, bool y_tiled) { return y_tiled && fast_cols_lookup(M).ok && fast_cols_stride_built(M); }
// rows or columns of an extent of n sampled at `step` from its first one
constexpr int strided_count(int n, int step) { return (n + step - 1) / step; }
// a step with what replaces the division by it in the kernel (fast_cols.hpp: StrideDiv); n: what it samples -- a step beyond n
// samples the first element alone, as n does, and n < 2^16 keeps the reciprocal exact
inline StrideDiv stride_div(int step, int n) {
    StrideDiv d;
    d.step = step < n ? step : n;
    if ((d.step & (d.step - 1)) == 0) {
        d.shift = 0;
        while ((1 << d.shift) < d.step) d.shift++;
        d.mask = (unsigned)d.step - 1u;
    } else {
        d.shift = -1;
        d.rcp = (unsigned)((((unsigned long long)1 << 32) + (unsigned)d.step - 1u) / (unsigned)d.step);
    }
    return d;
}
// The launch of nk strided maps: `a` as for fast_cols_rect_launch_shape, with `out` the first dense strided map and out_kernel_stride
// the elements between two of them (>= ceil(out_h / sh) * ceil(out_w / sw)); the extent (off_h, off_w, out_h, out_w) is the
// UNSAMPLED one.  Only tiles that hold a sampled column are launched: for sw <= T RECT's contiguous range, ending at the tile of the
// last sampled column; for sw > T one tile per sampled column (FastColsStrideArgs::tile_step).  sh == 1 keeps RECT's stores, the
// pair store under RECT's conditions; sh >= 2 stores elements.  fp32 maps only (launch_fast_cols_rect refuses the others), extents
// of fewer than 2^16 rows and columns (every one-pass window).
inline FastColsShape fast_cols_stride_launch_shape(int T, const FastColsArgs& a, int off_h, int off_w, int out_h, int out_w, int sh, int sw, int want) {
    const int nw = strided_count(out_w, sw), last_w = off_w + (nw - 1) * (sw < out_w ? sw : out_w);
    FastColsShape r = fast_cols_rect_launch_shape(T, a, off_h, off_w, out_h, last_w - off_w + 1, want);
    r.strided = true;
    r.stride.h = stride_div(sh, out_h);
    r.stride.w = stride_div(sw, out_w);
    r.a.out_pitch = strided_count(out_h, sh);
    if (r.stride.h.step != 1) r.a.rect_wide = 0;
    if (r.stride.w.step > T) {
        const int nk = a.tiles_per_kernel > 0 ? a.ntiles / a.tiles_per_kernel : 0;
        r.stride.tile_step = r.stride.w.step;
        r.a.tiles_per_kernel = nw; r.a.ntiles = nw * nk;
        r.grid = r.a.ntiles < want ? r.a.ntiles : want;
        if (r.variant == FastColsVariant::TILED_DYN) {
            r.a.queue_shift = 0;
            while ((16 << r.a.queue_shift) <= r.grid) r.a.queue_shift++;
        }
    }
    return r;
}

// Fused scale of normalised maps (fast_cols.hpp: NORM; plan entry fftconv_plan_set_normalisation): the fp32 rectangle kernel
// multiplies every value pair by the scale plane D at its window coordinate ahead of the store.  A configuration whose kernel
// spills registers, uses scratch or drops below the 3 waves per SIMD of its launch bounds in the build's reports (csrc/*.rpt) is
// NOT built and listed here: its plans scale the staged window while it is cropped (kernels_ncc.hip), as every plan without
// the specialised kernel does.  M = 544 and 2080 started here: their rectangle kernels are not built either.
constexpr int FC_COLS_NORM_NOT_BUILT[] = {544, 2080};
constexpr bool fast_cols_norm_built(int M) {
    for (int x : FC_COLS_NORM_NOT_BUILT)
        if (x == M) return false;
    return true;
}
inline bool fast_cols_norm_available(int M, bool y_tiled) { return y_tiled && fast_cols_lookup(M).ok && fast_cols_norm_built(M); }

// Fused additive store of matching score 4, SQDIFF (fast_cols.hpp: ADD; plan entry fftconv_plan_set_match_score): the fp32 rectangle
// kernel stores v + (Q + c) -- the plane Q at the pair's window coordinate, c the constant of the map's kernel.  Built by the NORM
// family's rule: a configuration whose kernel spills a vector register, uses scratch or drops below 3 waves per SIMD in the build's
// reports (csrc/kernels_cols_sqdiff_g*.rpt) is NOT built and listed here; its plans add while the staged window is cropped.
constexpr int FC_COLS_SQDIFF_NOT_BUILT[] = {544, 2080};
constexpr bool fast_cols_sqdiff_built(int M) {
    for (int x : FC_COLS_SQDIFF_NOT_BUILT)
        if (x == M) return false;
    return true;
}
inline bool fast_cols_sqdiff_available(int M, bool y_tiled) { return y_tiled && fast_cols_lookup(M).ok && fast_cols_sqdiff_built(M); }
// (whether a group's maps take the fused store or the staged combination: output_route.hpp)

// Per-map extrema found in the store (fast_cols.hpp: EXT; plan entry fftconv_plan_set_extrema): the three fp32 rectangle stores -- RECT
// (raw maps and score 2; the whole window too), RECT_SCALE (scores 1 and 3), RECT_ADD (score 4) -- with a running (max, index) and (min,
// index) per thread and a cross-lane reduction per wave and tile.  Built by the family's rule, against the sibling of the same
// store: a configuration whose kernel spills a vector register, uses scratch or holds a wave per SIMD less than its sibling in the
// build's reports (csrc/kernels_cols_*ext_g*.rpt) is NOT built and listed here; its plans find the extrema with the scan kernel
// (kernels_extrema.hip), as every route the fused store does not serve.  M = 544 and 2080 started here: their siblings are not built.
// The running pairs cost 2 ... 11 registers; what that did at the register steps of a wave per SIMD (VGPRs and waves per SIMD of the EXT
// kernel against its sibling's, static deal / dynamic queue where they differ):
//   RECT    640 static 84 / 5 against 78 / 6; 480 dynamic 83 / 5 against 79 / 6; 240 dynamic 83 / 5 against 79 / 6
//   SCALE   3072 static spills 1 register (8 bytes of scratch) at 128; 1152 dynamic 100 / 4 against 89 / 5; 768 dynamic 98 / 4 against
//           91 / 5; 480 and 240 dynamic 83 / 5 against 79 / 6
//   ADD     3072 static spills 1 register at 128; 1536 dynamic 98 / 4 against 95 / 5; 1152 101 / 4 and 97 / 4 against 91 / 5 and 88 / 5;
//           768 101 / 4 and 98 / 4 against 91 / 5 and 88 / 5; 480 84 / 5 and 81 / 5 against 79 / 6 and 76 / 6; 240 dynamic 83 / 5
//           against 79 / 6; 144 static 65 / 7 against 56 / 8
// Every other configuration keeps its sibling's waves without a spill (+2 ... +11 registers: 154 at M = 4224, 157 / 159 at 2112, 92 / 95
// at 576).  (tests/test_extrema_host.py holds the reports against the lists.)
constexpr int FC_COLS_RECT_EXT_NOT_BUILT[] = {544, 2080, 640, 480, 240};
constexpr int FC_COLS_NORM_EXT_NOT_BUILT[] = {544, 2080, 3072, 1152, 768, 480, 240};
constexpr int FC_COLS_SQDIFF_EXT_NOT_BUILT[] = {544, 2080, 3072, 1536, 1152, 768, 480, 240, 144};
constexpr bool fast_cols_rect_ext_built(int M) {
    for (int x : FC_COLS_RECT_EXT_NOT_BUILT)
        if (x == M) return false;
    return fast_cols_rect_built(M);
}
constexpr bool fast_cols_norm_ext_built(int M) {
    for (int x : FC_COLS_NORM_EXT_NOT_BUILT)
        if (x == M) return false;
    return fast_cols_norm_built(M);
}
constexpr bool fast_cols_sqdiff_ext_built(int M) {
    for (int x : FC_COLS_SQDIFF_EXT_NOT_BUILT)
        if (x == M) return false;
    return fast_cols_sqdiff_built(M);
}
// slots of the partials one map of a fused launch fills: the tiles that hold a column of it x the waves of a workgroup
inline int fast_cols_extrema_slots(const FastColsShape& sh, int NT) { return sh.a.tiles_per_kernel * (NT / 64); }

struct FastColsTables {
    Plan1D plan;                   // radices (R1, R2, R3)
    std::vector<c32> tw1, tw2;
    std::vector<PairEntry> pairs;  // positions in the fast plan's order
    std::vector<int> rowoff;       // M+1: row-major Y: row offset feeding LDS position p
    std::vector<int> pair_row_of;  // M+1: spectrum row i (producer order) -> row of the pair-adjacent tiled intermediate
};

// `producer`: the plan whose digit-reversed order the spectrum rows are produced in.
inline FastColsTables make_fast_cols_tables(const FastColsInfo& fi, const Plan1D& producer, int y_pitch) {
    FastColsTables t;
    t.plan = make_plan1d_seq(fi.M, {fi.R1, fi.R2, fi.R3});
    const int m1 = fi.M / fi.R1;
    const StageDesc& s1 = t.plan.desc.st[0];
    const StageDesc& s2 = t.plan.desc.st[1];
    t.tw1.assign(t.plan.tw.begin() + s1.tw_off, t.plan.tw.begin() + s1.tw_off + m1);
    t.tw2.assign(t.plan.tw.begin() + s2.tw_off, t.plan.tw.begin() + s2.tw_off + (fi.R2 - 1) * fi.R3);
    t.pairs = make_pair_table(t.plan);
    t.rowoff.assign(fi.M + 1, 0);
    for (int k = 0; k < fi.M; k++) t.rowoff[t.plan.pos[k]] = producer.pos[k] * y_pitch;
    t.rowoff[fi.M] = fi.M * y_pitch;
    // pair-adjacent tile rows: pair p = (bin p, bin M-p) at rows 2p, 2p+1;
    // p = 0: (DC, Nyquist); p = M/2: (middle bin, padding)
    t.pair_row_of.assign(fi.M + 1, 0);
    for (int k = 0; k < fi.M; k++) {
        int r = (k <= fi.M / 2) ? 2 * k : 2 * (fi.M - k) + 1;
        t.pair_row_of[producer.pos[k]] = r;
    }
    t.pair_row_of[fi.M] = 1;
    return t;
}

}  // namespace fc
