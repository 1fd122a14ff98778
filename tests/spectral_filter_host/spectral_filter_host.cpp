// spectral_filter_host.cpp -- TEST-ONLY stand-alone host program for the spectral filters (fftconv_plan_set_spectral_filter).
//
// Built by tests/test_spectral_filter_host.py with the host compiler from the product's headers and the phase context of
// tests/emu/emu_runners.hpp; it is not the emulator library and not part of the product.  Modes:
//   point    the pointwise function of csrc/spectral_filter.hpp on edge bins (P = 0, K = 0 with lambda = 0, denominators near the
//            fp32 extremes: 0 or finite, never NaN or inf), on ordinary bins against float64, and the setter's argument check
//   rows     fast_rows_multi_body with FILTER = true at five lengths through the wrapper's own text, and the generic body at a small
//            length, each in modes 1 and 2: every row of the first, a middle and the last (partial) row group against a float64 row
//            computation of the definition; walks of several maps and of one map write the same bits; nothing is written outside the
//            launch's slots; with the switch at mode 0 the FILTER body is bit-equal to the plain body.  The error bar of a mode is
//            relative to the plain product's own error against float64 at the same configuration: RATIO_BAR below.
// Having its own main, it is also the place for a host sanitizer build (-fsanitize=address,undefined) of this code.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "emu_runners.hpp"

using namespace fc;
using emu::HostPhaseCtx;
using cd = std::complex<double>;

namespace {

int g_failures = 0, g_ok = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            g_failures++;                                 \
            printf("FAIL ");                              \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
        } else g_ok++;                                    \
    } while (0)

// Twice the largest ratio (error of the mode) / (error of the plain product), both against float64 and each relative to its own
// row's largest magnitude, measured over the configurations of cmd_rows on random rows: phase 1.24 ... 1.50 (largest at 288), Wiener
// 3.83 ... 5.55 (largest at 2112) -- tests/test_spectral_filter_host.py quotes them per configuration.  Index: the mode.
const double RATIO_BAR[3] = {1.0, 3.0, 11.1};

// ---------------------------------------------------------------- point
bool finite2(c32 v) { return std::isfinite(v.x) && std::isfinite(v.y); }
bool zero2(c32 v) { return v.x == 0.f && v.y == 0.f; }

int cmd_point() {
    const float c = 1.0f / (288.f * 288.f);
    // P = 0: a zero kernel bin, a zero image bin, both
    CHECK(zero2(spectral_filter_phase(mk(0.f, 0.f), mk(0.3f, -0.2f), c)), "phase: K = 0 gives 0");
    CHECK(zero2(spectral_filter_phase(mk(1.5f, 2.f), mk(0.f, 0.f), c)), "phase: I = 0 gives 0");
    CHECK(zero2(spectral_filter_phase(mk(0.f, 0.f), mk(0.f, 0.f), c)), "phase: 0 . 0 gives 0");
    CHECK(zero2(spectral_filter_phase(mk(-0.f, 0.f), mk(0.f, -0.f), c)), "phase: signed zeros give 0");
    // lambda = 0 with K = 0: 0, whatever the image bin
    CHECK(zero2(spectral_filter_wiener(mk(0.f, 0.f), mk(0.7f, 0.1f), 0.f)), "wiener: K = 0, lambda = 0 gives 0");
    CHECK(zero2(spectral_filter_wiener(mk(0.f, 0.f), mk(0.f, 0.f), 0.f)), "wiener: all zero gives 0");
    // K = 0 with lambda > 0: the numerator is 0
    CHECK(zero2(spectral_filter_wiener(mk(0.f, 0.f), mk(0.7f, 0.1f), 1e-3f)), "wiener: K = 0, lambda > 0 gives 0");
    // denominators near the extremes: |K|^2 + lambda and |P_s|^2 up to and past FLT_MAX (the bins themselves finite in every product),
    // and down to and below FLT_MIN
    const float big[] = {1e18f, 1e19f, 1.3e19f, 1.5e19f, 3e19f}, small[] = {1e-18f, 1.1e-19f, 1e-19f, 2e-19f, 1e-22f, 1e-38f, 1e-42f};
    for (float b : big)
        for (float sv : {1.f, 1e-7f, -3.f}) {
            const c32 w = spectral_filter_wiener(mk(b, -b), mk(sv, 0.5f * sv), 0.f), w2 = spectral_filter_wiener(mk(1.f, 1.f), mk(sv, sv), b);
            const c32 p = spectral_filter_phase(mk(b, b), mk(sv, -sv), c);
            CHECK(finite2(w) && finite2(w2) && finite2(p), "large bin %g, image %g: wiener (%g, %g), lambda (%g, %g), phase (%g, %g)", (double)b, (double)sv, (double)w.x,
                  (double)w.y, (double)w2.x, (double)w2.y, (double)p.x, (double)p.y);
        }
    for (float e : small)
        for (float sv : {1.f, 1e-7f, -3.f}) {
            const c32 w = spectral_filter_wiener(mk(e, -e), mk(sv, 0.5f * sv), 0.f), w2 = spectral_filter_wiener(mk(e, e), mk(sv, sv), e * e);
            const c32 p = spectral_filter_phase(mk(e, e), mk(sv * e, -sv), c);
            CHECK(finite2(w) && finite2(w2) && finite2(p), "small bin %g, image %g: wiener (%g, %g), lambda (%g, %g), phase (%g, %g)", (double)e, (double)sv, (double)w.x,
                  (double)w.y, (double)w2.x, (double)w2.y, (double)p.x, (double)p.y);
        }
    // ordinary bins against float64
    uint32_t seed = 99u;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (float)((int32_t)(seed >> 8) - (1 << 23)) / (float)(1 << 23); };
    double worst_p = 0, worst_w = 0, worst_m = 0;
    for (int i = 0; i < 20000; i++) {
        const c32 k = mk(40.f * rnd(), 40.f * rnd()), s = mk(c * 300.f * rnd(), c * 300.f * rnd());
        const float lam = 0.5f + 0.5f * rnd() + 1.0f;
        const cd K(k.x, k.y), S(s.x, s.y), P = K * S;
        if (std::abs(P) < 1e-6 * c) continue;
        const cd rp = (double)c * P / std::abs(P), rw = S * std::conj(K) / (std::norm(K) + (double)lam);
        const c32 gp = spectral_filter_phase(k, s, c), gw = spectral_filter_wiener(k, s, lam), gm = spectral_filter_apply(0, 0.f, k, s);
        worst_p = std::max(worst_p, std::abs(cd(gp.x, gp.y) - rp) / (double)c);
        worst_w = std::max(worst_w, std::abs(cd(gw.x, gw.y) - rw) / std::abs(rw));
        worst_m = std::max(worst_m, std::abs(cd(gm.x, gm.y) - P) / std::abs(P));
        const c32 ap = spectral_filter_apply(1, c, k, s), aw = spectral_filter_apply(2, lam, k, s);
        if (memcmp(&ap, &gp, sizeof(c32)) || memcmp(&aw, &gw, sizeof(c32))) { CHECK(false, "spectral_filter_apply is not the mode's function"); break; }
    }
    CHECK(worst_p < 2e-6 && worst_w < 2e-6 && worst_m < 1e-6, "ordinary bins against float64: phase %.3g, wiener %.3g, product %.3g", worst_p, worst_w, worst_m);
    // the uniform of a launch
    CHECK(spectral_filter_launch_param(1, 5.f, 288, 384) == (float)(1.0 / (288.0 * 384.0)) && spectral_filter_launch_param(2, 5.f, 288, 384) == 5.f &&
              spectral_filter_launch_param(0, 5.f, 288, 384) == 0.f, "launch parameter");
    // the setter's argument check
    const float inf = INFINITY, nan = NAN;
    CHECK(!spectral_filter_args_error(0, 0.f) && !spectral_filter_args_error(1, 0.f) && !spectral_filter_args_error(2, 0.f) && !spectral_filter_args_error(2, 3.5f),
          "valid arguments");
    CHECK(spectral_filter_args_error(-1, 0.f) && spectral_filter_args_error(3, 0.f) && spectral_filter_args_error(1, 1e-3f) && spectral_filter_args_error(2, -1e-3f) &&
              spectral_filter_args_error(2, inf) && spectral_filter_args_error(2, nan) && spectral_filter_args_error(1, nan) && spectral_filter_args_error(0, inf),
          "refused arguments");
    printf("%d ok, %d failed\n%s\n", g_ok, g_failures, g_failures ? "FAILED" : "pointwise function ok");
    return g_failures ? 1 : 0;
}

// ---------------------------------------------------------------- rows
float rnd(uint32_t& s) {
    s = s * 1664525u + 1013904223u;
    return (float)((int32_t)(s >> 8) - (1 << 23)) / (float)(1 << 23);
}
constexpr size_t GUARD = 96;                    // poisoned c32 in front of and behind the launch's slots
const c32 POISON = {-7.0e37f, 7.5e37f};
bool same_bits(const c32& a, const c32& b) { return memcmp(&a, &b, sizeof(c32)) == 0; }

// element (row i, column w) of a map of the intermediate
size_t y_index(const Geometry& g, const Tables& t, int i, int w) {
    if (!g.y_tiled()) return (size_t)i * g.y_pitch + w;
    const int TL = g.y_tile_w;
    return (size_t)(w / TL) * (g.tile_rows() * TL) + (size_t)t.fcl.pair_row_of[i] * TL + (w % TL);
}

// the definition on one row, in float64: the kernel row x (kw entries) transformed, the filter against the stored image-spectrum row,
// the unnormalised inverse transform; returns the largest magnitude of the row
double reference_row(const Geometry& g, const Tables& t, const std::vector<cd>& tw, const c32* x, int kw, const c32* srow, int mode, float param,
                     std::vector<cd>& X, std::vector<cd>& ref) {
    const int L = g.Lw;
    for (int k = 0; k < L; k++) {
        cd K = 0;
        for (int j = 0; j < kw; j++) K += cd(x[j].x, x[j].y) * std::conj(tw[(size_t)j * k % L]);
        const c32 sv = srow[t.nat_col_of[k]];
        const cd S(sv.x, sv.y), P = K * S;
        if (mode == FC_FILTER_PHASE) X[k] = std::abs(P) > 0 ? (double)param * P / std::abs(P) : cd(0);
        else if (mode == FC_FILTER_WIENER) X[k] = std::norm(K) + (double)param > 0 ? S * std::conj(K) / (std::norm(K) + (double)param) : cd(0);
        else X[k] = P;
    }
    double top = 0;
    for (int w = 0; w < g.wout; w++) {
        cd acc = 0;
        for (int k = 0; k < L; k++) acc += X[k] * tw[(size_t)k * w % L];
        ref[w] = acc;
        top = std::max(top, std::abs(acc));
    }
    return top;
}

struct Shape { int H, W, kh, kw, path_mode, fft_h, fft_w, wout; bool tiled; };

struct RowData {
    Geometry g;
    Tables t;
    DeviceTables d;
    std::vector<c32> A, S;
    std::vector<cd> tw;
    std::vector<int> check_rows;
    size_t per_a, ye;
    float lambda, c;
    int kw, nk;
};

// random kernel rows and a random image spectrum; lambda = 1e-3 of the mean |K^|^2 of the rows (Parseval: the mean energy of a row)
void fill(RowData& r, int kw, int nk, int rpw, uint32_t seed) {
    const Geometry& g = r.g;
    r.kw = kw; r.nk = nk;
    r.per_a = (size_t)g.rows * a_pitch_for(kw); r.ye = g.y_elems_per_kernel();
    r.A.resize(r.per_a * nk); r.S.resize(g.spectrum_elems());
    double energy = 0;
    for (c32& v : r.A) v = mk(rnd(seed), rnd(seed));
    for (int k = 0; k < nk; k++)
        for (int row = 0; row < g.rows; row++)
            for (int j = 0; j < kw; j++) {
                const c32 v = r.A[(size_t)k * r.per_a + (size_t)row * a_pitch_for(kw) + j];
                energy += (double)v.x * v.x + (double)v.y * v.y;
            }
    r.lambda = (float)(1e-3 * energy / ((double)nk * g.rows));
    r.c = spectral_filter_launch_param(FC_FILTER_PHASE, 0.f, g.Lh, g.Lw);
    for (c32& v : r.S) v = mk(r.c * 50.f * rnd(seed), r.c * 50.f * rnd(seed));
    r.tw.resize(g.Lw);
    for (int n = 0; n < g.Lw; n++) r.tw[n] = std::polar(1.0, 2.0 * M_PI * n / g.Lw);
    const int groups = (g.rows + rpw - 1) / rpw;
    for (int grp : {0, groups / 2, groups - 1})
        for (int rr = 0; rr < rpw; rr++)
            if (grp * rpw + rr < g.rows && (r.check_rows.empty() || r.check_rows.back() < grp * rpw + rr)) r.check_rows.push_back(grp * rpw + rr);
}

// largest error of the maps at Y (behind the guard) against the definition, relative to each row's own largest magnitude
double error_against_definition(const RowData& r, const std::vector<c32>& Y, int mode, float param) {
    const Geometry& g = r.g;
    std::vector<cd> X(g.Lw), ref(g.wout);
    double err = 0;
    for (int k : {0, r.nk - 1})
        for (int row : r.check_rows) {
            const double top = reference_row(g, r.t, r.tw, r.A.data() + (size_t)k * r.per_a + (size_t)row * a_pitch_for(r.kw), r.kw, r.S.data() + (size_t)row * g.s_pitch,
                                             mode, param, X, ref);
            for (int w = 0; w < g.wout; w++) {
                const c32 a = Y[GUARD + (size_t)k * r.ye + y_index(g, r.t, row, w)];
                err = std::max(err, std::abs(cd(a.x, a.y) - ref[w]) / top);
            }
        }
    return err;
}

void bands(const std::vector<c32>& Y, size_t slots, size_t& stray, size_t& written) {
    stray = written = 0;
    for (size_t i = 0; i < GUARD; i++) stray += !same_bits(Y[i], POISON) + !same_bits(Y[GUARD + slots + i], POISON);
    for (size_t i = 0; i < slots; i++) written += !same_bits(Y[GUARD + i], POISON);
}

void judge(const char* what, const RowData& r, const std::vector<c32>& plain, const std::vector<c32>& mode0, const std::vector<c32> (&walk)[3],
           const std::vector<c32> (&one)[3]) {
    const bool mode0_equal = memcmp(plain.data(), mode0.data(), plain.size() * sizeof(c32)) == 0;
    CHECK(mode0_equal, "%s: the filter body at mode 0 is not the plain body's bits", what);
    const double err_plain = error_against_definition(r, plain, 0, 0.f);
    // (the plain body itself must be a float32 transform of that row: a reference with the wrong order or sign fails here)
    CHECK(err_plain < 1e-5, "%s: plain product against float64: %.3g", what, err_plain);
    double ratio[3] = {0, 0, 0};
    for (int mode : {FC_FILTER_PHASE, FC_FILTER_WIENER}) {
        const float param = mode == FC_FILTER_PHASE ? r.c : r.lambda;
        size_t stray = 0, written = 0;
        bands(walk[mode], r.ye * r.nk, stray, written);
        const bool walks_equal = memcmp(walk[mode].data(), one[mode].data(), walk[mode].size() * sizeof(c32)) == 0;
        const bool differs = memcmp(walk[mode].data(), plain.data(), plain.size() * sizeof(c32)) != 0;
        CHECK(walks_equal && stray == 0 && written > 0 && differs, "%s mode %d: walks of several maps and of one equal %d, stray stores %zu, written %zu, differs from the product %d",
              what, mode, walks_equal, stray, written, differs);
        const double err = error_against_definition(r, walk[mode], mode, param);
        ratio[mode] = err / err_plain;
        CHECK(err <= RATIO_BAR[mode] * err_plain, "%s mode %d: error against the float64 definition %.3g, plain product %.3g: ratio %.2f (bar %.1f)", what, mode, err,
              err_plain, ratio[mode], RATIO_BAR[mode]);
    }
    printf("ok   %s: mode 0 bit-equal to the plain body, walks bit-equal, bands intact; plain error %.3g, ratio phase %.2f, ratio wiener %.2f (lambda %.3g)\n", what,
           err_plain, ratio[1], ratio[2], (double)r.lambda);
}

template <class Cfg, int NZ2>
void run_fast(const Shape& sh, int nk) {
    PlanTuning tune;
    tune.path_mode = sh.path_mode;
    RowData r;
    Geometry& g = r.g;
    char what[96];
    snprintf(what, sizeof(what), "L=%d (%dx%d (*) %dx%d) nk=%d", Cfg::L, sh.H, sh.W, sh.kh, sh.kw, nk);
    if (!make_geometry(g, r.t, sh.H, sh.W, 1, sh.kh, sh.kw, tune) || !g.fast_rows.ok || g.Lh != sh.fft_h || g.Lw != Cfg::L || g.Lw != sh.fft_w ||
        g.fast_rows.RPW != Cfg::RPW || g.fast_rows.NT != Cfg::NT || g.fast_rows.R1 != Cfg::R1 || g.fast_rows.R3 != Cfg::R3 || g.wout != sh.wout ||
        g.y_tiled() != sh.tiled || fast_rows_nz2(g, sh.kw) > NZ2 || !fast_rows_filter_built(Cfg::L)) {
        CHECK(false, "%s: the plan does not run the configuration this case names (transform %d x %d, window %d, tiled %d)", what, g.Lh, g.Lw, g.wout, (int)g.y_tiled());
        return;
    }
    r.d.fr_tw1 = r.t.fr.tw1.data(); r.d.fr_tw2 = r.t.fr.tw2.data(); r.d.fr_relayout = r.t.fr.relayout.data();
    if (g.fast_cols.ok) r.d.fc_pair_row_of = r.t.fcl.pair_row_of.data();
    fill(r, sh.kw, nk, Cfg::RPW, 777u + (uint32_t)Cfg::L);
    std::vector<c32> lds(FC_LDS_BUDGET / sizeof(c32));
    // the wrapper's text (kernels_rows_filter.inc: k_fast_rows_filter; kernels_rows_multi.inc: k_fast_rows_multi) over the grid of a launch
    auto launch = [&](std::vector<c32>& Y, bool filter, int mode, float param, int per_wg) {
        FastRowsArgs base = fast_rows_args(g, r.d, r.A.data(), sh.kw, r.S.data(), Y.data() + GUARD);
        base.filter_mode = mode; base.filter_param = param;
        const FastRowsGrid grid = fast_rows_grid(g.rows, Cfg::RPW, nk, per_wg);
        for (int by = 0; by < grid.walks; by++)
            for (int bx = 0; bx < grid.groups; bx++) {
                FastRowsArgs a = base;
                const RowsWalk w = rows_walk_3d(bx, by, 0, nk, per_wg);
                rows_shift_to_image(a.S, a.Y, w.image, a.s_image_stride, nk, a.y_kernel_stride);
                for (int i = 0; i < Cfg::LDS_ELEMS; i++) lds[i] = mk(1e30f, -1e30f);
                if (filter) {
                    HostPhaseCtx<RowMultiState<Cfg, false, true>> ctx(Cfg::NT);
                    fast_rows_multi_body<Cfg, NZ2, true, false, true>(ctx, lds.data(), a, w.group, w.kernel0, w.nk, g.rows);
                } else {
                    HostPhaseCtx<RowMultiState<Cfg>> ctx(Cfg::NT);
                    fast_rows_multi_body<Cfg, NZ2, true>(ctx, lds.data(), a, w.group, w.kernel0, w.nk, g.rows);
                }
            }
    };
    const std::vector<c32> blank(GUARD + r.ye * nk + GUARD, POISON);
    std::vector<c32> plain(blank), mode0(blank), walk[3] = {blank, blank, blank}, one[3] = {blank, blank, blank};
    launch(plain, false, 0, 0.f, 16);
    launch(mode0, true, 0, 0.f, 16);
    for (int mode : {FC_FILTER_PHASE, FC_FILTER_WIENER}) {
        const float param = mode == FC_FILTER_PHASE ? r.c : r.lambda;
        launch(walk[mode], true, mode, param, 16);
        launch(one[mode], true, mode, param, 1);
    }
    judge(what, r, plain, mode0, walk, one);
}

// the generic body (kernel_path 1): the branch on the launch's mode
void run_generic(int H, int W, int kh, int kw, int nk) {
    PlanTuning tune;
    tune.path_mode = 0;
    RowData r;
    Geometry& g = r.g;
    char what[96];
    snprintf(what, sizeof(what), "generic %dx%d (*) %dx%d nk=%d", H, W, kh, kw, nk);
    if (!make_geometry(g, r.t, H, W, 1, kh, kw, tune) || g.fast_rows.ok) { CHECK(false, "%s: no generic plan", what); return; }
    r.d.tw_w = r.t.pw.tw.data();
    fill(r, kw, nk, 1, 4711u);
    std::vector<c32> lds(FC_LDS_BUDGET / sizeof(c32));
    emu::HostCtx ctx;
    auto launch = [&](std::vector<c32>& Y, int mode, float param) {
        SpectralRowsArgs a = spectral_rows_args(g, r.t, r.d, r.A.data(), kw, r.S.data(), Y.data() + GUARD);
        a.filter_mode = mode; a.filter_param = param;
        for (int k = 0; k < nk; k++)
            for (int row = 0; row < g.rows; row++) spectral_rows_body<-1>(ctx, lds.data(), a, row, k);
    };
    const std::vector<c32> blank(GUARD + r.ye * nk + GUARD, POISON);
    std::vector<c32> plain(blank), mode0(blank), walk[3] = {blank, blank, blank}, one[3] = {blank, blank, blank};
    launch(plain, 0, 0.f);
    launch(mode0, 0, 7.f);      // (mode 0 reads no parameter)
    for (int mode : {FC_FILTER_PHASE, FC_FILTER_WIENER}) {
        launch(walk[mode], mode, mode == FC_FILTER_PHASE ? r.c : r.lambda);
        one[mode] = walk[mode];      // (no walk in the generic kernel: one workgroup per row and map)
    }
    judge(what, r, plain, mode0, walk, one);
}

int cmd_rows() {
    // the configurations the planner picks for the shapes of tests/test_spectral_filter_gpu.py
    run_fast<RowCfg<288, 4, 6, 12, 192, 8>, 3>({270, 270, 19, 19, 2, 288, 288, 288, true}, 3);            // eight rows per workgroup, two store chains
    run_fast<RowCfg<384, 4, 8, 12, 192, 6>, 3>({282, 282, 23, 23, 2, 384, 384, 304, true}, 3);            // six rows, window 304
    run_fast<RowCfg<2112, 8, 12, 22, 192, 2>, 3>({250, 2100, 9, 13, 2, 288, 2112, 2112, true}, 3);        // two rows, two chains at R3 = 22
    run_fast<RowCfg<2560, 16, 16, 10, 256, 1>, 7>({250, 2500, 9, 41, 2, 288, 2560, 2544, true}, 3);       // one row, R1 = 16, cropped window
    run_fast<RowCfg<1152, 8, 12, 12, 192, 2>, 3>({40, 1100, 9, 31, 2, 48, 1152, 1136, false}, 3);         // row-major intermediate (generic output kernel)
    run_generic(40, 52, 7, 5, 3);
    printf("%d ok, %d failed\n%s\n", g_ok, g_failures, g_failures ? "FAILED" : "spectral filter rows ok");
    return g_failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "point") return cmd_point();
    if (mode == "rows") return cmd_rows();
    fprintf(stderr, "usage: %s point | rows\n", argv[0]);
    return 2;
}
