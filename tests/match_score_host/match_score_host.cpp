// match_score_host.cpp -- stand-alone host program over the product's headers csrc/ncc.hpp, csrc/fast_paths.hpp and csrc/fast_cols.hpp
// and the phase context of tests/emu/emu_runners.hpp (tests/test_match_score_host.py builds and runs it; it may also be built with
// -fsanitize=address,undefined and run directly).  The per-element bodies of the matching scores (fftconv_plan_set_match_score) run
// here exactly as the kernels of kernels_score.hip call them and are held to the table of include/fftconv.h, brute force in long double.
//   match_score_host planes    Dc = E^(-1/2) and Q = E, strip by strip; exact zeros exactly where no non-zero pixel lies under the box
//   match_score_host kernels   the preparations of scores 2, 3 and 4 and the constant c_k
//   match_score_host shape     fast_cols_rect_launch_shape with an Add plane and through it the ADD body of fast_cols.hpp on the phase context: every
//                              element is the plain body's element + (Q + c), bit for bit, and nothing else is written or read
//   match_score_host direct    fast_cols_sqdiff_available and the fused store of plan_output_route (output_route.hpp) over every combination; the argument checks
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "emu_runners.hpp"
#include "ncc.hpp"
#include "output_route.hpp"

using namespace fc;
using emu::HostPhaseCtx;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint64_t rng_state = 4242;
static double uniform() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}
static float gauss() {
    double s = 0;
    for (int i = 0; i < 12; i++) s += uniform();
    return (float)(s - 6.0);
}
static int ceil16(int n) { return (n + 15) / 16 * 16; }

struct Image {
    int H, W, F;
    std::vector<float> px;      // [f][W][H]
    float& at(int f, int w, int h) { return px[((size_t)f * W + w) * H + h]; }
    float pad(int f, int w, int h) const { return (h < 0 || h >= H || w < 0 || w >= W) ? 0.f : px[((size_t)f * W + w) * H + h]; }
};

// what launch_score_statistics_typed runs: per strip, pass 1 over the strip's columns of every plane, then score_plane
static std::vector<float> product_plane(int score, const Image& im, int fft_h, int fft_w, int bh, int bw, int strip_cols) {
    std::vector<float> P((size_t)fft_h * fft_w, -1.f);
    std::vector<double> scratch((size_t)2 * im.F * strip_cols * fft_h);
    const int per_strip = strip_cols - (bw - 1);
    for (int j0 = 0; j0 < fft_w; j0 += per_strip) {
        const int nout = fft_w - j0 < per_strip ? fft_w - j0 : per_strip, ncols = nout + bw - 1, w_start = j0 - (bw - 1);
        double* c1 = scratch.data();
        double* c2 = scratch.data() + (size_t)im.F * ncols * fft_h;
        for (int f = 0; f < im.F; f++)
            for (int c = 0; c < ncols; c++) {
                const int w = w_start + c;
                const bool data = w >= 0 && w < im.W;
                const float* col = im.px.data() + ((size_t)f * im.W + (data ? w : 0)) * im.H;
                for (int i = 0; i < fft_h; i++) {
                    double s1 = 0.0, s2 = 0.0;
                    if (data) ncc_column_sums(col, im.H, i, bh, s1, s2);
                    c1[((size_t)f * ncols + c) * fft_h + i] = s1;
                    c2[((size_t)f * ncols + c) * fft_h + i] = s2;
                }
            }
        for (int c = 0; c < nout; c++)
            for (int i = 0; i < fft_h; i++) P[(size_t)(j0 + c) * fft_h + i] = score_plane(score, c2, (size_t)ncols * fft_h, fft_h, im.F, c + bw - 1, i, bw);
    }
    return P;
}

static void planes_case(const char* name, const Image& im, int bh, int bw, int strip_cols, bool expect_all_zero = false) {
    const int fft_h = ceil16(im.H + bh - 1), fft_w = ceil16(im.W + bw - 1);
    const std::vector<float> dc = product_plane(FC_SCORE_CCORR_NORMED, im, fft_h, fft_w, bh, bw, strip_cols);
    const std::vector<float> q = product_plane(FC_SCORE_SQDIFF, im, fft_h, fft_w, bh, bw, strip_cols);
    long zeros = 0;
    double worst_dc = 0, worst_q = 0;
    const int before = failures;
    for (int j = 0; j < fft_w && failures - before <= 5; j++)
        for (int i = 0; i < fft_h; i++) {
            long double e = 0;
            bool any = false;      // a non-zero pixel under the box
            for (int f = 0; f < im.F; f++)
                for (int b = 0; b < bw; b++)
                    for (int a = 0; a < bh; a++) {
                        const long double v = im.pad(f, j - b, i - a);
                        e += v * v;
                        any = any || v != 0;
                    }
            const size_t at = (size_t)j * fft_h + i;
            if (!any) {
                zeros++;
                CHECK(dc[at] == 0.f && !std::signbit(dc[at]) && q[at] == 0.f && !std::signbit(q[at]), "%s: element %zu has no pixel under its box, Dc %g Q %g", name, at,
                      (double)dc[at], (double)q[at]);
                continue;
            }
            // float64 sums of at most 31 * 31 * F non-negative terms (relative n * 2^-53 at the very most), one rounding to fp32 (2^-24)
            const double rq = (double)e, rdc = (double)(1.0L / sqrtl(e));
            const double eq = std::fabs((double)q[at] - rq) / rq, edc = std::fabs((double)dc[at] - rdc) / rdc;
            worst_q = eq > worst_q ? eq : worst_q;
            worst_dc = edc > worst_dc ? edc : worst_dc;
            CHECK(q[at] > 0.f && eq <= 6.1e-8, "%s: Q element %zu: got %.9g, definition %.17g", name, at, (double)q[at], rq);
            CHECK(dc[at] > 0.f && edc <= 6.1e-8, "%s: Dc element %zu: got %.9g, definition %.17g", name, at, (double)dc[at], rdc);
        }
    if (expect_all_zero) CHECK(zeros == (long)dc.size(), "%s: the planes must be zero everywhere, %ld of %zu are", name, zeros, dc.size());
    if (failures == before) printf("ok   planes %s: %dx%dx%d box %dx%d window %dx%d strips of %d columns, %ld exact zeros, worst relative Dc %.3g Q %.3g\n", name, im.H,
                                   im.W, im.F, bh, bw, fft_h, fft_w, strip_cols, zeros, worst_dc, worst_q);
}

static Image noise_image(int H, int W, int F, bool holes) {
    Image im{H, W, F, std::vector<float>((size_t)H * W * F)};
    for (float& v : im.px) v = gauss();
    if (holes)      // a block of zeros larger than the box in every plane, and a +100 strip
        for (int f = 0; f < F; f++) {
            for (int w = W / 3; w < W / 3 + 14 && w < W; w++)
                for (int h = H / 4; h < H / 4 + 13 && h < H; h++) im.at(f, w, h) = 0.f;
            for (int h = 0; h < H; h++) im.at(f, 1, h) += 100.f;
        }
    return im;
}

static int run_planes() {
    struct { int H, W, F, bh, bw; } shapes[] = {{40, 36, 2, 9, 7}, {30, 50, 1, 5, 11}, {23, 17, 3, 3, 3}};
    for (auto& s : shapes) {
        const int whole = ceil16(s.W + s.bw - 1) + s.bw - 1;
        const Image a = noise_image(s.H, s.W, s.F, true);
        planes_case("zero block+strip, one strip", a, s.bh, s.bw, whole);
        planes_case("zero block+strip, narrow strips", a, s.bh, s.bw, s.bw - 1 + 5);
        planes_case("zero block+strip, one column per strip", a, s.bh, s.bw, s.bw);
        const Image b = noise_image(s.H, s.W, s.F, false);
        planes_case("noise, product strip width", b, s.bh, s.bw, ncc_strip_columns(ceil16(s.H + s.bh - 1), ceil16(s.W + s.bw - 1), s.F, s.bw, FC_NCC_SCRATCH_BYTES));
    }
    const Image c = noise_image(12, 10, 2, false);
    planes_case("box as large as the image", c, 12, 10, 13);
    const Image zero{16, 16, 2, std::vector<float>(512, 0.f)};
    planes_case("zero image", zero, 4, 3, 40, true);
    return failures;
}

static int run_kernels() {
    struct { int F, kh, kw; } shapes[] = {{2, 9, 7}, {1, 5, 11}, {3, 3, 3}, {1, 1, 1}, {4, 31, 31}};
    for (auto& s : shapes) {
        const int pe = s.kh * s.kw;
        for (int kind = 0; kind < 4; kind++) {      // noise; noise + offset 1000; constant 2.5; all zeros
            std::vector<float> k((size_t)s.F * pe);
            for (float& v : k) v = kind == 0 ? gauss() : kind == 1 ? 1000.f + gauss() : kind == 2 ? 2.5f : 0.f;
            // the product's order: plane statistics (score 2's means), t2 plane by plane in ascending order
            std::vector<double> stats((size_t)2 * s.F);
            double t2 = 0.0;
            for (int f = 0; f < s.F; f++) {
                ncc_plane_stats(k.data() + (size_t)f * pe, pe, stats[2 * f], stats[2 * f + 1]);
                t2 += score_plane_t2(k.data() + (size_t)f * pe, pe);
            }
            const float c = (float)t2;
            std::vector<long double> mean(s.F, 0);
            long double rt2 = 0;
            for (int f = 0; f < s.F; f++) {
                for (int e = 0; e < pe; e++) { const long double v = k[(size_t)f * pe + e]; mean[f] += v; rt2 += v * v; }
                mean[f] /= pe;
            }
            const int before = failures;
            // c_k: a float64 sum of exact squares (relative n * 2^-53 at the most) rounded once to fp32
            CHECK(rt2 == 0 ? (c == 0.f) : std::fabs((double)c - (double)rt2) <= 6.1e-8 * (double)rt2, "c_k: got %.9g, definition %.17Lg", (double)c, rt2);
            double worst = 0;
            for (int f = 0; f < s.F; f++)
                for (int e = 0; e < pe; e++) {
                    const float x = k[(size_t)f * pe + e];
                    const float g2 = score_kernel_elem(FC_SCORE_CCOEFF, x, stats[2 * f], 0.0, t2);
                    const float g3 = score_kernel_elem(FC_SCORE_CCORR_NORMED, x, stats[2 * f], 0.0, t2);
                    const float g4 = score_kernel_elem(FC_SCORE_SQDIFF, x, stats[2 * f], 0.0, t2);
                    CHECK(g4 == -2.f * x, "score 4: -2 T is exact, got %.9g for %.9g", (double)g4, (double)x);
                    const double r2 = (double)(x - mean[f]);
                    // the float64 mean of n values near 1000 is within n * 2^-53 * 1000 of the exact one; one fp32 rounding of the difference
                    const double e2 = std::fabs((double)g2 - r2);
                    CHECK(e2 <= 6e-8 * std::fabs(r2) + 1e-9, "score 2 kernel %dx%dx%d kind %d: got %.9g, definition %.17g", s.kh, s.kw, s.F, kind, (double)g2, r2);
                    if (kind >= 2) CHECK(g2 == 0.f, "score 2 of a constant kernel is all zeros, got %g", (double)g2);
                    if (rt2 == 0) CHECK(g3 == 0.f && !std::signbit(g3), "score 3 of a zero kernel is all zeros, got %g", (double)g3);
                    else {
                        const double r3 = (double)(x / sqrtl(rt2)), e3 = std::fabs((double)g3 - r3);
                        worst = e3 > worst ? e3 : worst;
                        CHECK(e3 <= 6.1e-8 * std::fabs(r3), "score 3 kernel %dx%dx%d kind %d: got %.9g, definition %.17g", s.kh, s.kw, s.F, kind, (double)g3, r3);
                    }
                }
            if (failures == before) printf("ok   kernel %dx%dx%d kind %d%s c_k %.9g worst %.3g\n", s.kh, s.kw, s.F, kind, rt2 == 0 ? " (zero kernel)" : "", (double)c, worst);
        }
    }
    // the two adds of score 4 in their fixed order
    CHECK(score_sqdiff(1.f, 1e8f, -1e8f) == 1.f && score_sqdiff(-1e8f, 1e8f, 1.f) == 0.f, "score_sqdiff adds q + c first");
    printf("ok   kernel add order\n");
    return failures;
}

struct Rect { int off_h, off_w, out_h, out_w; };

template <class Cfg>
static void shape_config(const char* what, int H, int W, int kh, int kw, bool exact, int want_fft_h, const std::vector<Rect>& rects) {
    // five maps from slot 3 of a grid of three kernels per image: the launch starts inside image 1 and ends inside image 2
    constexpr int NK = 5, PER_IMAGE = 3, FIRST = 3 + 1, PLANES = (FIRST + NK - 1) / PER_IMAGE + 1;
    constexpr size_t GUARD = 64;
    constexpr uint32_t POISON = 0xffc0dead;
    PlanTuning tune;
    tune.path_mode = 2;
    tune.exact_window = exact;
    Geometry g;
    Tables t;
    if (!make_geometry(g, t, H, W, 1, kh, kw, tune) || !g.fast_cols.ok || g.M != Cfg::M || g.fast_cols.T != Cfg::T || !g.y_tiled() || g.fft_h != want_fft_h ||
        g.fft_w != 288 || !fast_cols_sqdiff_available(g.M, g.y_tiled())) {
        CHECK(false, "%s: the plan does not run the configuration this case names (M %d, window %d x %d)", what, g.M, g.fft_h, g.fft_w);
        return;
    }
    DeviceTables d;
    d.fc_tw1 = t.fcl.tw1.data(); d.fc_tw2 = t.fcl.tw2.data(); d.fc_pairs = t.fcl.pairs.data(); d.fc_rowoff = t.fcl.rowoff.data();
    static int queue[FC_QUEUE_WORDS];
    std::vector<c32> Y(g.y_elems_per_kernel() * NK);
    for (c32& y : Y) y = mk(gauss(), gauss());
    const size_t ne = g.map_elems();
    std::vector<float> Q(ne * PLANES);          // (exactly the planes: nothing behind them; image 0 is never read: NaN)
    for (size_t i = 0; i < Q.size(); i++) Q[i] = i < ne ? std::nanf("") : (i % 7 == 0 ? 0.f : 50.f * (float)uniform());
    std::vector<float> consts(PER_IMAGE);       // (exactly the kernels of an image)
    for (int k = 0; k < PER_IMAGE; k++) consts[k] = 3.f + 17.f * k + (float)uniform();
    std::vector<c32> lds(FC_LDS_BUDGET / sizeof(c32));
    auto run_wgs = [&](int grid, auto&& body) {
        for (int wg = 0; wg < grid; wg++) {
            for (int i = 0; i < Cfg::LDS_ELEMS; i++) lds[i] = mk(1e30f, -1e30f);
            HostPhaseCtx<ColPairState<Cfg>> ctx(Cfg::NT);
            body(ctx, wg);
        }
    };
    std::vector<float> ref(ne * NK);
    {
        d.queue = nullptr;
        const FastColsArgs a = fast_cols_args(g, d, Y.data(), ref.data(), ne, NK, FC_MAP_F32);
        FastColsShape sh = fast_cols_launch_shape(Cfg::M, Cfg::T, a, 1 << 20);
        if (sh.variant != FastColsVariant::TILED) { CHECK(false, "%s: reference launch shape %d", what, (int)sh.variant); return; }
        sh.grid = 3;
        run_wgs(sh.grid, [&](auto& ctx, int wg) { fast_cols_body<Cfg, true>(ctx, lds.data(), sh.a, wg, sh.grid); });
    }
    for (const Rect& r : rects)
        for (int dyn = 0; dyn < 2; dyn++) {
            const int before = failures;
            const size_t oe = (size_t)r.out_h * r.out_w, stride = oe + GUARD, total = GUARD + NK * stride;
            std::vector<uint64_t> store((total * 4 + 7) / 8 + 1);
            float* base = reinterpret_cast<float*>(store.data());
            for (size_t i = 0; i < total; i++) memcpy(base + i, &POISON, 4);
            d.queue = dyn ? queue : nullptr;
            const FastColsArgs a = fast_cols_args(g, d, Y.data(), base + GUARD, stride, NK, FC_MAP_F32);
            // the product passes (image0, per_image) with the launch's first kernel at consts[0]; a launch that starts inside an image
            // is what `first` not being a multiple of per_image means, set here as the body reads it
            MapPlane pl;
            pl.kind = PlaneKind::Add; pl.plane = Q.data(); pl.consts = consts.data(); pl.plane_elems = (size_t)g.fft_h * g.fft_w; pl.pitch = g.fft_h;
            pl.first = 1 * PER_IMAGE; pl.per_image = PER_IMAGE;
            FastColsShape sh = fast_cols_rect_launch_shape(Cfg::T, a, r.off_h, r.off_w, r.out_h, r.out_w, 1 << 20, pl);
            FastColsSqdiffArgs q = fast_cols_sqdiff_args(sh.plane);      // what the launch hands the kernel
            const int w_lo = r.off_w / Cfg::T * Cfg::T, w_hi = (r.off_w + r.out_w + Cfg::T - 1) / Cfg::T * Cfg::T, tiles = (w_hi - w_lo) / Cfg::T * NK;
            const int want_wide = (r.off_h % 2 == 0 && r.out_h % 2 == 0) ? 1 : 0;
            CHECK(sh.variant == (dyn ? FastColsVariant::TILED_DYN : FastColsVariant::TILED), "%s: variant %d", what, (int)sh.variant);
            CHECK(sh.a.h_lo == r.off_h && sh.a.fft_h == r.off_h + r.out_h && sh.a.out_pitch == r.out_h, "%s: rows [%d, %d) pitch %d", what, sh.a.h_lo, sh.a.fft_h, sh.a.out_pitch);
            CHECK(sh.a.w_first == w_lo && sh.a.ntiles == tiles && sh.grid == tiles, "%s: %d tiles from column %d on %d workgroups", what, sh.a.ntiles, sh.a.w_first, sh.grid);
            CHECK(sh.a.rect_w_lo == r.off_w && sh.a.rect_w_n == r.out_w && sh.a.rect_wide == want_wide, "%s: columns [%d, +%d) wide %d", what, sh.a.rect_w_lo, sh.a.rect_w_n, sh.a.rect_wide);
            CHECK(q.q == Q.data() && q.c == consts.data() && q.plane == ne && q.pitch == g.fft_h && q.first == PER_IMAGE && q.per_image == PER_IMAGE &&
                  fast_cols_sqdiff_args_ok(q) && sh.plane.kind == PlaneKind::Add, "%s: planes of %zu elements, pitch %d, first %d, %d per image", what, q.plane, q.pitch, q.first, q.per_image);
            if (failures != before) continue;
            q.first = FIRST;
            if (dyn) sh.a.queue_shift = 1;
            sh.grid = sh.a.ntiles < 3 ? sh.a.ntiles : 3;
            run_wgs(sh.grid, [&](auto& ctx, int wg) {
                if (dyn) fast_cols_body<Cfg, true, false, true, ColStore::RECT_ADD>(ctx, lds.data(), sh.a, wg, sh.grid, q);
                else fast_cols_body<Cfg, true, false, false, ColStore::RECT_ADD>(ctx, lds.data(), sh.a, wg, sh.grid, q);
            });
            size_t bad = 0, first = 0, stray = 0, written = 0;
            for (size_t i = 0; i < total; i++) {
                uint32_t got;
                memcpy(&got, base + i, 4);
                const long rel = (long)i - (long)GUARD, k = rel >= 0 ? rel / (long)stride : -1, e = rel >= 0 ? rel % (long)stride : 0;
                if (k >= 0 && k < NK && (size_t)e < oe) {
                    const int w = r.off_w + (int)(e / r.out_h), h = r.off_h + (int)(e % r.out_h);
                    const size_t at = (size_t)w * g.fft_h + h;
                    const int slot = FIRST + (int)k;
                    const float s = Q[(size_t)(slot / PER_IMAGE) * ne + at] + consts[slot % PER_IMAGE];
                    const float want = ref[(size_t)k * ne + at] + s;
                    if (got != fc_float_bits(want) && !bad++) first = i;
                    written += got != POISON;
                } else if (got != POISON) stray++;
            }
            CHECK(!bad && !stray && written == NK * oe, "%s (%d, %d, %d, %d) %s: %zu elements differ (first at %zu), %zu stray stores, %zu written of %zu", what,
                  r.off_h, r.off_w, r.out_h, r.out_w, dyn ? "dynamic" : "static", bad, first, stray, written, NK * oe);
            if (failures == before) printf("ok   shape %s (%d, %d, %d, %d) %s %s: %zu elements = window + (Q + c) of slots %d.., bit for bit\n", what, r.off_h, r.off_w,
                                           r.out_h, r.out_w, dyn ? "dynamic" : "static", sh.a.rect_wide ? "wide" : "elementwise", written, FIRST);
        }
}

static int run_shape() {
    using C16 = ColCfg<144, 4, 6, 6, 16, 384>;        // cfg1's transform: the whole 288 x 288 window and the odd rectangle
    using CS = ColCfg<576, 6, 8, 12, 16, 768>;        // cfg2's: the 1088-row window on the 1152-point transform (rows beyond it have no Q)
    shape_config<C16>("T=16", 270, 272, 13, 11, true, 288, {{0, 0, 288, 288}, {3, 5, 271, 271}, {287, 287, 1, 1}});
    shape_config<CS>("short window", 1060, 270, 20, 11, false, 1088, {{0, 0, 1088, 288}, {1001, 9, 87, 21}});
    return failures;
}

static int run_direct() {
    std::vector<int> configs;
#define FC_X(MM, A, B, C, TT, NTT) configs.push_back(MM);
    FC_FAST_COL_CONFIGS(FC_X)
#undef FC_X
    int built = 0, norm_built = 0;
    for (int M : configs) {
        const bool listed = M == 544 || M == 2080;
        bool in_list = false;
        for (int x : FC_COLS_SQDIFF_NOT_BUILT) in_list = in_list || x == M;
        CHECK(!listed || in_list, "M = %d must be listed as not built", M);
        CHECK(fast_cols_sqdiff_built(M) == !in_list, "fast_cols_sqdiff_built(%d)", M);
        CHECK(fast_cols_sqdiff_available(M, true) == !in_list && !fast_cols_sqdiff_available(M, false), "fast_cols_sqdiff_available(%d)", M);
        CHECK(!fast_cols_sqdiff_built(M) || fast_cols_rect_built(M), "M = %d: a fused kernel without its rectangle kernel", M);
        built += !in_list;
        norm_built += fast_cols_norm_built(M);
    }
    for (int x : FC_COLS_SQDIFF_NOT_BUILT) {
        bool is_config = false;
        for (int M : configs) is_config = is_config || M == x;
        CHECK(is_config, "%d is listed as not built and is no configuration", x);
    }
    printf("ok   direct availability: %zu configurations, %d built\n", configs.size(), built);
    long ones[5] = {0, 0, 0, 0, 0}, walked = 0;
    std::vector<int> ms = configs;
    ms.push_back(56);
    for (int M : ms)
        for (int tiled_y = 0; tiled_y < 2; tiled_y++)
            for (int score = 0; score <= 4; score++)
                for (int store = 0; store < 2; store++)
                    for (int blockwise = 0; blockwise < 2; blockwise++)
                        for (int format = FC_MAP_F32; format <= FC_MAP_BF16; format++)
                            for (long region = 0; region <= 5; region++) {
                                const bool common = store == 1 && !blockwise && format == FC_MAP_F32 && (region == 0 || region == 5) && tiled_y && fast_cols_lookup(M).ok;
                                const bool want = score == 4 ? common && fast_cols_sqdiff_built(M) : (score == 1 || score == 3) ? common && fast_cols_norm_built(M) : false;
                                OutputRouteIn in;      // (the route of a packed sink: what read-only option "norm_direct" reports)
                                in.sink = SinkKind::Packed; in.region = region; in.rect_store = true; in.score = score; in.norm_store = store != 0;
                                in.blockwise = blockwise != 0; in.map_format = format; in.fast_cols = fast_cols_lookup(M).ok; in.y_tiled = tiled_y != 0;
                                in.rect_built = fast_cols_rect_built(M); in.norm_built = fast_cols_norm_built(M); in.sqdiff_built = fast_cols_sqdiff_built(M);
                                const OutputRoute route = plan_output_route(in);
                                const bool got = route.fused();
                                CHECK(got == want, "score_direct(M %d, tiled %d, score %d, store %d, block-wise %d, format %d, region %ld) = %d", M, tiled_y, score,
                                      store, blockwise, format, region, (int)got);
                                if (score == 1) CHECK(got == (route.store == OutStore::RectScale && route.plane == OutPlane::D), "score 1 is mode 1");
                                ones[score] += got;
                                walked++;
                            }
    CHECK(ones[0] == 0 && ones[2] == 0 && ones[1] == 2L * norm_built && ones[3] == ones[1] && ones[4] == 2L * built, "settings that read 1: %ld %ld %ld %ld %ld", ones[0],
          ones[1], ones[2], ones[3], ones[4]);
    printf("ok   direct predicate: %ld settings walked, %ld read 1 for score 4\n", walked, ones[4]);
    // the argument checks
    CHECK(!score_args_error(0, 0, 0, 31, 31) && !score_args_error(0, -5, 99, 31, 31), "score 0 takes any box");
    for (int sc = 1; sc <= 4; sc++) {
        CHECK(!score_args_error(sc, 31, 31, 31, 31) && !score_args_error(sc, 1, 1, 31, 31), "boxes on the bounds");
        CHECK(score_args_error(sc, 32, 31, 31, 31) && score_args_error(sc, 31, 32, 31, 31) && score_args_error(sc, 0, 3, 31, 31) && score_args_error(sc, 3, -1, 31, 31), "bad boxes");
    }
    CHECK(score_args_error(5, 3, 3, 31, 31) && score_args_error(-1, 3, 3, 31, 31), "bad scores");
    CHECK(ncc_args_error(2, 3, 3, 31, 31) && ncc_args_error(3, 3, 3, 31, 31) && ncc_args_error(4, 3, 3, 31, 31), "set_normalisation still takes modes 0 and 1 only");
    CHECK(score_has_plane(1) && !score_has_plane(2) && score_has_plane(3) && score_has_plane(4) && !score_has_plane(0), "scores with a plane");
    FastColsSqdiffArgs qa;
    CHECK(!fast_cols_sqdiff_args_ok(qa), "empty arguments are refused");
    float x = 0;
    qa.q = &x; qa.c = &x; qa.plane = 1; qa.pitch = 1; qa.per_image = 1;
    CHECK(fast_cols_sqdiff_args_ok(qa), "complete arguments");
    qa.c = nullptr;
    CHECK(!fast_cols_sqdiff_args_ok(qa), "no constants");
    qa.c = &x; qa.per_image = 0;
    CHECK(!fast_cols_sqdiff_args_ok(qa), "no kernels per image");
    printf("ok   direct argument checks\n");
    return failures;
}

int main(int argc, char** argv) {
    const char* what = argc > 1 ? argv[1] : "all";
    const bool all = !strcmp(what, "all");
    if (all || !strcmp(what, "planes")) run_planes();
    if (all || !strcmp(what, "kernels")) run_kernels();
    if (all || !strcmp(what, "shape")) run_shape();
    if (all || !strcmp(what, "direct")) run_direct();
    if (failures) printf("%d FAILURES\n", failures);
    else printf("all within the definition\n");
    return failures ? 1 : 0;
}
