// ncc_host.cpp -- stand-alone host program over the product's headers csrc/ncc.hpp, csrc/fast_paths.hpp and csrc/fast_cols.hpp and
// the phase context of tests/emu/emu_runners.hpp (tests/test_ncc_host.py builds and runs it; it may also be built with
// -fsanitize=address,undefined and run directly).  The per-element bodies of the window statistics and
// of the kernel normalisation run here exactly as the kernels of kernels_ncc.hip call them -- strips of columns included -- and
// are held to the brute-force definition of include/fftconv.h (fftconv_plan_set_normalisation) in long double.
//   ncc_host stats     window statistics, every case
//   ncc_host kernels   kernel normalisation
//   ncc_host index     map -> image, strip widths, argument check
//   ncc_host shape     the launch-shape decision of the fused scale (fast_paths.hpp: fast_cols_rect_launch_shape with a Scale plane), whole window
//                      and rectangle, image0 > 0 and per_image > 1, and through it the NORM body of fast_cols.hpp on the phase
//                      context of tests/emu: every stored element must be the plain body's element times D at its window
//                      coordinate in the plane of its map's image, bit for bit, and nothing else may be written or read (the
//                      plane of image 0 is NaN, the planes end with the window: a sanitizer build sees any read beyond them)
//   ncc_host direct    fast_cols_norm_available over every configuration, and the norm_direct predicate (output_route.hpp: the fused store of plan_output_route)
//                      over mode x store x block-wise x format x region x configuration x layout of the intermediate
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

static uint64_t rng_state = 12345;
static double uniform() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}
static float gauss() {      // sum of 12 uniforms: close enough to N(0, 1) for a test image
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

// what launch_ncc_statistics (kernels_ncc.hip) runs: per strip, pass 1 over the strip's columns of every plane, then pass 2
static std::vector<float> product_statistics(const Image& im, int fft_h, int fft_w, int bh, int bw, int strip_cols) {
    std::vector<float> D((size_t)fft_h * fft_w, -1.f);
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
            for (int i = 0; i < fft_h; i++)
                D[(size_t)(j0 + c) * fft_h + i] = ncc_scale(c1, c2, (size_t)ncols * fft_h, fft_h, im.F, c + bw - 1, i, bw, bh * bw);
    }
    return D;
}

// the definition, brute force in long double; near[...] = 1 where den2 lies within a factor 16 of the floor
static void definition(const Image& im, int fft_h, int fft_w, int bh, int bw, std::vector<double>& D, std::vector<char>& floored, std::vector<char>& near) {
    D.assign((size_t)fft_h * fft_w, 0.0);
    floored.assign(D.size(), 0);
    near.assign(D.size(), 0);
    const long double n = (long double)bh * bw, fl = 1.0L / 1073741824.0L;
    for (int j = 0; j < fft_w; j++)
        for (int i = 0; i < fft_h; i++) {
            long double den2 = 0, e = 0;
            for (int f = 0; f < im.F; f++) {
                long double s1 = 0, s2 = 0;
                for (int b = 0; b < bw; b++)
                    for (int a = 0; a < bh; a++) {
                        const long double v = im.pad(f, j - b, i - a);
                        s1 += v;
                        s2 += v * v;
                    }
                den2 += s2 - s1 * s1 / n;
                e += s2;
            }
            const size_t at = (size_t)j * fft_h + i;
            if (den2 <= fl * e) floored[at] = 1;
            else D[at] = (double)(1.0L / sqrtl(den2));
            if (e > 0 && den2 > fl * e / 16 && den2 < fl * e * 16) near[at] = 1;
        }
}

static void stats_case(const char* name, Image& im, int bh, int bw, int strip_cols, bool expect_all_zero = false) {
    const int fft_h = ceil16(im.H + bh - 1), fft_w = ceil16(im.W + bw - 1);
    std::vector<double> ref;
    std::vector<char> floored, near;
    definition(im, fft_h, fft_w, bh, bw, ref, floored, near);
    const std::vector<float> got = product_statistics(im, fft_h, fft_w, bh, bw, strip_cols);
    long zeros = 0, nnear = 0;
    double worst = 0;
    const int before = failures;
    for (size_t at = 0; at < ref.size(); at++) {
        if (near[at]) { nnear++; continue; }
        if (floored[at]) {
            zeros++;
            CHECK(got[at] == 0.f && !std::signbit(got[at]), "%s: element %zu is floored by the definition, got %g", name, at, (double)got[at]);
        } else {
            // one rounding to fp32 (2^-24) on top of float64 sums of a window at least 16 floors from flat (2^-52 * 2^26 at most)
            const double err = std::fabs((double)got[at] - ref[at]) / ref[at];
            if (err > worst) worst = err;
            CHECK(got[at] != 0.f && err <= 6.1e-8, "%s: element %zu: got %.9g, definition %.17g (relative %.3g)", name, at, (double)got[at], ref[at], err);
        }
        if (failures - before > 5) break;
    }
    CHECK(nnear == 0, "%s: %ld windows lie within a factor 16 of the floor", name, nnear);
    if (expect_all_zero) CHECK(zeros == (long)ref.size(), "%s: D must be zero everywhere, %ld of %zu are", name, zeros, ref.size());
    if (failures == before) printf("ok   stats %s: %dx%dx%d box %dx%d window %dx%d strips of %d columns, %ld exact zeros, worst relative %.3g\n", name, im.H,
                                   im.W, im.F, bh, bw, fft_h, fft_w, strip_cols, zeros, worst);
}

static Image noise_image(int H, int W, int F, bool patch, bool strip, int ph = 0, int pw = 0) {
    Image im{H, W, F, std::vector<float>((size_t)H * W * F)};
    for (float& v : im.px) v = gauss();
    if (strip)      // a +100 strip: columns 3..5 of every plane
        for (int f = 0; f < F; f++)
            for (int w = 3; w < 6 && w < W; w++)
                for (int h = 0; h < H; h++) im.at(f, w, h) += 100.f;
    if (patch)      // a flat patch larger than the box, every plane its own level
        for (int f = 0; f < F; f++)
            for (int w = W / 3; w < W / 3 + pw && w < W; w++)
                for (int h = H / 4; h < H / 4 + ph && h < H; h++) im.at(f, w, h) = 0.37f + 1.5f * f;
    return im;
}

static int run_stats() {
    struct { int H, W, F, bh, bw; } shapes[] = {{40, 36, 2, 9, 7}, {30, 50, 1, 5, 11}, {23, 17, 3, 3, 3}};
    for (auto& s : shapes) {
        const int whole = ceil16(s.W + s.bw - 1) + s.bw - 1;
        Image a = noise_image(s.H, s.W, s.F, true, true, s.bh + 4, s.bw + 5);
        char name[64];
        snprintf(name, sizeof(name), "patch+strip, one strip");
        stats_case(name, a, s.bh, s.bw, whole);
        snprintf(name, sizeof(name), "patch+strip, narrow strips");
        stats_case(name, a, s.bh, s.bw, s.bw - 1 + 5);
        snprintf(name, sizeof(name), "patch+strip, one column per strip");
        stats_case(name, a, s.bh, s.bw, s.bw);
        Image b = noise_image(s.H, s.W, s.F, false, false);
        stats_case("noise, product strip width", b, s.bh, s.bw, ncc_strip_columns(ceil16(s.H + s.bh - 1), ceil16(s.W + s.bw - 1), s.F, s.bw, FC_NCC_SCRATCH_BYTES));
        stats_case("box 1x1", b, 1, 1, 7, true);
    }
    Image c = noise_image(12, 10, 2, false, false);
    stats_case("box as large as the image", c, 12, 10, 13);
    Image flat{16, 16, 1, std::vector<float>(256, 3.25f)};
    stats_case("constant image", flat, 5, 5, 9);
    Image zero{16, 16, 2, std::vector<float>(512, 0.f)};
    stats_case("zero image", zero, 4, 3, 40, true);
    return failures;
}

static int run_kernels() {
    struct { int F, kh, kw; } shapes[] = {{2, 9, 7}, {1, 5, 11}, {3, 3, 3}, {1, 1, 1}, {4, 31, 31}};
    for (auto& s : shapes) {
        const int pe = s.kh * s.kw;
        for (int kind = 0; kind < 4; kind++) {      // noise; noise + offset 1000; constant; constant per plane (different levels)
            std::vector<float> k((size_t)s.F * pe);
            for (int f = 0; f < s.F; f++)
                for (int e = 0; e < pe; e++) k[(size_t)f * pe + e] = kind == 0 ? gauss() : kind == 1 ? 1000.f + gauss() : kind == 2 ? 2.5f : 1.f + f;
            std::vector<double> stats((size_t)2 * s.F);
            for (int f = 0; f < s.F; f++) ncc_plane_stats(k.data() + (size_t)f * pe, pe, stats[2 * f], stats[2 * f + 1]);
            const double norm = ncc_kernel_norm(stats.data(), s.F);
            std::vector<long double> mean(s.F, 0);
            long double ss = 0;
            for (int f = 0; f < s.F; f++) {
                for (int e = 0; e < pe; e++) mean[f] += k[(size_t)f * pe + e];
                mean[f] /= pe;
                for (int e = 0; e < pe; e++) { const long double d = k[(size_t)f * pe + e] - mean[f]; ss += d * d; }
            }
            const bool constant = kind >= 2 || pe == 1;
            const int before = failures;
            double worst = 0, sumsq = 0;
            for (int f = 0; f < s.F; f++)
                for (int e = 0; e < pe; e++) {
                    const float got = ncc_unit(k[(size_t)f * pe + e], stats[2 * f], norm);
                    if (constant) { CHECK(got == 0.f, "constant kernel: element is %g", (double)got); continue; }
                    const double ref = (double)((k[(size_t)f * pe + e] - mean[f]) / sqrtl(ss));
                    // |T''| <= 1: one fp32 rounding of the quotient; the float64 mean of values near 1000 moves an element by 1e-13
                    const double err = std::fabs((double)got - ref);
                    if (err > worst) worst = err;
                    sumsq += (double)got * got;
                    CHECK(err <= 6e-8 * std::fabs(ref) + 1e-12, "kernel %dx%dx%d kind %d: got %.9g, definition %.17g", s.kh, s.kw, s.F, kind, (double)got, ref);
                }
            if (!constant) CHECK(std::fabs(sumsq - 1.0) < 1e-5, "unit norm: sum of squares %.9g", sumsq);
            if (failures == before) printf("ok   kernel %dx%dx%d kind %d%s worst %.3g\n", s.kh, s.kw, s.F, kind, constant ? " (all zeros)" : "", worst);
        }
    }
    return failures;
}

static int run_index() {
    // maps of a launch are image-major: nb images from image0 on, per_image kernels each
    for (int image0 : {0, 2})
        for (int per : {1, 3, 64})
            for (int nb : {1, 3})
                for (int b = 0; b < nb; b++)
                    for (int k = 0; k < per; k++) CHECK(ncc_image_of(image0, b * per + k, per) == image0 + b, "image of slot %d", b * per + k);
    printf("ok   index image-major slots\n");
    // strips: within the budget where it allows 16 window columns, never fewer than that, never more than the window needs
    CHECK(ncc_strip_columns(288, 288, 1, 31, FC_NCC_SCRATCH_BYTES) == 288 + 30, "small window: one strip");
    const int s4096 = ncc_strip_columns(4128, 4128, 1, 31, FC_NCC_SCRATCH_BYTES);
    CHECK(s4096 >= 31 && (size_t)2 * s4096 * 4128 * 8 <= FC_NCC_SCRATCH_BYTES, "4128-row window: %d columns", s4096);
    // the budget holds while box_w columns fit it; beyond that a strip is ONE window column: 16 * F * fft_h * box_w bytes
    const int s3 = ncc_strip_columns(4224, 4224, 3, 127, FC_NCC_SCRATCH_BYTES), s4 = ncc_strip_columns(4224, 4224, 4, 127, FC_NCC_SCRATCH_BYTES);
    CHECK(s3 >= 127 && (size_t)2 * 3 * s3 * 4224 * 8 <= FC_NCC_SCRATCH_BYTES, "F = 3 at cfg3's window: %d columns", s3);
    CHECK(s4 == 127 && (size_t)2 * 4 * s4 * 4224 * 8 > FC_NCC_SCRATCH_BYTES, "F = 4 at cfg3's window: %d columns, one window column per strip", s4);
    CHECK(ncc_strip_columns(4128, 4128, 512, 31, FC_NCC_SCRATCH_BYTES) == 31, "F = 512: the least strip");
    printf("ok   index strips (4128-row window: %d columns, %zu bytes)\n", s4096, (size_t)2 * s4096 * 4128 * 8);
    CHECK(!ncc_args_error(0, 0, 0, 31, 31) && !ncc_args_error(0, -5, 99, 31, 31), "mode 0 takes any box");
    CHECK(!ncc_args_error(1, 31, 31, 31, 31) && !ncc_args_error(1, 1, 1, 31, 31), "boxes on the bounds");
    CHECK(ncc_args_error(1, 32, 31, 31, 31) && ncc_args_error(1, 31, 32, 31, 31) && ncc_args_error(1, 0, 3, 31, 31) && ncc_args_error(1, 3, -1, 31, 31), "bad boxes");
    CHECK(ncc_args_error(2, 3, 3, 31, 31) && ncc_args_error(-1, 3, 3, 31, 31), "bad modes");
    printf("ok   index argument check\n");
    return failures;
}

struct Rect { int off_h, off_w, out_h, out_w; };

template <class Cfg>
static void shape_config(const char* what, int H, int W, int kh, int kw, bool exact, int want_fft_h, const std::vector<Rect>& rects) {
    constexpr int NK = 4, IMAGE0 = 1, PER_IMAGE = 2, PLANES = IMAGE0 + NK / PER_IMAGE;      // maps 0, 1: image 1; maps 2, 3: image 2
    constexpr size_t GUARD = 64;
    constexpr uint32_t POISON = 0xffc0dead;
    PlanTuning tune;
    tune.path_mode = 2;
    tune.exact_window = exact;
    Geometry g;
    Tables t;
    if (!make_geometry(g, t, H, W, 1, kh, kw, tune) || !g.fast_cols.ok || g.M != Cfg::M || g.fast_cols.T != Cfg::T || !g.y_tiled() || g.fft_h != want_fft_h ||
        g.fft_w != 288 || !fast_cols_norm_available(g.M, g.y_tiled())) {
        CHECK(false, "%s: the plan does not run the configuration this case names (M %d, window %d x %d)", what, g.M, g.fft_h, g.fft_w);
        return;
    }
    DeviceTables d;
    d.fc_tw1 = t.fcl.tw1.data(); d.fc_tw2 = t.fcl.tw2.data(); d.fc_pairs = t.fcl.pairs.data(); d.fc_rowoff = t.fcl.rowoff.data();
    static int queue[FC_QUEUE_WORDS];
    std::vector<c32> Y(g.y_elems_per_kernel() * NK);
    for (c32& y : Y) y = mk(gauss(), gauss());
    const size_t ne = g.map_elems();
    std::vector<float> D(ne * PLANES);          // (exactly the planes: nothing behind them)
    for (size_t i = 0; i < D.size(); i++) D[i] = i < ne ? std::nanf("") : (i % 7 == 0 ? 0.f : 0.25f + (float)uniform());
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
            MapPlane pl;
            pl.kind = PlaneKind::Scale; pl.plane = D.data(); pl.plane_elems = (size_t)g.fft_h * g.fft_w; pl.pitch = g.fft_h; pl.first = IMAGE0 * PER_IMAGE; pl.per_image = PER_IMAGE;
            FastColsShape sh = fast_cols_rect_launch_shape(Cfg::T, a, r.off_h, r.off_w, r.out_h, r.out_w, 1 << 20, pl);
            const FastColsNormArgs n = fast_cols_norm_args(sh.plane);      // what the launch hands the kernel
            // the decision: the rectangle launch of fast_cols_rect_launch_shape, plus the planes
            const int w_lo = r.off_w / Cfg::T * Cfg::T, w_hi = (r.off_w + r.out_w + Cfg::T - 1) / Cfg::T * Cfg::T, tiles = (w_hi - w_lo) / Cfg::T * NK;
            const bool whole = r.off_h == 0 && r.off_w == 0 && r.out_h == g.fft_h && r.out_w == g.fft_w;
            const int want_wide = (r.off_h % 2 == 0 && r.out_h % 2 == 0) ? 1 : 0;       // (the buffer and the stride are even)
            CHECK(sh.variant == (dyn ? FastColsVariant::TILED_DYN : FastColsVariant::TILED), "%s: variant %d", what, (int)sh.variant);
            CHECK(sh.a.h_lo == r.off_h && sh.a.fft_h == r.off_h + r.out_h && sh.a.out_pitch == r.out_h, "%s: rows [%d, %d) pitch %d", what, sh.a.h_lo, sh.a.fft_h, sh.a.out_pitch);
            CHECK(sh.a.w_first == w_lo && sh.a.ntiles == tiles && sh.a.tiles_per_kernel * NK == tiles && sh.grid == tiles, "%s: %d tiles from column %d on %d workgroups",
                  what, sh.a.ntiles, sh.a.w_first, sh.grid);
            CHECK(sh.a.rect_w_lo == r.off_w && sh.a.rect_w_n == r.out_w && sh.a.rect_wide == want_wide, "%s: columns [%d, +%d) wide %d", what, sh.a.rect_w_lo, sh.a.rect_w_n, sh.a.rect_wide);
            CHECK(!whole || sh.a.rect_wide == 1, "%s: the whole window keeps the pair stores", what);
            CHECK(sh.a.out_format == FC_MAP_F32 && sh.a.tail_tiles == 0 && sh.a.slice_shift == 0, "%s: fp32, unsliced", what);
            CHECK(sh.plane.kind == PlaneKind::Scale && n.d == D.data() && n.plane == ne && n.pitch == g.fft_h && n.first == IMAGE0 * PER_IMAGE && n.per_image == PER_IMAGE,
                  "%s: planes of %zu elements, pitch %d, first %d, %d per image", what, n.plane, n.pitch, n.first, n.per_image);
            if (failures != before) continue;
            if (dyn) sh.a.queue_shift = 1;
            sh.grid = sh.a.ntiles < 3 ? sh.a.ntiles : 3;
            run_wgs(sh.grid, [&](auto& ctx, int wg) {
                if (dyn) fast_cols_body<Cfg, true, false, true, ColStore::RECT_SCALE>(ctx, lds.data(), sh.a, wg, sh.grid, n);
                else fast_cols_body<Cfg, true, false, false, ColStore::RECT_SCALE>(ctx, lds.data(), sh.a, wg, sh.grid, n);
            });
            size_t bad = 0, first = 0, stray = 0, written = 0;
            for (size_t i = 0; i < total; i++) {
                uint32_t got;
                memcpy(&got, base + i, 4);
                const long rel = (long)i - (long)GUARD, k = rel >= 0 ? rel / (long)stride : -1, e = rel >= 0 ? rel % (long)stride : 0;
                if (k >= 0 && k < NK && (size_t)e < oe) {
                    const int w = r.off_w + (int)(e / r.out_h), h = r.off_h + (int)(e % r.out_h);
                    const size_t at = (size_t)w * g.fft_h + h;
                    const float want = ref[(size_t)k * ne + at] * D[(size_t)ncc_image_of(IMAGE0, (int)k, PER_IMAGE) * ne + at];
                    if (got != fc_float_bits(want) && !bad++) first = i;
                    written += got != POISON;
                } else if (got != POISON) stray++;
            }
            CHECK(!bad && !stray && written == NK * oe, "%s (%d, %d, %d, %d) %s: %zu elements differ (first at %zu), %zu stray stores, %zu written of %zu", what,
                  r.off_h, r.off_w, r.out_h, r.out_w, dyn ? "dynamic" : "static", bad, first, stray, written, NK * oe);
            if (failures == before) printf("ok   shape %s (%d, %d, %d, %d) %s %s: %zu elements = window x D of images %d.., bit for bit\n", what, r.off_h, r.off_w,
                                           r.out_h, r.out_w, dyn ? "dynamic" : "static", sh.a.rect_wide ? "wide" : "elementwise", written, IMAGE0);
        }
}

static int run_shape() {
    using C16 = ColCfg<144, 4, 6, 6, 16, 384>;        // cfg1's transform: the whole 288 x 288 window and the odd rectangle
    using CS = ColCfg<576, 6, 8, 12, 16, 768>;        // cfg2's: the 1088-row window on the 1152-point transform (rows beyond it have no D)
    shape_config<C16>("T=16", 270, 272, 13, 11, true, 288, {{0, 0, 288, 288}, {3, 5, 271, 271}, {2, 32, 4, 48}, {287, 287, 1, 1}});
    shape_config<CS>("short window", 1060, 270, 20, 11, false, 1088, {{0, 0, 1088, 288}, {1001, 9, 87, 21}});
    return failures;
}

static int run_direct() {
    std::vector<int> configs;
#define FC_X(MM, A, B, C, TT, NTT) configs.push_back(MM);
    FC_FAST_COL_CONFIGS(FC_X)
#undef FC_X
    int built = 0;
    for (int M : configs) {
        const bool listed = M == 544 || M == 2080;      // what the issue starts the not-built list with
        bool in_list = false;
        for (int x : FC_COLS_NORM_NOT_BUILT) in_list = in_list || x == M;
        CHECK(!listed || in_list, "M = %d must be listed as not built", M);
        CHECK(fast_cols_norm_built(M) == !in_list, "fast_cols_norm_built(%d)", M);
        CHECK(fast_cols_norm_available(M, true) == !in_list && !fast_cols_norm_available(M, false), "fast_cols_norm_available(%d)", M);
        CHECK(!fast_cols_norm_built(M) || fast_cols_rect_built(M) , "M = %d: a fused kernel without its rectangle kernel", M);
        built += !in_list;
    }
    for (int x : FC_COLS_NORM_NOT_BUILT) {
        bool is_config = false;
        for (int M : configs) is_config = is_config || M == x;
        CHECK(is_config, "%d is listed as not built and is no configuration", x);
    }
    for (int M : {56, 152, 1000, 4225}) CHECK(!fast_cols_lookup(M).ok && !fast_cols_norm_available(M, true), "M = %d has no specialised kernel", M);
    printf("ok   direct availability: %zu configurations, %d built\n", configs.size(), built);
    // the predicate: 1 only for mode 1, norm_store 1, one-pass, fp32, the window or a rectangle, a built configuration on the tiled intermediate
    long ones = 0, walked = 0;
    std::vector<int> ms = configs;
    ms.push_back(56);                                   // a generic / Bluestein plan: no configuration
    for (int M : ms)
        for (int tiled_y = 0; tiled_y < 2; tiled_y++)      // (0: kernel_path 2, the row-major intermediate; kernel_path 1 has no configuration at all)
            for (int mode = 0; mode < 2; mode++)
                for (int store = 0; store < 2; store++)
                    for (int blockwise = 0; blockwise < 2; blockwise++)
                        for (int format = FC_MAP_F32; format <= FC_MAP_BF16; format++)
                            for (long region = 0; region <= 5; region++) {
                                const bool want = mode == 1 && store == 1 && !blockwise && format == FC_MAP_F32 && (region == 0 || region == 5) && tiled_y &&
                                                  fast_cols_lookup(M).ok && M != 544 && M != 2080 && fast_cols_norm_built(M);
                                OutputRouteIn in;      // (the route of a packed sink: what read-only option "norm_direct" reports)
                                in.sink = SinkKind::Packed; in.region = region; in.rect_store = true; in.score = mode; in.norm_store = store != 0;
                                in.blockwise = blockwise != 0; in.map_format = format; in.fast_cols = fast_cols_lookup(M).ok; in.y_tiled = tiled_y != 0;
                                in.rect_built = fast_cols_rect_built(M); in.norm_built = fast_cols_norm_built(M); in.sqdiff_built = fast_cols_sqdiff_built(M);
                                const bool got = plan_output_route(in).fused();
                                CHECK(got == want, "norm_direct(M %d, tiled %d, mode %d, store %d, block-wise %d, format %d, region %ld) = %d", M, tiled_y, mode,
                                      store, blockwise, format, region, (int)got);
                                ones += got;
                                walked++;
                            }
    CHECK(ones == 2L * built, "%ld settings read 1, %d configurations are built", ones, built);
    printf("ok   direct predicate: %ld settings walked, %ld read 1\n", walked, ones);
    return failures;
}

int main(int argc, char** argv) {
    const char* what = argc > 1 ? argv[1] : "all";
    const bool all = !strcmp(what, "all");
    if (all || !strcmp(what, "stats")) run_stats();
    if (all || !strcmp(what, "kernels")) run_kernels();
    if (all || !strcmp(what, "index")) run_index();
    if (all || !strcmp(what, "shape")) run_shape();
    if (all || !strcmp(what, "direct")) run_direct();
    if (failures) printf("%d FAILURES\n", failures);
    else printf("all within the definition\n");
    return failures ? 1 : 0;
}
