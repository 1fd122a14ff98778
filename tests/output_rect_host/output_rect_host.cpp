// output_rect_host.cpp -- TEST-ONLY stand-alone host program for the rectangle store of the specialised output kernel
// (fftconv_plan_set_output_rect; fast_cols.hpp: RECT).
//
// Built by tests/test_output_rect_host.py with the host compiler from the product's kernel headers and the phase context of
// tests/emu/emu_runners.hpp; it is not the emulator library and not part of the product.  Modes:
//   bodies     for one configuration of each tile width (T = 16, 8, 4) and for a window shorter than its transform: the unchanged
//              fast_cols_body stores the full fp32 window of two maps (the reference), then the RECT body stores a list of
//              rectangles in fp32, fp16 and bf16 through fast_cols_rect_launch_shape, static deal and dynamic tile queue, into
//              map buffers with a poisoned band in front of and behind every map.  Every element of a rectangle map must equal
//              the reference element (16-bit: converted by ref16 below) bit for bit, and nothing else may be written.  That the
//              tiles outside the rectangle are never gathered is pinned by the launch shape (ntiles, w_first, the grid); columns
//              of the intermediate outside that tile range are NaN besides, so a tile index that strays there shows in the maps.
//   validate   prints output_rect_error for a list of rectangles of a 288 x 288 window
// Having its own main, it is also the place for a host sanitizer build (-fsanitize=address,undefined) of this code.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "emu_runners.hpp"

using namespace fc;
using emu::HostPhaseCtx;

namespace {

// ---- the reference conversions: round to nearest even in floating point (nearbyint in the default rounding mode on an exactly
// ---- scaled double), nothing shared with the integer arithmetic of fc_common.hpp
uint16_t ref_bits(float x, int mant_bits, int e_min, int e_max, uint16_t inf_bits, uint16_t nan_bits) {
    const uint16_t sign = std::signbit(x) ? 0x8000u : 0u;
    if (std::isnan(x)) return sign | nan_bits;
    const double a = std::fabs((double)x);
    if (a == 0.0) return sign;
    if (std::isinf(x)) return sign | inf_bits;
    int e = 0;
    (void)std::frexp(a, &e);
    int E = e - 1;                                            // a = 1.m x 2^E
    if (E < e_min) {                                          // subnormal result: a whole number of 2^(e_min - mant_bits)
        const double q = std::nearbyint(std::ldexp(a, mant_bits - e_min));
        return sign | (uint16_t)q;                            // (q = 2^mant_bits is the smallest normal: the same bits)
    }
    double q = std::nearbyint(std::ldexp(a, mant_bits - E));  // in [2^mant_bits, 2^(mant_bits + 1)]
    if (q == std::ldexp(1.0, mant_bits + 1)) { q = std::ldexp(1.0, mant_bits); E++; }
    if (E > e_max) return sign | inf_bits;
    return sign | (uint16_t)(((E - e_min + 1) << mant_bits) | ((int)q - (1 << mant_bits)));
}
uint16_t ref16(float x, int format) {
    return format == FC_MAP_BF16 ? ref_bits(x, 7, -126, 127, 0x7f80u, 0x7fc0u) : ref_bits(x, 10, -14, 15, 0x7c00u, 0x7e00u);
}

int g_failures = 0, g_ok = 0;

// values whose magnitudes sweep 2^-30 .. 2^20 over the columns: fp16 subnormals, zeros and overflows all occur in the maps
float col_scale(int w) { return std::ldexp(1.0f, (w * 7) % 51 - 30); }
float rnd(uint32_t& s) {
    s = s * 1664525u + 1013904223u;
    return (float)((int32_t)(s >> 8) - (1 << 23)) / (float)(1 << 23);
}

struct Rect { int off_h, off_w, out_h, out_w; };

// The list of the 288-column window (the issue's list at T = 16, fft_h = 288), scaled to the window's height and the tile width
std::vector<Rect> rect_list(int fft_h, int T) {
    return {
        {0, 0, fft_h, 288},            // whole window
        {6, 5, fft_h - 18, 272},       // "same"
        {12, 10, fft_h - 30, 262},     // "valid"
        {1, 0, fft_h - 1, 288},        // odd offset, odd pitch
        {5, 3, fft_h - 6, 283},        // odd, odd, even pitch, odd width
        {7, T + 1, 33, 1},             // one column
        {3, T - 1, 1, 2},              // one row across a tile boundary
        {0, T, 2, T},                  // exactly one tile, one pair
        {fft_h - 1, 287, 1, 1},        // last element
        {2, 2 * T, 4, 3 * T},          // all even and tile-aligned: the wide-store case
    };
}

constexpr int NK = 2;              // maps per launch
constexpr size_t GUARD = 64;       // poisoned elements in front of and behind every map
constexpr uint32_t POISON32 = 0xffc0dead;
constexpr uint16_t POISON16 = 0xdead;

template <class Cfg>
void run_config(const char* what, int H, int W, int kh, int kw, bool exact, int want_fft_h, const std::vector<Rect>& rects) {
    PlanTuning tune;
    tune.path_mode = 2;
    tune.exact_window = exact;
    Geometry g;
    Tables t;
    const FastColsInfo fi = fast_cols_lookup(Cfg::M);
    if (!make_geometry(g, t, H, W, 1, kh, kw, tune) || !g.fast_cols.ok || g.M != Cfg::M || fi.R1 != Cfg::R1 || fi.R2 != Cfg::R2 || fi.R3 != Cfg::R3 ||
        fi.T != Cfg::T || fi.NT != Cfg::NT || !g.y_tiled() || g.fft_h != want_fft_h || g.fft_w != 288 || !fast_cols_rect_available(g.M, g.y_tiled())) {
        g_failures++;
        printf("FAIL %s: the plan does not run the configuration this case names (M %d, window %d x %d)\n", what, g.M, g.fft_h, g.fft_w);
        return;
    }
    DeviceTables d;
    d.fc_tw1 = t.fcl.tw1.data(); d.fc_tw2 = t.fcl.tw2.data(); d.fc_pairs = t.fcl.pairs.data(); d.fc_rowoff = t.fcl.rowoff.data();
    static int queue[FC_QUEUE_WORDS];
    const size_t yk = g.y_elems_per_kernel();
    std::vector<c32> Y(yk * NK);
    std::vector<int> col_of(yk);
    uint32_t seed = 4321u + (uint32_t)Cfg::M;
    for (size_t i = 0; i < yk; i++) col_of[i] = (int)(i / ((size_t)g.tile_rows() * g.y_tile_w)) * g.y_tile_w + (int)(i % g.y_tile_w);
    for (size_t i = 0; i < Y.size(); i++) {
        const float s = col_scale(col_of[i % yk]);
        Y[i] = mk(s * rnd(seed), s * rnd(seed));
    }
    std::vector<c32> lds(FC_LDS_BUDGET / sizeof(c32));
    auto run_wgs = [&](int grid, auto&& body) {
        for (int wg = 0; wg < grid; wg++) {
            for (int i = 0; i < Cfg::LDS_ELEMS; i++) lds[i] = mk(1e30f, -1e30f);
            HostPhaseCtx<ColPairState<Cfg>> ctx(Cfg::NT);
            body(ctx, wg);
        }
    };

    // the reference: the unchanged body, full fp32 window
    const size_t ne = g.map_elems();
    std::vector<float> ref(ne * NK);
    for (size_t i = 0; i < ref.size(); i++) memcpy(&ref[i], &POISON32, 4);
    {
        d.queue = nullptr;
        const FastColsArgs a = fast_cols_args(g, d, Y.data(), ref.data(), ne, NK, FC_MAP_F32);
        FastColsShape sh = fast_cols_launch_shape(Cfg::M, Cfg::T, a, 1 << 20);
        if (sh.variant != FastColsVariant::TILED) { g_failures++; printf("FAIL %s: reference launch shape %d\n", what, (int)sh.variant); return; }
        sh.grid = 3;
        run_wgs(sh.grid, [&](auto& ctx, int wg) { fast_cols_body<Cfg, true>(ctx, lds.data(), sh.a, wg, sh.grid); });
        for (size_t i = 0; i < ref.size(); i++)
            if (fc_float_bits(ref[i]) == POISON32) { g_failures++; printf("FAIL %s: the reference left element %zu unwritten\n", what, i); return; }
    }

    std::vector<c32> Yr(Y.size());
    for (const Rect& r : rects) {
        if (output_rect_error(r.off_h, r.off_w, r.out_h, r.out_w, g.fft_h, g.fft_w)) {
            g_failures++;
            printf("FAIL %s: rectangle (%d, %d, %d, %d) is not inside the window\n", what, r.off_h, r.off_w, r.out_h, r.out_w);
            continue;
        }
        // columns outside the tiles the launch may touch are NaN in the intermediate (a wrong tile index then stores NaNs; a
        // tile that were gathered and dropped would not show here: the launch-shape check below is what rules that out)
        const int w_lo = r.off_w / Cfg::T * Cfg::T, w_hi = (r.off_w + r.out_w + Cfg::T - 1) / Cfg::T * Cfg::T;
        const float nan = std::numeric_limits<float>::quiet_NaN();
        for (size_t i = 0; i < Y.size(); i++) {
            const int w = col_of[i % yk];
            Yr[i] = (w >= w_lo && w < w_hi) ? Y[i] : mk(nan, nan);
        }
        const size_t oe = (size_t)r.out_h * r.out_w, stride = oe + GUARD;
        const bool whole_or_wide = (r.off_h % 2 == 0 && r.out_h % 2 == 0);
        struct Run { bool dyn; int shift; };       // shift: elements the first map is moved off its aligned position
        std::vector<Run> runs = {{false, 0}, {true, 1}};
        if (whole_or_wide) { runs.push_back({false, 1}); runs.push_back({true, 0}); }
        for (int format = FC_MAP_F32; format <= FC_MAP_BF16; format++) {
            const size_t eb = fc_map_elem_bytes(format);
            for (const Run& run : runs) {
                // [guard][map 0][guard][map 1][guard] (+ the shift), 16-byte aligned storage
                const size_t total = GUARD + NK * stride + 2;
                std::vector<uint64_t> store((total * eb + 7) / 8 + 2);
                unsigned char* base = reinterpret_cast<unsigned char*>(store.data());
                for (size_t i = 0; i < total; i++) {
                    if (format == FC_MAP_F32) memcpy(base + 4 * i, &POISON32, 4);
                    else memcpy(base + 2 * i, &POISON16, 2);
                }
                float* out = reinterpret_cast<float*>(base + (GUARD + (size_t)run.shift) * eb);
                d.queue = run.dyn ? queue : nullptr;
                const FastColsArgs a = fast_cols_args(g, d, Yr.data(), out, stride, NK, format);
                FastColsShape sh = fast_cols_rect_launch_shape(Cfg::T, a, r.off_h, r.off_w, r.out_h, r.out_w, 1 << 20);
                const bool want_wide = whole_or_wide && run.shift == 0;
                const int want_tiles = (w_hi - w_lo) / Cfg::T * NK;
                if ((sh.variant == FastColsVariant::TILED_DYN) != run.dyn || (sh.variant != FastColsVariant::TILED_DYN && sh.variant != FastColsVariant::TILED) ||
                    sh.a.rect_wide != (want_wide ? 1 : 0) || sh.a.ntiles != want_tiles || sh.a.w_first != w_lo || sh.grid != want_tiles) {
                    g_failures++;
                    printf("FAIL %s (%d, %d, %d, %d): launch shape: variant %d, wide %d, %d tiles from column %d on %d workgroups\n", what, r.off_h,
                           r.off_w, r.out_h, r.out_w, (int)sh.variant, sh.a.rect_wide, sh.a.ntiles, sh.a.w_first, sh.grid);
                    continue;
                }
                if (run.dyn) sh.a.queue_shift = 1;
                sh.grid = sh.a.ntiles < 3 ? sh.a.ntiles : 3;
                run_wgs(sh.grid, [&](auto& ctx, int wg) {
                    if (format == FC_MAP_F32) {
                        if (run.dyn) fast_cols_body<Cfg, true, false, true, ColStore::RECT>(ctx, lds.data(), sh.a, wg, sh.grid);
                        else fast_cols_body<Cfg, true, false, false, ColStore::RECT>(ctx, lds.data(), sh.a, wg, sh.grid);
                    } else {
                        if (run.dyn) fast_cols_body<Cfg, true, false, true, ColStore::RECT16>(ctx, lds.data(), sh.a, wg, sh.grid);
                        else fast_cols_body<Cfg, true, false, false, ColStore::RECT16>(ctx, lds.data(), sh.a, wg, sh.grid);
                    }
                });
                // every element of the buffer: inside a map the reference element, everywhere else the poison
                size_t bad = 0, first = 0, written = 0, stray = 0;
                for (size_t i = 0; i < total; i++) {
                    uint32_t got = 0;
                    if (format == FC_MAP_F32) memcpy(&got, base + 4 * i, 4);
                    else { uint16_t h; memcpy(&h, base + 2 * i, 2); got = h; }
                    const uint32_t poison = format == FC_MAP_F32 ? POISON32 : POISON16;
                    const long rel = (long)i - (long)(GUARD + run.shift);
                    const long k = rel >= 0 ? rel / (long)stride : -1, e = rel >= 0 ? rel % (long)stride : 0;
                    if (k >= 0 && k < NK && (size_t)e < oe) {
                        const int w = r.off_w + (int)(e / r.out_h), h = r.off_h + (int)(e % r.out_h);
                        const float x = ref[(size_t)k * ne + (size_t)w * g.fft_h + h];
                        const uint32_t want = format == FC_MAP_F32 ? fc_float_bits(x) : ref16(x, format);
                        if (got != want && !bad++) first = i;
                        written += got != poison || want == poison;
                    } else if (got != poison) {
                        stray++;
                    }
                }
                if (bad || stray || written != NK * oe) {
                    g_failures++;
                    printf("FAIL %s (%d, %d, %d, %d) format %d %s shift %d: %zu elements differ (first at %zu), %zu stray stores, %zu written of %zu\n", what,
                           r.off_h, r.off_w, r.out_h, r.out_w, format, run.dyn ? "dynamic" : "static", run.shift, bad, first, stray, written, NK * oe);
                } else {
                    g_ok++;
                    printf("ok   %s (%d, %d, %d, %d) format %d %s shift %d %s: %zu elements bit-equal, guards intact\n", what, r.off_h, r.off_w, r.out_h,
                           r.out_w, format, run.dyn ? "dynamic" : "static", run.shift, sh.a.rect_wide ? "wide" : "elementwise", written);
                }
            }
        }
    }
}

int cmd_bodies() {
    // (M, R1, R2, R3, T, NT) as fast_paths.hpp lists them -- checked against fast_cols_lookup at run time; every window is 288 columns wide
    using C16 = ColCfg<144, 4, 6, 6, 16, 384>;        // cfg1's transform, dense LDS image
    using C8 = ColCfg<2112, 6, 16, 22, 8, 768>;       // cfg3's, padded LDS image
    using C4 = ColCfg<2560, 8, 32, 10, 4, 1024>;
    using CS = ColCfg<576, 6, 8, 12, 16, 768>;        // cfg2's: the 1088 window on the 1152 transform
    run_config<C16>("T=16", 270, 272, 13, 11, true, 288, rect_list(288, 16));
    run_config<C8>("T=8", 4206, 272, 13, 11, true, 4224, rect_list(4224, 8));
    run_config<C4>("T=4", 5102, 272, 13, 11, true, 5120, rect_list(5120, 4));
    // rows up to the last one of a window that is shorter than its transform (rows 1088 .. 1151 of the transform belong to nobody)
    run_config<CS>("short window", 1060, 270, 20, 11, false, 1088, {{1001, 9, 87, 21}, {0, 0, 1088, 288}, {1086, 16, 2, 16}});
    printf("%d ok, %d failed\n%s\n", g_ok, g_failures, g_failures ? "FAILED" : "all bit-equal");
    return g_failures ? 1 : 0;
}

int cmd_validate() {
    const long cases[][4] = {
        {0, 0, 288, 288}, {6, 5, 270, 272}, {287, 287, 1, 1}, {0, 287, 288, 1}, {287, 0, 1, 288}, {1, 1, 287, 287},        // inside, touching the edges
        {1, 0, 288, 288}, {0, 1, 288, 288}, {0, 0, 289, 1}, {0, 0, 1, 289}, {288, 0, 1, 1}, {0, 288, 1, 1},                // leaving the window
        {-1, 0, 10, 10}, {0, -1, 10, 10}, {0, 0, 0, 10}, {0, 0, 10, 0}, {0, 0, -3, 10}, {0, 0, 10, -3},                     // negative offsets, empty and negative sizes
        {2147483647, 0, 2147483647, 1}, {0, 2147483647, 1, 2147483647},                                                      // sums beyond an int
    };
    for (const auto& c : cases) {
        const char* why = output_rect_error(c[0], c[1], c[2], c[3], 288, 288);
        printf("%ld %ld %ld %ld | %s\n", c[0], c[1], c[2], c[3], why ? why : "ok");
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "bodies") return cmd_bodies();
    if (mode == "validate") return cmd_validate();
    fprintf(stderr, "usage: %s bodies | validate\n", argv[0]);
    return 2;
}
