// map_format_host.cpp -- TEST-ONLY stand-alone host program for the 16-bit result maps (plan option "map_format").
//
// Built by tests/test_map_format_host.py with the host compiler from the product's kernel headers and the phase context of
// tests/emu/emu_runners.hpp; it is not the emulator library and not part of the product.  Modes:
//   bodies            runs the output-kernel bodies (fast_cols_body for one configuration of each tile width, tiled and
//                     row-major, a sliced and a dynamic-queue launch shape; cols_c2r_body on a generic plan) in fp32 and in
//                     both 16-bit formats on the same intermediate.  The 16-bit maps must equal the fp32 maps converted by
//                     ref_f16 / ref_bf16 below, bit for bit.
//   convert IN OUT    IN: float32 values; OUT: per value four uint16 -- fc_map16 as fp16, as bf16, and the low / high half of
//                     fc_pack_map16(x, -x) ... see cmd_convert (the test compares them with NumPy's conversions)
//   options           prints map_format_error(value, blockwise) for every value in -1 .. 3, both ways
// Having its own main, it is also the place for a host sanitizer build (-fsanitize=address,undefined) of this code.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "emu_runners.hpp"

using namespace fc;
using emu::HostCtx;
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
uint16_t ref_f16(float x) { return ref_bits(x, 10, -14, 15, 0x7c00u, 0x7e00u); }
uint16_t ref_bf16(float x) { return ref_bits(x, 7, -126, 127, 0x7f80u, 0x7fc0u); }
uint16_t ref16(float x, int format) { return format == FC_MAP_BF16 ? ref_bf16(x) : ref_f16(x); }

int g_failures = 0;

// every map element: 16-bit output against the converted fp32 output; an element the fp32 run left alone keeps its fill pattern
void compare(const char* what, const std::vector<float>& f32, const std::vector<uint16_t>& h, int format, size_t expect_written) {
    size_t bad = 0, written = 0, first = 0;
    for (size_t i = 0; i < f32.size(); i++) {
        const bool wrote32 = fc_float_bits(f32[i]) != 0xffc0dead;
        written += wrote32;
        const bool ok = h[i] == (wrote32 ? ref16(f32[i], format) : 0xdead);
        if (!ok && !bad++) first = i;
    }
    if (bad || written != expect_written) {
        g_failures++;
        printf("FAIL %s format %d: %zu of %zu elements differ (first at %zu: fp32 %a -> %04x, want %04x), %zu written, %zu expected\n", what, format, bad,
               f32.size(), first, (double)f32[first], h[first], ref16(f32[first], format), written, expect_written);
    } else {
        printf("ok   %s format %d: %zu elements bit-equal\n", what, format, written);
    }
}

// values whose magnitudes sweep 2^-30 .. 2^20 over the columns: fp16 subnormals, zeros and overflows all occur in the maps
float col_scale(int w) { return std::ldexp(1.0f, (w * 7) % 51 - 30); }
float rnd(uint32_t& s) {
    s = s * 1664525u + 1013904223u;
    return (float)((int32_t)(s >> 8) - (1 << 23)) / (float)(1 << 23);
}

enum Shape { PLAIN, SLICED, DYN };

// One output launch of a plan in all three formats.  The instantiation and its arguments come from the product's launch layer
// (fast_cols_launch_shape / fast_cols_visit_variant), with the emulator's grids: 3 workgroups share the tiles of an unsliced
// launch, 8 a sliced one (two full rounds and a sliced tail at 18 tiles), chunks of two tiles from the dynamic queue.
template <class Cfg>
void run_fast_cols(const char* what, int H, int W, int kh, int kw, int path_mode, Shape shape) {
    PlanTuning tune;
    tune.path_mode = path_mode;
    tune.exact_window = true;
    Geometry g;
    Tables t;
    const FastColsInfo fi = fast_cols_lookup(Cfg::M);
    if (!make_geometry(g, t, H, W, 1, kh, kw, tune) || !g.fast_cols.ok || g.M != Cfg::M || fi.R1 != Cfg::R1 || fi.R2 != Cfg::R2 || fi.R3 != Cfg::R3 ||
        fi.T != Cfg::T || fi.NT != Cfg::NT || g.y_tiled() != (path_mode == 2)) {
        g_failures++;
        printf("FAIL %s: the plan does not run the configuration this case names\n", what);
        return;
    }
    DeviceTables d;
    d.fc_tw1 = t.fcl.tw1.data(); d.fc_tw2 = t.fcl.tw2.data(); d.fc_pairs = t.fcl.pairs.data(); d.fc_rowoff = t.fcl.rowoff.data();
    static int queue[FC_QUEUE_WORDS];
    d.queue = shape == DYN ? queue : nullptr;
    std::vector<c32> Y(g.y_elems_per_kernel());
    uint32_t seed = 12345u + (uint32_t)Cfg::M;
    for (size_t i = 0; i < Y.size(); i++) {
        const int w = g.y_tiled() ? (int)(i / ((size_t)g.tile_rows() * g.y_tile_w)) * g.y_tile_w + (int)(i % g.y_tile_w) : (int)(i % g.y_pitch);
        const float s = col_scale(w);
        Y[i] = mk(s * rnd(seed), s * rnd(seed));
    }
    std::vector<c32> lds(FC_LDS_BUDGET / sizeof(c32));
    const size_t ne = g.map_elems();
    std::vector<float> f32(ne);
    std::vector<uint16_t> h16(ne);
    for (int format = FC_MAP_F32; format <= FC_MAP_BF16; format++) {
        const uint32_t fill = 0xffc0dead;
        for (size_t i = 0; i < ne; i++) { if (format == FC_MAP_F32) memcpy(&f32[i], &fill, 4); else h16[i] = 0xdead; }
        float* out = format == FC_MAP_F32 ? f32.data() : reinterpret_cast<float*>(h16.data());
        const FastColsArgs a = fast_cols_args(g, d, Y.data(), out, 0, 1, format);
        FastColsShape sh = fast_cols_launch_shape(Cfg::M, Cfg::T, a, shape == SLICED ? 8 : 1 << 20);
        const FastColsVariant want = shape == SLICED ? FastColsVariant::TILED_SLICED : shape == DYN ? FastColsVariant::TILED_DYN
                                     : path_mode == 2 ? FastColsVariant::TILED : FastColsVariant::ROW_MAJOR;
        if (sh.variant != want) { g_failures++; printf("FAIL %s: launch shape %d, wanted %d\n", what, (int)sh.variant, (int)want); return; }
        if (sh.variant == FastColsVariant::TILED_DYN) sh.a.queue_shift = 1;
        if (sh.variant != FastColsVariant::TILED_SLICED) sh.grid = 3;
        fast_cols_visit_variant<Cfg>(sh.variant, [&](auto tiled, auto sliced, auto dyn) {
            for (int wg = 0; wg < sh.grid; wg++) {
                for (int i = 0; i < Cfg::LDS_ELEMS; i++) lds[i] = mk(1e30f, -1e30f);
                HostPhaseCtx<std::conditional_t<tiled.value, ColPairState<Cfg>, ColState<Cfg>>> ctx(Cfg::NT);
                if (format == FC_MAP_F32) fast_cols_body<Cfg, tiled.value, sliced.value, dyn.value>(ctx, lds.data(), sh.a, wg, sh.grid);
                else fast_cols_body<Cfg, tiled.value, sliced.value, dyn.value, ColStore::PAIRS16>(ctx, lds.data(), sh.a, wg, sh.grid);
            }
        });
        if (format != FC_MAP_F32) compare(what, f32, h16, format, ne);
    }
}

// the generic output kernel's body (direct transform, or Bluestein where the window does not factor)
void run_generic(const char* what, int H, int W, int kh, int kw, bool exact) {
    PlanTuning tune;
    tune.path_mode = 0;
    tune.exact_window = exact;
    Geometry g;
    Tables t;
    if (!make_geometry(g, t, H, W, 1, kh, kw, tune) || g.fast_cols.ok) { g_failures++; printf("FAIL %s: no generic plan\n", what); return; }
    DeviceTables d;
    d.tw_m = t.pm.tw.data(); d.tw_w = t.pw.tw.data(); d.pairs = t.pairs.data();
    std::vector<c32> Y(g.y_elems_per_kernel());
    uint32_t seed = 777u;
    for (size_t i = 0; i < Y.size(); i++) {
        const float s = col_scale((int)(i % g.y_pitch));
        Y[i] = mk(s * rnd(seed), s * rnd(seed));
    }
    std::vector<c32> lds(FC_LDS_BUDGET / sizeof(c32));
    const size_t ne = g.map_elems();
    std::vector<float> f32(ne);
    std::vector<uint16_t> h16(ne);
    HostCtx ctx;
    for (int format = FC_MAP_F32; format <= FC_MAP_BF16; format++) {
        const uint32_t fill = 0xffc0dead;
        for (size_t i = 0; i < ne; i++) { if (format == FC_MAP_F32) memcpy(&f32[i], &fill, 4); else h16[i] = 0xdead; }
        float* out = format == FC_MAP_F32 ? f32.data() : reinterpret_cast<float*>(h16.data());
        const ColsC2RArgs ca = cols_c2r_args(g, t, d, Y.data(), out, 0, format);
        for (int tile = 0; tile < tiles_for(g.fft_w, g.T_cols); tile++) {
            if (format == FC_MAP_F32) cols_c2r_body(ctx, lds.data(), ca, tile, 0);
            else cols_c2r_body<-1, true>(ctx, lds.data(), ca, tile, 0);
        }
        if (format != FC_MAP_F32) compare(what, f32, h16, format, ne);
    }
}

int cmd_bodies() {
    // (M, R1, R2, R3, T, NT) as fast_paths.hpp lists them -- checked against fast_cols_lookup at run time; every window is
    // 288 columns wide (18 layout tiles of 16 columns: 18 / 36 / 72 tiles of the output kernel)
    using C16 = ColCfg<144, 4, 6, 6, 16, 384>;        // cfg1's transform, dense LDS image
    using C8 = ColCfg<2112, 6, 16, 22, 8, 768>;       // cfg3's, padded LDS image
    using C4 = ColCfg<2560, 8, 32, 10, 4, 1024>;
    run_fast_cols<C16>("T=16 tiled", 276, 278, 13, 11, 2, PLAIN);
    run_fast_cols<C16>("T=16 row-major", 276, 278, 13, 11, 1, PLAIN);
    run_fast_cols<C16>("T=16 tiled, sliced tail round", 276, 278, 13, 11, 2, SLICED);
    run_fast_cols<C8>("T=8 tiled", 4212, 278, 13, 11, 2, PLAIN);
    run_fast_cols<C8>("T=8 row-major", 4212, 278, 13, 11, 1, PLAIN);
    run_fast_cols<C4>("T=4 tiled", 5108, 278, 13, 11, 2, PLAIN);
    run_fast_cols<C4>("T=4 row-major", 5108, 278, 13, 11, 1, PLAIN);
    run_fast_cols<C4>("T=4 tiled, dynamic tile queue", 5108, 278, 13, 11, 2, DYN);
    run_generic("generic", 64, 64, 3, 3, false);
    run_generic("generic, Bluestein", 282, 40, 23, 9, true);      // 304 = 16 x 19 along h: M = 152 by chirp-z
    printf("%s\n", g_failures ? "FAILED" : "all bit-equal");
    return g_failures ? 1 : 0;
}

int cmd_convert(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    std::vector<float> x;
    float v;
    while (fread(&v, 4, 1, f) == 1) x.push_back(v);
    fclose(f);
    // per value: fc_map16 fp16, fc_map16 bf16, then the pair (x, -x) through fc_pack_map16: low half, high half, both formats
    std::vector<uint16_t> r;
    for (float xi : x) {
        r.push_back(fc_map16(xi, false));
        r.push_back(fc_map16(xi, true));
        for (int bf = 0; bf < 2; bf++) {
            const uint32_t w = fc_pack_map16(xi, -xi, bf != 0);
            r.push_back((uint16_t)(w & 0xffffu));
            r.push_back((uint16_t)(w >> 16));
        }
        r.push_back(ref_f16(xi));       // the test checks this program's own reference against NumPy as well
        r.push_back(ref_bf16(xi));
    }
    f = fopen(out, "wb");
    if (!f) return 2;
    fwrite(r.data(), 2, r.size(), f);
    fclose(f);
    return 0;
}

int cmd_options() {
    for (int blockwise = 0; blockwise < 2; blockwise++)
        for (long v = -1; v <= 3; v++) {
            const char* why = map_format_error(v, blockwise != 0);
            printf("%ld %d %s\n", v, blockwise, why ? why : "ok");
        }
    printf("bytes %zu %zu %zu\n", fc_map_elem_bytes(FC_MAP_F32), fc_map_elem_bytes(FC_MAP_F16), fc_map_elem_bytes(FC_MAP_BF16));
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "bodies") return cmd_bodies();
    if (mode == "convert" && argc == 4) return cmd_convert(argv[2], argv[3]);
    if (mode == "options") return cmd_options();
    fprintf(stderr, "usage: %s bodies | convert IN OUT | options\n", argv[0]);
    return 2;
}
