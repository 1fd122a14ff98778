// pixel_format_host.cpp -- TEST-ONLY stand-alone host program for typed image pixels (fftconv_plan_set_images_typed).
//
// Built by tests/test_pixel_format_host.py with the host compiler from the product's kernel headers and the phase context of
// tests/emu/emu_runners.hpp; it is not the emulator library and not part of the product.  Modes:
//   bodies        runs fast_cols_fwd_body with every pixel type (uint8, uint16, fp16, bf16) against the fp32 body on the values
//                 converted by ref_value below: a T = 16, a T = 8 and a T = 4 configuration, h_in even and odd, the pair load
//                 and the element load, ncols no multiple of T, three planes, an odd plane stride, the dynamic tile queue.
//                 The spectra must be bit-equal.
//   ncc           ncc_column_sums of every pixel type against the fp32 text on the converted values: the float64 sums bit-equal
//   convert OUT   OUT: for each of the 65 536 bit patterns two uint32 -- the fp32 bits of fc_f16_to_f32 and of fc_bf16_to_f32
//                 (the test compares them with NumPy's conversions)
//   loadform      prints pixel_pair_load_ok over a table of (pointer offset, pitch, plane stride, element size)
//   routes        the not-built table and the direct-route predicate of fast_paths.hpp
// Having its own main, it is also the place for a host sanitizer build (-fsanitize=address,undefined) of this code.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "emu_runners.hpp"
#include "ncc.hpp"

using namespace fc;
using emu::HostPhaseCtx;

namespace {

int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_failures++; printf("FAIL "); printf(__VA_ARGS__); printf("\n"); } } while (0)

uint32_t rnd32(uint32_t& s) {
    s = s * 1664525u + 1013904223u;
    return s >> 8;
}

// ---- the reference value of an element: floating-point arithmetic (ldexp on the fields), nothing shared with the integer
// ---- arithmetic of pixel_format.hpp
float ref_value(uint32_t e, int format) {
    if (format == FC_PIXEL_U8 || format == FC_PIXEL_U16) return (float)(double)e;
    const int mant = format == FC_PIXEL_F16 ? 10 : 7, ebits = format == FC_PIXEL_F16 ? 5 : 8, bias = format == FC_PIXEL_F16 ? 15 : 127;
    const double sign = (e >> 15) ? -1.0 : 1.0;
    const int ex = (int)((e >> mant) & ((1u << ebits) - 1u)), m = (int)(e & ((1u << mant) - 1u));
    if (ex == (1 << ebits) - 1) return (float)(m ? NAN : sign * INFINITY);
    if (ex == 0) return (float)(sign * std::ldexp((double)m, 1 - bias - mant));
    return (float)(sign * std::ldexp((double)((1 << mant) + m), ex - bias - mant));
}

// element i of a test image: the values every format has to get right first, then random bit patterns without Inf / NaN
uint32_t test_element(size_t i, int format, uint32_t& seed) {
    static const uint32_t u8s[] = {0, 255, 1, 128, 254};
    static const uint32_t u16s[] = {0, 65535, 255, 256, 32768, 1};
    static const uint32_t f16s[] = {0x0000, 0x8000, 0x0001, 0x8001, 0x03ff, 0x0400, 0x7bff /* 65504 */, 0xfbff, 0x3c00, 0x0200};
    static const uint32_t bf16s[] = {0x0000, 0x8000, 0x0001, 0x8001, 0x007f, 0x0080, 0x7f7f, 0xff7f, 0x3f80, 0x0040};
    const uint32_t r = rnd32(seed);
    if (format == FC_PIXEL_U8) return i < 5 ? u8s[i] : (r & 0xffu);
    if (format == FC_PIXEL_U16) return i < 6 ? u16s[i] : (r & 0xffffu);
    if (format == FC_PIXEL_F16) {
        if (i < 10) return f16s[i];
        uint32_t e = r & 0xffffu;
        if (((e >> 10) & 0x1fu) == 0x1fu) e &= ~0x4000u;      // no Inf / NaN
        if ((r >> 16) % 7 == 0) e &= 0x83ffu;                  // a share of subnormals
        return e;
    }
    if (i < 10) return bf16s[i];
    uint32_t e = r & 0xffffu;
    if (((e >> 7) & 0xffu) == 0xffu) e &= ~0x4000u;
    if ((r >> 16) % 7 == 0) e &= 0x807fu;
    return e;
}

struct Layout {
    const char* name;
    int pitch_extra;       // column pitch = h_in + pitch_extra
    int stride_extra;      // plane stride = ncols * pitch + stride_extra
    int base;              // the image starts `base` elements into its (aligned) allocation
};

// One launch of the forward column body over `planes` planes in fp32 and in the four typed formats, `nwg` workgroups.
template <class Cfg>
void run_fwd(const char* what, int H, int kh, int h_in, int ncols, int planes, const Layout& lay, bool dyn, int force_element) {
    PlanTuning tune;
    tune.path_mode = 2;
    tune.exact_window = true;
    Geometry g;
    Tables t;
    const FastColsInfo fi = fast_cols_lookup(Cfg::M);
    if (!make_geometry(g, t, H, 278, 1, kh, 11, tune) || !g.fast_cols.ok || !g.fast_fwd || g.M != Cfg::M || fi.R1 != Cfg::R1 || fi.R2 != Cfg::R2 ||
        fi.R3 != Cfg::R3 || fi.T != Cfg::T || fi.NT != Cfg::NT || h_in > 2 * Cfg::M) {
        g_failures++;
        printf("FAIL %s: the plan does not run the configuration this case names\n", what);
        return;
    }
    DeviceTables d;
    d.fc_tw1 = t.fcl.tw1.data(); d.fc_tw2 = t.fcl.tw2.data(); d.fc_pairs = t.fcl.pairs.data();
    static int queue[FC_QUEUE_WORDS];
    d.queue = dyn ? queue : nullptr;
    d.queue_fwd = dyn;
    const int pitch = h_in + lay.pitch_extra;
    const size_t stride = (size_t)ncols * pitch + lay.stride_extra;
    // the allocation ends with the last sample of the last column: a load past it is a fault under a sanitizer build
    const size_t used = (size_t)(planes - 1) * stride + (size_t)(ncols - 1) * pitch + h_in;
    const int out_pitch = round_up(ncols, 8);
    const size_t out_plane = (size_t)(Cfg::M + 1) * out_pitch;
    std::vector<c32> lds(Cfg::LDS_ELEMS);
    const int nwg = 3;
    for (int format = FC_PIXEL_U8; format <= FC_PIXEL_BF16; format++) {
        const size_t eb = fc_pixel_elem_bytes(format);
        uint32_t seed = 777u + (uint32_t)Cfg::M * 13u + (uint32_t)format;
        // (operator new aligns for any element pair; `base` moves the image off it)
        std::vector<uint8_t> raw8;
        std::vector<uint16_t> raw16;
        std::vector<float> f32(lay.base + used);
        if (eb == 1) raw8.assign(lay.base + used, 0); else raw16.assign(lay.base + used, 0);
        for (size_t i = 0; i < used; i++) {
            const uint32_t e = test_element(i, format, seed);
            if (eb == 1) raw8[lay.base + i] = (uint8_t)e; else raw16[lay.base + i] = (uint16_t)e;
            f32[lay.base + i] = ref_value(e, format);
        }
        const void* typed = eb == 1 ? (const void*)(raw8.data() + lay.base) : (const void*)(raw16.data() + lay.base);
        std::vector<c32> s32(out_plane * planes), spx(out_plane * planes);
        const uint32_t fill = 0xffc0dead;
        for (auto* v : {&s32, &spx})
            for (c32& z : *v) { memcpy(&z.x, &fill, 4); memcpy(&z.y, &fill, 4); }
        auto run = [&](auto px_tag, const void* in, std::vector<c32>& out, const PixelLoad& px) {
            using Px = decltype(px_tag);
            FastColsFwdArgs a = fast_cols_fwd_args(g, d, static_cast<const float*>(in), stride, pitch, h_in, ncols, planes, out.data(), out_plane, out_pitch, false);
            for (int wg = 0; wg < nwg; wg++) {
                for (int i = 0; i < Cfg::LDS_ELEMS; i++) lds[i] = mk(1e30f, -1e30f);
                HostPhaseCtx<ColFwdState> ctx(Cfg::NT);
                fast_cols_fwd_body<Cfg, Cfg::R2, Px>(ctx, lds.data(), a, wg, nwg, px);
            }
            return a;
        };
        run(float{}, f32.data() + lay.base, s32, PixelLoad{});
        FastColsFwdArgs ta = fast_cols_fwd_args(g, d, static_cast<const float*>(typed), stride, pitch, h_in, ncols, planes, spx.data(), out_plane, out_pitch, false);
        PixelLoad px = fast_cols_fwd_pixel_load(ta, format);
        const bool expect_wide = lay.pitch_extra % 2 == h_in % 2 && stride % 2 == 0 && lay.base % 2 == 0;
        CHECK((px.wide != 0) == expect_wide, "%s format %d: load form %d, expected %d", what, format, px.wide, (int)expect_wide);
        if (force_element) px.wide = 0;
        if (eb == 1) run(Pixel8{}, typed, spx, px); else run(Pixel16{}, typed, spx, px);
        size_t written = 0;
        for (const c32& z : s32) written += fc_float_bits(z.x) != fill;
        const bool same = memcmp(s32.data(), spx.data(), s32.size() * sizeof(c32)) == 0;
        const size_t expect = (size_t)(Cfg::M + 1) * ncols * planes;
        if (!same || written != expect || (dyn && queue[8 * FC_QUEUE_STRIDE] != 0)) {
            g_failures++;
            printf("FAIL %s format %d (%s loads): spectra %s, %zu written, %zu expected\n", what, format, px.wide ? "pair" : "element", same ? "equal" : "DIFFER",
                   written, expect);
        } else {
            printf("ok   %s format %d (%s loads): %zu spectrum values bit-equal\n", what, format, px.wide ? "pair" : "element", written);
        }
    }
}

int cmd_bodies() {
    // (M, R1, R2, R3, T, NT) as fast_paths.hpp lists them -- checked against fast_cols_lookup at run time
    using C16 = ColCfg<144, 4, 6, 6, 16, 384>;        // cfg1's transform
    using C8 = ColCfg<1152, 8, 12, 12, 8, 768>;
    using C4 = ColCfg<2560, 8, 32, 10, 4, 1024>;
    const Layout dense{"dense", 0, 0, 0};               // pitch = h_in, planes back to back: what the plan launches
    const Layout odd_plane{"odd plane stride", 0, 1, 0};
    const Layout padded{"even pitch for an odd h_in", 1, 0, 0};
    const Layout off_base{"odd base", 0, 0, 1};
    // T = 16: 21 columns (two tiles, the second of 5), three planes
    run_fwd<C16>("T=16 h_in even, dense", 276, 13, 276, 21, 3, dense, false, 0);
    run_fwd<C16>("T=16 h_in even, dense, element loads forced", 276, 13, 276, 21, 3, dense, false, 1);
    run_fwd<C16>("T=16 h_in odd, dense", 276, 13, 275, 21, 3, dense, false, 0);
    run_fwd<C16>("T=16 h_in odd, even pitch", 276, 13, 275, 20, 3, padded, false, 0);
    run_fwd<C16>("T=16 h_in even, odd plane stride", 276, 13, 276, 21, 3, odd_plane, false, 0);
    run_fwd<C16>("T=16 h_in even, odd base", 276, 13, 276, 21, 3, off_base, false, 0);
    run_fwd<C16>("T=16 h_in even, dynamic tile queue", 276, 13, 276, 21, 3, dense, true, 0);
    run_fwd<C16>("T=16 short columns", 276, 13, 37, 5, 2, dense, false, 0);
    // T = 8: 11 columns; T = 4: 5 columns
    run_fwd<C8>("T=8 h_in even, dense", 2292, 13, 2292, 11, 2, dense, false, 0);
    run_fwd<C8>("T=8 h_in odd, dense", 2292, 13, 2291, 11, 3, dense, false, 0);
    run_fwd<C8>("T=8 h_in odd, even pitch, dynamic tile queue", 2292, 13, 2291, 10, 2, padded, true, 0);
    run_fwd<C4>("T=4 h_in even, dense", 5108, 13, 5108, 5, 2, dense, false, 0);
    run_fwd<C4>("T=4 h_in odd, dense", 5108, 13, 5107, 5, 3, dense, false, 0);
    if (!g_failures) printf("all bit-equal\n");
    return g_failures;
}

int cmd_ncc() {
    const int H = 37;
    for (int format = FC_PIXEL_U8; format <= FC_PIXEL_BF16; format++) {
        uint32_t seed = 99u + (uint32_t)format;
        std::vector<uint8_t> c8(H);
        std::vector<uint16_t> c16(H);
        std::vector<float> cf(H);
        for (int i = 0; i < H; i++) {
            const uint32_t e = test_element((size_t)i, format, seed);
            c8[i] = (uint8_t)e; c16[i] = (uint16_t)e; cf[i] = ref_value(e, format);
        }
        PixelLoad px;
        px.format = format;
        size_t checked = 0;
        for (int box = 1; box <= 9; box += 4)
            for (int i = 0; i < H + box - 1; i++) {
                double a1, a2, b1, b2;
                ncc_column_sums(cf.data(), H, i, box, a1, a2);
                if (format == FC_PIXEL_U8) ncc_column_sums<Pixel8>(c8.data(), H, i, box, b1, b2, px);
                else ncc_column_sums<Pixel16>(c16.data(), H, i, box, b1, b2, px);
                CHECK(memcmp(&a1, &b1, 8) == 0 && memcmp(&a2, &b2, 8) == 0, "ncc_column_sums format %d box %d row %d: %a %a against %a %a", format, box, i, b1, b2, a1, a2);
                checked++;
            }
        printf("ok   ncc_column_sums format %d: %zu sums\n", format, checked);
    }
    if (!g_failures) printf("all bit-equal\n");
    return g_failures;
}

int cmd_convert(const char* out) {
    FILE* f = fopen(out, "wb");
    if (!f) return 1;
    PixelLoad h, b, u;
    h.format = FC_PIXEL_F16; b.format = FC_PIXEL_BF16; u.format = FC_PIXEL_U16;
    for (uint32_t e = 0; e < 65536u; e++) {
        const float v[2] = {pixel_value((uint16_t)e, h), pixel_value((uint16_t)e, b)};
        fwrite(v, 4, 2, f);
        // the helpers by name, the uint16 path and the program's own reference agree with them (NaN: stays NaN)
        const float fh = fc_f16_to_f32((uint16_t)e), fb = fc_bf16_to_f32((uint16_t)e), rh = ref_value(e, FC_PIXEL_F16), rb = ref_value(e, FC_PIXEL_BF16);
        CHECK(memcmp(&fh, &v[0], 4) == 0 && memcmp(&fb, &v[1], 4) == 0, "pixel_value and the named helper differ at %04x", e);
        CHECK(std::isnan(rh) ? std::isnan(fh) : memcmp(&fh, &rh, 4) == 0, "fp16 %04x: %a, reference %a", e, (double)fh, (double)rh);
        CHECK(std::isnan(rb) ? std::isnan(fb) : memcmp(&fb, &rb, 4) == 0, "bf16 %04x: %a, reference %a", e, (double)fb, (double)rb);
        CHECK(pixel_value((uint16_t)e, u) == (float)e, "uint16 %u", e);
        if (e < 256) CHECK(pixel_value((uint8_t)e, PixelLoad{FC_PIXEL_U8, 0}) == (float)e, "uint8 %u", e);
        // a pair load gives the two elements' values, low address first
        const uint16_t two[2] = {(uint16_t)e, (uint16_t)(e * 40503u + 1u)};
        float x0, x1;
        pixel_pair(two, h, x0, x1);
        const float w1 = fc_f16_to_f32(two[1]);
        CHECK(memcmp(&x0, &fh, 4) == 0 && memcmp(&x1, &w1, 4) == 0, "pair load of 16-bit elements at %04x", e);
        const uint8_t b2[2] = {(uint8_t)e, (uint8_t)(e >> 8)};
        pixel_pair(b2, PixelLoad{FC_PIXEL_U8, 1}, x0, x1);
        CHECK(x0 == (float)(e & 255u) && x1 == (float)(e >> 8), "pair load of bytes at %04x", e);
    }
    fclose(f);
    return g_failures;
}

int cmd_loadform() {
    // (pointer offset in elements from a 16-byte boundary, pitch, plane stride, element size)
    alignas(16) static unsigned char buf[64];
    for (int off = 0; off < 4; off++)
        for (long pitch : {8L, 9L, 275L, 276L})
            for (size_t stride : {(size_t)64, (size_t)65, (size_t)75900, (size_t)75625})
                for (size_t eb : {(size_t)1, (size_t)2, (size_t)4})
                    printf("%d %ld %zu %zu %d\n", off, pitch, stride, eb, (int)pixel_pair_load_ok(reinterpret_cast<uintptr_t>(buf + off * eb), pitch, stride, eb));
    return 0;
}

int cmd_routes() {
    std::vector<int> configs;
#define FC_X(MM, A, B, C, TT, NTT) configs.push_back(MM);
    FC_FAST_COL_CONFIGS(FC_X)
#undef FC_X
    printf("configs");
    for (int M : configs) printf(" %d", M);
    printf("\nnot_built");
    for (int x : FC_COLS_FWD_PX_NOT_BUILT) {
        printf(" %d", x);
        bool is_config = false;
        for (int M : configs) is_config = is_config || M == x;
        CHECK(is_config, "%d is listed as not built and is no configuration", x);
    }
    printf("\n");
    long ones = 0, walked = 0, built = 0;
    std::vector<int> ms = configs;
    ms.push_back(56);      // a generic / Bluestein plan: no configuration
    for (int M : configs) built += fast_cols_fwd_px_built(M);
    for (int M : ms)
        for (int store = 0; store < 2; store++)
            for (int blockwise = 0; blockwise < 2; blockwise++)
                for (int fast_fwd = 0; fast_fwd < 2; fast_fwd++) {
                    bool listed = false;
                    for (int x : FC_COLS_FWD_PX_NOT_BUILT) listed = listed || x == M;
                    const bool want = store && !blockwise && fast_fwd && fast_cols_lookup(M).ok && !listed;
                    const bool got = fast_cols_fwd_px_direct(store, blockwise, fast_fwd, M);
                    CHECK(got == want, "pixel_direct(M %d, store %d, block-wise %d, fast_fwd %d) = %d", M, store, blockwise, fast_fwd, (int)got);
                    ones += got;
                    walked++;
                }
    CHECK(ones == built, "%ld settings read 1, %ld configurations are built", ones, built);
    printf("ok   direct predicate: %ld settings walked, %ld read 1\n", walked, ones);
    CHECK(fc_pixel_elem_bytes(FC_PIXEL_F32) == 4 && fc_pixel_elem_bytes(FC_PIXEL_U8) == 1 && fc_pixel_elem_bytes(FC_PIXEL_U16) == 2 &&
          fc_pixel_elem_bytes(FC_PIXEL_F16) == 2 && fc_pixel_elem_bytes(FC_PIXEL_BF16) == 2, "element sizes");
    CHECK(!fc_pixel_format_ok(-1) && fc_pixel_format_ok(0) && fc_pixel_format_ok(4) && !fc_pixel_format_ok(5), "format range");
    return g_failures;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "bodies") return cmd_bodies() ? 1 : 0;
    if (mode == "ncc") return cmd_ncc() ? 1 : 0;
    if (mode == "convert" && argc == 3) return cmd_convert(argv[2]) ? 1 : 0;
    if (mode == "loadform") return cmd_loadform();
    if (mode == "routes") return cmd_routes() ? 1 : 0;
    fprintf(stderr, "usage: pixel_format_host bodies | ncc | convert OUT | loadform | routes\n");
    return 2;
}
