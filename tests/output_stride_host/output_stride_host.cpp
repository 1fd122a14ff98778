// output_stride_host.cpp -- TEST-ONLY stand-alone host program for strided result maps (fftconv_plan_set_output_stride; fast_cols.hpp:
// the RECT_STRIDE store; output_route.hpp: OutStore::RectStride).
//
// Built by tests/test_output_stride_host.py with the host compiler from the product's kernel headers and the phase context of
// tests/emu/emu_runners.hpp; it is not the emulator library and not part of the product.  Modes:
//   bodies     for one configuration of each tile width (T = 16, 8, 4) and for a window shorter than its transform: the unchanged
//              fast_cols_body stores the full fp32 window of two maps (the reference), then the RECT_STRIDE body stores a list of
//              extents, each at a list of strides, through fast_cols_stride_launch_shape, static deal and dynamic tile queue, into map
//              buffers with a poisoned band in front of and behind every map.  Every element of a strided map must equal the
//              window element window[off_h + i * sh, off_w + j * sw] bit for bit, every element must be written and nothing else.
//              The launch's tile count must be the number of distinct window tiles that hold a sampled column; the columns of every
//              other tile are NaN in the intermediate, so a tile index that strays there shows in the maps.
//   routes     plan_output_route with a stride set, over sink x region x score x format x stride_store x built x plan kind:
//              RectStride exactly under its conditions, a crop from the fp32 window everywhere else; with stride (1, 1) the answer
//              of the record without the new fields
//   validate   prints output_stride_error for a list of (stride_h, stride_w, region)
// Having its own main, it is also the place for a host sanitizer build (-fsanitize=address,undefined) of this code.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <set>
#include <string>
#include <vector>

#include "emu_runners.hpp"
#include "output_route.hpp"

using namespace fc;
using emu::HostPhaseCtx;

namespace {

int g_failures = 0, g_ok = 0;

float rnd(uint32_t& s) {
    s = s * 1664525u + 1013904223u;
    return (float)((int32_t)(s >> 8) - (1 << 23)) / (float)(1 << 23);
}

struct Extent { const char* name; int off_h, off_w, out_h, out_w; };
struct Stride { int sh, sw; };

// the extents of a 288-column window of fft_h rows
std::vector<Extent> extent_list(int fft_h, int T) {
    return {
        {"window", 0, 0, fft_h, 288},
        {"same", 6, 5, fft_h - 18, 272},
        {"odd", 5, 3, fft_h - 7, 283},                 // odd offsets, odd sizes
        {"one column", 7, T + 1, 33, 1},
        {"one row", 3, T - 1, 1, T + 3},               // one row across a tile boundary
        {"last element", fft_h - 1, 287, 1, 1},
    };
}
// the strides of an extent: the fixed list, two whose column stride drops whole tiles, and one beyond the extent in each dimension
std::vector<Stride> stride_list(const Extent& e, int T) {
    return {{2, 1}, {1, 2}, {2, 2}, {3, 5}, {4, 4}, {7, 3}, {1, T + 1}, {2, 2 * T + 3}, {e.out_h + 3, 1}, {1, e.out_w + 5}};
}

constexpr int NK = 2;              // maps per launch
constexpr size_t GUARD = 64;       // poisoned elements in front of and behind every map
constexpr uint32_t POISON32 = 0xffc0dead;

template <class Cfg>
void run_config(const char* what, int H, int W, int kh, int kw, bool exact, int want_fft_h) {
    PlanTuning tune;
    tune.path_mode = 2;
    tune.exact_window = exact;
    Geometry g;
    Tables t;
    const FastColsInfo fi = fast_cols_lookup(Cfg::M);
    if (!make_geometry(g, t, H, W, 1, kh, kw, tune) || !g.fast_cols.ok || g.M != Cfg::M || fi.R1 != Cfg::R1 || fi.R2 != Cfg::R2 || fi.R3 != Cfg::R3 ||
        fi.T != Cfg::T || fi.NT != Cfg::NT || !g.y_tiled() || g.fft_h != want_fft_h || g.fft_w != 288 || !fast_cols_stride_available(g.M, g.y_tiled())) {
        g_failures++;
        printf("FAIL %s: the plan does not run the configuration this case names (M %d, window %d x %d)\n", what, g.M, g.fft_h, g.fft_w);
        return;
    }
    constexpr int T = Cfg::T;
    DeviceTables d;
    d.fc_tw1 = t.fcl.tw1.data(); d.fc_tw2 = t.fcl.tw2.data(); d.fc_pairs = t.fcl.pairs.data(); d.fc_rowoff = t.fcl.rowoff.data();
    static int queue[FC_QUEUE_WORDS];
    const size_t yk = g.y_elems_per_kernel();
    std::vector<c32> Y(yk * NK);
    std::vector<int> col_of(yk);
    uint32_t seed = 9876u + (uint32_t)Cfg::M;
    for (size_t i = 0; i < yk; i++) col_of[i] = (int)(i / ((size_t)g.tile_rows() * g.y_tile_w)) * g.y_tile_w + (int)(i % g.y_tile_w);
    for (size_t i = 0; i < Y.size(); i++) Y[i] = mk(rnd(seed), rnd(seed));
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
        FastColsShape sh = fast_cols_launch_shape(Cfg::M, T, a, 1 << 20);
        if (sh.variant != FastColsVariant::TILED) { g_failures++; printf("FAIL %s: reference launch shape %d\n", what, (int)sh.variant); return; }
        sh.grid = 3;
        run_wgs(sh.grid, [&](auto& ctx, int wg) { fast_cols_body<Cfg, true>(ctx, lds.data(), sh.a, wg, sh.grid); });
        for (size_t i = 0; i < ref.size(); i++)
            if (fc_float_bits(ref[i]) == POISON32) { g_failures++; printf("FAIL %s: the reference left element %zu unwritten\n", what, i); return; }
    }

    std::vector<c32> Ys(Y.size());
    for (const Extent& e : extent_list(g.fft_h, T)) {
        if (output_rect_error(e.off_h, e.off_w, e.out_h, e.out_w, g.fft_h, g.fft_w)) {
            g_failures++;
            printf("FAIL %s: extent %s is not inside the window\n", what, e.name);
            continue;
        }
        for (const Stride& st : stride_list(e, T)) {
            const int mh = strided_count(e.out_h, st.sh), mw = strided_count(e.out_w, st.sw);
            // the window tiles that hold a sampled column; the columns of every other tile are NaN in the intermediate
            std::set<int> tiles;
            for (int j = 0; j < mw; j++) tiles.insert((e.off_w + j * st.sw) / T);
            const float nan = std::numeric_limits<float>::quiet_NaN();
            for (size_t i = 0; i < Y.size(); i++) Ys[i] = tiles.count(col_of[i % yk] / T) ? Y[i] : mk(nan, nan);
            const size_t oe = (size_t)mh * mw, stride = oe + GUARD;
            const bool even = e.off_h % 2 == 0 && e.out_h % 2 == 0;
            struct Run { bool dyn; int shift; };       // shift: elements the first map is moved off its aligned position
            std::vector<Run> runs = {{false, 0}, {true, 1}};
            if (even && st.sh == 1) { runs.push_back({false, 1}); runs.push_back({true, 0}); }
            for (const Run& run : runs) {
                // [guard][map 0][guard][map 1][guard] (+ the shift), 16-byte aligned storage
                const size_t total = GUARD + NK * stride + 2;
                std::vector<uint64_t> store((total * 4 + 7) / 8 + 2);
                unsigned char* base = reinterpret_cast<unsigned char*>(store.data());
                for (size_t i = 0; i < total; i++) memcpy(base + 4 * i, &POISON32, 4);
                float* out = reinterpret_cast<float*>(base + (GUARD + (size_t)run.shift) * 4);
                d.queue = run.dyn ? queue : nullptr;
                const FastColsArgs a = fast_cols_args(g, d, Ys.data(), out, stride, NK, FC_MAP_F32);
                FastColsShape sh = fast_cols_stride_launch_shape(T, a, e.off_h, e.off_w, e.out_h, e.out_w, st.sh, st.sw, 1 << 20);
                const bool want_wide = even && st.sh == 1 && run.shift == 0;
                const int want_tiles = (int)tiles.size() * NK;
                if (!sh.strided || (sh.variant == FastColsVariant::TILED_DYN) != run.dyn || (sh.variant != FastColsVariant::TILED_DYN && sh.variant != FastColsVariant::TILED) ||
                    sh.a.rect_wide != (want_wide ? 1 : 0) || sh.a.ntiles != want_tiles || sh.grid != want_tiles || sh.a.out_pitch != mh ||
                    (sh.stride.tile_step != 0) != ((st.sw < e.out_w ? st.sw : e.out_w) > T)) {
                    g_failures++;
                    printf("FAIL %s %s stride (%d, %d): launch shape: variant %d, wide %d, %d tiles (want %d) on %d workgroups, pitch %d, tile step %d\n", what, e.name,
                           st.sh, st.sw, (int)sh.variant, sh.a.rect_wide, sh.a.ntiles, want_tiles, sh.grid, sh.a.out_pitch, sh.stride.tile_step);
                    continue;
                }
                if (run.dyn) sh.a.queue_shift = 1;
                sh.grid = sh.a.ntiles < 3 ? sh.a.ntiles : 3;
                run_wgs(sh.grid, [&](auto& ctx, int wg) {
                    if (run.dyn) fast_cols_body<Cfg, true, false, true, ColStore::RECT_STRIDE>(ctx, lds.data(), sh.a, wg, sh.grid, sh.stride);
                    else fast_cols_body<Cfg, true, false, false, ColStore::RECT_STRIDE>(ctx, lds.data(), sh.a, wg, sh.grid, sh.stride);
                });
                // the queue's counters are zero again after the launch
                bool queue_zero = true;
                for (int i = 0; i < FC_QUEUE_WORDS; i++) queue_zero = queue_zero && queue[i] == 0;
                // every element of the buffer: inside a map the window element, everywhere else the poison
                size_t bad = 0, first = 0, written = 0, stray = 0;
                for (size_t i = 0; i < total; i++) {
                    uint32_t got = 0;
                    memcpy(&got, base + 4 * i, 4);
                    const long rel = (long)i - (long)(GUARD + run.shift);
                    const long k = rel >= 0 ? rel / (long)stride : -1, el = rel >= 0 ? rel % (long)stride : 0;
                    if (k >= 0 && k < NK && (size_t)el < oe) {
                        const int w = e.off_w + (int)(el / mh) * st.sw, h = e.off_h + (int)(el % mh) * st.sh;
                        const uint32_t want = fc_float_bits(ref[(size_t)k * ne + (size_t)w * g.fft_h + h]);
                        if (got != want && !bad++) first = i;
                        written += got != POISON32;
                    } else if (got != POISON32) {
                        stray++;
                    }
                }
                if (bad || stray || written != NK * oe || !queue_zero) {
                    g_failures++;
                    printf("FAIL %s %s (%d, %d, %d, %d) stride (%d, %d) %s shift %d: %zu elements differ (first at %zu), %zu stray stores, %zu written of %zu, queue %s\n",
                           what, e.name, e.off_h, e.off_w, e.out_h, e.out_w, st.sh, st.sw, run.dyn ? "dynamic" : "static", run.shift, bad, first, stray, written, NK * oe,
                           queue_zero ? "zero" : "NOT zero");
                } else {
                    g_ok++;
                    printf("ok   %s %s (%d, %d, %d, %d) stride (%d, %d) %s shift %d %s: %d x %d maps, %zu elements bit-equal on %d tiles, guards intact\n", what, e.name,
                           e.off_h, e.off_w, e.out_h, e.out_w, st.sh, st.sw, run.dyn ? "dynamic" : "static", run.shift, sh.a.rect_wide ? "wide" : "elementwise", mh, mw,
                           written, want_tiles);
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
    run_config<C16>("T=16", 270, 272, 13, 11, true, 288);
    run_config<C8>("T=8", 4206, 272, 13, 11, true, 4224);
    run_config<C4>("T=4", 5102, 272, 13, 11, true, 5120);
    run_config<CS>("short window", 1060, 270, 20, 11, false, 1088);
    printf("%d ok, %d failed\n%s\n", g_ok, g_failures, g_failures ? "FAILED" : "all bit-equal");
    return g_failures ? 1 : 0;
}

bool same_route(const OutputRoute& a, const OutputRoute& b) {
    return ((a.error == nullptr) == (b.error == nullptr)) && a.route == b.route && a.plane == b.plane && a.store == b.store && a.kernel_format == b.kernel_format &&
           a.map_format == b.map_format && a.target == b.target && a.extent == b.extent && a.after == b.after && a.need_O == b.need_O && a.staging == b.staging &&
           a.staging_copies == b.staging_copies && a.pinned_one_map == b.pinned_one_map && a.probe == b.probe;
}

int cmd_routes() {
    long combos = 0, direct = 0, staged = 0, wrong = 0, unit = 0, unit_wrong = 0;
    const SinkKind sinks[] = {SinkKind::Packed, SinkKind::DevicePtrs, SinkKind::Host};
    struct Kind { bool fast_cols, y_tiled, blockwise; };
    const Kind kinds[] = {{true, true, false}, {true, false, false}, {false, false, false}, {true, true, true}};
    const Stride strides[] = {{2, 2}, {1, 3}, {4, 1}};
    for (SinkKind sink : sinks)
        for (long host_stream = 0; host_stream <= 2; host_stream += 2)
            for (size_t map_bytes : {(size_t)4096, (size_t)8 << 20})
                for (long region = 0; region <= 5; region++)
                    for (long score = 0; score <= 4; score++)
                        for (int format = FC_MAP_F32; format <= FC_MAP_BF16; format++)
                            for (int stride_store = 0; stride_store <= 1; stride_store++)
                                for (int built = 0; built <= 1; built++)
                                    for (const Kind& k : kinds) {
                                        OutputRouteIn in;
                                        in.sink = sink; in.map_bytes = map_bytes; in.host_stream = host_stream; in.host_min_kb = 1024; in.host_pinned = true;
                                        in.region = region; in.rect_store = true; in.score = score; in.norm_store = true; in.blockwise = k.blockwise;
                                        in.map_format = format; in.fast_cols = k.fast_cols; in.y_tiled = k.y_tiled;
                                        in.rect_built = in.norm_built = in.sqdiff_built = true;
                                        // stride (1, 1), whatever the other new fields say: the answer of the record without them
                                        {
                                            const OutputRoute plain = plan_output_route(in);
                                            OutputRouteIn one = in;
                                            one.stride_store = stride_store != 0; one.stride_built = built != 0;
                                            unit++;
                                            if (!same_route(plain, plan_output_route(one))) unit_wrong++;
                                        }
                                        if (region == 4) continue;      // (refused with a stride: output_stride_error)
                                        for (const Stride& st : strides) {
                                            in.stride_h = st.sh; in.stride_w = st.sw; in.stride_store = stride_store != 0; in.stride_built = built != 0;
                                            const OutputRoute r = plan_output_route(in);
                                            combos++;
                                            const bool want = stride_store && built && k.fast_cols && k.y_tiled && !k.blockwise && format == FC_MAP_F32 &&
                                                              (region == 0 || region == 5) && (score == 0 || score == FC_SCORE_CCOEFF);
                                            bool ok = !r.error && r.map_format == format;
                                            if (want) {
                                                direct++;
                                                ok = ok && r.store == OutStore::RectStride && r.after == OutAfter::None && !r.need_O && r.kernel_format == FC_MAP_F32 &&
                                                     r.plane == OutPlane::None && r.probe == TuneProbe::Rect &&
                                                     r.target == (r.staged() ? OutBuffer::OC : OutBuffer::Caller);
                                            } else {
                                                staged++;
                                                ok = ok && r.store != OutStore::RectStride && r.store != OutStore::Rect && !r.fused() && r.after == OutAfter::Crop &&
                                                     r.kernel_format == FC_MAP_F32 && r.need_O && r.target == OutBuffer::O &&
                                                     r.store == (k.fast_cols ? OutStore::Plain : OutStore::Generic);
                                            }
                                            ok = ok && r.staging == (r.staged() ? OutBuffer::OC : OutBuffer::Caller);
                                            if (!ok) {
                                                if (!wrong++)
                                                    printf("FAIL first wrong route: sink %d region %ld score %ld format %d stride_store %d built %d kind (%d, %d, %d): store %d after %d\n",
                                                           (int)sink, region, score, format, stride_store, built, k.fast_cols, k.y_tiled, k.blockwise, (int)r.store, (int)r.after);
                                            }
                                        }
                                    }
    printf("routes: %ld combinations with a stride, %ld RectStride, %ld cropped, %ld wrong\n", combos, direct, staged, wrong);
    printf("unit stride: %ld combinations, %ld differ from the record without the new fields\n", unit, unit_wrong);
    return wrong || unit_wrong || !direct || !staged ? 1 : 0;
}

int cmd_validate() {
    const long cases[][3] = {
        {1, 1, 0}, {2, 3, 0}, {1000000, 1, 0}, {2, 2, 1}, {2, 2, 2}, {2, 2, 3}, {2, 2, 5}, {1, 1, 4},      // fine
        {0, 1, 0}, {1, 0, 0}, {-2, 2, 0}, {2, -2, 5}, {0, 0, 4},                                         // a stride below 1
        {2, 1, 4}, {1, 2, 4}, {3, 3, 4},                                                                 // region 4 with a stride
    };
    for (const auto& c : cases) {
        const char* why = output_stride_error(c[0], c[1], c[2]);
        printf("%ld %ld %ld | %s\n", c[0], c[1], c[2], why ? why : "ok");
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "bodies") return cmd_bodies();
    if (mode == "routes") return cmd_routes();
    if (mode == "validate") return cmd_validate();
    fprintf(stderr, "usage: %s bodies | routes | validate\n", argv[0]);
    return 2;
}
