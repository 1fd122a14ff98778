// output_route_host.cpp -- TEST-ONLY stand-alone host program for csrc/output_route.hpp (plan_output_route: the way of a group's maps
// out of a plan, decided once per group).
//
// Built by tests/test_output_route_host.py with the host compiler from the product's headers alone.  Modes:
//   table    plan_output_route against a literal transcription of the conditions it replaced, as they stood in the commit before
//            the route existed (the predicates of plan_internal.hpp and fast_paths.hpp, plan_delivery, the branch orders of
//            launch_output_cols and launch_region, deliver_batch and the tuner's call in fftconv_api.cpp, the tuner's own reads in
//            placement.cpp; file and line are in the comments), over the full product of the axes listed in cmd_table -- the number
//            of combinations is printed, and the test holds it against the product
//   named    the routes the library documents, one line each, against expectations written by hand
// Having its own main, it is also the place for a host sanitizer build (-fsanitize=address,undefined) of this code.
#include <cstdio>
#include <cstring>

#include "fast_paths.hpp"
#include "output_route.hpp"

using namespace fc;

namespace {

int g_failures = 0;

// ---- the transcription ----
// the plan and the sink as the parent's conditions read them
struct Plan {
    bool window = false, packed = false, host = false;      // Sink::window, Sink::packed, Sink::location == FFTCONV_HOST
    long opt_host_stream = 0, opt_host_min_kb = 0, opt_host_pinned = 0;
    long opt_region = 0, opt_rect_store = 0, opt_score = 0, opt_norm_store = 0, opt_map_format = 0;
    bool tiled = false;                                     // block-wise
    bool fast_cols_ok = false, y_tiled = false;
    int M = 0;
    size_t out_elems = 0;
    size_t elem_bytes() const { return fc_map_elem_bytes((int)opt_map_format); }
    bool score_planes() const { return score_has_plane(opt_score); }                                        // plan_internal.hpp:286
    bool rect_direct() const {                                                                              // plan_internal.hpp:262
        return opt_region == 5 && opt_rect_store && !score_has_plane(opt_score) && !tiled && fast_cols_rect_available(M, y_tiled);
    }
    bool norm_direct() const;                                                                               // plan_internal.hpp:287
};
bool parent_fast_cols_norm_direct(bool normalise, bool norm_store, bool blockwise, int map_format, long region, int M, bool y_tiled) {      // fast_paths.hpp:663
    return normalise && norm_store && !blockwise && map_format == FC_MAP_F32 && (region == 0 || region == 5) && fast_cols_norm_available(M, y_tiled);
}
bool parent_fast_cols_score_direct(int score, bool norm_store, bool blockwise, int map_format, long region, int M, bool y_tiled) {          // fast_paths.hpp:694
    if (score == FC_SCORE_SQDIFF)
        return norm_store && !blockwise && map_format == FC_MAP_F32 && (region == 0 || region == 5) && fast_cols_sqdiff_available(M, y_tiled);
    return parent_fast_cols_norm_direct(score == FC_SCORE_CCOEFF_NORMED || score == FC_SCORE_CCORR_NORMED, norm_store, blockwise, map_format, region, M, y_tiled);
}
bool Plan::norm_direct() const { return parent_fast_cols_score_direct((int)opt_score, opt_norm_store != 0, tiled, (int)opt_map_format, opt_region, M, y_tiled); }

struct Parent {
    int error = 0;               // plan_delivery: 0 none, 1 "... needs the specialised output kernel", 2 "... takes no normalisation"
    int route = 0;               // Route, in the order of the enum
    bool cropped = false, rect = false, norm = false, norm_fused = false;      // Delivery
    int stage = 0;               // 0 O, 1 OC
    int kernel_format = 0;
    bool staged = false, ensure_O = false;
    int stage_copies = 0;        // what multiplies oe * nbY in the staging buffer's size; 0: not ensured
    int cols_branch = 0;         // launch_output_cols: 0 fused SQDIFF, 1 fused CCORR_NORMED, 2 fused D, 3 rectangle, 4 plain specialised, 5 generic
    bool shape_plan_rect = false;      // output_norm_shape / output_sqdiff_shape: the plan's rectangle (else the whole window)
    int region_line = -1;        // launch_region (cropped only): 0 staged SQDIFF, 1 staged CCORR_NORMED, 2 staged D, 3 rectangle, 4 region
    bool region_pad = false, region_whole = false;
    bool pinned_one_map = false;       // deliver_batch: a launch of one map on the pinned route goes through deliver_pinned
    bool tuner_skipped = false, tuner_k0 = false, tuner_rect = false, tuner_direct = false;
    int tuner_out = 0, tuner_format = 0;      // `out`: 0 the caller's packed maps, 1 O, 2 OC
    bool opt_rect_direct = false, opt_norm_direct = false;      // read-only options "rect_direct", "norm_direct"
};

Parent parent_route(const Plan& p) {
    Parent r;
    // fftconv_api.cpp:202-233, plan_delivery
    if (p.window && !p.fast_cols_ok) r.error = 1;                                                           // :204
    else if (p.window && p.opt_score) r.error = 2;                                                          // :205
    r.rect = !p.window && p.rect_direct();                                                                  // :206
    r.norm = p.score_planes();                                                                              // :207
    r.norm_fused = r.norm && !p.window && p.norm_direct();                                                  // :208
    r.cropped = ((p.opt_region != 0 && !r.rect) || r.norm) && !r.norm_fused;                                // :209
    r.stage = (r.cropped || r.rect || r.norm_fused) ? 1 : 0;                                                // :210
    r.kernel_format = r.cropped ? FC_MAP_F32 : (int)p.opt_map_format;                                       // :213
    const size_t map_bytes = p.out_elems * p.elem_bytes();                                                  // :214
    if (p.window) r.route = 1;                                                                              // :221
    else if (p.packed) r.route = 0;                                                                         // :222
    else if (!p.host) r.route = 2;                                                                          // :223
    else if (p.opt_host_stream != 0 && map_bytes >= ((size_t)p.opt_host_min_kb << 10)) r.route = 4;         // :224
    else if (p.opt_host_pinned && map_bytes <= FC_PIN_OUT_BYTES / 2) r.route = 3;                           // :225
    else r.route = 2;                                                                                       // :226
    r.staged = r.route == 2 || r.route == 3 || r.route == 4;                                                // :199
    r.ensure_O = r.cropped;                                                                                 // :227
    if (r.staged) r.stage_copies = r.route == 4 ? 2 : 1;                                                    // :229-230
    // fftconv_api.cpp:304-346, launch_output_cols(..., rect = d.rect, norm_fused = d.norm_fused)
    if (r.norm_fused && p.opt_score == FC_SCORE_SQDIFF) r.cols_branch = 0;                                  // :308
    else if (r.norm_fused && p.opt_score == FC_SCORE_CCORR_NORMED) r.cols_branch = 1;                       // :313
    else if (r.norm_fused) r.cols_branch = 2;                                                               // :318
    else if (r.rect) r.cols_branch = 3;                                                                     // :323
    else if (p.fast_cols_ok) r.cols_branch = 4;                                                             // :328
    else r.cols_branch = 5;                                                                                 // :340
    r.shape_plan_rect = p.opt_region == 5;                                                                  // :285, :292
    // fftconv_api.cpp:503-539, launch_region(..., scale = d.norm ? ND : nullptr), called when d.cropped (:439)
    if (r.cropped) {
        if (r.norm) {                                                                                       // :507
            r.region_whole = !p.opt_region;                                                                 // :508-509
            r.region_line = p.opt_score == FC_SCORE_SQDIFF ? 0 : p.opt_score == FC_SCORE_CCORR_NORMED ? 1 : 2;      // :510, :519, :523
        } else r.region_line = p.opt_region == 5 ? 3 : 4;                                                   // :531, :534
        r.region_pad = p.opt_region == 4;                                                                   // :513, :525, :536
    }
    r.pinned_one_map = map_bytes <= FC_PIN_ONE_MAP_BYTES;                                                   // :381
    // fftconv_api.cpp:412-414, the tuner's call; placement.cpp:33-37, what it reads itself
    r.tuner_skipped = p.score_planes();                                                                     // :412
    r.tuner_out = r.cropped ? 1 : r.staged ? 1 + r.stage : 0;                                               // :414
    r.tuner_direct = !r.cropped && !r.staged;                                                               // :414
    r.tuner_format = r.kernel_format;                                                                       // :414
    r.tuner_k0 = p.window;                                                                                  // placement.cpp:33
    r.tuner_rect = !p.window && p.rect_direct();                                                            // placement.cpp:37
    r.opt_rect_direct = p.rect_direct();                                                                    // fftconv_api.cpp:1062
    r.opt_norm_direct = p.norm_direct();                                                                    // fftconv_api.cpp:1066
    return r;
}

const char* const kErrors[] = {nullptr, "an output window needs the specialised output kernel", "an output window takes no normalisation"};

// ---- the route of the same plan and sink: what plan_output.cpp's output_route_in fills in ----
OutputRouteIn route_in(const Plan& p) {
    OutputRouteIn in;
    in.sink = p.window ? SinkKind::Window : p.packed ? SinkKind::Packed : p.host ? SinkKind::Host : SinkKind::DevicePtrs;
    in.map_bytes = p.out_elems * p.elem_bytes();
    in.host_stream = p.opt_host_stream; in.host_min_kb = p.opt_host_min_kb; in.host_pinned = p.opt_host_pinned != 0;
    in.region = p.opt_region; in.rect_store = p.opt_rect_store != 0;
    in.score = p.opt_score; in.norm_store = p.opt_norm_store != 0;
    in.blockwise = p.tiled;
    in.map_format = (int)p.opt_map_format;
    in.fast_cols = p.fast_cols_ok; in.y_tiled = p.y_tiled;
    in.rect_built = fast_cols_rect_built(p.M); in.norm_built = fast_cols_norm_built(p.M); in.sqdiff_built = fast_cols_sqdiff_built(p.M);
    return in;
}

// how the stages read the route (plan_output.cpp, placement.cpp, fftconv_api.cpp), against the parent's answers
bool same(const Parent& a, const Plan& p, const OutputRoute& b) {
    bool ok = (a.error == 0 ? b.error == nullptr : b.error && !strcmp(b.error, kErrors[a.error]));
    ok = ok && a.route == (int)b.route && a.staged == b.staged();
    ok = ok && a.rect == (b.store == OutStore::Rect) && a.norm == (b.plane != OutPlane::None) && a.norm_fused == b.fused() && a.cropped == (b.after != OutAfter::None);
    ok = ok && a.kernel_format == b.kernel_format && (int)p.opt_map_format == b.map_format && a.ensure_O == b.need_O && a.stage_copies == b.staging_copies;
    if (a.staged) ok = ok && b.staging == (a.stage ? OutBuffer::OC : OutBuffer::O);
    else ok = ok && b.staging == OutBuffer::Caller;
    // launch_output_cols branches on the store, and on the plane for the fused line
    static const OutStore store_of[] = {OutStore::RectAdd, OutStore::RectScale, OutStore::RectScale, OutStore::Rect, OutStore::Plain, OutStore::Generic};
    static const OutPlane plane_of[] = {OutPlane::Q, OutPlane::Dc, OutPlane::D};
    ok = ok && b.store == store_of[a.cols_branch];
    if (a.cols_branch < 3) ok = ok && b.plane == plane_of[a.cols_branch] && a.shape_plan_rect == (b.extent != OutExtent::Window);
    if (a.cols_branch == 3) ok = ok && b.extent == OutExtent::Rect;
    // launch_region branches on the plane, then on the extent; pad or crop; the whole window as the crop of a plane on region 0
    if (a.cropped) {
        const int line = b.plane == OutPlane::Q ? 0 : b.plane == OutPlane::Dc ? 1 : b.plane == OutPlane::D ? 2 : b.extent == OutExtent::Rect ? 3 : 4;
        ok = ok && a.region_line == line && a.region_pad == (b.after == OutAfter::Pad) && a.region_whole == (b.extent == OutExtent::Window);
    }
    ok = ok && a.pinned_one_map == b.pinned_one_map;
    // the tuner: skipped, or called with the route -- `out` is the route's target
    ok = ok && a.tuner_skipped == (b.probe == TuneProbe::Skip);
    if (!a.tuner_skipped) {
        ok = ok && a.tuner_k0 == (b.probe == TuneProbe::None) && a.tuner_rect == (b.probe == TuneProbe::Rect) && a.tuner_direct == (b.target == OutBuffer::Caller);
        ok = ok && a.tuner_format == b.kernel_format;
    }
    ok = ok && a.tuner_out == (b.target == OutBuffer::O ? 1 : b.target == OutBuffer::OC ? 2 : 0);
    // the read-only options: the route of a sink that is not a window
    Plan q = p;
    q.window = false; q.packed = true;
    const OutputRoute o = plan_output_route(route_in(q));
    return ok && a.opt_rect_direct == (o.store == OutStore::Rect) && a.opt_norm_direct == o.fused();
}

constexpr int M_GENERIC = 56, M_BUILT = 144, M_NOT_BUILT = 544;      // no configuration; every family built; none of the rectangle family built
constexpr long HOST_MIN_KB = 1024;

// the output kernel of a plan: 0 generic, 1 specialised on the row-major intermediate, 2 specialised and tiled with every family
// built, 3 specialised and tiled at M = 544
void set_kernel(Plan& p, int kernel) {
    p.fast_cols_ok = kernel != 0;
    p.y_tiled = kernel >= 2;
    p.M = kernel == 0 ? M_GENERIC : kernel == 3 ? M_NOT_BUILT : M_BUILT;
}
// 0 window, 1 packed, 2 device pointers, 3 host
void set_sink(Plan& p, int sink) { p.window = sink == 0; p.packed = sink == 1; p.host = sink == 3; }

int cmd_table() {
    if (fast_cols_lookup(M_GENERIC).ok || !fast_cols_lookup(M_BUILT).ok || !fast_cols_lookup(M_NOT_BUILT).ok || !fast_cols_rect_built(M_BUILT) ||
        !fast_cols_norm_built(M_BUILT) || !fast_cols_sqdiff_built(M_BUILT) || fast_cols_rect_built(M_NOT_BUILT) || fast_cols_norm_built(M_NOT_BUILT) ||
        fast_cols_sqdiff_built(M_NOT_BUILT)) {
        printf("FAIL the three lengths are not what this walk names them\n");
        return 1;
    }
    long compared = 0, differ = 0, seen_route[5] = {0, 0, 0, 0, 0}, seen_cols[6] = {0, 0, 0, 0, 0, 0}, seen_line[5] = {0, 0, 0, 0, 0}, seen_error[3] = {0, 0, 0};
    for (int sink = 0; sink < 4; sink++)
    for (int host_stream = 0; host_stream < 2; host_stream++)
    for (int size = 0; size < 4; size++)      // map bytes at, and one element past, host_min_kb and FC_PIN_OUT_BYTES / 2
    for (int pinned = 0; pinned < 2; pinned++)
    for (long region = 0; region <= 5; region++)
    for (int rect_store = 0; rect_store < 2; rect_store++)
    for (int score = 0; score <= 4; score++)
    for (int norm_store = 0; norm_store < 2; norm_store++)
    for (int blockwise = 0; blockwise < 2; blockwise++)
    for (int format = FC_MAP_F32; format <= FC_MAP_BF16; format++)
    for (int kernel = 0; kernel < 4; kernel++) {
        Plan p;
        set_sink(p, sink);
        set_kernel(p, kernel);
        p.opt_host_stream = host_stream; p.opt_host_min_kb = HOST_MIN_KB; p.opt_host_pinned = pinned;
        p.opt_region = region; p.opt_rect_store = rect_store; p.opt_score = score; p.opt_norm_store = norm_store; p.opt_map_format = format;
        p.tiled = blockwise != 0;
        p.out_elems = (size < 2 ? (size_t)HOST_MIN_KB << 10 : FC_PIN_OUT_BYTES / 2) / p.elem_bytes() + (size & 1);
        const Parent want = parent_route(p);
        const OutputRoute got = plan_output_route(route_in(p));
        compared++;
        seen_route[want.route]++;
        seen_cols[want.cols_branch]++;
        seen_error[want.error]++;
        if (want.cropped) seen_line[want.region_line]++;
        if (!same(want, p, got) && differ++ < 20)
            printf("FAIL sink %d host_stream %d size %d host_pinned %d region %ld rect_store %d score %d norm_store %d block-wise %d format %d kernel %d: "
                   "parent error %d route %d cropped %d rect %d norm %d fused %d stage %d x%d kernel_format %d cols %d line %d pad %d whole %d tuner %d%d%d%d out %d; "
                   "route error %s route %d plane %d store %d kernel_format %d target %d extent %d after %d need_O %d staging %d x%d probe %d\n",
                   sink, host_stream, size, pinned, region, rect_store, score, norm_store, blockwise, format, kernel, want.error, want.route, (int)want.cropped,
                   (int)want.rect, (int)want.norm, (int)want.norm_fused, want.stage, want.stage_copies, want.kernel_format, want.cols_branch, want.region_line,
                   (int)want.region_pad, (int)want.region_whole, (int)want.tuner_skipped, (int)want.tuner_k0, (int)want.tuner_rect, (int)want.tuner_direct, want.tuner_out,
                   got.error ? got.error : "-", (int)got.route, (int)got.plane, (int)got.store, got.kernel_format, (int)got.target, (int)got.extent, (int)got.after,
                   (int)got.need_O, (int)got.staging, got.staging_copies, (int)got.probe);
    }
    for (int i = 0; i < 5; i++)
        if (!seen_route[i]) { printf("FAIL no combination leaves by route %d: the walk misses a route\n", i); differ++; }
    for (int i = 0; i < 6; i++)
        if (!seen_cols[i]) { printf("FAIL no combination takes branch %d of the output launch: the walk misses a store\n", i); differ++; }
    for (int i = 0; i < 5; i++)
        if (!seen_line[i]) { printf("FAIL no combination takes line %d of the crop: the walk misses a crop\n", i); differ++; }
    for (int i = 0; i < 3; i++)
        if (!seen_error[i]) { printf("FAIL no combination takes error case %d\n", i); differ++; }
    printf("table: %ld combinations compared, %ld differ\n", compared, differ);
    return differ ? 1 : 0;
}

// ---- the documented routes ----
// a specialised one-pass plan on the tiled intermediate with every family built and everything on its default, 288 x 288 windows
Plan plan_of(int sink, long region = 0, int score = 0, int format = FC_MAP_F32, size_t out_elems = 288 * 288) {
    Plan p;
    set_sink(p, sink);
    set_kernel(p, 2);
    p.opt_host_stream = 1; p.opt_host_min_kb = HOST_MIN_KB; p.opt_host_pinned = 1;
    p.opt_region = region; p.opt_rect_store = 1; p.opt_score = score; p.opt_norm_store = 1; p.opt_map_format = format;
    p.out_elems = out_elems;
    return p;
}
enum { WINDOW = 0, PACKED = 1, DEVICE = 2, HOST = 3 };

void expect(const char* what, const Plan& p, Route route, OutStore store, OutPlane plane, int kernel_format, OutBuffer target, OutExtent extent, OutAfter after,
            bool need_O, OutBuffer staging, int staging_copies, TuneProbe probe, const char* error = nullptr) {
    const OutputRoute r = plan_output_route(route_in(p));
    const bool ok = r.route == route && r.store == store && r.plane == plane && r.kernel_format == kernel_format && r.map_format == (int)p.opt_map_format &&
                    r.target == target && r.extent == extent && r.after == after && r.need_O == need_O && r.staging == staging && r.staging_copies == staging_copies &&
                    r.probe == probe && (error ? r.error && !strcmp(r.error, error) : !r.error);
    printf("%s %s: route %d store %d plane %d kernel_format %d target %d extent %d after %d need_O %d staging %d x%d probe %d error %s\n", ok ? "ok  " : "FAIL", what,
           (int)r.route, (int)r.store, (int)r.plane, r.kernel_format, (int)r.target, (int)r.extent, (int)r.after, (int)r.need_O, (int)r.staging, r.staging_copies,
           (int)r.probe, r.error ? r.error : "-");
    g_failures += !ok;
}

int cmd_named() {
    using R = Route; using S = OutStore; using P = OutPlane; using B = OutBuffer; using E = OutExtent; using A = OutAfter; using T = TuneProbe;
    const int F32 = FC_MAP_F32, F16 = FC_MAP_F16, BF16 = FC_MAP_BF16;
    expect("region 0, packed, fp32: the kernel writes the caller's maps", plan_of(PACKED), R::Packed, S::Plain, P::None, F32, B::Caller, E::Window, A::None, false, B::Caller,
           0, T::Plain);
    expect("region 2, device pointers: the fp32 window in O, cropped into OC, copied", plan_of(DEVICE, 2), R::Copies, S::Plain, P::None, F32, B::O, E::Region, A::Crop, true,
           B::OC, 1, T::Plain);
    expect("region 2, bf16 maps, packed: the kernel still stores fp32 for the crop", plan_of(PACKED, 2, 0, BF16), R::Packed, S::Plain, P::None, F32, B::O, E::Region, A::Crop,
           true, B::Caller, 0, T::Plain);
    expect("region 4, packed: padded from O", plan_of(PACKED, 4), R::Packed, S::Plain, P::None, F32, B::O, E::Region, A::Pad, true, B::Caller, 0, T::Plain);
    expect("rectangle, packed, fp32: stored by the kernel, no O", plan_of(PACKED, 5), R::Packed, S::Rect, P::None, F32, B::Caller, E::Rect, A::None, false, B::Caller, 0, T::Rect);
    expect("rectangle, device pointers, bf16: stored by the kernel into OC", plan_of(DEVICE, 5, 0, BF16), R::Copies, S::Rect, P::None, BF16, B::OC, E::Rect, A::None, false, B::OC,
           1, T::Rect);
    {
        Plan p = plan_of(PACKED, 5);
        set_kernel(p, 3);
        expect("rectangle at M = 544 (kernel not built): cropped from O", p, R::Packed, S::Plain, P::None, F32, B::O, E::Rect, A::Crop, true, B::Caller, 0, T::Plain);
        p.opt_rect_store = 0; set_kernel(p, 2);
        expect("rectangle with rect_store off: cropped from O", p, R::Packed, S::Plain, P::None, F32, B::O, E::Rect, A::Crop, true, B::Caller, 0, T::Plain);
    }
    expect("score 1 on region 0, host maps: fused, the whole window as the rectangle, staged in OC", plan_of(HOST, 0, 1), R::Pinned, S::RectScale, P::D, F32, B::OC, E::Window,
           A::None, false, B::OC, 1, T::Skip);
    expect("score 1, fp16 maps: staged -- the window in O, scaled while it is cropped", plan_of(PACKED, 0, 1, F16), R::Packed, S::Plain, P::D, F32, B::O, E::Window, A::Crop, true,
           B::Caller, 0, T::Skip);
    expect("score 3 on a rectangle, packed: fused", plan_of(PACKED, 5, 3), R::Packed, S::RectScale, P::Dc, F32, B::Caller, E::Rect, A::None, false, B::Caller, 0, T::Skip);
    expect("score 4, packed: fused", plan_of(PACKED, 0, 4), R::Packed, S::RectAdd, P::Q, F32, B::Caller, E::Window, A::None, false, B::Caller, 0, T::Skip);
    expect("score 4 on region 2: staged", plan_of(PACKED, 2, 4), R::Packed, S::Plain, P::Q, F32, B::O, E::Region, A::Crop, true, B::Caller, 0, T::Skip);
    {
        Plan p = plan_of(PACKED, 0, 4);
        p.opt_norm_store = 0;
        expect("score 4 with norm_store off: staged", p, R::Packed, S::Plain, P::Q, F32, B::O, E::Window, A::Crop, true, B::Caller, 0, T::Skip);
    }
    expect("score 2, packed: leaves as score 0 does", plan_of(PACKED, 0, 2), R::Packed, S::Plain, P::None, F32, B::Caller, E::Window, A::None, false, B::Caller, 0, T::Plain);
    expect("score 2 on a rectangle: the rectangle store, as score 0", plan_of(PACKED, 5, 2), R::Packed, S::Rect, P::None, F32, B::Caller, E::Rect, A::None, false, B::Caller, 0,
           T::Rect);
    expect("an overlap-save window: the plain kernel into the caller's maps, never probed", plan_of(WINDOW), R::Window, S::Plain, P::None, F32, B::Caller, E::Window, A::None, false,
           B::Caller, 0, T::None);
    {
        Plan p = plan_of(PACKED);
        set_kernel(p, 0);
        expect("a generic plan, packed", p, R::Packed, S::Generic, P::None, F32, B::Caller, E::Window, A::None, false, B::Caller, 0, T::Plain);
        p.opt_region = 5; p.opt_score = 1;
        expect("a generic plan, score 1 on a rectangle: staged", p, R::Packed, S::Generic, P::D, F32, B::O, E::Rect, A::Crop, true, B::Caller, 0, T::Skip);
    }
    const size_t at = ((size_t)HOST_MIN_KB << 10) / 4;
    expect("host maps of exactly host_min_kb: the ring, two staging buffers in O", plan_of(HOST, 0, 0, F32, at), R::Ring, S::Plain, P::None, F32, B::O, E::Window, A::None, false,
           B::O, 2, T::Plain);
    expect("host maps one element below host_min_kb: pinned, one staging buffer", plan_of(HOST, 0, 0, F32, at - 1), R::Pinned, S::Plain, P::None, F32, B::O, E::Window, A::None,
           false, B::O, 1, T::Plain);
    {
        Plan p = plan_of(HOST, 0, 0, F32, FC_PIN_OUT_BYTES / 2 / 4 + 1);
        p.opt_host_stream = 0;
        expect("host maps one element past half the pinned buffer, host_stream off: plain copies", p, R::Copies, S::Plain, P::None, F32, B::O, E::Window, A::None, false, B::O, 1,
               T::Plain);
        const OutputRoute small = plan_output_route(route_in(plan_of(HOST, 0, 0, F32, FC_PIN_ONE_MAP_BYTES / 4))),
                          large = plan_output_route(route_in(plan_of(HOST, 0, 0, F32, FC_PIN_ONE_MAP_BYTES / 4 + 1)));
        const bool ok = small.route == Route::Pinned && small.pinned_one_map && large.route == Route::Pinned && !large.pinned_one_map;
        printf("%s a single map on the pinned route: through the pinned buffer up to FC_PIN_ONE_MAP_BYTES, plain copies above\n", ok ? "ok  " : "FAIL");
        g_failures += !ok;
    }
    {
        Plan p = plan_of(WINDOW);
        set_kernel(p, 0);
        expect("error: a window on a generic plan", p, R::Window, S::Generic, P::None, F32, B::Caller, E::Window, A::None, false, B::Caller, 0, T::None,
               "an output window needs the specialised output kernel");
        expect("error: a window with a score", plan_of(WINDOW, 0, 2), R::Window, S::Plain, P::None, F32, B::Caller, E::Window, A::None, false, B::Caller, 0, T::None,
               "an output window takes no normalisation");
    }
    printf("named: %d failed\n", g_failures);
    return g_failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    if (!strcmp(mode, "table")) return cmd_table();
    if (!strcmp(mode, "named")) return cmd_named();
    fprintf(stderr, "usage: output_route_host table|named\n");
    return 2;
}
