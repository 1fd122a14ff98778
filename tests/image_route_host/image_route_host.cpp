// image_route_host.cpp -- TEST-ONLY stand-alone host program for csrc/image_route.hpp (plan_image_route: the way of an image into a
// one-pass plan, decided once per call).
//
// Built by tests/test_image_route_host.py with the host compiler from the product's headers alone.  Modes:
//   table    plan_image_route against a literal transcription of the conditions of set_images_impl as it stood before the route
//            existed (one function of fftconv_api.cpp; its line numbers are in the comments), over the full product of the axes
//            listed in cmd_table -- the number of combinations is printed, and the test holds it against the product
//   named    the routes the library documents, one line each, against expectations written by hand
// Having its own main, it is also the place for a host sanitizer build (-fsanitize=address,undefined) of this code.
#include <cstdio>
#include <cstring>

#include "fast_paths.hpp"
#include "image_route.hpp"

using namespace fc;

namespace {

int g_failures = 0;

// ---- the transcription: fftconv_api.cpp, set_images_impl, lines 760-919 of the commit before plan_image.cpp ----
struct Parent {
    int source = 0;              // 0 the caller's device pointer, 1 pin_img in place, 2 a copy from pin_img, 3 a copy from pageable memory
    int dev = 0;                 // the copy's buffer: 0 none, 1 I, 2 IT
    bool convert = false, extend = false;
    int launch = 0;              // 0 generic, 1 specialised, 2 specialised typed, 3 specialised bordered, 4 image + deferred kernels
    bool flush = false;
    size_t I = 0, IT = 0, IE = 0;
    int sfmt = 0;
    bool image_pinned = false, sync = false;
};
size_t floats_for(size_t elems, size_t elem_bytes) { return (elems * elem_bytes + sizeof(float) - 1) / sizeof(float); }      // plan_internal.hpp:419

Parent parent_route(const ImageRouteIn& in) {
    Parent r;
    const int fmt = in.format;
    const bool pending = in.request != KernelRequest::None, pending_off_stream = in.request == KernelRequest::OtherStream;
    const bool typed = fmt != FC_PIXEL_F32;                                            // :760
    const size_t eb = fc_pixel_elem_bytes(fmt);                                        // :761
    const int planes = in.n_images * in.F;                                             // :787
    const bool direct = typed && in.pixel_direct;                                      // :788
    const bool border = in.border_mode, bdirect = border && in.border_direct;          // :793
    const int eh = in.H + in.max_kh - 1, ew = in.W + in.max_kw - 1;                    // :794
    const size_t n = (size_t)in.H * in.W * planes;                                     // :797
    if (in.host) {                                                                     // :798
        const int dev = typed ? 2 : 1;                                                 // :801
        if (in.host_pinned && n * eb <= ((size_t)1 << 20)) {                           // :802 (FC_PIN_IMAGE_BYTES, plan_internal.hpp:159)
            r.image_pinned = true;                                                     // :806
            if (n * eb <= ((size_t)512 << 10) && (!typed || direct)) r.source = 1;     // :807 (FC_PIN_INPLACE_BYTES, plan_internal.hpp:158)
            else { r.source = 2; r.dev = dev; }                                        // :810-812
        } else { r.source = 3; r.dev = dev; }                                          // :815-817
        if (r.dev == 1) r.I = floats_for(n, eb);
        if (r.dev == 2) r.IT = floats_for(n, eb);
    }
    if (typed && !direct) r.I = n;                                                     // :820
    if (border && !bdirect) r.IE = (size_t)eh * ew * planes;                           // :822
    r.flush = (direct || border) ? pending : pending_off_stream;                       // :847
    bool still_pending = pending && !r.flush;
    r.sfmt = fmt;                                                                      // :849
    if (typed && !direct) { r.convert = true; r.sfmt = FC_PIXEL_F32; }                 // :851-855
    if (border) {                                                                      // :858
        if (bdirect) r.launch = 3;                                                     // :860-863
        else { r.extend = true; r.launch = in.fast_fwd ? 1 : 0; }                      // :865-873
    } else if (direct) r.launch = 2;                                                   // :876-881
    else if (in.fast_fwd) r.launch = still_pending ? 4 : 1;                            // :882-894 (take_pending)
    else r.launch = 0;                                                                 // :895-897
    r.sync = in.host && !r.image_pinned;                                               // :919
    return r;
}

bool same(const Parent& a, const ImageRoute& b) {
    return a.source == (int)b.source && a.dev == (int)b.landing && a.convert == b.convert && a.extend == b.extend && a.launch == (int)b.columns &&
           a.flush == b.flush_first && a.I == b.i_elems && a.IT == b.it_elems && a.IE == b.ie_elems && a.sfmt == b.stats_format &&
           a.image_pinned == b.pinned && a.sync == b.sync_at_end;
}

// the plan's two predicates (plan_internal.hpp: pixel_direct, border_direct) of a one-pass plan with these settings
void set_predicates(ImageRouteIn& in, bool pixel_store, bool border_store, int M) {
    in.pixel_direct = !in.border_mode && fast_cols_fwd_px_direct(pixel_store, false, in.fast_fwd, M);
    in.border_direct = in.border_mode && fast_cols_fwd_border_direct(border_store, false, in.fast_fwd, M);
}

constexpr int M_BUILT = 144, M_NO_BORDER = 544;      // both have the specialised column kernels; 544 has no bordered instantiation

int cmd_table() {
    if (!fast_cols_lookup(M_BUILT).ok || !fast_cols_lookup(M_NO_BORDER).ok || !fast_cols_fwd_border_built(M_BUILT) || fast_cols_fwd_border_built(M_NO_BORDER) ||
        !fast_cols_fwd_px_built(M_BUILT)) {
        printf("FAIL the two configurations are not what this walk names them\n");
        return 1;
    }
    // (border, normalise): never both, as fftconv_plan_set_border / fftconv_plan_set_normalisation refuse it
    const bool modes[3][2] = {{false, false}, {false, true}, {true, false}};
    const KernelRequest requests[3] = {KernelRequest::None, KernelRequest::ThisStream, KernelRequest::OtherStream};
    long compared = 0, differ = 0, seen_launch[5] = {0, 0, 0, 0, 0}, seen_source[4] = {0, 0, 0, 0};
    for (int fmt = 0; fmt <= 4; fmt++)
    for (int host = 0; host < 2; host++)
    for (int pinned = 0; pinned < 2; pinned++)
    for (int size = 0; size < 4; size++)      // bytes at, and one element past, FC_PIN_INPLACE_BYTES and FC_PIN_IMAGE_BYTES
    for (int pixel_store = 0; pixel_store < 2; pixel_store++)
    for (int border_store = 0; border_store < 2; border_store++)
    for (int fast_fwd = 0; fast_fwd < 2; fast_fwd++)
    for (int built = 0; built < 2; built++)
    for (int mode = 0; mode < 3; mode++)
    for (int rq = 0; rq < 3; rq++) {
        ImageRouteIn in;
        in.format = fmt; in.host = host != 0; in.host_pinned = pinned != 0;
        const size_t at = (size < 2 ? FC_PIN_INPLACE_BYTES : FC_PIN_IMAGE_BYTES) / fc_pixel_elem_bytes(fmt);
        if (size & 1) { in.H = (int)at + 1; in.W = 1; in.F = 1; in.n_images = 1; }      // one element past the limit
        else { in.H = (int)(at / 16); in.W = 4; in.F = 2; in.n_images = 2; }            // at it: a batch of two images of two planes
        in.max_kh = 7; in.max_kw = 5;
        in.fast_fwd = fast_fwd != 0; in.border_mode = modes[mode][0]; in.normalise = modes[mode][1];
        set_predicates(in, pixel_store != 0, border_store != 0, built ? M_BUILT : M_NO_BORDER);
        in.request = requests[rq];
        const Parent want = parent_route(in);
        const ImageRoute got = plan_image_route(in);
        compared++;
        seen_launch[want.launch]++;
        seen_source[want.source]++;
        if (!same(want, got)) {
            if (differ++ < 20)
                printf("FAIL format %d host %d host_pinned %d size %d pixel_store %d border_store %d fast_fwd %d built %d border %d normalise %d request %d: "
                       "source %d/%d landing %d/%d convert %d/%d extend %d/%d launch %d/%d flush %d/%d I %zu/%zu IT %zu/%zu IE %zu/%zu stats %d/%d pinned %d/%d sync %d/%d\n",
                       fmt, host, pinned, size, pixel_store, border_store, fast_fwd, built, (int)in.border_mode, (int)in.normalise, rq, want.source,
                       (int)got.source, want.dev, (int)got.landing, (int)want.convert, (int)got.convert, (int)want.extend, (int)got.extend, want.launch,
                       (int)got.columns, (int)want.flush, (int)got.flush_first, want.I, got.i_elems, want.IT, got.it_elems, want.IE, got.ie_elems, want.sfmt,
                       got.stats_format, (int)want.image_pinned, (int)got.pinned, (int)want.sync, (int)got.sync_at_end);
        }
    }
    for (int l = 0; l < 5; l++)
        if (!seen_launch[l]) { printf("FAIL no combination takes column launch %d: the walk misses a route\n", l); differ++; }
    for (int s = 0; s < 4; s++)
        if (!seen_source[s]) { printf("FAIL no combination takes source %d: the walk misses a route\n", s); differ++; }
    printf("table: %ld combinations compared, %ld differ\n", compared, differ);
    return differ ? 1 : 0;
}

// ---- the documented routes ----
ImageRouteIn plan_of(int fmt, bool host, int H, int W) {      // a specialised one-pass plan, everything on its default
    ImageRouteIn in;
    in.format = fmt; in.host = host; in.H = H; in.W = W; in.F = 1; in.n_images = 1; in.max_kh = 9; in.max_kw = 9;
    in.host_pinned = true; in.fast_fwd = true;
    set_predicates(in, true, true, M_BUILT);
    return in;
}
ImageRouteIn with_border(ImageRouteIn in, bool border_store, int M = M_BUILT) {
    in.border_mode = true;
    set_predicates(in, true, border_store, M);
    return in;
}

void expect(const char* what, const ImageRouteIn& in, ImageSource source, ImageLanding landing, bool convert, bool extend, ImageColumns columns, bool flush_first,
            size_t i_elems, size_t it_elems, size_t ie_elems, int stats_format, bool pinned, bool sync_at_end) {
    const ImageRoute r = plan_image_route(in);
    const bool ok = r.source == source && r.landing == landing && r.convert == convert && r.extend == extend && r.columns == columns &&
                    r.flush_first == flush_first && r.i_elems == i_elems && r.it_elems == it_elems && r.ie_elems == ie_elems &&
                    r.stats_format == stats_format && r.pinned == pinned && r.sync_at_end == sync_at_end;
    printf("%s %s: source %d landing %d convert %d extend %d columns %d flush %d I %zu IT %zu IE %zu stats %d pinned %d sync %d\n", ok ? "ok  " : "FAIL", what,
           (int)r.source, (int)r.landing, (int)r.convert, (int)r.extend, (int)r.columns, (int)r.flush_first, r.i_elems, r.it_elems, r.ie_elems, r.stats_format,
           (int)r.pinned, (int)r.sync_at_end);
    g_failures += !ok;
}

int cmd_named() {
    using S = ImageSource; using L = ImageLanding; using C = ImageColumns;
    const int F32 = FC_PIXEL_F32, U8 = FC_PIXEL_U8;
    const size_t n = 64 * 64, ext = (size_t)72 * 72;      // a 64 x 64 image; extended by a 9 x 9 MAX_KERNEL
    expect("fp32 device, plain", plan_of(F32, false, 64, 64), S::Device, L::None, false, false, C::Fast, false, 0, 0, 0, F32, false, false);
    expect("fp32 host, small: pinned, read in place", plan_of(F32, true, 64, 64), S::PinnedInPlace, L::None, false, false, C::Fast, false, 0, 0, 0, F32, true, false);
    expect("fp32 host, 768 KiB: pinned, then copied into I", plan_of(F32, true, 512, 384), S::PinnedCopy, L::I, false, false, C::Fast, false, 512 * 384, 0, 0, F32, true, false);
    expect("fp32 host, 4 MiB: copied into I, sync at the end", plan_of(F32, true, 1024, 1024), S::PageableCopy, L::I, false, false, C::Fast, false, 1024 * 1024, 0, 0, F32,
           false, true);
    {
        ImageRouteIn in = plan_of(F32, true, 64, 64);
        in.host_pinned = false;
        expect("fp32 host, small, host_pinned off: copied into I, sync", in, S::PageableCopy, L::I, false, false, C::Fast, false, n, 0, 0, F32, false, true);
    }
    expect("uint8 host, direct: pinned, read in place", plan_of(U8, true, 64, 64), S::PinnedInPlace, L::None, false, false, C::FastTyped, false, 0, 0, 0, U8, true, false);
    {
        ImageRouteIn in = plan_of(U8, true, 64, 64);
        set_predicates(in, false, true, M_BUILT);      // "pixel_store" 0
        expect("uint8 host, staged: IT, then I", in, S::PinnedCopy, L::IT, true, false, C::Fast, false, n, n / 4, 0, F32, true, false);
    }
    expect("uint8 host with a border, border direct: converted, then bordered from I", with_border(plan_of(U8, true, 64, 64), true), S::PinnedCopy, L::IT, true, false,
           C::FastBorder, false, n, n / 4, 0, F32, true, false);
    expect("uint8 host with a border, border staged: converted, then extended into IE", with_border(plan_of(U8, true, 64, 64), false), S::PinnedCopy, L::IT, true, true,
           C::Fast, false, n, n / 4, ext, F32, true, false);
    expect("fp32 device with a border, no bordered kernel for the length: staged", with_border(plan_of(F32, false, 64, 64), true, M_NO_BORDER), S::Device, L::None, false,
           true, C::Fast, false, 0, 0, ext, F32, false, false);
    {
        ImageRouteIn in = plan_of(F32, false, 64, 64);
        in.fast_fwd = false;
        expect("fp32 device with a border on a generic plan: staged", with_border(in, true), S::Device, L::None, false, true, C::Generic, false, 0, 0, ext, F32, false,
               false);
        expect("uint8 device on a generic plan: staged", [&] { ImageRouteIn t = in; t.format = U8; set_predicates(t, true, true, M_BUILT); return t; }(), S::Device, L::None,
               true, false, C::Generic, false, n, 0, 0, F32, false, false);
    }
    {
        ImageRouteIn in = plan_of(F32, false, 64, 64);
        in.request = KernelRequest::ThisStream;
        expect("request pending on this stream: the pair", in, S::Device, L::None, false, false, C::Pair, false, 0, 0, 0, F32, false, false);
        in.request = KernelRequest::OtherStream;
        expect("request pending on another stream: flushed, then plain", in, S::Device, L::None, false, false, C::Fast, true, 0, 0, 0, F32, false, false);
        in.request = KernelRequest::ThisStream;
        in.format = U8;
        expect("request pending, typed direct: flushed by itself", in, S::Device, L::None, false, false, C::FastTyped, true, 0, 0, 0, U8, false, false);
        in.format = F32;
        expect("request pending, border direct: flushed by itself", with_border(in, true), S::Device, L::None, false, false, C::FastBorder, true, 0, 0, 0, F32, false,
               false);
        expect("request pending, border staged: flushed by itself", with_border(in, false), S::Device, L::None, false, true, C::Fast, true, 0, 0, ext, F32, false, false);
        in.format = U8;
        set_predicates(in, false, true, M_BUILT);
        expect("request pending on this stream, typed staged: converted, then the pair", in, S::Device, L::None, true, false, C::Pair, false, n, 0, 0, F32, false, false);
    }
    {
        ImageRouteIn in = plan_of(U8, false, 64, 64);
        in.normalise = true;
        expect("normalised, typed direct: the statistics read the typed pixels", in, S::Device, L::None, false, false, C::FastTyped, false, 0, 0, 0, U8, false, false);
        set_predicates(in, false, true, M_BUILT);
        expect("normalised, typed staged: the statistics read the fp32 image", in, S::Device, L::None, true, false, C::Fast, false, n, 0, 0, F32, false, false);
    }
    printf("named: %d failed\n", g_failures);
    return g_failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    if (!strcmp(mode, "table")) return cmd_table();
    if (!strcmp(mode, "named")) return cmd_named();
    fprintf(stderr, "usage: image_route_host table|named\n");
    return 2;
}
