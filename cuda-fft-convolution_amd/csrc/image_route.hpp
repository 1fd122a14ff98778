// image_route.hpp -- the way of an image into a one-pass plan (fftconv_plan_set_image / set_images / set_images_typed), decided ONCE
// per call: plan_image_route answers every question the call has, and the stages of plan_image.cpp (and the verbose lines that name
// them) only read the answers.  Host-only and HIP-free like column_cache.hpp: tests/image_route_host walks the whole table with
// the plain host compiler.
//
//   source    device image: read where it lies.  Host image: through the plan's pinned buffer while "host_pinned" is on and the
//             batch is at most FC_PIN_IMAGE_BYTES -- read there IN PLACE by the column pass up to FC_PIN_INPLACE_BYTES (fp32
//             pixels, and typed ones on the direct route), else copied on into the landing buffer; larger batches are copied from
//             the caller's pageable memory and the call ends with a sync.  The limits count the bytes that cross: typed ones.
//   landing   where a copy lands: I for fp32 pixels, IT for typed ones (a staged conversion reads them there).
//   convert   typed pixels that the column kernel does not convert in its load (fftconv_plan::pixel_direct; never direct while a
//             border is on) become fp32 in I first, and the call goes on as an fp32 one.
//   extend    a border that the column kernel does not map in its load (fftconv_plan::border_direct) is materialised in IE first.
//   columns   the one column launch: generic, specialised, specialised typed (direct pixels), specialised bordered (direct
//             border), or the pair -- a specialised fp32 launch without a border that carries the deferred column pass of
//             fftconv_plan_prepare_kernels_packed, recorded on this stream, in the same launch.
//   flush     a recorded preparation the launch cannot carry runs by itself first: always ahead of a typed-direct or bordered
//             launch, and ahead of any launch when it was recorded on another stream.
//   after     the window statistics of normalised maps read what the column pass read (stats_format); a pinned buffer is marked
//             behind its last reader and the call returns without a sync; a pageable copy ends with one.
#pragma once
#include <cstddef>

#include "pixel_format.hpp"

namespace fc {

// Pinned host staging of small host images (plan_internal.hpp: PinBuf)
constexpr size_t FC_PIN_INPLACE_BYTES = (size_t)512 << 10;
constexpr size_t FC_PIN_IMAGE_BYTES = (size_t)1 << 20;

enum class KernelRequest { None, ThisStream, OtherStream };      // ColumnCache: no recorded preparation, or one, and on which stream
enum class ImageSource { Device, PinnedInPlace, PinnedCopy, PageableCopy };
enum class ImageLanding { None, I, IT };
enum class ImageColumns { Generic, Fast, FastTyped, FastBorder, Pair };

struct ImageRouteIn {
    int format = FC_PIXEL_F32;      // FC_PIXEL_* of the caller's elements
    int n_images = 1;
    bool host = false;              // location == FFTCONV_HOST
    int H = 0, W = 0, F = 0, max_kh = 0, max_kw = 0;
    bool host_pinned = false;       // plan option "host_pinned"
    bool pixel_direct = false, border_direct = false;      // as the plan reports them: the only definitions of "direct"
    bool border_mode = false, fast_fwd = false;
    bool normalise = false;         // (no answer depends on it: the statistics read stats_format whenever they run)
    KernelRequest request = KernelRequest::None;
};

struct ImageRoute {
    ImageSource source = ImageSource::Device;
    ImageLanding landing = ImageLanding::None;
    bool convert = false, extend = false;
    ImageColumns columns = ImageColumns::Generic;
    bool flush_first = false;
    size_t i_elems = 0, it_elems = 0, ie_elems = 0;      // floats I / IT / IE must hold; 0: the call does not touch the buffer
    int stats_format = FC_PIXEL_F32;
    bool pinned = false, sync_at_end = false;
};

inline ImageRoute plan_image_route(const ImageRouteIn& in) {
    ImageRoute r;
    const bool typed = in.format != FC_PIXEL_F32, direct = typed && in.pixel_direct;
    const bool border = in.border_mode, bdirect = border && in.border_direct;
    const size_t eb = fc_pixel_elem_bytes(in.format), n = (size_t)in.H * in.W * in.F * in.n_images;
    if (in.host) {
        r.pinned = in.host_pinned && n * eb <= FC_PIN_IMAGE_BYTES;
        if (r.pinned && n * eb <= FC_PIN_INPLACE_BYTES && (!typed || direct)) r.source = ImageSource::PinnedInPlace;
        else {
            r.source = r.pinned ? ImageSource::PinnedCopy : ImageSource::PageableCopy;
            r.landing = typed ? ImageLanding::IT : ImageLanding::I;
        }
        r.sync_at_end = !r.pinned;
    }
    r.convert = typed && !direct;
    r.extend = border && !bdirect;
    if (r.landing == ImageLanding::I || r.convert) r.i_elems = n;
    if (r.landing == ImageLanding::IT) r.it_elems = (n * eb + sizeof(float) - 1) / sizeof(float);
    if (r.extend) r.ie_elems = (size_t)(in.H + in.max_kh - 1) * (in.W + in.max_kw - 1) * in.F * in.n_images;
    r.stats_format = r.convert ? FC_PIXEL_F32 : in.format;
    r.flush_first = (direct || border) ? in.request != KernelRequest::None : in.request == KernelRequest::OtherStream;
    if (border) r.columns = bdirect ? ImageColumns::FastBorder : in.fast_fwd ? ImageColumns::Fast : ImageColumns::Generic;
    else if (direct) r.columns = ImageColumns::FastTyped;
    else if (!in.fast_fwd) r.columns = ImageColumns::Generic;
    else r.columns = in.request == KernelRequest::ThisStream ? ImageColumns::Pair : ImageColumns::Fast;
    return r;
}

}  // namespace fc
