// output_route.hpp -- the way of a group's maps out of a plan (run_group; fftconv_plan_convolve[_packed], the blocks of an overlap-save
// plan), decided ONCE per group: plan_output_route answers every question the group has, and the stages of plan_output.cpp, the
// placement tuner and the verbose lines that name them only read the answers.  Host-only and HIP-free like image_route.hpp:
// tests/output_route_host walks the whole table with the plain host compiler.
//
//   route     how the maps leave.  An output window (the block plan of an overlap-save plan): Window.  The caller's packed device
//             buffer: Packed.  Device pointers: Copies (staged, one copy per map).  Host pointers: Ring while "host_stream" is on and
//             a map has at least "host_min_kb"; else Pinned while "host_pinned" is on and a map is at most FC_PIN_OUT_BYTES / 2 (a
//             single map above FC_PIN_ONE_MAP_BYTES takes plain copies all the same: pinned_one_map); else Copies.
//   plane     a score with a plane (1: D, 3: Dc, 4: Q with the kernels' constants) combines every map with it, whatever the sink --
//             in the output kernel's store (store RectScale / RectAdd) or while the staged window is cropped (after).
//   store     what the output kernel stores, one of: Generic (no specialised kernel); Plain (the window, or the OutWindow of a block);
//             Rect -- region 5 with "rect_store" on a one-pass plan whose rectangle kernel is built, no plane; RectScale (D, Dc) /
//             RectAdd (Q + c) -- a plane with "norm_store", fp32 maps, region 0 or 5, a one-pass plan whose NORM / ADD kernel is
//             built: the rectangle is the plan's (extent Rect) or the whole window standing in for one (extent Window).
//             RectStride -- strided maps (fftconv_plan_set_output_stride: a stride other than (1, 1)) with "stride_store" on, fp32
//             maps, no plane, region 0 or 5, a one-pass plan on the tiled intermediate whose STRIDE kernel is built: the kernel stores
//             the sampled rows and columns of the extent densely.  Every other strided group is sampled by the crop (after).
//   after     what follows the kernel: a region other than the window that the kernel did not store itself, and every plane it did not
//             combine itself (region 0 included: the crop of the whole window), go through the fp32 window in O and are cropped --
//             region 4: padded -- into the maps, times or plus the plane on the way.  A stride the kernel did not sample itself is
//             the crop's too, region 0 included (region 4 takes no stride: fftconv_plan_set_output_stride refuses it).
//   format    kernel_format: what the output kernel stores -- fp32 whenever a crop follows, else "map_format"; map_format: the maps'.
//   target    where the kernel writes: O when a crop follows, else the staging buffer of a staged route, else the caller's memory.
//   buffers   O for the crop (need_O), and the staging of Copies / Pinned / Ring (staging, twice for the ring: staging_copies): OC
//             for everything the kernel or the crop stores densely -- region maps, rectangles, every fused plane, region 0 included --
//             else O.
//   tuning    a score with a plane is never tuned and leaves the intermediate marked fresh (Skip); a window is never probed (None);
//             else the probes are the group's own launch, Rect (the strided launch of RectStride included) or Plain, into `target` -- every batch's destination when that is the
//             caller's memory, else the one staging buffer.
//   extrema   per-map extrema (fftconv_plan_set_extrema) while they are on: Fused -- found by the output kernel in its store (fast_cols.hpp:
//             EXT) -- where "extrema_store" is on and the group's store is one of the three fp32 rectangle stores whose EXT kernel is built:
//             Rect, RectScale, RectAdd as decided above, or the Plain store of the whole fp32 window of a one-pass plan on the tiled
//             intermediate, which then becomes Rect with the window standing in for the rectangle (as it does for RectScale / RectAdd).
//             Scan -- everything else (16-bit maps, named regions, strides, every crop / pad, generic and Bluestein output kernels, the
//             row-major intermediate, configurations that are not built, "extrema_store" 0): the scan kernel reads the delivered maps
//             where they lie on the device -- the caller's packed buffer or the staging -- before any copy-out.  The probes stay those of
//             the store without extrema (the Plain launch writes the same whole windows).
//   error     an output window on a plan without the specialised output kernel, or with any score on: refused.
#pragma once
#include <cstddef>

#include "fc_common.hpp"

namespace fc {

// Pinned host staging of small host maps (plan_internal.hpp: PinBuf)
constexpr size_t FC_PIN_OUT_BYTES = (size_t)8 << 20;
constexpr size_t FC_PIN_ONE_MAP_BYTES = (size_t)64 << 10;

enum class Route {
    Packed,   // the caller's packed device buffer: the output kernel (or the crop kernel) writes there
    Window,   // block plan of an overlap-save plan: the output kernel stores its window of the full maps (OutWindow)
    Copies,   // staged on the device, then one copy per map on the plan's stream (device pointers; host maps no other route takes)
    Pinned,   // small host maps: staged, a launch's maps come back in ONE copy into the plan's pinned buffer (deliver_pinned)
    Ring,     // host maps of at least host_min_kb: two staging buffers, the copy-out of batch b overlaps the compute of batch b + 1
};
enum class SinkKind { Window, Packed, DevicePtrs, Host };
enum class OutStore { Generic, Plain, Rect, RectScale, RectAdd, RectStride };
enum class OutPlane { None, D, Dc, Q };           // D, Dc: multiplied; Q: added with the constant of the map's kernel
enum class OutBuffer { Caller, O, OC };
enum class OutExtent { Window, Region, Rect };    // what a delivered map holds: "output_region" 0, 1-4, 5
enum class OutAfter { None, Crop, Pad };
enum class TuneProbe { Skip, None, Plain, Rect };
enum class OutExtrema { Off, Fused, Scan };

struct OutputRouteIn {
    SinkKind sink = SinkKind::Packed;
    size_t map_bytes = 0;                      // of one delivered map
    long host_stream = 0, host_min_kb = 0;     // plan options of the same names
    bool host_pinned = false;
    long region = 0;                           // "output_region" 0-5
    bool rect_store = false;
    long score = 0;                            // FC_SCORE_*
    bool norm_store = false;
    bool blockwise = false;
    int map_format = FC_MAP_F32;
    bool fast_cols = false, y_tiled = false;   // the plan has the specialised output kernel; its intermediate is tiled
    bool rect_built = false, norm_built = false, sqdiff_built = false;      // fast_paths.hpp: fast_cols_*_built of the plan's M
    // strided maps (fftconv_plan_set_output_stride); the defaults are "no stride"
    int stride_h = 1, stride_w = 1;
    bool stride_store = true, stride_built = false;
    bool strided() const { return stride_h != 1 || stride_w != 1; }
    // per-map extrema (fftconv_plan_set_extrema); the defaults are "off"
    bool extrema = false, extrema_store = true;
    bool extrema_rect_built = false, extrema_norm_built = false, extrema_sqdiff_built = false;      // fast_paths.hpp: fast_cols_*_ext_built of the plan's M
};

struct OutputRoute {
    const char* error = nullptr;               // the group is refused (FFTCONV_ERR_INVALID_ARG) with this message
    Route route = Route::Packed;
    OutPlane plane = OutPlane::None;
    OutStore store = OutStore::Generic;
    int kernel_format = FC_MAP_F32, map_format = FC_MAP_F32;
    OutBuffer target = OutBuffer::Caller;
    OutExtent extent = OutExtent::Window;
    OutAfter after = OutAfter::None;
    bool need_O = false;
    OutBuffer staging = OutBuffer::Caller;     // Caller: none
    int staging_copies = 0;
    bool pinned_one_map = false;               // Pinned: a launch of ONE map goes through the pinned buffer too
    TuneProbe probe = TuneProbe::Skip;
    OutExtrema extrema = OutExtrema::Off;
    bool staged() const { return route == Route::Copies || route == Route::Pinned || route == Route::Ring; }
    bool fused() const { return store == OutStore::RectScale || store == OutStore::RectAdd; }
};

inline OutputRoute plan_output_route(const OutputRouteIn& in) {
    OutputRoute r;
    const bool window = in.sink == SinkKind::Window;
    if (window && !in.fast_cols) r.error = "an output window needs the specialised output kernel";
    else if (window && in.score) r.error = "an output window takes no normalisation";
    r.plane = in.score == FC_SCORE_SQDIFF ? OutPlane::Q : in.score == FC_SCORE_CCORR_NORMED ? OutPlane::Dc
              : in.score == FC_SCORE_CCOEFF_NORMED ? OutPlane::D : OutPlane::None;
    r.extent = in.region == 0 ? OutExtent::Window : in.region == 5 ? OutExtent::Rect : OutExtent::Region;
    const bool one_pass_tiled = !window && !in.blockwise && in.fast_cols && in.y_tiled;      // (a tiled intermediate implies the kernel)
    if (r.plane != OutPlane::None) {
        const bool built = r.plane == OutPlane::Q ? in.sqdiff_built : in.norm_built;
        if (one_pass_tiled && in.norm_store && in.map_format == FC_MAP_F32 && r.extent != OutExtent::Region && built && !in.strided())      // (no fused plane + stride)
            r.store = r.plane == OutPlane::Q ? OutStore::RectAdd : OutStore::RectScale;
    } else if (in.strided()) {
        if (one_pass_tiled && in.stride_store && in.stride_built && in.map_format == FC_MAP_F32 && r.extent != OutExtent::Region) r.store = OutStore::RectStride;
    } else if (one_pass_tiled && r.extent == OutExtent::Rect && in.rect_store && in.rect_built) r.store = OutStore::Rect;
    if (r.store == OutStore::Generic && in.fast_cols) r.store = OutStore::Plain;
    const OutStore probe_store = r.store;
    if (in.extrema && !window) {
        r.extrema = OutExtrema::Scan;
        if (in.extrema_store && in.map_format == FC_MAP_F32) {
            if (r.fused()) {
                if (r.plane == OutPlane::Q ? in.extrema_sqdiff_built : in.extrema_norm_built) r.extrema = OutExtrema::Fused;
            } else if (r.store == OutStore::Rect) {
                if (in.extrema_rect_built) r.extrema = OutExtrema::Fused;
            } else if (r.store == OutStore::Plain && one_pass_tiled && r.plane == OutPlane::None && !in.strided() && r.extent == OutExtent::Window &&
                       in.rect_built && in.extrema_rect_built) {
                r.store = OutStore::Rect;
                r.extrema = OutExtrema::Fused;
            }
        }
    }
    const bool dense = r.store == OutStore::Rect || r.store == OutStore::RectStride || r.fused();      // the kernel stores the delivered maps itself
    if (!dense && (r.extent != OutExtent::Window || r.plane != OutPlane::None || in.strided())) r.after = in.region == 4 ? OutAfter::Pad : OutAfter::Crop;
    const bool cropped = r.after != OutAfter::None;
    r.map_format = in.map_format;
    r.kernel_format = cropped ? FC_MAP_F32 : in.map_format;
    if (window) r.route = Route::Window;
    else if (in.sink == SinkKind::Packed) r.route = Route::Packed;
    else if (in.sink != SinkKind::Host) r.route = Route::Copies;
    else if (in.host_stream != 0 && in.map_bytes >= ((size_t)in.host_min_kb << 10)) r.route = Route::Ring;
    else if (in.host_pinned && in.map_bytes <= FC_PIN_OUT_BYTES / 2) r.route = Route::Pinned;
    else r.route = Route::Copies;
    r.pinned_one_map = in.map_bytes <= FC_PIN_ONE_MAP_BYTES;
    r.need_O = cropped;
    if (r.staged()) {
        r.staging = (cropped || dense) ? OutBuffer::OC : OutBuffer::O;
        r.staging_copies = r.route == Route::Ring ? 2 : 1;
    }
    r.target = cropped ? OutBuffer::O : r.staging;
    r.probe = r.plane != OutPlane::None ? TuneProbe::Skip : window ? TuneProbe::None
              : probe_store == OutStore::Rect || probe_store == OutStore::RectStride ? TuneProbe::Rect : TuneProbe::Plain;
    return r;
}

}  // namespace fc
