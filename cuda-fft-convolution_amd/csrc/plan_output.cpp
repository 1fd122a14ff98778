// plan_output.cpp -- output side of the plan core: how the maps of a group leave the device.  plan_delivery decides the OutputRoute
// (output_route.hpp) once per group and sizes the buffers it names; the stages run_group_impl (fftconv_api.cpp) calls per batch --
// launch_output_cols, launch_region, deliver_batch -- and the verbose lines that name them only read that record.
#include "plan_internal.hpp"

namespace fc {

namespace {

const char* const kMapFormatNames[] = {"fp32", "fp16", "bf16"};      // FC_MAP_*

SinkKind sink_kind(const Sink& sink) {
    if (sink.window) return SinkKind::Window;
    if (sink.packed) return SinkKind::Packed;
    return sink.location != FFTCONV_HOST ? SinkKind::DevicePtrs : SinkKind::Host;
}

// the plane the maps of a launch are combined with -- by the output kernel's store or by the crop, whichever the route names
MapPlane output_plane(const fftconv_plan* p, const OutputRoute& r, const OutLaunch& l) {
    MapPlane pl;
    if (r.plane == OutPlane::None) return pl;
    pl.kind = r.plane == OutPlane::Q ? PlaneKind::Add : PlaneKind::Scale;
    pl.plane = p->ND.p;
    pl.consts = l.consts;
    pl.plane_elems = p->g.map_elems();
    pl.pitch = p->g.fft_h;
    pl.first = l.image0 * l.per_image;
    pl.per_image = l.per_image;
    return pl;
}

}  // namespace

OutputRouteIn output_route_in(const fftconv_plan* p, SinkKind sink) {
    const Geometry& g = p->g;
    OutputRouteIn in;
    in.sink = sink;
    in.map_bytes = p->out_map_bytes();
    in.host_stream = p->opt_host_stream; in.host_min_kb = p->opt_host_min_kb; in.host_pinned = p->opt_host_pinned != 0;
    in.region = p->opt_region; in.rect_store = p->opt_rect_store != 0;
    in.score = p->opt_score; in.norm_store = p->opt_norm_store != 0;
    in.blockwise = p->tiled != nullptr;
    in.map_format = (int)p->opt_map_format;
    in.fast_cols = g.fast_cols.ok; in.y_tiled = g.y_tiled();
    in.rect_built = fast_cols_rect_built(g.M); in.norm_built = fast_cols_norm_built(g.M); in.sqdiff_built = fast_cols_sqdiff_built(g.M);
    in.stride_h = p->stride_h; in.stride_w = p->stride_w; in.stride_store = p->opt_stride_store != 0; in.stride_built = fast_cols_stride_built(g.M);
    in.extrema = p->extrema_on(); in.extrema_store = p->opt_extrema_store != 0;
    in.extrema_rect_built = fast_cols_rect_ext_built(g.M); in.extrema_norm_built = fast_cols_norm_ext_built(g.M); in.extrema_sqdiff_built = fast_cols_sqdiff_ext_built(g.M);
    return in;
}

int plan_delivery(fftconv_plan* p, const Sink& sink, int nbY, Delivery& d) {
    d.r = plan_output_route(output_route_in(p, sink_kind(sink)));
    if (d.r.error) return api_fail(FFTCONV_ERR_INVALID_ARG, "%s", d.r.error);
    d.stage = d.r.staging == OutBuffer::OC ? &p->OC : d.r.staging == OutBuffer::O ? &p->O : nullptr;
    d.oe = p->out_elems();
    d.eb = p->elem_bytes();
    // host output: the ring for maps of at least host_min_kb (1 MiB).  Smaller ones leave by blocking copies on the plan's stream:
    // the copy threads buy them nothing (a one-shot call would start and join them for a few hundred KB), and
    // small destination buffers are heap neighbours that share pages, which the runtime pins in place from
    // several threads at once.  A one-shot call on 92-KB maps died (SIGABRT / SIGSEGV, no message) about once
    // in 50-100 runs of tests/test_gpu_parity.py::test_blockwise_one_shot_matches_oracle on some boxes of the
    // pool and never on others; the cause was not isolated, these threads are what that call had to itself.
    if (d.r.need_O)
        if (int rc = p->O.ensure(p->g.map_elems() * nbY)) return rc;
    if (d.stage)
        if (int rc = d.stage->ensure(floats_for(d.oe * nbY * d.r.staging_copies, d.eb))) return rc;
    if (d.r.extrema == OutExtrema::Fused)
        FC_VERBOSE(p, "extrema: fused -- found by the output kernel in its store, one partial per tile and wave, folded per launch");
    else if (d.r.extrema == OutExtrema::Scan)
        FC_VERBOSE(p, "extrema: scanned -- the %s maps of %zu elements are read where they lie, %d blocks per map, folded per launch", kMapFormatNames[d.r.map_format],
                   d.oe, extrema_scan_blocks(d.oe * d.eb));
    if (p->peaks_on())
        FC_VERBOSE(p, "peaks: scanned -- the %s maps of %zu elements are read where they lie, %d units per map, %s at threshold %g, radius (%d, %d), at most %d per map",
                   kMapFormatNames[d.r.map_format], d.oe, peaks_units(d.oe * d.eb), p->peaks_mode == FC_PEAKS_MIN ? "minima" : "maxima", (double)p->peaks_threshold,
                   p->peaks_radius_h, p->peaks_radius_w, p->peaks_max);
    if (d.r.route == Route::Ring) return ring_begin(p);
    return 0;
}

// the launch that stores ny maps of the route's rectangle -- the plan's, or the whole window standing in for one -- from the
// intermediate y, dense from `out` on; a fused route (RectScale, RectAdd): with the plane of the launch's images and kernels; RectStride:
// the strided launch of that extent
FastColsShape output_rect_shape(const fftconv_plan* p, const OutputRoute& r, const c32* y, float* out, int ny, const OutLaunch& l) {
    const Geometry& g = p->g;
    const bool whole = r.extent == OutExtent::Window;
    const FastColsArgs fa = fast_cols_args(g, p->d, y, out, p->out_elems(), ny, r.kernel_format);
    if (r.store == OutStore::RectStride)
        return fast_cols_stride_launch_shape(g.fast_cols.T, fa, whole ? 0 : p->off_h, whole ? 0 : p->off_w, p->ext_h(), p->ext_w(), p->stride_h, p->stride_w,
                                             persistent_want(g.fast_cols.lds_bytes, g.fast_cols.NT, p->num_cus));
    return fast_cols_rect_launch_shape(g.fast_cols.T, fa, whole ? 0 : p->off_h, whole ? 0 : p->off_w, whole ? g.fft_h : p->out_h, whole ? g.fft_w : p->out_w,
                                       persistent_want(g.fast_cols.lds_bytes, g.fast_cols.NT, p->num_cus), r.fused() ? output_plane(p, r, l) : MapPlane{});
}

// output columns of ny maps: Y transformed along h into the maps at obase (or into the window of an overlap-save block)
int launch_output_cols(fftconv_plan* p, const OutputRoute& r, const OutWindow* win, float* obase, int ny, const OutLaunch& l) {
    const Geometry& g = p->g;
    const int format = r.kernel_format;
    if (int rc = p->prof_begin(PK_OUT_COLS, ny)) return rc;
    if (r.store == OutStore::Generic) {
        FC_VERBOSE(p, "output kernel: generic%s, %s elements", g.bluestein_h() ? " (chirp-z)" : "", kMapFormatNames[format]);
        ColsC2RArgs ca = cols_c2r_args(g, p->t, p->d, p->Y.p, obase, g.map_elems(), format);
        HIP_TRY(launch_cols_c2r(ca, tiles_for(g.fft_w, g.T_cols), ny, cols_threads(g), p->cols_lds(), p->stream));
    } else if (r.store == OutStore::Plain) {
        FastColsArgs fa = fast_cols_args(g, p->d, p->Y.p, obase, win ? win->map_stride : g.map_elems(), ny, format);
        if (win) {
            fa.h_lo = win->h_lo; fa.fft_h = win->h_hi; fa.w_first = win->w_first; fa.out_pitch = win->pitch;
            fa.tiles_per_kernel = win->ncols / g.fast_cols.T; fa.ntiles = fa.tiles_per_kernel * ny;
        }
        if (p->opt_verbose) {      // which instantiation the launch layer picks (fast_paths.hpp: fast_cols_launch_shape), and what it stores
            static const char* const variants[] = {"row-major", "tiled", "tiled, sliced tail round", "tiled, dynamic tile queue"};
            const FastColsShape sh = fast_cols_launch_shape(g.M, g.fast_cols.T, fa, persistent_want(g.fast_cols.lds_bytes, g.fast_cols.NT, p->num_cus));
            FC_VERBOSE(p, "output kernel: %s intermediate, %d workgroups, %s elements", variants[(int)sh.variant], sh.grid, kMapFormatNames[format]);
        }
        HIP_TRY(launch_fast_cols(g.M, g.fast_cols.T, fa, p->num_cus, p->stream));
    } else {
        static const char* const fused[] = {"", "scaled by D (normalisation: fused)", "scaled by Dc (normalisation: fused CCORR_NORMED)",
                                            "plus Q + c (normalisation: fused SQDIFF)"};      // OutPlane
        FastColsShape sh = output_rect_shape(p, r, p->Y.p, obase, ny, l);
        const bool ext = r.extrema == OutExtrema::Fused;
        if (ext) {      // (the partials of the launch: sized by fftconv_plan_set_extrema for the whole window's tiles, never here)
            if (fast_cols_extrema_slots(sh, g.fast_cols.NT) > p->extrema_slots || ny > p->extrema_launch_maps)
                return api_fail(FFTCONV_ERR_INVALID_ARG, "per-map extrema: the launch needs %d partials per map for %d maps, the plan holds %d for %d",
                                fast_cols_extrema_slots(sh, g.fast_cols.NT), ny, p->extrema_slots, p->extrema_launch_maps);
            sh.extrema.partials = p->EXP.p;
        }
        if (r.store == OutStore::RectStride)
            FC_VERBOSE(p, "output kernel: tiled rectangle, stride (%d, %d) fused in the store (%s), %d workgroups on %d tiles, fp32 elements, rows [%d, %d) of columns [%d, %d) into %d x %d maps",
                       p->stride_h, p->stride_w, sh.a.rect_wide ? "pair stores" : "element stores", sh.grid, sh.a.ntiles, sh.a.h_lo, sh.a.fft_h, sh.a.rect_w_lo,
                       sh.a.rect_w_lo + p->ext_w(), p->map_h(), p->map_w());
        else if (r.fused())
            FC_VERBOSE(p, "output kernel: tiled rectangle %s, %d workgroups, fp32 elements, rows [%d, %d) of columns [%d, %d), images %d..", fused[(int)r.plane],
                       sh.grid, sh.a.h_lo, sh.a.fft_h, sh.a.rect_w_lo, sh.a.rect_w_lo + sh.a.rect_w_n, l.image0);
        else
            FC_VERBOSE(p, "output kernel: tiled rectangle, %d workgroups, %s elements, rows [%d, %d) of columns [%d, %d)", sh.grid, kMapFormatNames[format],
                       sh.a.h_lo, sh.a.fft_h, sh.a.rect_w_lo, sh.a.rect_w_lo + sh.a.rect_w_n);
        if (ext) HIP_TRY(launch_fast_cols_rect_extrema(g.M, g.fast_cols.T, sh, p->stream));
        else HIP_TRY(launch_fast_cols_rect(g.M, g.fast_cols.T, sh, p->stream));
    }
    return p->prof_end();
}

// per-map extrema of a launch's delivered maps: the records [l.record0, l.record0 + ny)
int launch_extrema(fftconv_plan* p, const OutputRoute& r, const float* dest, int ny, const OutLaunch& l) {
    if (r.extrema == OutExtrema::Off) return 0;
    const size_t oe = p->out_elems();
    const int out_h = r.after == OutAfter::Pad ? p->out_h : p->map_h();      // rows per column of a delivered map
    if (l.record0 < 0 || (long)l.record0 + ny > (long)p->extrema_max_maps || ny > p->extrema_launch_maps)
        return api_fail(FFTCONV_ERR_INVALID_ARG, "per-map extrema: records %d..%d in a launch of %d maps asked of a plan that holds %d records and the partials of %d maps "
                        "(fftconv_plan_set_extrema sizes them for the \"batch_maps\" of its time)", l.record0, l.record0 + ny - 1, ny, p->extrema_max_maps, p->extrema_launch_maps);
    int per_map;
    if (r.extrema == OutExtrema::Fused) {
        // (what launch_output_cols launched and checked: the tiles that hold a column of the extent x the waves of a workgroup)
        const FastColsShape sh = output_rect_shape(p, r, p->Y.p, const_cast<float*>(dest), ny, l);
        per_map = fast_cols_extrema_slots(sh, p->g.fast_cols.NT);
    } else {
        per_map = extrema_scan_blocks(oe * fc_map_elem_bytes(r.map_format));
        if (per_map > p->extrema_slots)
            return api_fail(FFTCONV_ERR_INVALID_ARG, "per-map extrema: the scan needs %d partials per map, the plan holds %d", per_map, p->extrema_slots);
        HIP_TRY(launch_extrema_scan(dest, oe, oe, r.map_format, ny, p->EXP.p, p->stream));
    }
    HIP_TRY(launch_extrema_fold(p->EXP.p, per_map, ny, out_h, p->EXR.p + l.record0, p->stream));
    return 0;
}

// peak lists of a launch's delivered maps: found and records [l.record0, l.record0 + ny), always by the scan of the maps where they lie
int launch_peaks_scan(fftconv_plan* p, const OutputRoute& r, const float* dest, int ny, const OutLaunch& l) {
    if (!p->peaks_on()) return 0;
    const size_t oe = p->out_elems();
    const int out_h = r.after == OutAfter::Pad ? p->out_h : p->map_h();      // rows per column of a delivered map
    if (l.record0 < 0 || (long)l.record0 + ny > (long)p->peaks_max_maps || ny > p->peaks_launch_maps)
        return api_fail(FFTCONV_ERR_INVALID_ARG, "peak lists: records %d..%d in a launch of %d maps asked of a plan that holds %d lists and the scratch of %d maps "
                        "(fftconv_plan_set_peaks sizes them for the \"batch_maps\" of its time)", l.record0, l.record0 + ny - 1, ny, p->peaks_max_maps, p->peaks_launch_maps);
    const PeakRule rule = peak_rule(p->peaks_mode, p->peaks_threshold, p->peaks_radius_h, p->peaks_radius_w);
    HIP_TRY(launch_peaks(dest, oe, oe, r.map_format, out_h, ny, rule, p->peaks_max, p->PKS.p, p->PKF.p + l.record0, p->PKR.p + (size_t)l.record0 * p->peaks_max, p->stream));
    return 0;
}

// what follows the output kernel on a route with a crop: nmaps full fp32 windows at src compacted into dst -- cropped, or padded to
// the pow2 window -- and combined with the route's plane on the way (the whole window is then a crop too)
int launch_region(const fftconv_plan* p, const OutputRoute& r, const float* src, float* dst, int nmaps, hipStream_t s, const OutLaunch& l) {
    const Geometry& g = p->g;      // (block-wise plans: g holds the whole window)
    const bool whole = r.extent == OutExtent::Window, pad = r.after == OutAfter::Pad;
    const int fh = whole ? 0 : p->off_h, fw = whole ? 0 : p->off_w;
    const int oh = pad ? p->out_h : p->map_h(), ow = pad ? p->out_w : p->map_w();      // of a delivered map (a stride: the sampled rows and columns; never padded)
    if (p->strided())
        FC_VERBOSE(p, "output stride (%d, %d): staged -- sampled by the crop from rows [%d, %d) of columns [%d, %d) of the fp32 window", p->stride_h, p->stride_w, fh,
                   fh + p->ext_h(), fw, fw + p->ext_w());
    const char* const how = pad ? "padded" : "cropped";
    const char* const format = kMapFormatNames[r.map_format];      // of dst; src is fp32
    if (r.plane != OutPlane::None) {
        static const char* const staged[] = {"", "staged", "staged CCORR_NORMED", "staged SQDIFF"};      // OutPlane
        static const char* const combined[] = {"", "scaled by D", "scaled by Dc", "plus Q + c"};
        FC_VERBOSE(p, "normalisation: %s -- %d maps of images %d.. %s while %s from the fp32 window into %d x %d %s maps", staged[(int)r.plane], nmaps, l.image0,
                   combined[(int)r.plane], how, oh, ow, format);
    } else if (r.extent == OutExtent::Rect)
        FC_VERBOSE(p, "output rectangle: %d maps cropped from the fp32 window, rows [%d, %d) of columns [%d, %d), into %s maps", nmaps, fh, fh + p->ext_h(), fw, fw + p->ext_w(), format);
    else FC_VERBOSE(p, "output region %ld: %d maps %s from the fp32 window into %d x %d %s maps", p->opt_region, nmaps, how, oh, ow, format);
    const MapPlane pl = output_plane(p, r, l);
    if (pad) HIP_TRY(launch_pad_maps(src, g.fft_h, g.fft_w, g.map_elems(), dst, oh, ow, p->out_elems(), nmaps, s, r.map_format, pl));
    else HIP_TRY(launch_crop_maps(src, g.fft_h, g.map_elems(), dst, oh, ow, p->out_elems(), fh, fw, nmaps, s, r.map_format, pl, p->stride_h, p->stride_w));
    return 0;
}

namespace {

// Route::Pinned -- small maps to host arrays: as many as fit the plan's pinned buffer come back in ONE copy and are handed
// out by the CPU (a copy into pageable memory is a blocking runtime call per map)
// (two halves: the copy of the next chunk runs while the CPU hands out the current one; a single map above
//  FC_PIN_ONE_MAP_BYTES takes the plain copy of deliver_batch: the CPU's pass over it costs more than the runtime's pinning --
//  one 324-KiB map: 77 against 60 us per convolve, four of them: 131 against 166, profiles/r04s_small_call_latency.txt)
int deliver_pinned(fftconv_plan* p, const Delivery& d, float* const* out, int ny) {
    const size_t mb = d.mb();
    const int per_copy = (int)std::min<size_t>((size_t)ny, (FC_PIN_OUT_BYTES / 2) / mb);
    const int nchunks = (ny + per_copy - 1) / per_copy;
    if (int rc = p->pin_out.ensure((size_t)per_copy * mb * (nchunks > 1 ? 2 : 1))) return rc;
    for (int h = 0; h < 2; h++)
        if (!p->pin_out_done[h]) HIP_TRY(hipEventCreateWithFlags(&p->pin_out_done[h], hipEventDisableTiming));
    auto copy_chunk = [&](int c) -> hipError_t {
        const int j0 = c * per_copy, nj = std::min(per_copy, ny - j0);
        hipError_t e = hipMemcpyAsync(p->pin_out.p + (size_t)(c & 1) * per_copy * mb, map_at(d.stage->p, (size_t)j0 * d.oe, d.eb), (size_t)nj * mb,
                                      hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipEventRecord(p->pin_out_done[c & 1], p->stream);
        return e;
    };
    HIP_TRY(copy_chunk(0));
    for (int c = 0; c < nchunks; c++) {
        if (c + 1 < nchunks) HIP_TRY(copy_chunk(c + 1));
        HIP_TRY(hipEventSynchronize(p->pin_out_done[c & 1]));
        const int j0 = c * per_copy, nj = std::min(per_copy, ny - j0);
        for (int j = 0; j < nj; j++)
            memcpy(out[j0 + j], p->pin_out.p + ((size_t)(c & 1) * per_copy + j) * mb, mb);
    }
    return 0;   // (the staging buffer is free again: its last copy has been waited for)
}

}  // namespace

// the maps [first, first + ny) are queued into `dest` (staging buffer buf of a streamed group): their way to the caller
int deliver_batch(fftconv_plan* p, const Delivery& d, const Sink& sink, int first, int ny, int buf, const float* dest) {
    if (d.r.route == Route::Ring) return ring_batch_launched(p, sink, first, ny, buf, dest);
    if (d.r.route == Route::Pinned && (ny > 1 || d.r.pinned_one_map)) return deliver_pinned(p, d, sink.ptrs + first, ny);
    if (!d.r.staged()) return 0;         // the kernels wrote where the caller reads
    for (int j = 0; j < ny; j++)
        HIP_TRY(hipMemcpyAsync(sink.ptrs[first + j], map_at(dest, (size_t)j * d.oe, d.eb), d.mb(), copy_kind(sink.location, false), p->stream));
    if (sink.location == FFTCONV_HOST) HIP_TRY(hipStreamSynchronize(p->stream));
    return 0;
}

}  // namespace fc
