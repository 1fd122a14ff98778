// plan_image.cpp -- image side of the plan core: the image's way into a plan (fftconv_plan_set_image / set_images /
// set_images_typed), the spectrum buffer and the spectrum exchange in the reference's order.  A one-pass call decides its route once
// (image_route.hpp: plan_image_route) and is then a sequence of stages that read it; what the stages queue, and in which order, is
// set_images_impl from top to bottom.
#include "plan_internal.hpp"

namespace {

// Typed elements at a device pointer, or at the host after their H2D copy into IT, become fp32 in I on stream s: the staged
// conversion of a one-pass call and of a block-wise plan.  (The caller has sized I, and IT for a host image.)
// stale: a flag that stops holding once the conversion is about to be queued (a block-wise plan's have_image), cleared here
int pixels_to_image_staging(fftconv_plan* p, const void* typed, int location, int fmt, size_t n, hipStream_t s, const char* note, bool* stale = nullptr) {
    if (location == FFTCONV_HOST) {
        HIP_TRY(hipMemcpyAsync(p->IT.p, typed, n * fc_pixel_elem_bytes(fmt), hipMemcpyHostToDevice, s));
        typed = p->IT.p;
    }
    FC_VERBOSE(p, "typed pixels (format %d): staged -- %zu elements converted into the fp32 image staging%s", fmt, n, note);
    if (stale) *stale = false;
    HIP_TRY(launch_pixels_to_f32(typed, fmt, p->I.p, n, s));
    return 0;
}

// A block-wise plan: its blocks are cut from an fp32 image, so typed pixels are converted on the device first (the plan's own stream
// is the block plan's) and the blocks are taken as from a device image.
int set_image_blockwise(fftconv_plan* p, const void* vdata, int fmt, int location) {
    if (fmt == FC_PIXEL_F32) {
        const int rc = tiled_set_image(p, static_cast<const float*>(vdata), location);
        if (!rc) p->pixel_format = FC_PIXEL_F32;
        return rc;
    }
    TiledState* ts = p->tiled;
    const hipStream_t st = ts->sub->stream;
    const size_t n = (size_t)ts->H * ts->W * ts->F;
    if (int rc = p->I.ensure(n)) return rc;
    if (location == FFTCONV_HOST)
        if (int rc = p->IT.ensure(floats_for(n, fc_pixel_elem_bytes(fmt)))) return rc;
    if (int rc = pixels_to_image_staging(p, vdata, location, fmt, n, st, " (block-wise plan)", &ts->have_image)) return rc;
    if (location == FFTCONV_HOST) HIP_TRY(hipStreamSynchronize(st));      // the caller's array has been consumed
    const int rc = tiled_set_image(p, p->I.p, FFTCONV_DEVICE);
    if (!rc) p->pixel_format = fmt;
    return rc;
}

ImageRoute image_route_of(const fftconv_plan* p, int fmt, int nimg, int location) {
    const Geometry& g = p->g;
    ImageRouteIn in;
    in.format = fmt; in.n_images = nimg; in.host = location == FFTCONV_HOST;
    in.H = g.H; in.W = g.W; in.F = g.F; in.max_kh = g.max_kh; in.max_kw = g.max_kw;
    in.host_pinned = p->opt_host_pinned != 0;
    in.pixel_direct = p->pixel_direct(); in.border_direct = p->border_direct();
    in.border_mode = p->border_mode != 0; in.fast_fwd = g.fast_fwd; in.normalise = p->score_planes();
    in.request = !p->a_holds.pending() ? KernelRequest::None : p->a_holds.pending_off_stream(p->stream) ? KernelRequest::OtherStream : KernelRequest::ThisStream;
    return plan_image_route(in);
}

// The caller's `bytes` of pixels on their way to the device, and the staging buffers the later stages write: hands back the
// device-visible pointer the first of them reads (elements of the caller's format).
int stage_image(fftconv_plan* p, const ImageRoute& r, const void* vdata, size_t bytes, const void** dimg) {
    const void* src = vdata;
    if (r.source == ImageSource::PinnedInPlace || r.source == ImageSource::PinnedCopy) {      // the CPU consumes the caller's array
        if (int rc = p->pin_img.ensure(bytes)) return rc;
        if (int rc = p->pin_img.wait()) return rc;
        memcpy(p->pin_img.p, vdata, bytes);
        src = p->pin_img.p;      // (PinnedInPlace: the column pass reads it there)
    }
    if (r.landing != ImageLanding::None) {
        const bool typed = r.landing == ImageLanding::IT;
        DevBuf<float>& dev = typed ? p->IT : p->I;
        if (int rc = dev.ensure(typed ? r.it_elems : r.i_elems)) return rc;
        HIP_TRY(hipMemcpyAsync(dev.p, src, bytes, hipMemcpyHostToDevice, p->stream));
        src = dev.p;
    }
    if (r.convert)
        if (int rc = p->I.ensure(r.i_elems)) return rc;
    if (r.extend)
        if (int rc = p->IE.ensure(r.ie_elems)) return rc;
    *dimg = src;
    return 0;
}

// the reference's debug lines of the image transform
void announce_image(const fftconv_plan* p, int nimg) {
    const Geometry& g = p->g;
    FC_VERBOSE(p, "Using GPU : %d", p->gpu_id);                                                    // src/cudaConvolutionFFT.cu:87
    FC_VERBOSE(p, "Data size: h=%d, w=%d, f=%d", g.H, g.W, g.F);                                   // :100
    if (nimg > 1) FC_VERBOSE(p, "Images: %d (one forward pass over %d planes)", nimg, nimg * g.F);
    char chirp[96] = "";          // windows that do not factor into the radices: Bluestein transforms on longer work lengths
    if (g.bluestein_h() || g.bluestein_w()) {
        char hs[32] = "", ws[32] = "";
        if (g.bluestein_h()) snprintf(hs, sizeof(hs), " h %d via %d", g.M, g.work_m);
        if (g.bluestein_w()) snprintf(ws, sizeof(ws), " w %d via %d", g.Lw, g.work_w);
        snprintf(chirp, sizeof(chirp), ", chirp-z passes:%s%s%s", hs, (hs[0] && ws[0]) ? "," : "", ws);
    }
    FC_VERBOSE(p, "FFT size: h=%d, w=%d (internal transform %d x %d, %s column pass, %s row pass, %s intermediate%s)", g.fft_h, g.fft_w, g.Lh, g.Lw,   // :114
               g.fast_fwd ? "specialised" : "generic", g.fast_rows.ok ? "specialised" : "generic", g.y_tiled() ? "tiled" : "row-major", chirp);
}

// The plan holds no image until the new spectra are queued (a larger batch reallocates the plan's own buffer): the spectrum buffer
// for nimg images and, for normalised maps, their scale planes and the statistics' scratch
int prepare_image_state(fftconv_plan* p, int nimg) {
    const Geometry& g = p->g;
    p->n_images = 0;
    p->pixel_format = FC_PIXEL_F32;
    if (int rc = p->ensure_spectrum(nimg)) return rc;
    if (p->score_planes()) {
        if (int rc = p->ND.ensure(g.map_elems() * (size_t)nimg)) return rc;
        if (int rc = p->NS64.ensure((size_t)2 * g.F * ncc_strip_columns(g.fft_h, g.fft_w, g.F, (int)p->norm_box_w, FC_NCC_SCRATCH_BYTES) * g.fft_h)) return rc;
    }
    return 0;
}

// The image's column pass (the staged conversion and extension count as part of it): h-transform of nimg * F planes into the
// spectrum buffer.  *pixels: what the pass read once a border is set aside -- dimg, or the fp32 image in I -- elements of
// r.stats_format, which the window statistics read too.
int launch_image_cols(fftconv_plan* p, const ImageRoute& r, const void* dimg, int fmt, int nimg, const void** pixels) {
    const Geometry& g = p->g;
    const int planes = nimg * g.F;
    const bool border = p->border_mode != 0;
    const int eh = g.H + g.max_kh - 1, ew = g.W + g.max_kw - 1;      // the image extended by a border
    if (int rc = p->prof_begin(PK_IMAGE_COLS, planes)) return rc;
    if (r.convert) {
        if (int rc = pixels_to_image_staging(p, dimg, FFTCONV_DEVICE, fmt, (size_t)g.H * g.W * planes, p->stream, "")) return rc;
        dimg = p->I.p;
    }
    *pixels = dimg;
    const float* in = static_cast<const float*>(dimg);      // (direct pixels: opaque -- elements of fmt)
    const BorderLoad bd = border ? border_load((int)p->border_mode, p->border_value, g.H, g.W, g.max_kh, g.max_kw) : BorderLoad();
    if (r.extend) {
        FC_VERBOSE(p, "border (mode %ld): staged -- %zu elements extended into the fp32 image staging", p->border_mode, r.ie_elems);
        HIP_TRY(launch_extend_image(in, p->IE.p, g.H, g.W, eh, ew, (size_t)planes, bd, p->stream));
        in = p->IE.p;
    }
    // the planes at `in` are the data's, or the extension's once it is materialised; a border transforms the extension's counts
    const int h_data = r.extend ? eh : g.H, w_data = r.extend ? ew : g.W, h_count = border ? eh : g.H, w_count = border ? ew : g.W;
    if (r.columns == ImageColumns::Generic) {
        ColsR2CArgs ia = image_cols_args(g, p->t, p->d, in, p->spec(), h_data, w_data);
        HIP_TRY(launch_cols_r2c(ia, tiles_for(w_data, g.T_cols), planes, cols_threads(g), p->cols_lds(), p->stream));
        return p->prof_end();
    }
    const FastColsFwdArgs fa = image_fwd_args(g, p->d, in, h_data, w_data, h_count, w_count, planes, p->spec());
    switch (r.columns) {
    case ImageColumns::FastBorder:
        FC_VERBOSE(p, "border (mode %ld): direct -- mapped in the column kernel's load", p->border_mode);
        HIP_TRY(launch_fast_cols_fwd_border(g.M, g.fast_cols.T, fa, bd, p->num_cus, p->stream));
        break;
    case ImageColumns::FastTyped: {
        const PixelLoad px = fast_cols_fwd_pixel_load(fa, fmt);
        FC_VERBOSE(p, "typed pixels (format %d): direct -- converted in the column kernel's load, %s loads", fmt, px.wide ? "pair" : "element");
        HIP_TRY(launch_fast_cols_fwd_px(g.M, g.fast_cols.T, fa, px, p->num_cus, p->stream));
        break;
    }
    case ImageColumns::Pair: {
        // the deferred kernel-column pass of fftconv_plan_prepare_kernels_packed and the image's column pass: ONE launch
        ColumnCache::Request pd;
        if (!p->a_holds.take_pending(pd)) {      // (not since the route saw it pending on p->stream; the image's pass alone is always right)
            HIP_TRY(launch_fast_cols_fwd(g.M, g.fast_cols.T, false, fa, p->num_cus, p->stream));
            break;
        }
        const FastColsFwdArgs fk = kernels_fwd_args(g, p->d, p->opt_score ? p->KN.p : pd.dk, pd.kh, pd.kw, pd.na * g.F, p->A.p);
        FC_VERBOSE(p, "image columns (%d tiles) and the columns of %d kernels (%d tiles) in one launch", fa.ntiles, pd.na, fk.ntiles);
        HIP_TRY(launch_fast_cols_fwd_pair(g.M, g.fast_cols.T, fa, fk, fast_cols_fwd_pruned_ok(g.fast_cols, pd.kh), p->num_cus, p->stream));
        p->a_holds.ready(pd);
        break;
    }
    default:
        HIP_TRY(launch_fast_cols_fwd(g.M, g.fast_cols.T, false, fa, p->num_cus, p->stream));
    }
    return p->prof_end();
}

// window statistics of normalised maps (ncc.hpp), while the pixels are still there: D of every image, in strips of columns
int launch_window_statistics(fftconv_plan* p, const void* pixels, int format, int nimg) {
    const Geometry& g = p->g;
    const int strip = ncc_strip_columns(g.fft_h, g.fft_w, g.F, (int)p->norm_box_w, FC_NCC_SCRATCH_BYTES);
    FC_VERBOSE(p, "window statistics: box %ld x %ld, %d images, strips of %d columns (%zu bytes of float64 scratch)", p->norm_box_h, p->norm_box_w,
               nimg, strip, (size_t)2 * g.F * strip * g.fft_h * sizeof(double));
    const size_t image_bytes = (size_t)g.F * g.H * g.W * fc_pixel_elem_bytes(format);
    for (int b = 0; b < nimg; b++)
        HIP_TRY(launch_score_statistics_typed((int)p->opt_score, static_cast<const char*>(pixels) + b * image_bytes, format, g.H, g.W, g.F, g.fft_h, g.fft_w,
                                            (int)p->norm_box_h, (int)p->norm_box_w, p->NS64.p, strip, p->ND.p + (size_t)b * g.map_elems(), p->stream));
    return 0;
}

// the image's row pass: w-transform of the spectrum rows, in place (with the fast row kernel it stores them in that kernel's
// register order)
int launch_image_rows(fftconv_plan* p, int planes) {
    const Geometry& g = p->g;
    if (int rc = p->prof_begin(PK_IMAGE_ROWS, planes)) return rc;
    if (g.fast_rows.ok) {
        HIP_TRY(launch_fast_rows_fwd(g.Lw, fast_rows_fwd_args(g, p->d, p->spec(), p->border_cols()), planes * g.rows, p->stream));
    } else {
        RowsFwdArgs ra = image_rows_args(g, p->t, p->d, p->spec(), p->border_cols());
        HIP_TRY(launch_rows_fwd(ra, planes * g.rows, rows_threads(g), g.rows_fwd_lds_bytes(), p->stream));
    }
    return p->prof_end();
}

// Zero-pad + forward transform of nimg images back to back at `vdata` ([b][f][w][h]), elements of fmt (FFTCONV_PIXEL_*): ONE
// forward pass over nimg * F planes -- the spectra land [b][f][row][s_pitch] in the spectrum buffer, so the column and row kernels
// run as for one image with more planes and rows, and the launch count is that of one image.
int set_images_impl(fftconv_plan* p, const void* vdata, int fmt, int nimg, int location) {
    if (nimg < 1) return api_fail(FFTCONV_ERR_INVALID_ARG, "n_images must be at least 1 (got %d)", nimg);
    if (!p || !vdata) return api_fail(FFTCONV_ERR_INVALID_ARG, "Invalid data input");
    if (!fc_pixel_format_ok(fmt))
        return api_fail(FFTCONV_ERR_INVALID_ARG, "pixel_format is 0 (fp32), 1 (uint8), 2 (uint16), 3 (fp16) or 4 (bfloat16), got %d", fmt);
    if (location != FFTCONV_HOST && location != FFTCONV_DEVICE) return api_fail(FFTCONV_ERR_INVALID_ARG, "bad location");
    const Geometry& g = p->g;
    if (p->tiled && nimg > 1)
        return api_fail(FFTCONV_ERR_INVALID_ARG, "a block-wise plan (%d blocks) holds one image: its block spectra are kept per image; "
                        "call fftconv_plan_set_image per image, or create a one-pass plan (fftconv_plan_options.blockwise = 1)", p->tiled->nblk);
    if (!p->tiled && p->Sx && p->Sx_bytes < (size_t)nimg * g.spectrum_elems() * sizeof(c32))
        return api_fail(FFTCONV_ERR_INVALID_ARG, "the caller's spectrum buffer (fftconv_plan_use_spectrum_buffer) holds %zu bytes, %d images need %zu",
                        p->Sx_bytes, nimg, (size_t)nimg * g.spectrum_elems() * sizeof(c32));
    if (int rc = use_device(p)) return rc;
    if (p->tiled) return set_image_blockwise(p, vdata, fmt, location);
    const ImageRoute r = image_route_of(p, fmt, nimg, location);
    const int planes = nimg * g.F;
    const void *dimg = nullptr, *pixels = nullptr;
    if (int rc = stage_image(p, r, vdata, (size_t)g.H * g.W * planes * fc_pixel_elem_bytes(fmt), &dimg)) return rc;
    announce_image(p, nimg);
    if (int rc = prepare_image_state(p, nimg)) return rc;
    if (r.flush_first)
        if (int rc = flush_pending_prepare(p)) return rc;
    if (int rc = launch_image_cols(p, r, dimg, fmt, nimg, &pixels)) return rc;
    if (p->score_planes())
        if (int rc = launch_window_statistics(p, pixels, r.stats_format, nimg)) return rc;
    if (r.pinned)
        if (int rc = p->pin_img.mark(p->stream)) return rc;      // the column pass, the copy or the statistics: the last reader
    if (int rc = launch_image_rows(p, planes)) return rc;
    if (r.sync_at_end) HIP_TRY(hipStreamSynchronize(p->stream));
    p->n_images = nimg;
    p->pixel_format = fmt;
    return 0;
}

}  // namespace

extern "C" {

int fftconv_plan_set_image(fftconv_plan* plan, const float* data, int location) { return set_images_impl(plan, data, FC_PIXEL_F32, 1, location); }
int fftconv_plan_set_images(fftconv_plan* plan, const float* data, int n_images, int location) {
    return set_images_impl(plan, data, FC_PIXEL_F32, n_images, location);
}
int fftconv_plan_set_images_typed(fftconv_plan* plan, const void* data, int pixel_format, int n_images, int location) {
    return set_images_impl(plan, data, pixel_format, n_images, location);
}

int fftconv_plan_spectrum(fftconv_plan* plan, void** device_ptr, size_t* bytes) {
    if (!plan) return api_fail(FFTCONV_ERR_INVALID_ARG, "plan is NULL");
    if (int rc = use_device(plan)) return rc;
    if (TiledState* ts = plan->tiled) {          // every block's spectrum, one after the other
        if (!ts->specs_x)
            if (int rc = ts->specs.ensure(ts->spec_total())) return rc;
        if (device_ptr) *device_ptr = ts->spec_base();
        if (bytes) *bytes = ts->spec_total() * sizeof(c32);
        return 0;
    }
    // (a plan holding B images: the whole buffer, image b at b * plan_info.spectrum_bytes)
    if (int rc = plan->ensure_spectrum()) return rc;
    if (device_ptr) *device_ptr = plan->spec();
    if (bytes) *bytes = plan->g.spectrum_elems() * sizeof(c32) * (size_t)plan->images_held();
    return 0;
}

static int spectrum_exchange(fftconv_plan* p, float* spectrum, int location, bool to_natural) {
    if (!p || !spectrum) return api_fail(FFTCONV_ERR_INVALID_ARG, "NULL argument");
    if (!to_natural)
        if (int rc = plan_refused(p, Ask::ImportSpectrum)) return rc;
    if (location != FFTCONV_HOST && location != FFTCONV_DEVICE) return api_fail(FFTCONV_ERR_INVALID_ARG, "bad location");
    if (p->tiled) return tiled_unsupported("the spectrum in the reference's order");
    const Geometry& g = p->g;
    if (!g.exact_window)
        return api_fail(FFTCONV_ERR_UNSUPPORTED_SIZE,
                    "this plan transforms %dx%d, not the %dx%d window: create it with fftconv_plan_options.exact_window = 1 to exchange "
                    "spectra in the reference's order", g.Lh, g.Lw, g.fft_h, g.fft_w);
    if (p->n_images > 1)
        return api_fail(FFTCONV_ERR_INVALID_ARG, "the plan holds %d images (fftconv_plan_set_images): the spectrum in the reference's order is "
                        "exchanged for one image -- call fftconv_plan_set_image first", p->n_images);
    if (to_natural && !p->have_image()) return api_fail(FFTCONV_ERR_NO_IMAGE, "no image spectrum: call fftconv_plan_set_image first");
    if (int rc = use_device(p)) return rc;
    if (int rc = p->ensure_spectrum()) return rc;
    if (!p->nat_col_of.p) {     // (the second of the two: both are there, or both are uploaded again)
        if (int rc = upload(p->nat_row_of, p->t.nat_row_of)) return rc;
        if (int rc = upload(p->nat_col_of, p->t.nat_col_of)) return rc;
    }
    const size_t n = (size_t)g.F * g.fft_w * g.rows;
    c32* nat = reinterpret_cast<c32*>(spectrum);
    if (location == FFTCONV_HOST) {
        if (int rc = p->NS.ensure(n)) return rc;
        nat = p->NS.p;
        if (!to_natural) HIP_TRY(hipMemcpyAsync(nat, spectrum, n * sizeof(c32), hipMemcpyHostToDevice, p->stream));
    }
    // the folded 1/(Lh*Lw) of src/cudaConvolutionFFT.cu:270 comes off on the way out and goes on on the way in
    const double norm = (double)g.Lh * (double)g.Lw;
    HIP_TRY(launch_spectrum_reorder(to_natural, p->spec(), (size_t)g.rows * g.s_pitch, g.s_pitch, nat, g.fft_w, g.rows, g.F,
                                    p->nat_row_of.p, p->nat_col_of.p, (float)(to_natural ? norm : 1.0 / norm), p->stream));
    if (location == FFTCONV_HOST) {
        if (to_natural) HIP_TRY(hipMemcpyAsync(spectrum, nat, n * sizeof(c32), hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
    }
    if (!to_natural) { p->n_images = 1; p->pixel_format = FC_PIXEL_F32; }
    return 0;
}

int fftconv_plan_export_spectrum(fftconv_plan* plan, float* spectrum, int location) { return spectrum_exchange(plan, spectrum, location, true); }
int fftconv_plan_import_spectrum(fftconv_plan* plan, const float* spectrum, int location) {
    return spectrum_exchange(plan, const_cast<float*>(spectrum), location, false);
}

int fftconv_plan_use_spectrum_buffer(fftconv_plan* plan, void* device_ptr, size_t bytes) {
    if (!plan) return api_fail(FFTCONV_ERR_INVALID_ARG, "plan is NULL");
    const size_t need = (plan->tiled ? plan->tiled->spec_total() : plan->g.spectrum_elems()) * sizeof(c32);
    if (device_ptr) {
        if (bytes < need || (reinterpret_cast<uintptr_t>(device_ptr) & 15))
            return api_fail(FFTCONV_ERR_INVALID_ARG, "spectrum buffer too small (%zu < %zu bytes) or not 16-byte aligned", bytes, need);
    }
    if (plan->tiled) {
        plan->tiled->specs_x = reinterpret_cast<c32*>(device_ptr);
        plan->tiled->have_image = false;
        return 0;
    }
    // (need: one image; fftconv_plan_set_images checks the size again for its batch)
    plan->Sx = reinterpret_cast<c32*>(device_ptr);
    plan->Sx_bytes = device_ptr ? bytes : 0;
    plan->n_images = 0;
    return 0;
}

int fftconv_plan_mark_spectrum_valid(fftconv_plan* plan) {
    if (!plan) return api_fail(FFTCONV_ERR_INVALID_ARG, "plan is NULL");
    if (int rc = plan_refused(plan, Ask::MarkSpectrumValid)) return rc;
    if (plan->tiled) {
        if (!plan->tiled->spec_base()) return api_fail(FFTCONV_ERR_NO_IMAGE, "the plan has no spectrum buffer yet (fftconv_plan_spectrum / fftconv_plan_use_spectrum_buffer)");
        if (!plan->tiled->have_image) plan->pixel_format = FC_PIXEL_F32;
        plan->tiled->have_image = true;
        return 0;
    }
    if (!plan->spec()) return api_fail(FFTCONV_ERR_NO_IMAGE, "the plan has no spectrum buffer yet (fftconv_plan_spectrum / fftconv_plan_use_spectrum_buffer)");
    if (plan->n_images < 1) { plan->n_images = 1; plan->pixel_format = FC_PIXEL_F32; }
    return 0;
}

}  // extern "C"
