// fftconv_api.cpp -- host side of libfftconv.so: the C ABI of include/fftconv.h on top of the
// HIP kernels.  C++ host code in the role of the reference's MEX gateways
// (src/cudaConvolutionFFT.cu, src/cudaFFTData.cu, src/cudaConvFFTData.cu); no CPU compute path.
#include <climits>
#include <cstdarg>
#include <cstdlib>
#include <mutex>
#include <new>
#include <set>

#include "plan_internal.hpp"

namespace {

thread_local std::string g_last_error;

}  // namespace

namespace fc {
int api_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}
std::string api_last_error() { return g_last_error; }
void api_set_last_error(const std::string& msg) { g_last_error = msg; }
}  // namespace fc

namespace {

// live plans of this process (fftconv_plan_is_live: the MEX gateways validate handles with it)
std::mutex g_live_mutex;
std::set<const fftconv_plan*> g_live_plans;

}  // namespace

namespace fc {

int cols_threads(const Geometry& g) {
    long work = (long)g.T_cols * g.work_m;   // (work lengths: a Bluestein direction runs on its longer work transform)
    if (work >= 4096) return 512;
    if (work >= 1024) return 256;
    if (work >= 256) return 128;
    return 64;
}
int rows_threads(const Geometry& g) {
    if (g.work_w >= 2048) return 256;
    if (g.work_w >= 512) return 128;
    return 64;
}

int use_device(const fftconv_plan* p) {
    HIP_TRY(hipSetDevice(p->gpu_id));
    return 0;
}

BatchSizes batch_sizes(const fftconv_plan* p, int n, int kw) {
    const Geometry& g = p->g;
    BatchSizes b;
    b.per_a = (size_t)g.F * g.rows * a_pitch_for(kw);
    const size_t y_bytes = g.y_elems_per_kernel() * sizeof(c32);
    // maps per launch.  auto: enough to amortise the last partially filled wave of workgroups (the
    // two hot kernels run ~2 "rounds" of workgroups per map on 256 CUs; 32 maps make both round
    // counts nearly integral at cfg3, and 64 let the multi-map row kernel walk 16 maps per workgroup
    // on a grid that still fills the chip), capped at 5 GiB of intermediate
    b.nbY = (int)p->opt_batch_maps;
    if (b.nbY <= 0) b.nbY = (int)std::max<size_t>(1, std::min<size_t>(64, ((size_t)5120 << 20) / y_bytes));
    // a plan holding several images: the same bound on the maps of a launch, which may then span images (pipeline.hpp: cut_launches);
    // the kernels per launch and per chunk below do not depend on the images held (prepared column spectra survive set_images)
    b.nbM = (int)std::min<long>(b.nbY, (long)n * p->images_held());
    b.nbY = std::min(b.nbY, n);
    // kernels per column-spectrum chunk.  auto: one chunk per launch of the row kernel -- the chunk (138 MB for
    // 64 kernels at cfg3) is then still in the 256-MB Infinity Cache when the row kernel prefetches its rows
    // (row kernel 22.55 -> 22.08 us per map against 192-kernel chunks, profiles/r02w_kernel_chunk_ab.txt);
    // option kernel_chunk_mb > 0: as many launches' worth as fit that budget
    b.nbA = b.nbY;
    if (p->opt_kernel_chunk_mb > 0) {
        const size_t a_budget = (size_t)p->opt_kernel_chunk_mb << 20;
        b.nbA = (int)std::max<size_t>(1, a_budget / (b.per_a * sizeof(c32)));
        b.nbA = std::max(b.nbY, b.nbA / b.nbY * b.nbY);
        b.nbA = std::min(b.nbA, (n + b.nbY - 1) / b.nbY * b.nbY);
    }
    return b;
}

int check_kernel_size(const fftconv_plan* p, int kh, int kw) {
    const Geometry& g = p->g;
    // normalised maps: the window statistics were taken over the plan's box, and a kernel of another size has another D
    if (p->opt_score && (kh != p->norm_box_h || kw != p->norm_box_w))
        return api_fail(FFTCONV_ERR_INVALID_ARG, "kernel %dx%d: while normalisation is on every kernel has the size of its box, %ldx%ld "
                        "(fftconv_plan_set_normalisation)", kh, kw, p->norm_box_h, p->norm_box_w);
    if (kh < 1 || kw < 1 || kh > g.fft_h || kw > g.fft_w)  // src/cudaConvolutionFFT.cu:242
        return api_fail(FFTCONV_ERR_KERNEL_SHAPE,
                    "Kernel and Data must have the same number of features and kernel size should be smaller than data size");
    if ((kh > g.max_kh || kw > g.max_kw) && !(g.exact_window && kh <= g.Lh && kw <= g.Lw))
        return api_fail(FFTCONV_ERR_KERNEL_EXCEEDS_MAX,
                    "kernel %dx%d exceeds MAX_KERNEL %dx%d and the internal transform (%dx%d) is not the %dx%d window",
                    kh, kw, g.max_kh, g.max_kw, g.Lh, g.Lw, g.fft_h, g.fft_w);
    if (g.fast_rows.ok && kw > g.fast_rows.max_kw)
        return api_fail(FFTCONV_ERR_KERNEL_EXCEEDS_MAX, "kernel width %d exceeds what this plan's row kernel accepts (%d)", kw,
                    g.fast_rows.max_kw);
    return 0;
}

}  // namespace fc

namespace {

// normalised maps (ncc.hpp): the na kernels at dk, centred per plane and scaled to unit joint norm, into the plan's scratch KN --
// one kernel for every kernel location, so every entry returns the same bits
// (the other scores, fftconv_plan_set_match_score: their preparation, and the constants c_k of the same na kernels into KC)
int normalise_kernels(fftconv_plan* p, const float* dk, int na, int kh, int kw) {
    const Geometry& g = p->g;
    if (int rc = p->KN.ensure((size_t)na * g.F * kh * kw)) return rc;
    if (int rc = p->NS64.ensure((size_t)2 * na * g.F)) return rc;
    if (p->opt_score == FC_SCORE_CCOEFF_NORMED) FC_VERBOSE(p, "kernel normalisation: %d kernels centred per plane and scaled to unit norm", na);
    else {
        if (int rc = p->KC.ensure((size_t)na)) return rc;
        FC_VERBOSE(p, "kernel preparation for score %s: %d kernels", score_name(p->opt_score), na);
    }
    HIP_TRY(launch_score_kernels((int)p->opt_score, dk, p->KN.p, na, g.F, kh * kw, p->NS64.p, p->KC.p, p->stream));
    return 0;
}

// h-transform of the kernels [a0, a0 + na) of a packed group into the column-spectrum buffer A
// (normalised maps: the column pass reads the normalised kernels in KN; in_kn: they are there already -- a deferred request)
int launch_kernel_cols(fftconv_plan* p, const float* dk, int a0, int na, int kh, int kw, bool in_kn = false) {
    const Geometry& g = p->g;
    if (p->opt_score) {
        if (!in_kn)
            if (int rc = normalise_kernels(p, dk + (size_t)a0 * g.F * kh * kw, na, kh, kw)) return rc;
        dk = p->KN.p;
        a0 = 0;
    }
    if (p->opt_flip_kernels) {   // template matching: correlate instead of convolve (demoCudaConvolutionFFT.m:63-69)
        const size_t chunk = (size_t)na * g.F * kh * kw;
        if (int rc = p->KF.ensure(chunk)) return rc;
        HIP_TRY(launch_flip_planes(dk + (size_t)a0 * g.F * kh * kw, p->KF.p, kh * kw, (long)na * g.F, p->stream));
        dk = p->KF.p;
        a0 = 0;
    }
    if (int rc = p->prof_begin(PK_KERNEL_COLS, na)) return rc;
    if (g.fast_fwd) {
        FastColsFwdArgs fa = kernels_fwd_args(g, p->d, dk + (size_t)a0 * g.F * kh * kw, kh, kw, na * g.F, p->A.p);
        HIP_TRY(launch_fast_cols_fwd(g.M, g.fast_cols.T, fast_cols_fwd_pruned_ok(g.fast_cols, kh), fa, p->num_cus, p->stream));
    } else {
        ColsR2CArgs ka = kernel_cols_args(g, p->t, p->d, dk + (size_t)a0 * g.F * kh * kw, kh, kw, p->A.p);
        HIP_TRY(launch_cols_r2c(ka, tiles_for(kw, g.T_cols), na * g.F, cols_threads(g), p->cols_lds(), p->stream));
    }
    return p->prof_end();
}

}  // namespace

namespace fc {
// the deferred kernel-column pass of fftconv_plan_prepare_kernels_packed, on its own (no set_image came first)
int flush_pending_prepare(fftconv_plan* p) {
    ColumnCache::Request pd;
    if (!p->a_holds.take_pending(pd)) return 0;
    const hipStream_t cur = p->stream;
    p->stream = static_cast<hipStream_t>(pd.stream);   // where the caller ordered the kernels' readiness
    const int rc = launch_kernel_cols(p, pd.dk, 0, pd.na, pd.kh, pd.kw, true);
    p->stream = cur;
    if (!rc) p->a_holds.ready(pd);
    return rc;
}
}  // namespace fc

namespace {

// spectral rows of nb x nk maps: the nk column spectra at `a` times the spectra of the images [b0, b0 + nb), transformed along w into
// the slots (b - b0) * nk + k of Y -- one launch, the image is a grid coordinate of the kernels (pipeline.hpp: rows_args_set_images;
// fast_paths.hpp: rows_walk_3d, rows_walk_flat, rows_shift_to_image, rows_generic_slot)
// Which walk a spectral-row launch of nb images x nk kernels runs and how long it is: decided ONCE per launch -- the launch and the
// verbose line that names it both read this.  image_walk: the kernel row stays in registers and the workgroup walks over images
// (fast_rows_images.hpp: "image_walk" on a plan that has the kernel, more than one image); else the walk over kernels.
struct RowsRoute {
    bool image_walk;
    int per_wg;        // images (image walk) or maps (kernel walk) per workgroup
};
RowsRoute rows_route(const fftconv_plan* p, int nb, int nk) {
    const Geometry& g = p->g;
    if (nb > 1 && p->image_walk_active()) return {true, g.images_group_for(nb, nk, p->num_cus)};
    return {false, g.rows_group_for(nk, p->num_cus)};      // (one map per workgroup where the multi-map walk is off; a walk never crosses an image)
}

int launch_spectral_rows_batch(fftconv_plan* p, const c32* a, int kw, int b0, int nb, int nk, const RowsRoute& route) {
    const Geometry& g = p->g;
    const c32* s = p->spec() + (size_t)b0 * g.spectrum_elems();
    if (int rc = p->prof_begin(PK_SPECTRAL, (long)nb * nk)) return rc;
    if (route.image_walk) {
        FastRowsArgs fa = fast_rows_args(g, p->d, a, kw, s, p->Y.p);
        rows_args_set_images(fa, g, nb, nk);
        HIP_TRY(launch_fast_rows_images(g.Lw, fa, g.rows, route.per_wg, p->stream));
    } else if (g.fast_rows.ok) {
        FastRowsArgs fa = fast_rows_args(g, p->d, a, kw, s, p->Y.p);
        rows_args_set_images(fa, g, nb, nk);
        if (p->opt_filter) {      // (fftconv_plan_set_spectral_filter: the FILTER instantiation, the mode and its parameter uniforms of the launch)
            fa.filter_mode = (int)p->opt_filter; fa.filter_param = spectral_filter_launch_param(p->opt_filter, p->filter_lambda, g.Lh, g.Lw);
            HIP_TRY(launch_fast_rows_filter(g.Lw, fast_rows_nz2(g, kw), fa, g.rows, nk, route.per_wg, p->stream));
        } else
        HIP_TRY(launch_fast_rows_multi(g.Lw, fast_rows_nz2(g, kw), fa, g.rows, nk, route.per_wg, p->stream));
    } else {
        SpectralRowsArgs sa = spectral_rows_args(g, p->t, p->d, a, kw, s, p->Y.p);
        rows_args_set_images(sa, g, nb, nk);
        sa.filter_mode = (int)p->opt_filter; sa.filter_param = spectral_filter_launch_param(p->opt_filter, p->filter_lambda, g.Lh, g.Lw);
        HIP_TRY(launch_spectral_rows(sa, g.rows, nk, rows_threads(g), p->rows_lds(), p->stream));
    }
    return p->prof_end();
}

// Core of the per-kernel loop (src/cudaConvolutionFFT.cu:204-291) for n kernels of one size,
// packed on the device at dk ([n][F][kw][kh]).  Per batch of maps: kernel columns (once per chunk), spectral rows, the wait
// for the staging buffer, output columns, crop or pad, then the batch's delivery.
int run_group_impl(fftconv_plan* p, int n, const float* dk, int kh, int kw, const Sink& sink) {
    const Geometry& g = p->g;
    if (!p->have_image()) return api_fail(FFTCONV_ERR_NO_IMAGE, "no image spectrum: call fftconv_plan_set_image first");
    if (int rc = check_kernel_size(p, kh, kw)) return rc;
    if (int rc = flush_pending_prepare(p)) return rc;
    const BatchSizes bs = batch_sizes(p, n, kw);
    // (a plan holding B images: the maps are the (image, kernel) grid, image-major, and nbY bounds the maps of a launch over it)
    const int B = p->images_held(), image_stride = sink.image_stride > 0 ? sink.image_stride : n;
    const int nbY = bs.nbM, nbA = bs.nbA;
    if (p->extrema_on()) {      // (refused ahead of any launch: the plan stays as it was)
        if (int rc = plan_refused(p, AskOutput::ExtremaGroup, 1, sink.window != nullptr)) return rc;
        if (nbY > p->extrema_launch_maps)
            return api_fail(FFTCONV_ERR_INVALID_ARG, "per-map extrema: a launch of %d maps, the partials were sized for %d (call fftconv_plan_set_extrema after \"batch_maps\")",
                            nbY, p->extrema_launch_maps);
    }
    if (p->peaks_on()) {        // (likewise)
        if (int rc = plan_refused(p, AskPeaks::PeaksGroup, 1, sink.window != nullptr)) return rc;
        if (nbY > p->peaks_launch_maps)
            return api_fail(FFTCONV_ERR_INVALID_ARG, "peak lists: a launch of %d maps, the scratch was sized for %d (call fftconv_plan_set_peaks after \"batch_maps\")", nbY,
                            p->peaks_launch_maps);
    }
    FC_VERBOSE(p, "Kernel size: h=%d, w=%d", kh, kw);                 // src/cudaConvolutionFFT.cu:240
    FC_VERBOSE(p, "N Kernel: %d (maps per launch %d, kernels per column-spectrum chunk %d, %s)", n, nbY, nbA,
               (sink.packed || sink.window) ? "packed device output" : sink.location == FFTCONV_HOST ? "host output" : "device output");   // :68
    if (int rc = p->A.ensure(bs.per_a * nbA)) return rc;
    if (int rc = p->Y.ensure(g.y_elems_per_kernel() * nbY)) return rc;
    Delivery d;
    if (int rc = plan_delivery(p, sink, nbY, d)) return rc;
    if (p->Y.fresh) {   // before anything is written into it: the tuner may keep another allocation
        // (several images: no automatic tuning -- the tuner's probe launches are shaped for the maps of one image)
        // (normalised maps: no tuning -- the probe launches are the plain output kernel's, not the scaled launch the group runs; the
        //  allocation stays marked fresh, so the first group after fftconv_plan_set_normalisation(0) tunes it as a fresh plan's)
        if (d.r.probe == TuneProbe::Skip) {}
        else if (B > 1 && p->opt_tune_placement < 0) p->Y.fresh = false;
        else if (int rc = tune_intermediate_placement(p, d.r, n * B, nbY, d.r.need_O ? p->O.p : d.stage ? d.stage->p : sink.packed)) return rc;
    }
    LaunchCutter cutter(B, n, image_stride, nbA, nbY);
    for (LaunchRect l; cutter.next(l);) {
        if (l.chunk_start) {
            const bool have_cols = p->a_holds.consume(KernelSet{dk, n, kh, kw, p->stream}) && l.a0 == 0;   // A is about to be consumed / overwritten
            if (!have_cols)
                if (int rc = launch_kernel_cols(p, dk, l.a0, l.na, kh, kw)) return rc;
        }
        {
            const int ny = l.ny(), first = l.first(image_stride);
            if (B > 1) FC_VERBOSE(p, "images %d..%d x kernels %d..%d", l.b0, l.b0 + l.nb - 1, l.k0, l.k0 + l.nk - 1);
            const RowsRoute route = rows_route(p, l.nb, l.nk);
            FC_VERBOSE(p, "maps %d..%d: spectral rows (%s, %d rows x %d points, %s%d %s per workgroup), output columns (%s, %d-point, %d columns per tile)",
                       first, first + ny - 1, g.fast_rows.ok ? "specialised" : "generic", g.rows, g.Lw, route.image_walk ? "image walk: " : "", route.per_wg,
                       route.image_walk ? "images" : "maps", g.fast_cols.ok ? "specialised" : "generic", g.M, g.fast_cols.ok ? g.fast_cols.T : g.T_cols);
            if (p->opt_filter)
                FC_VERBOSE(p, "spectral filter %ld (%s, lambda %g) in the product phase of the %s row kernel", p->opt_filter,
                           p->opt_filter == FC_FILTER_PHASE ? "phase" : "wiener", (double)p->filter_lambda, p->filter_fast() ? "specialised" : "generic");
            if (int rc = launch_spectral_rows_batch(p, p->A.p + (size_t)(l.k0 - l.a0) * bs.per_a, kw, l.b0, l.nb, l.nk, route)) return rc;
            int buf = 0;
            if (d.r.route == Route::Ring)
                if (int rc = ring_claim_staging(p, &buf)) return rc;
            float* dest = sink.window ? sink.window->base + (size_t)first * sink.window->map_stride            // where the maps of this batch go
                          : d.stage ? map_at(d.stage->p, (size_t)buf * nbY * d.oe, d.eb) : map_at(sink.packed, (size_t)first * d.oe, d.eb);
            const OutLaunch ol{l.b0, l.nk, p->KC.p ? p->KC.p + (l.k0 - l.a0) : nullptr, sink.map0 + first};      // (KC holds the chunk's kernels, as A does)
            if (int rc = launch_output_cols(p, d.r, sink.window, d.r.need_O ? p->O.p : dest, ny, ol)) return rc;
            if (d.r.after != OutAfter::None)
                if (int rc = launch_region(p, d.r, p->O.p, dest, ny, p->stream, ol)) return rc;
            if (int rc = launch_extrema(p, d.r, dest, ny, ol)) return rc;      // (behind the last kernel that writes the maps, ahead of their copy-out)
            if (int rc = launch_peaks_scan(p, d.r, dest, ny, ol)) return rc;
            if (int rc = deliver_batch(p, d, sink, first, ny, buf, dest)) return rc;
        }
    }
    if (d.r.route == Route::Ring)
        if (int rc = ring_finish(p, sink)) return rc;
    FC_VERBOSE(p, "FFT done");                                        // src/cudaConvolutionFFT.cu:258
    return 0;
}

// Options that are a `long` member of the plan and nothing else: fftconv_plan_set_option and fftconv_plan_get_option are both
// served from this table.  Options with logic of their own are code in fftconv_plan_set_option and rows of kComputedOptions.
enum : unsigned {
    OPT_BOOL = 1,       // stored as value != 0
    OPT_REJECT = 2,     // a value outside [lo, hi] is an error (otherwise it is clamped)
    OPT_OWN = 4,        // a block-wise plan answers it itself, set and get (every other name acts on its block plan)
    OPT_GET_ONLY = 16,  // get_option only: read-only, or set_option handles the name in code
    OPT_SET_ONLY = 32,
};
struct LongOption {
    const char* name;
    long fftconv_plan::*member;
    long lo, hi;
    unsigned flags;
    unsigned effects = 0;      // FX_* of plan_rules.hpp: what setting it invalidates
};
const LongOption kLongOptions[] = {
    {"tune_placement", &fftconv_plan::opt_tune_placement, -1, 8, 0},
    {"kernel_chunk_mb", &fftconv_plan::opt_kernel_chunk_mb, 0, LONG_MAX, 0, FX_COLUMNS},
    {"batch_maps", &fftconv_plan::opt_batch_maps, 0, LONG_MAX, 0, FX_COLUMNS},
    {"verbose", &fftconv_plan::opt_verbose, 0, 1, OPT_BOOL},
    {"flip_kernels", &fftconv_plan::opt_flip_kernels, 0, 1, OPT_BOOL, FX_COLUMNS},
    {"map_format", &fftconv_plan::opt_map_format, FC_MAP_F32, FC_MAP_BF16, OPT_REJECT, FX_WAIT | FX_RING | FX_COLUMNS},   // (the ring is sized for the map bytes)
    {"host_pinned", &fftconv_plan::opt_host_pinned, 0, 1, OPT_BOOL},
    {"host_min_kb", &fftconv_plan::opt_host_min_kb, 0, 1 << 30, OPT_REJECT},
    {"host_stream", &fftconv_plan::opt_host_stream, 0, 1 << 20, OPT_REJECT, FX_WAIT | FX_RING},   // (0, 1 or 2: checked once the ring is down)
    {"host_threads", &fftconv_plan::opt_host_threads, 0, 1 << 20, OPT_REJECT | OPT_SET_ONLY, FX_WAIT | FX_RING},
    {"host_chunk_kb", &fftconv_plan::opt_host_chunk_kb, 0, 1 << 20, OPT_REJECT | OPT_SET_ONLY, FX_WAIT | FX_RING},
    {"host_slots", &fftconv_plan::opt_host_slots, 0, 1 << 20, OPT_REJECT | OPT_SET_ONLY, FX_WAIT | FX_RING},
    {"tuned_candidates", &fftconv_plan::tuned_candidates, 0, 0, OPT_GET_ONLY},
    {"tuned_best", &fftconv_plan::tuned_best, 0, 0, OPT_GET_ONLY},
    {"output_region", &fftconv_plan::opt_region, 0, 0, OPT_GET_ONLY | OPT_OWN},      // (block-wise: cropped on delivery)
    {"rect_store", &fftconv_plan::opt_rect_store, 0, 1, OPT_BOOL | OPT_OWN},
    {"stride_store", &fftconv_plan::opt_stride_store, 0, 1, OPT_BOOL | OPT_OWN},   // (it only chooses the route of the next group: nothing cached depends on it)
    {"dynamic_tiles", &fftconv_plan::opt_dynamic_tiles, 0, 0, OPT_GET_ONLY},
    {"defer_prepare", &fftconv_plan::opt_defer_prepare, 0, 0, OPT_GET_ONLY},
    {"extrema_store", &fftconv_plan::opt_extrema_store, 0, 1, OPT_BOOL | OPT_OWN},   // (it only chooses the route of the next group: nothing cached depends on it)
    {"image_walk", &fftconv_plan::opt_image_walk, 0, 1, OPT_BOOL},      // (nothing cached depends on it: no FX_COLUMNS)
    {"norm_store", &fftconv_plan::opt_norm_store, 0, 1, OPT_BOOL},       // (the kernel column spectra are the same either way: no FX_COLUMNS)
    {"pixel_store", &fftconv_plan::opt_pixel_store, 0, 1, OPT_BOOL},     // (it only chooses the route of the next typed call: no FX_COLUMNS)
    {"border_store", &fftconv_plan::opt_border_store, 0, 1, OPT_BOOL},   // (it only chooses the route of the next image: no FX_COLUMNS)
    {"match_score", &fftconv_plan::opt_score, 0, 0, OPT_GET_ONLY},       // (fftconv_plan_set_match_score / _set_normalisation set the three; "normalise": get_option)
    {"norm_box_h", &fftconv_plan::norm_box_h, 0, 0, OPT_GET_ONLY},
    {"norm_box_w", &fftconv_plan::norm_box_w, 0, 0, OPT_GET_ONLY},
};
const LongOption* find_option(const char* name) {
    for (const LongOption& o : kLongOptions)
        if (!strcmp(name, o.name)) return &o;
    return nullptr;
}

// Read-only options that are computed from the plan: fftconv_plan_get_option looks here first.  own: as OPT_OWN -- a block-wise plan
// answers from its own state (the setters act on it; its routes are its own), every other name is its block plan's.
struct ComputedOption {
    const char* name;
    long (*get)(const fftconv_plan*);
    bool own;
};
const ComputedOption kComputedOptions[] = {
    // spectral filter (fftconv_plan_set_spectral_filter): the mode, and whether the next spectral-row launch under it runs the
    // specialised filter kernel (0 without a mode, and where the generic kernel's branch serves it)
    {"spectral_filter", [](const fftconv_plan* p) { return p->opt_filter; }, true},
    {"spectral_filter_fast", [](const fftconv_plan* p) { return (long)p->filter_fast(); }, true},
    // border modes (fftconv_plan_set_border): the mode, where data sample 0 lies in the window, and whether the next image on this
    // plan, with the options as they are, is mapped in the column kernel's load (0 without a border)
    {"border_mode", [](const fftconv_plan* p) { return p->border_mode; }, true},
    {"border_lead_h", [](const fftconv_plan* p) { return (long)(p->border_mode ? border_lead(p->g.max_kh) : 0); }, true},
    {"border_lead_w", [](const fftconv_plan* p) { return (long)(p->border_mode ? border_lead(p->g.max_kw) : 0); }, true},
    {"border_direct", [](const fftconv_plan* p) { return (long)p->border_direct(); }, true},
    // the caller's rectangle (fftconv_plan_set_output_rect): its offsets (0 without one), and whether the output kernel stores it
    // itself with the plan's current settings
    {"rect_off_h", [](const fftconv_plan* p) { return (long)(p->opt_region == 5 ? p->off_h : 0); }, true},
    {"rect_off_w", [](const fftconv_plan* p) { return (long)(p->opt_region == 5 ? p->off_w : 0); }, true},
    {"rect_direct", [](const fftconv_plan* p) { return (long)p->rect_direct(); }, true},
    // strided maps (fftconv_plan_set_output_stride): the strides, and whether the output kernel samples in its store with the plan's
    // current settings (else the staged crop does; a block-wise plan always crops)
    {"stride_h", [](const fftconv_plan* p) { return (long)p->stride_h; }, true},
    {"stride_w", [](const fftconv_plan* p) { return (long)p->stride_w; }, true},
    {"stride_direct", [](const fftconv_plan* p) { return (long)p->stride_direct(); }, true},
    // per-map extrema (fftconv_plan_set_extrema): the mode, the maps the records were sized for, and whether the output kernel finds them
    // in its store with the plan's current settings (else the scan kernel reads the delivered maps; 0 while it is off)
    {"extrema", [](const fftconv_plan* p) { return (long)p->extrema_on(); }, true},
    {"extrema_max_maps", [](const fftconv_plan* p) { return (long)p->extrema_max_maps; }, true},
    {"extrema_maps", [](const fftconv_plan* p) { return (long)p->extrema_maps; }, true},      // the maps of the last convolve under it (-1: none yet)
    {"extrema_direct", [](const fftconv_plan* p) { return (long)p->extrema_direct(); }, true},
    // peak lists (fftconv_plan_set_peaks): the mode, what the lists were sized for, the radii, the maps of the last convolve under it (-1: none yet)
    {"peaks", [](const fftconv_plan* p) { return (long)p->peaks_mode; }, true},
    {"peaks_max_maps", [](const fftconv_plan* p) { return (long)p->peaks_max_maps; }, true},
    {"peaks_max", [](const fftconv_plan* p) { return (long)p->peaks_max; }, true},
    {"peaks_radius_h", [](const fftconv_plan* p) { return (long)p->peaks_radius_h; }, true},
    {"peaks_radius_w", [](const fftconv_plan* p) { return (long)p->peaks_radius_w; }, true},
    {"peaks_maps", [](const fftconv_plan* p) { return (long)p->peaks_maps; }, true},
    // 1 if, with the plan's current settings, the output kernel itself scales normalised maps (else the staged crop does)
    {"normalise", [](const fftconv_plan* p) { return (long)(p->opt_score == FC_SCORE_CCOEFF_NORMED); }, true},      // (mode 1 is score 1)
    {"norm_direct", [](const fftconv_plan* p) { return (long)p->norm_direct(); }, true},
    // 1 if, with the plan's current settings, a spectral-row launch of more than one image walks over images
    {"image_walk_active", [](const fftconv_plan* p) { return (long)p->image_walk_active(); }, true},
    // typed image pixels (fftconv_plan_set_images_typed): 1 if a typed call on this plan, with the options as they are, converts in
    // the column kernel's load; the format of the images the plan holds (0: fp32, an imported spectrum, or none)
    {"pixel_direct", [](const fftconv_plan* p) { return (long)p->pixel_direct(); }, true},
    {"pixel_format", [](const fftconv_plan* p) { return (p->tiled ? p->tiled->have_image : p->have_image()) ? p->pixel_format : 0; }, true},
    {"blockwise", [](const fftconv_plan* p) { return (long)(p->tiled ? p->tiled->nblk : 0); }, true},      // number of blocks (0 = one pass)
    {"overlap_save", [](const fftconv_plan* p) { return (long)(p->tiled && p->tiled->save); }, true},      // blocks stored by the output kernel (1) or summed (0)
    // the images the plan holds -- fftconv_plan_set_images' count, 1 after fftconv_plan_set_image, 0 before any image
    {"images", [](const fftconv_plan* p) { return (long)(p->tiled ? p->tiled->have_image : p->n_images); }, true},
    {"rows_group", [](const fftconv_plan* p) { return (long)p->g.rows_group; }, false},
    // which passes of this plan run on specialised (compile-time) kernels: bit 0 the spectral rows (w), bit 1 the column passes
    // (h: image / kernel columns forwards, output columns); 3 = no generic kernel runs
    {"specialised_kernels", [](const fftconv_plan* p) { return (long)((p->g.fast_rows.ok ? 1 : 0) | (p->g.fast_cols.ok ? 2 : 0)); }, false},
    {"rows_slots_per_cu", [](const fftconv_plan* p) { return (long)p->g.rows_slots_per_cu; }, false},      // resident row workgroups per CU
    {"profile", [](const fftconv_plan* p) { return (long)p->profile; }, false},
    {"prepare_pending", [](const fftconv_plan* p) { return (long)p->a_holds.pending(); }, false},      // a recorded, not yet launched preparation
};

// the effects of a changed value (plan_rules.hpp: FX_*), in the order every setter performed them
int apply_effects(fftconv_plan* plan, unsigned effects) {
    if (effects & FX_WAIT) {
        if (int rc = use_device(plan)) return rc;
        HIP_TRY(hipStreamSynchronize(plan->stream));
    }
    if (effects & FX_RING) plan->release_ring();
    if (effects & FX_COLUMNS) plan->a_holds.forget();
    if (effects & FX_IMAGES) plan->n_images = 0;
    return 0;
}
// a setter behind its argument check and its rule lookup, ahead of its assignments: kSetterEffects' row for it.  True if the call
// ends here with rc -- a value that does not change where the row says so (0), or an effect that failed
template <class SetterId>      // (Setter, or SetterAdded: the rows plan_rules.hpp lists beside the first table)
bool setter_done(fftconv_plan* plan, SetterId s, bool unchanged, int& rc) {
    const auto& e = setter_effects(s);
    const bool early = e.unchanged_returns && unchanged;
    rc = early ? 0 : apply_effects(plan, e.changed);
    return early || rc != 0;
}

}  // namespace

namespace fc {

// run_group_impl + on failure: nothing of the host-output ring may still be writing into the
// caller's buffers when the error is returned
int run_group(fftconv_plan* p, int n, const float* dk, int kh, int kw, const Sink& sink) {
    const int rc = run_group_impl(p, n, dk, kh, kw, sink);
    if (rc && p->ring) (void)keep_error([&] { return p->ring->wait_idle(); });
    return rc;
}

int prepare_kernels(fftconv_plan* p, int n, const float* dk, int kh, int kw, bool force_defer) {
    if (int rc = use_device(p)) return rc;
    if (int rc = check_kernel_size(p, kh, kw)) return rc;
    const BatchSizes bs = batch_sizes(p, n, kw);
    if (int rc = flush_pending_prepare(p)) return rc;      // an earlier request nobody consumed
    if (int rc = p->A.ensure(bs.per_a * bs.nbA)) return rc;
    p->a_holds.forget();      // (a launch that fails below leaves nothing behind)
    const KernelSet ks{dk, n, kh, kw, p->stream};
    const int na = std::min(bs.nbA, n);
    const bool timed_apart = p->profile && (p->profile_mask & ((1u << PK_KERNEL_COLS) | (1u << PK_IMAGE_COLS)));   // per-kind figures wanted
    if ((force_defer || p->opt_defer_prepare) && p->g.fast_fwd && !p->opt_flip_kernels && !timed_apart) {   // deferred: rides in the launch of the next image's column pass
        if (p->opt_score)      // (now, while the caller's kernels are there: the deferred column pass reads KN)
            if (int rc = normalise_kernels(p, dk, na, kh, kw)) return rc;
        p->a_holds.request(ks, na);
        return 0;
    }
    if (int rc = launch_kernel_cols(p, dk, 0, na, kh, kw)) return rc;
    p->a_holds.ready(ks);
    return 0;
}

int check_thread_size(const double* thread_size, int n_thread_size) {
    // src/cudaConvolutionFFT.cu:72-73 -- the optional argument must have 4 elements
    if (thread_size != nullptr || n_thread_size != 0)
        if (n_thread_size != 4 || thread_size == nullptr)
            return api_fail(FFTCONV_ERR_THREAD_SIZE,
                        "CUDA Thread Size must be 4 integers : THREAD_PER_BLOCK_H, THREAD_PER_BLOCK_W, "
                        "THREAD_PER_BLOCK_D, THREAD_PER_BLOCK_2D");
    return 0;
}

}  // namespace fc

extern "C" {

int fftconv_fft_size16(int data_size) { return fft_size16(data_size); }
int fftconv_fft_size_pow2(int data_size) { return fft_size_pow2(data_size); }

const char* fftconv_last_error(void) { return g_last_error.c_str(); }

const char* fftconv_version(void) { return "fftconv-mi355x 0.1 (gfx950)"; }

int fftconv_device_count(int* count) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (count) *count = (e == hipSuccess) ? n : 0;
    if (e != hipSuccess || n == 0) return api_fail(FFTCONV_ERR_NO_DEVICE, "no HIP device: %s", hipGetErrorString(e));
    return 0;
}

int fftconv_plan_create(fftconv_plan** plan, int data_h, int data_w, int feature_dim, int max_kernel_h,
                        int max_kernel_w, int gpu_id, void* hip_stream) {
    return fftconv_plan_create_ex(plan, data_h, data_w, feature_dim, max_kernel_h, max_kernel_w, gpu_id, hip_stream, nullptr);
}

int fftconv_plan_is_live(const fftconv_plan* plan) {
    std::lock_guard<std::mutex> lk(g_live_mutex);
    return g_live_plans.count(plan) ? 1 : 0;
}

int fftconv_plan_create_ex(fftconv_plan** plan, int data_h, int data_w, int feature_dim, int max_kernel_h,
                           int max_kernel_w, int gpu_id, void* hip_stream, const fftconv_plan_options* options) {
    return plan_create_internal(plan, data_h, data_w, feature_dim, max_kernel_h, max_kernel_w, gpu_id, hip_stream, options, false);
}

}  // extern "C"

// What a fresh single-pass plan needs on its device: the kernels' attributes, its tables (Tables -> DeviceTables), the tile queue.
static int plan_device_setup(fftconv_plan* p) {
    const Tables& t = p->t;
    DeviceTables& d = p->d;
    if (int rc = use_device(p)) return rc;
    hipError_t e = kernels_init();
    if (e != hipSuccess) return api_fail(FFTCONV_ERR_HIP, "kernel setup failed: %s", hipGetErrorString(e));
    if (int rc = upload(p->tw_m, t.pm.tw, &d.tw_m)) return rc;
    if (int rc = upload(p->tw_w, t.pw.tw, &d.tw_w)) return rc;
    if (int rc = upload(p->pairs, t.pairs, &d.pairs)) return rc;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, p->gpu_id) == hipSuccess && prop.multiProcessorCount > 0) p->num_cus = prop.multiProcessorCount;
    if (p->g.fast_cols.ok) {
        const FastColsTables& ft = t.fcl;
        if (int rc = upload(p->fc_tw1, ft.tw1, &d.fc_tw1)) return rc;
        if (int rc = upload(p->fc_tw2, ft.tw2, &d.fc_tw2)) return rc;
        if (int rc = upload(p->fc_pairs, ft.pairs, &d.fc_pairs)) return rc;
        if (int rc = upload(p->fc_rowoff, ft.rowoff, &d.fc_rowoff)) return rc;
        if (int rc = upload(p->fc_pair_row_of, ft.pair_row_of, &d.fc_pair_row_of)) return rc;
        // Dynamic tile queue of the persistent OUTPUT kernel (option "dynamic_tiles"): on by default where a tile is long enough
        // for its one-ahead ticket to arrive in time -- M >= 432.  Alone on the GPU it then measures equal or up to 3 % faster
        // than the static deal, beside another kernel it loses half as much (profiles/r05a_contention_ab.txt); on the short
        // tiles of small transforms (M = 336: +18 %, cfg1's M = 144: +4 us a launch) it does not pay
        // (profiles/r05k_dynamic_tiles_by_size.txt).  Zeroed once; every launch leaves the counters at zero.
        if (int rc = p->queue.ensure(FC_QUEUE_WORDS)) return rc;
        if (hipMemset(p->queue.p, 0, FC_QUEUE_WORDS * sizeof(int)) != hipSuccess) return api_fail(FFTCONV_ERR_HIP, "hipMemset of the tile queue failed");
        p->opt_dynamic_tiles = p->g.M >= 432 ? 1 : 0;
        d.queue = p->opt_dynamic_tiles ? p->queue.p : nullptr;
    }
    if (p->g.fast_rows.ok && p->g.F == 1) {   // resident workgroups per CU of the multi-map row kernel: what rows_group_auto deals over
        FastRowsArgs qa = fast_rows_args(p->g, d, nullptr, p->g.max_kw, nullptr, nullptr);
        int per_cu = 0;
        if (fast_rows_multi_wgs_per_cu(p->g.Lw, fast_rows_nz2(p->g, std::min(p->g.max_kw, p->g.fast_rows.max_kw)), qa, &per_cu) == hipSuccess && per_cu > 0)
            p->g.rows_slots_per_cu = per_cu;
        else
            (void)hipGetLastError();
    }
    if (p->g.fast_rows.ok) {
        const FastRowsTables& fr = t.fr;
        if (int rc = upload(p->fr_tw1, fr.tw1, &d.fr_tw1)) return rc;
        if (int rc = upload(p->fr_tw2, fr.tw2, &d.fr_tw2)) return rc;
        if (int rc = upload(p->fr_map, fr.relayout, &d.fr_relayout)) return rc;
    }
    return 0;
}

// would plan_create_internal make a block-wise plan of these sizes and options?  (its own decision, on a geometry of its own)
static bool planner_goes_blockwise(int H, int W, int F, int mkh, int mkw, const fftconv_plan_options* options) {
    const PlanTuning tune = tuning_from(options);
    if (tune.exact_window || options_no_blockwise(options)) return false;
    Geometry g;
    Tables t;
    return !make_geometry(g, t, H, W, F, mkh, mkw, tune) || blocks_preferred(g, options);
}

// cyclic: the block plan of an overlap-save block-wise plan (PlanTuning::cyclic) -- never block-wise itself
int fc::plan_create_internal(fftconv_plan** plan, int data_h, int data_w, int feature_dim, int max_kernel_h, int max_kernel_w, int gpu_id,
                         void* hip_stream, const fftconv_plan_options* options, bool cyclic) {
    if (!plan) return api_fail(FFTCONV_ERR_INVALID_ARG, "plan is NULL");
    *plan = nullptr;
    if (data_h < 1 || data_w < 1 || feature_dim < 1) return api_fail(FFTCONV_ERR_INVALID_ARG, "Invalid data input");
    if (max_kernel_h < 1 || max_kernel_w < 1) return api_fail(FFTCONV_ERR_INVALID_ARG, "Invalid maximum kernel size");
    // 16-bit maps ("map_format"): a value out of range, or one on sizes the planner takes block-wise, is an argument error, found
    // before anything touches a device.  (a block plan stores fp32 whatever its options say)
    const int map_format = (cyclic || (options && options->struct_size < kOptionsMinSize)) ? FC_MAP_F32 : options_map_format(options);
    if (map_format != FC_MAP_F32) {
        const char* why = map_format_error(map_format, false);
        if (!why && planner_goes_blockwise(data_h, data_w, feature_dim, max_kernel_h, max_kernel_w, options)) why = map_format_error(map_format, true);
        if (why) return api_fail(FFTCONV_ERR_INVALID_ARG, "%s", why);
    }
    int ndev = 0;
    if (int rc = fftconv_device_count(&ndev)) return rc;
    if (gpu_id < 0) HIP_TRY(hipGetDevice(&gpu_id));
    if (gpu_id >= ndev) return api_fail(FFTCONV_ERR_NO_DEVICE, "gpu_id %d out of range (%d devices)", gpu_id, ndev);
    if (options && options->struct_size < kOptionsMinSize) return api_fail(FFTCONV_ERR_INVALID_ARG, "fftconv_plan_options.struct_size is not set");
    fftconv_plan* p = new (std::nothrow) fftconv_plan();
    if (!p) return api_fail(FFTCONV_ERR_ALLOC, "out of host memory");
    PlanTuning tune = tuning_from(options);
    tune.cyclic = cyclic;
    if (cyclic) { tune.exact_window = false; tune.max_transform = 0; }
    p->opt_verbose = options_verbose(options) ? 1 : 0;
    p->opt_map_format = map_format;
    p->gpu_id = gpu_id;
    p->stream = reinterpret_cast<hipStream_t>(hip_stream);
    const bool may_block = !cyclic && !options_no_blockwise(options) && !tune.exact_window;
    bool single_pass = make_geometry(p->g, p->t, data_h, data_w, feature_dim, max_kernel_h, max_kernel_w, tune);
    // large single-pass sizes run on the slower long-transform kernels: blocks of a mid-sized transform (overlap-save, the
    // output kernel storing each block's rectangle of the maps directly) are faster where the cost model says so
    if (single_pass && may_block && blocks_preferred(p->g, options)) single_pass = false;
    int rc = 0;
    if (single_pass)
        rc = plan_device_setup(p);
    // too large for one LDS-resident pass (or beyond max_transform), or faster in blocks: a block-wise plan, unless the caller opted out
    else if (cyclic)
        rc = api_fail(FFTCONV_ERR_UNSUPPORTED_SIZE, "no specialised kernels for a %dx%d block transform with kernels up to %dx%d", data_h, data_w,
                      max_kernel_h, max_kernel_w);
    else if (tune.exact_window)
        rc = api_fail(FFTCONV_ERR_UNSUPPORTED_SIZE,
                      "sizes %dx%dx%d with kernels up to %dx%d: exact_window needs transforms of the %dx%d window itself (complex lengths %d and %d, "
                      "direct or by Bluestein), and their work lengths do not fit the single-pass LDS transform%s", data_h, data_w, feature_dim,
                      max_kernel_h, max_kernel_w, fft_size16(data_h + max_kernel_h - 1), fft_size16(data_w + max_kernel_w - 1),
                      fft_size16(data_h + max_kernel_h - 1) / 2, fft_size16(data_w + max_kernel_w - 1), tune.max_transform > 0 ? " within max_transform" : "");
    else if (options_no_blockwise(options))
        rc = api_fail(FFTCONV_ERR_UNSUPPORTED_SIZE, "sizes %dx%dx%d with kernels up to %dx%d do not fit the single-pass LDS transform%s", data_h,
                      data_w, feature_dim, max_kernel_h, max_kernel_w, tune.max_transform > 0 ? " within max_transform" : "");
    else
        rc = tiled_create(p, data_h, data_w, feature_dim, max_kernel_h, max_kernel_w, hip_stream, options);
    if (rc) {
        p->release_all();      // (what plan_device_setup had uploaded; nothing in the other cases)
        delete p;
        return rc;
    }
    { std::lock_guard<std::mutex> lk(g_live_mutex); g_live_plans.insert(p); }
    *plan = p;
    return 0;
}

// per-map extrema around a convolve of n_kernel kernels on a one-pass plan: more maps than the records hold are refused ahead of any
// launch; the records count once every group has been queued
static int extrema_begin(fftconv_plan* p, int n_kernel) {
    if (!p->extrema_on()) return 0;
    const long maps = (long)n_kernel * p->images_held();
    if (maps > p->extrema_max_maps)
        return api_fail(FFTCONV_ERR_INVALID_ARG, "per-map extrema: a convolve of %ld maps on a plan whose records hold %d (fftconv_plan_set_extrema: max_maps)", maps,
                        p->extrema_max_maps);
    p->extrema_maps = -1;      // (a call that fails half-way leaves no records to read)
    return 0;
}
static void extrema_end(fftconv_plan* p, int n_kernel) {
    if (p->extrema_on()) p->extrema_maps = n_kernel * p->images_held();
}
// the same around the peak lists; both may be on, and either refusal comes ahead of either's bookkeeping
static int peaks_check(fftconv_plan* p, int n_kernel) {
    if (!p->peaks_on()) return 0;
    const long maps = (long)n_kernel * p->images_held();
    if (maps > p->peaks_max_maps)
        return api_fail(FFTCONV_ERR_INVALID_ARG, "peak lists: a convolve of %ld maps on a plan whose lists hold %d (fftconv_plan_set_peaks: max_maps)", maps, p->peaks_max_maps);
    return 0;
}
static int outputs_begin(fftconv_plan* p, int n_kernel) {
    if (int rc = peaks_check(p, n_kernel)) return rc;
    if (int rc = extrema_begin(p, n_kernel)) return rc;
    if (p->peaks_on()) p->peaks_maps = -1;      // (a call that fails half-way leaves no lists to read)
    return 0;
}
static void outputs_end(fftconv_plan* p, int n_kernel) {
    extrema_end(p, n_kernel);
    if (p->peaks_on()) p->peaks_maps = n_kernel * p->images_held();
}

extern "C" {

int fftconv_plan_destroy(fftconv_plan* plan) {
    if (!plan) return 0;
    {
        std::lock_guard<std::mutex> lk(g_live_mutex);
        if (!g_live_plans.erase(plan)) return api_fail(FFTCONV_ERR_INVALID_ARG, "not a live plan");
    }
    (void)hipSetDevice(plan->gpu_id);
    (void)hipStreamSynchronize(plan->stream);
    if (plan->tiled) {
        plan->tiled->release();
        delete plan->tiled;
        plan->tiled = nullptr;
    }
    plan->release_all();
    delete plan;
    return 0;
}

int fftconv_plan_get_info(const fftconv_plan* plan, fftconv_plan_info* info) {
    if (!plan || !info) return api_fail(FFTCONV_ERR_INVALID_ARG, "NULL argument");
    const Geometry& g = plan->g;
    info->data_h = g.H; info->data_w = g.W; info->feature_dim = g.F;
    info->max_kernel_h = g.max_kh; info->max_kernel_w = g.max_kw;
    info->fft_h = g.fft_h; info->fft_w = g.fft_w;
    info->transform_h = g.Lh; info->transform_w = g.Lw;
    info->spectrum_rows = g.rows; info->spectrum_pitch = g.s_pitch;
    info->gpu_id = plan->gpu_id;
    info->exact_window = g.exact_window ? 1 : 0;
    info->spectrum_bytes = g.spectrum_elems() * sizeof(c32);
    info->map_bytes = g.map_elems() * plan->elem_bytes();
    info->out_h = plan->map_h();      // (of the delivered map: the extent, sampled at the plan's strides)
    info->out_w = plan->map_w();
    info->out_map_bytes = plan->out_map_bytes();
    info->workspace_bytes = plan->A.bytes() + plan->Y.bytes() + plan->K.bytes() + plan->O.bytes() + plan->I.bytes() + plan->IT.bytes() + plan->IE.bytes() +
                            plan->ND.bytes() + plan->KN.bytes() + plan->KC.bytes() + plan->NS64.bytes() +      // (matching scores: all 0 until one is on)
                            plan->EXR.bytes() + plan->EXP.bytes() +                                            // (per-map extrema: likewise)
                            plan->PKF.bytes() + plan->PKS.bytes() + plan->PKR.bytes();                         // (peak lists: likewise)
    if (const TiledState* ts = plan->tiled) {     // block-wise: the window of the whole image; the spectrum is every block's
        info->spectrum_bytes = ts->spec_total() * sizeof(c32);
        info->map_bytes = ts->big_map() * sizeof(float);
        fftconv_plan_info si;
        if (fftconv_plan_get_info(ts->sub, &si) == 0)
            info->workspace_bytes = si.workspace_bytes + ts->big.bytes() + ts->tmp.bytes() + ts->blk.bytes() + ts->crop.bytes() + (ts->specs_x ? 0 : ts->specs.bytes());
    }
    return 0;
}

int fftconv_plan_convolve_packed(fftconv_plan* plan, int n_kernel, const float* kernels_device, int kernel_h,
                                 int kernel_w, float* out_device) {
    if (!plan || n_kernel < 0) return api_fail(FFTCONV_ERR_INVALID_ARG, "Wrong number of inputs");
    if (n_kernel == 0) return 0;
    if (!kernels_device || !out_device) return api_fail(FFTCONV_ERR_INVALID_ARG, "NULL kernel or output pointer");
    if (int rc = use_device(plan)) return rc;
    if (plan->tiled) {
        const size_t per = (size_t)plan->tiled->F * kernel_h * kernel_w;
        std::vector<const float*> kp(n_kernel);
        std::vector<int> khs(n_kernel, kernel_h), kws(n_kernel, kernel_w);
        for (int j = 0; j < n_kernel; j++) kp[j] = kernels_device + per * j;
        const int rc = tiled_convolve(plan, n_kernel, kp.data(), khs.data(), kws.data(), FFTCONV_DEVICE, nullptr, FFTCONV_DEVICE, out_device);
        // as fftconv_plan_convolve: nothing of a failed call may still be running when the error is returned
        if (rc) (void)keep_error([&] { return hipStreamSynchronize(plan->tiled->sub->stream); });
        return rc;
    }
    if (int rc = outputs_begin(plan, n_kernel)) return rc;
    Sink sink;
    sink.packed = out_device;
    const int rc = run_group(plan, n_kernel, kernels_device, kernel_h, kernel_w, sink);
    if (!rc) outputs_end(plan, n_kernel);
    return rc;
}

int fftconv_plan_prepare_kernels_packed(fftconv_plan* plan, int n_kernel, const float* kernels_device, int kernel_h,
                                        int kernel_w) {
    if (!plan || n_kernel < 0) return api_fail(FFTCONV_ERR_INVALID_ARG, "Wrong number of inputs");
    if (n_kernel == 0) return 0;
    if (!kernels_device) return api_fail(FFTCONV_ERR_INVALID_ARG, "NULL kernel pointer");
    if (plan->tiled) return 0;     // block-wise: the kernels are transformed per block inside convolve
    return prepare_kernels(plan, n_kernel, kernels_device, kernel_h, kernel_w, false);
}

int fftconv_plan_convolve(fftconv_plan* plan, int n_kernel, const float* const* kernels, const int* kernel_h,
                          const int* kernel_w, int kernel_location, float* const* out, int out_location) {
    if (!plan || n_kernel < 0) return api_fail(FFTCONV_ERR_INVALID_ARG, "Wrong number of inputs");
    if (n_kernel == 0) return 0;
    if (!kernels || !kernel_h || !kernel_w || !out) return api_fail(FFTCONV_ERR_INVALID_ARG, "Kernel must be a cell array");
    fftconv_plan* p = plan;
    const Geometry& g = p->g;
    if (int rc = use_device(p)) return rc;
    if (p->tiled) {
        const int rc = tiled_convolve(p, n_kernel, kernels, kernel_h, kernel_w, kernel_location, out, out_location, nullptr);
        if (rc) (void)keep_error([&] { return hipStreamSynchronize(p->tiled->sub->stream); });   // nothing may still be writing into the caller's buffers
        return rc;
    }
    if (!p->have_image()) return api_fail(FFTCONV_ERR_NO_IMAGE, "no image spectrum: call fftconv_plan_set_image first");
    // validate everything up front so nothing is launched on a bad cell (the reference fails
    // mid-loop and leaks: SURVEY D3)
    for (int k = 0; k < n_kernel; k++) {
        if (!kernels[k] || !out[k]) return api_fail(FFTCONV_ERR_INVALID_ARG, "kernel or output %d is NULL", k);
        if (int rc = check_kernel_size(p, kernel_h[k], kernel_w[k])) return rc;
    }
    // (a plan holding B images: out[] has B * n_kernel entries, image-major -- out[b * n_kernel + k] is image b (x) kernel k)
    for (long m = n_kernel; m < (long)n_kernel * p->images_held(); m++)
        if (!out[m]) return api_fail(FFTCONV_ERR_INVALID_ARG, "output %ld is NULL (the plan holds %d images: %ld maps)", m, p->n_images, (long)n_kernel * p->n_images);
    if (int rc = outputs_begin(p, n_kernel)) return rc;
    // groups of consecutive kernels of equal size
    for (int k0 = 0, k1; k0 < n_kernel; k0 = k1) {
        k1 = same_size_run_end(kernel_h, kernel_w, k0, n_kernel);
        const int n = k1 - k0, kh = kernel_h[k0], kw = kernel_w[k0];
        const size_t per = (size_t)g.F * kh * kw;
        const float* dk = nullptr;
        const bool kernels_pinned = kernel_location == FFTCONV_HOST && p->opt_host_pinned && per * n * sizeof(float) <= FC_PIN_INPLACE_BYTES;
        if (kernels_pinned) {
            // a small set of host kernels: gathered by the CPU into the plan's pinned buffer and read there, in place, by
            // the kernels' column pass (one pass over them) -- no copy command, against one blocking copy per kernel
            if (int rc = p->pin_k.ensure(per * n * sizeof(float))) return rc;
            if (int rc = p->pin_k.wait()) return rc;
            for (int j = 0; j < n; j++) memcpy(p->pin_k.p + per * j * sizeof(float), kernels[k0 + j], per * sizeof(float));
            dk = reinterpret_cast<const float*>(p->pin_k.p);
            p->a_holds.source_overwritten(dk);      // column spectra, or a request, of the buffer's previous contents
        } else {
            if (int rc = p->K.ensure(per * n)) return rc;
            for (int j = 0; j < n; j++)
                HIP_TRY(hipMemcpyAsync(p->K.p + per * j, kernels[k0 + j], per * sizeof(float), copy_kind(kernel_location, true), p->stream));
            dk = p->K.p;
        }
        Sink sink;
        sink.ptrs = out + k0;
        sink.location = out_location;
        sink.image_stride = n_kernel;
        sink.map0 = k0;
        const int rcg = run_group(p, n, dk, kh, kw, sink);
        if (kernels_pinned) {      // (whatever the group's outcome: the launches that read the buffer are in the stream)
            if (rcg) (void)keep_error([&] { return p->pin_k.mark(p->stream); });
            else if (int rcm = p->pin_k.mark(p->stream)) return rcm;
        }
        if (rcg) return rcg;
    }
    if (out_location == FFTCONV_HOST) HIP_TRY(hipStreamSynchronize(p->stream));
    outputs_end(p, n_kernel);
    return 0;
}

int fftconv_plan_set_stream(fftconv_plan* plan, void* hip_stream) {
    if (!plan) return api_fail(FFTCONV_ERR_INVALID_ARG, "plan is NULL");
    // (profile events already recorded stay valid: they are read later by fftconv_plan_get_profile,
    //  whichever stream they were recorded on -- collecting them here would block the host)
    // (prepared column spectra stay: they count again once the plan is back on the stream they were produced on --
    //  the image transform of the multi-GPU step borrows the plan for a side stream and hands it back; a DEFERRED
    //  preparation is launched now, on the stream it was asked for)
    if (!plan->tiled && plan->a_holds.pending()) {
        if (int rc = use_device(plan)) return rc;
        if (int rc = flush_pending_prepare(plan)) return rc;
    }
    plan->stream = reinterpret_cast<hipStream_t>(hip_stream);
    if (plan->tiled) return fftconv_plan_set_stream(plan->tiled->sub, hip_stream);
    return 0;
}

int fftconv_plan_synchronize(fftconv_plan* plan) {
    if (!plan) return api_fail(FFTCONV_ERR_INVALID_ARG, "plan is NULL");
    if (int rc = use_device(plan)) return rc;
    if (!plan->tiled)
        if (int rc = flush_pending_prepare(plan)) return rc;
    HIP_TRY(hipStreamSynchronize(plan->stream));
    return 0;
}

int fftconv_plan_set_option(fftconv_plan* plan, const char* name, long value) {
    if (!plan || !name) return api_fail(FFTCONV_ERR_INVALID_ARG, "NULL argument");
    if (!strcmp(name, "map_format"))
        if (const char* why = map_format_error(value, plan->tiled != nullptr)) return api_fail(FFTCONV_ERR_INVALID_ARG, "%s", why);
    const LongOption* o = find_option(name);
    if (plan->tiled && !(o && (o->flags & OPT_OWN))) {      // block-wise: options act on the block plan (OPT_OWN: on this one, below)
        if (!strcmp(name, "verbose")) plan->opt_verbose = value != 0;
        return fftconv_plan_set_option(plan->tiled->sub, name, value);
    }
    if (o && !(o->flags & OPT_GET_ONLY)) {
        if ((o->flags & OPT_REJECT) && (value < o->lo || value > o->hi)) return api_fail(FFTCONV_ERR_INVALID_ARG, "option '%s' out of range", name);
        if (int rc = apply_effects(plan, o->effects)) return rc;
        if (o->member == &fftconv_plan::opt_host_stream && value > 2) return api_fail(FFTCONV_ERR_INVALID_ARG, "host_stream is 0, 1 or 2");
        plan->*(o->member) = (o->flags & OPT_BOOL) ? (value != 0) : std::min(std::max(value, o->lo), o->hi);
        return 0;
    }
    if (!strcmp(name, "profile")) {
        if (value != 0 && plan->a_holds.pending() && (plan->profile_mask & ((1u << PK_KERNEL_COLS) | (1u << PK_IMAGE_COLS)))) {   // per-kind figures: the kernels' column pass is timed as a launch of its own
            if (int rc = use_device(plan)) return rc;
            if (int rc = flush_pending_prepare(plan)) return rc;
        }
        plan->profile = value != 0;
        return 0;
    }
    if (!strcmp(name, "dynamic_tiles")) {
        // 1: the persistent output kernel takes its tiles from a queue in device memory (fast_cols.hpp: TileQueue; the default
        // from M = 432 on) instead of a fixed share per workgroup (0); 2: the forward column kernels (image, kernels) too.  A step
        // that shares the GPU with another kernel -- the broadcast of a multi-GPU run, another library's work -- loses half as much
        // with the queue.
        if (value < 0 || value > 2) return api_fail(FFTCONV_ERR_INVALID_ARG, "dynamic_tiles is 0, 1 or 2");
        if (value && !plan->g.fast_cols.ok) value = 0;      // (generic kernels: one workgroup per tile, dealt by the hardware)
        if (value && !plan->queue.p) {     // zeroed once: every launch leaves the counters at zero (fast_cols.hpp: queue_leave)
            if (int rc = use_device(plan)) return rc;
            if (int rc = plan->queue.ensure(FC_QUEUE_WORDS)) return rc;
            HIP_TRY(hipMemset(plan->queue.p, 0, FC_QUEUE_WORDS * sizeof(int)));
        }
        plan->opt_dynamic_tiles = value;
        plan->d.queue = value ? plan->queue.p : nullptr;
        plan->d.queue_fwd = value == 2;
        return 0;
    }
    if (!strcmp(name, "defer_prepare")) {
        if (!value && plan->a_holds.pending()) {
            if (int rc = use_device(plan)) return rc;
            if (int rc = flush_pending_prepare(plan)) return rc;
        }
        plan->opt_defer_prepare = value != 0;
        return 0;
    }
    if (!strcmp(name, "profile_kinds")) { plan->profile_mask = value <= 0 ? ~0u : (unsigned)value; return 0; }
    if (!strcmp(name, "rows_group")) { plan->g.rows_group = value <= 0 ? -1 : (int)value; return 0; }
#if FC_ROWS_TIMELINE || FC_COLS_TIMELINE
    // diagnostic builds only (tools/rows_timeline.py, tools/cols_timeline.py): device buffer one workgroup stamps
    if (!strcmp(name, "timeline_ptr")) { plan->d.timeline = reinterpret_cast<unsigned long long*>((uintptr_t)value); return 0; }
#endif
    if (!strcmp(name, "output_region")) {
        const Geometry& g = plan->g;
        int oh = g.fft_h, ow = g.fft_w, fh = 0, fw = 0;
        if (value == 1) { oh = g.H + g.max_kh - 1; ow = g.W + g.max_kw - 1; }
        else if (value == 2) { oh = g.H; ow = g.W; fh = (g.max_kh - 1) / 2; fw = (g.max_kw - 1) / 2; }
        else if (value == 3) { oh = g.H - g.max_kh + 1; ow = g.W - g.max_kw + 1; fh = g.max_kh - 1; fw = g.max_kw - 1; }
        else if (value == 4) { oh = fft_size_pow2(g.H + g.max_kh - 1); ow = fft_size_pow2(g.W + g.max_kw - 1); }
        else if (value == 5) return api_fail(FFTCONV_ERR_INVALID_ARG, "output_region 5 (a rectangle of the window) is set with fftconv_plan_set_output_rect");
        else if (value != 0) return api_fail(FFTCONV_ERR_INVALID_ARG, "output_region is 0 (window), 1 (full), 2 (same), 3 (valid) or 4 (pow2 window)");
        if (const char* why = output_stride_error(plan->stride_h, plan->stride_w, value)) return api_fail(FFTCONV_ERR_INVALID_ARG, "%s", why);
        if (oh < 1 || ow < 1) return api_fail(FFTCONV_ERR_INVALID_ARG, "output_region %ld is empty for %dx%d data and %dx%d kernels", value, g.H, g.W, g.max_kh, g.max_kw);
        int rc;
        if (setter_done(plan, Setter::OutputRegion, plan->opt_region == value, rc)) return rc;
        // (block-wise plans: g is the whole image's geometry; the blocks keep storing full-window maps and the region is cropped
        //  out of them on delivery, blockwise.cpp: tiled_deliver)
        plan->opt_region = value; plan->out_h = oh; plan->out_w = ow; plan->off_h = fh; plan->off_w = fw;
        return 0;
    }
    return api_fail(FFTCONV_ERR_INVALID_ARG, "unknown option '%s'", name);
}

int fftconv_plan_set_output_rect(fftconv_plan* plan, int off_h, int off_w, int out_h, int out_w) {
    if (!plan) return api_fail(FFTCONV_ERR_INVALID_ARG, "plan is NULL");
    const Geometry& g = plan->g;      // (block-wise plans: the whole image's window)
    if (const char* why = output_rect_error(off_h, off_w, out_h, out_w, g.fft_h, g.fft_w))
        return api_fail(FFTCONV_ERR_INVALID_ARG, "%s (rows [%d, %d) of columns [%d, %d) asked of the %d x %d window)", why, off_h, off_h + out_h, off_w,
                        off_w + out_w, g.fft_h, g.fft_w);
    const bool same = plan->opt_region == 5 && plan->out_h == out_h && plan->out_w == out_w && plan->off_h == off_h && plan->off_w == off_w;
    int rc;
    if (setter_done(plan, Setter::OutputRect, same, rc)) return rc;
    plan->opt_region = 5; plan->out_h = out_h; plan->out_w = out_w; plan->off_h = off_h; plan->off_w = off_w;
    return 0;
}

int fftconv_plan_set_output_stride(fftconv_plan* plan, int stride_h, int stride_w) {
    if (!plan) return api_fail(FFTCONV_ERR_INVALID_ARG, "plan is NULL");
    if (const char* why = output_stride_error(stride_h, stride_w, plan->opt_region))
        return api_fail(FFTCONV_ERR_INVALID_ARG, "%s (strides (%d, %d) asked of a plan with output_region %ld)", why, stride_h, stride_w, plan->opt_region);
    int rc;
    if (setter_done(plan, Setter::OutputStride, plan->stride_h == stride_h && plan->stride_w == stride_w, rc)) return rc;
    // (output-side state alone: the image, the prepared kernels and the extent stay)
    plan->stride_h = stride_h; plan->stride_w = stride_w;
    return 0;
}

int fftconv_plan_set_extrema(fftconv_plan* plan, int mode, int max_maps) {
    if (!plan) return api_fail(FFTCONV_ERR_INVALID_ARG, "plan is NULL");
    if (mode != 0 && mode != 1) return api_fail(FFTCONV_ERR_INVALID_ARG, "per-map extrema: mode is 0 (off) or 1 (on), not %d", mode);
    if (mode == 1 && max_maps < 1) return api_fail(FFTCONV_ERR_INVALID_ARG, "per-map extrema: max_maps must be at least 1 (%d asked)", max_maps);
    if (int rc = plan_refused(plan, AskOutput::Extrema, mode)) return rc;
    if (mode == 0) max_maps = 0;
    int rc;
    if (setter_done(plan, SetterAdded::Extrema, plan->extrema_max_maps == max_maps, rc)) return rc;
    // (output-side state alone: the image, the prepared kernels, the stream and the extent stay)
    plan->EXR.release(); plan->EXP.release();
    plan->extrema_max_maps = plan->extrema_slots = plan->extrema_launch_maps = 0;
    plan->extrema_maps = -1;
    if (mode == 0) return 0;
    // the partials of one launch: per map the fused store's slots for the whole window (a rectangle has fewer tiles) or the scan's
    // blocks, whichever is more; the maps of a launch as batch_sizes bounds them
    const Geometry& g = plan->g;
    int slots = FC_EXTREMA_SCAN_MAX_BLOCKS;
    if (g.fast_cols.ok) slots = std::max(slots, tiles_for(g.fft_w, g.fast_cols.T) * (g.fast_cols.NT / 64));
    const int launch_maps = (int)std::min<long>(max_maps, plan->opt_batch_maps > 0 ? plan->opt_batch_maps : 64);
    if (int rce = plan->EXR.ensure((size_t)max_maps)) return rce;
    if (int rce = plan->EXP.ensure((size_t)slots * launch_maps)) { plan->EXR.release(); return rce; }
    plan->extrema_max_maps = max_maps; plan->extrema_slots = slots; plan->extrema_launch_maps = launch_maps;
    return 0;
}

int fftconv_plan_get_extrema(fftconv_plan* plan, int first_map, int n_maps, fftconv_extrema* out_host) {
    if (!plan || !out_host) return api_fail(FFTCONV_ERR_INVALID_ARG, "NULL argument");
    if (!plan->extrema_on()) return api_fail(FFTCONV_ERR_INVALID_ARG, "per-map extrema are off (fftconv_plan_set_extrema)");
    if (plan->extrema_maps < 0) return api_fail(FFTCONV_ERR_INVALID_ARG, "per-map extrema: no convolve has run since fftconv_plan_set_extrema");
    if (first_map < 0 || n_maps < 0 || (long)first_map + n_maps > plan->extrema_maps)
        return api_fail(FFTCONV_ERR_INVALID_ARG, "per-map extrema: records [%d, %d) asked, the last convolve wrote %d", first_map, first_map + n_maps, plan->extrema_maps);
    if (n_maps == 0) return 0;
    if (int rc = use_device(plan)) return rc;
    static_assert(sizeof(fftconv_extrema) == sizeof(ExtremaRecord), "the record the kernels write is the caller's");
    HIP_TRY(hipMemcpyAsync(out_host, plan->EXR.p + first_map, (size_t)n_maps * sizeof(ExtremaRecord), hipMemcpyDeviceToHost, plan->stream));
    HIP_TRY(hipStreamSynchronize(plan->stream));
    return 0;
}

int fftconv_plan_extrema_device(fftconv_plan* plan, void** device_ptr, size_t* bytes) {
    if (!plan || !device_ptr || !bytes) return api_fail(FFTCONV_ERR_INVALID_ARG, "NULL argument");
    if (!plan->extrema_on()) return api_fail(FFTCONV_ERR_INVALID_ARG, "per-map extrema are off (fftconv_plan_set_extrema)");
    *device_ptr = plan->EXR.p;
    *bytes = (size_t)plan->extrema_max_maps * sizeof(ExtremaRecord);
    return 0;
}

int fftconv_plan_set_peaks(fftconv_plan* plan, int mode, int max_maps, int max_peaks, float threshold, int radius_h, int radius_w) {
    if (!plan) return api_fail(FFTCONV_ERR_INVALID_ARG, "plan is NULL");
    if (mode < FC_PEAKS_OFF || mode > FC_PEAKS_MIN) return api_fail(FFTCONV_ERR_INVALID_ARG, "peak lists: mode is 0 (off), 1 (maxima) or 2 (minima), not %d", mode);
    if (mode != FC_PEAKS_OFF) {
        if (max_maps < 1) return api_fail(FFTCONV_ERR_INVALID_ARG, "peak lists: max_maps must be at least 1 (%d asked)", max_maps);
        if (max_peaks < 1) return api_fail(FFTCONV_ERR_INVALID_ARG, "peak lists: max_peaks must be at least 1 (%d asked)", max_peaks);
        if (threshold != threshold) return api_fail(FFTCONV_ERR_INVALID_ARG, "peak lists: the threshold is NaN (-inf takes every element)");
        if (radius_h < 0 || radius_w < 0) return api_fail(FFTCONV_ERR_INVALID_ARG, "peak lists: a radius cannot be negative (%d, %d asked)", radius_h, radius_w);
    }
    if (int rc = plan_refused(plan, AskPeaks::Peaks, mode)) return rc;
    if (mode == FC_PEAKS_OFF) { max_maps = max_peaks = radius_h = radius_w = 0; threshold = 0.0f; }
    const bool same_size = plan->peaks_max_maps == max_maps && plan->peaks_max == max_peaks;
    // (bits, not ==: a threshold of -0 after +0 is a change like any other)
    const bool same_rule = plan->peaks_mode == mode && fc_float_bits(plan->peaks_threshold) == fc_float_bits(threshold) && plan->peaks_radius_h == radius_h &&
                           plan->peaks_radius_w == radius_w;
    int rc;
    if (setter_done(plan, SetterPeaks::Peaks, same_size && same_rule, rc)) return rc;
    // (output-side state alone: the image, the prepared kernels, the stream and the extent stay)
    if (!same_size) {      // threshold, radius or mode alone: uniforms of the launches, the buffers stay
        plan->PKF.release(); plan->PKS.release(); plan->PKR.release();
        plan->peaks_mode = plan->peaks_max_maps = plan->peaks_max = plan->peaks_launch_maps = 0;
        plan->peaks_maps = -1;
        if (mode != FC_PEAKS_OFF) {
            // the scratch of one launch: the maps of a launch as fftconv_plan_set_extrema bounds them, the units of the largest map
            const int launch_maps = (int)std::min<long>(max_maps, plan->opt_batch_maps > 0 ? plan->opt_batch_maps : 64);
            int rce = plan->PKF.ensure((size_t)max_maps);
            if (!rce) rce = plan->PKR.ensure((size_t)max_maps * (size_t)max_peaks);
            if (!rce) rce = plan->PKS.ensure((size_t)2 * FC_PEAKS_MAX_UNITS * launch_maps);
            if (rce) { plan->PKF.release(); plan->PKS.release(); plan->PKR.release(); return rce; }
            plan->peaks_max_maps = max_maps; plan->peaks_max = max_peaks; plan->peaks_launch_maps = launch_maps;
        }
    }
    if (!same_rule) plan->peaks_maps = -1;      // (the lists of the last convolve belong to the rule it ran under)
    plan->peaks_mode = mode; plan->peaks_threshold = threshold; plan->peaks_radius_h = radius_h; plan->peaks_radius_w = radius_w;
    return 0;
}

int fftconv_plan_get_peaks(fftconv_plan* plan, int first_map, int n_maps, int* found_host, fftconv_peak* peaks_host) {
    if (!plan || !found_host || !peaks_host) return api_fail(FFTCONV_ERR_INVALID_ARG, "NULL argument");
    if (!plan->peaks_on()) return api_fail(FFTCONV_ERR_INVALID_ARG, "peak lists are off (fftconv_plan_set_peaks)");
    if (plan->peaks_maps < 0) return api_fail(FFTCONV_ERR_INVALID_ARG, "peak lists: no convolve has run since fftconv_plan_set_peaks");
    if (first_map < 0 || n_maps < 0 || (long)first_map + n_maps > plan->peaks_maps)
        return api_fail(FFTCONV_ERR_INVALID_ARG, "peak lists: maps [%d, %d) asked, the last convolve wrote %d", first_map, first_map + n_maps, plan->peaks_maps);
    if (n_maps == 0) return 0;
    if (int rc = use_device(plan)) return rc;
    static_assert(sizeof(fftconv_peak) == sizeof(PeakRecord) && sizeof(PeakRecord) == 20, "the record the kernels write is the caller's");
    HIP_TRY(hipMemcpyAsync(found_host, plan->PKF.p + first_map, (size_t)n_maps * sizeof(int), hipMemcpyDeviceToHost, plan->stream));
    HIP_TRY(hipMemcpyAsync(peaks_host, plan->PKR.p + (size_t)first_map * plan->peaks_max, (size_t)n_maps * plan->peaks_max * sizeof(PeakRecord), hipMemcpyDeviceToHost,
                           plan->stream));
    HIP_TRY(hipStreamSynchronize(plan->stream));
    return 0;
}

int fftconv_plan_peaks_device(fftconv_plan* plan, void** found_device, void** peaks_device, size_t* peaks_bytes) {
    if (!plan || !found_device || !peaks_device || !peaks_bytes) return api_fail(FFTCONV_ERR_INVALID_ARG, "NULL argument");
    if (!plan->peaks_on()) return api_fail(FFTCONV_ERR_INVALID_ARG, "peak lists are off (fftconv_plan_set_peaks)");
    *found_device = plan->PKF.p;
    *peaks_device = plan->PKR.p;
    *peaks_bytes = (size_t)plan->peaks_max_maps * plan->peaks_max * sizeof(PeakRecord);
    return 0;
}

// fftconv_plan_set_normalisation and fftconv_plan_set_match_score behind their argument checks: one state, one set of rules
static int set_score(fftconv_plan* plan, int score, int box_h, int box_w) {
    if (int rc = plan_refused(plan, Ask::Score, score)) return rc;
    if (score == 0) box_h = box_w = 0;
    // (a change: the kernel column spectra are those of the prepared kernels, or not; the plane belongs to (image, score, box) and the pixels are gone)
    int rc;
    if (setter_done(plan, Setter::Score, plan->opt_score == score && plan->norm_box_h == box_h && plan->norm_box_w == box_w, rc)) return rc;
    plan->opt_score = score; plan->norm_box_h = box_h; plan->norm_box_w = box_w;
    return 0;
}

int fftconv_plan_set_normalisation(fftconv_plan* plan, int mode, int box_h, int box_w) {
    if (!plan) return api_fail(FFTCONV_ERR_INVALID_ARG, "plan is NULL");
    const Geometry& g = plan->g;
    if (const char* why = ncc_args_error(mode, box_h, box_w, g.max_kh, g.max_kw))
        return api_fail(FFTCONV_ERR_INVALID_ARG, "%s (mode %d, box %d x %d asked of a plan with MAX_KERNEL %d x %d)", why, mode, box_h, box_w, g.max_kh, g.max_kw);
    return set_score(plan, mode, box_h, box_w);
}

int fftconv_plan_set_match_score(fftconv_plan* plan, int score, int box_h, int box_w) {
    if (!plan) return api_fail(FFTCONV_ERR_INVALID_ARG, "plan is NULL");
    const Geometry& g = plan->g;
    if (const char* why = score_args_error(score, box_h, box_w, g.max_kh, g.max_kw))
        return api_fail(FFTCONV_ERR_INVALID_ARG, "%s (score %d, box %d x %d asked of a plan with MAX_KERNEL %d x %d)", why, score, box_h, box_w, g.max_kh, g.max_kw);
    return set_score(plan, score, box_h, box_w);
}

int fftconv_plan_set_border(fftconv_plan* plan, int mode, float value) {
    if (!plan) return api_fail(FFTCONV_ERR_INVALID_ARG, "plan is NULL");
    const Geometry& g = plan->g;
    if (const char* why = border_args_error(mode, value, g.H, g.W, g.max_kh, g.max_kw))
        return api_fail(FFTCONV_ERR_INVALID_ARG, "%s (mode %d, value %g asked of a plan with DATA %d x %d and MAX_KERNEL %d x %d)", why, mode, (double)value, g.H,
                        g.W, g.max_kh, g.max_kw);
    if (int rc = plan_refused(plan, Ask::Border, mode)) return rc;
    if (mode != FC_BORDER_CONSTANT) value = 0.f;
    // (nothing changes: the image and the rectangle stay; a change: the spectrum belongs to (image, border))
    int rc;
    if (setter_done(plan, Setter::Border, plan->border_mode == mode && plan->border_value == value, rc)) return rc;
    plan->border_mode = mode; plan->border_value = value;
    if (mode) {      // the H x W "same" map anchored on the MAX_KERNEL box: the part of the window the cyclic wrap does not reach
        plan->opt_region = 5; plan->out_h = g.H; plan->out_w = g.W; plan->off_h = g.max_kh - 1; plan->off_w = g.max_kw - 1;
    } else {
        plan->opt_region = 0; plan->out_h = g.fft_h; plan->out_w = g.fft_w; plan->off_h = 0; plan->off_w = 0;
    }
    return 0;
}

int fftconv_plan_set_spectral_filter(fftconv_plan* plan, int mode, float param) {
    if (!plan) return api_fail(FFTCONV_ERR_INVALID_ARG, "plan is NULL");
    if (const char* why = spectral_filter_args_error(mode, param))
        return api_fail(FFTCONV_ERR_INVALID_ARG, "%s (mode %d, param %g)", why, mode, (double)param);
    if (int rc = plan_refused(plan, Ask::Filter, mode)) return rc;
    if (mode != FC_FILTER_WIENER) param = 0.f;
    // (state of the spectral-row launches alone: the image, the prepared kernels, the stream and the output side stay; nothing to wait for)
    int rc;
    if (setter_done(plan, Setter::Filter, plan->opt_filter == mode && plan->filter_lambda == param, rc)) return rc;
    plan->opt_filter = mode; plan->filter_lambda = param;
    return 0;
}

int fftconv_plan_get_option(fftconv_plan* plan, const char* name, long* value) {
    if (!plan || !name || !value) return api_fail(FFTCONV_ERR_INVALID_ARG, "null argument");
    const ComputedOption* c = nullptr;
    for (const ComputedOption& k : kComputedOptions)
        if (!strcmp(name, k.name)) { c = &k; break; }
    const LongOption* o = c ? nullptr : find_option(name);
    if (plan->tiled && !(c ? c->own : o && (o->flags & OPT_OWN))) return fftconv_plan_get_option(plan->tiled->sub, name, value);
    if (c) { *value = c->get(plan); return 0; }
    if (o && !(o->flags & OPT_SET_ONLY)) { *value = plan->*(o->member); return 0; }
    return api_fail(FFTCONV_ERR_INVALID_ARG, "unknown option '%s'", name);
}

int fftconv_plan_get_profile(fftconv_plan* plan, fftconv_profile* prof, int reset) {
    if (!plan || !prof) return api_fail(FFTCONV_ERR_INVALID_ARG, "NULL argument");
    if (plan->tiled) return fftconv_plan_get_profile(plan->tiled->sub, prof, reset);
    if (int rc = use_device(plan)) return rc;
    if (int rc = plan->prof_collect()) return rc;
    for (int i = 0; i < PK_COUNT; i++) {
        prof->ms[i] = plan->prof_ms[i];
        prof->launches[i] = plan->prof_launches[i];
        prof->units[i] = plan->prof_units[i];
        if (reset) { plan->prof_ms[i] = 0; plan->prof_launches[i] = 0; plan->prof_units[i] = 0; }
    }
    return 0;
}

int fftconv_fft_data(const float* data, int data_h, int data_w, int feature_dim, int kernel_h, int kernel_w, int gpu_id,
                     fftconv_plan** fft_data) {
    if (!fft_data) return api_fail(FFTCONV_ERR_INVALID_ARG, "Invalid input to MEX file.");
    *fft_data = nullptr;
    if (!data) return api_fail(FFTCONV_ERR_INVALID_ARG, "Invalid input to MEX file.");  // src/cudaFFTData.cu:49-54
    fftconv_plan* p = nullptr;
    if (int rc = fftconv_plan_create(&p, data_h, data_w, feature_dim, kernel_h, kernel_w, gpu_id, nullptr)) return rc;
    if (int rc = fftconv_plan_set_image(p, data, FFTCONV_HOST)) {
        (void)keep_error([&] { return fftconv_plan_destroy(p); });
        return rc;
    }
    *fft_data = p;
    return 0;
}

int fftconv_conv_fft_data(fftconv_plan* fft_data, int n_kernel, const float* const* kernels, const int* kernel_h,
                          const int* kernel_w, const int* kernel_f, const double* thread_size, int n_thread_size,
                          float* const* out) {
    if (!fft_data || !fftconv_plan_is_live(fft_data)) return api_fail(FFTCONV_ERR_INVALID_ARG, "Invalid input to MEX file.");  // src/cudaConvFFTData.cu:68
    if (int rc = check_thread_size(thread_size, n_thread_size)) return rc;
    if (kernel_f)
        for (int k = 0; k < n_kernel; k++)
            if (kernel_f[k] != fft_data->g.F)
                return api_fail(FFTCONV_ERR_KERNEL_SHAPE,
                            "Kernel and Data must have the same number of features and kernel size should be smaller than data size");
    return fftconv_plan_convolve(fft_data, n_kernel, kernels, kernel_h, kernel_w, FFTCONV_AUTO, out, FFTCONV_HOST);
}

}  // extern "C"
