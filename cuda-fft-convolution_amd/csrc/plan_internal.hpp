// plan_internal.hpp -- what the host translation units of libfftconv.so share (not installed): the plan object behind
// include/fftconv.h, its device / pinned buffers, and the internal entry points each unit offers the others.
//   column_cache.hpp   what the column-spectrum buffer A holds between calls (KernelSet, ColumnCache): the one owner of that record
//   image_route.hpp    the way of an image into a one-pass plan, decided once per call (ImageRoute, plan_image_route)
//   output_route.hpp   the way of a group's maps out of a plan, decided once per group (OutputRoute, plan_output_route)
//   plan_rules.hpp     which setter is refused while which state holds, and what a changed value invalidates (kPlanRules, kSetterEffects)
//   fftconv_api.cpp    plan core: creation (plan_device_setup), the per-kernel loop (run_group: launch_kernel_cols,
//                      launch_spectral_rows_batch, then the output stages), kernel preparation (prepare_kernels),
//                      options (kLongOptions), two-step pair
//   plan_output.cpp    output side of the plan core: plan_delivery (the OutputRoute and its buffers) and the stages that read it --
//                      launch_output_cols, launch_region, deliver_batch
//   plan_image.cpp     image side of the plan core: set_image / set_images / set_images_typed as a sequence of stages that read the
//                      ImageRoute, the spectrum buffer and the spectrum exchange in the reference's order
//   plan_cache.cpp     plan cache of the one-shot entries + fftconv_convolution_fft[_ex] (the MEX body)
//   host_ring.cpp      host-output streaming (copy threads, pinned ring, the two staging buffers of a streamed group)
//   blockwise.cpp      block-wise plans (overlap-save / overlap-add) and their planner
//   placement.cpp      opt-in placement tuning of the intermediate
//   fftconv_multi.cpp  several GPUs from one process (public API + api_internal.hpp only)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fftconv.h"
#include "api_internal.hpp"
#include "column_cache.hpp"
#include "image_route.hpp"
#include "kernels.hpp"
#include "ncc.hpp"
#include "output_route.hpp"
#include "pipeline.hpp"
#include "plan_rules.hpp"

// default of plan option "norm_store": fused -- it beat the staged route beyond the spread of alternating runs at both geometries
// measured (cfg3's with 64 maps: 3.90 against 4.98 ms per convolve; cfg2's with 16: 107 against 125 us; profiles/ncc_ab.txt)
// (score 4's additive store by the same rule: 3.96 against 4.97 ms and 103 against 121 us; profiles/match_score_ab.txt)
constexpr long FC_NORM_STORE_DEFAULT = 1;
// default of plan option "pixel_store" (typed image pixels, fftconv_plan_set_images_typed): direct -- the conversion in the column
// kernel's load (profiles/pixel_format_ab.txt)
constexpr long FC_PIXEL_STORE_DEFAULT = 1;
// default of plan option "border_store" (border modes, fftconv_plan_set_border): direct -- the index map in the column kernel's
// load beat the staged extension beyond the spread of alternating runs at every shape measured (the device-resident set_images
// step: cfg5's 35.3 against 44.8 us, cfg3's 91.3 against 124.7, cfg1's x 64 32.4 against 44.2; profiles/border_ab.txt)
constexpr long FC_BORDER_STORE_DEFAULT = 1;
// default of plan option "extrema_store" (per-map extrema, fftconv_plan_set_extrema): fused -- the output kernel finds them in its store.
// It beat the scan beyond the spread of alternating runs at cfg3's geometry with 64 maps (raw maps 3.57 against 3.76 ms per convolve,
// score 1 4.42 against 4.59, score 4 4.40 against 4.59); at cfg2's with 16 it is level for raw maps (100 against 99 us) and ahead under
// a score (123 against 128, 116 against 123; profiles/extrema_ab.txt)
constexpr long FC_EXTREMA_STORE_DEFAULT = 1;
constexpr long FC_HOST_MIN_KB = 1024;   // default of plan option "host_min_kb" (0 reproduces the threaded path for small maps: tests)

#define HIP_TRY(call)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fc::api_fail(FFTCONV_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),    \
                                __FILE__, __LINE__);                                               \
    } while (0)

namespace fc {

// smallest fftconv_plan_options this library accepts: the struct as it was before `blockwise` was appended
constexpr size_t kOptionsMinSize = offsetof(fftconv_plan_options, exact_window) + sizeof(int);
inline bool options_no_blockwise(const fftconv_plan_options* o) {
    return o && o->struct_size >= offsetof(fftconv_plan_options, blockwise) + sizeof(int) && o->blockwise == 1;
}
inline bool options_verbose(const fftconv_plan_options* o) {
    return o && o->struct_size >= offsetof(fftconv_plan_options, verbose) + sizeof(int) && o->verbose != 0;
}
// (appended after `verbose`: a struct_size without the field means 0 = fp32 maps)
inline int options_map_format(const fftconv_plan_options* o) {
    return o && o->struct_size >= offsetof(fftconv_plan_options, map_format) + sizeof(int) ? o->map_format : 0;
}
inline PlanTuning tuning_from(const fftconv_plan_options* o) {
    PlanTuning t;
    if (!o || o->struct_size < kOptionsMinSize) return t;
    t.path_mode = o->kernel_path == 1 ? 0 : o->kernel_path == 2 ? 1 : 2;
    t.rows_group = o->rows_group <= 0 ? -1 : o->rows_group;
    t.max_transform = o->max_transform > 0 ? o->max_transform : 0;
    t.exact_window = o->exact_window != 0;
    return t;
}

// fn() is a cleanup on a failing path (a wait, a destroy): the thread's last-error text -- the failure's -- survives it
template <class Fn>
auto keep_error(Fn&& fn) {
    const std::string keep = api_last_error();
    auto r = fn();
    api_set_last_error(keep);
    return r;
}

// copy between the plan's device buffers and memory at `location` (FFTCONV_AUTO names kernels only: towards the device)
inline hipMemcpyKind copy_kind(int location, bool to_device) {
    if (location == FFTCONV_HOST) return to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    return to_device && location == FFTCONV_AUTO ? hipMemcpyDefault : hipMemcpyDeviceToDevice;
}

// end of the run of consecutive kernels that have the size of kernel k0
inline int same_size_run_end(const int* kh, const int* kw, int k0, int n) {
    int k1 = k0 + 1;
    while (k1 < n && kh[k1] == kh[k0] && kw[k1] == kw[k0]) k1++;
    return k1;
}

// plan_cache.cpp: destroys every idle plan of the one-shot entries' cache (device scratch, pinned staging, copy threads);
// true if there was one.  Called by DevBuf::ensure when the device is out of memory.
bool cache_release_idle();

enum { PK_KERNEL_COLS = 0, PK_SPECTRAL = 1, PK_OUT_COLS = 2, PK_IMAGE_COLS = 3, PK_IMAGE_ROWS = 4, PK_COUNT = 5 };

struct EventPair {
    hipEvent_t start, stop;
    int kind;
    long units;
};

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;  // elements
    bool fresh = false;   // (re)allocated since the flag was last cleared
    int ensure(size_t n) {
        if (n <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        fresh = true;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
        if (e != hipSuccess && cache_release_idle()) {
            // out of device memory while the one-shot entries' plan cache holds idle plans (up to 48 GiB of scratch): they go
            // first -- the reference's contract is "all device memory is released" between calls -- and the request is repeated
            (void)hipGetLastError();
            e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
        }
        if (e != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();
            return api_fail(FFTCONV_ERR_ALLOC, "hipMalloc of %zu bytes failed: %s", n * sizeof(T), hipGetErrorString(e));
        }
        cap = n;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    size_t bytes() const { return cap * sizeof(T); }
};

// sizes buf for a host table, copies the table and stores the device pointer where the kernels' arguments read it
template <class T>
int upload(DevBuf<T>& buf, const std::vector<T>& v, const T** slot = nullptr) {
    if (int rc = buf.ensure(v.size())) return rc;
    HIP_TRY(hipMemcpy(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    if (slot) *slot = buf.p;
    return 0;
}

// Pinned host staging of the small-call path (host arrays in / out of a few hundred KB: the sizes the reference's demo
// calls with).  A copy between pageable memory and the device is a blocking runtime call of 10-25 us whatever its size,
// and the reference's entry makes one per kernel and one per map (src/cudaConvolutionFFT.cu:148,231,286).  Here the
// CPU copies the caller's small arrays into / out of pinned buffers of the plan: an image or a kernel set of at most
// FC_PIN_INPLACE_BYTES is then read by the column kernels IN PLACE over PCIe (no copy command at all), a larger one
// (up to FC_PIN_IMAGE_BYTES) crosses in one asynchronous copy (both limits: image_route.hpp), and the maps of a launch come back
// in ONE copy (FC_PIN_OUT_BYTES, FC_PIN_ONE_MAP_BYTES: output_route.hpp).  `busy` is recorded behind the last GPU work that reads
// the buffer; the next fill waits for it.
struct PinBuf {
    char* p = nullptr;
    size_t cap = 0;
    hipEvent_t busy = nullptr;
    bool in_use = false;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        if (int rc = wait()) return rc;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        const size_t want = (bytes + 65535) & ~(size_t)65535;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), want, hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; return api_fail(FFTCONV_ERR_ALLOC, "hipHostMalloc of %zu bytes failed: %s", want, hipGetErrorString(e)); }
        cap = want;
        return 0;
    }
    int wait() {                      // until the GPU work that reads the buffer is over
        if (!in_use) return 0;
        in_use = false;
        hipError_t e = hipEventSynchronize(busy);
        if (e != hipSuccess) return api_fail(FFTCONV_ERR_HIP, "hipEventSynchronize failed: %s", hipGetErrorString(e));
        return 0;
    }
    int mark(hipStream_t s) {         // everything queued on s so far may read the buffer
        if (!busy) {
            hipError_t e = hipEventCreateWithFlags(&busy, hipEventDisableTiming);
            if (e != hipSuccess) { busy = nullptr; return api_fail(FFTCONV_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(e)); }
        }
        hipError_t e = hipEventRecord(busy, s);
        if (e != hipSuccess) return api_fail(FFTCONV_ERR_HIP, "hipEventRecord failed: %s", hipGetErrorString(e));
        in_use = true;
        return 0;
    }
    void release() {
        if (in_use && busy) (void)hipEventSynchronize(busy);
        in_use = false;
        if (busy) (void)hipEventDestroy(busy);
        busy = nullptr;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
    }
};

}  // namespace fc

#include "host_ring.hpp"

struct TiledState;
struct fftconv_plan;
namespace fc {
// what plan_output_route decides on for this plan as it stands and a sink of that kind (plan_output.cpp)
OutputRouteIn output_route_in(const fftconv_plan* p, SinkKind sink);
}

// Where the block plan of an overlap-save block-wise plan stores its maps (Sink::window, built per block by tiled_convolve_save): rows
// [h_lo, h_hi) of columns [w_first, w_first + ncols) of the block's circular result, row h of column w of map j at
// base + j * map_stride + w * pitch + h -- the block's rectangle of the full maps (base is offset accordingly).
struct OutWindow {
    float* base;
    size_t map_stride;
    int pitch, h_lo, h_hi, w_first, ncols;
};

using namespace fc;   // (host units only: this header is not installed)

struct fftconv_plan {
    TiledState* tiled = nullptr;   // block-wise plan: sizes beyond one LDS-resident pass, or large sizes that run faster in blocks (see TiledState)
    Geometry g;
    Tables t;
    DeviceTables d;
    int gpu_id = 0;
    hipStream_t stream = nullptr;
    // device copies of the Tables (fftconv_api.cpp: plan_device_setup; the natural-order pair: on first use)
    DevBuf<c32> tw_m, tw_w, fr_tw1, fr_tw2, fc_tw1, fc_tw2;
    DevBuf<PairEntry> pairs, fc_pairs;
    DevBuf<int> fr_map, fc_rowoff, fc_pair_row_of, nat_row_of, nat_col_of;
    DevBuf<c32> S;     // image spectrum (own buffer)
    c32* Sx = nullptr; // caller-owned spectrum buffer, if any
    size_t Sx_bytes = 0;   // ... and its size (fftconv_plan_use_spectrum_buffer)
    // Images the plan holds (fftconv_plan_set_images; set_image: 1; 0 before any image and after the spectrum was invalidated):
    // their spectra lie [b][f][row][s_pitch] in the spectrum buffer, g.spectrum_elems() apart
    int n_images = 0;
    bool have_image() const { return n_images >= 1; }
    int images_held() const { return n_images > 1 ? n_images : 1; }   // what the spectrum buffer is sized and reported for
    c32* spec() const { return Sx ? Sx : S.p; }   // S is allocated by the first use that needs it (ensure_spectrum)
    // (the own buffer grows on demand: a larger batch reallocates it, and its contents are then gone -- the callers write all of it)
    int ensure_spectrum(int images = 0) { return Sx ? 0 : S.ensure(g.spectrum_elems() * (size_t)(images > 0 ? images : images_held())); }
    DevBuf<c32> A;     // kernel column spectra of the current chunk
    DevBuf<c32> Y;     // intermediate of the current map batch
    DevBuf<float> K;   // packed kernels staged on the device
    DevBuf<float> KF;  // flipped copy of the current chunk of kernels ("flip_kernels")
    long opt_flip_kernels = 0;
    // "output_region": which part of the padded window a map holds (MAX_KERNEL sizes K):
    // 0 window FFT_H x FFT_W (the reference), 1 full (DATA + K - 1), 2 same (DATA, centred), 3 valid (DATA - K + 1)
    // 5: the caller's rectangle (fftconv_plan_set_output_rect): rows [off_h, off_h + out_h) of columns [off_w, off_w + out_w)
    long opt_region = 0;
    int out_h = 0, out_w = 0, off_h = 0, off_w = 0;
    // "rect_store" 1: the specialised output kernel stores the rectangle of region 5 itself (fast_cols.hpp: RECT) where it can --
    // OutStore::Rect; 0, and every plan it cannot serve: the window goes through the fp32 staging O and is cropped like regions 1-3
    // (output_route.hpp: a score with a plane takes the fused or the staged combination instead; score 2 is a kernel preparation
    //  and nothing else, its maps leave as raw maps do)
    long opt_rect_store = 1;
    // read-only option "rect_direct": the store of the route of a sink that is not a window
    bool rect_direct() const { return plan_output_route(output_route_in(this, SinkKind::Packed)).store == OutStore::Rect; }
    // "image_walk" 1: a spectral-row launch of more than one image runs the kernel that keeps the transformed KERNEL row in
    // registers and walks over images (fast_rows_images.hpp) where the plan has it -- image_walk_active(); 0 (default), and
    // every plan it cannot serve: the walk over kernels.  Nothing cached depends on it.  (It gives way to a spectral filter without
    // a refusal: one of the two silent interactions plan_rules.hpp lists beside its table.)
    long opt_image_walk = 0;
    bool image_walk_active() const {
        return opt_image_walk && !opt_filter && !tiled && g.F == 1 && g.path_mode != 0 && g.fast_rows.ok && fast_rows_images_available(g.Lw, g.max_kw);
    }
    // fftconv_plan_set_spectral_filter (spectral_filter.hpp): FC_FILTER_* of the pointwise operation of the spectral-row launches and
    // the Wiener filter's lambda.  State of the row launches alone: nothing cached depends on it, and it allocates nothing.  While
    // a mode is on the launches walk over kernels (the image walk has no filter form) -- on the specialised kernel's FILTER
    // instantiation (filter_fast(); read-only option "spectral_filter_fast") or behind the generic kernel's branch.
    long opt_filter = 0;
    float filter_lambda = 0.f;
    bool filter_fast() const { return opt_filter && !tiled && g.fast_rows.ok && fast_rows_filter_built(g.Lw); }
    // fftconv_plan_set_normalisation (ncc.hpp): 1 = the maps are zero-mean normalised cross-correlations over the box norm_box_h x
    // norm_box_w, the size of every kernel while it is on.  ND holds the scale plane D of every image the plan holds
    // ([b][fft_w][fft_h], written by set_image / set_images beside the forward transform), KN the normalised kernels T'' of the
    // chunk whose column spectra are in A -- the column pass reads them instead of the caller's -- NS64 the float64 scratch of both.
    // "norm_store" 1: the specialised output kernel multiplies by D itself ahead of its store (fast_cols.hpp: NORM) where it
    // can -- OutputRoute::fused: fp32 maps of the window or of a rectangle on a plan that has the kernel.  0, and everything else
    // (16-bit maps, "output_region" 1-4, generic / Bluestein / kernel_path 1 or 2 output kernels, configurations that are not
    // built): STAGED -- the output kernel stores the fp32 window into O as for a cropped region, and the crop / pad kernel
    // multiplies by D at the window coordinate on the way into the maps (kernels_ncc.hip).
    // fftconv_plan_set_match_score: ONE state for both entries -- opt_score is FC_SCORE_* (fc_common.hpp; 1 is the mode 1 above, which
    // fftconv_plan_set_normalisation sets), over the same box.  Every score != 0 prepares the kernels into KN; the scores with a
    // plane (1, 3, 4: score_has_plane) fill ND -- D, Dc = E^(-1/2) or Q = E -- and combine in the output kernel's store (1, 3: NORM,
    // 4: ADD) or in the staged crop, as described above.  KC: the constants c_k = (float) t2 of the kernels in KN, written with
    // them by the same launch (score 4 reads them), so they are found wherever KN's column spectra are.
    long opt_score = 0, norm_box_h = 0, norm_box_w = 0;
    long opt_norm_store = FC_NORM_STORE_DEFAULT;
    bool score_planes() const { return score_has_plane(opt_score); }
    // read-only option "norm_direct": whether the route of a sink that is not a window combines in the output kernel's store
    bool norm_direct() const { return plan_output_route(output_route_in(this, SinkKind::Packed)).fused(); }
    DevBuf<float> ND, KN, KC;
    DevBuf<double> NS64;
    DevBuf<float> OC;  // cropped maps staged for the copy-out
    // fftconv_plan_set_output_stride: the delivered map S holds every stride_h-th row and stride_w-th column of the extent U the plan
    // would deliver without it (the window, a region, the rectangle: ext_h x ext_w at off_h, off_w), counted from U's first row and
    // column -- map_h x map_w elements, dense.  Output-side state of its own: it keeps the image and the prepared kernels, and it
    // stays while the extent changes (out_h, out_w, off_h, off_w always describe U).  "stride_store" 1: the specialised output kernel
    // samples in its store where it can (fast_cols.hpp: STRIDE) -- OutStore::RectStride; 0, and every plan it cannot serve: the fp32
    // window goes through O and the crop samples it (output_route.hpp).
    int stride_h = 1, stride_w = 1;
    long opt_stride_store = 1;
    bool strided() const { return stride_h != 1 || stride_w != 1; }
    int ext_h() const { return opt_region ? out_h : g.fft_h; }
    int ext_w() const { return opt_region ? out_w : g.fft_w; }
    int map_h() const { return strided_count(ext_h(), stride_h); }
    int map_w() const { return strided_count(ext_w(), stride_w); }
    // read-only option "stride_direct": the store of the route of a sink that is not a window
    bool stride_direct() const { return plan_output_route(output_route_in(this, SinkKind::Packed)).store == OutStore::RectStride; }
    size_t out_elems() const {      // (block-wise plans: g holds the whole window)
        if (strided()) return (size_t)map_h() * map_w();
        return opt_region ? (size_t)out_h * out_w : g.map_elems();
    }
    // "map_format": element format of every result map (fc_common.hpp: FC_MAP_*; one-pass plans only).  The staging buffers O / OC
    // stay arrays of float that are sized in bytes and addressed through map_at; the full-window buffer a crop reads is always fp32.
    long opt_map_format = 0;
    size_t elem_bytes() const { return fc_map_elem_bytes((int)opt_map_format); }
    size_t out_map_bytes() const { return out_elems() * elem_bytes(); }
    // fftconv_plan_set_extrema (extrema.hpp): per-map extrema of the delivered maps.  extrema_max_maps > 0 while it is on: EXR holds that
    // many records (record m: delivered map m of the last convolve), EXP the partials of ONE output launch -- extrema_slots per map,
    // enough for the fused store of the whole window (its tiles x the waves of a workgroup) and for the scan's blocks of the largest
    // map the plan can deliver, times extrema_launch_maps, the maps of a launch ("batch_maps" as the setter found it, at most max_maps) --
    // both sized by the setter, never by a convolve.  extrema_maps: the maps of the last
    // convolve under it (-1: none yet).  "extrema_store" 1: the output kernel finds them in its store where it can (fast_cols.hpp: EXT)
    // -- OutExtrema::Fused; 0, and every route it cannot serve: the scan kernel reads the delivered maps (output_route.hpp).
    long opt_extrema_store = FC_EXTREMA_STORE_DEFAULT;
    int extrema_max_maps = 0, extrema_slots = 0, extrema_launch_maps = 0, extrema_maps = -1;
    DevBuf<ExtremaRecord> EXR;
    DevBuf<ExtremaPartial> EXP;
    bool extrema_on() const { return extrema_max_maps > 0; }
    // read-only option "extrema_direct": whether the route of a sink that is not a window finds them in the store
    bool extrema_direct() const { return plan_output_route(output_route_in(this, SinkKind::Packed)).extrema == OutExtrema::Fused; }
    // fftconv_plan_set_peaks (peaks.hpp): the thresholded local maxima of every delivered map.  peaks_mode != 0 while it is on: PKF holds
    // peaks_max_maps counts and PKR peaks_max_maps x peaks_max records (map m of the last convolve: found[m], and its first
    // min(found[m], peaks_max) peaks from m * peaks_max on), PKS the unit counts and offsets of ONE launch -- 2 x FC_PEAKS_MAX_UNITS ints
    // per map, times peaks_launch_maps, the maps of a launch as the extrema setter bounds them -- all sized by the setter, never by a
    // convolve.  Threshold, radii and mode are uniforms of the launches: changing them alone keeps the buffers.  peaks_maps: the maps of
    // the last convolve under it (-1: none yet).
    int peaks_mode = 0, peaks_max_maps = 0, peaks_max = 0, peaks_launch_maps = 0, peaks_radius_h = 0, peaks_radius_w = 0, peaks_maps = -1;
    float peaks_threshold = 0.0f;
    DevBuf<int> PKF, PKS;
    DevBuf<PeakRecord> PKR;
    bool peaks_on() const { return peaks_mode != 0; }
    DevBuf<float> O;   // output staging (pointer-array / host output)
    DevBuf<float> I;   // image staging (host input)
    // Typed image pixels (fftconv_plan_set_images_typed; pixel_format.hpp).  "pixel_store" 1: the image's forward column kernel
    // converts the elements in its load where it can -- pixel_direct(): a one-pass plan whose image column pass is the specialised
    // kernel and has the typed instantiation; 0, and every plan it cannot serve (generic / Bluestein column pass, configurations
    // that are not built, block-wise plans): STAGED -- a small kernel writes the fp32 image into I and the call goes on as an fp32
    // one.  It only chooses a route: nothing cached depends on it, and it takes effect at the next typed call.
    // pixel_format: FC_PIXEL_* of the images the plan holds (0 after every other way an image gets in; read with have_image()).
    long opt_pixel_store = FC_PIXEL_STORE_DEFAULT;
    long pixel_format = 0;
    // (a typed image while a border is on is converted into I first and takes the fp32 border route from there: never direct --
    //  the other silent interaction plan_rules.hpp lists beside its table)
    bool pixel_direct() const { return !border_mode && fast_cols_fwd_px_direct(opt_pixel_store != 0, tiled != nullptr, g.fast_fwd, g.M); }
    DevBuf<float> IT;  // typed pixels on the device: the H2D copy of a typed host image (sized in bytes: floats_for)
    // Border modes (fftconv_plan_set_border; border.hpp): FC_BORDER_* of what the image is beyond its data (0: zeros, the library
    // as it always was) and the CONSTANT mode's value.  While a mode is on, the forward pass transforms the image extended to
    // (H + MAX_KERNEL_H - 1) x (W + MAX_KERNEL_W - 1) and the plan's rectangle is the H x W "same" map (set by the call).
    // "border_store" 1: the image's forward column kernel maps the indices in its load where it can -- border_direct(): a one-pass
    // plan whose image column pass is the specialised kernel and has the bordered instantiation; 0, and every plan it cannot serve
    // (generic / Bluestein column pass, configurations that are not built): STAGED -- a small kernel writes the extended image
    // into IE and the column pass runs on that.  It only chooses a route: nothing cached depends on it.
    long border_mode = 0;
    float border_value = 0.f;
    long opt_border_store = FC_BORDER_STORE_DEFAULT;
    bool border_direct() const { return border_mode && fast_cols_fwd_border_direct(opt_border_store != 0, tiled != nullptr, g.fast_fwd, g.M); }
    int border_cols() const { return border_mode ? g.max_kw - 1 : 0; }
    DevBuf<float> IE;  // the extended image of the staged border route (its own buffer: I may hold the image the extension reads)
    PinBuf pin_img, pin_k, pin_out;   // pinned host staging of small host arrays (PinBuf above)
    hipEvent_t pin_out_done[2] = {nullptr, nullptr};   // copy into each half of pin_out complete
    long opt_host_pinned = 1;         // 0: small host arrays take the plain copies (A/B, tests)
    DevBuf<int> queue;                    // counters of the dynamic tile queue (option "dynamic_tiles"; allocated when it is first set)
    long opt_dynamic_tiles = 0;           // 1: the persistent output kernel takes its tiles from a queue (fast_cols.hpp: TileQueue); 2: the forward column kernels too
    DevBuf<c32> NS;                       // device staging of the natural-order spectrum exchange for host callers
    int num_cus = 256;
    long opt_batch_maps = 0;
    long opt_kernel_chunk_mb = 0;
    long tuned_candidates = 0, tuned_best = 0;   // of the last placement tuning (fftconv_plan_get_option)
    long opt_tune_placement = -1;  // > 1: that many candidate allocations of the intermediate are tried (placement.cpp); 0 / 1: never;
                                   // -1 (default): automatic -- placement_auto_candidates (placement.cpp)
    long opt_host_stream = 1;      // copy-out of host maps: 0 blocking, 1 direct by host threads, 2 pinned ring
    long opt_host_min_kb = FC_HOST_MIN_KB;   // maps smaller than this leave by blocking copies whatever host_stream says
    long opt_host_threads = 0;     // host copy threads of the output ring (0 = auto)
    long opt_host_chunk_kb = 0;    // ring chunk size (0 = auto)
    long opt_host_slots = 0;       // ring chunks (0 = auto)
    long opt_defer_prepare = 0;    // 1: fftconv_plan_prepare_kernels_packed only records its request (column_cache.hpp: Pending)
    long opt_verbose = 0;          // 1: per-stage sizes and launch shapes to stderr (the reference's `debug`, src/cudaConvolutionFFT.cu:9)
    HostRing* ring = nullptr;      // created on the first host-output convolve
    bool profile = false;
    unsigned profile_mask = ~0u;   // which kinds (bit = PK_* index) are timed while `profile` is on
    bool prof_open = false;        // the last prof_begin recorded a start event
    ColumnCache a_holds;           // what A holds: nothing known, a recorded preparation, or the first chunk's column spectra
    std::vector<EventPair> pending;
    std::vector<EventPair> pool;
    double prof_ms[PK_COUNT] = {0, 0, 0, 0, 0};
    long prof_launches[PK_COUNT] = {0, 0, 0, 0, 0};
    long prof_units[PK_COUNT] = {0, 0, 0, 0, 0};

    size_t cols_lds() const { return (size_t)g.T_cols * g.lds_pitch * sizeof(c32); }
    size_t rows_lds() const { return g.rows_lds_bytes(); }

    int prof_begin(int kind, long units) {
        prof_open = profile && ((profile_mask >> kind) & 1u);
        if (!prof_open) return 0;
        EventPair ep;
        if (!pool.empty()) {
            ep = pool.back();
            pool.pop_back();
        } else {
            HIP_TRY(hipEventCreate(&ep.start));
            HIP_TRY(hipEventCreate(&ep.stop));
        }
        ep.kind = kind;
        ep.units = units;
        HIP_TRY(hipEventRecord(ep.start, stream));
        pending.push_back(ep);
        return 0;
    }
    int prof_end() {
        if (!prof_open) return 0;
        prof_open = false;
        HIP_TRY(hipEventRecord(pending.back().stop, stream));
        return 0;
    }
    int prof_collect() {
        for (EventPair& ep : pending) {
            HIP_TRY(hipEventSynchronize(ep.stop));
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ep.start, ep.stop));
            prof_ms[ep.kind] += ms;
            prof_launches[ep.kind] += 1;
            prof_units[ep.kind] += ep.units;
            pool.push_back(ep);
        }
        pending.clear();
        return 0;
    }
    void release_ring() {
        if (ring) {
            ring->shutdown();
            delete ring;
            ring = nullptr;
        }
    }
    void release_all() {
        release_ring();
        for (EventPair& ep : pending) { (void)hipEventDestroy(ep.start); (void)hipEventDestroy(ep.stop); }
        for (EventPair& ep : pool) { (void)hipEventDestroy(ep.start); (void)hipEventDestroy(ep.stop); }
        pending.clear();
        pool.clear();
        tw_m.release(); tw_w.release(); pairs.release();
        S.release(); A.release(); Y.release(); K.release(); KF.release(); O.release(); OC.release(); I.release(); IT.release(); IE.release();
        fr_tw1.release(); fr_tw2.release(); fr_map.release();
        fc_tw1.release(); fc_tw2.release(); fc_pairs.release(); fc_rowoff.release(); fc_pair_row_of.release();
        nat_row_of.release(); nat_col_of.release(); NS.release(); queue.release();
        ND.release(); KN.release(); KC.release(); NS64.release(); EXR.release(); EXP.release(); PKF.release(); PKS.release(); PKR.release();
        pin_img.release(); pin_k.release(); pin_out.release();
        for (int h = 0; h < 2; h++) { if (pin_out_done[h]) (void)hipEventDestroy(pin_out_done[h]); pin_out_done[h] = nullptr; }
    }
};

namespace fc {

// the reference's debug prints (src/cudaConvolutionFFT.cu:60,68,100,114,240,258), behind plan option "verbose"
#define FC_VERBOSE(p, ...) do { if ((p)->opt_verbose) { fprintf(stderr, "fftconv: " __VA_ARGS__); fputc('\n', stderr); } } while (0)

// element `elems` of a map buffer whose elements are `elem_bytes` wide (the `float*` of a 16-bit map buffer is opaque)
inline float* map_at(float* base, size_t elems, size_t elem_bytes) {
    return reinterpret_cast<float*>(reinterpret_cast<char*>(base) + elems * elem_bytes);
}
inline const float* map_at(const float* base, size_t elems, size_t elem_bytes) { return map_at(const_cast<float*>(base), elems, elem_bytes); }
// floats that hold `elems` map elements of that width
inline size_t floats_for(size_t elems, size_t elem_bytes) { return (elems * elem_bytes + sizeof(float) - 1) / sizeof(float); }

// where the maps of a group go
struct Sink {
    float* packed = nullptr;        // device base, maps consecutive
    float* const* ptrs = nullptr;   // or one pointer per map
    int location = FFTCONV_DEVICE;  // of ptrs
    const OutWindow* window = nullptr;   // or (block plan of an overlap-save plan) the output kernel stores this window of the full maps
    // a plan holding several images: maps between the first maps of two images in `packed` / `ptrs` -- the kernels of the whole
    // call, of which the group may be a part (ragged cells); 0 = the kernels of the group
    int image_stride = 0;
    // per-map extrema: the call's map index of the group's first map (`ptrs` of a later group of a ragged call starts there)
    int map0 = 0;
};

struct BatchSizes {
    size_t per_a;  // c32 of column spectrum per kernel
    int nbY;       // maps per spectral/output launch (kernels of one image)
    int nbM;       // maps per launch over the images the plan holds (>= nbY; equal on a one-image plan)
    int nbA;       // kernels per column-spectrum chunk (a multiple of nbY)
};

// ---- plan core (fftconv_api.cpp) ----
int use_device(const fftconv_plan* p);
BatchSizes batch_sizes(const fftconv_plan* p, int n, int kw);
int check_kernel_size(const fftconv_plan* p, int kh, int kw);
int check_thread_size(const double* thread_size, int n_thread_size);
// threads per workgroup of the generic column / row kernels
int cols_threads(const Geometry& g);
int rows_threads(const Geometry& g);
// the deferred kernel-column pass of fftconv_plan_prepare_kernels_packed, launched by itself on the stream it was recorded for
int flush_pending_prepare(fftconv_plan* p);
// Core of the per-kernel loop for n kernels of one size, packed on the device at dk ([n][F][kw][kh]); on failure nothing of the
// host-output ring is still writing into the caller's buffers when the error is returned
int run_group(fftconv_plan* p, int n, const float* dk, int kh, int kw, const Sink& sink);
// fftconv_plan_prepare_kernels_packed behind its argument checks (one-pass plans).  force_defer: as if option "defer_prepare" were
// set -- the one-shot entry stages its kernels ahead of the image; whether the request was in fact recorded: p->a_holds.pending()
int prepare_kernels(fftconv_plan* p, int n, const float* dk, int kh, int kw, bool force_defer);
// cyclic: the block plan of an overlap-save block-wise plan (PlanTuning::cyclic) -- never block-wise itself
int plan_create_internal(fftconv_plan** plan, int data_h, int data_w, int feature_dim, int max_kernel_h, int max_kernel_w, int gpu_id,
                         void* hip_stream, const fftconv_plan_options* options, bool cyclic);

// ---- output side of the plan core (plan_output.cpp) ----
// How the maps of a group leave the device: the route, decided once per group, and what the loop needs beside it
struct Delivery {
    OutputRoute r;
    DevBuf<float>* stage = nullptr;    // staged routes: where the maps wait for their copy (r.staging)
    size_t oe = 0;                     // elements per delivered map
    size_t eb = sizeof(float);         // bytes per element ("map_format")
    size_t mb() const { return oe * eb; }
};
// what one launch of a group adds to the route: its maps are image-major from image image0 on with per_image kernels each, and
// consts[0] is the constant of the launch's first kernel (score 4: KC at the kernel's place in the chunk)
struct OutLaunch {
    int image0 = 0, per_image = 1;
    const float* consts = nullptr;
    int record0 = 0;      // per-map extrema: the record of the launch's first map
};
// the route of a group into `sink` and the buffers it names, sized for nbY maps per launch (the ring: started)
int plan_delivery(fftconv_plan* p, const Sink& sink, int nbY, Delivery& d);
// output columns of ny maps: Y transformed along h into the maps at obase (win: into the window of an overlap-save block)
int launch_output_cols(fftconv_plan* p, const OutputRoute& r, const OutWindow* win, float* obase, int ny, const OutLaunch& l);
// per-map extrema of the ny delivered maps at `dest` (dense, in the route's map format), behind the last kernel that writes them and
// ahead of any copy-out: the fold of the partials the fused store wrote (r.extrema Fused), or the scan and its fold (Scan)
int launch_extrema(fftconv_plan* p, const OutputRoute& r, const float* dest, int ny, const OutLaunch& l);
// the peak lists of the same maps (fftconv_plan_set_peaks), behind launch_extrema: found and records [l.record0, l.record0 + ny)
int launch_peaks_scan(fftconv_plan* p, const OutputRoute& r, const float* dest, int ny, const OutLaunch& l);
// r.after: nmaps full fp32 windows at src cropped (padded) into dst and combined with the route's plane on the way
int launch_region(const fftconv_plan* p, const OutputRoute& r, const float* src, float* dst, int nmaps, hipStream_t s, const OutLaunch& l = {});
// the maps [first, first + ny) are queued into `dest` (staging buffer buf of a streamed group): their way to the caller
int deliver_batch(fftconv_plan* p, const Delivery& d, const Sink& sink, int first, int ny, int buf, const float* dest);
// the rectangle launch of a route whose store is Rect, RectScale, RectAdd or RectStride: ny maps from the intermediate y, dense from `out` on
FastColsShape output_rect_shape(const fftconv_plan* p, const OutputRoute& r, const c32* y, float* out, int ny, const OutLaunch& l = {});

// ---- host-output streaming (host_ring.cpp) ----
// A streamed group (run_group, host maps of at least host_min_kb) has two staging buffers on the device: batch b is computed into
// buffer b & 1 while the copy-out of batch b - 1 runs.
// start of a group: the plan's ring (pinned ring + copy stream + host copy threads, sized for its maps), created on first use
int ring_begin(fftconv_plan* p);
// which staging buffer the next batch is computed into; the plan's stream (or the host) waits until its previous contents have left
int ring_claim_staging(fftconv_plan* p, int* buf);
// the maps [first, first + count) have been launched into `staging` (buffer buf): queues the copy-out of the batch before it
int ring_batch_launched(fftconv_plan* p, const Sink& sink, int first, int count, int buf, const float* staging);
// end of a group: the last batch's copy-out, and every map in the caller's memory
int ring_finish(fftconv_plan* p, const Sink& sink);

// ---- placement tuning (placement.cpp) ----
// before the first launch of a group of n maps into a (re)allocated intermediate: times candidate allocations of it where the plan's
// tune_placement option (or its automatic default) says so.  route: the group's (its probe launch, what the output kernel stores and
// whether `out`, its target, is the caller's packed maps or a staging buffer)
int tune_intermediate_placement(fftconv_plan* p, const OutputRoute& route, int n, int nbY, float* out);

// ---- block-wise plans (blockwise.cpp) ----
bool blocks_preferred(const Geometry& g, const fftconv_plan_options* options);
int tiled_create(fftconv_plan* p, int H, int W, int F, int mkh, int mkw, void* hip_stream, const fftconv_plan_options* options);
int tiled_set_image(fftconv_plan* p, const float* data, int location);
int tiled_convolve(fftconv_plan* p, int n, const float* const* kernels, const int* kh, const int* kw, int kernel_location,
                   float* const* out, int out_location, float* out_packed);
int tiled_unsupported(const char* what);

}  // namespace fc

struct TiledState {
    fftconv_plan* sub = nullptr;     // the block plan (an ordinary plan on the same stream)
    int H = 0, W = 0, F = 0, mkh = 0, mkw = 0;
    int Bh = 0, Bw = 0, nbh = 0, nbw = 0, nblk = 0, FH = 0, FW = 0;
    // overlap-save (see the comment above): the block plan is cyclic over Lh x Lw samples, block (by, bx) reads the image rows
    // [by * Bh - Sh, by * Bh + Bh) and stores the rows [by * Bh, by * Bh + Bh) of the maps straight from the output kernel
    bool save = false;
    int Lh = 0, Lw = 0, Sh = 0, Sw = 0;
    size_t spec_elems = 0;           // c32 per block spectrum
    DevBuf<c32> specs;               // block spectra, [block][spec_elems] (own buffer)
    c32* specs_x = nullptr;          // caller-owned instead (fftconv_plan_use_spectrum_buffer)
    DevBuf<float> big, tmp, blk;     // full maps of a kernel chunk, block maps of that chunk, one zero-padded image block
    DevBuf<float> crop;              // "output_region" maps of a kernel chunk, cropped out of `big` for the copy-out
    DevBuf<float> kstage;            // host kernels of a chunk, staged on the device once (every block convolves them)
    std::vector<float> hblk;         // host staging of one image block
    bool have_image = false;
    c32* spec_base() const { return specs_x ? specs_x : specs.p; }
    size_t spec_total() const { return spec_elems * (size_t)nblk; }
    size_t big_map() const { return (size_t)FH * FW; }
    void release() {
        if (sub) fftconv_plan_destroy(sub);
        sub = nullptr;
        specs.release(); big.release(); tmp.release(); blk.release(); kstage.release(); crop.release();
    }
};

namespace fc {
// plan_rules.hpp on this plan: 0 if asking `ask` for `value` passes, else the first rule's code, with its message recorded
inline int plan_refused(const fftconv_plan* p, Ask ask, long value = 1) {
    PlanRuleState s;
    s.blocks = p->tiled ? p->tiled->nblk : 0;
    s.F = p->g.F;
    s.score = p->opt_score; s.border = p->border_mode; s.filter = p->opt_filter;
    s.rows_fast = p->g.fast_rows.ok; s.filter_built = fast_rows_filter_built(p->g.Lw); s.Lw = p->g.Lw;
    const Refusal r = plan_refusal(s, ask, value);
    return r ? api_fail(r.rule->code, r.rule->fmt, r.arg) : 0;
}
// ... of the output side's table (per-map extrema); window_sink: the group at hand stores through an output window
inline int plan_refused(const fftconv_plan* p, AskOutput ask, long value, bool window_sink = false) {
    PlanRuleState s;
    s.blocks = p->tiled ? p->tiled->nblk : 0;
    s.window_sink = window_sink;
    const OutputRefusal r = plan_refusal(s, ask, value);
    return r ? api_fail(r.rule->code, r.rule->fmt, r.arg) : 0;
}
// ... of the peak lists' table
inline int plan_refused(const fftconv_plan* p, AskPeaks ask, long value, bool window_sink = false) {
    PlanRuleState s;
    s.blocks = p->tiled ? p->tiled->nblk : 0;
    s.window_sink = window_sink;
    const PeaksRefusal r = plan_refusal(s, ask, value);
    return r ? api_fail(r.rule->code, r.rule->fmt, r.arg) : 0;
}
}  // namespace fc
