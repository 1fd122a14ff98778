/*
 * fftconv.h -- C ABI of the MI355X-native 2-D FFT-convolution engine (libfftconv.so).
 *
 * This is the drop-in boundary for the reference's `cudaConvolutionFFT` hot path
 * (chrischoy/CUDA-FFT-Convolution).  Every entry point names the reference interface it
 * replaces (paths relative to the reference tree).  Plain C: pointers and sizes only, no
 * torch / HIP types in the signatures (a HIP stream is passed as an opaque void*).
 *
 * Conventions shared by all entry points
 *   - Arrays use MATLAB column-major layout exactly as the reference reads them:
 *     data is H x W x F, element (y, x, z) at z*H*W + x*H + y
 *     (src/cudaConvFFTData.cuh:26-27); kernel k is kh x kw x F in the same layout.
 *   - Every result map is the FULL padded window FFT_H x FFT_W (column-major, NOT cropped),
 *     FFT_X = fftconv_fft_size16(DATA_X + MAX_KERNEL_X - 1)
 *     (src/cudaConvolutionFFT.cu:103-110,198-200).  Cells outside the linear-convolution
 *     support (DATA+k-1) are zero up to fp32 round-off, as in the reference.
 *   - The product is a plain complex multiply (convolution, not correlation:
 *     src/cudaConvFFTData.cuh:62-65); flip the kernel for template matching
 *     (demoCudaConvolutionFFT.m:63-69).
 *   - Functions return FFTCONV_OK (0) or a negative fftconv_status; the message of the last
 *     failure on the calling thread is returned by fftconv_last_error().  The library never
 *     calls exit() (the reference's CUDA_SAFE_CALL does: src/cudaConvFFTData.h:6-29) and
 *     releases all device memory on error paths.
 *   - There is no CPU fallback: without a usable HIP device every compute entry point fails
 *     with FFTCONV_ERR_NO_DEVICE / FFTCONV_ERR_HIP.
 */
#ifndef FFTCONV_H
#define FFTCONV_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum fftconv_status {
    FFTCONV_OK = 0,
    FFTCONV_ERR_INVALID_ARG = -1,      /* "Wrong number of inputs" / "Invalid data input" class (src/cudaConvolutionFFT.cu:45-54) */
    FFTCONV_ERR_THREAD_SIZE = -2,      /* thread-size array does not have 4 elements (src/cudaConvolutionFFT.cu:72-73) */
    FFTCONV_ERR_KERNEL_SHAPE = -3,     /* feature mismatch or kernel larger than the FFT window (src/cudaConvolutionFFT.cu:242-243) */
    FFTCONV_ERR_KERNEL_EXCEEDS_MAX = -4, /* kernel larger than MAX_KERNEL and the internal transform is not the ceil16 window */
    FFTCONV_ERR_UNSUPPORTED_SIZE = -5, /* transform does not fit the single-pass LDS engine */
    FFTCONV_ERR_NO_DEVICE = -6,
    FFTCONV_ERR_HIP = -7,              /* a HIP runtime call failed; message has the HIP error string */
    FFTCONV_ERR_ALLOC = -8,
    FFTCONV_ERR_NO_IMAGE = -9          /* convolve called before an image spectrum exists */
} fftconv_status;

/* Error id the MEX gateway raises for argument errors (src/cudaConvolutionFFT.cu:30). */
#define FFTCONV_MEX_ERROR_ID "cudaConvFFTData:InvalidInput"

enum { FFTCONV_HOST = 0, FFTCONV_DEVICE = 1,
       FFTCONV_AUTO = 2 /* kernels of fftconv_plan_convolve only: every pointer may be host or device memory, the
                           HIP runtime tells them apart (a cell mixing host arrays and gpuArrays:
                           src/cudaConvolutionFFT.cu:207-238) */ };

/* computeFFTsize16 (src/cudaConvFFTData.h:96-102): round up to a multiple of 16. */
int fftconv_fft_size16(int data_size);

/* computeFFTsize (src/cudaConvFFTData.h:67-94), the reference's alternative sizing: up to a
 * multiple of 16, then up to the next power of two.  Its shipped path never calls it; plans offer
 * it as "output_region" 4. */
int fftconv_fft_size_pow2(int data_size);

/* Message of the last failure on this thread ("" if none). */
const char *fftconv_last_error(void);

/* Library version string. */
const char *fftconv_version(void);

/* Number of visible HIP devices (0 and FFTCONV_ERR_NO_DEVICE when there is none). */
int fftconv_device_count(int *count);

/* ------------------------------------------------------------------------------------------
 * One-shot entry: the body of mexFunction in src/cudaConvolutionFFT.cu:27-311.
 *
 *   cvcell = cudaConvolutionFFT(data, maxKernelH, maxKernelW, kernelCell[, threadSize][, gpuId])
 *
 *   data, data_h, data_w, feature_dim   prhs[0]  host single H x W x F (:49-54,92-99); F = 1 is
 *                                                accepted (the reference rejects it)
 *   max_kernel_h, max_kernel_w          prhs[1], prhs[2] (:58-59)
 *   n_kernel, kernels, kernel_h/_w      prhs[3]  cell array of host single kh x kw x F (:64-67,207-222)
 *   kernel_f                            per-kernel feature count for the :242 check; NULL = F
 *   thread_size, n_thread_size          prhs[4]  optional; must have 4 elements (:72-73); the
 *                                                values are accepted and ignored (block shapes
 *                                                are the engine's business)
 *   gpu_id                              prhs[5]  0-based device (:85-89); < 0 = current device
 *   out                                 plhs[0]  n_kernel caller buffers of FFT_H*FFT_W floats
 *                                                (the reference allocates them: :284-288)
 *   fft_h, fft_w                        out, nullable: the window size
 * Synchronous: results are complete on return.  The plan (tables, device scratch) goes back into the
 * plan cache below instead of being torn down; fftconv_cache_clear() releases it.
 * Images whose padded size exceeds what one plan transforms in a single pass, and large images that
 * run faster that way, are convolved block-wise (fftconv_plan_options.blockwise): blocks of a
 * shorter transform, each block's rectangle of the FFT_H x FFT_W maps stored by the output kernel
 * (kernels larger than MAX_KERNEL are rejected on that path).
 * ------------------------------------------------------------------------------------------ */
int fftconv_convolution_fft(const float *data, int data_h, int data_w, int feature_dim,
                            int max_kernel_h, int max_kernel_w,
                            int n_kernel, const float *const *kernels,
                            const int *kernel_h, const int *kernel_w, const int *kernel_f,
                            const double *thread_size, int n_thread_size,
                            int gpu_id,
                            float *const *out, int *fft_h, int *fft_w);
/* The same with plan options (forward-declared below; NULL = defaults) and kernels that may be
 * device-resident: kernel_location FFTCONV_HOST, FFTCONV_DEVICE, or FFTCONV_AUTO for a cell that
 * mixes host arrays and gpuArrays as the reference's loop allows (src/cudaConvolutionFFT.cu:207-238). */
struct fftconv_plan_options;
int fftconv_convolution_fft_ex(const float *data, int data_h, int data_w, int feature_dim,
                               int max_kernel_h, int max_kernel_w,
                               int n_kernel, const float *const *kernels,
                               const int *kernel_h, const int *kernel_w, const int *kernel_f,
                               int kernel_location,
                               const double *thread_size, int n_thread_size,
                               int gpu_id,
                               float *const *out, int *fft_h, int *fft_w,
                               const struct fftconv_plan_options *options);

/* ------------------------------------------------------------------------------------------
 * Plan cache of the one-shot entries.  The reference builds its cuFFT plans, allocates its six device
 * buffers and tears everything down inside every MEX call (src/cudaConvolutionFFT.cu:127-142,144-185,
 * 302-310); here that state is a plan, and fftconv_convolution_fft / _ex (and with them the
 * cudaConvolutionFFT gateway) keep the plans of their last few distinct problems -- key: data size, F,
 * MAX_KERNEL, device, creation options -- with their tables, device scratch and host copy threads, so that
 * a repeated call pays for the transfers and the kernels only (cfg2: 15.9 ms -> the reused-plan time).
 * A plan is handed to one call at a time; a concurrent call with the same key builds a plan of its own.
 * A call that fails with a HIP / allocation error does not return its plan to the cache.
 *   fftconv_cache_configure  max_plans: plans kept (default 4; 0 switches the cache off and empties it),
 *                            max_bytes: device memory the idle cached plans may hold together (default: a quarter of
 *                            the device's memory, at most 48 GiB; 0 = keep the current value); least recently used plans go
 *                            first.  Whatever the limits, EVERY idle plan is released -- and the request repeated once -- when
 *                            a device allocation of this library fails (any entry, not only the one-shot ones): cached
 *                            scratch never turns a call that used to fit into an out-of-memory error
 *   fftconv_cache_clear      destroys every idle cached plan (device memory, host threads).  The gateways
 *                            register it with mexAtExit; a process that unloads the library calls it first.
 *   fftconv_cache_stats      nullable outputs: plans held now, hits / misses so far, device bytes held
 * ------------------------------------------------------------------------------------------ */
int fftconv_cache_configure(int max_plans, size_t max_bytes);
int fftconv_cache_clear(void);
int fftconv_cache_stats(long *plans, long *hits, long *misses, size_t *device_bytes);

/* Where the time of this thread's last one-shot call (fftconv_convolution_fft / _ex) went, milliseconds of wall
 * clock: what the reference spends in plan creation and allocation (src/cudaConvolutionFFT.cu:127-142,144-185), the
 * image upload + transform (:146-169), the per-kernel loop with its copies (:204-291) and the teardown (:302-310).
 * With plan option / fftconv_plan_options.verbose the same line goes to stderr. */
typedef struct fftconv_call_timing {
    double plan_ms;        /* cache lookup, or plan creation: tables, kernel set-up, device tables */
    double image_ms;       /* the image staged / copied and its transform QUEUED (small images go through pinned staging and the
                              call does not wait for the GPU: the transform's run time then shows in convolve_ms) */
    double convolve_ms;    /* kernel uploads, every map computed and copied into the caller's buffers */
    double release_ms;     /* plan back into the cache, or its teardown */
    double total_ms;
    int cache_hit;         /* 1: the plan came from the cache */
} fftconv_call_timing;
int fftconv_last_call_timing(fftconv_call_timing *timing);

/* ------------------------------------------------------------------------------------------
 * Plan API: the state the reference keeps inside one mexFunction call (cuFFT plans
 * src/cudaConvolutionFFT.cu:122-142, image spectrum d_CFFT_DATA :165-168, scratch :182-185)
 * and, in its multi-GPU sketch, inside a ConvPlan (src/cudaConvFFTDataStreams.cu:273-328),
 * made a first-class object so the image spectrum is computed once and reused against any
 * number of kernels and calls (what cudaFFTData / cudaConvFFTData exist for:
 * src/cudaFFTData.cu:18-160, src/cudaConvFFTData.cu:24-306).
 * A plan is bound to one device; calls on one plan must not overlap.
 * ------------------------------------------------------------------------------------------ */
typedef struct fftconv_plan fftconv_plan;

typedef struct fftconv_plan_info {
    int data_h, data_w, feature_dim;
    int max_kernel_h, max_kernel_w;
    int fft_h, fft_w;          /* output window (reference's ceil16 sizes) */
    int transform_h, transform_w; /* internal transform lengths (>= DATA + MAXK - 1) */
    int spectrum_rows;         /* transform_h / 2 + 1 */
    int spectrum_pitch;        /* complex elements per spectrum row */
    int gpu_id;
    int exact_window;          /* 1 if transform == window: circular modulus equals the reference's */
    size_t spectrum_bytes;     /* size of the image spectrum buffer */
    size_t map_bytes;          /* fft_h * fft_w elements of the plan's "map_format": 4 bytes each (fp32), or 2 */
    size_t workspace_bytes;    /* device scratch currently held */
    int out_h, out_w;          /* size of every result map: the window, or the "output_region" chosen */
    size_t out_map_bytes;      /* out_h * out_w elements of the plan's "map_format": what a result buffer holds per map */
} fftconv_plan_info;

/* hip_stream: hipStream_t to run on (NULL = the device's default stream). */
int fftconv_plan_create(fftconv_plan **plan, int data_h, int data_w, int feature_dim,
                        int max_kernel_h, int max_kernel_w, int gpu_id, void *hip_stream);

/* Choices fixed at plan creation.  Zero-initialise, set struct_size = sizeof(fftconv_plan_options),
 * then the fields wanted; NULL options = all defaults.  The library reads no environment
 * variables: everything that steers it goes through this struct or fftconv_plan_set_option. */
typedef struct fftconv_plan_options {
    size_t struct_size;
    int kernel_path;    /* 0 (default): specialised kernels where the transform lengths have them, tiled
                         *    intermediate; 1: generic kernels only (any supported length; the cross-check of
                         *    the specialised path); 2: specialised kernels with a row-major intermediate */
    int rows_group;     /* maps one workgroup of the spectral-row kernel walks with its image-spectrum row in
                         *    registers (F = 1): 0 (default) chosen per launch, 1 one map per workgroup, n > 1 fixed */
    int max_transform;  /* > 0: largest transform length a plan may use; beyond it the plan is block-wise
                         *    with block transforms of at most this size (see `blockwise`) */
    int exact_window;   /* 1: the transform lengths must be the ceil16 window FFT_H x FFT_W itself (the
                         *    reference's circular modulus, plan_info.exact_window = 1) -- what
                         *    fftconv_plan_export_spectrum / _import_spectrum need.  Any window works
                         *    whose transforms fit the LDS, every ceil16 window up to 8448 included: a
                         *    window length (FFT_W, or FFT_H / 2 for the real h transform) with a prime
                         *    factor above 17 runs Bluestein (chirp-z) transforms of a work length
                         *    >= 2 x that length on the generic kernels (slower than the specialised
                         *    ones).  Larger windows fail with FFTCONV_ERR_UNSUPPORTED_SIZE. */
    int blockwise;      /* 0 (default): the plan convolves block-wise where that is needed or faster -- padded sizes beyond one
                         *    LDS-resident transform pass (about 20 000 samples along w) or beyond max_transform, and sizes whose
                         *    one-pass transform would run on the slower long-transform kernels (from about 4900 x 4900 with
                         *    63 x 63 kernels; the planner weighs measured costs per length).  Blocks are overlap-save over a
                         *    block plan whose transform has specialised kernels: every block is a piece of the image with
                         *    MAX_KERNEL - 1 history rows / columns, convolved circularly, and the output kernel stores the part
                         *    that is not wrapped straight into the block's rectangle of the maps (nothing is summed, every
                         *    element is written once); where the block transform has no specialised kernels (kernel_path = 1,
                         *    very wide kernels) blocks are zero-padded and summed (overlap-add).  Block spectra are kept per
                         *    image; every plan entry point works (two-step, packed device-resident, multi-device), except the
                         *    spectrum exchange in the reference's order and "output_region"; kernels larger than MAX_KERNEL
                         *    are rejected there.  1: never block-wise -- one pass, or FFTCONV_ERR_UNSUPPORTED_SIZE.  (Appended
                         *    in 0.2: a struct_size without this field is accepted and means 0.)  fftconv_plan_get_option
                         *    "blockwise" reads the number of blocks of a plan (0 = single pass), "overlap_save" whether they are
                         *    stored (1) or summed (0); plan_info.transform_h / _w are the block transform then.  The reference
                         *    plans cuFFT for any size: src/cudaFFTData.cu:72-103, src/cudaConvFFTData.cu:92-98. */
    int verbose;        /* 1: the plan starts with option "verbose" on (the reference's compile-time `debug`,
                         *    src/cudaConvolutionFFT.cu:9), and a one-shot call prints where its time went
                         *    (fftconv_call_timing).  (Appended in 0.3; a struct_size without it means 0.) */
    int map_format;     /* element format of every result map: 0 (default) fp32, 1 IEEE fp16, 2 bfloat16 -- plan option
                         *    "map_format", which see; part of the key of the one-shot entries' plan cache.  With 1 or 2 every
                         *    `float *` that names result maps in this header (out, out_device, the members of out[]) is an
                         *    OPAQUE pointer to out_h x out_w 16-bit elements per map.  FFTCONV_ERR_INVALID_ARG where the planner
                         *    would make the plan block-wise (`blockwise`).  (Appended in 0.4; a struct_size without it means 0.) */
} fftconv_plan_options;
int fftconv_plan_create_ex(fftconv_plan **plan, int data_h, int data_w, int feature_dim,
                           int max_kernel_h, int max_kernel_w, int gpu_id, void *hip_stream,
                           const fftconv_plan_options *options);
/* 1 if `plan` is a live plan of this library (created and not yet destroyed), else 0.  The MEX
 * gateways check the uint64 handles MATLAB hands back with it before dereferencing them. */
int fftconv_plan_is_live(const fftconv_plan *plan);
int fftconv_plan_destroy(fftconv_plan *plan);
int fftconv_plan_get_info(const fftconv_plan *plan, fftconv_plan_info *info);

/* Zero-pad + forward transform of the image: padData + cufftExecR2C on the data
 * (src/cudaConvolutionFFT.cu:144-169; src/cudaFFTData.cu:105-147).
 * location: FFTCONV_HOST (pageable or pinned host memory) or FFTCONV_DEVICE.
 * Ordering: the transform is queued on the plan's stream and the call may return before it has run, for device AND host
 * input.  Host input: `data` has been consumed when the call returns (copied, or staged in the plan's pinned buffer -- images
 * up to 1 MiB -- in which case the call does not wait for the GPU at all); the spectrum is ordered on the plan's stream like
 * any other work of the plan.  A caller that reads fftconv_plan_spectrum() on ANOTHER stream orders that stream behind the
 * plan's (an event, or fftconv_plan_synchronize) whatever the location.  Device input: `data` must stay valid until the
 * stream has passed the transform.
 * A call that fails with an argument error leaves the plan as it was.  One that fails later -- an allocation, a copy or a launch
 * (FFTCONV_ERR_ALLOC / FFTCONV_ERR_HIP) -- leaves the plan WITHOUT an image once the transform has been started (option "images" reads 0,
 * a convolve fails with FFTCONV_ERR_NO_IMAGE): the spectrum buffer may have been reallocated or half overwritten by then.  The same holds for
 * fftconv_plan_set_images. */
int fftconv_plan_set_image(fftconv_plan *plan, const float *data, int location);

/* Image batches: the plan holds n_images images of its size and convolves ALL of them with the kernels of every following call --
 * video frames, equal-sized pyramid levels, tiles.  `data`: n_images images back to back ([b][f][w][h], each as
 * fftconv_plan_set_image takes it), host or device memory; ordering and consumption as for fftconv_plan_set_image (queued on the
 * plan's stream; host data consumed on return; the pinned staging takes a whole batch of at most 1 MiB).  The batch is ONE forward
 * pass over n_images * F planes -- the launches of one image -- and a convolve puts the (image, kernel) grid behind its launches:
 * where n_images * n_kernel maps fit one launch ("batch_maps"), one spectral-row launch and one output launch in all.
 *   fftconv_plan_convolve_packed  writes n_images * n_kernel consecutive maps, image-major: map b * n_kernel + k is image b (x) kernel k.
 *   fftconv_plan_convolve         takes out[] with n_images * n_kernel pointers in the same order; kernels[] keeps n_kernel entries
 *                                 (ragged cells as ever).
 * Every output option ("map_format", fftconv_plan_set_output_rect, "output_region", "flip_kernels") and every delivery route acts
 * per map; fftconv_plan_prepare_kernels_packed and "defer_prepare" work (the kernel half does not depend on the images).  After one
 * warm-up call with the same arguments fftconv_plan_set_images(DEVICE) + fftconv_plan_convolve_packed allocate nothing and never
 * synchronise.  The spectrum buffer grows on demand: fftconv_plan_spectrum returns n_images * plan_info.spectrum_bytes, image b at
 * offset b * spectrum_bytes (spectrum_bytes stays the size of ONE image); a caller's buffer (fftconv_plan_use_spectrum_buffer) must
 * hold that much.  fftconv_plan_set_image means one image and returns the plan to one image; read-only option "images" tells how
 * many the plan holds (0 before any).  FFTCONV_ERR_INVALID_ARG, the plan's state untouched: n_images < 1; n_images > 1 on a
 * block-wise plan ("blockwise" > 0: block spectra are kept per image); a caller's spectrum buffer that is too small.  While a plan
 * holds more than one image fftconv_plan_export_spectrum / _import_spectrum fail with FFTCONV_ERR_INVALID_ARG, and "tune_placement"
 * -1 (automatic) does not tune.  fftconv_multi_*, the one-shot and the two-step entries take one image. */
int fftconv_plan_set_images(fftconv_plan *plan, const float *data, int n_images, int location);

/* Typed images: camera pixels and half-precision tensors as they are, converted in the load -- the caller writes no fp32 copy,
 * and a host image crosses the bus in its own bytes (a quarter of fp32's for uint8; the pinned staging of at most 1 MiB and the
 * 512 KiB read in place are counted in those bytes, so four times the uint8 pixels fit).
 * `data`: n_images images in the layout of fftconv_plan_set_images ([b][f][w][h], h contiguous, no gaps) in ELEMENTS of
 * pixel_format, host or device memory, aligned for its element.  The VALUE of a pixel is its exact fp32 conversion -- all four
 * conversions are exact, so every map is bit-equal to the map fftconv_plan_set_images gives on those fp32 values.  There is no
 * implied 1/255: gain belongs in the kernels or in the maps; normalised maps (fftconv_plan_set_normalisation) do not depend on
 * gain anyway; raw uint8 / uint16 sums can overflow fp16 maps ("map_format" 1: 65504).  FFTCONV_PIXEL_BF16 / _F16 elements are
 * bit patterns (subnormals kept); Inf and NaN pass through as fp32 would carry them.
 * FFTCONV_PIXEL_F32 is fftconv_plan_set_images itself: the same code path, the same bits.
 * Failure contract: fftconv_plan_set_images'.  FFTCONV_ERR_INVALID_ARG, the plan's state untouched: NULL, a pixel_format outside
 * 0..4, n_images < 1, a bad location, n_images > 1 on a block-wise plan, a caller's spectrum buffer that is too small.  A failure
 * after the transform has started leaves the plan without an image.
 * Routes.  Direct: on a one-pass plan whose image column pass is the specialised kernel ("specialised_kernels" bit 1) that kernel
 * loads the typed elements -- rows 2n, 2n + 1 in one 16- / 32-bit load where every such pair is aligned (data pointer, H and H * W
 * all even in elements), else element by element -- and converts them in registers; the window statistics of normalised maps read
 * the typed elements too.  Staged: everywhere else (generic and Bluestein / exact_window column passes, block-wise plans) and with
 * option "pixel_store" 0 one small kernel writes the fp32 image into the plan's staging first (typed host data after its copy to
 * the device) and the call goes on as fftconv_plan_set_images from device memory.
 * Options: "pixel_store" (1 (default): direct where possible; 0: always staged -- takes effect at the next typed call),
 * read-only "pixel_direct" (1 if a typed call on this plan, with the options as they are, converts in the column kernel's load)
 * and "pixel_format" (the format of the images the plan holds: 0 after fftconv_plan_set_image / _set_images, an imported or
 * caller-written spectrum, or while it holds none).
 * "defer_prepare" merges a recorded kernel preparation with the column pass of fp32 images only: a typed image on the direct
 * route launches the pending kernels' column pass by itself, then its own.  A warm device-resident call allocates nothing, never
 * synchronises and can be captured into a graph.
 * Every other entry keeps fp32 images: fftconv_multi_*, the one-shot and two-step entries, the plan cache, the MEX gateways. */
enum { FFTCONV_PIXEL_F32 = 0, FFTCONV_PIXEL_U8 = 1, FFTCONV_PIXEL_U16 = 2, FFTCONV_PIXEL_F16 = 3, FFTCONV_PIXEL_BF16 = 4 };
int fftconv_plan_set_images_typed(fftconv_plan *plan, const void *data, int pixel_format, int n_images, int location);

/* Device pointer + size of the image spectrum (library-owned, valid until destroy).  This is the
 * buffer the multi-GPU path broadcasts (the reference's cudaMemcpyPeerAsync of d_CFFT_DATA,
 * src/cudaConvFFTDataStreams.cu:279-289): rank 0 fills it with set_image, the others receive it
 * and call fftconv_plan_mark_spectrum_valid.  The layout is internal. */
int fftconv_plan_spectrum(fftconv_plan *plan, void **device_ptr, size_t *bytes);
int fftconv_plan_mark_spectrum_valid(fftconv_plan *plan);
/* Make the plan keep its image spectrum in caller-owned device memory (>= spectrum_bytes, 16-byte
 * aligned, must outlive the plan or the next call of this function; NULL = back to the plan's own
 * buffer).  Lets a communication library that owns its buffers (torch.distributed / RCCL)
 * broadcast the spectrum with no staging copy.  Invalidates the current spectrum. */
int fftconv_plan_use_spectrum_buffer(fftconv_plan *plan, void *device_ptr, size_t bytes);

/* The image spectrum in the reference's own order: what cudaFFTData returns as a complex single
 * gpuArray of (FFT_H/2+1) x FFT_W x F (src/cudaFFTData.cu:90-103,150), i.e. cufftExecR2C's output
 * [f][FFT_W][FFT_H/2+1] (src/cudaConvolutionFFT.cu:122-142: the halved dimension is h), unnormalised,
 * interleaved (re, im) floats; spectrum_natural_bytes = 8 * F * FFT_W * (FFT_H/2+1).
 * export: after fftconv_plan_set_image; import: replaces set_image (a spectrum the caller kept or
 * edited).  Both need a plan whose transform is the window (fftconv_plan_options.exact_window, or
 * plan_info.exact_window = 1 anyway) and return FFTCONV_ERR_UNSUPPORTED_SIZE otherwise.
 * location: FFTCONV_HOST or FFTCONV_DEVICE; synchronous for host memory. */
int fftconv_plan_export_spectrum(fftconv_plan *plan, float *spectrum, int location);
int fftconv_plan_import_spectrum(fftconv_plan *plan, const float *spectrum, int location);

/* Per-kernel loop of src/cudaConvolutionFFT.cu:204-291 for arbitrary (possibly different)
 * kernel sizes.  kernels[k]: kh[k] x kw[k] x F, host or device (gpuArray kernels: :224-238);
 * out[k]: FFT_H*FFT_W floats, host or device.  Synchronous for host output.
 * Device output: the maps are queued on the plan's stream and the call may return before they are written.  HOST kernel
 * arrays (FFTCONV_HOST, and the host members of an FFTCONV_AUTO cell) have been consumed when the call returns, whatever
 * the output location: a group of at most 512 KiB is gathered by the CPU into the plan's pinned buffer and read from
 * there (the first such call does not wait for the GPU at all; a later one waits until the work that still reads the
 * buffer is over), a larger one goes through the runtime's copies from pageable memory, which have read the array when
 * they return.  Device kernels must stay valid until the stream has passed the call. */
int fftconv_plan_convolve(fftconv_plan *plan, int n_kernel,
                          const float *const *kernels, const int *kernel_h, const int *kernel_w,
                          int kernel_location,
                          float *const *out, int out_location);

/* Same for n_kernel equally-sized kernels packed contiguously in device memory
 * ([n][F][kw][kh], i.e. n consecutive MATLAB arrays) writing n consecutive maps to device
 * memory ([n][FFT_W][FFT_H]).  Fully asynchronous on the plan's stream: this is the
 * device-resident mode the benchmark times. */
int fftconv_plan_convolve_packed(fftconv_plan *plan, int n_kernel, const float *kernels_device,
                                 int kernel_h, int kernel_w, float *out_device);

/* Optional split of fftconv_plan_convolve_packed: queues only the part that does not depend on
 * the image (the h-transform of the kernels' columns, i.e. padData + the H half of cufftExecR2C on
 * the kernels, src/cudaConvolutionFFT.cu:245-255) on the plan's stream, at once, so that it overlaps
 * the arrival of the image spectrum (the RCCL broadcast on the other ranks).  The next
 * fftconv_plan_convolve_packed call with the same arguments reuses it; any other use of the plan discards it.
 * With plan option "defer_prepare" = 1 the call only RECORDS the request: the pass then rides in the launch of
 * the next fftconv_plan_set_image on the same stream (one launch fewer per step: what small problems want
 * when the image transform follows on the same stream), or is launched by the next convolve / set_stream /
 * synchronize -- the caller gives up the overlap above for it. */
int fftconv_plan_prepare_kernels_packed(fftconv_plan *plan, int n_kernel, const float *kernels_device,
                                        int kernel_h, int kernel_w);

/* Re-bind the plan to another stream (NULL = the default stream).  Everything queued so far stays
 * on the old stream; the caller orders the two.  After one warm-up call with the same arguments
 * (which sizes the scratch buffers) fftconv_plan_set_image(DEVICE) and
 * fftconv_plan_convolve_packed allocate nothing and never synchronise, so they can be recorded
 * into a HIP graph: bind the plan to the capturing stream, capture, replay the graph
 * (bench.py --graph; the launch-bound small configurations gain most).  This holds for one-pass plans only: a
 * block-wise plan (plan option "blockwise" > 0) synchronises its stream between chunks of kernels and cannot be
 * captured.  fftconv_plan_prepare_kernels_packed may be part of the captured step, deferred or not. */
int fftconv_plan_set_stream(fftconv_plan *plan, void *hip_stream);

/* Block until everything queued on the plan's stream has finished. */
int fftconv_plan_synchronize(fftconv_plan *plan);

/* Options: "batch_maps" (kernels per spectral/output launch, 0 = auto),
 *          "kernel_chunk_mb" (0 = auto: the kernels' column spectra are produced one launch's worth at a
 *             time, right before the row kernel reads them; > 0: as many launches' worth as fit that many MiB),
 *          "tune_placement" (k > 1: the next time the intermediate buffer is (re)allocated, k candidate
 *             allocations of it are timed with the output kernel writing into the caller's map buffer and
 *             the fastest is kept -- on MI355X the output kernel runs 3-4 % faster or slower depending on which
 *             physical allocations hold its two buffers; blocking, ~70-100 ms, once per
 *             allocation; transient device memory while it runs: k intermediates plus k - 1 spacer allocations of at
 *             most 12 GiB (an eighth of what is free) each; skipped inside a stream capture and on plans with an output
 *             window (the blocks of a block-wise plan); 0: never; -1 (default): automatic -- five candidates where a launch
 *             writes at least 2 GiB of maps (BASELINE cfg3 / cfg4) AND at least 60 % of the device's memory is free at that
 *             moment, nothing otherwise (and never in a one-shot call whose plan is not kept: cache switched off).  It pays for itself after ~600
 *             cfg3 steps (7 s of work on the plan).  Which state an untuned plan lands in is a property of the machine's allocation order:
 *             profiles/r05q_default_vs_tuned_final_library*.txt),
 *          "rows_group" (fftconv_plan_options.rows_group, changeable between calls),
 *          "dynamic_tiles" (1, the default for transforms of 864 points and more along h (M >= 432): the persistent workgroups of
 *             the output kernel take their tiles from a queue in device memory -- one counter per XCD, chunks of adjacent tiles,
 *             work stealing at the end -- instead of a fixed 1 / grid share each.  A workgroup whose CU is held by another
 *             kernel (the RCCL broadcast of a multi-GPU step, src/cudaConvFFTDataStreams.cu:279-289,338-447; another library)
 *             then delays nobody's tiles: beside 16-32 foreign workgroups a cfg4 step loses 2.5 % instead of 4.5-7 %, alone it
 *             runs equal or up to 3 % faster (profiles/r05a_contention_ab.txt).  0: the static deal -- the default of smaller
 *             transforms, whose tiles are too short for a ticket fetched one tile ahead (profiles/r05k_dynamic_tiles_by_size.txt);
 *             2: the forward column kernels take their tiles from a counter too (measured slower alone: A/B and tests).
 *             Results are identical bit for bit),
 *          "profile" (1: time every kernel launch with HIP events on the plan's stream),
 *          "profile_kinds" (bit mask over the indices of fftconv_profile: only those kinds are timed
 *             while "profile" is on, 0 = all -- lets a caller time the hot kernels inside its own timed
 *             region at the cost of two event records per launch),
 *          "host_stream" (how maps reach HOST output buffers -- the reference's blocking
 *             cudaMemcpy per map, src/cudaConvolutionFFT.cu:284-286: 0 = blocking copies after each
 *             batch; 1 (default) = host threads of the plan copy batch b straight into the caller's
 *             buffers while batch b+1 is computed; 2 = through a ring of pinned chunks),
 *          "host_threads", "host_chunk_kb", "host_slots" (shape of that machinery, 0 = auto),
 *          "host_min_kb" (maps smaller than this many KiB leave by blocking copies whatever "host_stream"
 *             says; default 1024: the copy threads buy small maps nothing),
 *          "host_pinned" (1, default: small HOST arrays go through pinned staging buffers of the plan -- an image of at most
 *             1 MiB and a kernel group of at most 512 KiB are copied by the CPU and read by the GPU from there (at most
 *             512 KiB: in place, no copy command), maps of at most 4 MiB that leave by blocking copies come back several
 *             per copy and are handed out by the CPU (a single map above 64 KiB keeps its plain copy); the reference issues
 *             one blocking cudaMemcpy per array, src/cudaConvolutionFFT.cu:148,231,286.  Cached one-shot calls of the
 *             reference's demo shape: 120 -> 75 us, profiles/r04s_small_call_latency.txt.  0: plain copies from / into
 *             the caller's arrays),
 *          "output_region" (which part of the padded window a result map holds, for the plan's
 *             MAX_KERNEL sizes K: 0 (default) the whole FFT_H x FFT_W window as the reference
 *             returns it; 1 "full" = the linear convolution, (DATA + K - 1), what the demo crops by
 *             hand (demoCudaConvolutionFFT.m:149); 2 "same" = DATA-sized, centred; 3 "valid" =
 *             DATA - K + 1, no zero padding involved; 4 "pow2 window" = fftconv_fft_size_pow2(DATA + K - 1)
 *             per dimension, the window the reference's unused computeFFTsize would give
 *             (src/cudaConvFFTData.h:67-94): the convolution in its top-left corner, zeros elsewhere.
 *             Result buffers then hold out_h x out_w floats (fftconv_plan_get_info).  Reads 5 after
 *             fftconv_plan_set_output_rect, a rectangle of the caller's; setting 0..4 replaces the rectangle, 5 itself is
 *             set through that entry only),
 *          "rect_store" (1 (default): the output kernel stores the rectangle of fftconv_plan_set_output_rect itself where the
 *             plan has the kernel for it; 0: the window goes through the fp32 staging and is cropped like regions 1-3.
 *             Read-only beside it: "rect_direct" (1 if, with the plan's current settings, the output kernel will store the
 *             rectangle itself), "rect_off_h" / "rect_off_w" (the rectangle's offsets; 0 without one)),
 *          "stride_store" (1 (default): the output kernel samples the strided maps of fftconv_plan_set_output_stride in its store
 *             where the plan can; 0: always the staged route -- the fp32 window, then the sampling crop.  Read-only beside it:
 *             "stride_h" / "stride_w" (the strides; 1 without any) and "stride_direct" (1 if, with the plan's current settings,
 *             the output kernel will sample in its store)),
 *          "image_walk" (image batches, fftconv_plan_set_images.  0 (default): a workgroup of the spectral-row kernel keeps an
 *             image-spectrum row in registers and walks over kernels.  1: where the plan has the kernel for it, a launch of more
 *             than one image keeps the transformed KERNEL row in registers and walks over the images of the launch ("rows_group"
 *             then counts images: automatic, or the walk itself when > 1) -- the forward transform of a kernel row is paid once
 *             per walk instead of once per map, the image-spectrum row is read once per map instead of once per walk: for
 *             many images against few kernels.  A launch of one image runs the kernel it runs at 0.  A convolve puts several
 *             images behind one launch only as whole images x all kernels of the call, "batch_maps" / n_kernel images at a time:
 *             with 64 kernels and the default "batch_maps" (64) every launch holds one image and the option changes nothing -- a
 *             caller raises "batch_maps".  The maps of an (image, kernel) pair are the same bits whatever the walk length and
 *             the batch; they differ from the maps at 0 in the last bits (another summation order in the kernel row's
 *             transform).  Nothing prepared is forgotten.  Read-only beside it: "image_walk_active" (1 if, with the plan's
 *             current settings, a launch of more than one image will walk over images; 0 with "image_walk" 0, F > 1, the
 *             generic or Bluestein row kernel (kernel_path 1), a block-wise plan, and the six row lengths whose kernel is not
 *             built because it would spill registers: 1920, 4160, 4608, 5120, 6144, 7040)),
 *          "defer_prepare" (1: fftconv_plan_prepare_kernels_packed records its request instead of launching it, see
             there; 0 (default): launched at once.  Read-only "prepare_pending": 1 while such a request waits),
          "verbose" (1: the sizes and launch shapes of every stage go to stderr as the work is queued -- the
 *             reference's compile-time `debug` switch, src/cudaConvolutionFFT.cu:9,60,100,114,240,258; 0 (default) silent),
 *          "map_format" (element format of the result maps: 0 (default) fp32, 1 IEEE fp16, 2 bfloat16.  The arithmetic is fp32
 *             up to the store of the output kernel, which converts every value once: round to nearest even, subnormal results
 *             kept, fp16 overflow to +-inf.  Every result buffer of the plan -- host or device, packed or one pointer per map,
 *             whatever the "output_region" -- then holds out_h x out_w 16-bit elements per map in the same column-major
 *             order, plan_info.map_bytes / out_map_bytes count 2 bytes per element, and the `float *` of the signatures is an
 *             opaque pointer.  Half the map memory and half the bytes of a host-output call; the output kernel moves 8C + 2P
 *             bytes per map instead of 8C + 4P.  One-pass plans only: on a block-wise plan ("blockwise" > 0) a
 *             non-zero value fails with FFTCONV_ERR_INVALID_ARG -- its blocks are stored at fp32 element offsets, or summed,
 *             in the maps.  Also fftconv_plan_options.map_format; changing it forgets prepared kernels),
 *          "flip_kernels" (1: every kernel is flipped along h and w on the device before it is
 *             transformed, i.e. the plan correlates -- the "Flip Kernel (Required)" step of
 *             demoCudaConvolutionFFT.m:63-69 done here instead of in MATLAB; the reference keeps a
 *             conjugate-product variant commented out, src/cudaConvFFTData.cuh:42-45,63). */
int fftconv_plan_set_option(fftconv_plan *plan, const char *name, long value);
/* Every result map of the plan becomes rows [off_h, off_h + out_h) of columns [off_w, off_w + out_w) of the FFT_H x FFT_W
 * window, column-major and dense (pitch out_h), in the plan's "map_format", on every delivery route: a region of interest, a
 * strip per consumer, or "same" / "valid" for kernels smaller than MAX_KERNEL.  out_h, out_w >= 1, offsets >= 0 and the
 * rectangle inside the window, else FFTCONV_ERR_INVALID_ARG (the previous setting stays).  Acts like setting "output_region"
 * (which then reads 5): the plan's stream is synchronised, and plan_info.out_h / out_w / out_map_bytes follow.  On a one-pass
 * plan with the specialised output kernel and the tiled intermediate (kernel_path 0) that kernel stores the rectangle itself:
 * only the column tiles that hold a column of it are transformed, nothing but the rectangle is written (8C + 4P' bytes per
 * map for a rectangle of P' elements) and no full-window staging is allocated.  Every other plan -- generic or
 * Bluestein output kernel, kernel_path 1 or 2, block-wise, option "rect_store" 0, and the two specialised transforms whose rectangle
 * kernel is not built because it would spill registers (1088 and 4160 points along h: exact_window plans of the 1088- / 4160-row
 * windows) -- computes the window and crops it; read-only option "rect_direct" tells which. */
int fftconv_plan_set_output_rect(fftconv_plan *plan, int off_h, int off_w, int out_h, int out_w);
/* Strided result maps.  Let U be the out_h x out_w map the plan delivers without this entry -- the window, an "output_region" 1-3,
 * the rectangle of fftconv_plan_set_output_rect, the "same" map of a border mode.  With strides (stride_h, stride_w) every result
 * map is S[i, j] = U[i * stride_h, j * stride_w], i < ceil(out_h / stride_h), j < ceil(out_w / stride_w): column-major and dense,
 * in the plan's "map_format", image-major for image batches, on every delivery route -- the response at the stride of a coarse
 * search or of a feature map's cells, as conv2d(stride=) gives it.  The sampling grid starts at U's own first row and column
 * (another phase: fftconv_plan_set_output_rect); a stride larger than the extent gives one row or column.  plan_info.out_h /
 * out_w / out_map_bytes are those of S.  A stride < 1 is FFTCONV_ERR_INVALID_ARG, and so is a stride other than (1, 1) while
 * "output_region" is 4 (the pow2-padded window is not a sampling of the window), as is region 4 while a stride is set; the
 * previous setting stays.  Output-side state of its own: the plan's stream is synchronised, the image and the prepared kernels
 * stay, and the stride survives fftconv_plan_set_output_rect, "output_region", fftconv_plan_set_border, "map_format",
 * fftconv_plan_set_images and fftconv_plan_set_stream (the extents are recomputed); (1, 1) restores the dense maps exactly.  On a
 * one-pass plan with the specialised output kernel and the tiled intermediate (kernel_path 0), fp32 maps of the window or of a
 * rectangle and no score with a plane (scores 0 and 2), that kernel samples in its store: a column that is not sampled is neither
 * transformed in the last inverse stage nor stored, only tiles that hold a sampled column are launched, and the map store falls
 * from 4P to 4P / (stride_h * stride_w) bytes.  Everything else is STAGED -- 16-bit maps, scores 1, 3 and 4,
 * "output_region" 1-3, generic / Bluestein / kernel_path 1 or 2 output kernels, block-wise plans, the two transforms whose kernel
 * is not built (1088 and 4160 points along h), option "stride_store" 0: the output kernel stores the fp32 window into the plan's
 * staging and the crop samples it (a plane is read at the element's window coordinate).  Both routes return the same bits, those
 * of the dense maps sliced; read-only option "stride_direct" tells which.  The one-shot, two-step, fftconv_multi_*, plan-cache and
 * MEX entries do not take strides. */
int fftconv_plan_set_output_stride(fftconv_plan *plan, int stride_h, int stride_w);
/* Per-map extrema: the largest and the smallest element of every delivered map and where they lie, found on the device while the
 * maps are written -- what a caller of a matching score does with a map (the largest CCOEFF_NORMED / CCORR_NORMED / phase-correlation
 * value, the smallest SQDIFF) without reading the maps again.  The maps themselves are written exactly as without this entry.
 *   What a record covers.  After a convolve of B * n_kernel maps (image-major, as the maps are) record m describes delivered map m --
 *     the map as the caller receives it: the window, an "output_region" 1-4 (4: the padded map), a rectangle, a strided map, a
 *     border's "same" map.  The values come from the delivered element; for 16-bit maps that is the exact fp32 value of the rounded
 *     element.  `row` is the fast index and `col` the slow one of the delivered map: the element lies at col * out_h + row.
 *   Ties.  The element with the smallest col * out_h + row wins, for max and for min independently; +0 and -0 compare equal, and the
 *     value reported is that element's bits.
 *   NaN.  A NaN never wins (the compares are ordered); a map without an element that compares reports NaN and row = col = -1.
 *   No atomics.  The records are a pure function of the maps: two runs, both routes (below) and both tile deals ("dynamic_tiles")
 *     give identical records.
 *   Allocation.  fftconv_plan_set_extrema(plan, 1, max_maps) sizes the record buffer and every scratch the launches need, for
 *     convolves of up to max_maps maps; a convolve of more maps is refused with FFTCONV_ERR_INVALID_ARG and leaves the plan usable.  A
 *     convolve under extrema allocates nothing for them and does not wait for the host: it can be captured into a graph.
 *   Reading.  fftconv_plan_get_extrema waits for the plan's stream and copies the records [first_map, first_map + n_maps) of the
 *     last convolve to out_host; before any convolve under extrema, and for a range beyond the maps of the last one, it fails with
 *     FFTCONV_ERR_INVALID_ARG.  fftconv_plan_extrema_device gives the device array of max_maps records and its size: the pointer is
 *     stable until the next fftconv_plan_set_extrema or fftconv_plan_destroy, its content is ordered on the plan's stream.
 *   State.  Output-side state of its own, as the stride is: it keeps the image, the prepared kernels and the stream, and it stays
 *     while extent, format, score or images change; a call that changes nothing returns early, a change synchronises the plan's
 *     stream.  mode 0 switches it off and frees the buffers.
 *   Refusals (FFTCONV_ERR_INVALID_ARG, the plan's state untouched): a mode other than 0 / 1, max_maps < 1 with mode 1; mode 1 on a
 *     block-wise plan, whose maps are stored through output windows block by block.
 * Routes: on a one-pass plan with the specialised output kernel and the tiled intermediate, fp32 maps of the window or of a
 * rectangle, no stride -- raw maps and every score -- the output kernel finds the extrema in its store, while it holds the values in
 * registers (read-only option "extrema_direct" 1).  Everything else -- 16-bit maps, "output_region" 1-4, strides, generic / Bluestein
 * output kernels, kernel_path 1 or 2, the configurations whose kernel is not built, option "extrema_store" 0 -- is
 * SCANNED: a small kernel reads the delivered maps once more where they lie on the device, before any copy-out (4P' bytes per map
 * of P' elements).  Options: "extrema_store" (1 (default): fused where the plan can; 0: always the scan), read-only "extrema" (the
 * mode), "extrema_direct", "extrema_max_maps", "extrema_maps" (the maps of the last convolve under it; -1 before any).  The one-shot, two-step, fftconv_multi_*, plan-cache and MEX entries do not take it. */
typedef struct { float max_value; int max_row, max_col; float min_value; int min_row, min_col; } fftconv_extrema;
int fftconv_plan_set_extrema(fftconv_plan *plan, int mode, int max_maps);   /* mode 0 off, 1 on */
int fftconv_plan_get_extrema(fftconv_plan *plan, int first_map, int n_maps, fftconv_extrema *out_host);
int fftconv_plan_extrema_device(fftconv_plan *plan, void **device_ptr, size_t *bytes);
/* Peak lists: the thresholded local maxima of every delivered map, found on the device behind the kernel that writes the maps -- what a
 * matcher that looks for more than one instance does with a score map (threshold, non-maximum suppression, a list of (row, col,
 * score)), and what a registration caller does around the peak of a phase correlation (the shift to a fraction of a pixel), without
 * reading the maps again.  The maps themselves are written exactly as without this entry.
 *   Modes.  0 off.  1 maxima at or above `threshold` (CCOEFF_NORMED, CCORR_NORMED, phase correlation).  2 minima at or below
 *     `threshold` (SQDIFF): mode 1 on the negated values with the negated threshold; the record carries the element's own value.
 *   The element.  (value, index), index = col * out_h + row of the delivered map -- the map as the caller receives it: the window, an
 *     "output_region" 1-4, a rectangle, a strided map, a border's "same" map.  For 16-bit maps the value is the exact fp32 of the
 *     rounded element.  `row` is the fast index.
 *   A peak (mode 1).  An element v at (r, c) with v >= threshold that no other element of its neighbourhood beats; the neighbourhood is
 *     rows r +- radius_h and columns c +- radius_w, clipped to the map.  The compare is ordered: a NaN is never a peak and never
 *     beats anything.  "Beats" is the tie rule of the extrema: a larger value, or an equal value at a smaller index; +0 and -0
 *     compare equal.  A plateau of equal values therefore yields exactly one peak per neighbourhood chain -- an all-equal map with a
 *     radius >= 1 has one peak, at index 0.  With radius (0, 0) every element that meets the threshold is a peak: plain thresholding.
 *   Sub-pixel offsets.  d_row and d_col are a three-point parabola per dimension, computed in float64 from the exact element values
 *     and rounded to fp32 once: along rows a = U[r-1, c], b = U[r+1, c], den = (a - v) + (b - v), d = 0.5 * (a - b) / den, clamped to
 *     [-0.5, 0.5]; 0 where the neighbour pair does not exist (a map edge), where a, b or v is not finite, where den == 0, and where
 *     the radius of that dimension is 0.  Columns likewise.  The peak lies at (row + d_row, col + d_col).
 *   What a convolve leaves.  Per delivered map m (image-major, numbered as the extrema records are): found[m], the number of peaks of
 *     the map, all of them; the first min(found[m], max_peaks) peaks in ascending index order (memory order) from
 *     peaks[m * max_peaks] on.  Records beyond that are undefined; nothing is cleared.  Overflow is not an error: the caller sees
 *     found[m] > max_peaks and raises the threshold.
 *   No atomics.  The lists are a pure function of the maps: two runs, both tile deals ("dynamic_tiles") and every delivery route give
 *     identical bytes.
 *   Allocation.  The setter sizes found, peaks and every scratch of a launch, for convolves of up to max_maps maps; a convolve of more
 *     maps is refused with FFTCONV_ERR_INVALID_ARG and leaves the plan usable.  A convolve under it allocates nothing, does not
 *     wait for the host and can be captured into a graph.  A change of threshold, radius or mode alone keeps the buffers (it
 *     synchronises the plan's stream, and the lists of the last convolve are no longer readable: they belong to the rule they were
 *     found under).
 *   Reading.  fftconv_plan_get_peaks waits for the plan's stream and copies found[first_map .. first_map + n_maps) to found_host and
 *     the n_maps * max_peaks records to peaks_host (map m's start at (m - first_map) * max_peaks); before any convolve under peaks,
 *     and for a range beyond the maps of the last one, it fails with FFTCONV_ERR_INVALID_ARG.  fftconv_plan_peaks_device gives the
 *     device arrays (max_maps ints; max_maps * max_peaks records and their size in bytes): stable until the next call that changes
 *     max_maps or max_peaks or switches the lists off, their content ordered on the plan's stream.
 *   State.  Output-side state of its own, beside the stride and the extrema, and independent of the extrema (both may be on): it
 *     keeps the image, the prepared kernels, the stream and the extent, and it stays while format, score, extent or images change; a
 *     call that changes nothing returns early.
 *   Refusals (FFTCONV_ERR_INVALID_ARG, the plan's state untouched): a mode outside 0..2; with a mode on, max_maps < 1, max_peaks < 1, a
 *     NaN threshold (+-inf are allowed), a negative radius (a radius larger than the map is simply clipped); a mode on on a
 *     block-wise plan, whose maps are stored through output windows block by block.
 *   Cost.  Three small launches behind every output launch: a pass that reads the delivered maps once more where they lie (4P' bytes
 *     per map of P' elements, 2P' for 16-bit maps) and walks the neighbourhood of the elements that meet the threshold alone; a scan
 *     of the per-wave counts; a pass that re-reads the runs that hold peaks.  A threshold of -inf with a large radius makes every
 *     element a candidate: the cost then grows with P' * (2 radius_h + 1) * (2 radius_w + 1).  That is the caller's choice and is
 *     not optimised.
 * Read-only options: "peaks" (the mode), "peaks_max_maps", "peaks_max", "peaks_radius_h", "peaks_radius_w", "peaks_maps" (the maps of
 * the last convolve under it; -1 before any).  There is no creation option.  The one-shot, two-step, fftconv_multi_*, plan-cache
 * and MEX entries do not take it. */
typedef struct { float value; int row, col; float d_row, d_col; } fftconv_peak;   /* 20 bytes */
int fftconv_plan_set_peaks(fftconv_plan *plan, int mode, int max_maps, int max_peaks,
                           float threshold, int radius_h, int radius_w);
int fftconv_plan_get_peaks(fftconv_plan *plan, int first_map, int n_maps, int *found_host, fftconv_peak *peaks_host);
int fftconv_plan_peaks_device(fftconv_plan *plan, void **found_device, void **peaks_device, size_t *peaks_bytes);
/* Normalised cross-correlation maps.  mode 0 (default): the maps are the raw sums of products, bit for bit what they are
 * without this entry.  mode 1: every map is the zero-mean normalised cross-correlation (MATLAB's normxcorr2, OpenCV's
 * TM_CCOEFF_NORMED) over the box box_h x box_w, n = box_h * box_w: in [-1, 1], 1 at a perfect match, invariant to gain and
 * offset of the kernel everywhere and of the image wherever the box lies wholly inside the data (rows >= box_h - 1 and columns
 * >= box_w - 1 of the window, up to the data's last: the "valid" part).  The padding is zero whatever the image's offset, so a
 * box that reaches into it sees the offset as an edge; gain alone is invariant everywhere.  With the zero-padded image I (zero outside the data) and, per feature plane f, the sums s1_f(u) /
 * s2_f(u) of I / I^2 over the box_h x box_w pixels that element u of the FFT_H x FFT_W window sums over:
 *     den2(u) = sum_f (s2_f - s1_f^2 / n),   e(u) = sum_f s2_f,
 *     D(u)    = 0 where den2(u) <= 2^-30 e(u) (a window flat to within 2^-15 of its RMS; every window wholly in the padding),
 *               else den2(u)^(-1/2), rounded once to fp32,
 *     T''     = the kernel minus its per-plane mean, divided by the joint norm of what is left (all zeros for a constant kernel),
 *     map_k(u) = D(u) * (I (*) T''_k)(u)          ("flip_kernels" decides convolution or correlation as ever; D is the same).
 * D is computed once per image by fftconv_plan_set_image / _set_images beside the forward transform (float64 direct sums, in
 * strips of columns: 32 MiB of transient scratch, or the 16 * F * FFT_H * box_w bytes of a strip of ONE window column where that is
 * more -- F * FFT_H * box_w > 2^21, e.g. F = 4 with 4224 rows and a 127-wide box: 34.3 MB), T'' once per kernel ahead of its transform (float64), on the device
 * for every kernel location.  The multiply by D is FUSED into the store of the specialised output kernel where the plan runs it
 * on the tiled intermediate (kernel_path 0) and stores fp32 maps of the window or of a rectangle: 8C + 4P + 4P bytes per map,
 * the read of D included.  Everything else is STAGED -- 16-bit maps, "output_region" 1-4, generic / Bluestein /
 * kernel_path 1 or 2 output kernels, the two transforms whose fused kernel is not built (1088 and 4160 points along h), option
 * "norm_store" 0: the output kernel stores the fp32 window into the plan's staging and the crop / pad kernel multiplies by D at
 * the window coordinate while it crops and converts, one extra pass.  Both routes return the same bits; every "map_format",
 * "output_region", rectangle, delivery route and image batch composes (read-only option "rect_direct" reads 0 meanwhile).
 * Options: "norm_store" (1 (default): fused where possible; 0: always staged), read-only "norm_direct" (1 if, with the plan's
 * current settings, the output kernel itself will scale).  Placement tuning does not run while mode 1 is on; an intermediate
 * allocated meanwhile is tuned by the first convolve after mode 0, as a fresh plan's is.  plan_info.workspace_bytes counts D, T''
 * and the float64 scratch.
 * While mode 1 is on EVERY kernel must be exactly box_h x box_w (1 <= box <= MAX_KERNEL per dimension).
 * Acts like fftconv_plan_set_output_rect: the plan's stream is synchronised and prepared kernels are forgotten.  A call that
 * changes mode or box leaves the plan WITHOUT an image (option "images" reads 0, a convolve fails with FFTCONV_ERR_NO_IMAGE): D
 * belongs to (image, box), and the pixels are gone once set_image has returned.  A call that changes nothing keeps the image.
 * Read-only options beside it: "normalise", "norm_box_h", "norm_box_w".
 * FFTCONV_ERR_INVALID_ARG, the plan's state untouched: a bad mode or box; a block-wise plan ("blockwise" > 0); while mode 1 is
 * on, a convolve or prepare whose kernels are not exactly box_h x box_w (ragged cells included), and
 * fftconv_plan_import_spectrum / fftconv_plan_mark_spectrum_valid (a spectrum carries no window statistics).
 * The one-shot and two-step entries, fftconv_multi_*, the plan cache and the MEX gateways do not take the option. */
int fftconv_plan_set_normalisation(fftconv_plan *plan, int mode, int box_h, int box_w);
/* Template-matching scores: the map of a kernel (template) T of F planes of box_h x box_w, n = box_h * box_w, as one of the scores
 * a matcher chooses from.  ONE state with fftconv_plan_set_normalisation: mode 1 there is score 1 here, and either entry reads
 * and replaces what the other set.  Notation: I is the zero-padded image; R(u) = sum_f (I_f (*) T_f)(u) is the plan's raw map --
 * convolution, or correlation with "flip_kernels" 1; the scores below are then those of the flipped template, exactly as mode 1
 * handles it; s2_f(u) is the float64 direct sum of I_f^2 over the box that ends at window position u (the sums and the fixed
 * order of mode 1); E(u) = sum_f s2_f(u); t2 = sum_f sum T_f^2, taken in float64 in the fixed lane order of the kernel
 * normalisation.
 *   score                   value of a map                               kernel preparation           per-image plane     store
 *   0 FFTCONV_SCORE_NONE          raw (as without this entry)                  none                         none                plain
 *   1 FFTCONV_SCORE_CCOEFF_NORMED exactly mode 1 of fftconv_plan_set_normalisation   T''                    D                   x * D
 *   2 FFTCONV_SCORE_CCOEFF        sum_f I_f (*) (T_f - mean(T_f))              centred per plane, not scaled   none             plain
 *   3 FFTCONV_SCORE_CCORR_NORMED  R(u) * E(u)^(-1/2), and 0 where E(u) = 0     T / sqrt(t2) (not centred; all zeros where t2 = 0)
 *                                                                                                       Dc = (float) E^(-1/2), 0 where E == 0   x * Dc
 *   4 FFTCONV_SCORE_SQDIFF        E(u) - 2 R(u) + t2 = sum_f sum_box (I - T)^2  -2 * T (exact in fp32)       Q = (float) E       x + (Q(u) + c_k), c_k = (float) t2
 * Score 2 equals OpenCV's TM_CCOEFF wherever the box lies inside the data (sum (I - mean_u I)(T - mean T) = sum I (T - mean T)).
 * Score 3 has no relative floor: E is a sum of non-negative float64 terms, so it is exactly 0 if and only if every pixel under the
 * box is 0, and otherwise it is accurate to a relative 2^-52.  Score 4 is always evaluated in one fixed order -- first s = Q + c_k,
 * one fp32 add, then x + s, one fp32 add -- on every route.  Where no data lies under the box (the slack of the window behind
 * DATA + box - 1) score 4 returns t2, the true sum of squared differences against zeros, and score 3 returns 0; what an
 * "output_region" 4 adds beyond the window is 0, as for every map.
 * The kernels are prepared on the device in float64 ahead of their transform, for every kernel location; the planes are computed
 * once per image by fftconv_plan_set_image / _set_images beside the forward transform, as D is.  Score 2 is a kernel preparation
 * and nothing else: no statistics, no plane, and its maps are delivered exactly as raw maps are ("rect_direct", 16-bit maps,
 * regions; "norm_direct" reads 0).  Scores 3 and 4 are combined in the store of the specialised output kernel under the conditions
 * of mode 1 (score 3 by mode 1's kernels with Dc in D's place; score 4 by kernels of its own, built for every transform but the
 * 1088- and 4160-point ones) and in the staged crop / pad everywhere else; both routes return the same bits.  "norm_store" and
 * "norm_direct" keep their meaning for every score.  plan_info.workspace_bytes counts the planes, the prepared kernels and their
 * constants.
 * The rules are those of fftconv_plan_set_normalisation, for every score, 2 included: a call that changes score or box leaves the
 * plan without an image, one that changes nothing keeps it; while a score is on EVERY kernel must be exactly box_h x box_w.
 * Read-only options: "match_score"; "normalise" (1 exactly when the score is 1); "norm_box_h", "norm_box_w" (the box of any score).
 * FFTCONV_ERR_INVALID_ARG, the plan's state untouched: a bad score or box; a block-wise plan; a border being on (and
 * fftconv_plan_set_border while any score is on); kernels of another size; fftconv_plan_import_spectrum /
 * fftconv_plan_mark_spectrum_valid under scores 1, 3 and 4, which carry window statistics (allowed under 0 and 2).
 * The one-shot and two-step entries, fftconv_multi_*, the plan cache and the MEX gateways do not take the option. */
enum { FFTCONV_SCORE_NONE = 0, FFTCONV_SCORE_CCOEFF_NORMED = 1, FFTCONV_SCORE_CCOEFF = 2, FFTCONV_SCORE_CCORR_NORMED = 3, FFTCONV_SCORE_SQDIFF = 4 };
int fftconv_plan_set_match_score(fftconv_plan *plan, int score, int box_h, int box_w);

/* Border modes: what the image is beyond its data.  The library's own border is zero; a caller who wanted another one had to
 * write a padded copy of every image, plan for the padded size and crop the rim.  Here the border is never materialised: the
 * loads of the forward column pass map the indices.  An image extended by MAX_KERNEL - 1 samples per dimension is exactly
 * DATA + MAX_KERNEL - 1 long -- the window every plan already transforms -- so a bordered map costs no larger transform.
 *     mode                          beyond the data, 1-D, data a b c d
 *     0 FFTCONV_BORDER_ZERO         the library as it is without this entry (default); every bit unchanged
 *     1 FFTCONV_BORDER_CONSTANT     v v | a b c d | v v      (`value`, finite; ignored by the other modes)
 *     2 FFTCONV_BORDER_REPLICATE    a a | a b c d | d d
 *     3 FFTCONV_BORDER_SYMMETRIC    b a | a b c d | d c      (MATLAB 'symmetric', numpy 'symmetric', OpenCV BORDER_REFLECT)
 *     4 FFTCONV_BORDER_REFLECT101   c b | a b c d | c b      (numpy 'reflect', OpenCV's default)
 *     5 FFTCONV_BORDER_CIRCULAR     c d | a b c d | a b      (MATLAB 'circular', numpy 'wrap')
 * Per dimension X in {H, W}: lead_X = MAX_KERNEL_X / 2 (integer division), trail_X = MAX_KERNEL_X - 1 - lead_X, c_X =
 * (MAX_KERNEL_X - 1) / 2 (= trail_X).  With Iext the image extended by the mode over all integers, modes 1-5 define every map
 * as the H x W "same" map anchored on the plan's MAX_KERNEL box:
 *     map_k[i, j] = sum_f sum_{a < kh, b < kw} Iext_f[i + c_H - a, j + c_W - b] * K_{k,f}[a, b]
 * -- the centred "same" map for a kernel of exactly MAX_KERNEL_H x MAX_KERNEL_W; a smaller kernel (ragged cells included) sits
 * at the top-left of the MAX_KERNEL box; "flip_kernels" decides convolution or correlation as ever, inside the kernel's own
 * kh x kw.  In window coordinates the forward pass transforms E[r, c] = Iext[r - lead_H, c - lead_W] for r < H + MAX_KERNEL_H - 1,
 * c < W + MAX_KERNEL_W - 1 (zeros beyond, up to the transform length), and the map is rows [MAX_KERNEL_H - 1, MAX_KERNEL_H - 1
 * + H) of columns [MAX_KERNEL_W - 1, MAX_KERNEL_W - 1 + W) of the window; everything outside that rectangle holds the cyclic
 * wrap and partial sums and is unspecified.
 * A mode other than 0 installs exactly that rectangle, as fftconv_plan_set_output_rect(MAX_KERNEL_H - 1, MAX_KERNEL_W - 1, H, W)
 * does: the plan's stream is synchronised, prepared kernels are forgotten, "rect_direct" and the store form are decided as for
 * any rectangle.  Afterwards the caller may set any other rectangle inside that one (a region of interest, in window
 * coordinates).  Mode 0 restores "output_region" 0.  A call that changes mode or value leaves the plan WITHOUT an image (option
 * "images" reads 0, a convolve fails with FFTCONV_ERR_NO_IMAGE): the spectrum belongs to (image, border).  A call that changes
 * nothing keeps the image and the rectangle.
 * Routes.  Direct: on a one-pass plan whose image column pass is the specialised kernel ("specialised_kernels" bit 1) that kernel
 * maps rows and columns in its load (compares and selects; a CONSTANT sample outside the data is not loaded).  Staged: everywhere
 * else (generic and Bluestein / exact_window column passes, kernel_path 1) and with option "border_store" 0 one small kernel
 * writes the extended image into the plan's staging and the column pass runs on that.  Both routes return the same bits.
 * Image batches compose (B * F planes).  A typed image (fftconv_plan_set_images_typed) is converted into the fp32 staging first
 * and takes the border route from there ("pixel_direct" reads 0 meanwhile).  "defer_prepare" merges a recorded preparation with
 * the column pass of zero-border images only: a bordered image launches the pending kernels' column pass by itself first.  A
 * warm device-resident call allocates nothing, never synchronises and can be captured into a graph.
 * plan_info.workspace_bytes counts the staging of the extended image.
 * Options: "border_store" (1 (default): direct where possible; 0: always staged -- takes effect at the next image), read-only
 * "border_direct" (1 if the next image on this plan, with the options as they are, is mapped in the column kernel's load),
 * "border_mode", "border_lead_h", "border_lead_w" (lead_X while a border is on, else 0).
 * Folds are single.  FFTCONV_ERR_INVALID_ARG, the plan's state untouched: a mode outside 0..5; a value that is not finite; modes
 * 3 and 5 where MAX_KERNEL_X / 2 > DATA_X; mode 4 where MAX_KERNEL_X / 2 > DATA_X - 1; a block-wise plan ("blockwise" > 0); a plan
 * with normalisation on -- likewise fftconv_plan_set_normalisation(1, ...) while a border is on (the window statistics assume
 * zero padding) -- and fftconv_plan_import_spectrum / fftconv_plan_mark_spectrum_valid while a border is on (a foreign spectrum
 * carries no border).
 * The one-shot and two-step entries, fftconv_multi_*, the plan cache and the MEX gateways do not take the option. */
enum { FFTCONV_BORDER_ZERO = 0, FFTCONV_BORDER_CONSTANT = 1, FFTCONV_BORDER_REPLICATE = 2, FFTCONV_BORDER_SYMMETRIC = 3,
       FFTCONV_BORDER_REFLECT101 = 4, FFTCONV_BORDER_CIRCULAR = 5 };
int fftconv_plan_set_border(fftconv_plan *plan, int mode, float value);
/* Spectral filters: what happens to every bin between the forward and the inverse transform.  Let L_h x L_w be the plan's
 * transform lengths (fftconv_plan_info.transform_h / transform_w), I^ the unnormalised L_h x L_w DFT of the window the plan
 * transforms -- the zero-padded image, or the bordered extension while a border is on -- and K^_k the DFT of kernel k as the plan
 * places it: at the origin, after "flip_kernels".  IDFT is the normalised inverse (numpy's ifft2).  Every map is the
 * FFT_H x FFT_W window (rows < fft_h, columns < fft_w) of
 *     mode 0 FFTCONV_FILTER_PRODUCT   IDFT(I^ . K^_k)                           the library as it is, every bit unchanged (default)
 *     mode 1 FFTCONV_FILTER_PHASE     IDFT(P / |P|),  P = I^ . K^_k             and 0 in a bin where P is zero
 *     mode 2 FFTCONV_FILTER_WIENER    IDFT(I^ . conj(K^_k) / (|K^_k|^2 + lambda))   and 0 in a bin where the denominator is zero
 * and everything downstream of it -- "output_region", rectangle, stride, "map_format", delivery -- works as ever.
 * Mode 1 is phase correlation (skimage's phase_cross_correlation, OpenCV's phaseCorrelate): it ignores illumination and contrast.
 * `param` must be 0 (reserved for a regulariser).  A pure cyclic shift gives a peak of height 1.  With "flip_kernels" 1 the
 * zero-shift peak of a template cut from the image at (y0, x0) lies at (y0 + kh - 1, x0 + kw - 1), as the raw correlation's
 * does; all shifts lie inside the window whatever L is.
 * Mode 2 is the Wiener / regularised inverse filter (deconvolution with a known point-spread function; the response of a
 * correlation filter): lambda = param >= 0, finite, in the units of |K^|^2 of the UNNORMALISED DFT.
 * The arithmetic is fp32 with the hardware's reciprocal and reciprocal square root (1 ulp); "zero" above means below the smallest
 * normal fp32 number in the kernel's own scaling (|P|^2 / (L_h L_w)^2 for mode 1, |K^|^2 + lambda for mode 2).
 * Unlike mode 0, modes 1 and 2 depend on the cyclic modulus: a default plan may transform a longer length than its window (1152
 * points for a 1088 window), and the filter is defined on THAT length.  A caller who needs the window itself as the modulus
 * creates the plan with fftconv_plan_options.exact_window = 1.
 * The setter changes spectral-row launches only: it keeps the image or images, the prepared kernels
 * (fftconv_plan_prepare_kernels_packed, deferred preparation, the column cache), the stream, the rectangle, the stride and the
 * format, allocates nothing and does not synchronise.  A warm device-resident convolve under a mode never synchronises and can
 * be captured into a graph.  A call that changes nothing is a no-op.  The filter runs in the product phase of the spectral-row
 * kernel: the specialised one in an instantiation of its own per (length, kernel width class) that serves all modes, the generic
 * and Bluestein one (kernel_path 1, exact_window windows that do not factor) behind a uniform branch.  While a mode is on,
 * "image_walk_active" reads 0 and image batches keep the walk over kernels.
 * Read-only options: "spectral_filter" (the mode), "spectral_filter_fast" (1 if the next spectral-row launch of this plan under
 * the mode runs the specialised filter kernel).
 * FFTCONV_ERR_INVALID_ARG, the plan's state untouched: a mode outside 0..2; a param that is not finite, negative, or non-zero in
 * mode 1 (mode 0 ignores a valid one); modes 1 and 2 with feature_dim > 1 (the filter of a feature sum is another formula), on a block-wise plan, on a
 * plan with normalisation or a matching score on -- likewise fftconv_plan_set_normalisation / fftconv_plan_set_match_score with a
 * non-zero mode while a filter is on -- and on a plan whose specialised row length has no filter kernel because it would spill
 * registers (7040 points along w: create such a plan with kernel_path 1).
 * The one-shot and two-step entries, fftconv_multi_*, the plan cache and the MEX gateways do not take the option. */
enum { FFTCONV_FILTER_PRODUCT = 0, FFTCONV_FILTER_PHASE = 1, FFTCONV_FILTER_WIENER = 2 };
int fftconv_plan_set_spectral_filter(fftconv_plan *plan, int mode, float param);
/* Current value of an option, plus read-only ones: "tuned_candidates" (allocations tried by the last placement tuning)
 * and "tuned_best" (index of the one kept), "blockwise" (blocks of a block-wise plan, 0 = one pass), "overlap_save" (1: the blocks are stored by the output kernel),
 * "rows_slots_per_cu" (workgroups of the multi-map row kernel a CU holds at once: what the walk length is chosen for),
 * "specialised_kernels" (bit 0: the spectral-row pass runs on a specialised kernel, bit 1: the column passes do; 3 = no
 * generic kernel runs for this plan), "images" (images the plan holds: fftconv_plan_set_images' n_images, 1 after
 * fftconv_plan_set_image, 0 before any image). */
int fftconv_plan_get_option(fftconv_plan *plan, const char *name, long *value);

typedef struct fftconv_profile {
    /* accumulated since the last reset; index 0 kernel_cols (h forward of the kernels),
     * 1 spectral_rows, 2 cols_c2r (output), 3 image_cols, 4 image_rows */
    double ms[5];
    long launches[5];
    long units[5];  /* kernels (maps) processed by those launches */
} fftconv_profile;
int fftconv_plan_get_profile(fftconv_plan *plan, fftconv_profile *prof, int reset);

/* ------------------------------------------------------------------------------------------
 * Two-step API of the reference, as thin aliases of the plan API:
 *   fftData = cudaFFTData(data, kernelH, kernelW)        src/cudaFFTData.cu:18-160
 *   cvcell  = cudaConvFFTData(fftData, kernelCell[, threadSize])  src/cudaConvFFTData.cu:24-306
 * The handle plays the role of the complex gpuArray the reference returns.
 * ------------------------------------------------------------------------------------------ */
int fftconv_fft_data(const float *data, int data_h, int data_w, int feature_dim,
                     int kernel_h, int kernel_w, int gpu_id, fftconv_plan **fft_data);
/* (kernels of fftconv_conv_fft_data: host arrays or device-resident ones, told apart by the HIP
 *  runtime -- FFTCONV_AUTO -- as src/cudaConvFFTData.cu accepts gpuArray cells too) */
int fftconv_conv_fft_data(fftconv_plan *fft_data, int n_kernel, const float *const *kernels,
                          const int *kernel_h, const int *kernel_w, const int *kernel_f,
                          const double *thread_size, int n_thread_size, float *const *out);

/* ------------------------------------------------------------------------------------------
 * Several GPUs from one process: the reference's multi-GPU / multi-stream sketch
 * (src/cudaConvFFTDataStreams.cu -- one ConvPlan per (GPU, stream) with private scratch :273-328,
 * the image spectrum copied from GPU 0 to GPU g with cudaMemcpyPeerAsync :279-289, kernels dealt
 * over the plans :338-447, a synchronisation barrier at the end :452-468; it never built or ran).
 * Here: one plan and one stream per listed device, the image transformed once on devices[0], its
 * spectrum copied to every other device over xGMI (hipMemcpyPeerAsync, each copy on the
 * destination's stream so that the links work in parallel), the kernels dealt in CONTIGUOUS
 * blocks (device g of n takes kernels [g*N/n, (g+1)*N/n), sizes differing by at most one), one
 * host thread per device while a call runs, everything complete on return.  The same device may
 * be listed more than once (two plans on one GPU: the reference's N_BATCH_PER_GPU = 2).
 * With one process per GPU (torch.distributed / RCCL) use the plan API and broadcast the
 * spectrum buffer instead: INTEGRATION.md.
 * ------------------------------------------------------------------------------------------ */
typedef struct fftconv_multi fftconv_multi;
int fftconv_multi_create(fftconv_multi **multi, int data_h, int data_w, int feature_dim,
                         int max_kernel_h, int max_kernel_w, const int *devices, int n_devices,
                         const fftconv_plan_options *options);
int fftconv_multi_destroy(fftconv_multi *multi);
/* After a successful fftconv_multi_create, fftconv_last_error() is "" -- or a warning naming the devices that have
 * no direct (xGMI peer) access to devices[0]: copies to those are staged by the runtime (slower, still correct).
 * Options: "spectrum_transport" 0 (default) = the reference's form, one peer copy per destination
 *             (src/cudaConvFFTDataStreams.cu:282-287); 1 = ONE collective: ncclBroadcast of the spectrum buffer over a
 *             communicator of the listed devices (RCCL over xGMI; librccl.so is loaded on first use, the devices must
 *             be distinct).  Where RCCL cannot be set up the copies are used and fftconv_last_error() says why;
 *          "verbose" 1 = what happens, to stderr (also sets every plan's "verbose").
 * Read-only: "transport_used" (what the last set_image / import_spectrum used), "peer_direct" (destinations with
 * direct access to devices[0]). */
int fftconv_multi_set_option(fftconv_multi *multi, const char *name, long value);
int fftconv_multi_get_option(const fftconv_multi *multi, const char *name, long *value);
/* padData + cufftExecR2C of the image on devices[0] (src/cudaConvolutionFFT.cu:144-169), then the
 * peer copies.  location FFTCONV_HOST, or FFTCONV_DEVICE for memory of devices[0]. */
int fftconv_multi_set_image(fftconv_multi *multi, const float *data, int location);
/* Instead of an image: its spectrum in the reference's order (fftconv_plan_import_spectrum; the handle
 * must have been created with fftconv_plan_options.exact_window = 1) -- what the reference's
 * multi-GPU MEX takes as its first argument (src/cudaConvFFTDataStreams.cu:160-187). */
int fftconv_multi_import_spectrum(fftconv_multi *multi, const float *spectrum, int location);
/* The per-kernel loop over all devices.  FFTCONV_HOST kernels / outputs are plain host arrays;
 * FFTCONV_DEVICE pointers must live on the device that owns the kernel (fftconv_multi_shard). */
int fftconv_multi_convolve(fftconv_multi *multi, int n_kernel, const float *const *kernels,
                           const int *kernel_h, const int *kernel_w, int kernel_location,
                           float *const *out, int out_location);
/* Block of kernels device `index` (position in devices[]) owns among n_kernel. */
int fftconv_multi_shard(const fftconv_multi *multi, int n_kernel, int index, int *first, int *count);
/* Number of plans, and the plan / device id at a position (for fftconv_plan_get_info, options,
 * or packed device-resident calls on one device; the plan stays owned by the multi handle). */
int fftconv_multi_size(const fftconv_multi *multi);
int fftconv_multi_plan(fftconv_multi *multi, int index, fftconv_plan **plan, int *device);
/* One-shot form: fftconv_convolution_fft with a list of devices instead of one gpu_id. */
int fftconv_convolution_fft_multi(const float *data, int data_h, int data_w, int feature_dim,
                                  int max_kernel_h, int max_kernel_w,
                                  int n_kernel, const float *const *kernels,
                                  const int *kernel_h, const int *kernel_w, const int *kernel_f,
                                  const int *devices, int n_devices,
                                  float *const *out, int *fft_h, int *fft_w);

#ifdef __cplusplus
}
#endif
#endif /* FFTCONV_H */
