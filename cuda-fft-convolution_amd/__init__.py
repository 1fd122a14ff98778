"""Python binding of libfftconv.so, the MI355X-native 2-D FFT-convolution engine.

The host side of the product is C++ (``csrc/fftconv_api.cpp`` and the units beside it (``csrc/plan_internal.hpp`` lists them), the role of the reference's MEX
gateways); this module is only the ctypes stub over the C ABI of ``include/fftconv.h`` plus a
mirror of the reference's MATLAB call surface so tests read like the reference's demo:

    cvcell  = cudaConvolutionFFT(data, maxKH, maxKW, kernelCell[, threads4][, gpuId])
              (reference: src/cudaConvolutionFFT.cu:27-311, demoCudaConvolutionFFT.m:124-129)
    fftData = cudaFFTData(data, kH, kW)                 (src/cudaFFTData.cu:18-160)
    cvcell  = cudaConvFFTData(fftData, kernelCell[, threads4])   (src/cudaConvFFTData.cu:24-306)

Arrays follow MATLAB conventions: ``data`` is H x W x F, kernels are kh x kw x F, every result is
the full FFT_H x FFT_W window (not cropped).  There is no CPU fallback: if the HIP library is
missing or no GPU is present the compute calls raise.

Environment (this stub only; libfftconv.so itself reads none): FFTCONV_LIB = path of an alternate
build of the library (A/B runs, tools/build_variant.sh); FFTCONV_NO_TORCH_RUNTIME = 1 skips the
preload of PyTorch's bundled HIP runtime (see _preload_hip_runtime).
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FFTCONV_LIB") or os.path.join(_HERE, "libfftconv.so")  # FFTCONV_LIB: kernel experiments

HOST, DEVICE, AUTO = 0, 1, 2
MEX_ERROR_ID = "cudaConvFFTData:InvalidInput"  # src/cudaConvolutionFFT.cu:30


class FFTConvError(RuntimeError):
    """Raised for any negative status of the C ABI; ``.status`` holds the code and ``.identifier``
    the MEX error id the reference raises for argument errors."""

    def __init__(self, status, message):
        super().__init__("fftconv status %d: %s" % (status, message))
        self.status = status
        self.identifier = MEX_ERROR_ID


class PlanInfo(ctypes.Structure):
    _fields_ = [
        ("data_h", ctypes.c_int), ("data_w", ctypes.c_int), ("feature_dim", ctypes.c_int),
        ("max_kernel_h", ctypes.c_int), ("max_kernel_w", ctypes.c_int),
        ("fft_h", ctypes.c_int), ("fft_w", ctypes.c_int),
        ("transform_h", ctypes.c_int), ("transform_w", ctypes.c_int),
        ("spectrum_rows", ctypes.c_int), ("spectrum_pitch", ctypes.c_int),
        ("gpu_id", ctypes.c_int), ("exact_window", ctypes.c_int),
        ("spectrum_bytes", ctypes.c_size_t), ("map_bytes", ctypes.c_size_t),
        ("workspace_bytes", ctypes.c_size_t),
        ("out_h", ctypes.c_int), ("out_w", ctypes.c_int), ("out_map_bytes", ctypes.c_size_t),
    ]


class PlanOptions(ctypes.Structure):
    """fftconv_plan_options (include/fftconv.h): choices fixed at plan creation."""
    _fields_ = [("struct_size", ctypes.c_size_t), ("kernel_path", ctypes.c_int), ("rows_group", ctypes.c_int),
                ("max_transform", ctypes.c_int), ("exact_window", ctypes.c_int), ("blockwise", ctypes.c_int),
                ("verbose", ctypes.c_int), ("map_format", ctypes.c_int)]

    def __init__(self, kernel_path=0, rows_group=0, max_transform=0, exact_window=0, blockwise=0, verbose=0, map_format=0):
        super().__init__(ctypes.sizeof(PlanOptions), int(kernel_path), int(rows_group), int(max_transform), int(exact_window), int(blockwise),
                         int(verbose), int(map_format))


# Element format of the result maps (plan option / PlanOptions field "map_format") and the NumPy dtype a host map comes back in.
# NumPy has no bfloat16: those maps are uint16 arrays of bfloat16 BIT PATTERNS (a float32 view: ``a.astype(np.uint32) << 16``
# viewed as float32; torch: ``torch.from_numpy(a).view(torch.bfloat16)``).
MAP_F32, MAP_F16, MAP_BF16 = 0, 1, 2
MAP_DTYPES = {MAP_F32: np.dtype(np.float32), MAP_F16: np.dtype(np.float16), MAP_BF16: np.dtype(np.uint16)}


# Element format of typed image pixels (Plan.set_images_typed / fftconv_plan_set_images_typed): the value of a pixel is its exact
# float32 conversion, no implied gain.  The format follows from the NumPy dtype; bfloat16 has none -- a uint16 array of bit
# patterns with pixel_format=PIXEL_BF16 given explicitly.
PIXEL_F32, PIXEL_U8, PIXEL_U16, PIXEL_F16, PIXEL_BF16 = 0, 1, 2, 3, 4
PIXEL_DTYPES = {PIXEL_F32: np.dtype(np.float32), PIXEL_U8: np.dtype(np.uint8), PIXEL_U16: np.dtype(np.uint16), PIXEL_F16: np.dtype(np.float16),
                PIXEL_BF16: np.dtype(np.uint16)}
_PIXEL_OF_DTYPE = {np.dtype(np.uint8): PIXEL_U8, np.dtype(np.uint16): PIXEL_U16, np.dtype(np.float16): PIXEL_F16}


# Border modes (Plan.set_border / fftconv_plan_set_border): what the image is beyond its data.  NumPy's np.pad modes of the same
# extension: constant, edge, symmetric, reflect, wrap.
# matching scores (Plan.set_match_score; FFTCONV_SCORE_* of include/fftconv.h)
SCORE_NONE, SCORE_CCOEFF_NORMED, SCORE_CCOEFF, SCORE_CCORR_NORMED, SCORE_SQDIFF = 0, 1, 2, 3, 4
# spectral filters (Plan.set_spectral_filter; FFTCONV_FILTER_* of include/fftconv.h)
FILTER_PRODUCT, FILTER_PHASE, FILTER_WIENER = 0, 1, 2
# fftconv_plan_set_peaks modes
PEAKS_OFF, PEAKS_MAX, PEAKS_MIN = 0, 1, 2
BORDER_ZERO, BORDER_CONSTANT, BORDER_REPLICATE, BORDER_SYMMETRIC, BORDER_REFLECT101, BORDER_CIRCULAR = 0, 1, 2, 3, 4, 5


def _options_map_dtype(options):
    """dtype of the maps a one-shot call with these options returns"""
    if options is None:
        return MAP_DTYPES[MAP_F32]
    fmt = options.get("map_format", 0) if isinstance(options, dict) else options.map_format
    if int(fmt) not in MAP_DTYPES:
        raise FFTConvError(-1, "map_format is 0 (fp32), 1 (fp16) or 2 (bfloat16)")
    return MAP_DTYPES[int(fmt)]


class CallTiming(ctypes.Structure):
    """fftconv_call_timing: where the time of the last one-shot call of this thread went (ms)."""
    _fields_ = [("plan_ms", ctypes.c_double), ("image_ms", ctypes.c_double), ("convolve_ms", ctypes.c_double),
                ("release_ms", ctypes.c_double), ("total_ms", ctypes.c_double), ("cache_hit", ctypes.c_int)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def _options_ptr(options):
    """None, a PlanOptions or a dict of its fields -> (pointer or None, keep-alive)"""
    if options is None:
        return None, None
    if isinstance(options, dict):
        options = PlanOptions(**options)
    return ctypes.byref(options), options


class Profile(ctypes.Structure):
    _fields_ = [("ms", ctypes.c_double * 5), ("launches", ctypes.c_long * 5), ("units", ctypes.c_long * 5)]

    NAMES = ("kernel_cols", "spectral_rows", "cols_c2r", "image_cols", "image_rows")

    def as_dict(self):
        return {n: {"ms": self.ms[i], "launches": self.launches[i], "units": self.units[i]}
                for i, n in enumerate(self.NAMES)}


# fftconv_extrema (include/fftconv.h): one record of Plan.extrema()
EXTREMA_DTYPE = [("max_value", "<f4"), ("max_row", "<i4"), ("max_col", "<i4"), ("min_value", "<f4"), ("min_row", "<i4"), ("min_col", "<i4")]
# fftconv_peak (include/fftconv.h): one record of Plan.peaks()
PEAK_DTYPE = [("value", "<f4"), ("row", "<i4"), ("col", "<i4"), ("d_row", "<f4"), ("d_col", "<f4")]

# every symbol include/fftconv.h declares
EXPORTED_SYMBOLS = (
    "fftconv_fft_size16", "fftconv_fft_size_pow2", "fftconv_last_error", "fftconv_version", "fftconv_device_count",
    "fftconv_convolution_fft", "fftconv_convolution_fft_ex",
    "fftconv_cache_configure", "fftconv_cache_clear", "fftconv_cache_stats", "fftconv_last_call_timing",
    "fftconv_plan_create", "fftconv_plan_create_ex",
    "fftconv_plan_is_live", "fftconv_plan_destroy", "fftconv_plan_get_info",
    "fftconv_plan_set_image", "fftconv_plan_set_images", "fftconv_plan_set_images_typed", "fftconv_plan_spectrum", "fftconv_plan_mark_spectrum_valid",
    "fftconv_plan_use_spectrum_buffer", "fftconv_plan_export_spectrum", "fftconv_plan_import_spectrum",
    "fftconv_plan_convolve", "fftconv_plan_convolve_packed", "fftconv_plan_prepare_kernels_packed",
    "fftconv_plan_synchronize", "fftconv_plan_set_stream",
    "fftconv_plan_set_option", "fftconv_plan_set_output_rect", "fftconv_plan_set_output_stride", "fftconv_plan_set_extrema", "fftconv_plan_get_extrema", "fftconv_plan_extrema_device", "fftconv_plan_set_peaks", "fftconv_plan_get_peaks", "fftconv_plan_peaks_device", "fftconv_plan_set_normalisation", "fftconv_plan_set_match_score", "fftconv_plan_set_border", "fftconv_plan_set_spectral_filter", "fftconv_plan_get_option", "fftconv_plan_get_profile",
    "fftconv_fft_data", "fftconv_conv_fft_data",
    "fftconv_multi_create", "fftconv_multi_destroy", "fftconv_multi_set_image", "fftconv_multi_import_spectrum",
    "fftconv_multi_convolve", "fftconv_multi_set_option", "fftconv_multi_get_option",
    "fftconv_multi_shard", "fftconv_multi_size", "fftconv_multi_plan", "fftconv_convolution_fft_multi",
)

_lib = None


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so (same
    SONAME as /opt/rocm's); if libfftconv.so pulled in the system copy first, a later
    `import torch` would bring a second runtime into the process and see no GPUs, and streams or
    events could not be shared.  So when torch is installed, its copy is loaded first (by path,
    without importing torch) and libfftconv.so binds to it through the SONAME."""
    if os.environ.get("FFTCONV_NO_TORCH_RUNTIME"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
    except Exception:
        pass


def load_library():
    """Loads libfftconv.so (built in-tree by ``__graft_entry__.build()`` / ``csrc/Makefile``).
    Fails loudly when it is missing: there is no fallback implementation."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FFTConvError(-7, "HIP extension %s is missing; build it with `make -C %s`"
                           % (LIB_PATH, os.path.join(_HERE, "csrc")))
    _preload_hip_runtime()
    lib = ctypes.CDLL(LIB_PATH)
    vp, ci, cs = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    pi = ctypes.POINTER(ctypes.c_int)
    lib.fftconv_fft_size16.argtypes = [ci]
    lib.fftconv_fft_size_pow2.argtypes = [ci]
    lib.fftconv_last_error.restype = ctypes.c_char_p
    lib.fftconv_version.restype = ctypes.c_char_p
    lib.fftconv_device_count.argtypes = [pi]
    lib.fftconv_convolution_fft.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, ci, vp, pi, pi]
    lib.fftconv_convolution_fft_ex.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, ci, ci, vp, pi, pi, vp]
    lib.fftconv_cache_configure.argtypes = [ci, cs]
    lib.fftconv_cache_clear.argtypes = []
    lib.fftconv_cache_stats.argtypes = [ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_long),
                                        ctypes.POINTER(cs)]
    lib.fftconv_last_call_timing.argtypes = [ctypes.POINTER(CallTiming)]
    lib.fftconv_plan_create.argtypes = [ctypes.POINTER(vp), ci, ci, ci, ci, ci, ci, vp]
    lib.fftconv_plan_create_ex.argtypes = [ctypes.POINTER(vp), ci, ci, ci, ci, ci, ci, vp, vp]
    lib.fftconv_plan_is_live.argtypes = [vp]
    lib.fftconv_plan_destroy.argtypes = [vp]
    lib.fftconv_plan_get_info.argtypes = [vp, ctypes.POINTER(PlanInfo)]
    lib.fftconv_plan_set_image.argtypes = [vp, vp, ci]
    lib.fftconv_plan_set_images.argtypes = [vp, vp, ci, ci]
    lib.fftconv_plan_set_images_typed.argtypes = [vp, vp, ci, ci, ci]
    lib.fftconv_plan_spectrum.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(cs)]
    lib.fftconv_plan_mark_spectrum_valid.argtypes = [vp]
    lib.fftconv_plan_use_spectrum_buffer.argtypes = [vp, vp, cs]
    lib.fftconv_plan_export_spectrum.argtypes = [vp, vp, ci]
    lib.fftconv_plan_import_spectrum.argtypes = [vp, vp, ci]
    lib.fftconv_plan_convolve.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci]
    lib.fftconv_plan_convolve_packed.argtypes = [vp, ci, vp, ci, ci, vp]
    lib.fftconv_plan_prepare_kernels_packed.argtypes = [vp, ci, vp, ci, ci]
    lib.fftconv_plan_synchronize.argtypes = [vp]
    lib.fftconv_plan_set_stream.argtypes = [vp, vp]
    lib.fftconv_plan_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_long]
    lib.fftconv_plan_set_output_rect.argtypes = [vp, ci, ci, ci, ci]
    lib.fftconv_plan_set_output_stride.argtypes = [vp, ci, ci]
    lib.fftconv_plan_set_extrema.argtypes = [vp, ci, ci]
    lib.fftconv_plan_get_extrema.argtypes = [vp, ci, ci, vp]
    lib.fftconv_plan_extrema_device.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(cs)]
    lib.fftconv_plan_set_peaks.argtypes = [vp, ci, ci, ci, ctypes.c_float, ci, ci]
    lib.fftconv_plan_get_peaks.argtypes = [vp, ci, ci, vp, vp]
    lib.fftconv_plan_peaks_device.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(cs)]
    lib.fftconv_plan_set_normalisation.argtypes = [vp, ci, ci, ci]
    lib.fftconv_plan_set_match_score.argtypes = [vp, ci, ci, ci]
    lib.fftconv_plan_set_border.argtypes = [vp, ci, ctypes.c_float]
    lib.fftconv_plan_set_spectral_filter.argtypes = [vp, ci, ctypes.c_float]
    lib.fftconv_plan_get_option.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_long)]
    lib.fftconv_plan_get_profile.argtypes = [vp, ctypes.POINTER(Profile), ci]
    lib.fftconv_fft_data.argtypes = [vp, ci, ci, ci, ci, ci, ci, ctypes.POINTER(vp)]
    lib.fftconv_conv_fft_data.argtypes = [vp, ci, vp, vp, vp, vp, vp, ci, vp]
    lib.fftconv_multi_create.argtypes = [ctypes.POINTER(vp), ci, ci, ci, ci, ci, pi, ci, vp]
    lib.fftconv_multi_destroy.argtypes = [vp]
    lib.fftconv_multi_set_image.argtypes = [vp, vp, ci]
    lib.fftconv_multi_import_spectrum.argtypes = [vp, vp, ci]
    lib.fftconv_multi_convolve.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci]
    lib.fftconv_multi_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_long]
    lib.fftconv_multi_get_option.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_long)]
    lib.fftconv_multi_shard.argtypes = [vp, ci, ci, pi, pi]
    lib.fftconv_multi_size.argtypes = [vp]
    lib.fftconv_multi_plan.argtypes = [vp, ci, ctypes.POINTER(vp), pi]
    lib.fftconv_convolution_fft_multi.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, pi, ci, vp, pi, pi]
    _lib = lib
    # the one-shot entries keep their last few plans (device scratch, host copy threads): released before the
    # interpreter tears the HIP runtime down (the MEX gateways do the same with mexAtExit)
    import atexit
    atexit.register(lib.fftconv_cache_clear)
    return lib


def _check(rc):
    if rc != 0:
        raise FFTConvError(rc, load_library().fftconv_last_error().decode("utf-8", "replace"))


def fft_size16(n):
    """computeFFTsize16 (src/cudaConvFFTData.h:96-102)."""
    return load_library().fftconv_fft_size16(int(n))


def fft_size_pow2(n):
    """computeFFTsize (src/cudaConvFFTData.h:67-94)."""
    return load_library().fftconv_fft_size_pow2(int(n))


def device_count():
    n = ctypes.c_int(0)
    load_library().fftconv_device_count(ctypes.byref(n))
    return n.value


def cache_configure(max_plans=4, max_bytes=0):
    """plan cache of the one-shot entry: plans kept (0 = off), device bytes they may hold (0 = unchanged)"""
    _check(load_library().fftconv_cache_configure(int(max_plans), int(max_bytes)))


def cache_clear():
    _check(load_library().fftconv_cache_clear())


def cache_stats():
    n, h, m, b = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_long(0), ctypes.c_size_t(0)
    _check(load_library().fftconv_cache_stats(ctypes.byref(n), ctypes.byref(h), ctypes.byref(m), ctypes.byref(b)))
    return {"plans": n.value, "hits": h.value, "misses": m.value, "device_bytes": b.value}


def last_call_timing():
    """where the time of this thread's last cudaConvolutionFFT call went (dict of ms + cache_hit)"""
    t = CallTiming()
    _check(load_library().fftconv_last_call_timing(ctypes.byref(t)))
    return t.as_dict()


def _as_matlab_single(a, what):
    """float32, column-major, 3-D (H x W x F); 2-D inputs are H x W x 1 (the reference rejects
    them -- SURVEY D4 -- this engine accepts F = 1)."""
    a = np.asarray(a)
    if a.dtype != np.float32:
        raise FFTConvError(-1, "%s must be single (float32), got %s" % (what, a.dtype))
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3:
        raise FFTConvError(-1, "Invalid %s input" % what)
    return np.asfortranarray(a)


def _kernel_tables(kernels):
    ks = [_as_matlab_single(k, "kernel") for k in kernels]
    n = len(ks)
    ptrs = (ctypes.c_void_p * n)(*[k.ctypes.data for k in ks])
    kh = (ctypes.c_int * n)(*[k.shape[0] for k in ks])
    kw = (ctypes.c_int * n)(*[k.shape[1] for k in ks])
    kf = (ctypes.c_int * n)(*[k.shape[2] for k in ks])
    return ks, ptrs, kh, kw, kf


def _thread_size(threads):
    if threads is None:
        return None, 0, None
    t = np.ascontiguousarray(np.asarray(threads, dtype=np.float64).ravel())
    return ctypes.c_void_p(t.ctypes.data), int(t.size), t


def cudaConvolutionFFT(data, maxKernelH, maxKernelW, kernelCell, threadSize=None, gpuId=0, options=None, out=None):
    """One-shot convolution, host arrays in / host arrays out (list of FFT_H x FFT_W float32,
    Fortran order).  Mirrors the MEX entry of src/cudaConvolutionFFT.cu.  ``options``: a
    PlanOptions (or a dict of its fields) for fftconv_convolution_fft_ex; ``out``: optional list of
    caller buffers (FFT_H x FFT_W float32, Fortran order) to fill instead of fresh arrays.
    With ``map_format`` 1 in the options the maps (and ``out``) are np.float16, with 2 np.uint16 arrays of
    bfloat16 bit patterns (MAP_DTYPES)."""
    lib = load_library()
    if not isinstance(kernelCell, (list, tuple)):
        raise FFTConvError(-1, "Kernel must be a cell array")  # src/cudaConvolutionFFT.cu:64-65
    d = _as_matlab_single(data, "data")
    H, W, F = d.shape
    ks, kptr, kh, kw, kf = _kernel_tables(kernelCell)
    n = len(ks)
    fh, fw = fft_size16(H + int(maxKernelH) - 1), fft_size16(W + int(maxKernelW) - 1)
    dt = _options_map_dtype(options)
    if out is None:
        outs = [np.empty((fh, fw), dtype=dt, order="F") for _ in range(n)]
    else:
        outs = list(out)
        if len(outs) != n or any(o.dtype != dt or o.shape != (fh, fw) or not o.flags.f_contiguous for o in outs):
            raise FFTConvError(-1, "out must hold one FFT_H x FFT_W %s Fortran-order buffer per kernel" % dt.name)
    optr = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
    tptr, tn, _keep = _thread_size(threadSize)
    ofh, ofw = ctypes.c_int(0), ctypes.c_int(0)
    oref, _okeep = _options_ptr(options)
    _check(lib.fftconv_convolution_fft_ex(ctypes.c_void_p(d.ctypes.data), H, W, F, int(maxKernelH), int(maxKernelW),
                                          n, kptr, kh, kw, kf, HOST, tptr, tn, int(gpuId), optr,
                                          ctypes.byref(ofh), ctypes.byref(ofw), oref))
    assert (ofh.value, ofw.value) == (fh, fw)
    return outs


class Plan:
    """Plan API: image spectrum computed once, reused for any number of kernels.  Pointers are
    plain integers (e.g. ``torch.Tensor.data_ptr()``); torch is not a dependency of this module."""

    def __init__(self, H, W, F, maxKernelH, maxKernelW, gpuId=0, stream=0, options=None):
        self._lib = load_library()
        self._h = ctypes.c_void_p(None)
        oref, _okeep = _options_ptr(options)
        _check(self._lib.fftconv_plan_create_ex(ctypes.byref(self._h), int(H), int(W), int(F), int(maxKernelH),
                                                int(maxKernelW), int(gpuId), ctypes.c_void_p(int(stream) or None), oref))
        self.info = PlanInfo()
        _check(self._lib.fftconv_plan_get_info(self._h, ctypes.byref(self.info)))
        self._images = 1       # images a convolve covers: what the image entries below last gave the plan (images())

    # -- lifetime
    def destroy(self):
        if self._h is not None and self._h.value:
            self._lib.fftconv_plan_destroy(self._h)
            self._h = ctypes.c_void_p(None)

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()

    # -- image
    def set_image(self, data):
        """host numpy H x W x F (or H x W) float32"""
        d = _as_matlab_single(data, "data")
        if d.shape != (self.info.data_h, self.info.data_w, self.info.feature_dim):
            raise FFTConvError(-1, "Invalid data input: shape %s does not match the plan" % (d.shape,))
        _check(self._lib.fftconv_plan_set_image(self._h, ctypes.c_void_p(d.ctypes.data), HOST))
        self._images = 1

    def set_image_device(self, ptr):
        _check(self._lib.fftconv_plan_set_image(self._h, ctypes.c_void_p(int(ptr)), DEVICE))
        self._images = 1

    def set_images(self, data):
        """a batch of images: host numpy H x W x F x B float32 in Fortran order (H x W x B where the plan's F is 1).  Every
        following convolve then returns B * n maps, image-major (fftconv_plan_set_images); set_image returns to one image."""
        a = np.asarray(data)
        if a.dtype != np.float32:
            raise FFTConvError(-1, "data must be single (float32), got %s" % a.dtype)
        i = self.info
        if a.ndim == 3 and i.feature_dim == 1:
            a = a[:, :, None, :]
        if a.ndim != 4 or a.shape[:3] != (i.data_h, i.data_w, i.feature_dim) or a.shape[3] < 1:
            raise FFTConvError(-1, "Invalid data input: shape %s is not H x W x F x B of the plan" % (a.shape,))
        a = np.asfortranarray(a)
        _check(self._lib.fftconv_plan_set_images(self._h, ctypes.c_void_p(a.ctypes.data), int(a.shape[3]), HOST))
        self._images = int(a.shape[3])

    def images(self):
        """images a convolve of this plan covers (its lists hold images() * n maps): what set_images last gave it, else 1.  Kept
        by this object; the library's own count is get_option("images") (0 while the plan has no image)."""
        return self._images

    def set_images_device(self, ptr, n):
        """n images back to back in device memory ([b][f][w][h] floats)"""
        _check(self._lib.fftconv_plan_set_images(self._h, ctypes.c_void_p(int(ptr)), int(n), DEVICE))
        self._images = int(n)

    # -- typed images: uint8 / uint16 / float16 / bfloat16 pixels, converted in the load (fftconv_plan_set_images_typed)
    def _typed_format(self, a, pixel_format):
        if pixel_format is None:
            if a.dtype not in _PIXEL_OF_DTYPE:
                raise FFTConvError(-1, "typed pixels are uint8, uint16 or float16 arrays (bfloat16: uint16 bit patterns with "
                                   "pixel_format=PIXEL_BF16), got %s" % a.dtype)
            return _PIXEL_OF_DTYPE[a.dtype]
        fmt = int(pixel_format)
        if fmt not in PIXEL_DTYPES or fmt == PIXEL_F32 or a.dtype != PIXEL_DTYPES[fmt]:
            raise FFTConvError(-1, "pixel_format %s does not describe a %s array (float32 images: set_image / set_images)" % (pixel_format, a.dtype))
        return fmt

    def set_images_typed(self, data, pixel_format=None):
        """a batch of typed images: host numpy H x W x F x B (H x W x B where the plan's F is 1) of uint8, uint16 or float16 --
        the format follows from the dtype; bfloat16 is a uint16 array of bit patterns with pixel_format=PIXEL_BF16.  A pixel's
        value is its exact float32 conversion (no 1/255): the maps are bit-equal to set_images of data.astype(float32)."""
        a = np.asarray(data)
        fmt = self._typed_format(a, pixel_format)
        i = self.info
        if a.ndim == 3 and i.feature_dim == 1:
            a = a[:, :, None, :]
        if a.ndim != 4 or a.shape[:3] != (i.data_h, i.data_w, i.feature_dim) or a.shape[3] < 1:
            raise FFTConvError(-1, "Invalid data input: shape %s is not H x W x F x B of the plan" % (a.shape,))
        a = np.asfortranarray(a)
        _check(self._lib.fftconv_plan_set_images_typed(self._h, ctypes.c_void_p(a.ctypes.data), fmt, int(a.shape[3]), HOST))
        self._images = int(a.shape[3])

    def set_image_typed(self, data, pixel_format=None):
        """one typed image: host numpy H x W x F (or H x W), as set_images_typed takes a batch"""
        a = np.asarray(data)
        i = self.info
        if a.ndim == 2:
            a = a[:, :, None]
        if a.shape != (i.data_h, i.data_w, i.feature_dim):
            raise FFTConvError(-1, "Invalid data input: shape %s does not match the plan" % (a.shape,))
        self.set_images_typed(a[:, :, :, None], pixel_format)

    def set_images_typed_device(self, ptr, pixel_format, n):
        """n typed images back to back in device memory ([b][f][w][h] elements of pixel_format)"""
        _check(self._lib.fftconv_plan_set_images_typed(self._h, ctypes.c_void_p(int(ptr)), int(pixel_format), int(n), DEVICE))
        self._images = int(n)

    def spectrum(self):
        """(device pointer, bytes) of the image spectrum buffer (for the RCCL broadcast); a plan holding B images: all B spectra,
        image b at b * info.spectrum_bytes."""
        p, n = ctypes.c_void_p(None), ctypes.c_size_t(0)
        _check(self._lib.fftconv_plan_spectrum(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def export_spectrum(self):
        """the image spectrum in the reference's order (what cudaFFTData returns, src/cudaFFTData.cu:
        90-103): complex64 [F][FFT_W][FFT_H/2+1], unnormalised, == numpy.fft.rfft2 of the padded
        [F][FFT_W][FFT_H] planes.  Needs a plan created with exact_window."""
        i = self.info
        a = np.empty((i.feature_dim, i.fft_w, i.fft_h // 2 + 1), dtype=np.complex64)
        _check(self._lib.fftconv_plan_export_spectrum(self._h, ctypes.c_void_p(a.ctypes.data), HOST))
        return a

    def import_spectrum(self, spectrum):
        """replaces set_image: a spectrum in the reference's order (see export_spectrum)"""
        i = self.info
        a = np.ascontiguousarray(spectrum, dtype=np.complex64)
        if a.shape != (i.feature_dim, i.fft_w, i.fft_h // 2 + 1):
            raise FFTConvError(-1, "spectrum must be [F][FFT_W][FFT_H/2+1], got %s" % (a.shape,))
        _check(self._lib.fftconv_plan_import_spectrum(self._h, ctypes.c_void_p(a.ctypes.data), HOST))
        self._images = 1

    def use_spectrum_buffer(self, ptr, nbytes):
        """keep the image spectrum in caller-owned device memory (e.g. a torch tensor); the plan then holds no image until
        set_image / set_images / mark_spectrum_valid (one image)"""
        _check(self._lib.fftconv_plan_use_spectrum_buffer(self._h, ctypes.c_void_p(int(ptr) or None), int(nbytes)))
        self._images = 1

    def mark_spectrum_valid(self):
        _check(self._lib.fftconv_plan_mark_spectrum_valid(self._h))

    # -- convolution
    def convolve(self, kernelCell, out=None):
        """host kernels (list of kh x kw x F float32) -> list of host maps.  ``out``: optional list
        of caller buffers to fill (FFT_H x FFT_W float32, Fortran order; pageable, or pinned for a
        direct DMA copy-out) instead of fresh arrays.  Plan option "map_format" 1: the maps (and ``out``)
        are np.float16; 2: np.uint16 arrays of bfloat16 bit patterns (MAP_DTYPES)."""
        ks, kptr, kh, kw, kf = _kernel_tables(kernelCell)
        for k in ks:
            if k.shape[2] != self.info.feature_dim:  # src/cudaConvolutionFFT.cu:242
                raise FFTConvError(-3, "Kernel and Data must have the same number of features and kernel "
                                       "size should be smaller than data size")
        n = len(ks)
        _check(self._lib.fftconv_plan_get_info(self._h, ctypes.byref(self.info)))   # out_h / out_w follow "output_region"
        oh, ow = self.info.out_h, self.info.out_w
        dt = MAP_DTYPES[self.get_option("map_format")]
        nmaps = n * self.images()      # a plan holding B images: the flat image-major list, map b * n + k
        if out is None:
            outs = [np.empty((oh, ow), dtype=dt, order="F") for _ in range(nmaps)]
        else:
            outs = list(out)
            if len(outs) != nmaps:
                raise FFTConvError(-1, "out must hold one buffer per kernel (and per image the plan holds)")
            for o in outs:
                if (o.dtype != dt or o.shape != (oh, ow)
                        or not o.flags.f_contiguous or not o.flags.writeable):
                    raise FFTConvError(-1, "out buffers must be writable out_h x out_w %s in Fortran order" % dt.name)
        optr = (ctypes.c_void_p * nmaps)(*[o.ctypes.data for o in outs])
        _check(self._lib.fftconv_plan_convolve(self._h, n, kptr, kh, kw, HOST, optr, HOST))
        return outs

    def convolve_to_device(self, kernelCell, out_ptrs, kernel_location=HOST):
        """fftconv_plan_convolve with maps in device memory: asynchronous on the plan's stream.  kernelCell: host arrays
        (kh x kw x F float32, consumed when the call returns) and / or (device pointer, kh, kw) triples of device-resident
        kernels ([F][kw][kh] floats, i.e. the same MATLAB array); kernel_location HOST (arrays only), DEVICE (triples only) or
        AUTO (any mix: the runtime tells them apart).  out_ptrs: one device pointer per kernel, out_h x out_w elements of the
        plan's "map_format" each (info.out_map_bytes: the caller sizes the buffers)."""
        ks, ptrs, khs, kws = [], [], [], []
        for k in kernelCell:
            if isinstance(k, tuple):
                if kernel_location == HOST:
                    raise FFTConvError(-1, "a device-resident kernel needs kernel_location DEVICE or AUTO")
                ptrs.append(int(k[0])), khs.append(int(k[1])), kws.append(int(k[2]))
                continue
            if kernel_location == DEVICE:
                raise FFTConvError(-1, "a host kernel needs kernel_location HOST or AUTO")
            a = _as_matlab_single(k, "kernel")
            if a.shape[2] != self.info.feature_dim:  # src/cudaConvolutionFFT.cu:242
                raise FFTConvError(-3, "Kernel and Data must have the same number of features and kernel "
                                       "size should be smaller than data size")
            ks.append(a)
            ptrs.append(a.ctypes.data), khs.append(a.shape[0]), kws.append(a.shape[1])
        n = len(ptrs)
        nmaps = n * self.images()      # (a plan holding B images: B * n pointers, image-major)
        if len(out_ptrs) != nmaps:
            raise FFTConvError(-1, "out_ptrs must hold one device pointer per kernel (and per image the plan holds)")
        _check(self._lib.fftconv_plan_convolve(self._h, n, (ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*khs),
                                               (ctypes.c_int * n)(*kws), int(kernel_location),
                                               (ctypes.c_void_p * nmaps)(*[int(o) for o in out_ptrs]), DEVICE))

    def convolve_packed_device(self, n, kernels_ptr, kh, kw, out_ptr):
        """n equally sized kernels packed in device memory -> n maps packed in device memory (info.out_map_bytes each:
        the caller sizes the buffer for the plan's "map_format"); asynchronous on the plan's stream."""
        _check(self._lib.fftconv_plan_convolve_packed(self._h, int(n), ctypes.c_void_p(int(kernels_ptr)),
                                                      int(kh), int(kw), ctypes.c_void_p(int(out_ptr))))

    def prepare_kernels_packed_device(self, n, kernels_ptr, kh, kw):
        """queue the image-independent part of convolve_packed_device (kernel column transforms);
        the next convolve_packed_device call with the same arguments reuses it"""
        _check(self._lib.fftconv_plan_prepare_kernels_packed(self._h, int(n), ctypes.c_void_p(int(kernels_ptr)),
                                                             int(kh), int(kw)))

    def synchronize(self):
        _check(self._lib.fftconv_plan_synchronize(self._h))

    def is_live(self):
        return bool(self._h is not None and self._h.value and self._lib.fftconv_plan_is_live(self._h))

    def set_stream(self, stream):
        """re-bind the plan to another HIP stream (integer handle, 0 = default stream)"""
        _check(self._lib.fftconv_plan_set_stream(self._h, ctypes.c_void_p(int(stream) or None)))

    def set_option(self, name, value):
        """plan options by name (include/fftconv.h: fftconv_plan_set_option), e.g. "batch_maps", "map_format", "rows_group", and for
        image batches "image_walk" (1: spectral-row launches of several images walk over images; read-only "image_walk_active"
        tells whether this plan has the kernel for it)"""
        _check(self._lib.fftconv_plan_set_option(self._h, name.encode(), int(value)))
        _check(self._lib.fftconv_plan_get_info(self._h, ctypes.byref(self.info)))

    def set_output_rect(self, off_h, off_w, out_h, out_w):
        """every result map becomes rows [off_h, off_h + out_h) of columns [off_w, off_w + out_w) of the FFT_H x FFT_W window
        (dense, column-major); info.out_h / out_w / out_map_bytes follow, option "output_region" then reads 5"""
        _check(self._lib.fftconv_plan_set_output_rect(self._h, int(off_h), int(off_w), int(out_h), int(out_w)))
        _check(self._lib.fftconv_plan_get_info(self._h, ctypes.byref(self.info)))

    def set_output_stride(self, stride_h, stride_w):
        """every result map becomes every stride_h-th row and stride_w-th column of the map the plan would deliver without it (the
        window, a region, the rectangle), counted from that map's first row and column (fftconv_plan_set_output_stride): dense,
        column-major, ceil(out_h / stride_h) x ceil(out_w / stride_w); info.out_h / out_w / out_map_bytes follow.  (1, 1) restores
        the dense maps.  Option "stride_store" (1, the default: the output kernel samples in its store where the plan can; 0:
        always the staged crop), read-only "stride_direct", "stride_h", "stride_w"."""
        _check(self._lib.fftconv_plan_set_output_stride(self._h, int(stride_h), int(stride_w)))
        _check(self._lib.fftconv_plan_get_info(self._h, ctypes.byref(self.info)))

    def set_extrema(self, on, max_maps=0):
        """per-map extrema (fftconv_plan_set_extrema): while on, every convolve of up to max_maps maps also leaves one record per
        delivered map on the device -- its largest and its smallest element and where they lie -- found while the maps are
        written; the maps themselves are unchanged.  Read them with extrema() or extrema_device().  Option "extrema_store" (1, the
        default: the output kernel finds them in its store where the plan can; 0: always the scan of the delivered maps),
        read-only "extrema", "extrema_direct", "extrema_max_maps"."""
        _check(self._lib.fftconv_plan_set_extrema(self._h, 1 if on else 0, int(max_maps)))
        _check(self._lib.fftconv_plan_get_info(self._h, ctypes.byref(self.info)))

    def extrema(self, first=0, n=None):
        """the records [first, first + n) of the last convolve under set_extrema (n None: up to its last map), as a structured
        NumPy array of EXTREMA_DTYPE: max_value, max_row, max_col, min_value, min_row, min_col -- row the fast index and col the
        slow one of the delivered map (the element lies at col * out_h + row); ties go to the smallest col * out_h + row, a map
        without an element that compares reports NaN and -1.  Waits for the plan's stream."""
        import numpy as np
        if n is None:      # ("extrema_maps": the maps of the last convolve under it; -1 before any -- the library then refuses the read)
            n = max(self.get_option("extrema_maps"), 0) - int(first)
        out = np.zeros(max(int(n), 0), dtype=EXTREMA_DTYPE)
        _check(self._lib.fftconv_plan_get_extrema(self._h, int(first), int(n), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def extrema_device(self):
        """(device pointer, bytes) of the plan's record array (max_maps records of EXTREMA_DTYPE): stable until the next set_extrema
        or the plan's end; its content is ordered on the plan's stream"""
        ptr, nbytes = ctypes.c_void_p(), ctypes.c_size_t(0)
        _check(self._lib.fftconv_plan_extrema_device(self._h, ctypes.byref(ptr), ctypes.byref(nbytes)))
        return int(ptr.value or 0), int(nbytes.value)

    def set_peaks(self, mode, max_maps=0, max_peaks=0, threshold=0.0, radius=(0, 0)):
        """peak lists (fftconv_plan_set_peaks): while on (PEAKS_MAX: maxima at or above threshold; PEAKS_MIN: minima at or below
        it), every convolve of up to max_maps maps also leaves, per delivered map, the number of its peaks and the first max_peaks
        of them in memory order on the device -- the elements that meet the threshold and that no other element within
        radius = (rows, columns) beats, with a sub-pixel offset per dimension; the maps themselves are unchanged.  Read them with
        peaks() or peaks_device().  A change of threshold, radius or mode alone keeps the buffers.  PEAKS_OFF frees them.  Read-only
        options "peaks", "peaks_max_maps", "peaks_max", "peaks_radius_h", "peaks_radius_w", "peaks_maps"."""
        rh, rw = radius
        _check(self._lib.fftconv_plan_set_peaks(self._h, int(mode), int(max_maps), int(max_peaks), float(threshold), int(rh), int(rw)))
        _check(self._lib.fftconv_plan_get_info(self._h, ctypes.byref(self.info)))

    def peaks(self, first=0, n=None, order="memory"):
        """(found, lists) of the maps [first, first + n) of the last convolve under set_peaks (n None: up to its last map): found an
        int32 array -- the peaks of each map, all of them -- and lists one structured array of PEAK_DTYPE per map (value, row, col,
        d_row, d_col; the peak lies at (row + d_row, col + d_col), row the fast index), trimmed to min(found, max_peaks).
        order "memory": ascending col * out_h + row, as the device leaves them; "strength": sorted here on the host by value
        (descending for PEAKS_MAX, ascending for PEAKS_MIN), ties by ascending index.  Waits for the plan's stream."""
        import numpy as np
        if order not in ("memory", "strength"):
            raise ValueError("order is \"memory\" or \"strength\", not %r" % (order,))
        if n is None:      # ("peaks_maps": the maps of the last convolve under it; -1 before any -- the library then refuses the read)
            n = max(self.get_option("peaks_maps"), 0) - int(first)
        n, cap = max(int(n), 0), max(self.get_option("peaks_max"), 0)
        found = np.zeros(n, dtype=np.int32)
        recs = np.zeros((n, cap), dtype=PEAK_DTYPE)
        # (zero maps asked: the arrays are empty, but the pointers the library checks must not be NULL)
        fbuf, rbuf = (found, recs) if n and cap else (np.zeros(1, dtype=np.int32), np.zeros(1, dtype=PEAK_DTYPE))
        _check(self._lib.fftconv_plan_get_peaks(self._h, int(first), n, fbuf.ctypes.data_as(ctypes.c_void_p), rbuf.ctypes.data_as(ctypes.c_void_p)))
        lists = [recs[m, :min(int(found[m]), cap)].copy() for m in range(n)]
        if order == "strength":
            out_h, minima = int(self.info.out_h), self.get_option("peaks") == PEAKS_MIN
            for m, l in enumerate(lists):
                index = l["col"].astype(np.int64) * out_h + l["row"]
                lists[m] = l[np.lexsort((index, l["value"] if minima else -l["value"]))]
        return found, lists

    def peaks_device(self):
        """(found pointer, records pointer, bytes of the records) of the plan's device arrays: max_maps int32 counts, and max_maps x
        max_peaks records of PEAK_DTYPE; stable until a set_peaks that changes max_maps or max_peaks or switches the lists off, their
        content ordered on the plan's stream"""
        found, recs, nbytes = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t(0)
        _check(self._lib.fftconv_plan_peaks_device(self._h, ctypes.byref(found), ctypes.byref(recs), ctypes.byref(nbytes)))
        return int(found.value or 0), int(recs.value or 0), int(nbytes.value)

    def set_normalisation(self, mode, box_h=0, box_w=0):
        """mode 1: every map becomes the zero-mean normalised cross-correlation over the box box_h x box_w -- the size every
        kernel then has (fftconv_plan_set_normalisation); mode 0: raw maps again.  A call that changes mode or box leaves the
        plan without an image: set_image / set_images again before the next convolve.  Option "norm_store" (1 default: the
        output kernel scales in its store where the plan can; 0: always the staged crop), read-only "norm_direct", "normalise",
        "norm_box_h", "norm_box_w"."""
        _check(self._lib.fftconv_plan_set_normalisation(self._h, int(mode), int(box_h), int(box_w)))

    def set_match_score(self, score, box_h=0, box_w=0):
        """the template-matching score every map holds (fftconv_plan_set_match_score), over the box box_h x box_w -- the size every
        kernel then has: SCORE_NONE (raw maps), SCORE_CCOEFF_NORMED (set_normalisation's mode 1: one state), SCORE_CCOEFF,
        SCORE_CCORR_NORMED, SCORE_SQDIFF.  A call that changes score or box leaves the plan without an image.  Read-only options
        "match_score", "norm_box_h", "norm_box_w", "norm_direct"; "norm_store" as for set_normalisation."""
        _check(self._lib.fftconv_plan_set_match_score(self._h, int(score), int(box_h), int(box_w)))

    def set_border(self, mode, value=0.0):
        """what the image is beyond its data (fftconv_plan_set_border): BORDER_ZERO (the default), BORDER_CONSTANT (`value`),
        BORDER_REPLICATE, BORDER_SYMMETRIC, BORDER_REFLECT101, BORDER_CIRCULAR.  A mode other than BORDER_ZERO makes every map the
        H x W "same" map anchored on the plan's MAX_KERNEL box (info.out_h / out_w follow; a rectangle inside it may be set
        afterwards with set_output_rect, in window coordinates); BORDER_ZERO restores the window.  A call that changes mode or
        value leaves the plan without an image: set_image / set_images again before the next convolve.  Option "border_store"
        (1, the default: the column kernel maps the indices in its load where the plan can; 0: always the staged extension), read-only
        "border_direct", "border_mode", "border_lead_h", "border_lead_w"."""
        _check(self._lib.fftconv_plan_set_border(self._h, int(mode), float(value)))
        _check(self._lib.fftconv_plan_get_info(self._h, ctypes.byref(self.info)))

    def set_spectral_filter(self, mode, param=0.0):
        """the pointwise operation between the forward and the inverse transform (fftconv_plan_set_spectral_filter): FILTER_PRODUCT
        (the default: I^ K^), FILTER_PHASE (phase correlation, P / |P| with P = I^ K^; param 0) or FILTER_WIENER (I^ conj(K^) /
        (|K^|^2 + param), param = lambda >= 0 in the units of |K^|^2 of the unnormalised DFT), on the plan's transform lengths
        (info.transform_h x transform_w; exact_window makes them the window).  feature_dim 1, one-pass plans without a matching
        score.  It keeps the image, the prepared kernels and the output side.  Read-only options "spectral_filter",
        "spectral_filter_fast"."""
        _check(self._lib.fftconv_plan_set_spectral_filter(self._h, int(mode), float(param)))

    def get_option(self, name):
        v = ctypes.c_long(0)
        _check(self._lib.fftconv_plan_get_option(self._h, name.encode(), ctypes.byref(v)))
        return int(v.value)

    def refresh_info(self):
        """reads `info` again from the plan and returns it (a call that raised has not refreshed it)"""
        _check(self._lib.fftconv_plan_get_info(self._h, ctypes.byref(self.info)))
        return self.info

    def profile(self, reset=True):
        pr = Profile()
        _check(self._lib.fftconv_plan_get_profile(self._h, ctypes.byref(pr), 1 if reset else 0))
        return pr.as_dict()


def cudaConvolutionFFTMulti(data, maxKernelH, maxKernelW, kernelCell, gpuIds):
    """One-shot convolution over several GPUs from this one process (fftconv_convolution_fft_multi:
    what src/cudaConvFFTDataStreams.cu set out to be): image transformed on gpuIds[0], spectrum
    peer-copied, kernels dealt in contiguous blocks.  Host arrays in / out like cudaConvolutionFFT."""
    lib = load_library()
    if not isinstance(kernelCell, (list, tuple)):
        raise FFTConvError(-1, "Kernel must be a cell array")
    d = _as_matlab_single(data, "data")
    H, W, F = d.shape
    ks, kptr, kh, kw, kf = _kernel_tables(kernelCell)
    n = len(ks)
    fh, fw = fft_size16(H + int(maxKernelH) - 1), fft_size16(W + int(maxKernelW) - 1)
    outs = [np.empty((fh, fw), dtype=np.float32, order="F") for _ in range(n)]
    optr = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
    devs = (ctypes.c_int * len(gpuIds))(*[int(g) for g in gpuIds])
    ofh, ofw = ctypes.c_int(0), ctypes.c_int(0)
    _check(lib.fftconv_convolution_fft_multi(ctypes.c_void_p(d.ctypes.data), H, W, F, int(maxKernelH), int(maxKernelW),
                                             n, kptr, kh, kw, kf, devs, len(gpuIds), optr, ctypes.byref(ofh), ctypes.byref(ofw)))
    return outs


class MultiPlan:
    """fftconv_multi_*: one plan per listed device driven from this process (image spectrum on
    gpuIds[0], peer copies, contiguous kernel blocks)."""

    def __init__(self, H, W, F, maxKernelH, maxKernelW, gpuIds, options=None):
        self._lib = load_library()
        self._h = ctypes.c_void_p(None)
        devs = (ctypes.c_int * len(gpuIds))(*[int(g) for g in gpuIds])
        oref, _okeep = _options_ptr(options)
        _check(self._lib.fftconv_multi_create(ctypes.byref(self._h), int(H), int(W), int(F), int(maxKernelH), int(maxKernelW),
                                              devs, len(gpuIds), oref))
        # "" or the warning naming destinations without direct peer access to gpuIds[0] (their copies are staged)
        self.warning = (self._lib.fftconv_last_error() or b"").decode()
        self.shape = (int(H), int(W), int(F))
        p, dev = ctypes.c_void_p(None), ctypes.c_int(0)
        _check(self._lib.fftconv_multi_plan(self._h, 0, ctypes.byref(p), ctypes.byref(dev)))
        self.info = PlanInfo()
        _check(self._lib.fftconv_plan_get_info(p, ctypes.byref(self.info)))
        fmt = ctypes.c_long(0)
        _check(self._lib.fftconv_plan_get_option(p, b"map_format", ctypes.byref(fmt)))
        self.map_dtype = MAP_DTYPES[int(fmt.value)]      # every plan of the handle was created with the same options

    def __len__(self):
        return self._lib.fftconv_multi_size(self._h)

    def set_option(self, name, value):
        """"spectrum_transport" 0 peer copies / 1 one RCCL broadcast; "verbose" (include/fftconv.h)"""
        _check(self._lib.fftconv_multi_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name):
        v = ctypes.c_long(0)
        _check(self._lib.fftconv_multi_get_option(self._h, name.encode(), ctypes.byref(v)))
        return v.value

    def last_message(self):
        """text of the calling thread's last error / warning (e.g. why the RCCL transport was not used)"""
        return (self._lib.fftconv_last_error() or b"").decode()

    def shard(self, n_kernel, index):
        first, count = ctypes.c_int(0), ctypes.c_int(0)
        _check(self._lib.fftconv_multi_shard(self._h, int(n_kernel), int(index), ctypes.byref(first), ctypes.byref(count)))
        return first.value, count.value

    def set_image(self, data):
        d = _as_matlab_single(data, "data")
        if d.shape != self.shape:
            raise FFTConvError(-1, "Invalid data input: shape %s does not match the plan" % (d.shape,))
        _check(self._lib.fftconv_multi_set_image(self._h, ctypes.c_void_p(d.ctypes.data), HOST))

    def convolve(self, kernelCell):
        ks, kptr, kh, kw, kf = _kernel_tables(kernelCell)
        for k in ks:
            if k.shape[2] != self.shape[2]:
                raise FFTConvError(-3, "Kernel and Data must have the same number of features and kernel "
                                       "size should be smaller than data size")
        n = len(ks)
        outs = [np.empty((self.info.fft_h, self.info.fft_w), dtype=self.map_dtype, order="F") for _ in range(n)]
        optr = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
        _check(self._lib.fftconv_multi_convolve(self._h, n, kptr, kh, kw, HOST, optr, HOST))
        return outs

    def destroy(self):
        if self._h is not None and self._h.value:
            self._lib.fftconv_multi_destroy(self._h)
            self._h = ctypes.c_void_p(None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def cudaFFTData(data, kernelH, kernelW, gpuId=0):
    """Two-step API, step 1 (src/cudaFFTData.cu): returns a handle holding the device-resident
    image spectrum (the role of the complex gpuArray the reference returns)."""
    d = _as_matlab_single(data, "data")
    H, W, F = d.shape
    p = Plan(H, W, F, kernelH, kernelW, gpuId)
    p.set_image(d)
    return p


def cudaConvFFTData(fftData, kernelCell, threadSize=None):
    """Two-step API, step 2 (src/cudaConvFFTData.cu)."""
    if not isinstance(fftData, Plan):
        raise FFTConvError(-1, "Invalid input to MEX file.")  # src/cudaConvFFTData.cu:68
    if not isinstance(kernelCell, (list, tuple)):
        raise FFTConvError(-1, "Kernel must be a cell array")
    if threadSize is not None and np.asarray(threadSize).size != 4:  # src/cudaConvFFTData.cu:76-77
        raise FFTConvError(-2, "CUDA Thread Size must be 4 integers")
    return fftData.convolve(kernelCell)
