// kernels.hip -- HIP kernels for gfx950 (MI355X): thin wrappers that bind the HIP thread index
// and workgroup barrier to the workgroup bodies of kernels_body.hpp (generic kernels, small helper
// kernels); the specialised kernels live in kernels_rows*.hip / kernels_cols*.hip.
//
// Roofline: every kernel here is HBM/LDS-bound streaming work (no dense contraction), so MFMA
// is deliberately unused; see DESIGN.md for the algorithmic bytes per launch.
#include "kernels.hpp"

namespace fc {
namespace {

struct DevCtx {
    int tid, nthreads;
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

extern __shared__ __attribute__((aligned(16))) unsigned char fc_smem[];

// BS = 1: the Bluestein form of the transforms (exact-window plans whose window does not factor), 0: direct
template <int BS>
__global__ void __launch_bounds__(512) k_cols_r2c(ColsR2CArgs a) {
    DevCtx ctx{(int)threadIdx.x, (int)blockDim.x};
    cols_r2c_body<BS>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)blockIdx.y);
}

template <int BS>
__global__ void __launch_bounds__(512) k_rows_fwd(RowsFwdArgs a) {
    DevCtx ctx{(int)threadIdx.x, (int)blockDim.x};
    rows_fwd_body<BS>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x);
}

template <int BS>
__global__ void __launch_bounds__(512) k_spectral_rows(SpectralRowsArgs a) {
    DevCtx ctx{(int)threadIdx.x, (int)blockDim.x};
    // blockIdx.z: the image of a batch.  The body takes it folded into the map slot (rows_generic_slot): shifting S and Y here
    // needs a private copy of the arguments, and the stage table in it (FftDesc, indexed at run time) then lives in scratch.
    // (a.kernels_per_image is what the body splits the slot with; 0 -- nobody set it -- is one image, blockIdx.z = 0)
    spectral_rows_body<BS>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, rows_generic_slot((int)blockIdx.y, (int)blockIdx.z, a.kernels_per_image));
}

template <int BS>
__global__ void __launch_bounds__(512) k_cols_c2r(ColsC2RArgs a) {
    DevCtx ctx{(int)threadIdx.x, (int)blockDim.x};
    cols_c2r_body<BS>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)blockIdx.y);
}
// the same with 16-bit maps (plan option "map_format"; a.out_format: fp16 or bf16)
template <int BS>
__global__ void __launch_bounds__(512) k_cols_c2r16(ColsC2RArgs a) {
    DevCtx ctx{(int)threadIdx.x, (int)blockDim.x};
    cols_c2r_body<BS, true>(ctx, reinterpret_cast<c32*>(fc_smem), a, (int)blockIdx.x, (int)blockIdx.y);
}

// Reverses every plane of `pe` floats: for a column-major kh x kw plane that is the flip along both
// axes, kernel(end:-1:1, end:-1:1, f) of demoCudaConvolutionFFT.m:67-69.
__global__ void __launch_bounds__(256) k_flip_planes(const float* __restrict__ src, float* __restrict__ dst, int pe, long total) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long plane = i / pe;
        const int e = (int)(i - plane * pe);
        dst[i] = src[plane * pe + (pe - 1 - e)];
    }
}

// dst window += src window (overlap-add of block results into the full map): maps are column-major,
// h contiguous; the source is clipped to the destination.
__global__ void __launch_bounds__(256) k_add_window(float* __restrict__ dst, int dst_h, int dst_w, size_t dst_map_stride, int y0, int x0,
                                                    const float* __restrict__ src, int src_h, int src_w, size_t src_map_stride) {
    const int x = (int)blockIdx.x, map = (int)blockIdx.y;
    if (x >= src_w || x0 + x >= dst_w) return;
    const float* s = src + (size_t)map * src_map_stride + (size_t)x * src_h;
    float* d = dst + (size_t)map * dst_map_stride + (size_t)(x0 + x) * dst_h + y0;
    const int n = src_h < dst_h - y0 ? src_h : dst_h - y0;
    for (int y = (int)threadIdx.x; y < n; y += (int)blockDim.x) d[y] += s[y];
}

// dst map (dst_h x dst_w, contiguous) = the window [off_h, off_h + dst_h) x [off_w, off_w + dst_w) of the
// src map (src_h rows per column): the "full" / "same" / "valid" regions of the padded window; sampled at the strides (sh, sw)
// from the window's first row and column (strided maps; 1, 1: the plain crop)
__global__ void __launch_bounds__(256) k_crop_maps(const float* __restrict__ src, int src_h, size_t src_map_stride, float* __restrict__ dst,
                                                   int dst_h, int dst_w, size_t dst_map_stride, int off_h, int off_w, int sh, int sw) {
    const int x = (int)blockIdx.x, map = (int)blockIdx.y;
    const float* s = src + (size_t)map * src_map_stride + (size_t)(off_w + x * sw) * src_h + off_h;
    float* d = dst + (size_t)map * dst_map_stride + (size_t)x * dst_h;
    for (int y = (int)threadIdx.x; y < dst_h; y += (int)blockDim.x) d[y] = s[(size_t)y * sh];
}

// the same into 16-bit maps (fp16 / bf16: fc_map16): the source is the fp32 full-window staging.  Region maps can have an odd
// out_h and an odd element count, so the destination is only 2-byte aligned: one element per store.
__global__ void __launch_bounds__(256) k_crop_maps16(const float* __restrict__ src, int src_h, size_t src_map_stride, uint16_t* __restrict__ dst,
                                                     int dst_h, int dst_w, size_t dst_map_stride, int off_h, int off_w, int sh, int sw, int bf16) {
    const int x = (int)blockIdx.x, map = (int)blockIdx.y;
    const float* s = src + (size_t)map * src_map_stride + (size_t)(off_w + x * sw) * src_h + off_h;
    uint16_t* d = dst + (size_t)map * dst_map_stride + (size_t)x * dst_h;
    for (int y = (int)threadIdx.x; y < dst_h; y += (int)blockDim.x) d[y] = fc_map16(s[(size_t)y * sh], bf16 != 0);
}

// Image spectrum between the engine's internal order and the reference's natural order
// [f][FFT_W][FFT_H/2+1] (cufftExecR2C output, src/cudaFFTData.cu:90-103): natural element (x, y) of
// plane f is internal element S[f][row_of[y]][col_of[x]]; `scale` undoes / applies the folded
// normalisation.  A one-off utility: no attempt at coalescing the permuted side.
template <bool EXPORT>
__global__ void __launch_bounds__(256) k_spectrum_reorder(c32* __restrict__ S, size_t s_plane, int s_pitch, c32* __restrict__ nat, int fw, int ch,
                                                          const int* __restrict__ row_of, const int* __restrict__ col_of, float scale) {
    const int x = (int)blockIdx.x, f = (int)blockIdx.y;
    const size_t base = (size_t)f * s_plane + col_of[x];
    c32* n = nat + ((size_t)f * fw + x) * ch;
    for (int y = (int)threadIdx.x; y < ch; y += (int)blockDim.x) {
        const size_t i = base + (size_t)row_of[y] * s_pitch;
        if (EXPORT) n[y] = scale * S[i];
        else S[i] = scale * n[y];
    }
}

// dst map (dst_h x dst_w, contiguous, LARGER than the source) = the src map in its top-left corner,
// zeros elsewhere: the reference's alternative next-power-of-two window (computeFFTsize,
// src/cudaConvFFTData.h:67-94) around the ceil16 window the engine computes
__global__ void __launch_bounds__(256) k_pad_maps(const float* __restrict__ src, int src_h, int src_w, size_t src_map_stride,
                                                  float* __restrict__ dst, int dst_h, size_t dst_map_stride) {
    const int x = (int)blockIdx.x, map = (int)blockIdx.y;
    const float* s = src + (size_t)map * src_map_stride + (size_t)x * src_h;
    float* d = dst + (size_t)map * dst_map_stride + (size_t)x * dst_h;
    const int n = x < src_w ? src_h : 0;
    for (int y = (int)threadIdx.x; y < dst_h; y += (int)blockDim.x) d[y] = y < n ? s[y] : 0.f;
}

__global__ void __launch_bounds__(256) k_pad_maps16(const float* __restrict__ src, int src_h, int src_w, size_t src_map_stride,
                                                    uint16_t* __restrict__ dst, int dst_h, size_t dst_map_stride, int bf16) {
    const int x = (int)blockIdx.x, map = (int)blockIdx.y;
    const float* s = src + (size_t)map * src_map_stride + (size_t)x * src_h;
    uint16_t* d = dst + (size_t)map * dst_map_stride + (size_t)x * dst_h;
    const int n = x < src_w ? src_h : 0;
    for (int y = (int)threadIdx.x; y < dst_h; y += (int)blockDim.x) d[y] = fc_map16(y < n ? s[y] : 0.f, bf16 != 0);
}

}  // namespace

// the plane of a crop / pad launch is filled in (fast_paths.hpp: MapPlane)
static bool maps_plane_ok(const MapPlane& pl) {
    if (pl.kind == PlaneKind::None) return true;
    return pl.plane && pl.per_image >= 1 && pl.first >= 0 && pl.first % pl.per_image == 0 && (pl.kind != PlaneKind::Add || pl.consts);
}

hipError_t launch_pad_maps(const float* src, int src_h, int src_w, size_t src_map_stride, float* dst, int dst_h, int dst_w,
                           size_t dst_map_stride, int nmaps, hipStream_t s, int format, const MapPlane& plane) {
    if (nmaps <= 0 || dst_h <= 0 || dst_w <= 0) return hipSuccess;
    if (!maps_plane_ok(plane) || (plane.kind != PlaneKind::None && dst_h < src_h)) return hipErrorInvalidValue;
    const MapsLaunch l{src, src_h, src_w, src_map_stride, dst, dst_h, dst_w, dst_map_stride, 0, 0, nmaps, format, s};
    if (plane.kind == PlaneKind::Scale) return pad_maps_scaled(l, plane);
    if (plane.kind == PlaneKind::Add) return pad_maps_added(l, plane);
    return l.run([&](dim3 g, dim3 b, uint16_t* d, int bf16) { hipLaunchKernelGGL(k_pad_maps16, g, b, 0, s, src, src_h, src_w, src_map_stride, d, dst_h, dst_map_stride, bf16); },
                 [&](dim3 g, dim3 b, float* d, int) { hipLaunchKernelGGL(k_pad_maps, g, b, 0, s, src, src_h, src_w, src_map_stride, d, dst_h, dst_map_stride); });
}

hipError_t launch_spectrum_reorder(bool to_natural, c32* S, size_t s_plane, int s_pitch, c32* nat, int fw, int ch, int planes,
                                   const int* row_of, const int* col_of, float scale, hipStream_t s) {
    if (fw <= 0 || ch <= 0 || planes <= 0) return hipSuccess;
    if (to_natural) hipLaunchKernelGGL(k_spectrum_reorder<true>, dim3((unsigned)fw, (unsigned)planes), dim3(256), 0, s, S, s_plane, s_pitch, nat, fw, ch, row_of, col_of, scale);
    else hipLaunchKernelGGL(k_spectrum_reorder<false>, dim3((unsigned)fw, (unsigned)planes), dim3(256), 0, s, S, s_plane, s_pitch, nat, fw, ch, row_of, col_of, scale);
    return hipGetLastError();
}

hipError_t launch_flip_planes(const float* src, float* dst, int plane_elems, long nplanes, hipStream_t s) {
    const long total = (long)plane_elems * nplanes;
    if (total <= 0) return hipSuccess;
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(k_flip_planes, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, src, dst, plane_elems, total);
    return hipGetLastError();
}

hipError_t launch_add_window(float* dst, int dst_h, int dst_w, size_t dst_map_stride, int y0, int x0, const float* src, int src_h,
                             int src_w, size_t src_map_stride, int nmaps, hipStream_t s) {
    if (nmaps <= 0 || src_w <= 0 || src_h <= 0 || y0 >= dst_h || x0 >= dst_w) return hipSuccess;
    hipLaunchKernelGGL(k_add_window, dim3((unsigned)src_w, (unsigned)nmaps), dim3(256), 0, s, dst, dst_h, dst_w, dst_map_stride, y0, x0,
                       src, src_h, src_w, src_map_stride);
    return hipGetLastError();
}

hipError_t launch_crop_maps(const float* src, int src_h, size_t src_map_stride, float* dst, int dst_h, int dst_w, size_t dst_map_stride,
                            int off_h, int off_w, int nmaps, hipStream_t s, int format, const MapPlane& plane, int stride_h, int stride_w) {
    if (nmaps <= 0 || dst_h <= 0 || dst_w <= 0) return hipSuccess;
    if (!maps_plane_ok(plane) || stride_h < 1 || stride_w < 1) return hipErrorInvalidValue;
    const MapsLaunch l{src, src_h, 0, src_map_stride, dst, dst_h, dst_w, dst_map_stride, off_h, off_w, nmaps, format, s, stride_h, stride_w};
    const int sh = stride_h, sw = stride_w;
    if (plane.kind == PlaneKind::Scale) return crop_maps_scaled(l, plane);
    if (plane.kind == PlaneKind::Add) return crop_maps_added(l, plane);
    return l.run([&](dim3 g, dim3 b, uint16_t* d, int bf16) { hipLaunchKernelGGL(k_crop_maps16, g, b, 0, s, src, src_h, src_map_stride, d, dst_h, dst_w, dst_map_stride, off_h, off_w, sh, sw, bf16); },
                 [&](dim3 g, dim3 b, float* d, int) { hipLaunchKernelGGL(k_crop_maps, g, b, 0, s, src, src_h, src_map_stride, d, dst_h, dst_w, dst_map_stride, off_h, off_w, sh, sw); });
}

// ---- the specialised kernels: their translation units (kernels_*_g<G>.hip) hold one group of configurations each; the
// ---- first group that has the length takes the launch (f: the call of group g.value's entry point, kernels.hpp)
template <int N, class F>
hipError_t in_first_group(F&& f) {
    return first_group<N>(f).value_or(hipErrorInvalidValue);
}

hipError_t launch_fast_rows_fwd(int L, const FastRowsFwdArgs& a, int rows, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    return in_first_group<FC_ROW_GROUPS>([&](auto g) { return launch_fast_rows_fwd_group<g.value>(L, a, rows, s); });
}

hipError_t launch_fast_rows_multi(int L, int nz2, const FastRowsArgs& a, int rows, int kernels, int kernels_per_wg, hipStream_t s) {
    if (rows <= 0 || kernels <= 0) return hipSuccess;
    if (a.F < 1 || kernels_per_wg < 1) return hipErrorInvalidValue;
    if (a.images > 1 && a.kernels_per_image != kernels) return hipErrorInvalidValue;   // (image batches: `kernels` counts per image)
    return in_first_group<FC_ROW_GROUPS>([&](auto g) { return launch_fast_rows_multi_group<g.value>(L, nz2, a, rows, kernels, kernels_per_wg, s); });
}

hipError_t launch_fast_rows_filter(int L, int nz2, const FastRowsArgs& a, int rows, int kernels, int kernels_per_wg, hipStream_t s) {
    if (rows <= 0 || kernels <= 0) return hipSuccess;
    if (a.F != 1 || kernels_per_wg < 1 || !fc_filter_mode_ok(a.filter_mode)) return hipErrorInvalidValue;
    if (a.images > 1 && a.kernels_per_image != kernels) return hipErrorInvalidValue;   // (image batches: `kernels` counts per image)
    return in_first_group<FC_ROW_GROUPS>([&](auto g) { return launch_fast_rows_filter_group<g.value>(L, nz2, a, rows, kernels, kernels_per_wg, s); });
}

hipError_t launch_fast_rows_images(int L, const FastRowsArgs& a, int rows, int images_per_wg, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (a.F != 1 || images_per_wg < 1 || a.images < 1 || a.kernels_per_image < 1) return hipErrorInvalidValue;
    return in_first_group<FC_ROW_GROUPS>([&](auto g) { return launch_fast_rows_images_group<g.value>(L, a, rows, images_per_wg, s); });
}

hipError_t fast_rows_multi_wgs_per_cu(int L, int nz2, const FastRowsArgs& a, int* wgs_per_cu) {
    return in_first_group<FC_ROW_GROUPS>([&](auto g) { return fast_rows_multi_wgs_per_cu_group<g.value>(L, nz2, a, wgs_per_cu); });
}

hipError_t launch_fast_cols(int M, int T, const FastColsArgs& a, int num_cus, hipStream_t s) {
    if (a.ntiles <= 0) return hipSuccess;
    if (a.out_format != FC_MAP_F32)     // 16-bit maps: the instantiations of kernels_cols16_g<G>.hip
        return in_first_group<FC_COL_GROUPS>([&](auto g) { return launch_fast_cols16_group<g.value>(M, T, a, num_cus, s); });
    return in_first_group<FC_COL_GROUPS>([&](auto g) { return launch_fast_cols_group<g.value>(M, T, a, num_cus, s); });
}

hipError_t launch_fast_cols_rect(int M, int T, const FastColsShape& shape, hipStream_t s) {
    if (shape.a.ntiles <= 0) return hipSuccess;
    if (!shape.a.y_tiled || (shape.variant != FastColsVariant::TILED && shape.variant != FastColsVariant::TILED_DYN)) return hipErrorInvalidValue;
    const bool f32 = shape.a.out_format == FC_MAP_F32;
    const MapPlane& pl = shape.plane;
    if (shape.strided) {
        // (fp32, no plane; the reciprocals of the strides are exact for extents below 2^16: fast_cols.hpp, StrideDiv)
        if (!f32 || pl.kind != PlaneKind::None || shape.a.fft_h - shape.a.h_lo >= 65536 || shape.a.rect_w_n >= 65536) return hipErrorInvalidValue;
        return in_first_group<FC_COL_GROUPS>([&](auto g) { return launch_fast_cols_rect_stride_group<g.value>(M, T, shape, s); });
    }
    if (pl.kind == PlaneKind::Scale) {
        if (!f32 || !pl.plane || pl.per_image < 1) return hipErrorInvalidValue;
        return in_first_group<FC_COL_GROUPS>([&](auto g) { return launch_fast_cols_rect_scale_group<g.value>(M, T, shape, s); });
    }
    if (pl.kind == PlaneKind::Add) {
        if (!f32 || !fast_cols_sqdiff_args_ok(fast_cols_sqdiff_args(pl))) return hipErrorInvalidValue;
        return in_first_group<FC_COL_GROUPS>([&](auto g) { return launch_fast_cols_rect_add_group<g.value>(M, T, shape, s); });
    }
    if (!f32) return in_first_group<FC_COL_GROUPS>([&](auto g) { return launch_fast_cols_rect16_group<g.value>(M, T, shape, s); });
    return in_first_group<FC_COL_GROUPS>([&](auto g) { return launch_fast_cols_rect_group<g.value>(M, T, shape, s); });
}

hipError_t launch_fast_cols_fwd(int M, int T, bool pruned, const FastColsFwdArgs& a, int num_cus, hipStream_t s) {
    if (a.ntiles <= 0) return hipSuccess;
    return in_first_group<FC_COL_GROUPS>([&](auto g) { return launch_fast_cols_fwd_group<g.value>(M, T, pruned, a, num_cus, s); });
}

hipError_t launch_fast_cols_fwd_px(int M, int T, const FastColsFwdArgs& a, const PixelLoad& px, int num_cus, hipStream_t s) {
    if (a.ntiles <= 0) return hipSuccess;
    if (!fc_pixel_format_ok(px.format) || px.format == FC_PIXEL_F32) return hipErrorInvalidValue;
    return in_first_group<FC_COL_GROUPS>([&](auto g) { return launch_fast_cols_fwd_px_group<g.value>(M, T, a, px, num_cus, s); });
}

hipError_t launch_fast_cols_fwd_border(int M, int T, const FastColsFwdArgs& a, const BorderLoad& bd, int num_cus, hipStream_t s) {
    if (a.ntiles <= 0) return hipSuccess;
    if (!fc_border_mode_ok(bd.mode) || bd.mode == FC_BORDER_ZERO) return hipErrorInvalidValue;
    return in_first_group<FC_COL_GROUPS>([&](auto g) { return launch_fast_cols_fwd_border_group<g.value>(M, T, a, bd, num_cus, s); });
}

hipError_t launch_fast_cols_fwd_pair(int M, int T, const FastColsFwdArgs& image, const FastColsFwdArgs& kernels, bool kernels_pruned,
                                     int num_cus, hipStream_t s) {
    if (image.ntiles <= 0 || kernels.ntiles <= 0) return hipErrorInvalidValue;
    return in_first_group<FC_COL_GROUPS>([&](auto g) { return launch_fast_cols_fwd_pair_group<g.value>(M, T, image, kernels, kernels_pruned, num_cus, s); });
}

hipError_t kernels_init() {
    const int lim = 160 * 1024;
    const void* generic[] = {reinterpret_cast<const void*>(k_cols_r2c<0>),      reinterpret_cast<const void*>(k_cols_r2c<1>),
                             reinterpret_cast<const void*>(k_rows_fwd<0>),      reinterpret_cast<const void*>(k_rows_fwd<1>),
                             reinterpret_cast<const void*>(k_spectral_rows<0>), reinterpret_cast<const void*>(k_spectral_rows<1>),
                             reinterpret_cast<const void*>(k_cols_c2r<0>),      reinterpret_cast<const void*>(k_cols_c2r<1>),
                             reinterpret_cast<const void*>(k_cols_c2r16<0>),    reinterpret_cast<const void*>(k_cols_c2r16<1>)};
    for (const void* k : generic) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lim);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_cols_r2c(const ColsR2CArgs& a, int tiles, int planes, int threads, size_t lds_bytes, hipStream_t s) {
    if (tiles <= 0 || planes <= 0) return hipSuccess;
    if (a.fd.bs_work > 0) hipLaunchKernelGGL(k_cols_r2c<1>, dim3(tiles, planes), dim3(threads), lds_bytes, s, a);
    else hipLaunchKernelGGL(k_cols_r2c<0>, dim3(tiles, planes), dim3(threads), lds_bytes, s, a);
    return hipGetLastError();
}
hipError_t launch_rows_fwd(const RowsFwdArgs& a, int rows, int threads, size_t lds_bytes, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (a.fd.bs_work > 0) hipLaunchKernelGGL(k_rows_fwd<1>, dim3(rows), dim3(threads), lds_bytes, s, a);
    else hipLaunchKernelGGL(k_rows_fwd<0>, dim3(rows), dim3(threads), lds_bytes, s, a);
    return hipGetLastError();
}
hipError_t launch_spectral_rows(const SpectralRowsArgs& a, int rows, int kernels, int threads, size_t lds_bytes, hipStream_t s) {
    if (rows <= 0 || kernels <= 0) return hipSuccess;
    // (image batches: `kernels` per image, a.images images -- a.kernels_per_image places an image's maps in Y)
    // (where it is set at all it must be the launch's kernel count: the body splits every slot with it)
    if ((a.images > 1 || a.kernels_per_image != 0) && a.kernels_per_image != kernels) return hipErrorInvalidValue;
    const dim3 grid(rows, kernels, rows_images(a.images));
    if (a.fd.bs_work > 0) hipLaunchKernelGGL(k_spectral_rows<1>, grid, dim3(threads), lds_bytes, s, a);
    else hipLaunchKernelGGL(k_spectral_rows<0>, grid, dim3(threads), lds_bytes, s, a);
    return hipGetLastError();
}
hipError_t launch_cols_c2r(const ColsC2RArgs& a, int tiles, int kernels, int threads, size_t lds_bytes, hipStream_t s) {
    if (tiles <= 0 || kernels <= 0) return hipSuccess;
    if (a.out_format != FC_MAP_F32) {
        if (a.fd.bs_work > 0) hipLaunchKernelGGL(k_cols_c2r16<1>, dim3(tiles, kernels), dim3(threads), lds_bytes, s, a);
        else hipLaunchKernelGGL(k_cols_c2r16<0>, dim3(tiles, kernels), dim3(threads), lds_bytes, s, a);
        return hipGetLastError();
    }
    if (a.fd.bs_work > 0) hipLaunchKernelGGL(k_cols_c2r<1>, dim3(tiles, kernels), dim3(threads), lds_bytes, s, a);
    else hipLaunchKernelGGL(k_cols_c2r<0>, dim3(tiles, kernels), dim3(threads), lds_bytes, s, a);
    return hipGetLastError();
}

}  // namespace fc
