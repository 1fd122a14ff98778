// kernels_ncc.hip -- normalised cross-correlation maps (fftconv_plan_set_normalisation; ncc.hpp): the window statistics of an
// image (once per image), the normalisation of the kernels (once per kernel), and the crop / pad kernels that scale a staged
// fp32 window by D on its way into the maps (the Scale plane of launch_crop_maps / launch_pad_maps).  None of the first two is on the hot path.
#include "kernels.hpp"
#include "ncc.hpp"
#include "ncc_device.hpp"

namespace fc {
namespace {

// pass 1 of the statistics: float64 sums along h over the box, for the strip columns [w_start, w_start + ncols) of every
// feature plane of one image ([f][W][H]); a strip column outside [0, W) is padding: zeros
__global__ void __launch_bounds__(256) k_ncc_column_sums(const float* __restrict__ img, int H, int W, int fft_h, int box_h, int w_start, int ncols,
                                                         double* __restrict__ c1, double* __restrict__ c2) {
    const int c = (int)blockIdx.x, f = (int)blockIdx.y, w = w_start + c;
    const size_t at = ((size_t)f * ncols + c) * fft_h;
    const bool data = w >= 0 && w < W;
    const float* col = img + ((size_t)f * W + (data ? w : 0)) * H;
    const int i = (int)(blockIdx.z * blockDim.x + threadIdx.x);      // (one element per thread: blockIdx.z walks the rows)
    if (i >= fft_h) return;
    double s1 = 0.0, s2 = 0.0;
    if (data) ncc_column_sums(col, H, i, box_h, s1, s2);
    c1[at + i] = s1;
    c2[at + i] = s2;
}

// pass 2: sums along w over the box, the feature sum and the floor -- window columns [j0, j0 + nout) of D (d: column j0)
__global__ void __launch_bounds__(256) k_ncc_scale(const double* __restrict__ c1, const double* __restrict__ c2, int ncols, int fft_h, int F, int box_w,
                                                   int n, float* __restrict__ d) {
    const int c = (int)blockIdx.x, i = (int)(blockIdx.y * blockDim.x + threadIdx.x);
    if (i >= fft_h) return;
    d[(size_t)c * fft_h + i] = ncc_scale(c1, c2, (size_t)ncols * fft_h, fft_h, F, c + box_w - 1, i, box_w, n);
}

// kernels: one workgroup of FC_NCC_LANES threads per plane (mean, sum of squares around it: ncc.hpp's lanes and fold), then
// T'' -- every thread of a kernel's workgroup sums the F plane figures in the same order
__global__ void __launch_bounds__(FC_NCC_LANES) k_ncc_plane_stats(const float* __restrict__ src, int pe, double* __restrict__ stats) {
    __shared__ double part[FC_NCC_LANES];
    const int t = (int)threadIdx.x;
    const size_t pl = blockIdx.x;
    const float* plane = src + pl * pe;
    const double mean = fold_lanes(part, t, ncc_lane_sum(plane, pe, t, 0.0, false)) / (double)pe;
    const double ssq = fold_lanes(part, t, ncc_lane_sum(plane, pe, t, mean, true));
    if (t == 0) {
        stats[2 * pl] = mean;
        stats[2 * pl + 1] = ssq;
    }
}
__global__ void __launch_bounds__(256) k_ncc_unit_kernels(const float* __restrict__ src, float* __restrict__ dst, int F, int pe,
                                                          const double* __restrict__ stats) {
    const int k = (int)blockIdx.x;
    const double* st = stats + (size_t)2 * F * k;
    const double norm = ncc_kernel_norm(st, F);
    const size_t base = (size_t)k * F * pe;
    for (int e = (int)threadIdx.x; e < F * pe; e += (int)blockDim.x) dst[base + e] = ncc_unit(src[base + e], st[2 * (e / pe)], norm);
}

// NORM siblings of k_crop_maps / k_crop_maps16 (kernels.hip): the element is scaled by D at its WINDOW coordinate while it is
// cropped (sampled at the strides sh, sw: strided maps) and converted.  Map `map` of the launch belongs to image image0 + map / per_image (ncc_image_of); D: [image][src_w][src_h]
template <bool OUT16>
__global__ void __launch_bounds__(256) k_crop_maps_norm(const float* __restrict__ src, int src_h, size_t src_map_stride,
                                                        std::conditional_t<OUT16, uint16_t, float>* __restrict__ dst, int dst_h, size_t dst_map_stride,
                                                        int off_h, int off_w, int sh, int sw, const float* __restrict__ D, int image0, int per_image, int bf16) {
    const int x = (int)blockIdx.x, map = (int)blockIdx.y;
    const size_t at = (size_t)(off_w + x * sw) * src_h + off_h;
    const float* s = src + (size_t)map * src_map_stride + at;
    const float* sc = D + (size_t)ncc_image_of(image0, map, per_image) * src_map_stride + at;
    auto* d = dst + (size_t)map * dst_map_stride + (size_t)x * dst_h;
    for (int y = (int)threadIdx.x; y < dst_h; y += (int)blockDim.x) put<OUT16>(d + y, s[(size_t)y * sh] * sc[(size_t)y * sh], bf16);
}

// ... and of k_pad_maps / k_pad_maps16
template <bool OUT16>
__global__ void __launch_bounds__(256) k_pad_maps_norm(const float* __restrict__ src, int src_h, int src_w, size_t src_map_stride,
                                                       std::conditional_t<OUT16, uint16_t, float>* __restrict__ dst, int dst_h, size_t dst_map_stride,
                                                       const float* __restrict__ D, int image0, int per_image, int bf16) {
    const int x = (int)blockIdx.x, map = (int)blockIdx.y;
    const int n = x < src_w ? src_h : 0;
    const size_t at = (size_t)(n ? x : 0) * src_h;
    const float* s = src + (size_t)map * src_map_stride + at;
    const float* sc = D + (size_t)ncc_image_of(image0, map, per_image) * src_map_stride + at;
    auto* d = dst + (size_t)map * dst_map_stride + (size_t)x * dst_h;
    for (int y = (int)threadIdx.x; y < dst_h; y += (int)blockDim.x) put<OUT16>(d + y, y < n ? s[y] * sc[y] : 0.f, bf16);
}

}  // namespace

hipError_t launch_ncc_statistics(const float* img, int H, int W, int F, int fft_h, int fft_w, int box_h, int box_w, double* scratch,
                                 int strip_cols, float* d, hipStream_t s) {
    return launch_ncc_statistics_typed(img, FC_PIXEL_F32, H, W, F, fft_h, fft_w, box_h, box_w, scratch, strip_cols, d, s);
}

hipError_t launch_ncc_statistics_typed(const void* vimg, int pixel_format, int H, int W, int F, int fft_h, int fft_w, int box_h, int box_w,
                                       double* scratch, int strip_cols, float* d, hipStream_t s) {
    return launch_score_statistics_typed(FC_SCORE_CCOEFF_NORMED, vimg, pixel_format, H, W, F, fft_h, fft_w, box_h, box_w, scratch, strip_cols, d, s);
}

hipError_t launch_score_statistics_typed(int score, const void* vimg, int pixel_format, int H, int W, int F, int fft_h, int fft_w, int box_h, int box_w,
                                         double* scratch, int strip_cols, float* d, hipStream_t s) {
    if (!score_has_plane(score)) return hipErrorInvalidValue;
    if (fft_h <= 0 || fft_w <= 0 || F <= 0) return hipSuccess;
    if (box_h < 1 || box_w < 1 || strip_cols < box_w || !fc_pixel_format_ok(pixel_format)) return hipErrorInvalidValue;
    const float* img = static_cast<const float*>(vimg);
    PixelLoad px;
    px.format = pixel_format;
    const int per_strip = strip_cols - (box_w - 1);      // window columns a strip yields
    for (int j0 = 0; j0 < fft_w; j0 += per_strip) {
        const int nout = fft_w - j0 < per_strip ? fft_w - j0 : per_strip, ncols = nout + box_w - 1;
        double* c1 = scratch;
        double* c2 = scratch + (size_t)F * ncols * fft_h;
        const unsigned zr = (unsigned)((fft_h + 255) / 256);
        const dim3 grid((unsigned)ncols, (unsigned)F, zr);
        if (pixel_format == FC_PIXEL_F32)
            hipLaunchKernelGGL(k_ncc_column_sums, grid, dim3(256), 0, s, img, H, W, fft_h, box_h, j0 - (box_w - 1), ncols, c1, c2);
        else      // (typed pixels: the kernel lives in kernels_pixels.hip, so that this unit's device code stays what it was)
            launch_ncc_column_sums_px(vimg, px, H, W, F, fft_h, box_h, j0 - (box_w - 1), ncols, c1, c2, s);
        if (score == FC_SCORE_CCOEFF_NORMED)
            hipLaunchKernelGGL(k_ncc_scale, dim3((unsigned)nout, zr), dim3(256), 0, s, c1, c2, ncols, fft_h, F, box_w, box_h * box_w, d + (size_t)j0 * fft_h);
        else launch_score_plane(score, c2, ncols, nout, fft_h, F, box_w, d + (size_t)j0 * fft_h, s);      // (kernels_score.hip)
    }
    return hipGetLastError();
}

hipError_t launch_ncc_unit_kernels(const float* src, float* dst, int n, int F, int plane_elems, double* stats, hipStream_t s) {
    if (n <= 0 || F <= 0 || plane_elems <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ncc_plane_stats, dim3((unsigned)((long)n * F)), dim3(FC_NCC_LANES), 0, s, src, plane_elems, stats);
    hipLaunchKernelGGL(k_ncc_unit_kernels, dim3((unsigned)n), dim3(256), 0, s, src, dst, F, plane_elems, stats);
    return hipGetLastError();
}

void launch_ncc_plane_stats(const float* src, int planes, int plane_elems, double* stats, hipStream_t s) {
    hipLaunchKernelGGL(k_ncc_plane_stats, dim3((unsigned)planes), dim3(FC_NCC_LANES), 0, s, src, plane_elems, stats);
}

// the Scale entries of launch_crop_maps / launch_pad_maps (kernels.hpp: the arguments are checked there)
hipError_t crop_maps_scaled(const MapsLaunch& l, const MapPlane& pl) {
    const int image0 = pl.first / pl.per_image;
    auto launch = [&](auto kernel, dim3 g, dim3 b, auto* d, int bf16) {
        hipLaunchKernelGGL(kernel, g, b, 0, l.s, l.src, l.src_h, l.src_map_stride, d, l.dst_h, l.dst_map_stride, l.off_h, l.off_w, l.stride_h, l.stride_w, pl.plane, image0, pl.per_image, bf16);
    };
    return l.run([&](dim3 g, dim3 b, uint16_t* d, int bf16) { launch(k_crop_maps_norm<true>, g, b, d, bf16); },
                 [&](dim3 g, dim3 b, float* d, int bf16) { launch(k_crop_maps_norm<false>, g, b, d, bf16); });
}

hipError_t pad_maps_scaled(const MapsLaunch& l, const MapPlane& pl) {
    const int image0 = pl.first / pl.per_image;
    auto launch = [&](auto kernel, dim3 g, dim3 b, auto* d, int bf16) {
        hipLaunchKernelGGL(kernel, g, b, 0, l.s, l.src, l.src_h, l.src_w, l.src_map_stride, d, l.dst_h, l.dst_map_stride, pl.plane, image0, pl.per_image, bf16);
    };
    return l.run([&](dim3 g, dim3 b, uint16_t* d, int bf16) { launch(k_pad_maps_norm<true>, g, b, d, bf16); },
                 [&](dim3 g, dim3 b, float* d, int bf16) { launch(k_pad_maps_norm<false>, g, b, d, bf16); });
}

}  // namespace fc
