// kernels_score.hip -- the matching scores beside mode 1 (fftconv_plan_set_match_score; ncc.hpp): the planes Dc / Q of an image
// (once per image), the preparation of the kernels with their constants (once per kernel), and the crop / pad kernels of score 4
// that add Q + c to a staged fp32 window on its way into the maps.  A unit of its own, so that kernels_ncc.hip compiles the device
// code it compiled before.  Only the crop / pad kernels run per convolve, and only on the staged route.
#include "kernels.hpp"
#include "ncc.hpp"
#include "ncc_device.hpp"

namespace fc {
namespace {

// ... of scores 3 and 4 (ncc.hpp: score_plane): Dc or Q from the pass-1 sums of squares
__global__ void __launch_bounds__(256) k_score_plane(const double* __restrict__ c2, int ncols, int fft_h, int F, int box_w, int score, float* __restrict__ d) {
    const int c = (int)blockIdx.x, i = (int)(blockIdx.y * blockDim.x + threadIdx.x);
    if (i >= fft_h) return;
    d[(size_t)c * fft_h + i] = score_plane(score, c2, (size_t)ncols * fft_h, fft_h, F, c + box_w - 1, i, box_w);
}

// scores 2, 3 and 4 (ncc.hpp: score_kernel_elem): a workgroup per kernel takes t2 -- each plane's sum of squares by the lanes and
// the fold, the planes added in ascending order -- then writes the prepared kernel and, thread 0, its constant c_k = (float) t2
// (score 4 reads it; written for every score so that the array never holds stale values)
__global__ void __launch_bounds__(FC_NCC_LANES) k_score_kernels(const float* __restrict__ src, float* __restrict__ dst, int F, int pe, int score,
                                                                const double* __restrict__ stats, float* __restrict__ consts) {
    __shared__ double part[FC_NCC_LANES];
    const int k = (int)blockIdx.x, t = (int)threadIdx.x;
    const double* st = stats + (size_t)2 * F * k;
    const size_t base = (size_t)k * F * pe;
    double t2 = 0.0;
    for (int f = 0; f < F; f++) t2 += fold_lanes(part, t, ncc_lane_sum(src + base + (size_t)f * pe, pe, t, 0.0, true));
    for (int e = t; e < F * pe; e += FC_NCC_LANES) dst[base + e] = score_kernel_elem(score, src[base + e], st[2 * (e / pe)], 0.0, t2);
    if (t == 0) consts[k] = (float)t2;
}

// ADD siblings (score 4, SQDIFF): the element becomes s + (Q + c) -- score_sqdiff: two fp32 adds in that order -- with Q the plane
// of the map's image and c the constant of its kernel, consts[map % per_image]
template <bool OUT16>
__global__ void __launch_bounds__(256) k_crop_maps_sqdiff(const float* __restrict__ src, int src_h, size_t src_map_stride,
                                                          std::conditional_t<OUT16, uint16_t, float>* __restrict__ dst, int dst_h, size_t dst_map_stride,
                                                          int off_h, int off_w, int sh, int sw, const float* __restrict__ Q, const float* __restrict__ consts,
                                                          int image0, int per_image, int bf16) {
    const int x = (int)blockIdx.x, map = (int)blockIdx.y;
    const size_t at = (size_t)(off_w + x * sw) * src_h + off_h;
    const float* s = src + (size_t)map * src_map_stride + at;
    const float* q = Q + (size_t)ncc_image_of(image0, map, per_image) * src_map_stride + at;
    const float c = consts[map % per_image];
    auto* d = dst + (size_t)map * dst_map_stride + (size_t)x * dst_h;
    for (int y = (int)threadIdx.x; y < dst_h; y += (int)blockDim.x) put<OUT16>(d + y, score_sqdiff(s[(size_t)y * sh], q[(size_t)y * sh], c), bf16);
}
template <bool OUT16>
__global__ void __launch_bounds__(256) k_pad_maps_sqdiff(const float* __restrict__ src, int src_h, int src_w, size_t src_map_stride,
                                                         std::conditional_t<OUT16, uint16_t, float>* __restrict__ dst, int dst_h, size_t dst_map_stride,
                                                         const float* __restrict__ Q, const float* __restrict__ consts, int image0, int per_image, int bf16) {
    const int x = (int)blockIdx.x, map = (int)blockIdx.y;
    const int n = x < src_w ? src_h : 0;
    const size_t at = (size_t)(n ? x : 0) * src_h;
    const float* s = src + (size_t)map * src_map_stride + at;
    const float* q = Q + (size_t)ncc_image_of(image0, map, per_image) * src_map_stride + at;
    const float c = consts[map % per_image];
    auto* d = dst + (size_t)map * dst_map_stride + (size_t)x * dst_h;
    for (int y = (int)threadIdx.x; y < dst_h; y += (int)blockDim.x) put<OUT16>(d + y, y < n ? score_sqdiff(s[y], q[y], c) : 0.f, bf16);
}

}  // namespace

void launch_score_plane(int score, const double* c2, int ncols, int nout, int fft_h, int F, int box_w, float* d, hipStream_t s) {
    hipLaunchKernelGGL(k_score_plane, dim3((unsigned)nout, (unsigned)((fft_h + 255) / 256)), dim3(256), 0, s, c2, ncols, fft_h, F, box_w, score, d);
}

hipError_t launch_score_kernels(int score, const float* src, float* dst, int n, int F, int plane_elems, double* stats, float* consts, hipStream_t s) {
    if (score == FC_SCORE_CCOEFF_NORMED) return launch_ncc_unit_kernels(src, dst, n, F, plane_elems, stats, s);
    if (n <= 0 || F <= 0 || plane_elems <= 0) return hipSuccess;
    if (score < FC_SCORE_CCOEFF || score > FC_SCORE_SQDIFF || !consts) return hipErrorInvalidValue;
    if (score == FC_SCORE_CCOEFF)      // (the means; scores 3 and 4 read no plane statistics)
        launch_ncc_plane_stats(src, n * F, plane_elems, stats, s);
    hipLaunchKernelGGL(k_score_kernels, dim3((unsigned)n), dim3(FC_NCC_LANES), 0, s, src, dst, F, plane_elems, score, stats, consts);
    return hipGetLastError();
}

// the Add entries of launch_crop_maps / launch_pad_maps (kernels.hpp: the arguments are checked there)
hipError_t crop_maps_added(const MapsLaunch& l, const MapPlane& pl) {
    const int image0 = pl.first / pl.per_image;
    auto launch = [&](auto kernel, dim3 g, dim3 b, auto* d, int bf16) {
        hipLaunchKernelGGL(kernel, g, b, 0, l.s, l.src, l.src_h, l.src_map_stride, d, l.dst_h, l.dst_map_stride, l.off_h, l.off_w, l.stride_h, l.stride_w, pl.plane, pl.consts, image0,
                           pl.per_image, bf16);
    };
    return l.run([&](dim3 g, dim3 b, uint16_t* d, int bf16) { launch(k_crop_maps_sqdiff<true>, g, b, d, bf16); },
                 [&](dim3 g, dim3 b, float* d, int bf16) { launch(k_crop_maps_sqdiff<false>, g, b, d, bf16); });
}

hipError_t pad_maps_added(const MapsLaunch& l, const MapPlane& pl) {
    const int image0 = pl.first / pl.per_image;
    auto launch = [&](auto kernel, dim3 g, dim3 b, auto* d, int bf16) {
        hipLaunchKernelGGL(kernel, g, b, 0, l.s, l.src, l.src_h, l.src_w, l.src_map_stride, d, l.dst_h, l.dst_map_stride, pl.plane, pl.consts, image0, pl.per_image, bf16);
    };
    return l.run([&](dim3 g, dim3 b, uint16_t* d, int bf16) { launch(k_pad_maps_sqdiff<true>, g, b, d, bf16); },
                 [&](dim3 g, dim3 b, float* d, int bf16) { launch(k_pad_maps_sqdiff<false>, g, b, d, bf16); });
}

}  // namespace fc
