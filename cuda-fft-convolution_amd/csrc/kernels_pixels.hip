// kernels_pixels.hip -- typed image pixels (fftconv_plan_set_images_typed; pixel_format.hpp), the STAGED route: one small kernel
// writes the exact fp32 value of every uint8 / uint16 / fp16 / bf16 element into the plan's fp32 image staging, and everything
// then runs as for an fp32 image.  Serves the plans whose image column pass is not the specialised kernel (generic, Bluestein,
// block-wise), the configurations whose typed column kernel is not built, and plan option "pixel_store" 0.  Not on the hot path
// of a plan that has the typed column kernel.  Also here, so that kernels_ncc.hip compiles what it compiled before: pass 1 of
// the window statistics of normalised maps over typed pixels, which the DIRECT route needs.
#include "kernels.hpp"
#include "border.hpp"
#include "ncc.hpp"
#include "pixel_format.hpp"

namespace fc {
namespace {

// element loads (the source may start at any element) in a grid-stride loop
template <class Px>
__global__ void __launch_bounds__(256) k_pixels_to_f32(const pixel_elem_t<Px>* __restrict__ src, float* __restrict__ dst, size_t n, PixelLoad px) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) dst[i] = pixel_value(src[i], px);
}

// pass 1 of the window statistics of normalised maps (kernels_ncc.hip: k_ncc_column_sums, whose text this is) over an image of
// typed pixels: on the direct route no fp32 image exists for the fp32 kernel to read.  The element goes to float64 through
// its exact fp32 value, so the sums are the fp32 image's to the bit.
template <class Px>
__global__ void __launch_bounds__(256) k_ncc_column_sums_px(const pixel_elem_t<Px>* __restrict__ img, int H, int W, int fft_h, int box_h, int w_start,
                                                            int ncols, double* __restrict__ c1, double* __restrict__ c2, PixelLoad px) {
    const int c = (int)blockIdx.x, f = (int)blockIdx.y, w = w_start + c;
    const size_t at = ((size_t)f * ncols + c) * fft_h;
    const bool data = w >= 0 && w < W;
    const pixel_elem_t<Px>* col = img + ((size_t)f * W + (data ? w : 0)) * H;
    const int i = (int)(blockIdx.z * blockDim.x + threadIdx.x);      // (one element per thread: blockIdx.z walks the rows)
    if (i >= fft_h) return;
    double s1 = 0.0, s2 = 0.0;
    if (data) ncc_column_sums<Px>(col, H, i, box_h, s1, s2, px);
    c1[at + i] = s1;
    c2[at + i] = s2;
}

// Border modes (border.hpp; fftconv_plan_set_border), the STAGED route: the extended image E -- (H + MAXK_H - 1) x (W + MAXK_W - 1)
// samples per plane, through the index function the bordered column kernel maps its loads with -- written into the plan's
// staging; the column pass then runs on it as on an image of that size.  Not on the hot path of a plan that has the bordered
// column kernel.  (One element per iteration of a grid-stride loop; the divisions are by uniforms.)
__global__ void __launch_bounds__(256) k_extend_image(const float* __restrict__ src, float* __restrict__ dst, int H, int W, int ext_h, int ext_w,
                                                      size_t n, BorderLoad bd) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const size_t cq = i / (size_t)ext_h;
        const int r = (int)(i - cq * (size_t)ext_h);
        const size_t q = cq / (size_t)ext_w;
        const int c = (int)(cq - q * (size_t)ext_w);
        dst[i] = border_sample(src + q * ((size_t)H * W), H, bd, r, c);
    }
}

}  // namespace

hipError_t launch_extend_image(const float* src, float* dst, int H, int W, int ext_h, int ext_w, size_t planes, const BorderLoad& bd, hipStream_t s) {
    const size_t n = planes * (size_t)ext_h * ext_w;
    if (n == 0) return hipSuccess;
    if (!fc_border_mode_ok(bd.mode) || bd.mode == FC_BORDER_ZERO || ext_h < H || ext_w < W) return hipErrorInvalidValue;
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_extend_image, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s, src, dst, H, W, ext_h, ext_w, n, bd);
    return hipGetLastError();
}

void launch_ncc_column_sums_px(const void* img, const PixelLoad& px, int H, int W, int F, int fft_h, int box_h, int w_start, int ncols, double* c1,
                               double* c2, hipStream_t s) {
    const dim3 grid((unsigned)ncols, (unsigned)F, (unsigned)((fft_h + 255) / 256));
    if (fc_pixel_elem_bytes(px.format) == 1)
        hipLaunchKernelGGL(k_ncc_column_sums_px<Pixel8>, grid, dim3(256), 0, s, static_cast<const uint8_t*>(img), H, W, fft_h, box_h, w_start, ncols, c1, c2, px);
    else
        hipLaunchKernelGGL(k_ncc_column_sums_px<Pixel16>, grid, dim3(256), 0, s, static_cast<const uint16_t*>(img), H, W, fft_h, box_h, w_start, ncols, c1, c2, px);
}

hipError_t launch_pixels_to_f32(const void* src, int pixel_format, float* dst, size_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (!fc_pixel_format_ok(pixel_format) || pixel_format == FC_PIXEL_F32) return hipErrorInvalidValue;
    const size_t blocks = (n + 255) / 256;
    const dim3 grid((unsigned)(blocks < 8192 ? blocks : 8192));
    PixelLoad px;
    px.format = pixel_format;
    if (fc_pixel_elem_bytes(pixel_format) == 1)
        hipLaunchKernelGGL(k_pixels_to_f32<Pixel8>, grid, dim3(256), 0, s, static_cast<const uint8_t*>(src), dst, n, px);
    else
        hipLaunchKernelGGL(k_pixels_to_f32<Pixel16>, grid, dim3(256), 0, s, static_cast<const uint16_t*>(src), dst, n, px);
    return hipGetLastError();
}

}  // namespace fc
