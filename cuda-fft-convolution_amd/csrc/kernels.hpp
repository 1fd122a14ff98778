// kernels.hpp -- host-callable launchers of the HIP kernels (kernels*.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <optional>

#include "fast_paths.hpp"
#include "kernels_body.hpp"
#include "peaks.hpp"

namespace fc {

// Raises the dynamic-LDS limit of every kernel to the full 160 KiB of a gfx950 CU.
hipError_t kernels_init();

// dst plane = src plane reversed (flip of a column-major kh x kw plane along both axes)
hipError_t launch_flip_planes(const float* src, float* dst, int plane_elems, long nplanes, hipStream_t s);
// dst[map][x0 + x][y0 + y] += src[map][x][y], clipped to the dst_h x dst_w window (column-major maps)
hipError_t launch_add_window(float* dst, int dst_h, int dst_w, size_t dst_map_stride, int y0, int x0, const float* src, int src_h,
                             int src_w, size_t src_map_stride, int nmaps, hipStream_t s);
// dst[map] (dst_h x dst_w, contiguous) = window of src[map] at (off_h, off_w); src has src_h rows per column
// (format: FC_MAP_* of dst -- a 16-bit dst is an opaque pointer whose stride counts 2-byte elements; src is fp32 whatever the format)
// (plane: every element is combined with the plane at its WINDOW coordinate on the way -- Scale: times D; Add: s + (Q + c), c =
//  consts[m % per_image] for map m of the launch -- the planes [image][src_w][src_h], src_map_stride apart; map m belongs to image
//  first / per_image + m / per_image, first a multiple of per_image.  The kernels: kernels_ncc.hip (Scale), kernels_score.hip (Add))
// (stride_h, stride_w: strided maps, fftconv_plan_set_output_stride -- dst element (y, x) is the window's (off_h + y * stride_h,
//  off_w + x * stride_w), dst_h and dst_w counting the SAMPLED rows and columns; the plane is read at that window coordinate)
hipError_t launch_crop_maps(const float* src, int src_h, size_t src_map_stride, float* dst, int dst_h, int dst_w, size_t dst_map_stride,
                            int off_h, int off_w, int nmaps, hipStream_t s, int format = FC_MAP_F32, const MapPlane& plane = {},
                            int stride_h = 1, int stride_w = 1);
// natural [f][fw][ch] <-> internal image-spectrum order (see kernels.hip: k_spectrum_reorder)
hipError_t launch_spectrum_reorder(bool to_natural, c32* S, size_t s_plane, int s_pitch, c32* nat, int fw, int ch, int planes,
                                   const int* row_of, const int* col_of, float scale, hipStream_t s);
// dst[map] (dst_h x dst_w >= src) = src[map] in the top-left corner, zero elsewhere (format, plane: as launch_crop_maps)
hipError_t launch_pad_maps(const float* src, int src_h, int src_w, size_t src_map_stride, float* dst, int dst_h, int dst_w,
                           size_t dst_map_stride, int nmaps, hipStream_t s, int format = FC_MAP_F32, const MapPlane& plane = {});
// One crop or pad launch as its unit's entry takes it -- the kernels of the three combinations live in three units (kernels.hip,
// kernels_ncc.hip, kernels_score.hip), so that each unit compiles the device code it always did: launch_crop_maps / launch_pad_maps
// check the arguments and pick the entry, the entry launches its kernel for the element class (pad: off_h, off_w unused)
struct MapsLaunch {
    const float* src;
    int src_h, src_w;
    size_t src_map_stride;
    float* dst;
    int dst_h, dst_w;
    size_t dst_map_stride;
    int off_h, off_w, nmaps, format;
    hipStream_t s;
    int stride_h = 1, stride_w = 1;      // crops only
    // k16 / k32(grid, block, dst as the kernel takes it, bf16): the fp32 and the 16-bit launch of a crop or pad kernel, written once
    template <class K16, class K32>
    hipError_t run(K16&& k16, K32&& k32) const {
        const dim3 grid((unsigned)dst_w, (unsigned)nmaps), block(256);
        if (format != FC_MAP_F32) k16(grid, block, reinterpret_cast<uint16_t*>(dst), format == FC_MAP_BF16 ? 1 : 0);
        else k32(grid, block, dst, 0);
        return hipGetLastError();
    }
};
hipError_t crop_maps_scaled(const MapsLaunch& l, const MapPlane& plane);      // kernels_ncc.hip
hipError_t pad_maps_scaled(const MapsLaunch& l, const MapPlane& plane);
hipError_t crop_maps_added(const MapsLaunch& l, const MapPlane& plane);       // kernels_score.hip
hipError_t pad_maps_added(const MapsLaunch& l, const MapPlane& plane);
// ---- normalised cross-correlation maps (kernels_ncc.hip; ncc.hpp)
// window statistics of ONE image ([f][W][H] at img): the fp32 plane D [fft_w][fft_h] at d, in strips of window columns --
// scratch holds 2 * F * strip_cols * fft_h doubles (ncc_strip_columns)
hipError_t launch_ncc_statistics(const float* img, int H, int W, int F, int fft_h, int fft_w, int box_h, int box_w, double* scratch,
                                 int strip_cols, float* d, hipStream_t s);
// ... of an image of typed pixels (pixel_format: FC_PIXEL_* of pixel_format.hpp; F32: the call above)
hipError_t launch_ncc_statistics_typed(const void* img, int pixel_format, int H, int W, int F, int fft_h, int fft_w, int box_h, int box_w,
                                       double* scratch, int strip_cols, float* d, hipStream_t s);
// (its pass 1 over one strip of typed pixels, kernels_pixels.hip; the error is collected by the caller's hipGetLastError)
void launch_ncc_column_sums_px(const void* img, const PixelLoad& px, int H, int W, int F, int fft_h, int box_h, int w_start, int ncols, double* c1,
                               double* c2, hipStream_t s);
// dst = the n kernels at src ([n][F][plane_elems]) centred per plane and scaled to unit joint norm; stats: 2 * n * F doubles of scratch
hipError_t launch_ncc_unit_kernels(const float* src, float* dst, int n, int F, int plane_elems, double* stats, hipStream_t s);
// ---- the other matching scores (fftconv_plan_set_match_score; ncc.hpp): FC_SCORE_*
// launch_ncc_statistics_typed for a score with a plane: 1 the call above, 3 Dc = E^(-1/2), 4 Q = E at d
hipError_t launch_score_statistics_typed(int score, const void* img, int pixel_format, int H, int W, int F, int fft_h, int fft_w, int box_h, int box_w,
                                         double* scratch, int strip_cols, float* d, hipStream_t s);
// (pass 2 of scores 3 and 4 over one strip, kernels_score.hip, and the plane statistics of kernels_ncc.hip for score 2's means; errors
//  are collected by the caller's hipGetLastError)
void launch_score_plane(int score, const double* c2, int ncols, int nout, int fft_h, int F, int box_w, float* d, hipStream_t s);
void launch_ncc_plane_stats(const float* src, int planes, int plane_elems, double* stats, hipStream_t s);
// launch_ncc_unit_kernels for any score: 2 centred, 3 T / sqrt(t2), 4 -2 T; consts[k] = (float) t2 of kernel k (scores 2-4; n floats)
hipError_t launch_score_kernels(int score, const float* src, float* dst, int n, int F, int plane_elems, double* stats, float* consts, hipStream_t s);
hipError_t launch_cols_r2c(const ColsR2CArgs& a, int tiles, int planes, int threads, size_t lds_bytes, hipStream_t s);
hipError_t launch_rows_fwd(const RowsFwdArgs& a, int rows, int threads, size_t lds_bytes, hipStream_t s);
// specialised forward image rows (fast_rows_fwd.hpp); hipErrorInvalidValue if L has no configuration
hipError_t launch_fast_rows_fwd(int L, const FastRowsFwdArgs& a, int rows, hipStream_t s);
hipError_t launch_spectral_rows(const SpectralRowsArgs& a, int rows, int kernels, int threads, size_t lds_bytes, hipStream_t s);
// specialised spectral rows (fast_rows_multi.hpp): kernels_per_wg (>= 1) consecutive kernels share one fetch of the image-spectrum
// row; hipErrorInvalidValue if no instantiation matches (L, nz2)
hipError_t launch_fast_rows_multi(int L, int nz2, const FastRowsArgs& a, int rows, int kernels, int kernels_per_wg, hipStream_t s);
// the same walk with a spectral filter in the product phase (kernels_rows_filter_g<G>.hip; a.filter_mode, a.filter_param): F = 1;
// hipErrorInvalidValue besides for a length that is not built (fast_paths.hpp: fast_rows_filter_built)
hipError_t launch_fast_rows_filter(int L, int nz2, const FastRowsArgs& a, int rows, int kernels, int kernels_per_wg, hipStream_t s);
// how many workgroups of that kernel a CU holds at once (hipOccupancyMaxActiveBlocksPerMultiprocessor)
hipError_t fast_rows_multi_wgs_per_cu(int L, int nz2, const FastRowsArgs& a, int* wgs_per_cu);
// image-walk spectral rows (fast_rows_images.hpp; F = 1): the a.images x a.kernels_per_image maps of the launch, a workgroup per
// (row group, kernel) walking images_per_wg (>= 1) consecutive images; hipErrorInvalidValue if L has no such kernel
// (fast_paths.hpp: fast_rows_images_built)
hipError_t launch_fast_rows_images(int L, const FastRowsArgs& a, int rows, int images_per_wg, hipStream_t s);
hipError_t launch_fast_cols(int M, int T, const FastColsArgs& a, int num_cus, hipStream_t s);
// the rectangle family of the output kernel (fast_cols.hpp: RECT, and on it NORM and ADD): `shape` from fast_cols_rect_launch_shape
// (fast_paths.hpp) -- shape.plane picks the fused scale of normalised maps (Scale) or the fused additive store of score 4 (Add), both
// fp32 only; without a plane the rectangle store in shape.a.out_format.  A shape from fast_cols_stride_launch_shape (shape.strided) runs
// the strided store: fp32 maps, no plane.  hipErrorInvalidValue for a launch the family does not have (row-major or sliced), for a
// plane that is not filled in, and for a configuration whose kernel is not built (fast_cols_*_built)
hipError_t launch_fast_cols_rect(int M, int T, const FastColsShape& shape, hipStream_t s);
// the same family with the per-map extrema found in the store (kernels_cols_*ext_g<G>.hip; fast_cols.hpp: EXT): fp32 maps, no stride;
// shape.extrema.partials takes fast_cols_extrema_slots partials per map of the launch.  hipErrorInvalidValue as above, and for a
// configuration whose EXT kernel is not built (fast_cols_*_ext_built)
hipError_t launch_fast_cols_rect_extrema(int M, int T, const FastColsShape& shape, hipStream_t s);
// ---- per-map extrema (kernels_extrema.hip; extrema.hpp)
// the scan: nmaps dense maps of map_elems elements of `format` (FC_MAP_*) from maps on, map_stride elements apart, where they lie on
// the device; extrema_scan_blocks(map bytes) partials per map, from partials on
hipError_t launch_extrema_scan(const void* maps, size_t map_elems, size_t map_stride, int format, int nmaps, ExtremaPartial* partials, hipStream_t s);
// the fold: records[m] = the record of the per_map partials of map m (maps of out_h rows per column), m < nmaps
hipError_t launch_extrema_fold(const ExtremaPartial* partials, int per_map, int nmaps, int out_h, ExtremaRecord* records, hipStream_t s);
// ---- peak lists (kernels_peaks.hip; peaks.hpp)
// nmaps dense maps as launch_extrema_scan takes them, of out_h rows per column: found[m] = the peaks of map m under `rule`, all of them;
// peaks[m * max_peaks ...] the first min(found[m], max_peaks) in ascending index order.  scratch: 2 * peaks_units(map bytes) ints per map
hipError_t launch_peaks(const void* maps, size_t map_elems, size_t map_stride, int format, int out_h, int nmaps, const PeakRule& rule, int max_peaks, int* scratch,
                        int* found, PeakRecord* peaks, hipStream_t s);
hipError_t launch_fast_cols_fwd(int M, int T, bool pruned, const FastColsFwdArgs& a, int num_cus, hipStream_t s);
// image columns of typed pixels (kernels_cols_fwd_px_g<G>.hip; pixel_format.hpp): a.in holds elements of px.format, px from
// fast_cols_fwd_pixel_load; hipErrorInvalidValue for fp32 pixels and for a configuration that is not built (fast_cols_fwd_px_built)
hipError_t launch_fast_cols_fwd_px(int M, int T, const FastColsFwdArgs& a, const PixelLoad& px, int num_cus, hipStream_t s);
// the staged route of typed pixels (kernels_pixels.hip): dst[i] = the exact fp32 value of element i of src, n elements
hipError_t launch_pixels_to_f32(const void* src, int pixel_format, float* dst, size_t n, hipStream_t s);
// image columns with a border (kernels_cols_fwd_border_g<G>.hip; border.hpp): a.in is the data, a.h_in / a.ncols count the extended
// image, bd from border_load; hipErrorInvalidValue for mode 0 and for a configuration that is not built (fast_cols_fwd_border_built)
hipError_t launch_fast_cols_fwd_border(int M, int T, const FastColsFwdArgs& a, const BorderLoad& bd, int num_cus, hipStream_t s);
// the staged route of a border (kernels_pixels.hip): dst = the extended image E of `planes` planes of H x W fp32 pixels at src,
// (H + MAXK_H - 1) x (W + MAXK_W - 1) per plane, dense
hipError_t launch_extend_image(const float* src, float* dst, int H, int W, int ext_h, int ext_w, size_t planes, const BorderLoad& bd, hipStream_t s);
// image columns (full variant) and kernel columns (pruned or full) of one plan in ONE launch (kernels_cols_fwd.hip)
hipError_t launch_fast_cols_fwd_pair(int M, int T, const FastColsFwdArgs& image, const FastColsFwdArgs& kernels, bool kernels_pruned,
                                     int num_cus, hipStream_t s);
hipError_t launch_cols_c2r(const ColsC2RArgs& a, int tiles, int kernels, int threads, size_t lds_bytes, hipStream_t s);


// The specialised launchers' per-group entry points: the translation unit kernels_*_g<G>.hip defines the specialisation for its
// group G of configurations (fast_paths.hpp); empty: no configuration of that group matches.  kernels.hip tries the groups in order.
using GroupResult = std::optional<hipError_t>;
template <int G> GroupResult launch_fast_rows_fwd_group(int L, const FastRowsFwdArgs& a, int rows, hipStream_t s);
template <int G> GroupResult launch_fast_rows_multi_group(int L, int nz2, const FastRowsArgs& a, int rows, int kernels, int kernels_per_wg, hipStream_t s);
// (with a spectral filter: kernels_rows_filter_g<G>.hip)
template <int G> GroupResult launch_fast_rows_filter_group(int L, int nz2, const FastRowsArgs& a, int rows, int kernels, int kernels_per_wg, hipStream_t s);
template <int G> GroupResult fast_rows_multi_wgs_per_cu_group(int L, int nz2, const FastRowsArgs& a, int* wgs_per_cu);
// (the image walk: kernels_rows_images_g<G>.hip)
template <int G> GroupResult launch_fast_rows_images_group(int L, const FastRowsArgs& a, int rows, int images_per_wg, hipStream_t s);
template <int G> GroupResult launch_fast_cols_group(int M, int T, const FastColsArgs& a, int num_cus, hipStream_t s);
// (the 16-bit-map instantiations of the same configurations: kernels_cols16_g<G>.hip)
template <int G> GroupResult launch_fast_cols16_group(int M, int T, const FastColsArgs& a, int num_cus, hipStream_t s);
// (the rectangle family, all from kernels_cols_rect.inc: the store in fp32 and 16-bit maps -- kernels_cols_rect_g<G>.hip,
//  kernels_cols_rect16_g<G>.hip -- the fused scale of normalised maps -- kernels_cols_norm_g<G>.hip -- and the fused additive store of
//  score 4 -- kernels_cols_sqdiff_g<G>.hip; launch_fast_cols_rect picks among them)
template <int G> GroupResult launch_fast_cols_rect_group(int M, int T, const FastColsShape& shape, hipStream_t s);
template <int G> GroupResult launch_fast_cols_rect16_group(int M, int T, const FastColsShape& shape, hipStream_t s);
template <int G> GroupResult launch_fast_cols_rect_scale_group(int M, int T, const FastColsShape& shape, hipStream_t s);
template <int G> GroupResult launch_fast_cols_rect_add_group(int M, int T, const FastColsShape& shape, hipStream_t s);
// (the fp32 stores with the per-map extrema found in the store: kernels_cols_ext_g<G>.hip, kernels_cols_norm_ext_g<G>.hip,
//  kernels_cols_sqdiff_ext_g<G>.hip; launch_fast_cols_rect_extrema picks among them)
template <int G> GroupResult launch_fast_cols_rect_ext_group(int M, int T, const FastColsShape& shape, hipStream_t s);
template <int G> GroupResult launch_fast_cols_rect_scale_ext_group(int M, int T, const FastColsShape& shape, hipStream_t s);
template <int G> GroupResult launch_fast_cols_rect_add_ext_group(int M, int T, const FastColsShape& shape, hipStream_t s);
// (the strided store: kernels_cols_stride_g<G>.hip)
template <int G> GroupResult launch_fast_cols_rect_stride_group(int M, int T, const FastColsShape& shape, hipStream_t s);
template <int G> GroupResult launch_fast_cols_fwd_group(int M, int T, bool pruned, const FastColsFwdArgs& a, int num_cus, hipStream_t s);
// (typed image pixels: kernels_cols_fwd_px_g<G>.hip)
template <int G> GroupResult launch_fast_cols_fwd_px_group(int M, int T, const FastColsFwdArgs& a, const PixelLoad& px, int num_cus, hipStream_t s);
// (an image with a border: kernels_cols_fwd_border_g<G>.hip)
template <int G> GroupResult launch_fast_cols_fwd_border_group(int M, int T, const FastColsFwdArgs& a, const BorderLoad& bd, int num_cus, hipStream_t s);
template <int G> GroupResult launch_fast_cols_fwd_pair_group(int M, int T, const FastColsFwdArgs& image, const FastColsFwdArgs& kernels,
                                                             bool kernels_pruned, int num_cus, hipStream_t s);

}  // namespace fc
