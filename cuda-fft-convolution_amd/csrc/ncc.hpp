// ncc.hpp -- zero-mean normalised cross-correlation maps (fftconv_plan_set_normalisation): the per-element bodies of the
// window statistics and of the kernel normalisation, and the host decisions around them.  Written once, compiled twice like
// every header here: by hipcc into kernels_ncc.hip and by the host compiler into tests/ncc_host.
//
// With one box kh x kw (n = kh * kw) for the window sums and for every kernel,
//     sum (I - mean_u(I)) (T - mean(T))  =  sum I (T - mean(T)),
// so with kernels centred per plane and scaled to unit joint norm (T'') ahead of their transform the whole normalisation of
// a map is one multiply per element by the plane
//     D(u) = 0 where den2(u) <= 2^-30 e(u), else den2(u)^(-1/2),   den2 = sum_f (s2_f - s1_f^2 / n),  e = sum_f s2_f,
// s1_f / s2_f the sums of the zero-padded image / of its square over the box that ends at window position u.  D depends on
// (image, box) only.  All sums here are float64, DIRECT sums in a fixed order -- no prefix differences, no shift by a global
// mean: a window that lies wholly in the padding then sums to exactly 0, and the floor (a window flat to within 2^-15 of its
// RMS) is met by rounding errors of 2^-52.
#pragma once
#include <cmath>

#include "fc_common.hpp"
#include "pixel_format.hpp"

namespace fc {

constexpr double FC_NCC_FLOOR = 1.0 / 1073741824.0;      // 2^-30

// pass 1, one element: sum and sum of squares of rows i - a, a < box_h, of one image column (`col`: its H floats; rows
// outside [0, H) are the padding)
// Px: the pixel type of the image (pixel_format.hpp; float: the text as it was) -- a typed element goes to float64 through its
// exact fp32 value, so the sums, and D, are those of the fp32 image to the bit
template <class Px = float>
FC_HD void ncc_column_sums(const pixel_elem_t<Px>* col, int H, int i, int box_h, double& s1, double& s2, [[maybe_unused]] const PixelLoad px = {}) {
    s1 = 0.0;
    s2 = 0.0;
    for (int a = 0; a < box_h; a++) {
        const int r = i - a;
        if (r >= 0 && r < H) {
            const double v = (double)pixel_value(col[r], px);
            s1 += v;
            s2 += v * v;      // (exact in float64: a product of two 24-bit significands)
        }
    }
}

// pass 2, one element: D at row i of the window column whose pass-1 column lies at `col_hi` of the strip.  c1 / c2: the
// pass-1 sums, [f][column of the strip][pitch] with `plane` doubles per feature plane; the box covers the strip columns
// col_hi - b, b < box_w (the strip starts box_w - 1 columns ahead of its first window column: all of them exist)
FC_HD float ncc_scale(const double* c1, const double* c2, size_t plane, int pitch, int F, int col_hi, int i, int box_w, int n) {
    double den2 = 0.0, e = 0.0;
    for (int f = 0; f < F; f++) {
        double s1 = 0.0, s2 = 0.0;
        for (int b = 0; b < box_w; b++) {
            const size_t at = (size_t)f * plane + (size_t)(col_hi - b) * pitch + i;
            s1 += c1[at];
            s2 += c2[at];
        }
        den2 += s2 - s1 * s1 / (double)n;
        e += s2;
    }
    if (den2 <= FC_NCC_FLOOR * e) return 0.f;
    return (float)(1.0 / sqrt(den2));
}

// Matching scores beside mode 1 (fftconv_plan_set_match_score; the table of include/fftconv.h).  The planes of scores 3 and 4
// come from the pass-1 sums of squares alone: E(u) = sum_f s2_f(u), summed in the order ncc_scale sums its e.
//   score 3 (CCORR_NORMED): Dc = (float) E^(-1/2), 0 where E == 0.  No relative floor is needed: E is a sum of non-negative float64
//   terms (exact squares of fp32 values), so it is exactly 0 if and only if every pixel under the box is 0 -- no cancellation can
//   produce a small non-zero E -- and otherwise it is accurate to a relative 2^-52.
//   score 4 (SQDIFF): Q = (float) E.
inline const char* score_name(long score) {
    static const char* const names[] = {"none", "CCOEFF_NORMED", "CCOEFF", "CCORR_NORMED", "SQDIFF"};
    return score >= 0 && score <= 4 ? names[score] : "?";
}
FC_HD double ncc_energy(const double* c2, size_t plane, int pitch, int F, int col_hi, int i, int box_w) {
    double e = 0.0;
    for (int f = 0; f < F; f++) {
        double s2 = 0.0;
        for (int b = 0; b < box_w; b++) s2 += c2[(size_t)f * plane + (size_t)(col_hi - b) * pitch + i];
        e += s2;
    }
    return e;
}
// pass 2 of scores 3 and 4, one element (the arguments of ncc_scale; c2 only)
FC_HD float score_plane(int score, const double* c2, size_t plane, int pitch, int F, int col_hi, int i, int box_w) {
    const double e = ncc_energy(c2, plane, pitch, F, col_hi, i, box_w);
    if (score == FC_SCORE_SQDIFF) return (float)e;
    return e == 0.0 ? 0.f : (float)(1.0 / sqrt(e));
}

// kernel normalisation: the sums of one plane of `pe` floats are taken by FC_NCC_LANES lanes -- lane t adds the elements t,
// t + FC_NCC_LANES, ... in ascending order -- whose partial sums are then folded by halves (lane t += lane t + s for s =
// FC_NCC_LANES / 2 ... 1): one fixed order, whoever runs the lanes (a workgroup per plane on the device, a loop on the host)
constexpr int FC_NCC_LANES = 256;
// lane t's share of sum (x - centre) (sq false) or sum (x - centre)^2 (sq true)
FC_HD double ncc_lane_sum(const float* plane, int pe, int t, double centre, bool sq) {
    double s = 0.0;
    for (int i = t; i < pe; i += FC_NCC_LANES) {
        const double d = (double)plane[i] - centre;
        s += sq ? d * d : d;
    }
    return s;
}
// (host form of the fold; the device folds in LDS with a barrier per step)
FC_HD double ncc_fold(double* part) {
    for (int s = FC_NCC_LANES / 2; s > 0; s >>= 1)
        for (int t = 0; t < s; t++) part[t] += part[t + s];
    return part[0];
}
// mean of one plane and the sum of squares around it (host: tests/ncc_host)
inline void ncc_plane_stats(const float* plane, int pe, double& mean, double& ssq) {
    double part[FC_NCC_LANES];
    for (int t = 0; t < FC_NCC_LANES; t++) part[t] = ncc_lane_sum(plane, pe, t, 0.0, false);
    mean = ncc_fold(part) / (double)pe;
    for (int t = 0; t < FC_NCC_LANES; t++) part[t] = ncc_lane_sum(plane, pe, t, mean, true);
    ssq = ncc_fold(part);
}
// ... the joint norm of a kernel's F planes (stats: [f][2] = mean, ssq), 0 for a constant kernel
FC_HD double ncc_kernel_norm(const double* stats, int F) {
    double ss = 0.0;
    for (int f = 0; f < F; f++) ss += stats[2 * f + 1];
    return sqrt(ss);
}
// ... and one element of T'': all zeros where the norm is 0
FC_HD float ncc_unit(float x, double mean, double norm) { return norm > 0.0 ? (float)(((double)x - mean) / norm) : 0.f; }

// ... and of the other scores' kernels.  `t2`: the joint sum of squares sum_f sum T_f^2 of a kernel's F planes, each plane's taken
// with centre 0 by the lanes and the fold above, the planes added in ascending order.
//   score 2: centred per plane, not scaled;  score 3: T / sqrt(t2), all zeros where t2 = 0;  score 4: -2 T (exact in fp32)
FC_HD float score_kernel_elem(int score, float x, double mean, double norm, double t2) {
    if (score == FC_SCORE_CCOEFF_NORMED) return ncc_unit(x, mean, norm);
    if (score == FC_SCORE_CCOEFF) return (float)((double)x - mean);
    if (score == FC_SCORE_CCORR_NORMED) return t2 > 0.0 ? (float)((double)x / sqrt(t2)) : 0.f;
    return -2.f * x;
}
// sum of squares (centre 0) of one plane, host form (tests/match_score_host)
inline double score_plane_t2(const float* plane, int pe) {
    double part[FC_NCC_LANES];
    for (int t = 0; t < FC_NCC_LANES; t++) part[t] = ncc_lane_sum(plane, pe, t, 0.0, true);
    return ncc_fold(part);
}
// score 4, one element of a map: first s = q + c, one fp32 add, then x + s, one fp32 add -- on every route.  Written with
// intrinsic-free plain adds: an addition cannot be contracted with another addition, so fused and staged stores agree to the bit.
FC_HD float score_sqdiff(float x, float q, float c) {
    const float s = q + c;
    return x + s;
}

// image of map `slot` of a launch that covers the images from image0 on with per_image kernels each (slots are image-major)
FC_HD int ncc_image_of(int image0, int slot, int per_image) { return image0 + slot / per_image; }

// fftconv_plan_set_normalisation: why (mode, box) is refused, or nullptr
inline const char* ncc_args_error(long mode, long box_h, long box_w, int max_kh, int max_kw) {
    if (mode != 0 && mode != 1) return "normalisation mode is 0 (off) or 1 (zero-mean normalised cross-correlation)";
    if (mode == 1 && (box_h < 1 || box_w < 1 || box_h > max_kh || box_w > max_kw)) return "normalisation box: 1 <= box <= MAX_KERNEL per dimension";
    return nullptr;
}

// fftconv_plan_set_match_score: why (score, box) is refused, or nullptr
inline const char* score_args_error(long score, long box_h, long box_w, int max_kh, int max_kw) {
    if (score < FC_SCORE_NONE || score > FC_SCORE_SQDIFF)
        return "matching score is 0 (none), 1 (CCOEFF_NORMED), 2 (CCOEFF), 3 (CCORR_NORMED) or 4 (SQDIFF)";
    if (score != 0 && (box_h < 1 || box_w < 1 || box_h > max_kh || box_w > max_kw)) return "matching score box: 1 <= box <= MAX_KERNEL per dimension";
    return nullptr;
}

// The window statistics work in strips of window columns so that their float64 scratch stays bounded: columns of pass-1 sums
// a strip holds (its window columns + box_w - 1 ahead of them), at most `budget` bytes for the 2 * F planes of fft_h rows --
// but never fewer than the box_w a strip of ONE window column needs, and never more than the whole window needs.  The scratch
// is therefore max(budget, 16 * F * fft_h * box_w bytes) at the most: the budget, unless F * fft_h * box_w exceeds 2^21
// (at cfg3's 4224 rows and 127 columns F = 3 is within it, F = 4 takes 34.3 MB, and it grows with F from there)
inline int ncc_strip_columns(int fft_h, int fft_w, int F, int box_w, size_t budget) {
    const size_t per_col = (size_t)2 * F * fft_h * sizeof(double);
    const long fit = (long)(budget / per_col), least = box_w, all = (long)fft_w + box_w - 1;
    const long c = fit < least ? least : fit;
    return (int)(c < all ? c : all);
}
constexpr size_t FC_NCC_SCRATCH_BYTES = (size_t)32 << 20;

}  // namespace fc
