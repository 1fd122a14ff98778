// extrema.hpp -- per-map extrema (fftconv_plan_set_extrema): the largest and the smallest element of every delivered map and where
// they lie.  The bodies every place shares, written once: the per-element compare-and-take, the tie rule, the "empty" sentinel,
// the fold step and the record a partial becomes.  Host/device and HIP-free: the output kernel's fused store (fast_cols.hpp: EXT),
// the scan and fold kernels (kernels_extrema.hip) and tests/extrema_host all compile this text.
//
// The rules (include/fftconv.h states them for the caller):
//   * an element is (value, index), index = col * out_h + row of the DELIVERED map (memory order);
//   * the compares are ordered, so a NaN never wins; +0 and -0 compare equal;
//   * among equal values the smallest index wins, for max and min independently, and the value kept is that element's bits;
//   * no atomics anywhere: a partial depends on the elements it covers alone, and merging is associative and commutative, so the
//     result does not depend on which workgroup or wave covered which element, nor on the order of the fold.
#pragma once
#include <cstdint>

#include "fc_common.hpp"

namespace fc {

// "no element yet": an index no element has (a map has fewer than 2^31 elements), beside the value every element beats or ties --
// an element equal to the sentinel's value still wins on its smaller index, so -inf / +inf elements are reported as elements
constexpr int FC_EXTREMA_NONE = 0x7fffffff;

struct alignas(16) ExtremaPartial {
    float max_value;
    int max_index;
    float min_value;
    int min_index;
};

FC_HD float extrema_inf() { return __builtin_huge_valf(); }
FC_HD ExtremaPartial extrema_empty() { return {-extrema_inf(), FC_EXTREMA_NONE, extrema_inf(), FC_EXTREMA_NONE}; }

// the tie rule: does (v, i) replace (best, bi) as the maximum / the minimum?
FC_HD bool extrema_beats_max(float v, int i, float best, int bi) { return v > best || (v == best && i < bi); }
FC_HD bool extrema_beats_min(float v, int i, float best, int bi) { return v < best || (v == best && i < bi); }

// one element
FC_HD void extrema_take(ExtremaPartial& p, float v, int i) {
    if (extrema_beats_max(v, i, p.max_value, p.max_index)) { p.max_value = v; p.max_index = i; }
    if (extrema_beats_min(v, i, p.min_value, p.min_index)) { p.min_value = v; p.min_index = i; }
}

// the fold step: two partials over disjoint elements of one map
FC_HD ExtremaPartial extrema_merge(ExtremaPartial a, const ExtremaPartial& b) {
    if (extrema_beats_max(b.max_value, b.max_index, a.max_value, a.max_index)) { a.max_value = b.max_value; a.max_index = b.max_index; }
    if (extrema_beats_min(b.min_value, b.min_index, a.min_value, a.min_index)) { a.min_value = b.min_value; a.min_index = b.min_index; }
    return a;
}

// The caller's record (the layout of fftconv_extrema, include/fftconv.h): `row` the fast index and `col` the slow one of the
// delivered map of out_h rows per column.  A side no element took -- an empty map, or one whose elements are all NaN -- reports NaN
// and row = col = -1.
struct ExtremaRecord {
    float max_value;
    int max_row, max_col;
    float min_value;
    int min_row, min_col;
};
FC_HD ExtremaRecord extrema_record(const ExtremaPartial& p, int out_h) {
    const float nan = __builtin_nanf("");
    ExtremaRecord r;
    const bool has_max = p.max_index != FC_EXTREMA_NONE, has_min = p.min_index != FC_EXTREMA_NONE;
    r.max_value = has_max ? p.max_value : nan;
    r.max_col = has_max ? p.max_index / out_h : -1;
    r.max_row = has_max ? p.max_index - r.max_col * out_h : -1;
    r.min_value = has_min ? p.min_value : nan;
    r.min_col = has_min ? p.min_index / out_h : -1;
    r.min_row = has_min ? p.min_index - r.min_col * out_h : -1;
    return r;
}

// the exact fp32 value of a 16-bit map element (FC_MAP_F16 / FC_MAP_BF16: what the scan reads back)
FC_HD float extrema_map16_value(uint16_t bits, bool bf16) {
    uint32_t w;
    if (bf16) w = (uint32_t)bits << 16;
    else {
        const uint32_t sign = (uint32_t)(bits & 0x8000u) << 16, exp = (bits >> 10) & 0x1fu, man = bits & 0x3ffu;
        if (exp == 0x1fu) w = sign | 0x7f800000u | (man << 13);                      // inf, NaN
        else if (exp != 0) w = sign | ((exp + 112u) << 23) | (man << 13);            // normal
        else if (man == 0) w = sign;                                                 // +-0
        else {                                                                       // subnormal: man * 2^-24
            int e = 113;
            uint32_t m = man;
            while (!(m & 0x400u)) { m <<= 1; e--; }
            w = sign | ((uint32_t)e << 23) | ((m & 0x3ffu) << 13);
        }
    }
    union { uint32_t u; float f; } cv;
    cv.u = w;
    return cv.f;
}

// Index arithmetic of the fused store (fast_cols.hpp, RECT stores): the element of the dense rectangle map -- rows [h_lo, fft_h) of
// columns [rect_w_lo, ...) of the window, out_pitch = fft_h - h_lo rows per column -- that window row h of window column w is
FC_HD int extrema_rect_index(int w, int h, int rect_w_lo, int h_lo, int out_pitch) { return (w - rect_w_lo) * out_pitch + (h - h_lo); }

// Partials of a launch: [map in launch][slot], `per_map` slots each (fused: tiles of a map x waves of a workgroup; scan: blocks per map)
// The scan's cut of a map: blocks per map for `bytes` of map, each block a whole number of 16-byte vectors
constexpr int FC_EXTREMA_SCAN_THREADS = 256;
constexpr int FC_EXTREMA_SCAN_MAX_BLOCKS = 256;      // per map
constexpr size_t FC_EXTREMA_SCAN_BLOCK_BYTES = (size_t)64 << 10;      // at least this much per block: 16 vectors per thread
FC_HD int extrema_scan_blocks(size_t map_bytes) {
    const size_t n = (map_bytes + FC_EXTREMA_SCAN_BLOCK_BYTES - 1) / FC_EXTREMA_SCAN_BLOCK_BYTES;
    return n < 1 ? 1 : n > (size_t)FC_EXTREMA_SCAN_MAX_BLOCKS ? FC_EXTREMA_SCAN_MAX_BLOCKS : (int)n;
}

}  // namespace fc
