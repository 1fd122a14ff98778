// peaks.hpp -- peak lists (fftconv_plan_set_peaks): the thresholded local maxima of every delivered map, in memory order.  The bodies
// every place shares, written once: the candidate test, the neighbourhood walk with its early exit, the sub-pixel fit, the record,
// the cut of a map into units and the rank of a flagged element within a unit's step.  Host/device and HIP-free: the kernels
// (kernels_peaks.hip) and tests/peaks_host both compile this text.
//
// The rules (include/fftconv.h states them for the caller):
//   * an element is (value, index), index = col * out_h + row of the DELIVERED map (memory order), as in extrema.hpp;
//   * mode 1: an element at or above the threshold that no other element of its neighbourhood -- rows r +- radius_h, columns
//     c +- radius_w, clipped to the map -- beats (extrema_beats_max: a larger value, or an equal one at a smaller index);
//   * the compares are ordered, so a NaN is never a peak and never beats anything; +0 and -0 compare equal;
//   * mode 2 is mode 1 on the negated values with the negated threshold (negation is exact, so the walk below sees `sign * value`);
//     the record carries the element's own value;
//   * no atomics anywhere: a unit's count and its records depend on the map alone, and the units are laid end to end in index order.
#pragma once
#include <cstddef>
#include <cstdint>

#include "extrema.hpp"

namespace fc {

enum { FC_PEAKS_OFF = 0, FC_PEAKS_MAX = 1, FC_PEAKS_MIN = 2 };

// the caller's record (the layout of fftconv_peak, include/fftconv.h): `row` the fast index
struct PeakRecord {
    float value;
    int row, col;
    float d_row, d_col;
};

// what a launch holds uniform: the threshold and the sign the walk applies to every value (mode 2: -threshold, -1), the radii
struct PeakRule {
    float threshold;      // of the signed values
    float sign;           // +1 (maxima) or -1 (minima)
    int radius_h, radius_w;
};
FC_HD PeakRule peak_rule(int mode, float threshold, int radius_h, int radius_w) {
    const bool min = mode == FC_PEAKS_MIN;
    return {min ? -threshold : threshold, min ? -1.0f : 1.0f, radius_h, radius_w};
}
FC_HD float peak_signed(const PeakRule& k, float v) { return k.sign < 0 ? -v : v; }

// the candidate test, on the signed value (ordered: false for a NaN)
FC_HD bool peak_candidate(const PeakRule& k, float u) { return u >= k.threshold; }

// The neighbourhood walk.  U(index) is the signed value of an element of a map of out_h rows per column and out_w columns; (u, i)
// is the candidate at row r, column c.  True if no other element of the clipped neighbourhood beats it; the walk ends at the first
// one that does.
template <class Map>
FC_HD bool peak_unbeaten(const Map& U, int out_h, int out_w, int r, int c, float u, const PeakRule& k) {
    // (a radius beyond the map is clipped first: r + radius cannot overflow then)
    const int rh = k.radius_h < out_h ? k.radius_h : out_h - 1, rw = k.radius_w < out_w ? k.radius_w : out_w - 1;
    const int r0 = r - rh > 0 ? r - rh : 0, r1 = r + rh < out_h - 1 ? r + rh : out_h - 1;
    const int c0 = c - rw > 0 ? c - rw : 0, c1 = c + rw < out_w - 1 ? c + rw : out_w - 1;
    const int i = c * out_h + r;
    for (int cc = c0; cc <= c1; cc++)
        for (int rr = r0; rr <= r1; rr++) {
            const int j = cc * out_h + rr;
            if (j != i && extrema_beats_max(U(j), j, u, i)) return false;
        }
    return true;
}
// candidate and walk together: is element i of the map a peak?
template <class Map>
FC_HD bool peak_test(const Map& U, int out_h, int out_w, int i, float u, const PeakRule& k) {
    if (!peak_candidate(k, u)) return false;
    const int c = i / out_h;
    return peak_unbeaten(U, out_h, out_w, i - c * out_h, c, u, k);
}

// The sub-pixel fit of one dimension: the vertex of the parabola through (-1, a), (0, v), (+1, b), in float64 from the exact element
// values with + - * / alone, clamped to [-0.5, 0.5] and rounded to fp32 once.  0 where a value is not finite or the three are collinear.
FC_HD bool peak_finite(float x) { return x - x == 0.0f; }
FC_HD float peak_fit(float a, float v, float b) {
    if (!peak_finite(a) || !peak_finite(v) || !peak_finite(b)) return 0.0f;
    const double A = a, V = v, B = b;
    const double den = (A - V) + (B - V);
    if (den == 0.0) return 0.0f;
    double d = 0.5 * (A - B) / den;
    d = d > 0.5 ? 0.5 : d < -0.5 ? -0.5 : d;
    return (float)d;
}

// The record of the peak at index i.  V(index) is the element's OWN value (not signed: the fit is the same for both signs, and the
// record carries the element).  An offset is 0 at a map edge and where that dimension's radius is 0.
template <class Map>
FC_HD PeakRecord peak_record(const Map& V, int out_h, int out_w, int i, const PeakRule& k) {
    PeakRecord p;
    p.value = V(i);
    p.col = i / out_h;
    p.row = i - p.col * out_h;
    p.d_row = k.radius_h > 0 && p.row > 0 && p.row < out_h - 1 ? peak_fit(V(i - 1), p.value, V(i + 1)) : 0.0f;
    p.d_col = k.radius_w > 0 && p.col > 0 && p.col < out_w - 1 ? peak_fit(V(i - out_h), p.value, V(i + out_h)) : 0.0f;
    return p;
}

// ---- the cut of a map into units ----
// A unit is a contiguous run of the 16-byte vectors that touch the map, cut at 16-byte ADDRESSES as the extrema scan cuts its blocks
// (a map with an odd number of elements starts unaligned); a wave owns one unit and walks it in address order, 64 vectors a step.
constexpr int FC_PEAKS_LANES = 64;
constexpr int FC_PEAKS_MAX_UNITS = 1024;                             // per map
constexpr size_t FC_PEAKS_UNIT_BYTES = (size_t)16 << 10;             // at least this much per unit: 16 steps
FC_HD int peaks_units(size_t map_bytes) {
    const size_t n = (map_bytes + FC_PEAKS_UNIT_BYTES - 1) / FC_PEAKS_UNIT_BYTES;
    return n < 1 ? 1 : n > (size_t)FC_PEAKS_MAX_UNITS ? FC_PEAKS_MAX_UNITS : (int)n;
}
struct PeakCut {
    uintptr_t v0;           // the first vector that touches the map (address / 16)
    size_t nv, per_unit;    // the vectors that touch it; a unit's share
};
FC_HD PeakCut peaks_cut(uintptr_t map_address, size_t map_bytes, int units) {
    const uintptr_t v0 = map_address / 16, v1 = (map_address + map_bytes + 15) / 16;
    const size_t nv = v1 - v0;
    return {v0, nv, (nv + (size_t)units - 1) / (size_t)units};
}
// the vectors [lo, hi) of unit u, relative to cut.v0 (empty for a unit beyond the map's last vector)
FC_HD void peaks_unit_range(const PeakCut& cut, int u, size_t& lo, size_t& hi) {
    lo = (size_t)u * cut.per_unit;
    hi = lo + cut.per_unit;
    if (lo > cut.nv) lo = cut.nv;
    if (hi > cut.nv) hi = cut.nv;
}
// the index of the element in slot 0 of vector v (relative to cut.v0) of a map at map_address: negative in the vector ahead of an
// unaligned map
FC_HD long peaks_vector_element(const PeakCut& cut, size_t v, uintptr_t map_address, size_t elem_bytes) {
    return ((long)((cut.v0 + v) * 16) - (long)map_address) / (long)elem_bytes;
}

// ---- the rank within a step ----
// A step of a wave flags up to nslots elements per lane (nslots: the elements of a vector); flags[s] holds the lanes whose slot s is
// a peak.  Ascending index is lane-major, then slot.  The rank of (lane, slot) among the step's flags, and the step's total:
FC_HD int peaks_popcount(uint64_t x) { return __builtin_popcountll(x); }
FC_HD int peaks_rank(const uint64_t* flags, int nslots, int lane, int slot) {
    const uint64_t lower = lane == 0 ? 0 : ~(uint64_t)0 >> (64 - lane);
    int r = 0;
    for (int s = 0; s < nslots; s++) r += peaks_popcount(flags[s] & lower);
    for (int s = 0; s < slot; s++) r += (int)(flags[s] >> lane & 1);
    return r;
}
FC_HD int peaks_step_total(const uint64_t* flags, int nslots) {
    int n = 0;
    for (int s = 0; s < nslots; s++) n += peaks_popcount(flags[s]);
    return n;
}

}  // namespace fc
