// kernels_peaks.hip -- peak lists (fftconv_plan_set_peaks; peaks.hpp): the thresholded local maxima of the delivered maps, read where
// they lie on the device behind the last kernel that writes them.
//
// The unit of work is a wave: it owns a contiguous run of the 16-byte vectors of one map (peaks.hpp: the cut) and walks it in address
// order, 64 vectors a step.  Three launches per output launch, no atomics, no barriers, no clearing:
//   k_peaks_count    every wave counts the peaks of its unit -- the neighbourhood walk runs for the elements that meet the threshold
//                    alone, its loads come straight from global memory -- and writes one count;
//   k_peaks_offsets  one wave per map: the exclusive scan of the map's counts, and found[m];
//   k_peaks_write    a wave whose count is 0, or whose offset lies beyond max_peaks, exits at once; the others repeat the walk and
//                    store each peak at offset + the peaks of the steps before + its rank within the step (one ballot per element
//                    slot of the vector; lane-major, then slot: ascending index).
// Every slot the later launches read was written by the launch before on the same stream.
#include "kernels_common.hpp"
#include "peaks.hpp"

namespace fc {
namespace {

constexpr int FC_PEAKS_THREADS = 256;      // 4 waves, 4 units

struct PeaksArgs {
    const void* maps;
    size_t map_elems, map_stride;      // elements
    int out_h, out_w;
    int bf16;
    int units;                         // per map
    PeakRule rule;
    int max_peaks;
    int* counts;                       // [map in launch][unit]
    int* offsets;                      // likewise
    int* found;                        // [map in launch], at the launch's first record
    PeakRecord* peaks;                 // [map in launch][max_peaks], likewise
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <class E, bool WRITE>
__device__ __forceinline__ void peaks_walk(const PeaksArgs& a) {
    constexpr int EPV = 16 / sizeof(E);      // elements per vector: the slots of a lane
    const int m = (int)blockIdx.y, lane = (int)threadIdx.x & 63, u = (int)blockIdx.x * (FC_PEAKS_THREADS / 64) + ((int)threadIdx.x >> 6);
    if (u >= a.units) return;      // (wave-uniform, as every branch around a ballot below)
    const size_t unit = (size_t)m * a.units + u;
    int base = 0;
    if constexpr (WRITE) {
        if (a.counts[unit] == 0) return;
        base = a.offsets[unit];
        if (base >= a.max_peaks) return;
    }
    const E* map = static_cast<const E*>(a.maps) + (size_t)m * a.map_stride;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(map), a1 = a0 + a.map_elems * sizeof(E);
    const PeakCut cut = peaks_cut(a0, a.map_elems * sizeof(E), a.units);
    size_t lo, hi;
    peaks_unit_range(cut, u, lo, hi);
    auto value = [&](E e) -> float {
        if constexpr (sizeof(E) == 4) return e;
        else return extrema_map16_value(e, a.bf16 != 0);
    };
    auto V = [&](int j) -> float { return value(map[j]); };                        // the element's own value
    auto U = [&](int j) -> float { return peak_signed(a.rule, value(map[j])); };   // what the rule compares
    PeakRecord* out = a.peaks + (size_t)m * a.max_peaks;
    int count = 0;
    for (size_t b = lo; b < hi; b += FC_PEAKS_LANES) {
        const size_t v = b + lane;
        const bool mine = v < hi;
        const uintptr_t va = (cut.v0 + v) * 16;
        const long e0 = peaks_vector_element(cut, v, a0, sizeof(E));      // (signed: the first vector may start ahead of the map)
        E e[EPV];
        bool valid[EPV];
        if (mine && va >= a0 && va + 16 <= a1) {
            const u32x4 w = *reinterpret_cast<const u32x4*>(va);
            __builtin_memcpy(e, &w, 16);
#pragma unroll
            for (int i = 0; i < EPV; i++) valid[i] = true;
        } else {
#pragma unroll
            for (int i = 0; i < EPV; i++) {
                const long ei = e0 + i;
                valid[i] = mine && ei >= 0 && (size_t)ei < a.map_elems;
                e[i] = valid[i] ? map[ei] : E(0);
            }
        }
        bool flag[EPV];
        uint64_t flags[EPV];
#pragma unroll
        for (int i = 0; i < EPV; i++) {
            flag[i] = valid[i] && peak_test(U, a.out_h, a.out_w, (int)(e0 + i), peak_signed(a.rule, value(e[i])), a.rule);
            flags[i] = __ballot(flag[i]);
        }
        const int total = peaks_step_total(flags, EPV);
        if constexpr (WRITE) {
            if (total) {
#pragma unroll
                for (int i = 0; i < EPV; i++)
                    if (flag[i]) {
                        const int slot = base + count + peaks_rank(flags, EPV, lane, i);
                        if (slot < a.max_peaks) out[slot] = peak_record(V, a.out_h, a.out_w, (int)(e0 + i), a.rule);
                    }
            }
        }
        count += total;
        if constexpr (WRITE)
            if (base + count >= a.max_peaks) break;
    }
    if constexpr (!WRITE)
        if (lane == 0) a.counts[unit] = count;
}

template <class E>
__global__ void __launch_bounds__(FC_PEAKS_THREADS) k_peaks_count(const PeaksArgs a) { peaks_walk<E, false>(a); }
template <class E>
__global__ void __launch_bounds__(FC_PEAKS_THREADS) k_peaks_write(const PeaksArgs a) { peaks_walk<E, true>(a); }

// one wave per map: lane l sums its run of consecutive counts, the wave scans the 64 sums, the lane lays its run's offsets down
__global__ void __launch_bounds__(FC_PEAKS_LANES) k_peaks_offsets(const int* counts, int units, int* offsets, int* found) {
    const int m = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int per = (units + FC_PEAKS_LANES - 1) / FC_PEAKS_LANES;
    const int u0 = lane * per < units ? lane * per : units, u1 = u0 + per < units ? u0 + per : units;
    const int* c = counts + (size_t)m * units;
    int sum = 0;
    for (int u = u0; u < u1; u++) sum += c[u];
    int incl = sum;
#pragma unroll
    for (int d = 1; d < FC_PEAKS_LANES; d <<= 1) {
        const int below = __shfl_up(incl, d, FC_PEAKS_LANES);
        if (lane >= d) incl += below;
    }
    int run = incl - sum;
    int* o = offsets + (size_t)m * units;
    for (int u = u0; u < u1; u++) { o[u] = run; run += c[u]; }
    if (lane == FC_PEAKS_LANES - 1) found[m] = incl;
}

}  // namespace

hipError_t launch_peaks(const void* maps, size_t map_elems, size_t map_stride, int format, int out_h, int nmaps, const PeakRule& rule, int max_peaks, int* scratch,
                        int* found, PeakRecord* peaks, hipStream_t s) {
    if (nmaps <= 0) return hipSuccess;
    if (!maps || !scratch || !found || !peaks || map_elems < 1 || map_elems >= (size_t)FC_EXTREMA_NONE || map_stride < map_elems) return hipErrorInvalidValue;
    if (out_h < 1 || map_elems % (size_t)out_h != 0 || max_peaks < 1 || rule.radius_h < 0 || rule.radius_w < 0 || rule.threshold != rule.threshold)
        return hipErrorInvalidValue;
    PeaksArgs a;
    a.maps = maps; a.map_elems = map_elems; a.map_stride = map_stride;
    a.out_h = out_h; a.out_w = (int)(map_elems / (size_t)out_h);
    a.bf16 = format == FC_MAP_BF16 ? 1 : 0;
    a.units = peaks_units(map_elems * fc_map_elem_bytes(format));
    a.rule = rule; a.max_peaks = max_peaks;
    a.counts = scratch; a.offsets = scratch + (size_t)nmaps * a.units;
    a.found = found; a.peaks = peaks;
    const dim3 grid((unsigned)((a.units + FC_PEAKS_THREADS / 64 - 1) / (FC_PEAKS_THREADS / 64)), (unsigned)nmaps), block(FC_PEAKS_THREADS);
    const bool f32 = format == FC_MAP_F32;
    if (f32) hipLaunchKernelGGL(k_peaks_count<float>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_peaks_count<uint16_t>, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_peaks_offsets, dim3((unsigned)nmaps), dim3(FC_PEAKS_LANES), 0, s, a.counts, a.units, a.offsets, a.found);
    if (f32) hipLaunchKernelGGL(k_peaks_write<float>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_peaks_write<uint16_t>, grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace fc
