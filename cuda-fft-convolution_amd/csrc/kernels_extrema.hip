// kernels_extrema.hip -- per-map extrema (fftconv_plan_set_extrema; extrema.hpp): the scan kernel for every route the output kernel's
// fused store does not serve, the fold kernel both feed, and the launcher of the fused stores (kernels_cols_*ext_g<G>.hip).
//
// Both routes end in the same place: per map a run of partials (fused: one per tile and wave of the output launch; scan: one per
// block), reduced by ONE fold launch per output launch into the caller's records.  No atomics, no clearing: every slot the fold
// reads was written by the launch before it on the same stream.
#include "kernels_common.hpp"

namespace fc {
namespace {

// the workgroup's partial from its threads': the waves' by cross-lane exchanges (fast_cols.hpp), the workgroup's through LDS
template <int NT>
__device__ __forceinline__ ExtremaPartial extrema_block_reduce(ExtremaPartial p) {
    __shared__ ExtremaPartial wave_partial[NT / 64];
    p = extrema_wave_reduce(p);
    const int t = (int)threadIdx.x;
    if ((t & 63) == 0) wave_partial[t >> 6] = p;
    __syncthreads();
    ExtremaPartial r = wave_partial[0];
    for (int w = 1; w < NT / 64; w++) r = extrema_merge(r, wave_partial[w]);
    return r;
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// The scan: block (b, m) reads its share of map m -- whole 16-byte vectors of the map's bytes, cut at 16-byte ADDRESSES so that a map
// whose first element is not aligned (an odd number of elements per map) still loads wide; the vectors that straddle the map's first
// or last byte are read element by element.  E: the element type (float, or uint16_t of `bf16` or fp16).
template <class E>
__global__ void __launch_bounds__(FC_EXTREMA_SCAN_THREADS) k_extrema_scan(const E* maps, size_t map_elems, size_t map_stride, int bf16, int blocks_per_map,
                                                                          ExtremaPartial* partials) {
    constexpr int EPV = 16 / sizeof(E);      // elements per vector
    const int m = (int)blockIdx.y, b = (int)blockIdx.x, t = (int)threadIdx.x;
    const E* map = maps + (size_t)m * map_stride;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(map), a1 = a0 + map_elems * sizeof(E);
    const uintptr_t v0 = a0 / 16, v1 = (a1 + 15) / 16;      // vectors [v0, v1) touch the map
    const size_t nv = v1 - v0, per_block = (nv + blocks_per_map - 1) / blocks_per_map;
    const size_t lo = (size_t)b * per_block, hi = lo + per_block < nv ? lo + per_block : nv;
    auto value = [&](E e) -> float {
        if constexpr (sizeof(E) == 4) return e;
        else return extrema_map16_value(e, bf16 != 0);
    };
    ExtremaPartial ex = extrema_empty();
    for (size_t v = lo + t; v < hi; v += FC_EXTREMA_SCAN_THREADS) {
        const uintptr_t va = (v0 + v) * 16;
        // (signed: the first vector may start ahead of the map)
        const long e0 = ((long)va - (long)a0) / (long)sizeof(E);
        if (va >= a0 && va + 16 <= a1) {
            const u32x4 w = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(va));
            E e[EPV];
            __builtin_memcpy(e, &w, 16);
#pragma unroll
            for (int i = 0; i < EPV; i++) extrema_take(ex, value(e[i]), (int)(e0 + i));
        } else {
            for (int i = 0; i < EPV; i++) {
                const long ei = e0 + i;
                if (ei >= 0 && (size_t)ei < map_elems) extrema_take(ex, value(map[ei]), (int)ei);
            }
        }
    }
    ex = extrema_block_reduce<FC_EXTREMA_SCAN_THREADS>(ex);
    if (t == 0) partials[(size_t)m * blocks_per_map + b] = ex;
}

constexpr int FC_EXTREMA_FOLD_THREADS = 256;
// The fold: block m reduces the per_map partials of map m to its record
__global__ void __launch_bounds__(FC_EXTREMA_FOLD_THREADS) k_extrema_fold(const ExtremaPartial* partials, int per_map, int out_h, ExtremaRecord* records) {
    const int m = (int)blockIdx.x, t = (int)threadIdx.x;
    const ExtremaPartial* p = partials + (size_t)m * per_map;
    ExtremaPartial ex = extrema_empty();
    for (int i = t; i < per_map; i += FC_EXTREMA_FOLD_THREADS) ex = extrema_merge(ex, p[i]);
    ex = extrema_block_reduce<FC_EXTREMA_FOLD_THREADS>(ex);
    if (t == 0) records[m] = extrema_record(ex, out_h);
}

template <int N, class F>
hipError_t in_first_group(F&& f) {
    return first_group<N>(f).value_or(hipErrorInvalidValue);
}

}  // namespace

hipError_t launch_extrema_scan(const void* maps, size_t map_elems, size_t map_stride, int format, int nmaps, ExtremaPartial* partials, hipStream_t s) {
    if (nmaps <= 0) return hipSuccess;
    if (!maps || !partials || map_elems < 1 || map_elems >= (size_t)FC_EXTREMA_NONE || map_stride < map_elems) return hipErrorInvalidValue;
    const int nb = extrema_scan_blocks(map_elems * fc_map_elem_bytes(format));
    const dim3 grid((unsigned)nb, (unsigned)nmaps), block(FC_EXTREMA_SCAN_THREADS);
    if (format == FC_MAP_F32) hipLaunchKernelGGL(k_extrema_scan<float>, grid, block, 0, s, static_cast<const float*>(maps), map_elems, map_stride, 0, nb, partials);
    else hipLaunchKernelGGL(k_extrema_scan<uint16_t>, grid, block, 0, s, static_cast<const uint16_t*>(maps), map_elems, map_stride, format == FC_MAP_BF16 ? 1 : 0, nb, partials);
    return hipGetLastError();
}

hipError_t launch_extrema_fold(const ExtremaPartial* partials, int per_map, int nmaps, int out_h, ExtremaRecord* records, hipStream_t s) {
    if (nmaps <= 0) return hipSuccess;
    if (!partials || !records || per_map < 1 || out_h < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_extrema_fold, dim3((unsigned)nmaps), dim3(FC_EXTREMA_FOLD_THREADS), 0, s, partials, per_map, out_h, records);
    return hipGetLastError();
}

hipError_t launch_fast_cols_rect_extrema(int M, int T, const FastColsShape& shape, hipStream_t s) {
    if (shape.a.ntiles <= 0) return hipSuccess;
    if (!shape.a.y_tiled || (shape.variant != FastColsVariant::TILED && shape.variant != FastColsVariant::TILED_DYN)) return hipErrorInvalidValue;
    if (!shape.extrema.partials || shape.strided || shape.a.out_format != FC_MAP_F32) return hipErrorInvalidValue;
    // (the index of a delivered element is an int: extrema.hpp)
    if ((size_t)(shape.a.fft_h - shape.a.h_lo) * (size_t)shape.a.rect_w_n >= (size_t)FC_EXTREMA_NONE) return hipErrorInvalidValue;
    const MapPlane& pl = shape.plane;
    if (pl.kind == PlaneKind::Scale) {
        if (!pl.plane || pl.per_image < 1) return hipErrorInvalidValue;
        return in_first_group<FC_COL_GROUPS>([&](auto g) { return launch_fast_cols_rect_scale_ext_group<g.value>(M, T, shape, s); });
    }
    if (pl.kind == PlaneKind::Add) {
        if (!fast_cols_sqdiff_args_ok(fast_cols_sqdiff_args(pl))) return hipErrorInvalidValue;
        return in_first_group<FC_COL_GROUPS>([&](auto g) { return launch_fast_cols_rect_add_ext_group<g.value>(M, T, shape, s); });
    }
    return in_first_group<FC_COL_GROUPS>([&](auto g) { return launch_fast_cols_rect_ext_group<g.value>(M, T, shape, s); });
}

}  // namespace fc
