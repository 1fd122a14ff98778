// spectral_filter.hpp -- the pointwise operation between the forward and the inverse w-transform of the spectral-row kernels
// (fftconv_plan_set_spectral_filter; the definition: include/fftconv.h).  Written once: the specialised row kernel
// (fast_rows_multi.hpp P3, FILTER), the generic one (kernels_body.hpp: spectral_rows_body) and the CPU tier
// (tests/spectral_filter_host) all call this text.
//
// What reaches it: k, a bin of the kernel's UNSCALED 2-D spectrum, and s, the same bin of the image spectrum PRE-SCALED by
// c = 1 / (Lh * Lw) (kernels_body.hpp: the layouts) -- the inverse transforms behind it are unnormalised, so the value that
// leaves must carry that one factor c:
//   PRODUCT  k * s                                             = c * I K
//   PHASE    P_s = k * s, m = |P_s|^2:  P_s * (c * rsq(m))     = c * P / |P|       (c: `param`)
//   WIENER   s * conj(k) * rcp(|k|^2 + lambda)                 = c * I conj(K) / (|K|^2 + lambda)      (lambda: `param`)
// A bin whose m or whose denominator is below the smallest normal float (zero, or a subnormal the reciprocal instructions
// would take for zero) gives 0, never inf or NaN; one whose m or denominator overflows gives 0 too (rsq / rcp of inf), as long as
// the products themselves are finite -- where they are not, the plain product overflows at the same bin.  The reciprocals are the
// hardware's v_rcp_f32 / v_rsq_f32 (1 ulp).
#pragma once
#include "fc_common.hpp"

namespace fc {

enum { FC_FILTER_PRODUCT = 0, FC_FILTER_PHASE = 1, FC_FILTER_WIENER = 2 };
FC_HD constexpr bool fc_filter_mode_ok(long mode) { return mode >= FC_FILTER_PRODUCT && mode <= FC_FILTER_WIENER; }

constexpr float FC_FILTER_TINY = 1.17549435e-38f;      // FLT_MIN

FC_HD float fc_rcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);
#else
    return 1.0f / x;
#endif
}
FC_HD float fc_rsq(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rsqf(x);
#else
    return 1.0f / __builtin_sqrtf(x);
#endif
}

// c * P / |P| with P = I K (s = c I)
FC_HD c32 spectral_filter_phase(c32 k, c32 s, float c) {
    const c32 p = cmul(k, s);
    const float m = __builtin_fmaf(p.x, p.x, p.y * p.y);
    const float r = m >= FC_FILTER_TINY ? c * fc_rsq(m) : 0.f;
    return m >= FC_FILTER_TINY ? scale(p, r) : mk(0.f, 0.f);
}
// c * I conj(K) / (|K|^2 + lambda)
FC_HD c32 spectral_filter_wiener(c32 k, c32 s, float lambda) {
    const float den = __builtin_fmaf(k.x, k.x, __builtin_fmaf(k.y, k.y, lambda));
    const c32 n = cmulc(s, k);
    return den >= FC_FILTER_TINY ? scale(n, fc_rcp(den)) : mk(0.f, 0.f);
}
// the uniform `param` of a launch under `mode`: c for PHASE (formed in double), lambda for WIENER
inline float spectral_filter_launch_param(long mode, float lambda, int Lh, int Lw) {
    if (mode == FC_FILTER_PHASE) return (float)(1.0 / ((double)Lh * (double)Lw));
    return mode == FC_FILTER_WIENER ? lambda : 0.f;
}
// any mode behind a run-time branch (the generic kernel, one bin at a time)
FC_HD c32 spectral_filter_apply(int mode, float param, c32 k, c32 s) {
    if (mode == FC_FILTER_PHASE) return spectral_filter_phase(k, s, param);
    if (mode == FC_FILTER_WIENER) return spectral_filter_wiener(k, s, param);
    return cmul(k, s);
}
// fftconv_plan_set_spectral_filter: why (mode, param) is refused, or nullptr
inline const char* spectral_filter_args_error(int mode, float param) {
    if (!fc_filter_mode_ok(mode)) return "the spectral filter is 0 (product), 1 (phase correlation) or 2 (Wiener)";
    if (!(param == param) || param - param != 0.f) return "the filter parameter must be finite";
    if (param < 0.f) return "the filter parameter must not be negative";
    if (mode == FC_FILTER_PHASE && param != 0.f) return "the filter parameter must be 0 in mode 1 (reserved for a regulariser)";
    return nullptr;
}

}  // namespace fc
