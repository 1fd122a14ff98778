// border.hpp -- border modes (fftconv_plan_set_border): what the image is beyond its data -- a constant, its edge sample, its
// mirror image (with or without the edge sample repeated) or its periodic continuation -- mapped in the LOAD of the forward column
// pass: the border is never materialised by the caller.  Written once, compiled twice like every header here: by hipcc into the
// kernels (fast_cols_fwd.hpp: the Bd parameter of the body; kernels_pixels.hip: the staged route) and by the host compiler into
// the plan core and tests/border_host.
//
// Per dimension X with n = DATA_X samples and a plan's MAXK_X: lead = MAXK_X / 2, trail = MAXK_X - 1 - lead.  The forward pass
// transforms E[r] = Iext[r - lead] for window coordinates r < n + MAXK_X - 1 (zeros beyond, up to the transform length), and the
// "same" map is rows [MAXK_X - 1, MAXK_X - 1 + n) of the window.  The source index of window coordinate r, with t = r - lead:
//     t < 0 ? a0 + s0 * t : t >= n ? a1 + s1 * t : t
// -- compares and selects, four constants per (mode, dimension) made on the host; no division, no branch on the mode.  A fold is
// SINGLE: border_args_error refuses the sizes at which an index would have to be folded twice.
#pragma once
#include <cmath>

#include "fc_common.hpp"

namespace fc {

// (the values of FFTCONV_BORDER_* in include/fftconv.h)
constexpr int FC_BORDER_ZERO = 0, FC_BORDER_CONSTANT = 1, FC_BORDER_REPLICATE = 2, FC_BORDER_SYMMETRIC = 3, FC_BORDER_REFLECT101 = 4,
              FC_BORDER_CIRCULAR = 5;
constexpr bool fc_border_mode_ok(long m) { return m >= FC_BORDER_ZERO && m <= FC_BORDER_CIRCULAR; }
constexpr int border_lead(int maxk) { return maxk / 2; }
constexpr int border_trail(int maxk) { return maxk - 1 - maxk / 2; }

struct BorderAxis {
    int lead = 0;    // window coordinate of data sample 0
    int n = 0;       // data samples
    int a0 = 0, s0 = 0, a1 = 0, s1 = 0;
};

// The border uniforms of a launch, a kernel argument of its own (the bodies without a border never read it)
struct BorderLoad {
    int mode = FC_BORDER_ZERO;
    int fill = 0;        // CONSTANT: a sample outside the data in either dimension is `value` and is not loaded
    float value = 0.f;
    BorderAxis h, w;
};

// the body's border types: NoBorder is the text of every body as it was
struct NoBorder {};
struct Bordered {};

FC_HD bool border_outside(const BorderAxis& ax, int r) {
    const int t = r - ax.lead;
    return t < 0 || t >= ax.n;
}
// source index of window coordinate r in [0, n + MAXK - 1): always inside [0, n) for the sizes border_args_error admits (a
// `fill` axis gives 0 outside the data: the caller takes BorderLoad::value instead)
FC_HD int border_index(const BorderAxis& ax, int r) {
    const int t = r - ax.lead;
    return t < 0 ? ax.a0 + ax.s0 * t : t >= ax.n ? ax.a1 + ax.s1 * t : t;
}

inline BorderAxis border_axis(int mode, int n, int maxk) {
    BorderAxis ax;
    ax.lead = border_lead(maxk);
    ax.n = n;
    switch (mode) {
    case FC_BORDER_REPLICATE: ax.a0 = 0; ax.s0 = 0; ax.a1 = n - 1; ax.s1 = 0; break;                    // a a | a b c d | d d
    case FC_BORDER_SYMMETRIC: ax.a0 = -1; ax.s0 = -1; ax.a1 = 2 * n - 1; ax.s1 = -1; break;              // b a | a b c d | d c
    case FC_BORDER_REFLECT101: ax.a0 = 0; ax.s0 = -1; ax.a1 = 2 * n - 2; ax.s1 = -1; break;              // c b | a b c d | c b
    case FC_BORDER_CIRCULAR: ax.a0 = n; ax.s0 = 1; ax.a1 = -n; ax.s1 = 1; break;                         // c d | a b c d | a b
    default: break;                                                                                      // ZERO / CONSTANT: index 0, never loaded
    }
    return ax;
}

inline BorderLoad border_load(int mode, float value, int H, int W, int maxk_h, int maxk_w) {
    BorderLoad b;
    b.mode = mode;
    b.fill = (mode == FC_BORDER_CONSTANT || mode == FC_BORDER_ZERO) ? 1 : 0;
    b.value = mode == FC_BORDER_CONSTANT ? value : 0.f;
    b.h = border_axis(mode, H, maxk_h);
    b.w = border_axis(mode, W, maxk_w);
    return b;
}

// nullptr if (mode, value) is a border a plan of these sizes can have, else why not (the plan-state refusals -- block-wise,
// normalisation -- are the plan core's)
inline const char* border_args_error(int mode, float value, int H, int W, int maxk_h, int maxk_w) {
    if (!fc_border_mode_ok(mode)) return "the border mode is 0 (zero), 1 (constant), 2 (replicate), 3 (symmetric), 4 (reflect-101) or 5 (circular)";
    if (!std::isfinite(value)) return "the border value must be finite";
    const int lh = border_lead(maxk_h), lw = border_lead(maxk_w);
    if ((mode == FC_BORDER_SYMMETRIC || mode == FC_BORDER_CIRCULAR) && (lh > H || lw > W))
        return "the border would fold an index twice: symmetric and circular borders need MAX_KERNEL / 2 <= DATA in both dimensions";
    if (mode == FC_BORDER_REFLECT101 && (lh > H - 1 || lw > W - 1))
        return "the border would fold an index twice: a reflect-101 border needs MAX_KERNEL / 2 <= DATA - 1 in both dimensions";
    return nullptr;
}

// one sample of the extension E at window coordinates (r, c) of a plane `img` (column c' at img + c' * col_pitch, h contiguous)
FC_HD float border_sample(const float* img, int col_pitch, const BorderLoad& b, int r, int c) {
    if (b.fill && (border_outside(b.h, r) || border_outside(b.w, c))) return b.value;
    return img[(size_t)border_index(b.w, c) * col_pitch + border_index(b.h, r)];
}

}  // namespace fc
