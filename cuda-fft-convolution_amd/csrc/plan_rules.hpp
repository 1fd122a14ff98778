// plan_rules.hpp -- what refuses what, and what invalidates what, among the plan's setters: two tables, the one place where the
// interactions of the plan's mutable state are written down ("Plan state", repeats them as the reference).  The setters of
// fftconv_api.cpp and the spectrum entries of plan_image.cpp only look a request up (plan_refusal) and perform the effects the
// table names (fftconv_api.cpp: apply_effects).  Host-only and HIP-free like output_route.hpp: tests/plan_rules_host holds both
// tables against the conditions and the sequences they replaced, with the plain host compiler.
//
// Not here, because nothing is refused: the route conditions that silently give way -- fftconv_plan::image_walk_active() to a
// spectral filter (the image walk has no filter form), fftconv_plan::pixel_direct() to a border (typed pixels under a border are
// converted first) -- and the argument checks of one setter alone (output_rect_error, output_stride_error, map_format_error,
// ncc_args_error, score_args_error, border_args_error, spectral_filter_args_error).
#pragma once
#include "../../include/fftconv.h"
#include "fc_common.hpp"

namespace fc {

// ---- effects: what a changed value invalidates, performed in this order ----
enum : unsigned {
    FX_WAIT = 1,      // the plan's stream is waited for (launches in flight read the state that changes)
    FX_RING = 2,      // the host-output ring is sized by it: torn down, rebuilt by the next host-output call
    FX_COLUMNS = 4,   // the kernel column spectra in A depend on it: ColumnCache::forget
    FX_IMAGES = 8,    // the spectrum (and the plane of a score) belongs to it: the plan holds no image afterwards
};

enum class Setter { OutputRect, OutputRegion, OutputStride, Score, Border, Filter };
struct SetterEffects {
    Setter setter;
    unsigned changed;        // FX_* of a call that changes the value
    bool unchanged_returns;  // a call that changes nothing returns ahead of them
};
// (the plain `long` options name their effects in kLongOptions, fftconv_api.cpp: FX_WAIT | FX_RING or FX_COLUMNS, never an early return)
constexpr SetterEffects kSetterEffects[] = {
    {Setter::OutputRect, FX_WAIT | FX_RING, false},      // fftconv_plan_set_output_rect: the ring is sized for the map bytes
    {Setter::OutputRegion, FX_WAIT | FX_RING, false},    // option "output_region"
    {Setter::OutputStride, FX_WAIT | FX_RING, true},     // fftconv_plan_set_output_stride: output-side state alone
    // fftconv_plan_set_normalisation / _set_match_score: the kernels are prepared per score, the plane belongs to (image, score, box).
    // No FX_RING: every score stores maps of the size the plan had (DESIGN.md 5 discusses the asymmetries)
    {Setter::Score, FX_WAIT | FX_COLUMNS | FX_IMAGES, true},
    {Setter::Border, FX_WAIT | FX_RING | FX_COLUMNS | FX_IMAGES, true},      // fftconv_plan_set_border: it rewrites the region too
    {Setter::Filter, 0, false},                          // fftconv_plan_set_spectral_filter: state of the row launches alone
};
constexpr const SetterEffects& setter_effects(Setter s) { return kSetterEffects[(int)s]; }

// ---- exclusions: "asking X is refused while Y holds" ----
enum class Ask { Score, Border, Filter, ImportSpectrum, MarkSpectrumValid };
enum class Holds { Blockwise, ScoreOn, ScorePlane, BorderOn, FilterOn, Features, NoFilterKernel, WindowSink };

// the state the rules read
struct PlanRuleState {
    int blocks = 0;             // of a block-wise plan; 0: one pass
    int F = 1;
    long score = 0, border = 0, filter = 0;      // opt_score, border_mode, opt_filter
    bool rows_fast = false;     // the spectral rows run a specialised kernel ...
    bool filter_built = false;  // ... whose FILTER form exists (fast_paths.hpp: fast_rows_filter_built)
    int Lw = 0;                 // the row length
    bool window_sink = false;   // the group at hand stores through an output window (the block plan of an overlap-save plan)
};

// 0 while Y does not hold, else the integer the rule's message names (block count, score, mode, feature_dim, row length)
inline long holds_value(const PlanRuleState& s, Holds y) {
    switch (y) {
    case Holds::Blockwise: return s.blocks;
    case Holds::ScoreOn: return s.score;
    case Holds::ScorePlane: return score_has_plane(s.score) ? s.score : 0;
    case Holds::BorderOn: return s.border;
    case Holds::FilterOn: return s.filter;
    case Holds::Features: return s.F > 1 ? s.F : 0;
    case Holds::NoFilterKernel: return s.rows_fast && !s.filter_built ? s.Lw : 0;
    case Holds::WindowSink: return s.window_sink ? 1 : 0;
    }
    return 0;
}

struct PlanRule {
    Ask ask;
    Holds holds;
    bool off_too;       // also refused when the call switches X off (value 0); otherwise switching off always passes
    int code;
    const char* fmt;    // at most one conversion, %ld: holds_value
};
// In the order the checks are made: the first rule that applies is the refusal.  The set is closed -- a new feature adds its rows here.
constexpr PlanRule kPlanRules[] = {
    {Ask::Score, Holds::Blockwise, true, FFTCONV_ERR_INVALID_ARG,
     "normalisation is not available on a block-wise plan (%ld blocks: the window statistics span blocks); create a one-pass plan "
     "(fftconv_plan_options.blockwise = 1)"},
    {Ask::Score, Holds::BorderOn, false, FFTCONV_ERR_INVALID_ARG,
     "a border is on (fftconv_plan_set_border, mode %ld): the window statistics of normalised maps assume zero padding"},
    {Ask::Score, Holds::FilterOn, false, FFTCONV_ERR_INVALID_ARG,
     "spectral filter %ld is on (fftconv_plan_set_spectral_filter): the window statistics of a score belong to the plain product"},
    {Ask::Border, Holds::Blockwise, true, FFTCONV_ERR_INVALID_ARG,
     "a border is not available on a block-wise plan (%ld blocks: the blocks' own rims lie inside the image); create a one-pass plan "
     "(fftconv_plan_options.blockwise = 1)"},
    {Ask::Border, Holds::ScoreOn, false, FFTCONV_ERR_INVALID_ARG,
     "normalisation is on (fftconv_plan_set_normalisation): the window statistics of normalised maps assume zero padding"},
    {Ask::Filter, Holds::Blockwise, false, FFTCONV_ERR_INVALID_ARG,
     "a spectral filter is not available on a block-wise plan (%ld blocks: the filter is defined on one transform of the whole window); "
     "create a one-pass plan (fftconv_plan_options.blockwise = 1)"},
    {Ask::Filter, Holds::Features, false, FFTCONV_ERR_INVALID_ARG,
     "a spectral filter needs feature_dim 1 (this plan: %ld): the filter of a feature sum is another formula"},
    {Ask::Filter, Holds::ScoreOn, false, FFTCONV_ERR_INVALID_ARG,
     "matching score %ld is on (fftconv_plan_set_match_score / _set_normalisation): its window statistics belong to the plain product"},
    {Ask::Filter, Holds::NoFilterKernel, false, FFTCONV_ERR_INVALID_ARG,
     "the specialised spectral-row kernel of %ld points has no filter form (it would spill registers); create the plan with "
     "fftconv_plan_options.kernel_path = 1 (generic kernels)"},
    {Ask::ImportSpectrum, Holds::ScorePlane, true, FFTCONV_ERR_INVALID_ARG,
     "normalisation is on (fftconv_plan_set_normalisation): an imported spectrum carries no window statistics"},
    {Ask::ImportSpectrum, Holds::BorderOn, true, FFTCONV_ERR_INVALID_ARG,
     "a border is on (fftconv_plan_set_border, mode %ld): an imported spectrum carries no border"},
    {Ask::MarkSpectrumValid, Holds::ScorePlane, true, FFTCONV_ERR_INVALID_ARG,
     "normalisation is on (fftconv_plan_set_normalisation): a spectrum written by the caller carries no window statistics"},
    {Ask::MarkSpectrumValid, Holds::BorderOn, true, FFTCONV_ERR_INVALID_ARG,
     "a border is on (fftconv_plan_set_border, mode %ld): a spectrum written by the caller carries no border"},
};

// ---- the output side: per-map extrema (fftconv_plan_set_extrema) ----
// Tables of their own beside the two above, with the same row types and the same lookups: tests/plan_rules_host holds kSetterEffects and
// kPlanRules row for row against the entry points they replaced (every row counted, every request of `Ask` walked), so the rows of an
// entry point that commit did not have are listed here, and setter_effects / plan_refusal answer from both.
//   effects   output-side state of its own, as the stride is: it keeps the image, the prepared kernels and the stream, stays while extent,
//             format, score or images change, and a call that changes nothing returns early.  FX_WAIT: launches in flight write the
//             records and the partials the call reallocates.
//   refusals  switching it ON on a block-wise plan, whose maps are stored through output windows block by block; a group under
//             extrema whose sink is such a window.
enum class SetterAdded { Extrema };
struct AddedSetterEffects {
    SetterAdded setter;
    unsigned changed;
    bool unchanged_returns;
};
constexpr AddedSetterEffects kSetterEffectsAdded[] = {
    {SetterAdded::Extrema, FX_WAIT, true},      // fftconv_plan_set_extrema
};
constexpr const AddedSetterEffects& setter_effects(SetterAdded s) { return kSetterEffectsAdded[(int)s]; }

enum class AskOutput { Extrema, ExtremaGroup };
struct OutputRule {
    AskOutput ask;
    Holds holds;
    bool off_too;
    int code;
    const char* fmt;
};
constexpr OutputRule kOutputRules[] = {
    {AskOutput::Extrema, Holds::Blockwise, false, FFTCONV_ERR_INVALID_ARG,
     "per-map extrema are not available on a block-wise plan (%ld blocks: its maps are stored through output windows block by block); create a "
     "one-pass plan (fftconv_plan_options.blockwise = 1)"},
    {AskOutput::ExtremaGroup, Holds::WindowSink, true, FFTCONV_ERR_INVALID_ARG,
     "per-map extrema are on (fftconv_plan_set_extrema): an output window holds a part of a map (%ld), not a delivered map"},
};

// ---- the output side: peak lists (fftconv_plan_set_peaks) ----
// Tables of their own again, for the same reason: tests/extrema_host counts the rows of the two tables above.  The rows are the extrema
// rows' in effect and in wording -- output-side state of its own, FX_WAIT because launches in flight write the lists a change
// reallocates, an early return for a call that changes nothing; refused on a block-wise plan and for a group whose sink is a window.
enum class SetterPeaks { Peaks };
struct PeaksSetterEffects {
    SetterPeaks setter;
    unsigned changed;
    bool unchanged_returns;
};
constexpr PeaksSetterEffects kSetterEffectsPeaks[] = {
    {SetterPeaks::Peaks, FX_WAIT, true},      // fftconv_plan_set_peaks: the effects the extrema setter has
};
constexpr const PeaksSetterEffects& setter_effects(SetterPeaks s) { return kSetterEffectsPeaks[(int)s]; }

enum class AskPeaks { Peaks, PeaksGroup };
struct PeaksRule {
    AskPeaks ask;
    Holds holds;
    bool off_too;
    int code;
    const char* fmt;
};
constexpr PeaksRule kPeaksRules[] = {
    {AskPeaks::Peaks, Holds::Blockwise, false, FFTCONV_ERR_INVALID_ARG,
     "peak lists are not available on a block-wise plan (%ld blocks: its maps are stored through output windows block by block); create a "
     "one-pass plan (fftconv_plan_options.blockwise = 1)"},
    {AskPeaks::PeaksGroup, Holds::WindowSink, true, FFTCONV_ERR_INVALID_ARG,
     "peak lists are on (fftconv_plan_set_peaks): an output window holds a part of a map (%ld), not a delivered map"},
};

struct Refusal {
    const PlanRule* rule = nullptr;      // nullptr: the request passes
    long arg = 0;                        // what rule->fmt formats
    explicit operator bool() const { return rule != nullptr; }
};
// the first rule that refuses asking `ask` for `value` (the score, the border mode, the filter mode; the spectrum entries: any)
inline Refusal plan_refusal(const PlanRuleState& s, Ask ask, long value) {
    for (const PlanRule& r : kPlanRules) {
        if (r.ask != ask || (value == 0 && !r.off_too)) continue;
        if (const long arg = holds_value(s, r.holds)) return {&r, arg};
    }
    return {};
}
struct OutputRefusal {
    const OutputRule* rule = nullptr;
    long arg = 0;
    explicit operator bool() const { return rule != nullptr; }
};
inline OutputRefusal plan_refusal(const PlanRuleState& s, AskOutput ask, long value) {
    for (const OutputRule& r : kOutputRules) {
        if (r.ask != ask || (value == 0 && !r.off_too)) continue;
        if (const long arg = holds_value(s, r.holds)) return {&r, arg};
    }
    return {};
}
struct PeaksRefusal {
    const PeaksRule* rule = nullptr;
    long arg = 0;
    explicit operator bool() const { return rule != nullptr; }
};
inline PeaksRefusal plan_refusal(const PlanRuleState& s, AskPeaks ask, long value) {
    for (const PeaksRule& r : kPeaksRules) {
        if (r.ask != ask || (value == 0 && !r.off_too)) continue;
        if (const long arg = holds_value(s, r.holds)) return {&r, arg};
    }
    return {};
}

}  // namespace fc
