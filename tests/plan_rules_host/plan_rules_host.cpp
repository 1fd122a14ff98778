// plan_rules_host.cpp -- TEST-ONLY stand-alone host program for csrc/plan_rules.hpp (kPlanRules / plan_refusal: which setter is refused
// while which state holds; kSetterEffects: what a changed value invalidates).
//
// Built by tests/test_plan_rules_host.py with the host compiler from the product's headers alone.  Modes:
//   rules    plan_refusal against a literal transcription of the conditions it replaced, as they stood in the commit before the table
//            existed -- the `if` chains of set_score, fftconv_plan_set_border and fftconv_plan_set_spectral_filter (fftconv_api.cpp) and
//            of the import and mark-valid entries (plan_image.cpp), in their order; file and line are in the comments -- over the full
//            product of the state axes and the requests listed in cmd_rules: refused or not, the code, and the formatted message
//            byte for byte.  The number of comparisons is printed, and the test holds it against the product
//   effects  kSetterEffects against a literal list of what each entry point did ahead of its assignments in that commit
// Having its own main, it is also the place for a host sanitizer build (-fsanitize=address,undefined) of this code.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "fast_paths.hpp"
#include "plan_rules.hpp"

using namespace fc;

namespace {

// ---- the transcription ----
char g_msg[512];
int api_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int api_fail(int code, const char* fmt, ...) {      // fftconv_api.cpp:20
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
    return code;
}

// the plan as the parent's conditions read it
struct Tiled { int nblk; };
struct Plan {
    const Tiled* tiled = nullptr;
    struct { int F = 1, Lw = 0; struct { bool ok = false; } fast_rows; } g;
    long opt_score = 0, border_mode = 0, opt_filter = 0;
    bool score_planes() const { return score_has_plane(opt_score); }      // plan_internal.hpp:302
};

int parent_set_score(const Plan* plan, int score) {      // fftconv_api.cpp:794-803
    if (plan->tiled)
        return api_fail(FFTCONV_ERR_INVALID_ARG, "normalisation is not available on a block-wise plan (%d blocks: the window statistics span blocks); "
                        "create a one-pass plan (fftconv_plan_options.blockwise = 1)", plan->tiled->nblk);
    if (score != 0 && plan->border_mode)
        return api_fail(FFTCONV_ERR_INVALID_ARG, "a border is on (fftconv_plan_set_border, mode %ld): the window statistics of normalised maps assume zero padding",
                        plan->border_mode);
    if (score != 0 && plan->opt_filter)
        return api_fail(FFTCONV_ERR_INVALID_ARG, "spectral filter %ld is on (fftconv_plan_set_spectral_filter): the window statistics of a score belong to the "
                        "plain product", plan->opt_filter);
    return 0;
}

int parent_set_border(const Plan* plan, int mode) {      // fftconv_api.cpp:837-841 (behind border_args_error, which stays)
    if (plan->tiled)
        return api_fail(FFTCONV_ERR_INVALID_ARG, "a border is not available on a block-wise plan (%d blocks: the blocks' own rims lie inside the image); "
                        "create a one-pass plan (fftconv_plan_options.blockwise = 1)", plan->tiled->nblk);
    if (mode != 0 && plan->opt_score)
        return api_fail(FFTCONV_ERR_INVALID_ARG, "normalisation is on (fftconv_plan_set_normalisation): the window statistics of normalised maps assume zero padding");
    return 0;
}

int parent_set_spectral_filter(const Plan* plan, int mode) {      // fftconv_api.cpp:865-877 (behind spectral_filter_args_error, which stays)
    const auto& g = plan->g;
    if (mode != FC_FILTER_PRODUCT) {
        if (plan->tiled)
            return api_fail(FFTCONV_ERR_INVALID_ARG, "a spectral filter is not available on a block-wise plan (%d blocks: the filter is defined on one transform of the "
                            "whole window); create a one-pass plan (fftconv_plan_options.blockwise = 1)", plan->tiled->nblk);
        if (g.F > 1)
            return api_fail(FFTCONV_ERR_INVALID_ARG, "a spectral filter needs feature_dim 1 (this plan: %d): the filter of a feature sum is another formula", g.F);
        if (plan->opt_score)
            return api_fail(FFTCONV_ERR_INVALID_ARG, "matching score %ld is on (fftconv_plan_set_match_score / _set_normalisation): its window statistics belong to "
                            "the plain product", plan->opt_score);
        if (g.fast_rows.ok && !fast_rows_filter_built(g.Lw))
            return api_fail(FFTCONV_ERR_INVALID_ARG, "the specialised spectral-row kernel of %d points has no filter form (it would spill registers); create the plan "
                            "with fftconv_plan_options.kernel_path = 1 (generic kernels)", g.Lw);
    }
    return 0;
}

int parent_import_spectrum(const Plan* p) {      // plan_image.cpp:267-270 (spectrum_exchange with to_natural false)
    const bool to_natural = false;
    if (!to_natural && p->score_planes())
        return api_fail(FFTCONV_ERR_INVALID_ARG, "normalisation is on (fftconv_plan_set_normalisation): an imported spectrum carries no window statistics");
    if (!to_natural && p->border_mode)
        return api_fail(FFTCONV_ERR_INVALID_ARG, "a border is on (fftconv_plan_set_border, mode %ld): an imported spectrum carries no border", p->border_mode);
    return 0;
}

int parent_mark_spectrum_valid(const Plan* plan) {      // plan_image.cpp:333-336
    if (plan->score_planes())
        return api_fail(FFTCONV_ERR_INVALID_ARG, "normalisation is on (fftconv_plan_set_normalisation): a spectrum written by the caller carries no window statistics");
    if (plan->border_mode)
        return api_fail(FFTCONV_ERR_INVALID_ARG, "a border is on (fftconv_plan_set_border, mode %ld): a spectrum written by the caller carries no border", plan->border_mode);
    return 0;
}

// ---- the table on the same plan: what plan_internal.hpp's plan_refused fills in ----
PlanRuleState rule_state(const Plan& p) {
    PlanRuleState s;
    s.blocks = p.tiled ? p.tiled->nblk : 0;
    s.F = p.g.F;
    s.score = p.opt_score; s.border = p.border_mode; s.filter = p.opt_filter;
    s.rows_fast = p.g.fast_rows.ok; s.filter_built = fast_rows_filter_built(p.g.Lw); s.Lw = p.g.Lw;
    return s;
}

constexpr int L_GENERIC = 56, L_BUILT = 288, L_NOT_BUILT = 7040;      // no specialised row kernel; one with its filter form; one without

// the 16 requests: score 0-4, border 0-5, filter 0-2, import, mark-valid
struct Request { Ask ask; long value; };
Request request_of(int r) {
    if (r < 5) return {Ask::Score, r};
    if (r < 11) return {Ask::Border, r - 5};
    if (r < 14) return {Ask::Filter, r - 11};
    return {r == 14 ? Ask::ImportSpectrum : Ask::MarkSpectrumValid, 1};
}
int parent_answer(const Plan& p, const Request& q) {
    g_msg[0] = 0;
    switch (q.ask) {
    case Ask::Score: return parent_set_score(&p, (int)q.value);
    case Ask::Border: return parent_set_border(&p, (int)q.value);
    case Ask::Filter: return parent_set_spectral_filter(&p, (int)q.value);
    case Ask::ImportSpectrum: return parent_import_spectrum(&p);
    case Ask::MarkSpectrumValid: return parent_mark_spectrum_valid(&p);
    }
    return 0;
}

int cmd_rules() {
    if (fast_rows_length(L_GENERIC, 1) || !fast_rows_length(L_BUILT, 1) || !fast_rows_length(L_NOT_BUILT, 1) || !fast_rows_filter_built(L_BUILT) ||
        fast_rows_filter_built(L_NOT_BUILT)) {
        printf("FAIL the three row lengths are not what this walk names them\n");
        return 1;
    }
    const Tiled one_block_plan = {1};
    long compared = 0, differ = 0, refused = 0, seen_rule[sizeof(kPlanRules) / sizeof(kPlanRules[0])] = {};
    for (int blockwise = 0; blockwise < 2; blockwise++)
    for (int F = 1; F <= 2; F++)
    for (long score = 0; score <= 4; score++)
    for (long border = 0; border <= 5; border++)
    for (long filter = 0; filter <= 2; filter++)
    for (int rows = 0; rows < 3; rows++)      // generic, specialised with the filter kernel, specialised at 7040
    for (int r = 0; r < 16; r++) {
        Plan p;
        p.tiled = blockwise ? &one_block_plan : nullptr;
        p.g.F = F; p.g.fast_rows.ok = rows != 0; p.g.Lw = rows == 0 ? L_GENERIC : rows == 1 ? L_BUILT : L_NOT_BUILT;
        p.opt_score = score; p.border_mode = border; p.opt_filter = filter;
        const Request q = request_of(r);
        const int want = parent_answer(p, q);
        const Refusal got = plan_refusal(rule_state(p), q.ask, q.value);
        char msg[512] = "";
        if (got) {
            snprintf(msg, sizeof(msg), got.rule->fmt, got.arg);
            seen_rule[got.rule - kPlanRules]++;
        }
        compared++;
        refused += want != 0;
        if (((want != 0) != (bool)got || (got && got.rule->code != want) || strcmp(msg, g_msg)) && differ++ < 20)
            printf("FAIL block-wise %d F %d score %ld border %ld filter %ld rows %d request %d (value %ld): parent %d '%s'; table %d '%s'\n", blockwise, F, score, border,
                   filter, rows, r, q.value, want, g_msg, got ? got.rule->code : 0, msg);
    }
    for (size_t i = 0; i < sizeof(seen_rule) / sizeof(seen_rule[0]); i++)
        if (!seen_rule[i]) { printf("FAIL no combination is refused by rule %zu: a dead row, or the walk misses it\n", i); differ++; }
    printf("rules: %ld comparisons, %ld refused, %ld differ\n", compared, refused, differ);
    return differ ? 1 : 0;
}

// ---- the effects ----
// what each entry point did ahead of its assignments in the parent, in the order use_device + hipStreamSynchronize, release_ring,
// a_holds.forget, n_images = 0; early: `return 0` ahead of them for a value that does not change
struct ParentEffects { Setter setter; const char* where; bool wait, ring, forget, images, early; };
const ParentEffects kParent[] = {
    {Setter::OutputRect, "fftconv_plan_set_output_rect, fftconv_api.cpp:773-775", true, true, false, false, false},
    {Setter::OutputRegion, "option output_region, fftconv_api.cpp:756-758", true, true, false, false, false},
    {Setter::OutputStride, "fftconv_plan_set_output_stride, fftconv_api.cpp:784-787", true, true, false, false, true},
    {Setter::Score, "set_score, fftconv_api.cpp:805-810", true, false, true, true, true},
    {Setter::Border, "fftconv_plan_set_border, fftconv_api.cpp:843-849", true, true, true, true, true},
    {Setter::Filter, "fftconv_plan_set_spectral_filter, fftconv_api.cpp:878-879", false, false, false, false, false},
};

int cmd_effects() {
    int failed = 0;
    if (sizeof(kParent) / sizeof(kParent[0]) != sizeof(kSetterEffects) / sizeof(kSetterEffects[0])) { printf("FAIL the table has another number of rows\n"); failed++; }
    for (const ParentEffects& w : kParent) {
        const SetterEffects& e = setter_effects(w.setter);
        const unsigned want = (w.wait ? FX_WAIT : 0) | (w.ring ? FX_RING : 0) | (w.forget ? FX_COLUMNS : 0) | (w.images ? FX_IMAGES : 0);
        const bool ok = e.setter == w.setter && e.changed == want && e.unchanged_returns == w.early;
        printf("%s %s: effects %u (table %u), early return %d (table %d)\n", ok ? "ok  " : "FAIL", w.where, want, e.changed, (int)w.early, (int)e.unchanged_returns);
        failed += !ok;
    }
    // the flags are four distinct bits, performed in ascending order (fftconv_api.cpp: apply_effects)
    if (!(FX_WAIT < FX_RING && FX_RING < FX_COLUMNS && FX_COLUMNS < FX_IMAGES) || (FX_WAIT | FX_RING | FX_COLUMNS | FX_IMAGES) != 15u) { printf("FAIL the flags\n"); failed++; }
    printf("effects: %d failed\n", failed);
    return failed ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    if (!strcmp(mode, "rules")) return cmd_rules();
    if (!strcmp(mode, "effects")) return cmd_effects();
    fprintf(stderr, "usage: plan_rules_host rules|effects\n");
    return 2;
}
