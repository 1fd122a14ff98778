// extrema_host.cpp -- TEST-ONLY stand-alone host program for per-map extrema (fftconv_plan_set_extrema): the shared bodies of
// csrc/extrema.hpp (what the output kernel's fused store, the scan kernel and the fold kernel all compile), the route table of
// csrc/output_route.hpp with the new fields, the not-built lists of csrc/fast_paths.hpp and the refusals of csrc/plan_rules.hpp.
// Built by tests/test_extrema_host.py with the plain host compiler (and once more with -fsanitize=address,undefined).
//   fold      partials of a map in shuffled orders and groupings: always the lowest index among equals, +-0, NaN, all-NaN, the
//             empty sentinel, -inf / +inf maps, against a brute-force first-occurrence argmax / argmin
//   values    the 16-bit map values the scan reads back: every fp16 and bf16 bit pattern against the conversion written out here
//   index     the rectangle store's element walk (pairs of window rows, odd h_lo / rect_w_lo): every delivered element exactly once,
//             at its memory-order index
//   routes    fused or scan for every combination of (store family, format, stride, region, built, extrema_store, plan kind, sink),
//             and every pre-existing answer unchanged
//   rules     the refusals, from the table
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "extrema.hpp"
#include "fast_paths.hpp"
#include "output_route.hpp"
#include "plan_rules.hpp"

using namespace fc;

namespace {

int g_failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            if (g_failures++ < 20) {          \
                printf("FAIL ");              \
                printf(__VA_ARGS__);          \
                printf("\n");                 \
            }                                 \
        }                                     \
    } while (0)

uint32_t bits_of(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }

// NumPy's answer on the map in memory order: argmax / argmin return the first occurrence of the extreme value, and the FIRST NaN
// if there is one -- the records differ there on purpose (a NaN never wins), so the yardstick here skips NaNs
ExtremaRecord brute(const std::vector<float>& map, int out_h) {
    long imax = -1, imin = -1;
    for (size_t i = 0; i < map.size(); i++) {
        if (map[i] != map[i]) continue;
        if (imax < 0 || map[i] > map[imax]) imax = (long)i;
        if (imin < 0 || map[i] < map[imin]) imin = (long)i;
    }
    const float nan = std::numeric_limits<float>::quiet_NaN();
    ExtremaRecord r;
    r.max_value = imax < 0 ? nan : map[imax]; r.max_col = imax < 0 ? -1 : (int)(imax / out_h); r.max_row = imax < 0 ? -1 : (int)(imax % out_h);
    r.min_value = imin < 0 ? nan : map[imin]; r.min_col = imin < 0 ? -1 : (int)(imin / out_h); r.min_row = imin < 0 ? -1 : (int)(imin % out_h);
    return r;
}
bool same_record(const ExtremaRecord& a, const ExtremaRecord& b) {
    return bits_of(a.max_value) == bits_of(b.max_value) && a.max_row == b.max_row && a.max_col == b.max_col && bits_of(a.min_value) == bits_of(b.min_value) &&
           a.min_row == b.min_row && a.min_col == b.min_col;
}
bool same_record_nan(const ExtremaRecord& a, const ExtremaRecord& b) {      // (any NaN bits are a NaN)
    auto v = [](float x, float y) { return (x != x && y != y) || bits_of(x) == bits_of(y); };
    return v(a.max_value, b.max_value) && a.max_row == b.max_row && a.max_col == b.max_col && v(a.min_value, b.min_value) && a.min_row == b.min_row &&
           a.min_col == b.min_col;
}

// the map cut into `parts` partials by a random assignment of elements (what tiles, waves and lanes do), folded in a random order
// and a random grouping (what the wave reduction, the fold's strided loop and its tree do)
ExtremaRecord fold_shuffled(const std::vector<float>& map, int out_h, int parts, std::mt19937& rng) {
    std::vector<ExtremaPartial> p((size_t)parts, extrema_empty());      // (parts beyond the elements stay empty: the sentinel is folded too)
    std::vector<size_t> order(map.size());
    for (size_t i = 0; i < map.size(); i++) order[i] = i;
    std::shuffle(order.begin(), order.end(), rng);
    for (size_t i : order) extrema_take(p[rng() % (unsigned)parts], map[i], (int)i);
    while (p.size() > 1) {      // merge two random partials, either way round
        std::shuffle(p.begin(), p.end(), rng);
        const ExtremaPartial b = p.back();
        p.pop_back();
        ExtremaPartial& a = p[rng() % p.size()];
        a = (rng() & 1) ? extrema_merge(a, b) : extrema_merge(b, a);
    }
    return extrema_record(p[0], out_h);
}

int cmd_fold() {
    std::mt19937 rng(12345);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    struct Case { const char* name; std::vector<float> map; int out_h; };
    std::vector<Case> cases;
    {
        std::vector<float> m(7 * 13);
        for (float& x : m) x = (float)((int)(rng() % 9) - 4);      // few distinct values: ties everywhere
        cases.push_back({"ties among nine values", m, 7});
    }
    cases.push_back({"all equal", std::vector<float>(5 * 11, 2.5f), 5});
    cases.push_back({"all zero", std::vector<float>(6 * 6, 0.f), 6});
    {
        std::vector<float> m(4 * 9, 0.f);
        for (size_t i = 0; i < m.size(); i += 2) m[i] = -0.f;      // -0 first: max and min both report element 0, with its bits (-0)
        cases.push_back({"+-0 alternating, -0 first", m, 4});
        m[0] = 0.f;
        cases.push_back({"+-0 alternating, +0 first", m, 4});
    }
    {
        std::vector<float> m(8 * 5);
        for (size_t i = 0; i < m.size(); i++) m[i] = (i % 3 == 0) ? nan : (float)(i % 5);
        cases.push_back({"NaN elements", m, 8});
        m[0] = 7.f; m[1] = nan; m[2] = -7.f;
        cases.push_back({"NaN between the extremes", m, 8});
    }
    cases.push_back({"all NaN", std::vector<float>(3 * 7, nan), 3});
    cases.push_back({"all -inf", std::vector<float>(5 * 5, -inf), 5});
    cases.push_back({"all +inf", std::vector<float>(5 * 5, inf), 5});
    {
        std::vector<float> m(9 * 4, 1.f);
        m[17] = inf; m[23] = inf; m[5] = -inf; m[30] = -inf;
        cases.push_back({"planted +-inf twice", m, 9});
        m[2] = nan;
        cases.push_back({"planted +-inf and a NaN", m, 9});
    }
    cases.push_back({"one element", std::vector<float>(1, -3.f), 1});
    {
        std::vector<float> m(31 * 17);
        std::normal_distribution<float> d(0.f, 1.f);
        for (float& x : m) x = d(rng);
        cases.push_back({"random", m, 31});
    }
    int ok = 0;
    for (const Case& c : cases) {
        const ExtremaRecord want = brute(c.map, c.out_h);
        int bad = 0;
        for (int parts : {1, 2, 7, 64, 1000})
            for (int rep = 0; rep < 20; rep++) {
                const ExtremaRecord got = fold_shuffled(c.map, c.out_h, parts, rng);
                if (!same_record_nan(got, want)) bad++;
            }
        CHECK(!bad, "%s: %d of 100 shuffled folds differ from the first occurrence", c.name, bad);
        // what the issue states in words
        const std::string name = c.name;
        if (name == "all NaN") CHECK(want.max_row == -1 && want.max_col == -1 && want.min_row == -1 && want.min_col == -1 && want.max_value != want.max_value, "all NaN");
        if (name == "all zero" || name == "all equal" || name == "all -inf" || name == "all +inf")
            CHECK(want.max_row == 0 && want.max_col == 0 && want.min_row == 0 && want.min_col == 0 && bits_of(want.max_value) == bits_of(c.map[0]), "%s", c.name);
        if (name == "+-0 alternating, -0 first") {
            const ExtremaRecord got = fold_shuffled(c.map, c.out_h, 7, rng);
            CHECK(bits_of(got.max_value) == 0x80000000u && bits_of(got.min_value) == 0x80000000u && got.max_row == 0 && got.min_row == 0, "-0 first: element 0's bits");
        }
        if (name == "+-0 alternating, +0 first") {
            const ExtremaRecord got = fold_shuffled(c.map, c.out_h, 7, rng);
            CHECK(bits_of(got.max_value) == 0u && bits_of(got.min_value) == 0u && got.max_row == 0 && got.min_row == 0, "+0 first: element 0's bits");
        }
        if (name == "planted +-inf twice") CHECK(want.max_value == inf && want.max_col * c.out_h + want.max_row == 17 && want.min_value == -inf && want.min_col * c.out_h + want.min_row == 5, "planted inf");
        if (!bad) ok++;
    }
    // the empty sentinel: a partial nothing was taken into reports NaN, -1, -1 on both sides, and merging it changes nothing
    {
        const ExtremaRecord e = extrema_record(extrema_empty(), 5);
        CHECK(e.max_value != e.max_value && e.min_value != e.min_value && e.max_row == -1 && e.max_col == -1 && e.min_row == -1 && e.min_col == -1, "the empty record");
        ExtremaPartial p = extrema_empty();
        extrema_take(p, -inf, 3);      // an element equal to the sentinel's value still wins on its index
        CHECK(p.max_index == 3 && p.min_index == 3 && p.max_value == -inf, "-inf element against the sentinel");
        const ExtremaPartial q = extrema_merge(extrema_empty(), p), r = extrema_merge(p, extrema_empty());
        CHECK(!memcmp(&q, &p, sizeof p) && !memcmp(&r, &p, sizeof p), "merging the sentinel");
        ExtremaPartial n = extrema_empty();
        extrema_take(n, nan, 0);
        CHECK(n.max_index == FC_EXTREMA_NONE && n.min_index == FC_EXTREMA_NONE, "a NaN is never taken");
        static_assert(sizeof(ExtremaPartial) == 16 && sizeof(ExtremaRecord) == 24, "the layouts the kernels and the caller share");
    }
    printf("fold: %d of %zu maps agree in all 100 shuffled folds, %d failures\n", ok, cases.size(), g_failures);
    return g_failures ? 1 : 0;
}

// the conversions written out independently of extrema.hpp
float half_value(uint16_t h) {
    const int s = h >> 15, e = (h >> 10) & 31, m = h & 1023;
    double v;
    if (e == 31) v = m ? std::numeric_limits<double>::quiet_NaN() : std::numeric_limits<double>::infinity();
    else if (e == 0) v = std::ldexp((double)m, -24);
    else v = std::ldexp(1.0 + m / 1024.0, e - 15);
    return (float)(s ? -v : v);
}
int cmd_values() {
    long bad = 0;
    for (uint32_t b = 0; b < 65536; b++) {
        const float got = extrema_map16_value((uint16_t)b, false), want = half_value((uint16_t)b);
        if (want != want ? got == got : bits_of(got) != bits_of(want)) bad++;
        const float gb = extrema_map16_value((uint16_t)b, true);
        if (bits_of(gb) != (b << 16)) bad++;
    }
    CHECK(!bad, "%ld of 2 x 65536 16-bit values differ", bad);
    // ... and back: what the store rounds to is what the scan reads (fc_common.hpp: fc_map16)
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> d(-70000.f, 70000.f);
    long back = 0;
    for (int i = 0; i < 100000; i++) {
        const float x = d(rng);
        for (int bf = 0; bf < 2; bf++) {
            const uint16_t h = fc_map16(x, bf != 0);
            const float v = extrema_map16_value(h, bf != 0);
            if (fc_map16(v, bf != 0) != h) back++;
        }
    }
    CHECK(!back, "%ld values do not survive store -> read -> store", back);
    printf("values: 131072 bit patterns, 200000 round trips, %d failures\n", g_failures);
    return g_failures ? 1 : 0;
}

// the element walk of the RECT stores (fast_cols.hpp, C4): per window column of the rectangle the complex values n hold window rows
// 2n, 2n + 1; hr = 2n - h_lo; the pair is looked at while (unsigned)(hr + 1) <= nrows, row hr is stored if hr >= 0, row hr + 1 if it
// is < nrows -- with the indices the store takes into its running extrema
int cmd_index() {
    struct Rect { int h_lo, w_lo, out_h, out_w; };
    const Rect rects[] = {{3, 5, 2 * 144 - 17 - 3, 271 - 5}, {0, 0, 288, 288}, {1, 1, 1, 1}, {7, 16, 5, 17}, {2, 3, 10, 1}, {287, 287, 1, 1}, {0, 15, 287, 2}};
    const int M = 144, T = 16, fft_w = 288;
    std::mt19937 rng(99);
    int ok = 0;
    for (const Rect& r : rects) {
        const int nrows = r.out_h;
        std::vector<int> seen((size_t)r.out_h * r.out_w, 0);
        std::vector<float> map((size_t)r.out_h * r.out_w);
        for (float& x : map) x = (float)((int)(rng() % 21) - 10);
        ExtremaPartial ex = extrema_empty();
        long outside = 0;
        for (int w0 = (r.w_lo / T) * T; w0 < fft_w; w0 += T)
            for (int col = 0; col < T; col++) {
                if (!((unsigned)(w0 + col - r.w_lo) < (unsigned)r.out_w)) continue;
                for (int n = 0; n < M; n++) {
                    const int hr = 2 * n - r.h_lo;
                    if (!((unsigned)(hr + 1) <= (unsigned)nrows)) continue;
                    const int e0 = extrema_rect_index(w0 + col, 2 * n, r.w_lo, r.h_lo, r.out_h);
                    if (hr >= 0) {
                        if (e0 < 0 || (size_t)e0 >= map.size()) outside++;
                        else { seen[e0]++; extrema_take(ex, map[e0], e0); }
                    }
                    if ((unsigned)(hr + 1) < (unsigned)nrows) {
                        if (e0 + 1 < 0 || (size_t)(e0 + 1) >= map.size()) outside++;
                        else { seen[e0 + 1]++; extrema_take(ex, map[e0 + 1], e0 + 1); }
                    }
                }
            }
        long not_once = 0;
        for (int s : seen) not_once += s != 1;
        // the index is the memory-order one: element (row, col) of the dense map at col * out_h + row
        long wrong = 0;
        for (int w = r.w_lo; w < r.w_lo + r.out_w; w++)
            for (int h = r.h_lo; h < r.h_lo + r.out_h; h++)
                wrong += extrema_rect_index(w, h, r.w_lo, r.h_lo, r.out_h) != (w - r.w_lo) * r.out_h + (h - r.h_lo);
        const bool same = same_record(extrema_record(ex, r.out_h), brute(map, r.out_h));
        CHECK(!outside && !not_once && !wrong && same, "rectangle (%d, %d, %d, %d): %ld indices outside, %ld elements not taken exactly once, %ld wrong, record %s", r.h_lo,
              r.w_lo, r.out_h, r.out_w, outside, not_once, wrong, same ? "equal" : "differs");
        ok += !outside && !not_once && !wrong && same;
    }
    printf("index: %d of %zu rectangles walked exactly once at their memory-order indices, %d failures\n", ok, sizeof(rects) / sizeof(rects[0]), g_failures);
    return g_failures ? 1 : 0;
}

// every answer but `extrema`, and -- where the whole window's Plain store became Rect for the fused extrema -- but what follows from a
// dense store (store, staging of a staged route, target)
bool same_but_extrema(const OutputRoute& a, const OutputRoute& b, bool dense_swap) {
    bool same = ((a.error == nullptr) == (b.error == nullptr)) && a.route == b.route && a.plane == b.plane && a.kernel_format == b.kernel_format &&
                a.map_format == b.map_format && a.extent == b.extent && a.after == b.after && a.need_O == b.need_O && a.staging_copies == b.staging_copies &&
                a.pinned_one_map == b.pinned_one_map && a.probe == b.probe;
    if (!dense_swap) return same && a.store == b.store && a.target == b.target && a.staging == b.staging;
    return same && a.store == OutStore::Plain && b.store == OutStore::Rect && b.staging == (b.staged() ? OutBuffer::OC : OutBuffer::Caller) && b.target == b.staging;
}

int cmd_routes() {
    long combos = 0, off_same = 0, fused = 0, scanned = 0, wrong = 0, swapped = 0;
    const SinkKind sinks[] = {SinkKind::Packed, SinkKind::DevicePtrs, SinkKind::Host, SinkKind::Window};
    struct Kind { bool fast_cols, y_tiled, blockwise; };
    const Kind kinds[] = {{true, true, false}, {true, false, false}, {false, false, false}, {true, true, true}};
    struct Stride { int sh, sw; };
    const Stride strides[] = {{1, 1}, {2, 3}};
    for (SinkKind sink : sinks)
    for (long host_stream = 0; host_stream <= 2; host_stream += 2)
    for (size_t map_bytes : {(size_t)4096, (size_t)8 << 20})
    for (long region = 0; region <= 5; region++)
    for (long score = 0; score <= 4; score++)
    for (int format = FC_MAP_F32; format <= FC_MAP_BF16; format++)
    for (const Stride& st : strides)
    for (int stores_on = 0; stores_on <= 1; stores_on++)      // rect_store, norm_store, stride_store together
    for (int built = 0; built < 8; built++)                   // bit 0 RECT, 1 SCALE, 2 ADD: the EXT kernels
    for (int extrema_store = 0; extrema_store <= 1; extrema_store++)
    for (const Kind& k : kinds) {
        if (region == 4 && st.sh != 1) continue;
        OutputRouteIn in;
        in.sink = sink; in.map_bytes = map_bytes; in.host_stream = host_stream; in.host_min_kb = 1024; in.host_pinned = true;
        in.region = region; in.rect_store = stores_on != 0; in.score = score; in.norm_store = stores_on != 0; in.blockwise = k.blockwise;
        in.map_format = format; in.fast_cols = k.fast_cols; in.y_tiled = k.y_tiled;
        in.rect_built = in.norm_built = in.sqdiff_built = in.stride_built = true;
        in.stride_h = st.sh; in.stride_w = st.sw; in.stride_store = stores_on != 0;
        const OutputRoute before = plan_output_route(in);      // the record as it was: the new fields at their defaults
        OutputRouteIn off = in;
        off.extrema_store = extrema_store != 0; off.extrema_rect_built = built & 1; off.extrema_norm_built = (built & 2) != 0; off.extrema_sqdiff_built = (built & 4) != 0;
        const OutputRoute r_off = plan_output_route(off);
        combos++;
        if (same_but_extrema(before, r_off, false) && r_off.extrema == OutExtrema::Off) off_same++;
        OutputRouteIn on = off;
        on.extrema = true;
        const OutputRoute r = plan_output_route(on);
        if (sink == SinkKind::Window) {      // (refused by the rule table ahead of the route; the route itself answers Off)
            if (r.extrema != OutExtrema::Off || !same_but_extrema(before, r, false)) wrong++;
            continue;
        }
        // the store family the group would take without extrema, and whether its EXT kernel serves it
        const bool fp32 = format == FC_MAP_F32, one_pass_tiled = k.fast_cols && k.y_tiled && !k.blockwise, unit = st.sh == 1 && st.sw == 1;
        bool want = false, swap = false;
        if (extrema_store && fp32 && one_pass_tiled && unit && (region == 0 || region == 5)) {
            const bool plane = score == 1 || score == 3 || score == 4;
            if (plane) want = stores_on && (score == 4 ? (built & 4) != 0 : (built & 2) != 0);
            else if (region == 5) want = stores_on && (built & 1);
            else { want = (built & 1) != 0; swap = want; }      // the whole window: Rect stands in, whatever "rect_store" says
        }
        bool ok = r.extrema == (want ? OutExtrema::Fused : OutExtrema::Scan) && same_but_extrema(before, r, swap);
        if (want) ok = ok && (r.store == OutStore::Rect || r.fused()) && r.after == OutAfter::None && r.kernel_format == FC_MAP_F32;
        fused += want; scanned += !want; swapped += swap;
        if (!ok && !wrong++)
            printf("FAIL first wrong route: sink %d region %ld score %ld format %d stride (%d, %d) stores %d built %d extrema_store %d kind (%d, %d, %d): extrema %d store %d (before %d)\n",
                   (int)sink, region, score, format, st.sh, st.sw, stores_on, built, extrema_store, k.fast_cols, k.y_tiled, k.blockwise, (int)r.extrema, (int)r.store, (int)before.store);
    }
    printf("routes: %ld combinations, %ld unchanged with extrema off, %ld fused (%ld with the window standing in for a rectangle), %ld scanned, %ld wrong\n", combos,
           off_same, fused, swapped, scanned, wrong);
    // the lists of fast_paths.hpp: an EXT kernel exists only where its sibling does
    int lists_bad = 0;
#define FC_X(MM, A, B, C, TT, NTT)                                                                                              \
    lists_bad += (fast_cols_rect_ext_built(MM) && !fast_cols_rect_built(MM)) || (fast_cols_norm_ext_built(MM) && !fast_cols_norm_built(MM)) || \
                 (fast_cols_sqdiff_ext_built(MM) && !fast_cols_sqdiff_built(MM)) || (fast_cols_rect_ext_built(MM) && NTT % 64 != 0);
    FC_FAST_COL_CONFIGS(FC_X)
#undef FC_X
    printf("lists: %d inconsistent\n", lists_bad);
    return wrong || off_same != combos || !fused || !scanned || !swapped || lists_bad ? 1 : 0;
}

int cmd_rules() {
    char msg[512];
    int rows = 0;
    for (int blocks : {0, 1, 12})
        for (long mode : {0L, 1L})
            for (int window : {0, 1}) {
                PlanRuleState s;
                s.blocks = blocks; s.window_sink = window != 0;
                const OutputRefusal a = plan_refusal(s, AskOutput::Extrema, mode);
                const bool want_a = blocks > 0 && mode == 1;      // (switching it off always passes)
                CHECK((bool)a == want_a, "set_extrema(%ld) on %d blocks: %s", mode, blocks, a ? "refused" : "passes");
                if (a) {
                    snprintf(msg, sizeof msg, a.rule->fmt, a.arg);
                    CHECK(a.rule->code == FFTCONV_ERR_INVALID_ARG && a.arg == blocks && strstr(msg, "block-wise") && a.rule == &kOutputRules[0], "the block-wise row: %s", msg);
                    printf("refusal | extrema on %d blocks | %s\n", blocks, msg);
                    rows++;
                }
                const OutputRefusal g = plan_refusal(s, AskOutput::ExtremaGroup, 1);
                CHECK((bool)g == (window != 0), "a group into %s", window ? "a window" : "maps");
                if (g) {
                    snprintf(msg, sizeof msg, g.rule->fmt, g.arg);
                    CHECK(g.rule->code == FFTCONV_ERR_INVALID_ARG && strstr(msg, "output window") && g.rule == &kOutputRules[1], "the window row: %s", msg);
                }
            }
    const AddedSetterEffects& e = setter_effects(SetterAdded::Extrema);
    CHECK(e.setter == SetterAdded::Extrema && e.changed == FX_WAIT && e.unchanged_returns, "the effects row: output-side state alone, early return");
    CHECK(sizeof(kOutputRules) / sizeof(kOutputRules[0]) == 2 && sizeof(kSetterEffectsAdded) / sizeof(kSetterEffectsAdded[0]) == 1, "the added tables' rows");
    printf("rules: %d refusals printed, %d failures\n", rows, g_failures);
    return g_failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "fold") return cmd_fold();
    if (mode == "values") return cmd_values();
    if (mode == "index") return cmd_index();
    if (mode == "routes") return cmd_routes();
    if (mode == "rules") return cmd_rules();
    if (mode == "all") return (cmd_fold() | cmd_values() | cmd_index() | cmd_routes() | cmd_rules()) ? 1 : 0;
    fprintf(stderr, "usage: %s fold | values | index | routes | rules | all\n", argv[0]);
    return 2;
}
