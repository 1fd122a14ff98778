// peaks_host.cpp -- TEST-ONLY stand-alone host program for peak lists (fftconv_plan_set_peaks): the shared bodies of csrc/peaks.hpp
// (what the kernels of csrc/kernels_peaks.hip compile) and the refusals of csrc/plan_rules.hpp.
// Built by tests/test_peaks_host.py with the plain host compiler (and once more with -fsanitize=address,undefined).
//   rule      crafted maps against a brute-force restatement of the rule: ties, plateaus, +-0, NaN, +-inf, 1 x 1, 1 x n, radii beyond the
//             map, mode 2 against mode 1 on the negated map
//   cut       a map that starts off a 16-byte address cut into 1, 2, 7, 64 and 1000 units, walked as a wave walks a unit (64 lanes, the
//             slots of a vector, ballots, ranks), counts scanned, lists assembled: the ascending-index list and the total, for
//             max_peaks below, at and above the count
//   rank      the rank of a flagged element within a step against a serial count
//   subpixel  the fit: a sampled parabola's vertex, the cases that give 0, the clamp
//   values16  16-bit elements go through extrema_map16_value
//   rules     the refusals and the effects, from the tables
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "peaks.hpp"
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
const float INF = std::numeric_limits<float>::infinity();
const float QNAN = std::numeric_limits<float>::quiet_NaN();

struct Peak { long index; float value; };

// the rule restated without the header: mode 1 on `map` (out_h rows per column, memory order)
std::vector<Peak> brute(const std::vector<float>& map, int out_h, float threshold, long rh, long rw) {
    const long H = out_h, W = (long)map.size() / out_h;
    std::vector<Peak> out;
    for (long c = 0; c < W; c++)
        for (long r = 0; r < H; r++) {
            const long i = c * H + r;
            const float v = map[i];
            if (!(v >= threshold)) continue;
            bool beaten = false;
            for (long cc = std::max(0L, c - rw); cc <= std::min(W - 1, c + rw) && !beaten; cc++)
                for (long rr = std::max(0L, r - rh); rr <= std::min(H - 1, r + rh) && !beaten; rr++) {
                    const long j = cc * H + rr;
                    if (j == i) continue;
                    if (map[j] > v || (map[j] == v && j < i)) beaten = true;
                }
            if (!beaten) out.push_back({i, v});
        }
    return out;
}

// the header's answer, element by element
std::vector<Peak> by_header(const std::vector<float>& map, int out_h, int mode, float threshold, int rh, int rw) {
    const int W = (int)(map.size() / out_h);
    const PeakRule k = peak_rule(mode, threshold, rh, rw);
    auto U = [&](int j) { return peak_signed(k, map[j]); };
    std::vector<Peak> out;
    for (int i = 0; i < (int)map.size(); i++)
        if (peak_test(U, out_h, W, i, U(i), k)) out.push_back({i, map[i]});
    return out;
}

bool same_list(const std::vector<Peak>& a, const std::vector<Peak>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].index != b[i].index || bits_of(a[i].value) != bits_of(b[i].value)) return false;
    return true;
}

struct Crafted { std::string name; int out_h; std::vector<float> map; };
std::vector<Crafted> crafted_maps() {
    std::mt19937 rng(1234);
    std::vector<Crafted> ms;
    auto fill = [&](const char* name, int h, int w, auto&& f) {
        Crafted c{name, h, std::vector<float>((size_t)h * w)};
        for (size_t i = 0; i < c.map.size(); i++) c.map[i] = f(i);
        ms.push_back(c);
    };
    std::uniform_int_distribution<int> few(0, 3);
    std::normal_distribution<float> gauss(0.0f, 1.0f);
    fill("ties among few values", 13, 11, [&](size_t) { return (float)few(rng); });
    fill("all equal", 9, 7, [&](size_t) { return 2.5f; });
    fill("all zero", 8, 8, [&](size_t) { return 0.0f; });
    fill("+-0 alternating, +0 first", 7, 9, [&](size_t i) { return i % 2 ? -0.0f : 0.0f; });
    fill("+-0 alternating, -0 first", 7, 9, [&](size_t i) { return i % 2 ? 0.0f : -0.0f; });
    fill("NaN elements", 12, 10, [&](size_t i) { return i % 5 == 2 ? QNAN : gauss(rng); });
    fill("all NaN", 6, 5, [&](size_t) { return QNAN; });
    fill("+inf planted twice", 11, 12, [&](size_t i) { return i == 17 || i == 95 ? INF : gauss(rng); });
    fill("-inf planted twice", 11, 12, [&](size_t i) { return i == 17 || i == 95 ? -INF : gauss(rng); });
    fill("all -inf", 5, 4, [&](size_t) { return -INF; });
    fill("1 x 1", 1, 1, [&](size_t) { return 3.0f; });
    fill("1 x n", 1, 17, [&](size_t) { return (float)few(rng); });
    fill("n x 1", 17, 1, [&](size_t) { return (float)few(rng); });
    fill("random", 31, 29, [&](size_t) { return gauss(rng); });
    return ms;
}
const int kRadii[][2] = {{0, 0}, {1, 1}, {3, 3}, {1, 5}, {0, 2}, {2, 0}, {100, 100}, {0x7fffffff, 0x7fffffff}};
const float kThresholds[] = {-INF, -1.0f, 0.0f, 0.5f, 2.5f, INF};

void mode_rule() {
    const std::vector<Crafted> ms = crafted_maps();
    int agree = 0, cases = 0;
    for (const Crafted& c : ms) {
        bool ok = true;
        std::vector<float> neg(c.map.size());
        for (size_t i = 0; i < neg.size(); i++) neg[i] = -c.map[i];
        for (const auto& rad : kRadii)
            for (float thr : kThresholds) {
                cases++;
                const std::vector<Peak> want = brute(c.map, c.out_h, thr, rad[0], rad[1]);
                const std::vector<Peak> got = by_header(c.map, c.out_h, FC_PEAKS_MAX, thr, rad[0], rad[1]);
                if (!same_list(want, got)) { ok = false; CHECK(false, "%s radius (%d, %d) threshold %g: %zu peaks, brute force %zu", c.name.c_str(), rad[0], rad[1], thr, got.size(), want.size()); }
                // mode 2 on the map = mode 1 on the negated map with the negated threshold: the same indices, the element's own value
                const std::vector<Peak> min2 = by_header(neg, c.out_h, FC_PEAKS_MIN, -thr, rad[0], rad[1]);
                bool same = min2.size() == want.size();
                for (size_t i = 0; same && i < want.size(); i++) same = min2[i].index == want[i].index && bits_of(min2[i].value) == bits_of(-want[i].value);
                if (!same) { ok = false; CHECK(false, "%s radius (%d, %d): mode 2 on the negated map differs", c.name.c_str(), rad[0], rad[1]); }
            }
        agree += ok;
    }
    // the statements of the contract, one by one
    const Crafted& eq = ms[1];
    CHECK(by_header(eq.map, eq.out_h, 1, 2.5f, 1, 1).size() == 1 && by_header(eq.map, eq.out_h, 1, 2.5f, 1, 1)[0].index == 0, "all equal, radius 1: one peak at index 0");
    CHECK(by_header(eq.map, eq.out_h, 1, 2.5f, 0, 0).size() == eq.map.size(), "all equal, radius 0: every element");
    CHECK(by_header(eq.map, eq.out_h, 1, 2.6f, 0, 0).empty(), "all equal below the threshold: none");
    CHECK(by_header(ms[3].map, ms[3].out_h, 1, 0.0f, 1, 1).size() == 1 && by_header(ms[4].map, ms[4].out_h, 1, 0.0f, 1, 1)[0].index == 0, "+-0 compare equal: index 0");
    CHECK(bits_of(by_header(ms[4].map, ms[4].out_h, 1, 0.0f, 1, 1)[0].value) == 0x80000000u, "the value is the element's bits (-0)");
    CHECK(by_header(ms[6].map, ms[6].out_h, 1, -INF, 0, 0).empty() && by_header(ms[6].map, ms[6].out_h, 2, INF, 3, 3).empty(), "all NaN: no peak");
    CHECK(by_header(ms[9].map, ms[9].out_h, 1, -INF, 0, 0).size() == ms[9].map.size(), "-inf elements meet a threshold of -inf");
    CHECK(by_header(ms[10].map, 1, 1, 3.0f, 5, 5).size() == 1, "1 x 1");
    printf("rule: %d of %zu maps agree with the brute force in all %d cases (radius x threshold, both modes), %d failures\n", agree, ms.size(), cases / (int)ms.size(), g_failures);
}

// ---- a map as the kernels see it: walked by units, 64 lanes a step, the slots of a vector ----
template <class E>
struct Walk {
    const E* map;
    size_t n;
    int out_h, out_w;
    bool bf16;
    PeakRule k;
    int units;
    float val(E e) const {
        if constexpr (sizeof(E) == 4) return e;
        else return extrema_map16_value(e, bf16);
    }
    // unit u as k_peaks_count (out == nullptr) or k_peaks_write walks it
    int unit(int u, int base, int max_peaks, PeakRecord* out) const {
        constexpr int EPV = 16 / sizeof(E);
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(map);
        const PeakCut cut = peaks_cut(a0, n * sizeof(E), units);
        size_t lo, hi;
        peaks_unit_range(cut, u, lo, hi);
        auto V = [&](int j) { return val(map[j]); };
        auto U = [&](int j) { return peak_signed(k, val(map[j])); };
        int count = 0;
        for (size_t b = lo; b < hi; b += FC_PEAKS_LANES) {
            bool flag[FC_PEAKS_LANES][EPV];
            uint64_t flags[EPV] = {};
            for (int lane = 0; lane < FC_PEAKS_LANES; lane++) {
                const size_t v = b + lane;
                const long e0 = peaks_vector_element(cut, v, a0, sizeof(E));
                for (int i = 0; i < EPV; i++) {
                    const long ei = e0 + i;
                    const bool valid = v < hi && ei >= 0 && (size_t)ei < n;
                    flag[lane][i] = valid && peak_test(U, out_h, out_w, (int)ei, U((int)(valid ? ei : 0)), k);
                    if (flag[lane][i]) flags[i] |= (uint64_t)1 << lane;
                }
            }
            if (out)
                for (int lane = 0; lane < FC_PEAKS_LANES; lane++)
                    for (int i = 0; i < EPV; i++)
                        if (flag[lane][i]) {
                            const int slot = base + count + peaks_rank(flags, EPV, lane, i);
                            const long ei = peaks_vector_element(cut, b + lane, a0, sizeof(E)) + i;
                            if (slot < max_peaks) out[slot] = peak_record(V, out_h, out_w, (int)ei, k);
                        }
            count += peaks_step_total(flags, EPV);
        }
        return count;
    }
    // count, scan, write: found, and the first min(found, max_peaks) records
    int lists(int max_peaks, std::vector<PeakRecord>& out) const {
        std::vector<int> counts(units), offsets(units);
        for (int u = 0; u < units; u++) counts[u] = unit(u, 0, 0, nullptr);
        int found = 0;
        for (int u = 0; u < units; u++) { offsets[u] = found; found += counts[u]; }
        PeakRecord none;
        memset(&none, 0xee, sizeof(none));
        out.assign(max_peaks, none);
        for (int u = 0; u < units; u++)
            if (counts[u] && offsets[u] < max_peaks) CHECK(unit(u, offsets[u], max_peaks, out.data()) == counts[u], "a unit counts the same twice");
        return found;
    }
};

void mode_cut() {
    std::mt19937 rng(99);
    std::normal_distribution<float> gauss(0.0f, 1.0f);
    const int units_list[] = {1, 2, 7, 64, 1000};
    int walks = 0, good = 0;
    for (int off : {1, 3, 0, 2})
        for (const auto& hw : {std::pair<int, int>{37, 41}, {1, 263}, {129, 3}, {1, 1}}) {
            const int H = hw.first, W = hw.second;
            const size_t n = (size_t)H * W;
            std::vector<float> store(n + 16);
            // a 16-byte address inside the store, then `off` elements on: the map starts 4 * off bytes past a vector boundary
            const uintptr_t s0 = (reinterpret_cast<uintptr_t>(store.data()) + 15) / 16 * 16;
            float* map = reinterpret_cast<float*>(s0) + off;
            std::vector<float> m(n);
            for (size_t i = 0; i < n; i++) m[i] = map[i] = std::round(gauss(rng) * 4.0f) / 4.0f;      // (quantised: ties occur)
            for (const auto& rad : {std::pair<int, int>{0, 0}, {2, 2}, {1, 3}})
                for (float thr : {-INF, 0.5f}) {
                    const std::vector<Peak> want = brute(m, H, thr, rad.first, rad.second);
                    const int cnt = (int)want.size();
                    for (int units : units_list)
                        for (int max_peaks : {std::max(cnt / 2, 1), std::max(cnt, 1), cnt + 5}) {
                            Walk<float> w{map, n, H, W, false, peak_rule(FC_PEAKS_MAX, thr, rad.first, rad.second), units};
                            std::vector<PeakRecord> got;
                            const int found = w.lists(max_peaks, got);
                            bool ok = found == cnt;
                            for (int i = 0; ok && i < std::min(cnt, max_peaks); i++)
                                ok = (long)got[i].col * H + got[i].row == want[i].index && bits_of(got[i].value) == bits_of(want[i].value);
                            for (int i = cnt; ok && i < max_peaks; i++) ok = bits_of(got[i].value) == 0xeeeeeeeeu;      // (nothing beyond the list is written)
                            walks++; good += ok;
                            CHECK(ok, "cut: %d x %d at offset %d, %d units, max_peaks %d: found %d, brute force %d", H, W, off, units, max_peaks, found, cnt);
                        }
                }
        }
    // the units cover every vector once, in order, for sizes around the bounds
    for (size_t bytes : {(size_t)4, (size_t)16, (size_t)16385, (size_t)331776, (size_t)71000000, (size_t)1 << 31})
        for (uintptr_t addr : {(uintptr_t)4096, (uintptr_t)4100, (uintptr_t)4110}) {
            const int units = peaks_units(bytes);
            const PeakCut cut = peaks_cut(addr, bytes, units);
            size_t next = 0;
            for (int u = 0; u < units; u++) {
                size_t lo, hi;
                peaks_unit_range(cut, u, lo, hi);
                CHECK(lo == next && hi >= lo, "units are laid end to end");
                next = hi;
            }
            CHECK(next == cut.nv && units >= 1 && units <= FC_PEAKS_MAX_UNITS && cut.v0 * 16 <= addr && (cut.v0 + cut.nv) * 16 >= addr + bytes, "the units cover the map");
        }
    printf("cut: %d of %d walks give the ascending-index list and the total, %d failures\n", good, walks, g_failures);
}

void mode_rank() {
    std::mt19937_64 rng(7);
    int sets = 0;
    for (int nslots : {4, 8})
        for (int rep = 0; rep < 400; rep++) {
            uint64_t flags[8];
            for (int s = 0; s < nslots; s++) {
                uint64_t f = rng();
                if (rep % 4 == 1) f &= rng() & rng();      // sparse
                if (rep % 4 == 2) f = 0;
                if (rep % 4 == 3) f = ~(uint64_t)0;
                flags[s] = f;
            }
            int serial = 0;
            bool ok = true;
            for (int lane = 0; lane < 64; lane++)
                for (int s = 0; s < nslots; s++) {
                    if (flags[s] >> lane & 1) ok = ok && peaks_rank(flags, nslots, lane, s) == serial++;
                }
            ok = ok && peaks_step_total(flags, nslots) == serial;
            CHECK(ok, "rank: %d slots, set %d", nslots, rep);
            sets++;
        }
    printf("rank: %d flag sets, every rank the serial count, %d failures\n", sets, g_failures);
}

void mode_subpixel() {
    std::mt19937 rng(5);
    std::uniform_real_distribution<double> vertex(-0.5, 0.5), curve(0.2, 4.0), height(-3.0, 3.0);
    int n = 0;
    double worst = 0;
    for (int i = 0; i < 20000; i++) {
        // y = h - k (x - x0)^2 sampled at -1, 0, 1, in float64 rounded to fp32: the fit recovers x0 to the rounding of the samples
        const double x0 = vertex(rng), k = curve(rng), h = height(rng);
        const float a = (float)(h - k * (-1 - x0) * (-1 - x0)), v = (float)(h - k * x0 * x0), b = (float)(h - k * (1 - x0) * (1 - x0));
        const float d = peak_fit(a, v, b);
        worst = std::max(worst, std::fabs((double)d - x0));
        CHECK(std::fabs(d) <= 0.5f, "the clamp");
        CHECK(peak_fit(-a, -v, -b) == d, "the fit of the negated values is the same (mode 2)");
        n++;
    }
    // (samples of magnitude up to 12 carry 4.8e-7 each; |den| = 2k >= 0.4: (da + db) / (2 |den|) + |d| (da + db + 2 dv) / |den| < 4e-6)
    CHECK(worst < 1e-5, "a sampled parabola returns its vertex (worst %g)", worst);
    CHECK(peak_fit(1.0f, 2.0f, 1.0f) == 0.0f && peak_fit(0.0f, 3.0f, 2.0f) == 0.25f && peak_fit(2.0f, 3.0f, 0.0f) == -0.25f, "by hand");
    CHECK(peak_fit(2.0f, 2.0f, 2.0f) == 0.0f && peak_fit(1.0f, 2.0f, 3.0f) == 0.0f, "den == 0");
    CHECK(peak_fit(QNAN, 2.0f, 1.0f) == 0.0f && peak_fit(1.0f, INF, 1.0f) == 0.0f && peak_fit(1.0f, 2.0f, -INF) == 0.0f, "not finite");
    CHECK(peak_fit(2.0f, 2.0f, 0.0f) == -0.5f && peak_fit(0.0f, 2.0f, 2.0f) == 0.5f, "a tie with a neighbour: half a pixel");
    CHECK(peak_fit(3.0f, 2.0f, 0.0f) == -0.5f && peak_fit(5.0f, 0.0f, -1.0f) == 0.5f, "clamped (not a peak of the three)");
    // the record: edges and radius 0 give 0
    const int H = 5, W = 4;
    std::vector<float> m((size_t)H * W);
    for (size_t i = 0; i < m.size(); i++) m[i] = (float)((i * 7) % 11);
    auto V = [&](int j) { return m[j]; };
    for (int i = 0; i < H * W; i++) {
        const int c = i / H, r = i % H;
        const PeakRecord full = peak_record(V, H, W, i, peak_rule(1, 0, 2, 2)), rows = peak_record(V, H, W, i, peak_rule(1, 0, 1, 0)), none = peak_record(V, H, W, i, peak_rule(1, 0, 0, 0));
        CHECK(full.row == r && full.col == c && full.value == m[i], "the record's position and value");
        CHECK((r > 0 && r < H - 1) || full.d_row == 0.0f, "a row edge");
        CHECK((c > 0 && c < W - 1) || full.d_col == 0.0f, "a column edge");
        if (r > 0 && r < H - 1) CHECK(full.d_row == peak_fit(m[i - 1], m[i], m[i + 1]), "rows: the neighbours are i - 1 and i + 1");
        if (c > 0 && c < W - 1) CHECK(full.d_col == peak_fit(m[i - H], m[i], m[i + H]), "columns: i - out_h and i + out_h");
        CHECK(rows.d_col == 0.0f && rows.d_row == full.d_row && none.d_row == 0.0f && none.d_col == 0.0f, "a radius of 0 gives 0");
    }
    CHECK(sizeof(PeakRecord) == 20, "the record is 20 bytes");
    printf("subpixel: %d parabolas within %.2g of their vertex, edges, non-finite values and den == 0 give 0, %d failures\n", n, worst, g_failures);
}

void mode_values16() {
    // a 16-bit map (fp16 and bf16 bit patterns) walked as the kernels walk it, against the brute force on its fp32 values
    std::mt19937 rng(3);
    int maps = 0;
    for (bool bf16 : {false, true}) {
        const int H = 45, W = 37;
        const size_t n = (size_t)H * W;
        std::vector<uint16_t> store(n + 16);
        const uintptr_t s0 = (reinterpret_cast<uintptr_t>(store.data()) + 15) / 16 * 16;
        uint16_t* map = reinterpret_cast<uint16_t*>(s0) + 3;      // 6 bytes past a vector boundary
        std::vector<float> m(n);
        for (size_t i = 0; i < n; i++) {
            uint16_t bits = (uint16_t)rng();
            if (i % 3) bits = (uint16_t)((bf16 ? 0x3f80 : 0x3c00) + (rng() % 64) * (rng() % 2 ? 1 : 0) + (rng() % 2 ? 0x8000 : 0));      // near +-1: ties
            map[i] = bits;
            m[i] = extrema_map16_value(bits, bf16);
        }
        for (int units : {1, 7, 64}) {
            const std::vector<Peak> want = brute(m, H, 0.5f, 2, 1);
            Walk<uint16_t> w{map, n, H, W, bf16, peak_rule(FC_PEAKS_MAX, 0.5f, 2, 1), units};
            std::vector<PeakRecord> got;
            const int found = w.lists((int)want.size() + 1, got);
            bool ok = found == (int)want.size() && found > 3;
            for (int i = 0; ok && i < found; i++) ok = (long)got[i].col * H + got[i].row == want[i].index && bits_of(got[i].value) == bits_of(want[i].value);
            CHECK(ok, "values16: %s, %d units: found %d, brute force %zu", bf16 ? "bf16" : "fp16", units, found, want.size());
            maps++;
        }
    }
    CHECK(extrema_map16_value(0x3c00, false) == 1.0f && extrema_map16_value(0x3f80, true) == 1.0f && extrema_map16_value(0x0001, false) == 5.9604644775390625e-08f, "spot values");
    printf("values16: %d walks of 16-bit maps agree with the brute force on their fp32 values, %d failures\n", maps, g_failures);
}

void mode_rules() {
    for (int blocks : {0, 12})
        for (int mode = 0; mode <= 2; mode++) {
            PlanRuleState s;
            s.blocks = blocks;
            const PeaksRefusal a = plan_refusal(s, AskPeaks::Peaks, mode);
            CHECK((bool)a == (blocks > 0 && mode != 0), "peaks on a block-wise plan: refused exactly when switched on");
            if (a) {
                char msg[512];
                snprintf(msg, sizeof msg, a.rule->fmt, a.arg);
                CHECK(a.rule->code == FFTCONV_ERR_INVALID_ARG && a.arg == blocks && a.rule == &kPeaksRules[0], "the block-wise row");
                printf("refusal | peaks mode %d on %d blocks | %s\n", mode, blocks, msg);
            }
            for (bool window : {false, true}) {
                s.window_sink = window;
                const PeaksRefusal g = plan_refusal(s, AskPeaks::PeaksGroup, 1);
                CHECK((bool)g == window, "a group under peaks: refused exactly for a window sink");
                if (g && blocks == 0 && mode == 0) {
                    char msg[512];
                    snprintf(msg, sizeof msg, g.rule->fmt, g.arg);
                    CHECK(g.rule == &kPeaksRules[1] && g.rule->code == FFTCONV_ERR_INVALID_ARG, "the window row");
                    printf("refusal | a window sink under peaks | %s\n", msg);
                }
            }
        }
    const PeaksSetterEffects& e = setter_effects(SetterPeaks::Peaks);
    const AddedSetterEffects& x = setter_effects(SetterAdded::Extrema);
    CHECK(e.setter == SetterPeaks::Peaks && e.changed == x.changed && e.unchanged_returns == x.unchanged_returns, "the effects the extrema setter has");
    CHECK(sizeof(kPeaksRules) / sizeof(kPeaksRules[0]) == 2 && sizeof(kSetterEffectsPeaks) / sizeof(kSetterEffectsPeaks[0]) == 1, "the peaks tables' rows");
    printf("rules: the peaks rows refuse a block-wise plan and a window sink, effects as the extrema setter's, %d failures\n", g_failures);
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "all";
    const bool all = mode == "all";
    if (all || mode == "rule") mode_rule();
    if (all || mode == "cut") mode_cut();
    if (all || mode == "rank") mode_rank();
    if (all || mode == "subpixel") mode_subpixel();
    if (all || mode == "values16") mode_values16();
    if (all || mode == "rules") mode_rules();
    printf("%s\n", g_failures ? "FAILED" : "ok");
    return g_failures ? 1 : 0;
}
