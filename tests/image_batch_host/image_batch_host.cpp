// image_batch_host.cpp -- TEST-ONLY stand-alone host program for image batches (fftconv_plan_set_images).
//
// Built by tests/test_image_batch_host.py with the host compiler from the product's headers and the phase context of
// tests/emu/emu_runners.hpp; it is not the emulator library and not part of the product.  Modes:
//   index    the block -> (image, kernel0, nk) mappings of the spectral-row wrappers (fast_paths.hpp: rows_walk_3d,
//            rows_walk_flat, rows_generic_slot) over grids of (B, N, per_wg): every (image, row group, kernel) is visited exactly
//            once, no walk crosses an image, the F > 1 order keeps the walks of an image adjacent within a row group
//   cut      the launch cutting of a convolve (pipeline.hpp: cut_launches): the rectangles tile the (image, kernel) grid exactly
//            once, a rectangle's maps are consecutive in the output, one image reproduces the (first, ny) loop of a one-image plan
//   rows     the row bodies at L = 288 through the wrappers' pointer shift (rows_shift_to_image), F = 1 and F = 2, and the generic
//            body through its map slot: a batch run writes the same bits into Y as per-image runs with the same walk length, and
//            nothing outside its slots (poisoned bands)
// Having its own main, it is also the place for a host sanitizer build (-fsanitize=address,undefined) of this code.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "emu_runners.hpp"

using namespace fc;
using emu::HostPhaseCtx;

namespace {

int g_failures = 0, g_ok = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            g_failures++;                                 \
            printf("FAIL ");                              \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
        } else g_ok++;                                    \
    } while (0)

// ---------------------------------------------------------------- index
int cmd_index() {
    struct Case { int B, N, per_wg, groups; };
    const Case cases[] = {{1, 1, 1, 3},  {1, 17, 16, 19}, {3, 17, 16, 19}, {3, 20, 16, 19}, {2, 3, 2, 5}, {3, 5, 2, 9},
                          {5, 1, 1, 8},  {1, 4, 4, 1},    {3, 7, 3, 10},   {4, 16, 16, 17}, {2, 9, 4, 16}};
    for (const Case& c : cases) {
        const FastRowsGrid g = fast_rows_grid(c.groups, 1, c.N, c.per_wg);     // (rows = groups at one row per workgroup)
        // F = 1 / generic: the 3-D grid (group, walk, image)
        std::map<std::tuple<int, int, int>, int> seen;
        bool inside = true;
        for (int bz = 0; bz < c.B; bz++)
            for (int by = 0; by < g.walks; by++)
                for (int bx = 0; bx < g.groups; bx++) {
                    const RowsWalk w = rows_walk_3d(bx, by, bz, c.N, c.per_wg);
                    inside = inside && w.image == bz && w.group == bx && w.nk >= 1 && w.nk <= c.per_wg && w.kernel0 >= 0 && w.kernel0 + w.nk <= c.N;
                    for (int k = 0; k < w.nk; k++) seen[{w.image, w.group, w.kernel0 + k}]++;
                }
        bool once = (long)seen.size() == (long)c.B * c.groups * c.N;
        for (auto& kv : seen) once = once && kv.second == 1;
        CHECK(inside && once, "3-D grid B=%d N=%d per_wg=%d: inside %d, every pair once %d (%zu pairs)", c.B, c.N, c.per_wg, inside, once, seen.size());
        // generic kernel: slot = image * N + kernel, split again as the body does
        bool slots = true;
        for (int bz = 0; bz < c.B; bz++)
            for (int by = 0; by < c.N; by++) {
                const int slot = rows_generic_slot(by, bz, c.N);
                slots = slots && slot == bz * c.N + by && slot / c.N == bz && slot - (slot / c.N) * c.N == by;
            }
        CHECK(slots, "generic slot B=%d N=%d", c.B, c.N);
        // F > 1: the flat XCD-aware grid
        seen.clear();
        inside = true;
        bool adjacent = true;
        const int flat = g.flat * c.B;
        CHECK(flat == 8 * ((c.groups + 7) / 8) * g.walks * c.B, "flat grid size");
        std::map<int, std::vector<int>> images_of_group;     // row group -> the images of its blocks in block order (per XCD: ascending sq)
        for (int b = 0; b < flat; b++) {
            const RowsWalk w = rows_walk_flat(b, c.groups, g.walks, c.B, c.N, c.per_wg);
            if (w.group >= c.groups) continue;
            inside = inside && w.group >= 0 && w.image >= 0 && w.image < c.B && w.nk >= 1 && w.nk <= c.per_wg && w.kernel0 >= 0 && w.kernel0 + w.nk <= c.N &&
                     (w.group & 7) == (b & 7);
            images_of_group[w.group].push_back(w.image);
            for (int k = 0; k < w.nk; k++) seen[{w.image, w.group, w.kernel0 + k}]++;
        }
        once = (long)seen.size() == (long)c.B * c.groups * c.N;
        for (auto& kv : seen) once = once && kv.second == 1;
        for (auto& kv : images_of_group) {      // the walks of an image: one run of `walks` consecutive blocks of the group's XCD, images ascending
            const std::vector<int>& v = kv.second;
            adjacent = adjacent && (int)v.size() == g.walks * c.B;
            for (size_t i = 0; i < v.size(); i++) adjacent = adjacent && v[i] == (int)i / g.walks;
        }
        CHECK(inside && once && adjacent, "flat grid B=%d N=%d per_wg=%d (walks %d, B x walks %s a multiple of 8): inside %d, once %d, adjacent %d", c.B, c.N,
              c.per_wg, g.walks, (c.B * g.walks) % 8 ? "not" : "is", inside, once, adjacent);
    }
    // zero defaults: one image
    CHECK(rows_images(0) == 1 && rows_images(1) == 1 && rows_images(4) == 4, "rows_images");
    printf("%d ok, %d failed\n%s\n", g_ok, g_failures, g_failures ? "FAILED" : "index functions ok");
    return g_failures ? 1 : 0;
}

// ---------------------------------------------------------------- cut
int cmd_cut() {
    // (B, n kernels of the group, image stride = kernels of the call, kernels per chunk, maps per launch); chunk 0 = all, maps 0 = 64 (auto)
    struct Case { int B, n, stride, chunk, maps; const char* want; };
    const Case cases[] = {
        {3, 2, 2, 0, 4, "whole"},   {2, 5, 5, 0, 3, "ranges"},  {3, 5, 5, 2, 0, "ranges"}, {1, 7, 7, 0, 0, "one"},     {1, 70, 70, 64, 64, "one"},
        {2, 5, 5, 3, 3, "ranges"},  {3, 7, 7, 6, 2, "ranges"},  {2, 4, 9, 0, 3, "ranges"},      // chunk of 3 = one launch; chunks of several launches
        {1, 9, 9, 4, 2, "one"},     {3, 2, 2, 0, 0, "single"},  {4, 16, 16, 0, 64, "whole"}, {2, 2, 5, 0, 0, "ranges"}, {5, 1, 1, 0, 2, "whole"},
        {3, 20, 20, 0, 0, "single"}, {2, 3, 3, 0, 5, "whole"},
    };
    for (const Case& c : cases) {
        const int nbA = c.chunk > 0 ? c.chunk : c.n, nbY = c.maps > 0 ? c.maps : 64;
        const std::vector<LaunchRect> rs = cut_launches(c.B, c.n, c.stride, nbA, nbY);
        std::vector<int> hits((size_t)c.B * c.n, 0);
        bool consecutive = true, bounded = true, chunks = true, shape = true;
        int chunk_seen = -1, nstart = 0;
        for (const LaunchRect& r : rs) {
            nstart += r.chunk_start;
            bounded = bounded && r.nb >= 1 && r.nk >= 1 && r.ny() <= nbY && r.b0 >= 0 && r.b0 + r.nb <= c.B && r.k0 >= r.a0 && r.k0 + r.nk <= r.a0 + r.na &&
                      r.na <= nbA && r.a0 + r.na <= c.n;
            // one image x a kernel range, or whole images x every kernel of the call
            shape = shape && (r.nb == 1 || (r.k0 == 0 && r.nk == c.n && c.n == c.stride && r.na == c.n));
            if (r.chunk_start) { chunks = chunks && r.a0 > chunk_seen; chunk_seen = r.a0; }
            else chunks = chunks && r.a0 == chunk_seen;
            for (int b = r.b0; b < r.b0 + r.nb; b++)
                for (int k = r.k0; k < r.k0 + r.nk; k++) {
                    hits[(size_t)b * c.n + k]++;
                    // slot (b - b0) * nk + (k - k0) of the intermediate is map first + slot of the output
                    consecutive = consecutive && b * c.stride + k == r.first(c.stride) + (b - r.b0) * r.nk + (k - r.k0);
                }
        }
        chunks = chunks && nstart == (c.n + nbA - 1) / nbA;      // the column spectra of a chunk are produced once, for every image
        bool once = true;
        for (int h : hits) once = once && h == 1;
        bool kind = true;
        if (!strcmp(c.want, "single")) kind = rs.size() == 1 && rs[0].nb == c.B && rs[0].nk == c.n;
        if (!strcmp(c.want, "whole")) for (const LaunchRect& r : rs) kind = kind && r.nk == c.n && r.k0 == 0;
        if (!strcmp(c.want, "ranges")) for (const LaunchRect& r : rs) kind = kind && r.nb == 1;
        if (!strcmp(c.want, "one")) {      // the loop of a one-image plan
            std::vector<std::pair<int, int>> today;
            for (int a0 = 0; a0 < c.n; a0 += nbA) {
                const int na = std::min(nbA, c.n - a0);
                for (int y0 = 0; y0 < na; y0 += nbY) today.push_back({a0 + y0, std::min(nbY, na - y0)});
            }
            kind = today.size() == rs.size();
            for (size_t i = 0; kind && i < rs.size(); i++)
                kind = rs[i].first(c.stride) == today[i].first && rs[i].ny() == today[i].second && rs[i].nb == 1 && rs[i].chunk_start == (rs[i].k0 == rs[i].a0);
        }
        CHECK(once && consecutive && bounded && chunks && shape && kind,
              "cut B=%d n=%d stride=%d chunk=%d maps=%d (%s): %zu launches, once %d consecutive %d bounded %d chunks %d shape %d kind %d", c.B, c.n, c.stride,
              nbA, nbY, c.want, rs.size(), once, consecutive, bounded, chunks, shape, kind);
        printf("     B=%d n=%d stride=%d chunk=%d maps=%d:", c.B, c.n, c.stride, nbA, nbY);
        for (const LaunchRect& r : rs) printf(" [img %d+%d x k %d+%d]", r.b0, r.nb, r.k0, r.nk);
        printf("\n");
    }
    // the issue's examples by shape
    {
        const auto a = cut_launches(3, 2, 2, 2, 4);
        CHECK(a.size() == 2 && a[0].nb == 2 && a[1].nb == 1 && a[1].b0 == 2, "(3, 2, all, 4): whole-image launches 2 + 1");
        // one chunk holds all five kernels, a launch three maps: every image walks the chunk in two launches, the second at
        // offset 3 in the chunk, and the chunk's column spectra are produced once
        const auto b = cut_launches(2, 5, 5, 5, 3);
        bool b_ok = b.size() == 4 && b[0].chunk_start;
        const int want_b[4][3] = {{0, 0, 3}, {0, 3, 2}, {1, 0, 3}, {1, 3, 2}};      // image, k0, nk
        for (size_t i = 0; b_ok && i < 4; i++)
            b_ok = b[i].b0 == want_b[i][0] && b[i].nb == 1 && b[i].k0 == want_b[i][1] && b[i].nk == want_b[i][2] && b[i].a0 == 0 && b[i].na == 5 &&
                   b[i].chunk_start == (i == 0) && b[i].first(5) == want_b[i][0] * 5 + want_b[i][1];
        CHECK(b_ok, "(2, 5, all, 3): kernel ranges of one image, one chunk");
        const auto b3 = cut_launches(2, 5, 5, 3, 3);
        CHECK(b3.size() == 4 && b3[0].nk == 3 && b3[0].chunk_start && b3[1].b0 == 1 && !b3[1].chunk_start && b3[2].k0 == 3 && b3[2].nk == 2 && b3[2].chunk_start &&
              b3[2].a0 == 3 && !b3[3].chunk_start, "(2, 5, chunk of 3, 3): a chunk per launch, each serving both images");
        const auto c = cut_launches(3, 5, 5, 2, 64);
        CHECK(c.size() == 9 && c[0].chunk_start && !c[1].chunk_start && c[3].chunk_start && c[3].k0 == 2, "(3, 5, chunk of 2, auto)");
    }
    printf("%d ok, %d failed\n%s\n", g_ok, g_failures, g_failures ? "FAILED" : "launch cutting ok");
    return g_failures ? 1 : 0;
}

// ---------------------------------------------------------------- rows
float rnd(uint32_t& s) {
    s = s * 1664525u + 1013904223u;
    return (float)((int32_t)(s >> 8) - (1 << 23)) / (float)(1 << 23);
}
constexpr size_t GUARD = 96;                    // poisoned c32 in front of and behind the batch's slots
const c32 POISON = {-7.0e37f, 7.5e37f};
bool same_bits(const c32& a, const c32& b) { return memcmp(&a, &b, sizeof(c32)) == 0; }

// specialised bodies, RowCfg of 288 points: B images x nk kernels, walks of per_wg
template <class Cfg, int NZ2>
void run_fast(int F, int B, int nk, int per_wg, int kw, int kernel_path_mode) {
    PlanTuning tune;
    tune.path_mode = kernel_path_mode;
    Geometry g;
    Tables t;
    char what[96];
    snprintf(what, sizeof(what), "L=288 F=%d B=%d nk=%d per_wg=%d path_mode=%d", F, B, nk, per_wg, kernel_path_mode);
    if (!make_geometry(g, t, 270, 270, F, 19, 19, tune) || !g.fast_rows.ok || g.Lw != Cfg::L || g.fast_rows.RPW != Cfg::RPW || g.fast_rows.NT != Cfg::NT ||
        fast_rows_nz2(g, kw) > NZ2) {
        CHECK(false, "%s: the plan does not run the configuration this case names (Lw %d)", what, g.Lw);
        return;
    }
    DeviceTables d;
    d.fr_tw1 = t.fr.tw1.data(); d.fr_tw2 = t.fr.tw2.data(); d.fr_relayout = t.fr.relayout.data();
    if (g.fast_cols.ok) d.fc_pair_row_of = t.fcl.pair_row_of.data();
    uint32_t seed = 99u + (uint32_t)(F * 131 + B * 17 + nk);
    const size_t per_a = (size_t)g.F * g.rows * a_pitch_for(kw), se = g.spectrum_elems(), ye = g.y_elems_per_kernel();
    std::vector<c32> A(per_a * nk), S(se * B);
    for (c32& v : A) v = mk(rnd(seed), rnd(seed));
    for (c32& v : S) v = mk(rnd(seed), rnd(seed));
    std::vector<c32> lds(FC_LDS_BUDGET / sizeof(c32));
    auto body = [&](const FastRowsArgs& a, const RowsWalk& w) {
        for (int i = 0; i < Cfg::LDS_ELEMS; i++) lds[i] = mk(1e30f, -1e30f);
        if (F > 1) {
            HostPhaseCtx<RowMultiState<Cfg, true>> ctx(Cfg::NT);
            fast_rows_multi_body<Cfg, NZ2, true, true>(ctx, lds.data(), a, w.group, w.kernel0, w.nk, g.rows);
        } else {
            HostPhaseCtx<RowMultiState<Cfg>> ctx(Cfg::NT);
            fast_rows_multi_body<Cfg, NZ2, true>(ctx, lds.data(), a, w.group, w.kernel0, w.nk, g.rows);
        }
    };
    const FastRowsGrid grid = fast_rows_grid(g.rows, Cfg::RPW, nk, per_wg);
    // the reference: one run per image into a buffer of its own, the same walk length
    std::vector<std::vector<c32>> ref(B, std::vector<c32>(ye * nk, POISON));
    for (int b = 0; b < B; b++) {
        FastRowsArgs a = fast_rows_args(g, d, A.data(), kw, S.data() + (size_t)b * se, ref[b].data());     // (image fields zero: one image)
        for (int by = 0; by < grid.walks; by++)
            for (int bx = 0; bx < grid.groups; bx++) body(a, rows_walk_3d(bx, by, 0, nk, per_wg));
    }
    // the batch: the wrappers' text -- block -> walk, then the pointer shift in the by-value copy of the arguments
    std::vector<c32> Y(GUARD + ye * nk * B + GUARD, POISON);
    FastRowsArgs base = fast_rows_args(g, d, A.data(), kw, S.data(), Y.data() + GUARD);
    rows_args_set_images(base, g, B, nk);
    if (F > 1) {
        for (int blk = 0; blk < grid.flat * rows_images(base.images); blk++) {
            FastRowsArgs a = base;
            const RowsWalk w = rows_walk_flat(blk, grid.groups, grid.walks, a.images, nk, per_wg);
            if (w.group >= grid.groups) continue;
            rows_shift_to_image(a.S, a.Y, w.image, a.s_image_stride, nk, a.y_kernel_stride);
            body(a, w);
        }
    } else {
        for (int bz = 0; bz < rows_images(base.images); bz++)
            for (int by = 0; by < grid.walks; by++)
                for (int bx = 0; bx < grid.groups; bx++) {
                    FastRowsArgs a = base;
                    const RowsWalk w = rows_walk_3d(bx, by, bz, nk, per_wg);
                    rows_shift_to_image(a.S, a.Y, w.image, a.s_image_stride, nk, a.y_kernel_stride);
                    body(a, w);
                }
    }
    size_t differ = 0, stray = 0, written = 0;
    for (size_t i = 0; i < GUARD; i++) stray += !same_bits(Y[i], POISON) + !same_bits(Y[GUARD + ye * nk * B + i], POISON);
    for (int b = 0; b < B; b++)
        for (size_t i = 0; i < ye * nk; i++) {
            const c32& got = Y[GUARD + (size_t)b * ye * nk + i];
            differ += !same_bits(got, ref[b][i]);
            written += !same_bits(got, POISON);
        }
    // (images differ: the test would pass trivially on equal spectra)
    bool images_differ = B < 2 || memcmp(ref[0].data(), ref[1].data(), ye * nk * sizeof(c32)) != 0;
    CHECK(differ == 0 && stray == 0 && written > 0 && images_differ, "%s: %zu elements differ from the per-image runs, %zu stray stores, %zu written, images differ %d",
          what, differ, stray, written, images_differ);
    if (!differ && !stray) printf("ok   %s: %zu elements bit-equal to the per-image runs, bands intact\n", what, written);
}

// generic body (kernel_path 1 and the Bluestein rows): image through the map slot
void run_generic(int F, int B, int nk, int H, int W, int kh, int kw, bool exact) {
    PlanTuning tune;
    tune.path_mode = 0;
    tune.exact_window = exact;
    Geometry g;
    Tables t;
    char what[96];
    snprintf(what, sizeof(what), "generic %dx%d F=%d B=%d nk=%d%s", H, W, F, B, nk, exact ? " exact_window" : "");
    if (!make_geometry(g, t, H, W, F, kh, kw, tune) || g.fast_rows.ok) { CHECK(false, "%s: no generic plan", what); return; }
    DeviceTables d;
    d.tw_w = t.pw.tw.data();
    uint32_t seed = 7u + (uint32_t)(F * 31 + B);
    const size_t per_a = (size_t)g.F * g.rows * a_pitch_for(kw), se = g.spectrum_elems(), ye = g.y_elems_per_kernel();
    std::vector<c32> A(per_a * nk), S(se * B);
    for (c32& v : A) v = mk(rnd(seed), rnd(seed));
    for (c32& v : S) v = mk(rnd(seed), rnd(seed));
    std::vector<c32> lds(FC_LDS_BUDGET / sizeof(c32));
    emu::HostCtx ctx;
    std::vector<std::vector<c32>> ref(B, std::vector<c32>(ye * nk, POISON));
    for (int b = 0; b < B; b++) {
        const SpectralRowsArgs a = spectral_rows_args(g, t, d, A.data(), kw, S.data() + (size_t)b * se, ref[b].data());
        for (int k = 0; k < nk; k++)
            for (int row = 0; row < g.rows; row++) spectral_rows_body<-1>(ctx, lds.data(), a, row, k);
    }
    std::vector<c32> Y(GUARD + ye * nk * B + GUARD, POISON);
    SpectralRowsArgs a = spectral_rows_args(g, t, d, A.data(), kw, S.data(), Y.data() + GUARD);
    rows_args_set_images(a, g, B, nk);
    for (int bz = 0; bz < rows_images(a.images); bz++)
        for (int by = 0; by < nk; by++)
            for (int row = 0; row < g.rows; row++) spectral_rows_body<-1>(ctx, lds.data(), a, row, rows_generic_slot(by, bz, nk));
    size_t differ = 0, stray = 0, written = 0;
    for (size_t i = 0; i < GUARD; i++) stray += !same_bits(Y[i], POISON) + !same_bits(Y[GUARD + ye * nk * B + i], POISON);
    for (int b = 0; b < B; b++)
        for (size_t i = 0; i < ye * nk; i++) {
            const c32& got = Y[GUARD + (size_t)b * ye * nk + i];
            differ += !same_bits(got, ref[b][i]);
            written += !same_bits(got, POISON);
        }
    CHECK(differ == 0 && stray == 0 && written > 0, "%s (acc_in_y %d, work length %d): %zu differ, %zu stray, %zu written", what, (int)g.acc_in_y, g.work_w, differ,
          stray, written);
    if (!differ && !stray) printf("ok   %s: %zu elements bit-equal to the per-image runs, bands intact\n", what, written);
}

int cmd_rows() {
    using C288 = RowCfg<288, 4, 6, 12, 192, 8>;      // cfg1's row transform: eight rows per workgroup
    run_fast<C288, 3>(1, 3, 20, 16, 19, 2);          // a walk boundary at 16 and image boundaries
    run_fast<C288, 3>(1, 2, 3, 2, 19, 2);
    run_fast<C288, 3>(1, 1, 3, 2, 19, 2);            // one image through the same text
    run_fast<C288, 3>(1, 2, 3, 1, 19, 1);            // row-major intermediate
    run_fast<C288, 3>(2, 2, 3, 2, 19, 2);            // F > 1: the flat grid over (image, walk) pairs
    run_fast<C288, 3>(3, 3, 5, 4, 19, 2);
    run_generic(1, 3, 2, 40, 56, 5, 7, false);
    run_generic(3, 3, 2, 40, 56, 5, 7, false);
    run_generic(2, 2, 2, 290, 290, 15, 15, true);    // Bluestein rows (window 304)
    printf("%d ok, %d failed\n%s\n", g_ok, g_failures, g_failures ? "FAILED" : "all bit-equal");
    return g_failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "index") return cmd_index();
    if (mode == "cut") return cmd_cut();
    if (mode == "rows") return cmd_rows();
    fprintf(stderr, "usage: %s index | cut | rows\n", argv[0]);
    return 2;
}
