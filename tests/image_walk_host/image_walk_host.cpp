// image_walk_host.cpp -- TEST-ONLY stand-alone host program for the image-walk spectral-row kernel (plan option "image_walk").
//
// Built by tests/test_image_walk_host.py with the host compiler from the product's headers and the phase context of
// tests/emu/emu_runners.hpp; it is not the emulator library and not part of the product.  Modes:
//   index    the block -> (row group, kernel, image0, ni) mapping of the wrapper (fast_paths.hpp: rows_walk_images) over grids of
//            (groups, N, B, per_wg): every (row group, kernel, image) is visited exactly once, no walk runs past the images of the
//            launch, and within a row group the blocks of one image walk are consecutive over kernels
//   rows     fast_rows_images_body at five lengths through the wrapper's own text: the maps of (image, kernel) are the same bits
//            whatever the walk length and whatever the batch, nothing outside the B x nk slots is written (poisoned bands), and
//            every row of the first, a middle and the last row group (each row slot of a workgroup) is as close to a float64 row
//            transform as the kernel-walk body's (<= 2 x its maximum error)
// Having its own main, it is also the place for a host sanitizer build (-fsanitize=address,undefined) of this code.
#include <cmath>
#include <complex>
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
    struct Case { int groups, N, B, per_wg; };
    const Case cases[] = {{3, 1, 1, 1},   {19, 1, 64, 16}, {19, 3, 17, 16}, {5, 2, 17, 16}, {8, 3, 19, 16}, {16, 1, 5, 4},
                          {10, 7, 3, 3},  {17, 16, 4, 1},  {1, 4, 9, 2},    {145, 1, 2, 2}, {9, 5, 1, 16},  {12, 2, 33, 16}};
    for (const Case& c : cases) {
        const int iwalks = rows_image_walks(c.B, c.per_wg), grid = rows_images_grid(c.groups, c.N, iwalks);
        std::map<std::tuple<int, int, int>, int> seen;
        std::map<std::pair<int, int>, std::vector<int>> kernels_of_walk;      // (row group, image0) -> kernels in block order
        std::map<int, std::vector<int>> walks_of_group;                       // row group -> image0 of its blocks in block order
        bool inside = true;
        CHECK(grid == 8 * ((c.groups + 7) / 8) * iwalks * c.N && iwalks == (c.B + c.per_wg - 1) / c.per_wg, "grid size");
        for (int b = 0; b < grid; b++) {
            const RowsImageWalk w = rows_walk_images(b, c.groups, c.N, iwalks, c.B, c.per_wg);
            if (w.group >= c.groups) continue;      // padding of the last round of XCDs
            inside = inside && w.group >= 0 && (w.group & 7) == (b & 7) && w.kernel >= 0 && w.kernel < c.N && w.image0 >= 0 && w.ni >= 1 &&
                     w.ni <= c.per_wg && w.image0 + w.ni <= c.B && w.image0 % c.per_wg == 0;
            kernels_of_walk[{w.group, w.image0}].push_back(w.kernel);
            walks_of_group[w.group].push_back(w.image0);
            for (int m = 0; m < w.ni; m++) seen[{w.group, w.kernel, w.image0 + m}]++;
        }
        bool once = (long)seen.size() == (long)c.groups * c.N * c.B;
        for (auto& kv : seen) once = once && kv.second == 1;
        // the kernel is the fastest coordinate: the N blocks of a walk are consecutive (on their XCD) and ascending, then the next walk
        bool adjacent = true;
        for (auto& kv : kernels_of_walk) {
            adjacent = adjacent && (int)kv.second.size() == c.N;
            for (size_t i = 0; i < kv.second.size(); i++) adjacent = adjacent && kv.second[i] == (int)i;
        }
        for (auto& kv : walks_of_group) {
            const std::vector<int>& v = kv.second;
            adjacent = adjacent && (int)v.size() == iwalks * c.N;
            for (size_t i = 0; i < v.size(); i++) adjacent = adjacent && v[i] == (int)(i / c.N) * c.per_wg;
        }
        CHECK(inside && once && adjacent, "grid groups=%d N=%d B=%d per_wg=%d (%d walks, %d blocks): inside %d, once %d, adjacent %d", c.groups, c.N, c.B,
              c.per_wg, iwalks, grid, inside, once, adjacent);
    }
    CHECK(rows_image_walks(0, 4) == 1 && rows_image_walks(17, 16) == 2 && rows_image_walks(16, 16) == 1, "rows_image_walks");
    printf("%d ok, %d failed\n%s\n", g_ok, g_failures, g_failures ? "FAILED" : "index function ok");
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

// element (row i, column w) of a map of the intermediate
size_t y_index(const Geometry& g, const Tables& t, int i, int w) {
    if (!g.y_tiled()) return (size_t)i * g.y_pitch + w;
    const int TL = g.y_tile_w;
    return (size_t)(w / TL) * (g.tile_rows() * TL) + (size_t)t.fcl.pair_row_of[i] * TL + (w % TL);
}

struct Shape { int H, W, kh, kw, path_mode, fft_h, fft_w, wout; bool tiled; };

// B images x nk kernels at the plan of `sh`, which must run RowCfg Cfg (and the kernel walk its NZ2_OLD variant)
template <class Cfg, int NZ2_OLD>
void run_images(const Shape& sh, int B, int nk) {
    PlanTuning tune;
    tune.path_mode = sh.path_mode;
    Geometry g;
    Tables t;
    char what[96];
    snprintf(what, sizeof(what), "L=%d (%dx%d (*) %dx%d) B=%d nk=%d", Cfg::L, sh.H, sh.W, sh.kh, sh.kw, B, nk);
    if (!make_geometry(g, t, sh.H, sh.W, 1, sh.kh, sh.kw, tune) || !g.fast_rows.ok || g.Lh != sh.fft_h || g.Lw != Cfg::L || g.Lw != sh.fft_w ||
        g.fast_rows.RPW != Cfg::RPW || g.fast_rows.NT != Cfg::NT || g.fast_rows.R1 != Cfg::R1 || g.fast_rows.R3 != Cfg::R3 || g.wout != sh.wout ||
        g.y_tiled() != sh.tiled || fast_rows_nz2(g, sh.kw) > NZ2_OLD) {
        CHECK(false, "%s: the plan does not run the configuration this case names (transform %d x %d, window %d, tiled %d)", what, g.Lh, g.Lw, g.wout,
              (int)g.y_tiled());
        return;
    }
    const int kw = sh.kw;
    DeviceTables d;
    d.fr_tw1 = t.fr.tw1.data(); d.fr_tw2 = t.fr.tw2.data(); d.fr_relayout = t.fr.relayout.data();
    if (g.fast_cols.ok) d.fc_pair_row_of = t.fcl.pair_row_of.data();
    uint32_t seed = 4242u + (uint32_t)(Cfg::L * 7 + B);
    const size_t per_a = (size_t)g.rows * a_pitch_for(kw), se = g.spectrum_elems(), ye = g.y_elems_per_kernel();
    std::vector<c32> A(per_a * nk), S(se * B);
    for (c32& v : A) v = mk(rnd(seed), rnd(seed));
    for (c32& v : S) v = mk(rnd(seed), rnd(seed));
    std::vector<c32> lds(FC_LDS_BUDGET / sizeof(c32));
    const int groups = fast_rows_grid(g.rows, Cfg::RPW, 1, 1).groups;

    // the wrapper's text (kernels_rows_images.inc: k_fast_rows_images) over the whole grid of a launch of `images` images
    auto launch = [&](std::vector<c32>& Y, int images, int per_wg) {
        FastRowsArgs a = fast_rows_args(g, d, A.data(), kw, S.data(), Y.data() + GUARD);
        rows_args_set_images(a, g, images, nk);
        const int iwalks = rows_image_walks(a.images, per_wg);
        for (int blk = 0; blk < rows_images_grid(groups, a.kernels_per_image, iwalks); blk++) {
            const RowsImageWalk w = rows_walk_images(blk, groups, a.kernels_per_image, iwalks, a.images, per_wg);
            if (w.group >= groups) continue;
            for (int i = 0; i < Cfg::LDS_ELEMS; i++) lds[i] = mk(1e30f, -1e30f);
            HostPhaseCtx<RowImagesState<Cfg>> ctx(Cfg::NT);
            fast_rows_images_body<Cfg>(ctx, lds.data(), a, w.group, w.kernel, w.image0, w.ni, g.rows);
        }
    };
    auto bands = [&](const std::vector<c32>& Y, int images, size_t& stray, size_t& written) {
        stray = written = 0;
        for (size_t i = 0; i < GUARD; i++) stray += !same_bits(Y[i], POISON) + !same_bits(Y[GUARD + ye * nk * images + i], POISON);
        for (size_t i = 0; i < ye * nk * images; i++) written += !same_bits(Y[GUARD + i], POISON);
    };

    // 1, 2: walks of 16 + 1, of 3 and of 1 image, and a batch of the first two images only
    std::vector<c32> Y16(GUARD + ye * nk * B + GUARD, POISON), Y3(Y16), Y1(Y16), Y2(GUARD + ye * nk * 2 + GUARD, POISON);
    launch(Y16, B, 16);
    launch(Y3, B, 3);
    launch(Y1, B, 1);
    launch(Y2, 2, 16);
    size_t stray = 0, written = 0, stray2 = 0, written2 = 0;
    bands(Y16, B, stray, written);
    bands(Y2, 2, stray2, written2);
    const bool walks_equal = memcmp(Y16.data(), Y3.data(), Y16.size() * sizeof(c32)) == 0 && memcmp(Y16.data(), Y1.data(), Y16.size() * sizeof(c32)) == 0;
    const bool batch_equal = memcmp(Y16.data(), Y2.data(), (GUARD + ye * nk * 2) * sizeof(c32)) == 0;
    const bool images_differ = memcmp(Y16.data() + GUARD, Y16.data() + GUARD + ye * nk, ye * nk * sizeof(c32)) != 0;
    CHECK(walks_equal && batch_equal && stray == 0 && stray2 == 0 && written > 0 && written2 > 0 && images_differ,
          "%s: walks of 16 / 3 / 1 equal %d, batch of 2 equal %d, stray stores %zu + %zu, written %zu, images differ %d", what, walks_equal, batch_equal, stray,
          stray2, written, images_differ);

    // 3: against a float64 row transform, beside the kernel-walk body on the same data
    std::vector<c32> Yold(GUARD + ye * nk * B + GUARD, POISON);
    {
        FastRowsArgs base = fast_rows_args(g, d, A.data(), kw, S.data(), Yold.data() + GUARD);
        rows_args_set_images(base, g, B, nk);
        const FastRowsGrid grid = fast_rows_grid(g.rows, Cfg::RPW, nk, 16);
        for (int bz = 0; bz < B; bz++)
            for (int by = 0; by < grid.walks; by++)
                for (int bx = 0; bx < grid.groups; bx++) {
                    FastRowsArgs a = base;
                    const RowsWalk w = rows_walk_3d(bx, by, bz, nk, 16);
                    rows_shift_to_image(a.S, a.Y, w.image, a.s_image_stride, nk, a.y_kernel_stride);
                    for (int i = 0; i < Cfg::LDS_ELEMS; i++) lds[i] = mk(1e30f, -1e30f);
                    HostPhaseCtx<RowMultiState<Cfg>> ctx(Cfg::NT);
                    fast_rows_multi_body<Cfg, NZ2_OLD, true>(ctx, lds.data(), a, w.group, w.kernel0, w.nk, g.rows);
                }
    }
    const int L = Cfg::L;
    std::vector<std::complex<double>> tw(L), X(L), ref(g.wout);
    for (int n = 0; n < L; n++) tw[n] = std::polar(1.0, 2.0 * M_PI * n / L);
    double err_new = 0, err_old = 0;
    // every row of the first, a middle and the last (partial) row group: each row slot rr < RPW of a workgroup is held against the reference
    std::vector<int> check_rows;
    for (int grp : {0, groups / 2, groups - 1})
        for (int rr = 0; rr < Cfg::RPW; rr++)
            if (grp * Cfg::RPW + rr < g.rows && (check_rows.empty() || check_rows.back() < grp * Cfg::RPW + rr)) check_rows.push_back(grp * Cfg::RPW + rr);
    std::vector<int> slots_seen(Cfg::RPW, 0);
    for (int row : check_rows) slots_seen[row % Cfg::RPW]++;
    for (int rr = 0; rr < Cfg::RPW; rr++) CHECK(slots_seen[rr] >= 1 || g.rows <= rr, "%s: row slot %d of a workgroup is not sampled", what, rr);
    const int check_maps[][2] = {{0, 0}, {B - 1, nk - 1}, {B / 2, 0}};      // (image, kernel)
    for (const auto& bm : check_maps)
        for (int row : check_rows) {
            const c32* x = A.data() + (size_t)bm[1] * per_a + (size_t)row * a_pitch_for(kw);
            const c32* srow = S.data() + (size_t)bm[0] * se + (size_t)row * g.s_pitch;
            for (int k = 0; k < L; k++) {
                std::complex<double> acc = 0;
                for (int j = 0; j < kw; j++) acc += std::complex<double>(x[j].x, x[j].y) * std::conj(tw[(size_t)j * k % L]);
                const c32 sv = srow[t.nat_col_of[k]];
                X[k] = acc * std::complex<double>(sv.x, sv.y);
            }
            double top = 0;
            for (int w = 0; w < g.wout; w++) {
                std::complex<double> acc = 0;
                for (int k = 0; k < L; k++) acc += X[k] * tw[(size_t)k * w % L];
                ref[w] = acc;
                top = std::max(top, std::abs(acc));
            }
            const size_t slot = GUARD + ((size_t)bm[0] * nk + bm[1]) * ye;
            for (int w = 0; w < g.wout; w++) {
                const c32 a = Y16[slot + y_index(g, t, row, w)], b = Yold[slot + y_index(g, t, row, w)];
                err_new = std::max(err_new, std::abs(std::complex<double>(a.x, a.y) - ref[w]) / top);
                err_old = std::max(err_old, std::abs(std::complex<double>(b.x, b.y) - ref[w]) / top);
            }
        }
    // (the kernel walk itself must be a float32 transform of that row: a reference with the wrong order or sign fails here)
    CHECK(err_old < 1e-5 && err_new <= 2 * err_old, "%s: error against float64 rows: image walk %.3g, kernel walk %.3g (bar: 2 x the kernel walk's)", what, err_new,
          err_old);
    printf("ok   %s: walks and batches bit-equal, %zu elements written, bands intact; error against float64 rows: image walk %.3g, kernel walk %.3g\n", what,
           written, err_new, err_old);
}

int cmd_rows() {
    // the configurations the planner picks for the shapes of tests/test_image_walk_gpu.py
    run_images<RowCfg<288, 4, 6, 12, 192, 8>, 3>({250, 250, 31, 31, 2, 288, 288, 288, true}, 17, 3);       // eight rows per workgroup, two store chains
    run_images<RowCfg<384, 4, 8, 12, 192, 6>, 3>({270, 270, 31, 31, 2, 384, 384, 304, true}, 17, 2);       // six rows, cropped window
    run_images<RowCfg<2112, 8, 12, 22, 192, 2>, 3>({250, 2100, 9, 13, 2, 288, 2112, 2112, true}, 17, 1);   // two rows, two chains at R3 = 22
    run_images<RowCfg<2560, 16, 16, 10, 256, 1>, 7>({250, 2500, 9, 41, 2, 288, 2560, 2544, true}, 17, 2);  // one row, R1 = 16, cropped
    run_images<RowCfg<1152, 8, 12, 12, 192, 2>, 3>({40, 1100, 9, 31, 2, 48, 1152, 1136, false}, 17, 2);    // row-major intermediate (generic output kernel)
    printf("%d ok, %d failed\n%s\n", g_ok, g_failures, g_failures ? "FAILED" : "image walk ok");
    return g_failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "index") return cmd_index();
    if (mode == "rows") return cmd_rows();
    fprintf(stderr, "usage: %s index | rows\n", argv[0]);
    return 2;
}
