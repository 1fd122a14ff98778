// border_host.cpp -- TEST-ONLY stand-alone host program for border modes (fftconv_plan_set_border; csrc/border.hpp).
//
// Built by tests/test_border_host.py with the host compiler from the product's kernel headers and the phase context of
// tests/emu/emu_runners.hpp; it is not the emulator library and not part of the product.  Modes:
//   index         for every mode 1..5, n = 1..40 and every admissible MAXK one line "mode n maxk : s_0 s_1 ..." -- the source
//                 index of every window coordinate r < n + MAXK - 1 (-1: CONSTANT's value); the test compares with numpy.pad.
//                 The first MAXK border_args_error refuses ends each (mode, n): "limit mode n maxk".
//   errors        border_args_error over a table: "mode value H W mkh mkw -> ok | <text>"
//   routes        the not-built table and the direct-route predicate of fast_paths.hpp
//   bodies        fast_cols_fwd_body<Cfg, R2, float, Bordered> on the data against the plain body on the extension materialised
//                 by this program's own reference (ref_source below: nothing shared with border.hpp), on the 288-point
//                 configuration (M = 144): every mode, H odd and even, MAXK odd and even, W no multiple of T, three planes,
//                 static deal and dynamic tile queue.  The spectra must be bit-equal.
//   spectrum IN OUT H W F MKH MKW MODE VALUE
//                 the image spectrum of a bordered plan (default tuning; M = 144 along h and 288 along w) of the fp32 image at
//                 IN ([f][w][h]) into OUT, as fftconv_plan_set_image leaves it: the bordered column body, then the forward row
//                 body over W + MKW - 1 valid columns.  The test runs the emulator's per-kernel loop on it.
// Having its own main, it is also the place for a host sanitizer build (-fsanitize=address,undefined) of this code.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "emu_runners.hpp"

using namespace fc;
using emu::HostPhaseCtx;

namespace {

int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_failures++; printf("FAIL "); printf(__VA_ARGS__); printf("\n"); } } while (0)

using C16 = ColCfg<144, 4, 6, 6, 16, 384>;        // the 288-point transform along h
using R288 = RowCfg<288, 4, 6, 12, 192, 8>;       // ... and along w

// ---- the reference: the extension over ALL integers by its definition (modular arithmetic), nothing shared with border.hpp.
// ---- Returns the data index of integer position t, or -1 for CONSTANT's value.
int ref_source(int mode, int n, int t) {
    if (t >= 0 && t < n) return t;
    switch (mode) {
    case 1: return -1;
    case 2: return t < 0 ? 0 : n - 1;
    case 3: { const int p = 2 * n; int m = ((t % p) + p) % p; return m < n ? m : p - 1 - m; }                    // period 2n: a b c d d c b a
    case 4: { if (n == 1) return 0; const int p = 2 * n - 2; int m = ((t % p) + p) % p; return m < n ? m : p - m; }   // period 2n - 2: a b c d c b
    default: return ((t % n) + n) % n;
    }
}

int cmd_index() {
    for (int mode = 1; mode <= 5; mode++)
        for (int n = 1; n <= 40; n++)
            for (int maxk = 1;; maxk++) {
                if (border_args_error(mode, 0.5f, n, n, maxk, maxk) || maxk > 2 * n + 3) {      // (modes 1, 2: no limit; stop beyond 2n + 3)
                    printf("limit %d %d %d\n", mode, n, maxk);
                    break;
                }
                const BorderLoad b = border_load(mode, 0.5f, n, n, maxk, maxk);
                printf("%d %d %d :", mode, n, maxk);
                for (int r = 0; r < n + maxk - 1; r++) {
                    const int s = (b.fill && border_outside(b.h, r)) ? -1 : border_index(b.h, r);
                    CHECK(b.fill ? true : (s >= 0 && s < n), "mode %d n %d maxk %d r %d: index %d outside the data", mode, n, maxk, r, s);
                    CHECK(border_index(b.h, r) >= 0 && border_index(b.h, r) < n, "mode %d n %d maxk %d r %d: raw index outside the data", mode, n, maxk, r);
                    CHECK(s == ref_source(mode, n, r - border_lead(maxk)), "mode %d n %d maxk %d r %d: %d, reference %d", mode, n, maxk, r, s,
                          ref_source(mode, n, r - border_lead(maxk)));
                    printf(" %d", s);
                }
                printf("\n");
            }
    return g_failures;
}

int cmd_errors() {
    struct Row { int mode; float value; int H, W, mkh, mkw; };
    const float inf = INFINITY, nan = NAN;
    const Row rows[] = {
        {-1, 0.f, 8, 8, 3, 3}, {6, 0.f, 8, 8, 3, 3}, {0, 0.f, 8, 8, 3, 3}, {5, 0.f, 8, 8, 3, 3},
        {1, inf, 8, 8, 3, 3}, {1, -inf, 8, 8, 3, 3}, {1, nan, 8, 8, 3, 3}, {2, nan, 8, 8, 3, 3}, {1, -1.25f, 8, 8, 3, 3},
        // the fold limits: MAXK / 2 <= DATA (3, 5), <= DATA - 1 (4); the limit of each dimension by itself
        {3, 0.f, 4, 9, 9, 3}, {3, 0.f, 4, 9, 10, 3}, {3, 0.f, 9, 4, 3, 9}, {3, 0.f, 9, 4, 3, 10},
        {5, 0.f, 4, 9, 9, 3}, {5, 0.f, 4, 9, 10, 3}, {5, 0.f, 9, 4, 3, 9}, {5, 0.f, 9, 4, 3, 10},
        {4, 0.f, 4, 9, 7, 3}, {4, 0.f, 4, 9, 8, 3}, {4, 0.f, 9, 4, 3, 7}, {4, 0.f, 9, 4, 3, 8},
        {4, 0.f, 1, 1, 1, 1}, {4, 0.f, 1, 1, 2, 1}, {3, 0.f, 1, 1, 3, 3}, {3, 0.f, 1, 1, 4, 1},
        {2, 0.f, 1, 1, 31, 31}, {1, 0.f, 1, 1, 31, 31},
    };
    for (const Row& r : rows) {
        const char* why = border_args_error(r.mode, r.value, r.H, r.W, r.mkh, r.mkw);
        printf("%d %g %d %d %d %d -> %s\n", r.mode, (double)r.value, r.H, r.W, r.mkh, r.mkw, why ? why : "ok");
    }
    return 0;
}

int cmd_routes() {
    std::vector<int> configs;
#define FC_X(MM, A, B, C, TT, NTT) configs.push_back(MM);
    FC_FAST_COL_CONFIGS(FC_X)
#undef FC_X
    printf("configs");
    for (int M : configs) printf(" %d", M);
    printf("\nnot_built");
    for (int x : FC_COLS_FWD_BORDER_NOT_BUILT) {
        printf(" %d", x);
        bool is_config = false;
        for (int M : configs) is_config = is_config || M == x;
        CHECK(is_config, "%d is listed as not built and is no configuration", x);
    }
    printf("\n");
    long ones = 0, walked = 0, built = 0;
    std::vector<int> ms = configs;
    ms.push_back(56);      // a generic / Bluestein plan: no configuration
    for (int M : configs) built += fast_cols_fwd_border_built(M);
    for (int M : ms)
        for (int store = 0; store < 2; store++)
            for (int blockwise = 0; blockwise < 2; blockwise++)
                for (int fast_fwd = 0; fast_fwd < 2; fast_fwd++) {
                    bool listed = false;
                    for (int x : FC_COLS_FWD_BORDER_NOT_BUILT) listed = listed || x == M;
                    const bool want = store && !blockwise && fast_fwd && fast_cols_lookup(M).ok && !listed;
                    const bool got = fast_cols_fwd_border_direct(store, blockwise, fast_fwd, M);
                    CHECK(got == want, "border_direct(M %d, store %d, block-wise %d, fast_fwd %d) = %d", M, store, blockwise, fast_fwd, (int)got);
                    ones += got;
                    walked++;
                }
    CHECK(ones == built, "%ld settings read 1, %ld configurations are built", ones, built);
    printf("ok   direct predicate: %ld settings walked, %ld read 1\n", walked, ones);
    CHECK(!fc_border_mode_ok(-1) && fc_border_mode_ok(0) && fc_border_mode_ok(5) && !fc_border_mode_ok(6), "mode range");
    CHECK(border_lead(31) == 15 && border_trail(31) == 15 && border_lead(12) == 6 && border_trail(12) == 5 && border_lead(1) == 0 && border_trail(1) == 0, "lead / trail");
    return g_failures;
}

// the extension of `planes` planes of H x W data ([q][w][h]) by this program's reference: eh x ew per plane
std::vector<float> ref_extension(const std::vector<float>& img, int H, int W, int planes, int mkh, int mkw, int mode, float value) {
    const int eh = H + mkh - 1, ew = W + mkw - 1, lh = mkh / 2, lw = mkw / 2;
    std::vector<float> e((size_t)planes * eh * ew);
    for (int q = 0; q < planes; q++)
        for (int c = 0; c < ew; c++)
            for (int r = 0; r < eh; r++) {
                const int sr = ref_source(mode, H, r - lh), sc = ref_source(mode, W, c - lw);
                e[((size_t)q * ew + c) * eh + r] = (sr < 0 || sc < 0) ? value : img[((size_t)q * W + sc) * H + sr];
            }
    return e;
}

struct FwdSetup {
    Geometry g;
    Tables t;
    DeviceTables d;
    bool ok = false;
};

// (static: the tables the DeviceTables point into must outlive the call)
bool make_setup(FwdSetup& s, int H, int W, int F, int mkh, int mkw, int* queue) {
    PlanTuning tune;
    tune.path_mode = 2;
    if (!make_geometry(s.g, s.t, H, W, F, mkh, mkw, tune) || !s.g.fast_fwd || s.g.M != C16::M || s.g.fast_cols.T != C16::T) return false;
    s.d.fc_tw1 = s.t.fcl.tw1.data(); s.d.fc_tw2 = s.t.fcl.tw2.data(); s.d.fc_pairs = s.t.fcl.pairs.data();
    s.d.queue = queue;
    s.d.queue_fwd = queue != nullptr;
    s.ok = true;
    return true;
}

void run_body(const char* what, int H, int W, int mkh, int mkw, int mode, float value, int planes, bool dyn) {
    static int queue[FC_QUEUE_WORDS];
    FwdSetup s;      // (the tables of the 288-point transform; the launch below has its own counts)
    if (!make_setup(s, 258, 258, 1, 31, 31, dyn ? queue : nullptr) || H + mkh - 1 > 2 * C16::M) {
        g_failures++;
        printf("FAIL %s: the plan does not run the configuration this case names\n", what);
        return;
    }
    const Geometry& g = s.g;
    const int eh = H + mkh - 1, ew = W + mkw - 1;
    uint32_t seed = 4242u + (uint32_t)(H * 31 + W * 7 + mkh * 3 + mode);
    std::vector<float> img((size_t)planes * H * W);      // (ends with the last sample: a load past it is a fault under a sanitizer build)
    for (float& v : img) { seed = seed * 1664525u + 1013904223u; v = (float)(int)((seed >> 8) & 0xffffu) / 4096.f - 8.f; }
    const std::vector<float> ext = ref_extension(img, H, W, planes, mkh, mkw, mode, value);
    const int out_pitch = round_up(ew, 8);
    const size_t out_plane = (size_t)(C16::M + 1) * out_pitch;
    std::vector<c32> sa(out_plane * planes), sb(out_plane * planes);
    const uint32_t fill = 0xffc0dead;
    for (auto* v : {&sa, &sb})
        for (c32& z : *v) { memcpy(&z.x, &fill, 4); memcpy(&z.y, &fill, 4); }
    std::vector<c32> lds(C16::LDS_ELEMS);
    const int nwg = 3;
    const BorderLoad bd = border_load(mode, value, H, W, mkh, mkw);
    const FastColsFwdArgs fa = fast_cols_fwd_args(g, s.d, img.data(), (size_t)H * W, H, eh, ew, planes, sa.data(), out_plane, out_pitch, false);
    const FastColsFwdArgs fb = fast_cols_fwd_args(g, s.d, ext.data(), (size_t)eh * ew, eh, eh, ew, planes, sb.data(), out_plane, out_pitch, false);
    for (int wg = 0; wg < nwg; wg++) {
        for (int i = 0; i < C16::LDS_ELEMS; i++) lds[i] = mk(1e30f, -1e30f);
        HostPhaseCtx<ColFwdState> ctx(C16::NT);
        fast_cols_fwd_body<C16, C16::R2, float, Bordered>(ctx, lds.data(), fa, wg, nwg, PixelLoad{}, bd);
    }
    for (int wg = 0; wg < nwg; wg++) {
        for (int i = 0; i < C16::LDS_ELEMS; i++) lds[i] = mk(1e30f, -1e30f);
        HostPhaseCtx<ColFwdState> ctx(C16::NT);
        fast_cols_fwd_body<C16, C16::R2>(ctx, lds.data(), fb, wg, nwg);
    }
    size_t written = 0;
    for (const c32& z : sa) written += fc_float_bits(z.x) != fill;
    const bool same = memcmp(sa.data(), sb.data(), sa.size() * sizeof(c32)) == 0;
    const size_t expect = (size_t)(C16::M + 1) * ew * planes;
    if (!same || written != expect || (dyn && queue[8 * FC_QUEUE_STRIDE] != 0)) {
        g_failures++;
        printf("FAIL %s mode %d: spectra %s, %zu written, %zu expected\n", what, mode, same ? "equal" : "DIFFER", written, expect);
    } else {
        printf("ok   %s mode %d: %zu spectrum values bit-equal\n", what, mode, written);
    }
}

int cmd_bodies() {
    for (int mode = 1; mode <= 5; mode++) {
        const float value = mode == 1 ? -1.25f : 0.f;
        run_body("H even, MAXK odd", 258, 250, 31, 31, mode, value, 3, false);
        run_body("H odd, MAXK odd", 251, 243, 13, 11, mode, value, 3, false);
        run_body("H even, MAXK even", 250, 251, 12, 10, mode, value, 3, false);
        run_body("H odd, MAXK even", 251, 249, 12, 10, mode, value, 3, false);
        run_body("H odd, MAXK even, dynamic tile queue", 251, 249, 12, 10, mode, value, 2, true);
        run_body("small data, deep border", 16, 20, 31, 29, mode, value, 2, false);
    }
    if (!g_failures) printf("all bit-equal\n");
    return g_failures;
}

int cmd_spectrum(int argc, char** argv) {
    const int H = atoi(argv[4]), W = atoi(argv[5]), F = atoi(argv[6]), mkh = atoi(argv[7]), mkw = atoi(argv[8]), mode = atoi(argv[9]);
    const float value = (float)atof(argv[10]);
    FwdSetup s;
    if (!make_setup(s, H, W, F, mkh, mkw, nullptr) || !s.g.fast_rows.ok || s.g.Lw != 288) { printf("FAIL no such plan\n"); return 1; }
    if (const char* why = border_args_error(mode, value, H, W, mkh, mkw)) { printf("FAIL %s\n", why); return 1; }
    const Geometry& g = s.g;
    std::vector<float> img((size_t)H * W * F);
    FILE* f = fopen(argv[2], "rb");
    if (!f || fread(img.data(), sizeof(float), img.size(), f) != img.size()) { printf("FAIL cannot read %s\n", argv[2]); return 1; }
    fclose(f);
    std::vector<c32> S(g.spectrum_elems(), mk(1e30f, -1e30f));      // (garbage-fill: reads of never-written cells show)
    std::vector<c32> lds(FC_LDS_BUDGET / sizeof(c32));
    const int eh = H + mkh - 1, ew = W + mkw - 1;
    const BorderLoad bd = border_load(mode, value, H, W, mkh, mkw);
    const FastColsFwdArgs fa = image_fwd_args(g, s.d, img.data(), H, W, eh, ew, F, S.data());
    for (int wg = 0; wg < 3; wg++) {
        for (int i = 0; i < C16::LDS_ELEMS; i++) lds[i] = mk(1e30f, -1e30f);
        HostPhaseCtx<ColFwdState> ctx(C16::NT);
        fast_cols_fwd_body<C16, C16::R2, float, Bordered>(ctx, lds.data(), fa, wg, 3, PixelLoad{}, bd);
    }
    s.d.fr_tw1 = s.t.fr.tw1.data();
    s.d.fr_tw2 = s.t.fr.tw2.data();
    const FastRowsFwdArgs ra = fast_rows_fwd_args(g, s.d, S.data(), mkw - 1);
    emu::EmuFastRowsFwd rows{ra, lds.data(), F * g.rows};
    rows.go<R288>();
    f = fopen(argv[3], "wb");
    if (!f || fwrite(S.data(), sizeof(c32), S.size(), f) != S.size()) { printf("FAIL cannot write %s\n", argv[3]); return 1; }
    fclose(f);
    printf("ok   spectrum: %zu elements, transform %d x %d, window %d x %d\n", S.size(), g.Lh, g.Lw, g.fft_h, g.fft_w);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "index") return cmd_index() ? 1 : 0;
    if (mode == "errors") return cmd_errors();
    if (mode == "routes") return cmd_routes() ? 1 : 0;
    if (mode == "bodies") return cmd_bodies() ? 1 : 0;
    if (mode == "spectrum" && argc == 11) return cmd_spectrum(argc, argv);
    fprintf(stderr, "usage: border_host index | errors | routes | bodies | spectrum IN OUT H W F MKH MKW MODE VALUE\n");
    return 2;
}
