// pipeline.hpp -- geometry of one plan and the argument blocks of its kernels.
// Host-only, shared by the product library (fftconv_api.cpp, plan_image.cpp) and the test-only emulator so
// that both drive the workgroup bodies with identical arguments.
#pragma once
#include <algorithm>
#include <cstddef>

#include "fast_paths.hpp"
#include "kernels_body.hpp"
#include "planner.hpp"

namespace fc {

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Choices fixed at plan creation (include/fftconv.h: fftconv_plan_options).  The product reads no
// environment variables; tests and A/B runs pass these through fftconv_plan_create_ex.
struct PlanTuning {
    // 0 generic kernels only; 1 specialised kernels with a row-major intermediate; 2 (default)
    // specialised kernels with the tiled, pair-adjacent intermediate
    int path_mode = 2;
    // maps per workgroup of the multi-map row kernel (fast_rows_multi.hpp): -1 = chosen per
    // launch (rows_group_for), 0 / 1 = one map per workgroup (the same kernel, a walk of one), > 1 = fixed
    int rows_group = -1;
    // largest transform length a plan may use (0 = whatever fits the LDS); larger problems are left
    // to the block-wise path of the one-shot entry
    int max_transform = 0;
    // transform lengths must equal the ceil16 window (the reference's circular modulus; needed to
    // exchange spectra in the reference's order); a window that does not factor into the radices runs
    // Bluestein transforms on the generic kernels, one whose work length does not fit the LDS fails
    bool exact_window = false;
    // the block plan of an overlap-save block-wise plan (fftconv_api.cpp): H x W IS the transform (a block of the image with
    // its history rows / columns), the result is the circular convolution modulo H x W, and the caller stores the part of
    // it that is not wrapped.  Needs both specialised hot kernels and the tiled intermediate.
    bool cyclic = false;
};

struct Geometry {
    // problem (src/cudaConvolutionFFT.cu:92-112)
    int H = 0, W = 0, F = 0;
    int max_kh = 0, max_kw = 0;
    int fft_h = 0, fft_w = 0;  // output window: computeFFTsize16(DATA + MAXK - 1)
    // internal transform
    int Lh = 0, Lw = 0;        // transform lengths (Lh even)
    int M = 0;                 // Lh / 2
    int rows = 0;              // M + 1 spectrum rows
    int s_pitch = 0;           // c32 per image-spectrum row
    int y_pitch = 0;           // c32 per intermediate row
    int wout = 0;              // columns of Y consumed by the output pass: min(Lw, fft_w)
    int work_m = 0, work_w = 0; // complex lengths the h / w transforms run on: M / Lw, or their Bluestein work lengths
    bool acc_in_y = false;     // generic spectral rows, F > 1: the feature sum accumulates in Y (SpectralRowsArgs::acc_in_y)
    int lds_pitch = 0;         // c32 per LDS-resident column
    int T_cols = 1;            // columns per workgroup in the h-passes
    bool exact_window = false; // Lh == fft_h && Lw == fft_w: circular modulus equals the reference's
    FastRowsInfo fast_rows;    // specialised spectral-row kernel, if one exists for (Lw, max_kw)
    FastColsInfo fast_cols;    // specialised output kernel, if one exists for M
    bool fast_fwd = false;     // forward column transforms (image, kernels) by fast_cols_fwd.hpp: the
                               // spectrum rows are then in the fast plan's order, not the generic plan's
    int path_mode = 2;         // PlanTuning::path_mode
    // tiled intermediate [w / 16][row][16] (one 128-byte line per row and tile), rows of bins
    // (k, M-k) adjacent so that the output kernel merges them while landing: both hot kernels
    // specialised and the window a whole number of layout tiles
    static constexpr int y_tile_w = FC_Y_TILE_W;
    static constexpr int y_tile_shift = FC_Y_TILE_SHIFT;
    bool y_tiled() const { return path_mode == 2 && fast_rows.ok && fast_cols.ok && y_tile_w % fast_cols.T == 0 && fft_w % y_tile_w == 0; }
    int tile_rows() const { return y_tiled() ? M + 2 : rows; }
    int rows_group = -1;       // PlanTuning::rows_group
    bool rows_multi_ok() const { return rows_group != 0 && rows_group != 1 && fast_rows.ok; }
    // As many maps per workgroup as leaves >= 4 workgroups per resident slot (4 per CU), at most 16:
    // the walk amortises the image-spectrum row, the launch and the store drain, but a grid
    // that no longer fills the chip loses more than that.
    int rows_group_for(int nmaps, int num_cus) const {
        if (!rows_multi_ok()) return 1;
        if (rows_group > 1) return std::min(rows_group, nmaps);
        const int g1 = rows_group_auto(nmaps, num_cus);
        if (F == 1) return g1;
        // F > 1: the F image-spectrum rows of a workgroup are re-read for every map from the XCD's L2, and they
        // stay there only while few row groups are in flight per XCD, i.e. while many workgroups share a row
        // group: short walks (measured optimum 4-6 maps at F <= 8, 2 at F = 32; tools/f_group.py,
        // profiles/r02x_f_walk_length.txt: 16-map walks fetch 205 MB per map at F = 8, 4-map walks 62)
        // (round 3, spill-free kernel: 3 / 4 / 6 / 8 / 12 maps at F = 4: 56.2 / 55.1 / 56.9 / 56.7 / 60.0 us per map)
        return std::min(g1, std::max(2, std::min(4, 32 / F)));
    }
    int rows_slots_per_cu = 4; // resident workgroups of the multi-map row kernel per CU (the plan asks the runtime: light
                               // configurations hold 5-6, the 4224-point one 4)
    // Maps per workgroup of the multi-map row kernel for a launch of nmaps.  Large launches (eight or more rounds of
    // one-map workgroups): as many as leaves >= 4 rounds, at most 16 -- the walk amortises the image-spectrum row, the
    // launch and the store drain, but a grid that no longer fills the chip loses more than that.  Small launches: the
    // shortest walk whose FULL walks are all resident at once (the remainder walk of every row group, launched last,
    // fills the slots they leave and the first ones to free up) -- cfg2, 289 row groups x 16 maps on 1536 slots: walks of
    // 1 / 2 / 3 / 4 / 5 maps take 84.6 / 81.4 / 79.2 / 82.6 / 83.6 us per step; 3 = 1445 full walks + 289 single maps.
    int rows_group_auto(int nmaps, int num_cus) const { return walk_auto((rows + fast_rows.RPW - 1) / fast_rows.RPW, nmaps, num_cus); }
    // the rule itself: `units` workgroups would run per walked item (row groups; row groups x kernels for the image walk), `count` items
    // (maps of the launch; images of the launch) are dealt into walks
    int walk_auto(long units, int count, int num_cus) const {
        const long slots = (long)num_cus * std::max(1, rows_slots_per_cu), total = units * count;
        if (total >= 8 * slots) return (int)std::max<long>(1, std::min<long>(16, std::min<long>(total / (4 * slots), count)));
        if (total <= slots) return 1;        // everything resident at once
        for (int w = 2; w <= std::min(16, count); w++)
            if (units * (count / w) <= slots) return w;
        return std::min(16, count);
    }
    // Image walk (fast_rows_images.hpp): images per workgroup for a launch of `images` images x nk kernels -- the same rule over
    // the same slots with workgroups = groups * nk * walks: fill the chip first, at most 16; a fixed rows_group > 1 is the walk
    // (capped by the images of the launch), rows_group 0 / 1 walks of one image.
    int images_group_auto(int images, int nk, int num_cus) const {
        return walk_auto((long)((rows + fast_rows.RPW - 1) / fast_rows.RPW) * nk, images, num_cus);
    }
    int images_group_for(int images, int nk, int num_cus) const {
        if (!rows_multi_ok()) return 1;
        if (rows_group > 1) return std::min(rows_group, images);
        return images_group_auto(images, nk, num_cus);
    }
    size_t spectrum_elems() const { return (size_t)F * rows * s_pitch; }
    size_t y_elems_per_kernel() const {
        return y_tiled() ? (size_t)(fft_w / y_tile_w) * tile_rows() * y_tile_w : (size_t)rows * y_pitch;
    }
    size_t map_elems() const { return (size_t)fft_h * fft_w; }
    bool bluestein_h() const { return work_m != M; }
    bool bluestein_w() const { return work_w != Lw; }
    // dynamic LDS of the generic row kernels: the image's forward rows, the spectral rows (+ the accumulator)
    size_t rows_fwd_lds_bytes() const { return (size_t)work_w * sizeof(c32); }
    size_t rows_lds_bytes() const { return ((size_t)work_w + (F > 1 && !acc_in_y ? Lw : 0)) * sizeof(c32); }
};

struct Tables {
    Plan1D pm;  // M-point complex transform (h direction)
    Plan1D pw;  // Lw-point complex transform (w direction)
    std::vector<PairEntry> pairs;
    FastRowsTables fr;  // only if Geometry::fast_rows.ok
    FastColsTables fcl; // only if Geometry::fast_cols.ok
    // natural h-frequency y -> spectrum row, natural w-frequency x -> element of a stored image-spectrum row
    std::vector<int> nat_row_of, nat_col_of;
};

// returns false if the sizes are invalid / unsupported
inline bool make_geometry(Geometry& g, Tables& t, int H, int W, int F, int max_kh, int max_kw, const PlanTuning& tune = PlanTuning()) {
    const int path_mode = (tune.path_mode < 0 || tune.path_mode > 2) ? 2 : tune.path_mode;
    const bool allow_fast = path_mode > 0;
    g.path_mode = path_mode;
    g.rows_group = tune.rows_group;
    if (H < 1 || W < 1 || F < 1 || max_kh < 1 || max_kw < 1) return false;
    g.H = H; g.W = W; g.F = F; g.max_kh = max_kh; g.max_kw = max_kw;
    // (F > 1: the XCD-aware workgroup order -- the workgroups that read the same F image-spectrum rows side by side on one L2 --
    //  lives in the walk kernel itself: kernels_rows_multi.inc: k_fast_rows_multi_f)
    g.fft_h = tune.cyclic ? H : fft_size16(H + max_kh - 1);
    g.fft_w = tune.cyclic ? W : fft_size16(W + max_kw - 1);
    if (tune.cyclic && (!allow_fast || (H & 1) || max_kh > H || max_kw > W)) return false;
    LengthPrefs prefs;   // the planner prefers lengths with specialised kernels (able to take max_kw)
    if (allow_fast) { prefs.fast_rows = &fast_rows_factor; prefs.fast_cols = &fast_cols_factor; prefs.max_kw = max_kw; }
    // (max_transform caps the search: a cheaper length above it must not turn a size that fits into one that does not)
    g.Lh = choose_length(H + max_kh - 1, true, g.fft_h, prefs, tune.max_transform);
    g.Lw = choose_length(W + max_kw - 1, false, g.fft_w, prefs, tune.max_transform);
    if (tune.cyclic) {
        if (!length_supported(g.fft_h / 2) || !length_supported(g.fft_w)) return false;
        g.Lh = g.fft_h;
        g.Lw = g.fft_w;
    } else if (tune.exact_window) {   // windows that do not factor: Bluestein transforms (make_plan1d_bluestein)
        if (!length_transformable(g.fft_h / 2) || !length_transformable(g.fft_w)) return false;
        g.Lh = g.fft_h;
        g.Lw = g.fft_w;
    }
    if (g.Lh < 2 || g.Lw < 1) return false;
    if (tune.max_transform > 0 && (g.Lh > tune.max_transform || g.Lw > tune.max_transform)) return false;
    g.M = g.Lh / 2;
    g.rows = g.M + 1;
    g.s_pitch = round_up(g.Lw, 8);
    g.wout = std::min(g.Lw, g.fft_w);
    g.y_pitch = round_up(g.wout, 8);
    g.work_m = length_supported(g.M) ? g.M : bluestein_work_length(g.M);
    g.work_w = length_supported(g.Lw) ? g.Lw : bluestein_work_length(g.Lw);
    if (g.work_m < 1 || g.work_w < 1) return false;
    g.lds_pitch = lds_col_pitch(std::max(g.M, g.work_m - 1));   // (>= M + 1 and >= the work length)
    g.T_cols = 8;
    while (g.T_cols > 1 && (size_t)g.T_cols * g.lds_pitch * sizeof(c32) > FC_LDS_BUDGET) g.T_cols /= 2;
    if ((size_t)g.T_cols * g.lds_pitch * sizeof(c32) > FC_LDS_BUDGET) return false;
    // (a Bluestein row whose accumulator does not fit beside its work buffer sums the features in Y instead)
    g.acc_in_y = F > 1 && g.bluestein_w() && g.rows_lds_bytes() > FC_LDS_BUDGET;
    if (g.rows_lds_bytes() > FC_LDS_BUDGET) return false;
    g.exact_window = (g.Lh == g.fft_h && g.Lw == g.fft_w);
    t.pm = g.bluestein_h() ? make_plan1d_bluestein(g.M, g.work_m) : make_plan1d(g.M);
    t.pw = g.bluestein_w() ? make_plan1d_bluestein(g.Lw, g.work_w) : make_plan1d(g.Lw);
    t.pairs = make_pair_table(t.pm);
    g.fast_rows = allow_fast ? fast_rows_lookup(g.Lw, max_kw) : FastRowsInfo();
    if (g.fast_rows.ok) t.fr = make_fast_rows_tables(g.fast_rows, t.pw);
    // the fast output kernel crops (window <= transform) but does not zero-fill (window > transform)
    g.fast_cols = (allow_fast && g.Lh >= g.fft_h && g.Lw >= g.fft_w) ? fast_cols_lookup(g.M) : FastColsInfo();
    if (g.fast_cols.ok && (g.fft_w % g.fast_cols.T != 0)) g.fast_cols = FastColsInfo();
    g.fast_fwd = g.fast_cols.ok;
    // the plan whose digit-reversed order the spectrum rows are produced in
    Plan1D producer = g.fast_fwd ? make_plan1d_seq(g.M, {g.fast_cols.R1, g.fast_cols.R2, g.fast_cols.R3}) : t.pm;
    if (g.fast_cols.ok) t.fcl = make_fast_cols_tables(g.fast_cols, producer, g.y_pitch);
    if (tune.cyclic && !g.y_tiled()) return false;
    t.nat_row_of.assign(g.rows, g.M);                       // bin M (Nyquist) lives in the extra row M
    for (int k = 0; k < g.M; k++) t.nat_row_of[k] = producer.pos[k];
    t.nat_col_of.assign(g.Lw, 0);
    if (g.fast_rows.ok) {                                   // stored element x holds transform position relayout[x]
        std::vector<int> inv(g.Lw, 0);
        for (int x = 0; x < g.Lw; x++) inv[t.fr.relayout[x]] = x;
        for (int k = 0; k < g.Lw; k++) t.nat_col_of[k] = inv[t.pw.pos[k]];
    } else {
        for (int k = 0; k < g.Lw; k++) t.nat_col_of[k] = t.pw.pos[k];
    }
    return true;
}

// Device-resident copies of the tables (pointers valid on whichever side runs the bodies).
struct DeviceTables {
    const c32* tw_m = nullptr;
    const c32* tw_w = nullptr;
    const PairEntry* pairs = nullptr;
    const c32* fr_tw1 = nullptr;
    const c32* fr_tw2 = nullptr;
    const int* fr_relayout = nullptr;
    const c32* fc_tw1 = nullptr;
    const c32* fc_tw2 = nullptr;
    const PairEntry* fc_pairs = nullptr;
    const int* fc_rowoff = nullptr;
    const int* fc_pair_row_of = nullptr;
    int* queue = nullptr;                     // dynamic tile queue of the persistent column kernels (FC_QUEUE_WORDS ints; plan option "dynamic_tiles")
    bool queue_fwd = false;                   // ... also for the forward column kernels ("dynamic_tiles" = 2; off by default, see fast_cols_fwd_args)
    unsigned long long* timeline = nullptr;   // FC_ROWS_TIMELINE / FC_COLS_TIMELINE builds only (plan option "timeline_ptr")
};

// image columns: planes = F, columns = W, valid samples = H
// (h_ext x w_ext: the dense planes at `image` are the extended image of the staged border route instead; 0 = the data's H x W)
inline ColsR2CArgs image_cols_args(const Geometry& g, const Tables& t, const DeviceTables& d,
                                   const float* image, c32* S, int h_ext = 0, int w_ext = 0) {
    ColsR2CArgs a{};
    const int h = h_ext > 0 ? h_ext : g.H, w = w_ext > 0 ? w_ext : g.W;
    a.in = image; a.in_plane_stride = (size_t)h * w; a.in_col_pitch = h; a.h_in = h; a.ncols = w;
    a.out = S; a.out_plane_stride = (size_t)g.rows * g.s_pitch; a.out_pitch = g.s_pitch;
    a.M = g.M; a.T = g.T_cols; a.lds_pitch = g.lds_pitch;
    a.fd = t.pm.desc; a.tw = d.tw_m; a.pairs = d.pairs; a.npairs = (int)t.pairs.size();
    return a;
}

// (border_cols: the columns a border adds to the image -- MAX_KERNEL_W - 1 while fftconv_plan_set_border is on, else 0: the column
//  pass has written the spectra of W + border_cols columns)
inline RowsFwdArgs image_rows_args(const Geometry& g, const Tables& t, const DeviceTables& d, c32* S, int border_cols = 0) {
    RowsFwdArgs a{};
    a.S = S; a.pitch = g.s_pitch; a.nvalid = g.W + border_cols;
    a.scale = (float)(1.0 / ((double)g.Lh * (double)g.Lw));
    a.fd = t.pw.desc; a.tw = d.tw_w;
    a.out_map = g.fast_rows.ok ? d.fr_relayout : nullptr;   // store straight in the fast row kernel's order
    return a;
}

// the same pass by the specialised kernel (fast_rows_fwd.hpp), when the row length has one
inline FastRowsFwdArgs fast_rows_fwd_args(const Geometry& g, const DeviceTables& d, c32* S, int border_cols = 0) {
    FastRowsFwdArgs a{};
    a.S = S; a.pitch = g.s_pitch; a.nvalid = g.W + border_cols;
    a.scale = (float)(1.0 / ((double)g.Lh * (double)g.Lw));
    a.tw1 = d.fr_tw1; a.tw2 = d.fr_tw2;
    return a;
}

// kernel columns of a group of same-sized kernels, packed [n][f][kw][kh]: planes = nk*F
inline int a_pitch_for(int kw) { return round_up(kw, 8); }

inline ColsR2CArgs kernel_cols_args(const Geometry& g, const Tables& t, const DeviceTables& d,
                                    const float* kernels, int kh, int kw, c32* A) {
    ColsR2CArgs a{};
    a.in = kernels; a.in_plane_stride = (size_t)kh * kw; a.in_col_pitch = kh; a.h_in = kh; a.ncols = kw;
    a.out = A; a.out_plane_stride = (size_t)g.rows * a_pitch_for(kw); a.out_pitch = a_pitch_for(kw);
    a.M = g.M; a.T = g.T_cols; a.lds_pitch = g.lds_pitch;
    a.fd = t.pm.desc; a.tw = d.tw_m; a.pairs = d.pairs; a.npairs = (int)t.pairs.size();
    return a;
}

inline SpectralRowsArgs spectral_rows_args(const Geometry& g, const Tables& t, const DeviceTables& d,
                                           const c32* A, int kw, const c32* S, c32* Y) {
    SpectralRowsArgs a{};
    a.A = A; a.a_pitch = a_pitch_for(kw); a.a_feat_stride = (size_t)g.rows * a.a_pitch;
    a.a_kernel_stride = (size_t)g.F * a.a_feat_stride; a.kw = kw;
    a.S = S; a.s_feat_stride = (size_t)g.rows * g.s_pitch; a.s_pitch = g.s_pitch;
    a.Y = Y; a.y_kernel_stride = g.y_elems_per_kernel(); a.y_pitch = g.y_pitch; a.wout = g.wout;
    a.F = g.F; a.fd = t.pw.desc; a.tw = d.tw_w;
    a.acc_in_y = g.acc_in_y ? 1 : 0;
    return a;
}

// fast spectral rows (S in register order)
inline FastRowsArgs fast_rows_args(const Geometry& g, const DeviceTables& d, const c32* A, int kw, const c32* S, c32* Y) {
    FastRowsArgs a{};
    a.A = A; a.a_pitch = a_pitch_for(kw); a.a_feat_stride = (size_t)g.rows * a.a_pitch;
    a.a_kernel_stride = (size_t)g.F * a.a_feat_stride; a.kw = kw;
    a.S = S; a.s_feat_stride = (size_t)g.rows * g.s_pitch; a.s_pitch = g.s_pitch;
    a.Y = Y; a.y_kernel_stride = g.y_elems_per_kernel(); a.y_pitch = g.y_pitch; a.wout = g.wout;
    a.F = g.F; a.tw1 = d.fr_tw1; a.tw2 = d.fr_tw2;
    a.y_row_of = g.y_tiled() ? d.fc_pair_row_of : nullptr;
    a.y_tile_elems = g.tile_rows() * g.y_tile_w; a.y_tile_shift = g.y_tile_shift;
    a.timeline = d.timeline;
    return a;
}

// fast output columns: nk kernels of the current batch
// (out_format: FC_MAP_* of the maps at `out`; strides count elements whatever their size)
inline FastColsArgs fast_cols_args(const Geometry& g, const DeviceTables& d, const c32* Y, float* out,
                                   size_t out_kernel_stride, int nk, int out_format = FC_MAP_F32) {
    FastColsArgs a{};
    a.out_format = out_format;
    a.Y = Y; a.y_kernel_stride = g.y_elems_per_kernel(); a.y_pitch = g.y_pitch;
    a.out = out; a.out_kernel_stride = out_kernel_stride; a.fft_h = g.fft_h; a.fft_w = g.fft_w;
    a.h_lo = 0; a.w_first = 0; a.out_pitch = g.fft_h;
    a.tiles_per_kernel = g.fft_w / g.fast_cols.T; a.ntiles = a.tiles_per_kernel * nk;
    a.rowoff = d.fc_rowoff; a.tw1 = d.fc_tw1; a.tw2 = d.fc_tw2; a.pairs = d.fc_pairs;
    a.y_tiled = g.y_tiled() ? 1 : 0; a.y_tile_elems = g.tile_rows() * g.y_tile_w; a.y_tile_shift = g.y_tile_shift;
    a.timeline = d.timeline;
    a.queue = d.queue;          // counters 0..7 (one per XCD)
    return a;
}

// forward column pass of `planes` planes of `ncols` columns with h_in valid samples each; of_kernels: the kernels' pass
// (counter 9 of the dynamic tile queue; the image's pass has counter 8 -- the two may run at the same time, on two
// streams or in one launch)
inline FastColsFwdArgs fast_cols_fwd_args(const Geometry& g, const DeviceTables& d, const float* in, size_t in_plane_stride,
                                          int in_col_pitch, int h_in, int ncols, int planes, c32* out,
                                          size_t out_plane_stride, int out_pitch, bool of_kernels) {
    FastColsFwdArgs a{};
    a.in = in; a.in_plane_stride = in_plane_stride; a.in_col_pitch = in_col_pitch; a.h_in = h_in; a.ncols = ncols;
    a.out = out; a.out_plane_stride = out_plane_stride; a.out_pitch = out_pitch;
    a.tiles_per_plane = (ncols + g.fast_cols.T - 1) / g.fast_cols.T; a.ntiles = a.tiles_per_plane * planes;
    a.tw1 = d.fc_tw1; a.tw2 = d.fc_tw2; a.pairs = d.fc_pairs;
    // The forward kernels take their tiles from ONE counter each, and their tiles are short (a pruned kernel column pass is ~2 us a
    // tile): the 1 024 tickets of a 64-kernel pass queue up on that one cache line -- +12 us per pass at every size, +6-10 us per
    // image pass (profiles/r05k_dynamic_tiles_by_size.txt).  They are 1-3 % of a step and lose next to nothing to a neighbour
    // that holds CUs: static deal unless "dynamic_tiles" = 2 asks for the queue (A/B, tests).
    a.queue = (d.queue && d.queue_fwd) ? d.queue + (of_kernels ? 9 : 8) * FC_QUEUE_STRIDE : nullptr;
    return a;
}
// the two passes a plan launches, in the long form's terms.  The image's: `planes` dense planes of h_data x w_data samples at `in`,
// transformed as w_count columns of h_count samples -- the data's own counts, or the extension's where a border is mapped in the
// load (the data then as it lies) -- into the spectrum layout at S
inline FastColsFwdArgs image_fwd_args(const Geometry& g, const DeviceTables& d, const float* in, int h_data, int w_data, int h_count,
                                      int w_count, int planes, c32* S) {
    return fast_cols_fwd_args(g, d, in, (size_t)h_data * w_data, h_data, h_count, w_count, planes, S, (size_t)g.rows * g.s_pitch, g.s_pitch, false);
}
// ... and the kernels': `planes` packed kh x kw planes at dk into the column-spectrum layout at A
inline FastColsFwdArgs kernels_fwd_args(const Geometry& g, const DeviceTables& d, const float* dk, int kh, int kw, int planes, c32* A) {
    return fast_cols_fwd_args(g, d, dk, (size_t)kh * kw, kh, kh, kw, planes, A, (size_t)g.rows * a_pitch_for(kw), a_pitch_for(kw), true);
}

// Image batches: the image coordinate of a spectral-row launch (FastRowsArgs / SpectralRowsArgs) -- `images` spectra from a.S on,
// one per spectrum_elems, times the nk kernels of the launch
template <class Args>
inline void rows_args_set_images(Args& a, const Geometry& g, int images, int nk) {
    a.s_image_stride = g.spectrum_elems(); a.images = images; a.kernels_per_image = nk;
}

// Launch cutting of a convolve on a plan that holds B images: the maps are the (image, kernel) grid, image-major -- map
// b * image_stride + k is image b (x) kernel k of the group (image_stride: the kernels of the whole call, >= n).  One spectral-row /
// output launch covers a rectangle of that grid, images [b0, b0 + nb) x kernels [k0, k0 + nk), whose maps sit in the slots
// (b - b0) * nk + (k - k0) of the intermediate and must be consecutive in the output: one image x a kernel range, or several
// whole images x every kernel of the call -- the latter only where the column-spectrum chunk holds all of them.  The kernels'
// column spectra are produced per chunk of nbA kernels (`chunk_start`: this launch is the first of its chunk); a launch has at
// most nbY maps.  B = 1 gives the (first, ny) sequence of a one-image plan.
struct LaunchRect {
    int b0, nb, k0, nk;      // k0 counts from the start of the group
    int a0, na;              // the chunk of kernels [a0, a0 + na) whose column spectra the launch reads (k0 - a0: its offset in A)
    bool chunk_start;
    int first(int image_stride) const { return b0 * image_stride + k0; }
    int ny() const { return nb * nk; }
};
// The launches one after the other, without a list of them (the per-kernel loop of a convolve allocates nothing on the host
// either): chunks outermost, then images, then kernel ranges of the chunk -- a chunk's column spectra serve every image.
struct LaunchCutter {
    int B, n, image_stride, nbA, nbY;
    int a0 = 0, b = 0, y0 = 0;       // the next launch: chunk start, image, kernel offset within the chunk
    bool start = true;               // ... is the first of its chunk
    LaunchCutter(int B_, int n_, int image_stride_, int nbA_, int nbY_)
        : B(B_), n(n_), image_stride(image_stride_), nbA(std::max(1, nbA_)), nbY(std::max(1, nbY_)) {}
    bool next(LaunchRect& r) {
        if (B < 1 || n < 1 || a0 >= n) return false;
        const int na = std::min(nbA, n - a0);
        if (na == n && image_stride == n && nbY >= n) {      // whole images x all kernels of the call
            const int per = nbY / n;
            r = {b, std::min(per, B - b), 0, n, a0, na, start};
            b += per;
        } else {                                             // one image x a kernel range of the chunk
            const int step = std::min(nbY, na);
            r = {b, 1, a0 + y0, std::min(step, na - y0), a0, na, start};
            y0 += step;
            if (y0 >= na) { y0 = 0; b++; }
        }
        start = false;
        if (b >= B) { b = 0; y0 = 0; a0 += nbA; start = true; }
        return true;
    }
};
// the same as a list (the CPU tier checks it)
inline std::vector<LaunchRect> cut_launches(int B, int n, int image_stride, int nbA, int nbY) {
    std::vector<LaunchRect> r;
    LaunchCutter cut(B, n, image_stride, nbA, nbY);
    for (LaunchRect l; cut.next(l);) r.push_back(l);
    return r;
}

inline int fast_rows_nz2(const Geometry& g, int kw) { return (kw + g.fast_rows.R3 - 1) / g.fast_rows.R3; }

inline ColsC2RArgs cols_c2r_args(const Geometry& g, const Tables& t, const DeviceTables& d,
                                 const c32* Y, float* out, size_t out_kernel_stride, int out_format = FC_MAP_F32) {
    ColsC2RArgs a{};
    a.out_format = out_format;
    a.Y = Y; a.y_kernel_stride = g.y_elems_per_kernel(); a.y_pitch = g.y_pitch; a.wvalid = g.wout;
    a.out = out; a.out_kernel_stride = out_kernel_stride; a.fft_h = g.fft_h; a.fft_w = g.fft_w;
    a.M = g.M; a.T = g.T_cols; a.lds_pitch = g.lds_pitch;
    a.fd = t.pm.desc; a.tw = d.tw_m; a.pairs = d.pairs; a.npairs = (int)t.pairs.size();
    return a;
}

inline int tiles_for(int ncols, int T) { return (ncols + T - 1) / T; }

// Plan option "map_format" (fc_common.hpp: FC_MAP_*): why `value` cannot be set, or nullptr if it can.  Block-wise plans keep
// fp32 maps: overlap-save blocks store rectangles at element offsets computed for 4-byte elements, and overlap-add sums in the maps.
inline const char* map_format_error(long value, bool blockwise) {
    if (value < FC_MAP_F32 || value > FC_MAP_BF16) return "map_format is 0 (fp32), 1 (fp16) or 2 (bfloat16)";
    if (value != FC_MAP_F32 && blockwise)
        return "map_format: 16-bit maps are not available on a block-wise plan (its blocks are stored at fp32 element offsets, or summed, in "
               "the maps); use fp32 maps, or a one-pass plan (fftconv_plan_options.blockwise = 1)";
    return nullptr;
}

// fftconv_plan_set_output_rect: why rows [off_h, off_h + out_h) of columns [off_w, off_w + out_w) are not a rectangle of the
// fft_h x fft_w window, or nullptr if they are.  (Sums in 64 bits: the arguments are any ints.)
inline const char* output_rect_error(long off_h, long off_w, long out_h, long out_w, int fft_h, int fft_w) {
    if (out_h < 1 || out_w < 1) return "output rectangle: out_h and out_w must be at least 1";
    if (off_h < 0 || off_w < 0) return "output rectangle: off_h and off_w must not be negative";
    if (off_h + out_h > fft_h || off_w + out_w > fft_w) return "output rectangle: it must lie inside the window";
    return nullptr;
}

// fftconv_plan_set_output_stride and "output_region": why a plan cannot have the strides (stride_h, stride_w) and that region at once,
// or nullptr if it can.  Region 4 is the window PADDED to the next power of two, not a sampling of the window: it takes no stride
// other than (1, 1), whichever of the two is asked for last.
inline const char* output_stride_error(long stride_h, long stride_w, long region) {
    if (stride_h < 1 || stride_w < 1) return "output stride: stride_h and stride_w must be at least 1";
    if ((stride_h != 1 || stride_w != 1) && region == 4)
        return "output stride: output_region 4 (the pow2-padded window) is not a sampling of the window and takes no stride; "
               "set the stride back to (1, 1) or choose another region";
    return nullptr;
}

}  // namespace fc
